"""The budget of pb_px_hot_kernel, read from the compiler's listing of the product build like the other ISA tests: ten
instantiations, no scratch, no float64, the tile entry in scalar registers, at least four waves per SIMD - and the listing's own figures
per pixel size, pinned."""

import re

import pytest

from tests import kernel_listing

# VGPRs and waves per SIMD of the listing, per bytes per pixel (both source kinds alike; recorded in DESIGN 3.11)
PINNED = {1: (64, 7), 2: (64, 7), 4: (64, 7), 6: (80, 6), 8: (89, 5)}


@pytest.fixture(scope="module")
def stats():
    return kernel_listing.stats()


def _px(stats):
    got = {}
    for k, v in stats.items():
        m = re.fullmatch(r"pb_px_hot_kernel<(\d+), (\d+)>", k)
        if m:
            got[(int(m.group(1)), int(m.group(2)))] = v
    return got


def test_ten_instantiations(stats):
    got = _px(stats)
    assert len(got) == 10, sorted(got)
    assert {b for _, b in got} == {1, 2, 4, 6, 8} and len({k for k, _ in got}) == 2  # {camera, panorama} x five pixel sizes
    assert not [k for k in stats if k.startswith("pb_hot_win_kernel") and "px" in k]  # (the 64-VGPR budget's prefix is not ours)


def test_budget(stats):
    hot = [v for k, v in stats.items() if k.startswith("pb_hot_win_kernel")]
    assert hot
    for key, r in _px(stats).items():
        assert r["scratch"] == 0 and r["f64"] == 0, (key, r)
        assert r["vgpr"] <= 128 and r["occupancy"] >= 4, (key, r)
        # the other tile kernels' level (0 for pb_hot_win_kernel, <= 8 for the Catmull-Rom kernel); a spilled entry is 1 300-1 500
        assert r["lane_traffic"] <= 8, (key, r)


def test_the_listing_is_pinned(stats):
    for (kind, B), r in _px(stats).items():
        assert (r["vgpr"], r["occupancy"]) == PINNED[B], (kind, B, r["vgpr"], r["occupancy"])
