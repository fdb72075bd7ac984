"""The budget of pb_video_hot_kernel's PAIRS form - NV12 and P010 -, read from the compiler's listing of the product build like
the other ISA tests: four instantiations <SRC_KIND, S, 4:2:0, true>, no scratch, no float64, the tile entry in scalar registers, at most
128 VGPRs (four waves per SIMD) - and the listing's own figures per sample size, pinned."""

import re

import pytest

from tests import kernel_listing

# VGPRs and waves per SIMD of the listing, per bytes per sample (both source kinds alike; recorded in DESIGN 3.15)
PINNED = {1: (99, 4), 2: (94, 5)}  # (pb_nv12_hot_kernel, the kernel of its own before the merge: 97 and 94)


@pytest.fixture(scope="module")
def stats():
    return kernel_listing.stats()


def _nv12(stats):
    got = {}
    for k, v in stats.items():
        m = re.fullmatch(r"pb_video_hot_kernel<(\d+), (\d+), 2, true>", k)
        if m:
            got[(int(m.group(1)), int(m.group(2)))] = v
    return got


def test_four_instantiations(stats):
    got = _nv12(stats)
    assert len(got) == 4, sorted(got)
    assert {s for _, s in got} == {1, 2} and len({k for k, _ in got}) == 2  # {camera, panorama} x two sample sizes


def test_budget(stats):
    for key, r in _nv12(stats).items():
        assert r["scratch"] == 0 and r["f64"] == 0, (key, r)
        assert r["vgpr"] <= 128 and r["occupancy"] >= 4, (key, r)
        # the other tile kernels' level (0 for pb_hot_win_kernel, 6 for pb_px_hot_kernel: exec masks of the MASKED path); a quarter of
        # the entry pushed out of the scalar registers is 16 writes and 16 reads per use, a whole entry 1 300-1 500
        assert r["lane_traffic"] <= 8, (key, r)


def test_the_listing_is_pinned(stats):
    for (kind, S), r in _nv12(stats).items():
        assert (r["vgpr"], r["occupancy"]) == PINNED[S], (kind, S, r["vgpr"], r["occupancy"])
