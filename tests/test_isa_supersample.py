"""The supersampled kernels' budgets, read from the compiler's listing of the product build (like test_isa_budget.py).  The fused kernel runs
pb_hot_win_kernel's tile code and adds the n x n reduction: it must stay inside the same register budget - 64 VGPRs, seven waves per SIMD -
or it loses the latency hiding the windowed tiles live on."""

import pytest

from tests import kernel_listing


@pytest.fixture(scope="module")
def stats():
    return kernel_listing.stats()


def _pick(stats, prefix):
    got = {k: v for k, v in stats.items() if k.startswith(prefix)}
    assert got, prefix
    return got


def test_fused_kernel_budget(stats):
    got = _pick(stats, "pb_ss_win_kernel")
    assert len(got) == 4, sorted(got)  # {camera, panorama} x {2, 4}
    for name, r in got.items():
        assert r["scratch"] == 0 and r["f64"] == 0, (name, r)
        assert r["vgpr"] <= 64 and r["occupancy"] >= 7, (name, r)
        assert r["lane_traffic"] <= 8, (name, r)  # the fix-pixel hand-round (v_readlane), not a spilled tile entry


def test_box_reduce_budget(stats):
    got = _pick(stats, "pb_box_reduce_kernel")
    assert len(got) == 4, sorted(got)
    for name, r in got.items():
        assert r["scratch"] == 0 and r["f64"] == 0, (name, r)
