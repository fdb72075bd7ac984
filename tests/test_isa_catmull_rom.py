"""The Catmull-Rom tile kernel's budget, read from the compiler's listing of the product build (like test_isa_supersample.py): no scratch,
no float64, and no tile entry dragged through VGPR lanes (DESIGN 3.4 "A finding worth its own line")."""

import pytest

from tests import kernel_listing


@pytest.fixture(scope="module")
def stats():
    return kernel_listing.stats()


def test_tile_kernel_budget(stats):
    got = {k: v for k, v in stats.items() if k.startswith("pb_catmull_rom_hot_kernel")}
    assert len(got) == 2, sorted(got)  # {camera, panorama}
    for name, r in got.items():
        assert r["scratch"] == 0 and r["f64"] == 0, (name, r)
        assert r["vgpr"] <= 168 and r["occupancy"] >= 3, (name, r)
        assert r["lane_traffic"] <= 8, (name, r)


def test_float64_kernels_are_there(stats):
    # the shared sampler templates (pb_kernels_bilinear.hpp), pinned from both filters' side
    for flt in ("PbCatmullRom", "PbBilinear"):
        for prefix, n in ((f"pb_interp_fix_kernel<{flt},", 2), (f"pb_interp_double_kernel<{flt}>", 1), (f"pb_sample_map_interp_kernel<{flt},", 6)):
            got = [k for k in stats if k.startswith(prefix)]
            assert len(got) == n, (prefix, sorted(got))
