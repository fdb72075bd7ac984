"""The rotation-track kernels in the compiler's listing of the product build (like test_isa_budget.py).  A resource pin only:
the instantiations that exist, no scratch, and the waves per SIMD the kernels were measured at.  What stays live across the frame loop is
two float64 and a flag per pixel; a build that hoists the transcendental kernels' constants out of that loop shows here as lost waves."""

import pytest

from tests import kernel_listing

KINDS = {0: "camera", 1: "double fisheye", 2: "panorama", 5: "cube"}  # pb_kind (include/photonbend_hip.h)
# PB_TRACK_WPE (csrc/pb_kernels_track.hpp): a panorama and a camera source are held to eight waves per SIMD (at most 64 VGPRs and 96 scalar
# registers), a cube and a double-fisheye source take seven (held to eight they would spill)
NEAREST_WAVES = {0: 8, 1: 7, 2: 8, 5: 7}
INTERP_WAVES = {"PbBilinear": 8, "PbCatmullRom": 6}  # one pixel per work-item; the cubic's sixteen float64 taps and weights take more


@pytest.fixture(scope="module")
def stats():
    return kernel_listing.stats()


def test_the_nearest_track_kernel_exists_per_source_kind_without_scratch_at_its_waves(stats):
    got = {k: v for k, v in stats.items() if k.startswith("pb_track_kernel<")}
    assert sorted(got) == sorted(f"pb_track_kernel<{kind}>" for kind in KINDS), sorted(got)
    for name, r in got.items():
        print(f"{name:48s} vgpr {r['vgpr']:3d} sgpr {r['sgpr']:3d} scratch {r['scratch']} waves {r['occupancy']} instructions {r['instr']}")
        assert r["scratch"] == 0 and r["agpr"] == 0, (name, r)
        waves = NEAREST_WAVES[int(name[len("pb_track_kernel<"):-1])]
        assert r["occupancy"] >= waves and r["vgpr"] <= (64 if waves == 8 else 72), (name, r)


def test_the_interpolating_track_kernels_exist_per_source_kind_and_filter_without_scratch(stats):
    got = {k: v for k, v in stats.items() if k.startswith("pb_track_interp_kernel<")}
    assert sorted(got) == sorted(f"pb_track_interp_kernel<{kind}, {flt}>" for kind in KINDS for flt in INTERP_WAVES), sorted(got)
    for name, r in got.items():
        print(f"{name:48s} vgpr {r['vgpr']:3d} sgpr {r['sgpr']:3d} scratch {r['scratch']} waves {r['occupancy']} instructions {r['instr']}")
        flt = name.split(", ")[1].rstrip(">")
        assert r["scratch"] == 0 and r["agpr"] == 0, (name, r)
        assert r["occupancy"] >= INTERP_WAVES[flt], (name, r)


def test_a_track_frame_costs_no_more_registers_than_the_float64_kernel_of_the_same_chain(stats):
    """pb_remap_kernel<kind, any rotation count> is what a caller launched per frame before: the track kernel holds the same chain plus
    the map entries of its four pixels, and must not fall below that kernel's waves."""
    for kind in KINDS:
        ref, r = stats[f"pb_remap_kernel<{kind}, -1>"], stats[f"pb_track_kernel<{kind}>"]
        assert r["occupancy"] >= ref["occupancy"], (kind, r, ref)
