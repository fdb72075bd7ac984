"""The rotation-track kernels of grey, RGBA and 16-bit frames in the compiler's listing of the product build (like test_isa_track.py;
DESIGN 3.22).  A resource pin only: the instantiations that exist, no scratch, no AGPRs, and the waves per SIMD this build's listing shows.
The pixel size is a run-time argument of the nearest kernels: one per source kind, not one per size.  What stays live across their frame
loop is two float64 and a flag per pixel, and across a frame's four chains one source index per pixel - a pixel's two dwords held there
instead show here as scratch in the panorama and camera kernels."""

import pytest

from tests import kernel_listing

KINDS = {0: "camera", 1: "double fisheye", 2: "panorama", 5: "cube"}  # pb_kind (include/photonbend_hip.h)
SINGLE = [k for k in KINDS if k != 1]
# PB_TRACK_PX_WPE (csrc/pb_kernels_track_px.hpp): a panorama and a camera source are held to eight waves per SIMD (63 VGPRs, 78 scalar
# registers), a cube and a double-fisheye source take seven under the budget of four (61-67 VGPRs, 106 scalar registers)
NEAREST_WAVES = {0: 8, 1: 7, 2: 8, 5: 7}
EAC_WAVES = 7
# one pixel per work-item; the cubic's sixteen float64 taps and weights take more, two eyes' more again
INTERP_WAVES = {("PbBilinear", 0): 8, ("PbBilinear", 2): 8, ("PbBilinear", 5): 8, ("PbBilinear", 1): 7,
                ("PbCatmullRom", 0): 5, ("PbCatmullRom", 2): 6, ("PbCatmullRom", 5): 5, ("PbCatmullRom", 1): 3}
INTERP_EAC_WAVES = {"PbBilinear": 8, "PbCatmullRom": 5}
SAMPLES = ("unsigned char", "unsigned short")


@pytest.fixture(scope="module")
def stats():
    return kernel_listing.stats()


def show(name, r):
    print(f"{name:64s} vgpr {r['vgpr']:3d} sgpr {r['sgpr']:3d} scratch {r['scratch']} waves {r['occupancy']} instructions {r['instr']}")


def test_the_nearest_kernel_exists_once_per_source_kind_without_scratch_at_its_waves(stats):
    got = {k: v for k, v in stats.items() if k.startswith("pb_track_px_kernel")}
    assert sorted(got) == sorted(f"pb_track_px_kernel<{kind}>" for kind in KINDS), sorted(got)
    got["pb_track_px_equiangular_kernel"] = stats["pb_track_px_equiangular_kernel"]
    assert [k for k in stats if k.startswith("pb_track_px_equiangular_kernel")] == ["pb_track_px_equiangular_kernel"]
    for name, r in got.items():
        show(name, r)
        assert r["scratch"] == 0 and r["agpr"] == 0, (name, r)
        waves = EAC_WAVES if name == "pb_track_px_equiangular_kernel" else NEAREST_WAVES[int(name[len("pb_track_px_kernel<"):-1])]
        assert r["occupancy"] >= waves and r["vgpr"] <= (64 if waves == 8 else 72), (name, r)


def test_the_interpolating_kernels_exist_per_source_kind_filter_and_sample_type_without_scratch(stats):
    """a double fisheye blends to uint8: instantiated for uint8 samples alone"""
    got = {k: v for k, v in stats.items() if k.startswith("pb_track_px_interp_kernel<")}
    want = {f"pb_track_px_interp_kernel<{kind}, {flt}, {smp}>": INTERP_WAVES[flt, kind]
            for flt in ("PbBilinear", "PbCatmullRom") for kind in KINDS for smp in (SAMPLES[:1] if kind == 1 else SAMPLES)}
    assert sorted(got) == sorted(want), sorted(got)
    eac = {k: v for k, v in stats.items() if k.startswith("pb_track_px_interp_equiangular_kernel")}
    want_eac = {f"pb_track_px_interp_equiangular_kernel<{flt}, {smp}>": INTERP_EAC_WAVES[flt] for flt in INTERP_EAC_WAVES for smp in SAMPLES}
    assert sorted(eac) == sorted(want_eac), sorted(eac)
    for name, r in {**got, **eac}.items():
        show(name, r)
        assert r["scratch"] == 0 and r["agpr"] == 0, (name, r)
        assert r["occupancy"] >= {**want, **want_eac}[name], (name, r)


def test_nothing_else_carries_the_new_names(stats):
    names = [k for k in stats if "track_px" in k]
    assert len(names) == 5 + 14 + 4, sorted(names)


def test_a_track_frame_costs_no_more_waves_than_the_float64_kernel_of_the_same_chain(stats):
    """pb_remap_kernel<kind, any rotation count> runs the same chain for one frame: the track kernel holds that chain plus the map
    entries of its four pixels, and must not fall below that kernel's waves."""
    for kind in KINDS:
        ref, r = stats[f"pb_remap_kernel<{kind}, -1>"], stats[f"pb_track_px_kernel<{kind}>"]
        assert r["occupancy"] >= ref["occupancy"], (kind, r, ref)
    assert stats["pb_track_px_equiangular_kernel"]["occupancy"] >= stats["pb_remap_kernel<8, -1>"]["occupancy"]
