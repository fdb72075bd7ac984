"""The rotation-track kernel for NV12 / P010 video frames in the compiler's listing of the product build (like test_isa_track.py; DESIGN
3.16).  A resource pin only: the eight instantiations that exist, no scratch and no AGPRs, and the waves per SIMD and vector registers of
the shipped listing - those of pb_track_kernel of the same source kind, whose float64 chain it runs.  The kernel is pb_track_video_kernel's
PAIRS form, <S, SRC_KIND, true>: the equi-angular source's two instantiations, <1, 8, true> and <2, 8, true>, are pinned here, beside the
plain cube's."""

import pytest

from tests import kernel_listing

KINDS = {0: "camera", 2: "panorama", 5: "cube", 8: "equi-angular cube"}  # pb_kind (include/photonbend_hip.h); a double fisheye is refused
SAMPLES = (1, 2)  # NV12; P010 / P016
# the shipped listing (DESIGN 3.16's table): PB_TRACK_WPE holds a panorama and a camera source to eight waves per SIMD (at most 64 VGPRs),
# the two cube mappings get the budget of four and take seven
WAVES = {0: 8, 2: 8, 5: 7, 8: 7}
VGPRS = {0: 63, 2: 63, 5: 63, 8: 63}
TRACK_KERNEL = {0: "pb_track_kernel<0>", 2: "pb_track_kernel<2>", 5: "pb_track_kernel<5>", 8: "pb_track_eac_kernel"}


@pytest.fixture(scope="module")
def stats():
    return kernel_listing.stats()


def test_the_eight_instantiations_exist_without_scratch_at_the_pinned_waves_and_registers(stats):
    got = {k: v for k, v in stats.items() if k.startswith("pb_track_video_kernel<") and k.endswith(", true>")}
    assert sorted(got) == sorted(f"pb_track_video_kernel<{S}, {kind}, true>" for kind in KINDS for S in SAMPLES), sorted(got)
    assert len([n for n in stats if n.startswith("pb_track_video_kernel<")]) == 16  # (these and tests/test_isa_planar.py's eight)
    for name, r in got.items():
        print(f"{name:40s} vgpr {r['vgpr']:3d} sgpr {r['sgpr']:3d} scratch {r['scratch']} waves {r['occupancy']} instructions {r['instr']}")
        kind = int(name[len("pb_track_video_kernel<"):-1].split(",")[1])
        assert r["scratch"] == 0 and r["agpr"] == 0, (name, r)  # no frame-loop kernel of this library spills: a condition
        assert r["occupancy"] >= WAVES[kind] and r["vgpr"] <= VGPRS[kind], (name, r)


def test_a_video_frame_costs_no_waves_against_the_rgb8_track_kernel_of_the_same_source(stats):
    """The same chain, the same two float64 and a flag per pixel across the frame loop; the planes' layouts and fills must not cost a wave."""
    for kind in KINDS:
        ref = stats[TRACK_KERNEL[kind]]
        for S in SAMPLES:
            r = stats[f"pb_track_video_kernel<{S}, {kind}, true>"]
            assert r["occupancy"] >= ref["occupancy"], (kind, S, r, ref)
            assert r["f64"] <= ref["f64"], (kind, S, r["f64"], ref["f64"])  # chroma costs no float64
