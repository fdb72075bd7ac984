"""The rotation-track kernel for double-fisheye video frames in the compiler's listing of the product build (like test_isa_track_nv12.py;
DESIGN 3.21).  A resource pin only: exactly the four instantiations of pb_track_stitch_kernel <S, PAIRS> and nothing else under the name,
no scratch and no AGPRs, and the waves per SIMD and vector registers of the shipped listing - those of pb_track_kernel of a double-fisheye
source, whose float64 chain and taps it runs."""

import re

import pytest

from tests import kernel_listing

INSTANTIATIONS = [(1, False), (1, True), (2, False), (2, True)]  # (bytes per sample, interleaved pairs): yuv*p, NV12, yuv*p10/16, P010 / P016
BUDGET = 4  # PB_TRACK_WPE of a double-fisheye source (csrc/pb_kernels_track.hpp)
WAVES, VGPRS = 7, 63  # the shipped listing (DESIGN 3.21's table): under the budget of four the compiler takes seven, as for pb_track_kernel<1>
RGB8 = "pb_track_kernel<1>"  # pb_kind 1: the double fisheye


@pytest.fixture(scope="module")
def stats():
    return kernel_listing.stats()


def _kernels(stats):
    got = {}
    for k, v in stats.items():
        m = re.fullmatch(r"pb_track_stitch_kernel<(\d+), (true|false)>", k)
        if m:
            got[(int(m.group(1)), m.group(2) == "true")] = v
    return got


def test_four_instantiations_and_nothing_else_under_the_name(stats):
    assert sorted(_kernels(stats)) == sorted(INSTANTIATIONS), sorted(_kernels(stats))
    assert len([n for n in stats if n.startswith("pb_track_stitch")]) == 4


def test_no_scratch_and_the_pinned_waves_and_registers(stats):
    for key, r in _kernels(stats).items():
        print(f"pb_track_stitch_kernel{key}: vgpr {r['vgpr']} sgpr {r['sgpr']} scratch {r['scratch']} waves {r['occupancy']} f64 {r['f64']} instructions {r['instr']}")
        assert r["scratch"] == 0 and r["agpr"] == 0, (key, r)  # no frame-loop kernel of this library spills: a condition
        assert r["occupancy"] >= BUDGET, (key, r)
        assert r["occupancy"] >= WAVES and r["vgpr"] <= VGPRS, (key, r)


def test_a_video_frame_costs_no_waves_against_the_rgb8_track_kernel_of_a_double_fisheye(stats):
    """The same chain and taps, the same two float64 and a flag per pixel across the frame loop; the planes' layouts, the second eye's loads
    and the chroma blends must not cost a wave."""
    ref = stats[RGB8]
    assert ref["occupancy"] == WAVES, ref
    for key, r in _kernels(stats).items():
        assert r["occupancy"] >= ref["occupancy"] and r["scratch"] == ref["scratch"] == 0, (key, r, ref)
