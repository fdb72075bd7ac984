"""The budget of the double-fisheye video kernel, read from the compiler's listing of the product build like the other ISA
tests: eight instantiations of pb_stitch_video_kernel <S, SUB, PAIRS> and nothing else under the name, no scratch, waves per SIMD not
below pb_hot_double_kernel's single-frame instantiations in the same listing, and the listing's own figures, pinned.  Register
statistics only."""

import re

import pytest

from tests import kernel_listing

# (bytes per sample, subsampling, pairs) -> (VGPRs, SGPRs, v_readlane / v_writelane instructions) of the listing; recorded in DESIGN 3.20.
# The lane traffic is the kernel's own: the two lane-held tile entries of a two-eye tile are read with one v_readlane per field and
# coefficient (pb_desc_of_lanes, pb_coefs_of_lanes: 2 x 50 coefficients, 2 x 3 fields, the flags, the slots and the fix lists).
PINNED = {(1, 0, False): (128, 97, 112), (1, 1, False): (121, 98, 112), (1, 2, False): (122, 98, 112), (1, 2, True): (121, 97, 112),
          (2, 0, False): (128, 97, 112), (2, 1, False): (121, 98, 112), (2, 2, False): (122, 98, 112), (2, 2, True): (123, 97, 112)}


@pytest.fixture(scope="module")
def stats():
    return kernel_listing.stats()


def _kernels(stats):
    got = {}
    for k, v in stats.items():
        m = re.fullmatch(r"pb_stitch_video_kernel<(\d+), (\d+), (true|false)>", k)
        if m:
            got[(int(m.group(1)), int(m.group(2)), m.group(3) == "true")] = v
    return got


def test_eight_instantiations_and_nothing_else_under_the_name(stats):
    got = _kernels(stats)
    assert sorted(got) == sorted(PINNED), sorted(got)
    assert len([n for n in stats if n.startswith("pb_stitch_video")]) == 8
    assert "pb_stitch_mix_kernel" in stats


def test_no_scratch_and_the_waves_of_the_rgb8_two_eye_kernel(stats):
    double = {k: v for k, v in stats.items() if re.fullmatch(r"pb_hot_double_kernel<\d+, true, false>", k)}  # <WMODE, ONE, VEC>: the single-frame form
    assert len(double) == 3, sorted(double)
    bar = max(r["occupancy"] for r in double.values())
    for key, r in _kernels(stats).items():
        print(f"pb_stitch_video_kernel{key}: vgpr {r['vgpr']} sgpr {r['sgpr']} scratch {r['scratch']} waves {r['occupancy']} lane traffic {r['lane_traffic']} "
              f"f64 {r['f64']} instructions {r['instr']}")
        assert r["scratch"] == 0 and r["agpr"] == 0, (key, r)
        assert r["occupancy"] >= bar, (key, r["occupancy"], {k: v["occupancy"] for k, v in double.items()})


def test_the_listing_is_pinned(stats):
    for key, r in _kernels(stats).items():
        assert (r["vgpr"], r["sgpr"], r["lane_traffic"]) == PINNED[key], (key, r["vgpr"], r["sgpr"], r["lane_traffic"])
