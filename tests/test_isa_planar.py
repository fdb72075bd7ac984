"""The budget of the planar kernels, read from the compiler's listing of the product build like the other ISA tests.
pb_video_hot_kernel without PAIRS: twelve instantiations - {camera, panorama} x two sample sizes x three subsamplings - at
tests/test_isa_nv12.py's bar: no scratch, no float64, the tile entry in scalar registers, at most 128 VGPRs (four waves per SIMD); and the
listing's own figures, pinned.  pb_track_video_kernel without PAIRS: eight instantiations <S, SRC_KIND, false> without scratch, at the
waves of their PAIRS twins <S, SRC_KIND, true> (tests/test_isa_track_nv12.py)."""

import re

import pytest

from tests import kernel_listing

# VGPRs and waves per SIMD of the listing, per (bytes per sample, subsampling) - both source kinds alike; recorded in DESIGN 3.17
# (pb_planar_hot_kernel, before the merge with the NV12 kernel: 122, 123, 117, 123, 122, 115)
PINNED = {(1, 0): (121, 4), (1, 1): (116, 4), (1, 2): (116, 4), (2, 0): (122, 4), (2, 1): (115, 4), (2, 2): (116, 4)}
KINDS = (0, 2, 5, 8)  # camera, panorama, cube, equi-angular cube (a double fisheye is refused)
TRACK_VGPRS = 63  # every instantiation of the track kernel, as for its PAIRS form


@pytest.fixture(scope="module")
def stats():
    return kernel_listing.stats()


def _hot(stats):
    got = {}
    for k, v in stats.items():
        m = re.fullmatch(r"pb_video_hot_kernel<(\d+), (\d+), (\d+), false>", k)
        if m:
            got[tuple(int(g) for g in m.groups())] = v
    return got


def test_twelve_instantiations(stats):
    got = _hot(stats)
    assert len(got) == 12, sorted(got)
    assert {k for k, _, _ in got} == {0, 2} and {s for _, s, _ in got} == {1, 2} and {sub for _, _, sub in got} == {0, 1, 2}
    assert len([n for n in stats if n.startswith("pb_video_hot_kernel")]) == 16  # (and nothing else under the name but tests/test_isa_nv12.py's four)


def test_budget(stats):
    for key, r in _hot(stats).items():
        assert r["scratch"] == 0 and r["f64"] == 0, (key, r)
        assert r["vgpr"] <= 128 and r["occupancy"] >= 4, (key, r)
        assert r["lane_traffic"] <= 8, (key, r)  # (tests/test_isa_nv12.py's level: a spilled tile entry is 1 300-1 500)


def test_the_listing_is_pinned(stats):
    for (kind, S, sub), r in _hot(stats).items():
        assert (r["vgpr"], r["occupancy"]) == PINNED[(S, sub)], (kind, S, sub, r["vgpr"], r["occupancy"])


def test_the_track_kernels_have_no_scratch_and_the_waves_of_their_nv12_twins(stats):
    got = {k: v for k, v in stats.items() if k.startswith("pb_track_video_kernel<") and k.endswith(", false>")}
    assert sorted(got) == sorted(f"pb_track_video_kernel<{S}, {kind}, false>" for kind in KINDS for S in (1, 2)), sorted(got)
    for name, r in got.items():
        twin = stats[name.replace(", false>", ", true>")]
        print(f"{name:40s} vgpr {r['vgpr']:3d} sgpr {r['sgpr']:3d} scratch {r['scratch']} waves {r['occupancy']} instructions {r['instr']} (twin: {twin['occupancy']} waves)")
        assert r["scratch"] == 0 and r["agpr"] == 0, (name, r)
        assert r["occupancy"] >= twin["occupancy"] and r["vgpr"] <= TRACK_VGPRS, (name, r, twin)
        assert r["f64"] <= twin["f64"], (name, r["f64"], twin["f64"])  # the third plane costs no float64
