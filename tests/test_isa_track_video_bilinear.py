"""The bilinear rotation-track kernel for video frames in the compiler's listing of the product build (like test_isa_track_nv12.py; DESIGN
3.19).  A resource pin only: exactly the eight instantiations exist under the kernel's name, without scratch and without AGPRs - a
condition: no frame-loop kernel of this library spills - and the waves per SIMD and vector registers are those of the shipped listing,
the figures of DESIGN 3.19's table (measured, not set in advance).  The template arguments are <S, SRC_KIND, PAIRS>."""

import pytest

from tests import kernel_listing

NAME = "pb_track_video_bilinear_kernel"
KINDS = {0: "camera", 2: "panorama"}  # pb_kind (include/photonbend_hip.h): the sources the definition covers
SAMPLES = (1, 2)
PAIRS = ("false", "true")  # three planes at a run-time subsampling; NV12 / P010's interleaved pair plane
# the shipped listing: a panorama source is compiled for eight waves per SIMD and has them; a camera source, which spills 20 bytes when
# held to eight, gets the budget of four, under which the compiler takes seven
WAVES = {0: 7, 2: 8}
VGPRS = {0: 67, 2: 63}


@pytest.fixture(scope="module")
def stats():
    return kernel_listing.stats()


def _mine(stats):
    return {k: v for k, v in stats.items() if k.startswith(NAME)}


def test_exactly_the_eight_instantiations_exist_under_the_name(stats):
    assert sorted(_mine(stats)) == sorted(f"{NAME}<{S}, {kind}, {p}>" for kind in KINDS for S in SAMPLES for p in PAIRS), sorted(_mine(stats))


def test_no_scratch_no_agprs_and_the_pinned_waves_and_registers(stats):
    for name, r in _mine(stats).items():
        print(f"{name:48s} vgpr {r['vgpr']:3d} sgpr {r['sgpr']:3d} scratch {r['scratch']} waves {r['occupancy']} float64 {r['f64']} instructions {r['instr']}")
        kind = int(name[len(NAME) + 1:-1].split(",")[1])
        assert r["scratch"] == 0 and r["agpr"] == 0, (name, r)
        assert r["occupancy"] == WAVES[kind] and r["vgpr"] == VGPRS[kind], (name, r)
