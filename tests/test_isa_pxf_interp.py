"""The budget of the interpolating tile kernel for float16 and float32 frames (pb_pxf_interp_kernel), read from the compiler's
listing of the product build like the other ISA tests: thirty-two instantiations - {camera, panorama} x {bilinear, Catmull-Rom} x the eight
(channels, sample bytes) -, no scratch, no float64, the tile entry in scalar registers.  Pixels of up to 8 bytes have pb_px_interp_kernel's
code shape and its bars: four waves per SIMD for the bilinear rows, three for the Catmull-Rom rows.  Pixels of 12 and 16 bytes park one
regrouping plane per dword - 3 x and 4 x 16 896 bytes of LDS a workgroup, three and two workgroups in a CU's 160 KiB - and their occupancy
is pinned at what the listing shows, three and two waves per SIMD: LDS sets it, their 119 to 140 VGPRs would allow three or four
(DESIGN 3.24)."""

import re

import pytest

from tests import kernel_listing
from tests import pxf_cases as fc

KINDS = (0, 2)  # PB_KIND_CAMERA, PB_KIND_PANO as the listing prints them (tests/test_isa_px_interp.py)
BILINEAR, CATMULL_ROM = 1, 2
WIDE_OCCUPANCY = {12: 3, 16: 2}  # rows with B = 12 and 16: the listing's figure, pinned


@pytest.fixture(scope="module")
def stats():
    return kernel_listing.stats()


def _kernels(stats):
    got = {}
    for k, v in stats.items():
        m = re.fullmatch(r"pb_pxf_interp_kernel<(\d+), (\d+), (\d+), (\d+)>", k)
        if m:
            got[tuple(int(g) for g in m.groups())] = v
    return got


def test_thirty_two_instantiations(stats):
    got = _kernels(stats)
    want = sorted((kind, f, c, s) for kind in KINDS for f in (BILINEAR, CATMULL_ROM) for c, s in fc.FORMATS)
    assert sorted(got) == want and len(want) == 32, sorted(got)
    assert len([n for n in stats if n.startswith("pb_pxf_interp")]) == 32  # (and nothing else under the name)


def test_budget(stats):
    for key, r in sorted(_kernels(stats).items()):
        print(f"pb_pxf_interp_kernel{key}: vgpr {r['vgpr']} sgpr {r['sgpr']} waves {r['occupancy']} lane traffic {r['lane_traffic']} instructions {r['instr']}")
        assert r["scratch"] == 0 and r["f64"] == 0, (key, r)
        assert r["lane_traffic"] <= 200, (key, r)  # (a spilled tile entry is 1 300-1 500)
        B = key[2] * key[3]
        if B > 8:
            assert r["occupancy"] == WIDE_OCCUPANCY[B], (key, r["occupancy"])
        elif key[1] == BILINEAR:
            assert r["occupancy"] >= 4, (key, r["occupancy"])
        else:
            assert r["occupancy"] >= 3, (key, r["occupancy"])
