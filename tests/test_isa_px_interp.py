"""The budget of the interpolating tile kernel for grey, RGBA and 16-bit frames (pb_px_interp_kernel), read from the compiler's
listing of the product build like the other ISA tests: twenty-eight instantiations - {camera, panorama} x {bilinear, Catmull-Rom} x the
seven (channels, sample bytes) without (3, 1) -, no scratch, no float64, the tile entry in scalar registers, and the waves per SIMD of the
kernels whose launch shape it has: four for the bilinear rows (pb_planar_bilinear_kernel's), three for the Catmull-Rom rows
(pb_catmull_rom_hot_kernel's floor)."""

import re

import pytest

from tests import kernel_listing
from tests import px_interp_cases as pc

KINDS = (0, 2)  # PB_KIND_CAMERA, PB_KIND_PANO as the listing prints them (tests/test_isa_video_bilinear.py)
BILINEAR, CATMULL_ROM = 1, 2


@pytest.fixture(scope="module")
def stats():
    return kernel_listing.stats()


def _kernels(stats):
    got = {}
    for k, v in stats.items():
        m = re.fullmatch(r"pb_px_interp_kernel<(\d+), (\d+), (\d+), (\d+)>", k)
        if m:
            got[tuple(int(g) for g in m.groups())] = v
    return got


def test_twenty_eight_instantiations(stats):
    got = _kernels(stats)
    want = sorted((kind, f, c, s) for kind in KINDS for f in (BILINEAR, CATMULL_ROM) for c, s in pc.FORMATS)
    assert sorted(got) == want and len(want) == 28, sorted(got)
    assert len([n for n in stats if n.startswith("pb_px_interp")]) == 28  # (and nothing else under the name)
    assert not any(c * s == 3 for _, _, c, s in got)  # uint8 RGB has tile kernels of its own


def test_budget(stats):
    cr = [v for k, v in stats.items() if k.startswith("pb_catmull_rom_hot_kernel<")]
    assert cr, "pb_catmull_rom_hot_kernel is not in the listing"
    for key, r in _kernels(stats).items():
        print(f"pb_px_interp_kernel{key}: vgpr {r['vgpr']} sgpr {r['sgpr']} waves {r['occupancy']} lane traffic {r['lane_traffic']} instructions {r['instr']} lds {r.get('lds')}")
        assert r["scratch"] == 0 and r["f64"] == 0, (key, r)
        assert r["lane_traffic"] <= 200, (key, r)  # (a spilled tile entry is 1 300-1 500)
        if key[1] == BILINEAR:
            assert r["occupancy"] >= 4, (key, r["occupancy"])
        else:
            assert r["occupancy"] >= 3 and r["occupancy"] >= min(c["occupancy"] for c in cr), (key, r["occupancy"])
