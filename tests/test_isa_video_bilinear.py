"""The budget of the bilinear video kernel (pb_planar_bilinear_kernel), read from the compiler's listing of the product build
like the other ISA tests: sixteen instantiations - {camera, panorama} x two sample sizes x {4:4:4, 4:2:2, 4:2:0, 4:2:0 with interleaved
pairs} -, no scratch, no float64, the tile entry in scalar registers, at least the waves per SIMD of pb_catmull_rom_hot_kernel (whose launch
shape it has) in the same listing; and the listing's own figures, pinned."""

import re

import pytest

from tests import kernel_listing

# VGPRs and waves per SIMD of the listing, per (source kind, bytes per sample, subsampling, pairs); recorded in DESIGN 3.18
PINNED = {
    (0, 1, 0, False): (107, 4), (0, 1, 1, False): (91, 4), (0, 1, 2, False): (92, 4), (0, 1, 2, True): (89, 4),
    (0, 2, 0, False): (108, 4), (0, 2, 1, False): (91, 4), (0, 2, 2, False): (92, 4), (0, 2, 2, True): (89, 4),
    (2, 1, 0, False): (107, 4), (2, 1, 1, False): (91, 4), (2, 1, 2, False): (91, 4), (2, 1, 2, True): (88, 4),
    (2, 2, 0, False): (108, 4), (2, 2, 1, False): (91, 4), (2, 2, 2, False): (90, 4), (2, 2, 2, True): (88, 4),
}


@pytest.fixture(scope="module")
def stats():
    return kernel_listing.stats()


def _kernels(stats):
    got = {}
    for k, v in stats.items():
        m = re.fullmatch(r"pb_planar_bilinear_kernel<(\d+), (\d+), (\d+), (true|false)>", k)
        if m:
            got[(int(m.group(1)), int(m.group(2)), int(m.group(3)), m.group(4) == "true")] = v
    return got


def test_sixteen_instantiations(stats):
    got = _kernels(stats)
    assert sorted(got) == sorted(PINNED), sorted(got)
    assert len([n for n in stats if n.startswith("pb_planar_bilinear_kernel")]) == 16  # (and nothing else under the name)
    assert all(sub == 2 for _, _, sub, pairs in got if pairs)  # interleaved pairs are 4:2:0


def test_budget(stats):
    cr = [v for k, v in stats.items() if k.startswith("pb_catmull_rom_hot_kernel<")]
    assert cr, "pb_catmull_rom_hot_kernel is not in the listing"
    for key, r in _kernels(stats).items():
        assert r["scratch"] == 0 and r["f64"] == 0, (key, r)
        assert r["lane_traffic"] <= 8, (key, r)  # (tests/test_isa_nv12.py's level: a spilled tile entry is 1 300-1 500)
        assert r["occupancy"] >= max(c["occupancy"] for c in cr), (key, r["occupancy"], [c["occupancy"] for c in cr])


def test_the_listing_is_pinned(stats):
    for key, r in _kernels(stats).items():
        print(f"pb_planar_bilinear_kernel{key}: vgpr {r['vgpr']} sgpr {r['sgpr']} waves {r['occupancy']} instructions {r['instr']}")
        assert (r["vgpr"], r["occupancy"]) == PINNED[key], (key, r["vgpr"], r["occupancy"])
