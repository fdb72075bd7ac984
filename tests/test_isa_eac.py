"""The equi-angular cube map's kernels in the compiler's listing of the product build (like test_isa_cubemap.py).  Such a
SOURCE adds no model-evaluating kernel: the hot, windowed, supersampled, pixel-size and interpolating tile kernels it launches are the
camera's instantiations, made exact by pb_certify_kernel<8>.  What is new runs the float64 chain - kind 8's own instantiations of the
per-pixel kernels, four kernels of their own name, and the map kernel of a cube destination, which now holds the destination's warp - and
must not spill; their waves per SIMD are pinned at what the build gives, beside the plain cube's counterpart.  An equi-angular source
carries two arctan more than a cube source (one rolled copy): it costs no wave anywhere."""

import re

import pytest

from tests import kernel_listing

EAC, CUBE = 8, 5  # PB_KIND_EAC, PB_KIND_CUBE (include/photonbend_hip.h)
HOT = ("pb_hot_win_kernel", "pb_hot_kernel", "pb_ss_win_kernel", "pb_px_hot_kernel", "pb_bilinear_hot_kernel", "pb_catmull_rom_hot_kernel")
# kind 8's float64 kernels -> (the plain cube's counterpart, waves per SIMD)
PINNED = {
    "pb_remap_kernel<8, -1>": ("pb_remap_kernel<5, -1>", 7),
    "pb_remap_kernel<8, 0>": ("pb_remap_kernel<5, 0>", 8),
    "pb_remap_kernel<8, 1>": ("pb_remap_kernel<5, 1>", 7),
    "pb_index_kernel<8, -1>": ("pb_index_kernel<5, -1>", 8),
    "pb_index_kernel<8, 0>": ("pb_index_kernel<5, 0>", 8),
    "pb_index_kernel<8, 1>": ("pb_index_kernel<5, 1>", 8),
    "pb_sample_map_kernel<8>": ("pb_sample_map_kernel<5>", 8),
    "pb_index_from_map_kernel<8>": ("pb_index_from_map_kernel<5>", 8),
    "pb_model_kernel<8>": ("pb_model_kernel<5>", 8),
    "pb_window_kernel<8>": ("pb_window_kernel<5>", 7),
    "pb_certify_kernel<8, -1>": ("pb_certify_kernel<5, -1>", 5),
    "pb_certify_kernel<8, 0>": ("pb_certify_kernel<5, 0>", 5),
    "pb_certify_kernel<8, 1>": ("pb_certify_kernel<5, 1>", 5),
    "pb_fix_tables_kernel<8>": ("pb_fix_tables_kernel<5>", 8),
    "pb_track_eac_kernel": ("pb_track_kernel<5>", 7),
    "pb_track_interp_eac_kernel<PbBilinear>": ("pb_track_interp_kernel<5, PbBilinear>", 8),
    "pb_track_interp_eac_kernel<PbCatmullRom>": ("pb_track_interp_kernel<5, PbCatmullRom>", 7),
    "pb_interp_eac_kernel<PbBilinear>": ("pb_interp_cube_kernel<PbBilinear>", 8),
    "pb_interp_eac_kernel<PbCatmullRom>": ("pb_interp_cube_kernel<PbCatmullRom>", 4),
    "pb_sample_map_interp_eac_kernel<PbBilinear, unsigned char>": ("pb_sample_map_interp_cube_kernel<PbBilinear, unsigned char>", 8),
    "pb_sample_map_interp_eac_kernel<PbBilinear, unsigned short>": ("pb_sample_map_interp_cube_kernel<PbBilinear, unsigned short>", 8),
    "pb_sample_map_interp_eac_kernel<PbCatmullRom, unsigned char>": ("pb_sample_map_interp_cube_kernel<PbCatmullRom, unsigned char>", 7),
    "pb_sample_map_interp_eac_kernel<PbCatmullRom, unsigned short>": ("pb_sample_map_interp_cube_kernel<PbCatmullRom, unsigned short>", 7),
    # the map kernel of a cube destination of either mapping: pb_coordmap_kernel's chain, the warp and one rotation
    "pb_coordmap_cube_kernel": ("pb_coordmap_kernel", 8),
}


@pytest.fixture(scope="module")
def stats():
    return kernel_listing.stats()


def _kind_args(name):
    m = re.match(r"^(\w+)<(.*)>$", name)
    return (m.group(1), [a.strip() for a in m.group(2).split(",")]) if m else (name, [])


def test_no_hot_kernel_has_an_instantiation_for_the_kind(stats):
    for name in stats:
        base, args = _kind_args(name)
        if base in HOT:
            assert args and args[0] != str(EAC), f"{name}: an equi-angular source is served by the camera's hot kernels (DESIGN 3.14)"
    assert any(_kind_args(n)[0] == "pb_hot_win_kernel" for n in stats)


def test_every_kernel_of_the_kind_is_listed_here(stats):
    """Whatever the build instantiates for kind 8, or names after it, is pinned below - and the plain cube's kernels kept their names."""
    mine = {n for n in stats if "eac" in n or (_kind_args(n)[0] not in HOT and _kind_args(n)[1][:1] == [str(EAC)])}
    assert mine == set(PINNED) - {"pb_coordmap_cube_kernel"}, sorted(mine ^ (set(PINNED) - {"pb_coordmap_cube_kernel"}))
    assert all(twin in stats for twin, _ in PINNED.values())


def test_the_float64_kernels_of_the_kind_have_no_scratch_and_keep_their_waves(stats):
    for name, (twin, waves) in PINNED.items():
        r, ref = stats[name], stats[twin]
        print(f"{name:62s} vgpr {r['vgpr']:3d} sgpr {r['sgpr']:3d} scratch {r['scratch']} waves {r['occupancy']} instructions {r['instr']:5d}"
              f"   ({twin}: vgpr {ref['vgpr']}, waves {ref['occupancy']}, instructions {ref['instr']})")
        assert r["scratch"] == 0 and r["agpr"] == 0, (name, r)
        assert r["occupancy"] == waves, (name, r["occupancy"], waves)
        if twin != "pb_coordmap_kernel":  # two arctan more than the cube source's kernel, in one rolled copy: no wave lost
            assert r["occupancy"] >= ref["occupancy"], (name, r, ref)
    w = stats["pb_window_kernel<8>"]
    assert w["f64"] == 0 and w["vgpr"] <= stats["pb_window_kernel<0>"]["vgpr"], w


def test_the_warps_are_one_rolled_copy_each(stats):
    """An equi-angular source's kernel grows over the cube's by ONE arctan and the unwarp around it, not two; the destination's tangent
    lives in the run-time-rotation-count instantiations alone (a cube destination runs no other: pb_rot_count), in one copy."""
    one_rotation = stats["pb_index_kernel<2, 1>"]["instr"] - stats["pb_index_kernel<2, 0>"]["instr"]
    for rot in (-1, 0, 1):
        grown = stats[f"pb_index_kernel<8, {rot}>"]["instr"] - stats[f"pb_index_kernel<5, {rot}>"]["instr"]
        print(f"pb_index_kernel<8, {rot}> holds {grown} instructions more than <5, {rot}>; one rotation is {one_rotation}")
        assert 0 < grown < one_rotation // 8, (rot, grown, one_rotation)
    for kind in (0, 2, 5, 8):
        grown = stats[f"pb_index_kernel<{kind}, -1>"]["instr"] - stats[f"pb_index_kernel<{kind}, 1>"]["instr"]
        print(f"pb_index_kernel<{kind}, -1> holds {grown} instructions more than <{kind}, 1> (the face rotation's multiply-adds and the destination's tangent)")
        assert grown < one_rotation // 4, (kind, grown, one_rotation)
