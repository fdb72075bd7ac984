"""The cube map's kernels in the compiler's listing of the product build (like test_isa_budget.py).  A cube SOURCE adds no model-evaluating
kernel: the hot, windowed, supersampled and interpolating tile kernels it launches are the camera's instantiations, made exact by
pb_certify_kernel<5> - so there is nothing new on the hot path to budget, and this test says so: should a cube instantiation of
a hot kernel ever appear it is held to the camera's registers, without scratch or float64.  What IS new runs the float64 chain - the
cube's own instantiations of the per-pixel kernels and the cube destination's map kernel - and must not spill or lose waves against
the camera's."""

import re

import pytest

from tests import kernel_listing

CUBE, CAMERA = 5, 0  # PB_KIND_CUBE, PB_KIND_CAMERA (include/photonbend_hip.h)
HOT = ("pb_hot_win_kernel", "pb_hot_kernel", "pb_ss_win_kernel", "pb_bilinear_hot_kernel", "pb_catmull_rom_hot_kernel")
# kernels of the float64 chain that exist per source kind: the template argument that is the kind
FLOAT64 = {"pb_remap_kernel": 0, "pb_index_kernel": 0, "pb_sample_map_kernel": 0, "pb_index_from_map_kernel": 0, "pb_model_kernel": 0,
           "pb_certify_kernel": 0, "pb_fix_tables_kernel": 0}
# ... and the cube's interpolating kernels, which carry names of their own: cube kernel -> the camera's counterpart
NAMED = {
    "pb_interp_cube_kernel<PbBilinear>": "pb_interp_fix_kernel<PbBilinear, 0>",
    "pb_interp_cube_kernel<PbCatmullRom>": "pb_interp_fix_kernel<PbCatmullRom, 0>",
    "pb_sample_map_interp_cube_kernel<PbBilinear, unsigned char>": "pb_sample_map_interp_kernel<PbBilinear, 0, unsigned char>",
    "pb_sample_map_interp_cube_kernel<PbBilinear, unsigned short>": "pb_sample_map_interp_kernel<PbBilinear, 0, unsigned short>",
    "pb_sample_map_interp_cube_kernel<PbCatmullRom, unsigned char>": "pb_sample_map_interp_kernel<PbCatmullRom, 0, unsigned char>",
    "pb_sample_map_interp_cube_kernel<PbCatmullRom, unsigned short>": "pb_sample_map_interp_kernel<PbCatmullRom, 0, unsigned short>",
}


@pytest.fixture(scope="module")
def stats():
    return kernel_listing.stats()


def _split(name):
    m = re.match(r"^(\w+)<(.*)>$", name)
    return (m.group(1), [a.strip() for a in m.group(2).split(",")]) if m else (name, [])


def _of_kind(stats, base, pos, kind):
    out = {}
    for name, r in stats.items():
        b, args = _split(name)
        if b == base and len(args) > pos and args[pos] == str(kind):
            out[tuple(args[:pos] + args[pos + 1:])] = (name, r)
    return out


def test_a_cube_source_launches_the_camera_s_hot_kernels(stats):
    for base in HOT:
        cam = _of_kind(stats, base, 0, CAMERA)
        assert cam, f"{base}: no camera instantiation"
        for rest, (name, r) in _of_kind(stats, base, 0, CUBE).items():  # (none today: the bound a new one would be held to)
            ref = cam[rest][1]
            assert r["scratch"] == 0 and r["f64"] == 0 and r["vgpr"] <= ref["vgpr"], (name, r, ref)
        for name, r in cam.values():
            assert r["scratch"] == 0, (name, r)
            if base != "pb_hot_kernel":  # (pb_hot_kernel's OUT = 1 form is the index-map writer)
                assert r["f64"] == 0, (name, r)
    assert not any(_of_kind(stats, base, 0, CUBE) for base in HOT), "a cube source is served by the camera's hot kernels (DESIGN 3.10)"


def test_the_cube_s_float64_kernels_keep_the_camera_s_waves_without_scratch(stats):
    seen = 0
    for base, pos in FLOAT64.items():
        cube, cam = _of_kind(stats, base, pos, CUBE), _of_kind(stats, base, pos, CAMERA)
        assert cube and set(cube) == set(cam), f"{base}: cube instantiations {sorted(cube)} against the camera's {sorted(cam)}"
        for rest, (name, r) in cube.items():
            ref = cam[rest][1]
            print(f"{name:64s} vgpr {r['vgpr']:3d} sgpr {r['sgpr']:3d} scratch {r['scratch']} waves {r['occupancy']} (camera: vgpr {ref['vgpr']}, waves {ref['occupancy']})")
            assert r["scratch"] == 0 and r["occupancy"] >= ref["occupancy"], (name, r, ref)
            seen += 1
    for name, twin in NAMED.items():
        r, ref = stats[name], stats[twin]
        print(f"{name:64s} vgpr {r['vgpr']:3d} sgpr {r['sgpr']:3d} scratch {r['scratch']} waves {r['occupancy']} (camera: vgpr {ref['vgpr']}, waves {ref['occupancy']})")
        assert r["scratch"] == 0 and r["occupancy"] >= ref["occupancy"], (name, r, ref)
        seen += 1
    assert seen == 13 + len(NAMED), seen
    # the cube destination's map kernel: pb_coordmap_kernel's chain plus one rotation
    r = stats["pb_coordmap_cube_kernel"]
    assert r["scratch"] == 0 and r["occupancy"] >= stats["pb_coordmap_kernel"]["occupancy"], r
    w = stats["pb_window_kernel<5>"]
    assert w["scratch"] == 0 and w["f64"] == 0 and w["vgpr"] <= stats["pb_window_kernel<0>"]["vgpr"], w


def test_the_face_rotation_did_not_copy_the_rotation_s_transcendentals(stats):
    """pb_rotate_all's loop holds one sine, cosine, complex exponential, arccosine and atan2 for the caller's rotations and the face's:
    the instantiations with a run-time rotation count grow by the nine multiply-adds of the face's matrix, not by a second rotation
    (a whole one is about 2 600 instructions: pb_index_kernel<2, 1> against pb_index_kernel<2, 0>)."""
    one = stats["pb_index_kernel<2, 1>"]["instr"] - stats["pb_index_kernel<2, 0>"]["instr"]
    assert one > 1500
    for kind in (0, 2):
        grown = stats[f"pb_index_kernel<{kind}, -1>"]["instr"] - stats[f"pb_index_kernel<{kind}, 1>"]["instr"]
        print(f"pb_index_kernel<{kind}, -1> holds {grown} instructions more than <{kind}, 1>; one rotation is {one}")
        assert grown < one // 4, (kind, grown, one)
