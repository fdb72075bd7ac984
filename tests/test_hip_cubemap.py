"""The cube map on the device, as a destination and as a source, on every route, against what the REFERENCE produces for the
composition that defines it (tests/golden/cubemap.npz, cubemap_full.json) and against that definition (tests/cubemap_ref.py) at sizes the
tile kernels run at.  A face is a rectilinear camera behind a fixed rotation and the chain has both stages to the bit: the nearest paths
are compared without a tolerance and without a pixel excepted; interpolation FROM a cube is the definition's float64 to the bit;
interpolation INTO a cube rides the tile routes and keeps their modes' 1 LSB."""

import ctypes
import hashlib
import json
import os
import socket

import numpy as np
import pytest
import torch
from click.testing import CliRunner
from PIL import Image

import photonbend_amd as pb
import photonbend_amd.batch  # noqa: F401  (pb.batch)
from oracle import reference_path as orc
from oracle.synth import synth_frame
from photonbend_amd import _native as nat
from photonbend_amd import parallel
from photonbend_amd.scripts import cli
from tests import catmull_rom_ref as crr
from tests import cubemap_cases as cc
from tests import cubemap_ref as cr
from tests import helpers as H
from tests import ss_ref
from tests.cases import Case, cam, inscribed, pano
from tests.test_hip_bilinear import smooth_frame
from tests.test_hip_catmull_rom import _within_one

pytestmark = pytest.mark.gpu
GOLD = np.load(os.path.join(H.GOLD, "cubemap.npz"))
SMALL = cc.small_cases()
cube = cc.cube
rad = pb.utils.to_radians
# about 1000 px a side: sizes at which the windowed tile kernels run (a launch table needs more than a handful of tiles)
MID = [
    Case("KM_pano_cube320_rot", cube(320), pano(768, 1536), [(12, -30, 7)]),      # N = 320: no tile straddles a face
    Case("KM_pano_cube300", cube(300), pano(768, 1536)),                          # N = 300: tiles straddle faces (listed as failed)
    Case("KM_cube384_pano_rot", pano(640, 1280), cube(384), [(5, 60, -20)]),
    Case("KM_cube256_camera", cam(768, 768, "equisolid", 200, inscribed(768)), cube(256), [(-8, 15, 100)]),
    Case("KM_cube320_cube256_rot", cube(256), cube(320), [(3, 90, -7)]),
]


def _private_plan(case, **kw):
    src, cmap = cc.pb_chain(case, image=np.zeros((case.src[1], case.src[2], 3), np.uint8))
    return nat.Plan(cmap.dst_proj, cmap.rotations, src._proj("src"), **kw)


def _same_bits(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and bool(((H.bits(a) == H.bits(b)) | (np.isnan(a) & np.isnan(b))).all())


def _n_diff(a, b):
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    return int((a != b).reshape(a.shape[0], a.shape[1], -1).any(axis=2).sum())


def _gold_index(case):
    n = case.name
    if case.src[0] == "double":
        return GOLD[f"{n}/idx_l"], GOLD[f"{n}/idx_r"], GOLD[f"{n}/w_l"].view(np.float64), GOLD[f"{n}/w_r"].view(np.float64)
    return GOLD[f"{n}/idx"]


def _check_index(plan, case, want):
    """The plan's own index map, written by the kernels its route launches (pb_index_map_i32: the tile kernel + the exact tables on a
    prepared plan, the float64 kernel otherwise)."""
    if case.src[0] == "double":
        i2, w2 = plan.index_map(weights=True)
        i2, w2 = i2.cpu().numpy(), w2.cpu().numpy()
        assert np.array_equal(i2[0], want[0]) and np.array_equal(i2[1], want[1]), case.name
        assert _same_bits(w2[0], want[2]) and _same_bits(w2[1], want[3]), case.name
    else:
        got = plan.index_map().cpu().numpy()
        assert int((got != want).sum()) == 0, f"{case.name}: {int((got != want).sum())} indices differ"


# ---- the reference's bytes, index maps and float64 maps on every path ----------------------------------------------------------------
@pytest.mark.parametrize("case", SMALL, ids=lambda c: c.name)
def test_small_cases_equal_the_reference_on_every_path(case):
    n, want = case.name, GOLD[f"{case.name}/u8"]
    frame = cc.case_frame(case)
    dev = torch.from_numpy(frame).cuda()
    # the materialised float64 maps, stage by stage, to the bit (a cube destination's first map is the already face-rotated one)
    cmap = cc.pb_obj(case.dst).get_coordinate_map()
    assert cmap.is_lazy
    stages = [np.array(np.asarray(cmap))]
    for rot in case.rotations:
        cmap = pb.Rotation(*map(rad, rot)).rotate_coordinate_map(cmap)
        stages.append(np.array(np.asarray(cmap)))
    for k, st in enumerate(stages):
        assert _same_bits(st, GOLD[cc.map_key(case, k)].view(np.float64)), f"{n}: float64 map stage {k} differs from the reference's"
    # a prepared plan: the tile kernels + exact tables
    plan = _private_plan(case)
    assert _n_diff(plan.remap(dev).cpu().numpy(), want) == 0, n
    _check_index(plan, case, _gold_index(case))
    # PB_MODE_FAITHFUL on the same plan: the float64 kernel
    plan.set_mode(nat.MODE_FAITHFUL)
    assert _n_diff(plan.remap(dev).cpu().numpy(), want) == 0, n
    _check_index(plan, case, _gold_index(case))
    # a deferred plan: no preparation, the float64 kernel
    deferred = _private_plan(case, defer=True)
    assert _n_diff(deferred.remap(dev).cpu().numpy(), want) == 0, n
    _check_index(deferred, case, _gold_index(case))
    # the facade, ndarray in -> ndarray out, twice (the first use of a geometry runs a deferred plan, the second prepares it)
    for _ in range(2):
        src, lazy = cc.pb_chain(case, image=frame)
        got = src.process_coordinate_map(lazy)
        assert isinstance(got, np.ndarray) and _n_diff(got, want) == 0, n
    # ... and through a materialised map (the map-stage kernels); a cube source leaves the caller's map unmodified
    src, lazy = cc.pb_chain(case, image=frame)
    host = np.array(np.asarray(lazy))
    keep = host.copy()
    assert _n_diff(src.process_coordinate_map(host), want) == 0, n
    if case.src[0] == "cube":
        assert _same_bits(host, keep), f"{n}: process_coordinate_map of a cube modified the caller's map"


@pytest.mark.parametrize("layout", ["L", "RGBA", "I;16"])
@pytest.mark.parametrize("name", ["K_pano_cube24_chain", "K_inscribed_cube24_rot", "K_cube_pano_rot", "K_cube_camera_corners", "K_cube_cube24_rot", "K_poly_cube24"])
def test_grey_rgba_and_16_bit_images(name, layout):
    """Images the fused uint8 RGB kernel does not take go through the index map and the gather: the reference fancy-indexes whatever
    array it is given, and so does the definition."""
    case = cc.case_by_name(name)
    image = cc.case_frame(case, layout=layout)
    with np.errstate(all="ignore"):
        want = cc.ref_remap(case, image)
    for materialised in (False, True):
        src, lazy = cc.pb_chain(case, image=image)
        got = src.process_coordinate_map(np.array(np.asarray(lazy)) if materialised else lazy)
        assert got.dtype == image.dtype and got.shape == want.shape and int((got != want).sum()) == 0, (name, layout, materialised)
    if image.dtype == np.uint8:  # a device image stays on the device
        src, lazy = cc.pb_chain(case, image=torch.from_numpy(image).cuda())
        got = src.process_coordinate_map(lazy)
        assert got.is_cuda and int((got.cpu().numpy() != want).sum()) == 0


# ---- supersampling: DESIGN 3.6's rule, the n x destination of a cube is the cube of face size n N ---------------------------------------
def _scaled(case, n):
    kind, h, w, lens, fov, mag = case.dst
    if kind == "cube":
        dst = cube(n * (h // 2))
    elif kind == "pano":
        dst = pano(n * h, n * w)
    elif kind == "double":
        dst = ("double", n * h, n * 2 * (w // 2), lens, fov, None)
    else:
        dst = ("camera", n * h, n * w, lens, fov, (h / 2.0 if mag is None else mag) * n)
    return Case(case.name + f"_x{n}", dst, case.src, case.rotations, mask=case.mask)


@pytest.mark.parametrize("n", [2, 4])
@pytest.mark.parametrize("case", SMALL, ids=lambda c: c.name)
def test_supersampled_equals_ss_ref_of_the_definition(case, n):
    frame = cc.case_frame(case)
    with np.errstate(all="ignore"):
        want = ss_ref.block_mean(cc.ref_remap(_scaled(case, n), frame), n)
    src, cm = cc.pb_chain(case, image=frame, supersample=n)
    assert cm.supersample == n and cm.shape[:2] == (n * case.dst[1], n * (2 * (case.dst[2] // 2) if case.dst[0] == "double" else case.dst[2]))
    got = src.process_coordinate_map(cm)  # the facade (a deferred plan at first use)
    assert got.shape == want.shape and _n_diff(got, want) == 0, f"{case.name} n={n}: {_n_diff(got, want)} pixels differ"
    plan = nat.Plan(cm.dst_proj, cm.rotations, src._proj("src"))  # a prepared plan: its own route, and the generic one
    dev = torch.from_numpy(frame).cuda()
    assert _n_diff(plan.remap(dev, supersample=n).cpu().numpy(), want) == 0, (case.name, n)
    assert _n_diff(plan.remap(dev, supersample=n, generic=True).cpu().numpy(), want) == 0, (case.name, n)
    # ... and from a materialised n x map
    assert _n_diff(src.process_coordinate_map(np.array(np.asarray(cm)), supersample=n), want) == 0, (case.name, n)


# ---- the interpolated modes ---------------------------------------------------------------------------------------------------------------
FROM_CUBE = [c for c in SMALL if c.src[0] == "cube"]


@pytest.mark.parametrize("interp", ["bilinear", "catmull-rom"])
@pytest.mark.parametrize("case", FROM_CUBE, ids=lambda c: c.name)
def test_interpolation_from_a_cube_is_the_definition_to_the_bit(case, interp):
    """The camera definition on the selected face, the taps clamped to that face: float64 per pixel on every route a cube source has."""
    ref = cr.remap_bilinear if interp == "bilinear" else cr.remap_catmull_rom
    for layout in ("RGB", "I;16"):
        image = cc.case_frame(case, layout=layout)
        with np.errstate(all="ignore"):
            want = ref(image, cc.ref_stages(case)[-1])
        src, lazy = cc.pb_chain(case, image=image)
        host = np.array(np.asarray(lazy))
        keep = host.copy()
        got = src.process_coordinate_map(host, interpolation=interp)  # the map kernels
        assert got.dtype == want.dtype and got.shape == want.shape and int((got != want).sum()) == 0, f"{case.name} {interp} {layout}: {int((got != want).sum())} samples differ"
        assert _same_bits(host, keep)
        src, lazy = cc.pb_chain(case, image=image)
        got = src.process_coordinate_map(lazy, interpolation=interp)  # the facade: a plan for uint8 RGB, the map kernels otherwise
        assert int((got != want).sum()) == 0, f"{case.name} {interp} {layout} (lazy): {int((got != want).sum())} samples differ"
    frame = cc.case_frame(case)
    with np.errstate(all="ignore"):
        want = ref(frame, cc.ref_stages(case)[-1])
    for kw in ({"bilinear": True}, {"defer": True}):  # the plan's route: per pixel in float64, prepared or not
        plan = _private_plan(case, **kw)
        got = plan.remap(torch.from_numpy(frame).cuda(), interpolation=interp).cpu().numpy()
        assert int((got != want).sum()) == 0, f"{case.name} {interp} plan {kw}: {int((got != want).sum())} samples differ"
        if "bilinear" in kw:
            # no tile tables for a cube source: the library reports every tile as served by the float64 chain
            assert plan.info()["bilinear_float64_tiles"] == plan.info()["tiles"] > 0 and plan.bilinear_tile_mix()["entries"] == 0


def test_taps_stay_on_the_selected_face():
    """Seams are not filtered across faces: six flat faces of different colours never mix, whatever the sampler.  An interpolated pixel is
    its own face's colour - or black where the camera definition is black: the position on the selected face lies in [-0.5, N - 0.5] on
    either axis, the truncating sampler takes (-1, 0) for texel 0, the interpolating modes' liveness test wants a position >= 0."""
    n = 16
    colours = np.array([[250, 10, 10], [10, 250, 10], [10, 10, 250], [250, 250, 10], [10, 250, 250], [250, 10, 250]], np.uint8)
    img = pb.utils.cubemap_from_faces({name: np.broadcast_to(colours[k], (n, n, 3)).copy() for k, name in enumerate(pb.utils.CUBEMAP_FACES)})
    cmap = pb.Rotation(rad(7), rad(33), rad(-12)).rotate_coordinate_map(pb.PanoramaImage(np.zeros((96, 192, 3), np.uint8)).get_coordinate_map())
    with np.errstate(all="ignore"):
        face, fy, fx = cr.pretrunc(n, np.array(np.asarray(cmap)))
    nearest = pb.CubemapImage(img).process_coordinate_map(cmap)
    assert np.array_equal(nearest, colours[face]) and len(np.unique(face)) == 6
    live = (fy >= 0) & (fy < n) & (fx >= 0) & (fx < n)
    assert 0 < int((~live).sum()) < live.size // 8
    want = np.where(live[..., None], colours[face], 0).astype(np.uint8)
    for interp in ("bilinear", "catmull-rom"):
        got = pb.CubemapImage(img).process_coordinate_map(cmap, interpolation=interp)
        assert np.array_equal(got, want), f"{interp}: {int((got != want).any(axis=2).sum())} pixels are neither their face's colour nor the definition's black"


INTO_CUBE = [
    Case("KI_pano_cube256_rot", cube(256), pano(512, 1024), [(12, -30, 7)]),
    Case("KI_pano_cube272_chain", cube(272), pano(640, 1280), [(10, 20, 30), (-40, 5, 77)]),
    # a fisheye and a polynomial-lens source: their frames have an edge, so the modes' existing allowance for the black rim applies
    # (tests/test_hip_catmull_rom.py _within_one, as tests/test_hip_polynomial.py uses it: at most two flips, on a rim of the definition's black)
    Case("KI_fisheye_cube256_rot", cube(256), cam(1024, 1024, "equidistant", 360, inscribed(1024)), [(30, 45, 10)]),
    Case("KI_poly_cube256_rot", cube(256), cam(1024, 1024, "CAL", 200, inscribed(1024)), [(12, -30, 7)]),
]


@pytest.mark.parametrize("case", INTO_CUBE, ids=lambda c: c.name)
def test_interpolation_into_a_cube_rides_the_tile_routes_within_one_lsb(case):
    plan = _private_plan(case, bilinear=True)
    info, mix = plan.info(), plan.bilinear_tile_mix()
    print(f"{case.name}: {info['tiles']} tiles, {info['fix_tiles']} listed whole, bilinear mix {mix}")
    assert info["fast_path"] and mix["entries"] > 0 and mix["window"] + mix["direct"] > 0, (info, mix)  # (the tile kernels, not the float64 route)
    os_ = cr.orc_proj(case.src, cc.lens_of)
    rim = 0 if case.src[0] == "pano" else 2
    with np.errstate(all="ignore"):
        final = cc.ref_stages(case)[-1]
        frame = smooth_frame(case.src[1], case.src[2])  # (on noise every pixel sits on an interpolation edge)
        want = orc.remap_bilinear(None, os_, frame, cmap=np.copy(final))
        got = plan.remap(torch.from_numpy(frame).cuda(), interpolation="bilinear").cpu().numpy()
        d = np.abs(got.astype(np.int16) - want.astype(np.int16))
        print(f"{case.name}: bilinear max difference {int(d.max())} LSB, {100 * float((d.max(axis=2) > 0).mean()):.3f} % of the pixels 1 LSB off")
        _within_one(got, want, False, case.name + " bilinear", rim_flips=rim)
        frame = cc.case_frame(case)
        want = crr.remap(None, os_, frame, cmap=np.copy(final))
        got = plan.remap(torch.from_numpy(frame).cuda(), interpolation="catmull-rom").cpu().numpy()
        share = _within_one(got, want, False, case.name + " catmull-rom", rim_flips=rim)
        print(f"{case.name}: catmull-rom {100 * share:.3f} % of the pixels 1 LSB off")
        # ... and PB_MODE_FAITHFUL: catmull-rom's float64 route is its definition, bilinear's keeps float32 taps
        plan.set_mode(nat.MODE_FAITHFUL)
        got = plan.remap(torch.from_numpy(frame).cuda(), interpolation="catmull-rom").cpu().numpy()
        assert int((got != want).sum()) == 0


def test_double_fisheye_into_a_cube_catmull_rom_is_the_definition():
    """A double-fisheye source's Catmull-Rom runs per pixel in float64 whatever the destination: into a cube, at a size the tile
    kernels of the nearest mode run at, its bytes are the definition's."""
    case = Case("KI_double_cube192_rot", cube(192), ("double", 512, 1024, "equidistant", 195.0, None), [(3, 90, -7)], mask=2)
    frame = cc.case_frame(case)
    with np.errstate(all="ignore"):
        final = cc.ref_stages(case)[-1]
        want = crr.remap(None, cr.orc_proj(case.src), frame, cmap=np.copy(final))
        near = cc.ref_remap(case, frame, final)
    plan = _private_plan(case, bilinear=True)
    dev = torch.from_numpy(frame).cuda()
    got = plan.remap(dev, interpolation="catmull-rom").cpu().numpy()
    assert int((got != want).sum()) == 0, f"{int((got != want).sum())} samples differ"
    assert _n_diff(plan.remap(dev).cpu().numpy(), near) == 0


# ---- mid size: the windowed tile kernels, the exact tables, the tile mix --------------------------------------------------------------
@pytest.mark.parametrize("case", MID, ids=lambda c: c.name)
def test_mid_cases_prepared_plan_float64_kernel_and_definition_agree(case):
    frame = cc.case_frame(case)
    dev = torch.from_numpy(frame).cuda()
    with np.errstate(all="ignore"):
        final = cc.ref_stages(case)[-1]
        want = cc.ref_remap(case, frame, final)
        widx = cc.ref_index(case, final)
    plan = _private_plan(case)
    info = plan.info()
    keys = ("tiles", "fix_tiles", "fix_pixels", "model_diff_pixels", "lean_tiles", "black_tiles", "direct_tiles")
    print(f"{case.name}: {({k: info[k] for k in keys})}")
    # the certified fast path through the windowed tile kernel (a supersampled call needs no workspace exactly when the plain route is WIN)
    assert info["fast_path"] and info["tiles"] > 0 and plan.supersample_workspace_bytes(2) == 0, info
    assert info["fix_tiles"] < info["tiles"] // 2, info  # the models serve most tiles; face edges and seams go to the exact tables
    fast = plan.remap(dev).cpu().numpy()
    assert _n_diff(fast, want) == 0, f"{case.name}: {_n_diff(fast, want)} pixels of the prepared plan differ from the definition"
    _check_index(plan, case, widx)
    # an unaligned frame: the direct-gather kernel + the fix kernel
    odd = torch.empty(frame.size + 1, dtype=torch.uint8, device="cuda")[1:].view(frame.shape)
    odd.copy_(dev)
    assert _n_diff(plan.remap(odd).cpu().numpy(), want) == 0
    plan.set_mode(nat.MODE_FAITHFUL)
    assert _n_diff(plan.remap(dev).cpu().numpy(), want) == 0, case.name
    plan.set_mode(nat.MODE_AUTO)
    if case.dst[0] == "cube":
        n = case.dst[1] // 2
        tiles_x, tiles_y = -(-3 * n // 32), -(-2 * n // 32)
        straddling = sum(1 for ty in range(tiles_y) for tx in range(tiles_x)
                         if (32 * tx) // n != (min(32 * tx + 32, 3 * n) - 1) // n or (32 * ty) // n != (min(32 * ty + 32, 2 * n) - 1) // n)
        assert info["fix_tiles"] >= straddling and (straddling > 0) == (n % 32 != 0), (info, straddling)
    # batches and separately allocated frames: byte-equal to single launches
    frames = [cc.case_frame(case, frame=f) for f in range(3)]
    singles = [plan.remap(torch.from_numpy(f).cuda()).cpu().numpy() for f in frames]
    assert _n_diff(singles[0], want) == 0 and _n_diff(singles[1], singles[0]) > 0
    batch = plan.remap(torch.stack([torch.from_numpy(f) for f in frames]).cuda()).cpu().numpy()
    each = plan.remap_each([torch.from_numpy(f).cuda() for f in frames])
    for k in range(3):
        assert _n_diff(batch[k], singles[k]) == 0 and _n_diff(each[k].cpu().numpy(), singles[k]) == 0, (case.name, k)
    # the fused supersampled kernel on the same plan (the plan as the 2 x destination of a half-size output)
    if case.dst[1] % 2 == 0 and case.dst[2] % 2 == 0:
        assert _n_diff(plan.remap(dev, supersample=2).cpu().numpy(), ss_ref.block_mean(want, 2)) == 0


def test_small_batches_and_remap_each_equal_single_launches():
    for name in ("K_pano_cube28", "K_cube_pano_rot", "K_cube_cube24_rot", "K_double_cube24_rot"):
        case = cc.case_by_name(name)
        frames = [cc.case_frame(case, frame=f) for f in range(4)]
        for kw in ({}, {"defer": True}):
            plan = _private_plan(case, **kw)
            singles = [plan.remap(torch.from_numpy(f).cuda()).cpu().numpy() for f in frames]
            assert _n_diff(singles[0], GOLD[f"{name}/u8"]) == 0
            batch = plan.remap(torch.stack([torch.from_numpy(f) for f in frames]).cuda()).cpu().numpy()
            each = plan.remap_each([torch.from_numpy(f).cuda() for f in frames])
            for k in range(4):
                assert _n_diff(batch[k], singles[k]) == 0 and _n_diff(each[k].cpu().numpy(), singles[k]) == 0, (name, kw, k)
        src, cmap = cc.pb_chain(case, image=frames[0])
        plan = pb.batch.plan_for(cc.pb_obj(case.dst), [pb.Rotation(*map(rad, r)) for r in case.rotations], src)
        outs = list(pb.batch.remap_frames(plan, frames))
        assert all(_n_diff(o, s) == 0 for o, s in zip(outs, singles))


def test_a_blob_carries_the_kind(tmp_path):
    for name in ("KM_pano_cube300", "KM_cube384_pano_rot"):
        case = [c for c in MID if c.name == name][0]
        src, cmap = cc.pb_chain(case, image=np.zeros((case.src[1], case.src[2], 3), np.uint8))
        plan = nat.Plan(cmap.dst_proj, cmap.rotations, src._proj("src"))
        back = nat.Plan.deserialize(plan.serialize(), cmap.dst_proj, cmap.rotations, src._proj("src"))
        assert back.info()["fast_path"] and back.info()["fix_tiles"] == plan.info()["fix_tiles"]
        dev = torch.from_numpy(cc.case_frame(case)).cuda()
        assert torch.equal(back.remap(dev), plan.remap(dev))
        assert torch.equal(back.remap(dev, interpolation="bilinear"), plan.remap(dev, interpolation="bilinear"))
        # the blob of a cube is not the plan of a panorama of the same shape
        swap = lambda p: nat.make_proj(nat.KIND_PANO, p.height, p.width) if p.kind == nat.KIND_CUBE else p  # noqa: E731
        with pytest.raises(nat.PbError):
            nat.Plan.deserialize(plan.serialize(), swap(cmap.dst_proj), cmap.rotations, swap(src._proj("src")))


# ---- full size ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", cc.full_cases(), ids=lambda c: c.name)
def test_full_size_pair_matches_its_pins(case):
    with open(os.path.join(H.GOLD, "cubemap_full.json")) as f:
        pin = json.load(f)[case.name]
    dev = nat.synth_frame(case.src[1], case.src[2], frame=0, seed=0, circle_mask=case.mask)
    plan = _private_plan(case)
    info = plan.info()
    print(f"{case.name}: {({k: info[k] for k in ('tiles', 'fix_tiles', 'fix_pixels', 'lean_tiles', 'direct_tiles', 'black_tiles')})}")
    assert info["fast_path"] and plan.supersample_workspace_bytes(2) == 0
    sha = lambda t: hashlib.sha256(t.contiguous().cpu().numpy().tobytes()).hexdigest()  # noqa: E731
    out, idx = plan.remap(dev), plan.index_map()
    assert list(out.shape) == pin["shape"] and int((idx < 0).sum()) == pin["black"]
    for r, c, *v in pin["samples_u8"]:
        assert out[r, c].tolist() == v, (r, c)
    for r, c, v in pin["samples_idx"]:
        assert int(idx[r, c]) == v, (r, c)
    assert sha(idx) == pin["sha256_idx"], "the prepared plan's index map is not the definition's"
    assert sha(out) == pin["sha256_u8"], "the prepared plan's bytes are not the definition's"
    del out, idx
    plan.set_mode(nat.MODE_FAITHFUL)
    assert sha(plan.remap(dev)) == pin["sha256_u8"] and sha(plan.index_map()) == pin["sha256_idx"], "the float64 kernel"


# ---- the C ABI, the CLI, two ranks ----------------------------------------------------------------------------------------------------------
def test_c_abi_cube_projections():
    """What a C host does: kind, height = 2N and width = 3N; everything else in the pb_proj is ignored."""
    lib = nat.load()
    n = 40
    dst = nat.make_proj(nat.KIND_CUBE, 2 * n, 3 * n, 77, 9.0, 9.0, 9.0)
    m = torch.empty((2 * n, 3 * n, 3), dtype=torch.float64, device="cuda")
    assert lib.pb_coordmap_f64(ctypes.byref(dst), m.data_ptr(), None) == 0
    torch.cuda.synchronize()
    with np.errstate(all="ignore"):
        want_map = cr.coordinate_map(n)
    assert _same_bits(m.cpu().numpy(), want_map)
    # all PB_MAX_ROTATIONS rotations behind the face's, in one plan, against the materialised chain
    rots = [pb.Rotation(rad(5.0 * k), rad(-7.0 * k), rad(3.0 * k + 1)).rotation_matrix for k in range(1, nat.PB_MAX_ROTATIONS + 1)]
    final = want_map
    with np.errstate(all="ignore"):
        for R in rots:
            final = orc.rotate_map(np.asarray(R, np.float64), final)
    src = nat.make_proj(nat.KIND_CUBE, 64, 96)
    frame = synth_frame(64, 96, frame=2, seed=0)
    with np.errstate(all="ignore"):
        want, widx = cr.sample(frame, np.copy(final)), cr.source_index(32, np.copy(final))
    flat = (ctypes.c_double * (9 * len(rots)))(*np.asarray(rots, np.float64).ravel())
    for flags in (0, nat.PLAN_DEFER):
        plan = ctypes.c_void_p()
        assert lib.pb_plan_create_ex(ctypes.byref(dst), flat, len(rots), ctypes.byref(src), flags, 0, ctypes.byref(plan)) == 0
        s, o = torch.from_numpy(frame).cuda(), torch.zeros((2 * n, 3 * n, 3), dtype=torch.uint8, device="cuda")
        idx = torch.empty((2 * n, 3 * n), dtype=torch.int32, device="cuda")
        assert lib.pb_remap_u8(plan, s.data_ptr(), o.data_ptr(), 1, 0, 0, None) == 0
        assert lib.pb_index_map_i32(plan, idx.data_ptr(), None, None) == 0
        torch.cuda.synchronize()
        assert np.array_equal(o.cpu().numpy(), want) and np.array_equal(idx.cpu().numpy(), widx), flags
        lib.pb_plan_destroy(plan)
    # the map-stage calls with a cube source
    dm = torch.from_numpy(final.copy()).cuda()
    s, o = torch.from_numpy(frame).cuda(), torch.zeros((2 * n, 3 * n, 3), dtype=torch.uint8, device="cuda")
    idx = torch.empty((2 * n, 3 * n), dtype=torch.int32, device="cuda")
    assert lib.pb_sample_map_u8(ctypes.byref(src), dm.data_ptr(), 2 * n, 3 * n, s.data_ptr(), o.data_ptr(), None) == 0
    assert lib.pb_index_from_map_i32(ctypes.byref(src), dm.data_ptr(), 2 * n, 3 * n, None, None, idx.data_ptr(), None, None) == 0
    torch.cuda.synchronize()
    assert np.array_equal(o.cpu().numpy(), want) and np.array_equal(idx.cpu().numpy(), widx) and _same_bits(dm.cpu().numpy(), final)


def test_cli_equals_api_and_definition(tmp_path):
    pano_img = synth_frame(64, 128, frame=5, seed=0)
    inp, out = tmp_path / "pano.png", tmp_path / "cube.png"
    Image.fromarray(pano_img).save(inp)
    res = CliRunner().invoke(cli.main, ["pano-to-cubemap", str(inp), "-r", "15", "-40", "5", str(out)])
    assert res.exit_code == 0, (res.output, res.exception)
    got = np.asarray(Image.open(out))
    assert got.shape == (64, 96, 3)  # --face-size defaults to the input height // 2
    case = Case("cli", cube(32), pano(64, 128), [(15, -40, 5)])
    with np.errstate(all="ignore"):
        assert np.array_equal(got, cc.ref_remap(case, pano_img))
    # the way back, with a size, a sampler and supersampling
    back = tmp_path / "back.png"
    res = CliRunner().invoke(cli.main, ["cubemap-to-pano", str(out), "--height", "40", "--supersample", "2", "--interpolation", "bilinear", str(back)])
    assert res.exit_code == 0, (res.output, res.exception)
    cm = pb.PanoramaImage(np.zeros((40, 80, 3), np.uint8)).get_coordinate_map(supersample=2)
    want = pb.CubemapImage(got).process_coordinate_map(cm, interpolation="bilinear")
    assert np.array_equal(np.asarray(Image.open(back)), want) and want.shape == (40, 80, 3)
    with np.errstate(all="ignore"):
        full = cr.remap_bilinear(got, orc.coordinate_map(orc.Proj("pano", 80, 160)))
    assert np.array_equal(want, ss_ref.block_mean(full, 2))
    res = CliRunner().invoke(cli.main, ["cubemap-to-pano", str(out), str(tmp_path / "plain.png")])
    assert res.exit_code == 0 and np.asarray(Image.open(tmp_path / "plain.png")).shape == (64, 128, 3)  # --height defaults to 2 x the face size
    res = CliRunner().invoke(cli.main, ["pano-to-cubemap", str(inp), "--face-size", "20", "--interpolation", "catmull-rom", str(tmp_path / "c20.png")])
    assert res.exit_code == 0 and np.asarray(Image.open(tmp_path / "c20.png")).shape == (40, 60, 3)
    # a grey panorama stays grey
    grey = tmp_path / "grey.png"
    Image.fromarray(pano_img[:, :, 0]).save(grey)
    res = CliRunner().invoke(cli.main, ["pano-to-cubemap", str(grey), str(tmp_path / "gcube.png")])
    assert res.exit_code == 0, (res.output, res.exception)
    with np.errstate(all="ignore"):
        assert np.array_equal(np.asarray(Image.open(tmp_path / "gcube.png")), cc.ref_remap(Case("g", cube(32), pano(64, 128)), np.ascontiguousarray(pano_img[:, :, 0])))


N_FRAMES = 7


def _two_rank_projs():
    dst = pb.CubemapImage(np.zeros((2 * 96, 3 * 96, 3), np.uint8))._proj("dst")
    rots = [pb.Rotation(0.3, -0.7, 0.2).rotation_matrix]
    return dst, rots, pb.CubemapImage(np.zeros((2 * 128, 3 * 128, 3), np.uint8))._proj("src")


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _remap_worker(rank, world, port, q):
    import torch.distributed as dist

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        d, rots, s = _two_rank_projs()
        if rank != 0:  # rank 0's parameters must win: everyone else starts from a panorama and another rotation
            d, rots = nat.make_proj(nat.KIND_PANO, d.height, d.width), [pb.Rotation(1.0, 1.0, 1.0).rotation_matrix]
        load = lambda i: nat.synth_frame(s.height, s.width, frame=i, seed=0)  # noqa: E731
        ids, outs = parallel.remap_batch_sharded(d, rots, s, load, N_FRAMES, device="cpu", chunk=4)
        sha = lambda t: hashlib.sha256(t.contiguous().cpu().numpy().tobytes()).hexdigest()  # noqa: E731
        q.put((rank, ids, [sha(o) for o in outs]))
    finally:
        dist.destroy_process_group()


def test_two_ranks_share_a_cube_batch():
    import torch.multiprocessing as mp

    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_remap_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=300) for _ in procs)
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    (r0, ids0, sh0), (r1, ids1, sh1) = res
    assert (r0, r1) == (0, 1) and ids0 + ids1 == list(range(N_FRAMES)) and len(ids0) == 4
    d, rots, s = _two_rank_projs()
    final = cr.coordinate_map(96)
    with np.errstate(all="ignore"):
        final = orc.rotate_map(np.asarray(rots[0], np.float64), final)
        want = [hashlib.sha256(cr.sample(synth_frame(s.height, s.width, frame=i, seed=0), np.copy(final)).tobytes()).hexdigest() for i in range(N_FRAMES)]
    assert sh0 + sh1 == want, "the sharded union differs from the definition"
