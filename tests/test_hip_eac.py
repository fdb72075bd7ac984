"""The equi-angular cube map on the device, as a destination and as a source, on every route, against its written NumPy
definition (tests/eac_ref.py; tests/golden/eac.npz holds its bits on the goldens' platform).  The chain evaluates the two warp functions
with the very np.tan / np.arctan it restates for the lenses, so the nearest paths are compared without a tolerance and without a pixel
excepted; interpolation FROM an equi-angular cube is the definition's float64 to the bit; interpolation INTO one rides the tile routes
and keeps their modes' bar (tests/interp_cases.py: no pixel beyond 1 LSB)."""

import ctypes
import os

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
from photonbend_amd.scripts import cli
from tests import catmull_rom_ref as crr
from tests import cubemap_ref as cr
from tests import eac_cases as ec
from tests import eac_ref as er
from tests import helpers as H
from tests import interp_cases as ic
from tests import ss_ref
from tests.cases import Case, cam, inscribed, pano
from tests.test_hip_catmull_rom_tiles import _check as tile_bar

pytestmark = pytest.mark.gpu
GOLD = np.load(os.path.join(H.GOLD, "eac.npz"))
SMALL = ec.small_cases()
eac, cube = ec.eac, ec.cube
rad = pb.utils.to_radians


def _private_plan(case, **kw):
    src, cmap = ec.pb_chain(case, image=np.zeros((case.src[1], case.src[2], 3), np.uint8))
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
    if case.src[0] == "double":
        i2, w2 = plan.index_map(weights=True)
        i2, w2 = i2.cpu().numpy(), w2.cpu().numpy()
        assert np.array_equal(i2[0], want[0]) and np.array_equal(i2[1], want[1]), case.name
        assert _same_bits(w2[0], want[2]) and _same_bits(w2[1], want[3]), case.name
    else:
        got = plan.index_map().cpu().numpy()
        assert int((got != want).sum()) == 0, f"{case.name}: {int((got != want).sum())} indices differ"


# ---- the definition's bytes, index maps and float64 maps on every nearest path ----------------------------------------------------------
@pytest.mark.parametrize("case", SMALL, ids=lambda c: c.name)
def test_small_cases_equal_the_definition_on_every_path(case):
    n, want = case.name, GOLD[f"{case.name}/u8"]
    frame = ec.case_frame(case)
    dev = torch.from_numpy(frame).cuda()
    # the materialised float64 maps, stage by stage, to the bit
    cmap = ec.pb_obj(case.dst).get_coordinate_map()
    assert cmap.is_lazy
    stages = [np.array(np.asarray(cmap))]
    for rot in case.rotations:
        cmap = pb.Rotation(*map(rad, rot)).rotate_coordinate_map(cmap)
        stages.append(np.array(np.asarray(cmap)))
    for k, st in enumerate(stages):
        assert _same_bits(st, GOLD[ec.map_key(case, k)].view(np.float64)), f"{n}: float64 map stage {k} differs from the definition's"
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
        src, lazy = ec.pb_chain(case, image=frame)
        got = src.process_coordinate_map(lazy)
        assert isinstance(got, np.ndarray) and _n_diff(got, want) == 0, n
    # ... and through a materialised map (the map-stage kernels); a cube source of either mapping leaves the caller's map unmodified
    src, lazy = ec.pb_chain(case, image=frame)
    host = np.array(np.asarray(lazy))
    keep = host.copy()
    assert _n_diff(src.process_coordinate_map(host), want) == 0, n
    if case.src[0] in ("cube", "eac"):
        assert _same_bits(host, keep), f"{n}: process_coordinate_map of a cube modified the caller's map"


def test_the_fixture_is_the_live_definition_where_the_host_is_the_goldens_platform():
    if not H.live_numpy_is_the_goldens_numpy():
        pytest.skip("this host's NumPy is not the goldens'")
    case = ec.case_by_name("E_eac_eac24_rot")
    with np.errstate(all="ignore"):
        assert np.array_equal(ec.ref_remap(case, ec.case_frame(case)), GOLD[f"{case.name}/u8"])


@pytest.mark.parametrize("layout", ["L", "RGBA", "I;16"])
@pytest.mark.parametrize("name", ["E_pano_eac24_chain", "E_inscribed_eac24_rot", "E_eac_pano_rot", "E_eac_camera_corners", "E_eac_eac24_rot", "E_eac24_cube32_rot"])
def test_grey_rgba_and_16_bit_images(name, layout):
    """Through pb_remap_px on a prepared plan (the second use of a geometry) and through the index map and the gather (the first use, a
    materialised map): the definition fancy-indexes whatever array it is given."""
    case = ec.case_by_name(name)
    image = ec.case_frame(case, layout=layout)
    with np.errstate(all="ignore"):
        want = ec.ref_remap(case, image)
    for materialised in (False, False, True):
        src, lazy = ec.pb_chain(case, image=image)
        got = src.process_coordinate_map(np.array(np.asarray(lazy)) if materialised else lazy)
        assert got.dtype == image.dtype and got.shape == want.shape and int((got != want).sum()) == 0, (name, layout, materialised)
    # pb_remap_px itself: a prepared plan of a single source takes pixels of 1, 2 and 4 bytes (pb_remap_px_supported); a deferred plan
    # does not, which is why the facade's first use of a geometry went through the gather above
    plan = _private_plan(case)
    dev = torch.from_numpy(image.view(np.uint8).reshape(image.shape[0], image.shape[1], -1)).cuda()
    bpp = dev.shape[2]
    assert bpp == {"L": 1, "I;16": 2, "RGBA": 4}[layout] and plan.px_supported(bpp), (name, layout, bpp)
    got = plan.remap_px(dev).cpu().numpy().reshape(-1).view(image.dtype).reshape(want.shape)
    assert int((got != want).sum()) == 0, (name, layout, "pb_remap_px")
    assert not _private_plan(case, defer=True).px_supported(bpp)
    if image.dtype == np.uint8:  # a device image stays on the device
        src, lazy = ec.pb_chain(case, image=torch.from_numpy(image).cuda())
        got = src.process_coordinate_map(lazy)
        assert got.is_cuda and int((got.cpu().numpy() != want).sum()) == 0


# ---- supersampling: DESIGN 3.6's rule, the n x destination of an equi-angular cube is the one of face size n N ---------------------------
@pytest.mark.parametrize("n", [2, 4])
@pytest.mark.parametrize("case", SMALL, ids=lambda c: c.name)
def test_supersampled_equals_the_box_mean_of_the_definition(case, n):
    frame = ec.case_frame(case)
    with np.errstate(all="ignore"):
        want = ss_ref.block_mean(ec.ref_remap(ec.scaled(case, n), frame), n)
    src, cm = ec.pb_chain(case, image=frame, supersample=n)
    assert cm.supersample == n and cm.shape[:2] == (n * case.dst[1], n * (2 * (case.dst[2] // 2) if case.dst[0] == "double" else case.dst[2]))
    got = src.process_coordinate_map(cm)  # the facade (a deferred plan at first use)
    assert got.shape == want.shape and _n_diff(got, want) == 0, f"{case.name} n={n}: {_n_diff(got, want)} pixels differ"
    plan = nat.Plan(cm.dst_proj, cm.rotations, src._proj("src"))  # a prepared plan: its own route, and the generic one
    dev = torch.from_numpy(frame).cuda()
    assert _n_diff(plan.remap(dev, supersample=n).cpu().numpy(), want) == 0, (case.name, n)
    assert _n_diff(plan.remap(dev, supersample=n, generic=True).cpu().numpy(), want) == 0, (case.name, n)
    assert _n_diff(src.process_coordinate_map(np.array(np.asarray(cm)), supersample=n), want) == 0, (case.name, n)


# ---- the interpolated modes ---------------------------------------------------------------------------------------------------------------
FROM_EAC = [c for c in SMALL if c.src[0] == "eac"]


@pytest.mark.parametrize("interp", ["bilinear", "catmull-rom"])
@pytest.mark.parametrize("case", FROM_EAC, ids=lambda c: c.name)
def test_interpolation_from_an_equiangular_cube_is_the_definition_to_the_bit(case, interp):
    """The camera definition on the selected face at the unwarped position, the taps clamped to that face: float64 per pixel on every route."""
    ref = er.remap_bilinear if interp == "bilinear" else er.remap_catmull_rom
    for layout in ("RGB", "I;16"):
        image = ec.case_frame(case, layout=layout)
        with np.errstate(all="ignore"):
            want = ref(image, ec.ref_stages(case)[-1])
        src, lazy = ec.pb_chain(case, image=image)
        host = np.array(np.asarray(lazy))
        keep = host.copy()
        got = src.process_coordinate_map(host, interpolation=interp)  # the map kernels
        assert got.dtype == want.dtype and got.shape == want.shape and int((got != want).sum()) == 0, f"{case.name} {interp} {layout}: {int((got != want).sum())} samples differ"
        assert _same_bits(host, keep)
        src, lazy = ec.pb_chain(case, image=image)
        got = src.process_coordinate_map(lazy, interpolation=interp)  # the facade: a plan for uint8 RGB, the map kernels otherwise
        assert int((got != want).sum()) == 0, f"{case.name} {interp} {layout} (lazy): {int((got != want).sum())} samples differ"
    frame = ec.case_frame(case)
    with np.errstate(all="ignore"):
        want = ref(frame, ec.ref_stages(case)[-1])
    for kw in ({"bilinear": True}, {"defer": True}):  # the plan's route: per pixel in float64, prepared or not
        plan = _private_plan(case, **kw)
        got = plan.remap(torch.from_numpy(frame).cuda(), interpolation=interp).cpu().numpy()
        assert int((got != want).sum()) == 0, f"{case.name} {interp} plan {kw}: {int((got != want).sum())} samples differ"
        if "bilinear" in kw:  # no tile tables for such a source: every tile is served by the float64 chain
            assert plan.info()["bilinear_float64_tiles"] == plan.info()["tiles"] > 0 and plan.bilinear_tile_mix()["entries"] == 0


INTO_EAC = [
    Case("EI_pano_eac256_rot", eac(256), pano(512, 1024), [(12, -30, 7)]),
    Case("EI_pano_eac272_chain", eac(272), pano(640, 1280), [(10, 20, 30), (-40, 5, 77)]),  # N = 272: 32-px tiles straddle faces
    Case("EI_fisheye_eac256_rot", eac(256), cam(1024, 1024, "equidistant", 360, inscribed(1024)), [(30, 45, 10)]),  # a source with a frame edge
]


@pytest.mark.parametrize("case", INTO_EAC, ids=lambda c: c.name)
def test_interpolation_into_an_equiangular_cube_rides_the_tile_routes_within_one_lsb(case):
    """tests/interp_cases.py's bar (tests/test_hip_catmull_rom_tiles._check), every pixel on a frame of independent random texels: no channel
    beyond 1 LSB of the definition; black in one result and sampled in the other only within 1 / 512 px of a camera source's frame edge -
    nowhere for a panorama source."""
    plan = _private_plan(case, bilinear=True)
    info, mix = plan.info(), plan.bilinear_tile_mix()
    print(f"{case.name}: {info['tiles']} tiles, {info['fix_tiles']} listed whole, bilinear mix {mix}")
    assert info["fast_path"] and mix["entries"] > 0 and mix["window"] + mix["direct"] > 0, (info, mix)  # (the tile kernels, not the float64 route)
    os_ = cr.orc_proj(case.src, ec.lens_of)
    frame = ic.noise_frame(case)
    dev = torch.from_numpy(frame).cuda()
    with np.errstate(all="ignore"):
        final = ec.ref_stages(case)[-1]
        band = ic.edge_band(case, final, 1.0 / 512.0)
        assert not band.any() or case.src[0] == "camera"
        want = orc.remap_bilinear(None, os_, frame, cmap=np.copy(final))
        share = tile_bar(plan.remap(dev, interpolation="bilinear").cpu().numpy(), want, band, False, case.name + " bilinear")
        print(f"{case.name}: bilinear {100 * share:.3f} % of the pixels 1 LSB off")
        want = crr.remap(None, os_, frame, cmap=np.copy(final))
        share = tile_bar(plan.remap(dev, interpolation="catmull-rom").cpu().numpy(), want, band, False, case.name + " catmull-rom")
        print(f"{case.name}: catmull-rom {100 * share:.3f} % of the pixels 1 LSB off")
        plan.set_mode(nat.MODE_FAITHFUL)  # catmull-rom's float64 route is its definition
        assert int((plan.remap(dev, interpolation="catmull-rom").cpu().numpy() != want).sum()) == 0


# ---- mid size: the windowed tile kernels, the exact tables, the tile mix --------------------------------------------------------------
@pytest.mark.parametrize("case", ec.mid_cases(), ids=lambda c: c.name)
def test_mid_cases_prepared_plan_float64_kernel_and_definition_agree(case):
    frame = ec.case_frame(case)
    dev = torch.from_numpy(frame).cuda()
    with np.errstate(all="ignore"):
        final = ec.ref_stages(case)[-1]
        want = ec.ref_remap(case, frame, final)
        widx = ec.ref_index(case, final)
    plan = _private_plan(case)
    info = plan.info()
    keys = ("tiles", "fix_tiles", "fix_pixels", "model_diff_pixels", "lean_tiles", "black_tiles", "direct_tiles")
    print(f"{case.name}: {({k: info[k] for k in keys})}")
    assert info["fast_path"] and info["tiles"] > 0, info
    fast = plan.remap(dev).cpu().numpy()
    assert _n_diff(fast, want) == 0, f"{case.name}: {_n_diff(fast, want)} pixels of the prepared plan differ from the definition"
    _check_index(plan, case, widx)
    odd = torch.empty(frame.size + 1, dtype=torch.uint8, device="cuda")[1:].view(frame.shape)  # an unaligned frame: the direct-gather kernel
    odd.copy_(dev)
    assert _n_diff(plan.remap(odd).cpu().numpy(), want) == 0
    plan.set_mode(nat.MODE_FAITHFUL)
    assert _n_diff(plan.remap(dev).cpu().numpy(), want) == 0, case.name
    _check_index(plan, case, widx)
    if case.dst[0] == "eac":
        n = case.dst[1] // 2
        tiles_x, tiles_y = -(-3 * n // 32), -(-2 * n // 32)
        straddling = sum(1 for ty in range(tiles_y) for tx in range(tiles_x)
                         if (32 * tx) // n != (min(32 * tx + 32, 3 * n) - 1) // n or (32 * ty) // n != (min(32 * ty + 32, 2 * n) - 1) // n)
        assert info["fix_tiles"] >= straddling > 0, (info, straddling)
    else:  # window (LEAN) and direct tiles, whole tiles from the exact tables and fix pixels in one plan
        assert info["lean_tiles"] > 0 and info["direct_tiles"] > 0, info
        assert info["fix_tiles"] > 0 and info["fix_pixels"] > 0 and info["fix_tiles"] < info["tiles"], info


# ---- batches and rotation tracks ---------------------------------------------------------------------------------------------------------------
def test_batches_remap_each_and_remap_frames_equal_single_launches():
    for name in ("E_pano_eac28", "E_eac_pano_rot", "E_eac_eac24_rot"):
        case = ec.case_by_name(name)
        frames = [ec.case_frame(case, frame=f) for f in range(3)]
        for kw in ({}, {"defer": True}):
            plan = _private_plan(case, **kw)
            singles = [plan.remap(torch.from_numpy(f).cuda()).cpu().numpy() for f in frames]
            assert _n_diff(singles[0], GOLD[f"{name}/u8"]) == 0 and _n_diff(singles[1], singles[0]) > 0
            batch = plan.remap(torch.stack([torch.from_numpy(f) for f in frames]).cuda()).cpu().numpy()
            each = plan.remap_each([torch.from_numpy(f).cuda() for f in frames])  # pb_remap_u8v
            for k in range(3):
                assert _n_diff(batch[k], singles[k]) == 0 and _n_diff(each[k].cpu().numpy(), singles[k]) == 0, (name, kw, k)
        src, cmap = ec.pb_chain(case, image=frames[0])
        plan = pb.batch.plan_for(ec.pb_obj(case.dst), [pb.Rotation(*map(rad, r)) for r in case.rotations], src)
        outs = list(pb.batch.remap_frames(plan, frames))
        assert all(_n_diff(o, s) == 0 for o, s in zip(outs, singles))


@pytest.mark.parametrize("interp", ["nearest", "bilinear"])
@pytest.mark.parametrize("name", ["E_pano_eac28", "E_eac_pano_rot"])
def test_a_rotation_track_equals_single_faithful_plans_of_each_frame_s_chain(name, interp):
    case = ec.case_by_name(name)
    frames = np.stack([ec.case_frame(case, frame=f) for f in range(4)])
    track = [pb.Rotation(rad(4.0 * f), rad(-9.0 * f + 1), rad(2.5 * f)) for f in range(4)]
    plan = _private_plan(case)
    got = plan.remap_track(torch.from_numpy(frames).cuda(), track, interpolation=interp).cpu().numpy()
    src, cmap = ec.pb_chain(case, image=frames[0])
    streamed = list(pb.batch.remap_frames(plan, list(frames), interpolation=interp, rotations=track))
    for f in range(4):
        single = nat.Plan(cmap.dst_proj, list(cmap.rotations) + [track[f].rotation_matrix], src._proj("src"), defer=True)
        single.set_mode(nat.MODE_FAITHFUL)
        want = single.remap(torch.from_numpy(frames[f]).cuda(), interpolation=interp).cpu().numpy()
        assert _n_diff(got[f], want) == 0 and _n_diff(np.asarray(streamed[f]), want) == 0, (name, interp, f)
        if interp == "nearest":  # ... which is the definition's chain of that frame
            chain = Case("t", case.dst, case.src, list(case.rotations))
            with np.errstate(all="ignore"):
                m = orc.rotate_map(np.asarray(track[f].rotation_matrix, np.float64), ec.ref_stages(chain)[-1])
                assert _n_diff(got[f], ec.ref_remap(case, frames[f], m)) == 0, (name, f)


# ---- blobs, the C ABI, the CLI ------------------------------------------------------------------------------------------------------------------
def test_a_cube_blob_and_an_equiangular_blob_refuse_each_other_s_request():
    for case in ec.mid_cases():
        src, cmap = ec.pb_chain(case, image=np.zeros((case.src[1], case.src[2], 3), np.uint8))
        dst_p, src_p = cmap.dst_proj, src._proj("src")
        flip = lambda p: nat.make_proj({nat.KIND_CUBE: nat.KIND_EAC, nat.KIND_EAC: nat.KIND_CUBE}.get(p.kind, p.kind), p.height, p.width)  # noqa: E731
        plan, twin = nat.Plan(dst_p, cmap.rotations, src_p), nat.Plan(flip(dst_p), cmap.rotations, flip(src_p))
        blob, twin_blob = plan.serialize(), twin.serialize()
        assert len(blob) > 0 and len(twin_blob) > 0
        back = nat.Plan.deserialize(blob, dst_p, cmap.rotations, src_p)
        dev = torch.from_numpy(ec.case_frame(case)).cuda()
        assert back.info()["fast_path"] and torch.equal(back.remap(dev), plan.remap(dev))
        with pytest.raises(nat.PbError):
            nat.Plan.deserialize(blob, flip(dst_p), cmap.rotations, flip(src_p))
        with pytest.raises(nat.PbError):
            nat.Plan.deserialize(twin_blob, dst_p, cmap.rotations, src_p)
        assert int((twin.remap(dev) != plan.remap(dev)).sum()) > 0  # (the two mappings are different images)


def test_c_abi_equiangular_projections():
    """What a C host does: kind 8, height = 2N and width = 3N; everything else in the pb_proj is ignored; a wrong shape is PB_ERR_INVALID."""
    lib = nat.load()
    n = 40
    dst = nat.make_proj(nat.KIND_EAC, 2 * n, 3 * n, 77, 9.0, 9.0, 9.0)
    m = torch.empty((2 * n, 3 * n, 3), dtype=torch.float64, device="cuda")
    assert lib.pb_coordmap_f64(ctypes.byref(dst), m.data_ptr(), None) == 0
    torch.cuda.synchronize()
    with np.errstate(all="ignore"):
        want_map = er.coordinate_map(n)
    assert _same_bits(m.cpu().numpy(), want_map)
    rots = [pb.Rotation(rad(5.0 * k), rad(-7.0 * k), rad(3.0 * k + 1)).rotation_matrix for k in range(1, nat.PB_MAX_ROTATIONS + 1)]
    final = want_map
    with np.errstate(all="ignore"):
        for R in rots:
            final = orc.rotate_map(np.asarray(R, np.float64), final)
    src = nat.make_proj(nat.KIND_EAC, 64, 96)
    frame = synth_frame(64, 96, frame=2, seed=0)
    with np.errstate(all="ignore"):
        want, widx = er.sample(frame, np.copy(final)), er.source_index(32, np.copy(final))
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
    dm = torch.from_numpy(final.copy()).cuda()  # the map-stage calls with such a source
    s, o = torch.from_numpy(frame).cuda(), torch.zeros((2 * n, 3 * n, 3), dtype=torch.uint8, device="cuda")
    idx = torch.empty((2 * n, 3 * n), dtype=torch.int32, device="cuda")
    assert lib.pb_sample_map_u8(ctypes.byref(src), dm.data_ptr(), 2 * n, 3 * n, s.data_ptr(), o.data_ptr(), None) == 0
    assert lib.pb_index_from_map_i32(ctypes.byref(src), dm.data_ptr(), 2 * n, 3 * n, None, None, idx.data_ptr(), None, None) == 0
    torch.cuda.synchronize()
    assert np.array_equal(o.cpu().numpy(), want) and np.array_equal(idx.cpu().numpy(), widx) and _same_bits(dm.cpu().numpy(), final)
    bad = nat.make_proj(nat.KIND_EAC, 2 * n, 3 * n + 1)
    plan = ctypes.c_void_p()
    assert lib.pb_plan_create_ex(ctypes.byref(bad), None, 0, ctypes.byref(src), 0, 0, ctypes.byref(plan)) == -1 and b"(2N, 3N)" in lib.pb_last_error()
    assert lib.pb_coordmap_f64(ctypes.byref(bad), m.data_ptr(), None) == -1


def test_the_three_cli_commands_equal_the_api(tmp_path):
    pano_img = synth_frame(64, 128, frame=5, seed=0)
    inp, out = tmp_path / "pano.png", tmp_path / "eac.png"
    Image.fromarray(pano_img).save(inp)
    run = lambda *a: CliRunner().invoke(cli.main, list(a))  # noqa: E731
    res = run("pano-to-cubemap", str(inp), "--mapping", "equiangular", "-r", "15", "-40", "5", str(out))
    assert res.exit_code == 0, (res.output, res.exception)
    got = np.asarray(Image.open(out))
    case = Case("cli", eac(32), pano(64, 128), [(15, -40, 5)])
    with np.errstate(all="ignore"):
        assert got.shape == (64, 96, 3) and np.array_equal(got, ec.ref_remap(case, pano_img))
    plain = tmp_path / "cube.png"  # the default mapping is the plain cube's
    assert run("pano-to-cubemap", str(inp), "-r", "15", "-40", "5", str(plain)).exit_code == 0
    with np.errstate(all="ignore"):
        assert np.array_equal(np.asarray(Image.open(plain)), ec.ref_remap(Case("cli", cube(32), pano(64, 128), [(15, -40, 5)]), pano_img))
    # the way back, with a size, a sampler and supersampling
    back = tmp_path / "back.png"
    res = run("cubemap-to-pano", str(out), "--mapping", "equiangular", "--height", "40", "--supersample", "2", "--interpolation", "bilinear", str(back))
    assert res.exit_code == 0, (res.output, res.exception)
    cm = pb.PanoramaImage(np.zeros((40, 80, 3), np.uint8)).get_coordinate_map(supersample=2)
    want = pb.CubemapImage(got, mapping="equiangular").process_coordinate_map(cm, interpolation="bilinear")
    assert np.array_equal(np.asarray(Image.open(back)), want) and want.shape == (40, 80, 3)
    with np.errstate(all="ignore"):
        full = er.remap_bilinear(got, orc.coordinate_map(orc.Proj("pano", 80, 160)))
    assert np.array_equal(want, ss_ref.block_mean(full, 2))
    # cubemap-to-cubemap: the two classes chained - a conversion, a re-orientation with another face size
    conv = tmp_path / "conv.png"
    res = run("cubemap-to-cubemap", str(out), "--input-mapping", "equiangular", "--output-mapping", "gnomonic", str(conv))
    assert res.exit_code == 0, (res.output, res.exception)
    want = pb.CubemapImage(got, mapping="equiangular").process_coordinate_map(pb.CubemapImage(np.zeros((64, 96, 3), np.uint8)).get_coordinate_map())
    assert np.array_equal(np.asarray(Image.open(conv)), want)
    with np.errstate(all="ignore"):
        assert np.array_equal(want, ec.ref_remap(Case("c", cube(32), eac(32)), got))
    turn = tmp_path / "turn.png"
    res = run("cubemap-to-cubemap", str(conv), "--output-mapping", "equiangular", "--face-size", "24", "-r", "0", "90", "0", "--interpolation", "catmull-rom", str(turn))
    assert res.exit_code == 0, (res.output, res.exception)
    cm = pb.Rotation(0.0, rad(90), 0.0).rotate_coordinate_map(pb.CubemapImage(np.zeros((48, 72, 3), np.uint8), mapping="equiangular").get_coordinate_map())
    assert np.array_equal(np.asarray(Image.open(turn)), pb.CubemapImage(want).process_coordinate_map(cm, interpolation="catmull-rom"))
