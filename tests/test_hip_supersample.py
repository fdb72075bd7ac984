"""The supersampled mode on the GPU: against the live oracle (the n x destination's remap, block-averaged), the fused kernel
against the forced generic path at full size, and every route of the API (double sources, bilinear, grey / RGBA / 16-bit images, materialised
and edited maps, ndarray in / out, streamed batches, the CLI)."""

import numpy as np
import pytest
import torch
from click.testing import CliRunner
from PIL import Image

import photonbend_amd as pb
from oracle.synth import synth_frame, synth_image
from photonbend_amd import _native as nat
from photonbend_amd import batch
from photonbend_amd.core.projection import _plan_for
from photonbend_amd.scripts import cli
from tests import helpers as H
from tests import ss_ref
from tests.cases import Case, cam, full_cases, inscribed, mid_cases, pano, small_cases
from tests.test_hip_random import random_case

pytestmark = pytest.mark.gpu
rad = pb.utils.to_radians


def _chain(case, n, image):
    """(source object, lazy map of the n x destination with the case's rotations)."""
    dst = H.pb_obj(case.dst)
    cm = dst.get_coordinate_map(supersample=n)
    for rot in case.rotations:
        cm = pb.Rotation(*map(rad, rot)).rotate_coordinate_map(cm)
    return H.pb_obj(case.src, image), cm


def _ss_plan(case, n):
    src, cm = _chain(case, n, np.zeros((case.src[1], case.src[2], 3), np.uint8))
    plan = _plan_for(cm.dst_proj, cm.rotations, src._proj())
    plan.set_mode(nat.MODE_AUTO)
    return plan


def _workspace(plan, n, interp=0, flags=0):
    import ctypes

    need = ctypes.c_size_t()
    nat.check(nat.load().pb_remap_ss_workspace(plan.handle, n, interp, flags, ctypes.byref(need)))
    return need.value


def _assert_route(plan, n, dev):
    """The route of plan.remap(dev, supersample=n), asserted: a prepared single-source plan (info()["fast_path"]) takes the fused kernel -
    no workspace for this very frame - unless its packed frame size 3 h w is no multiple of 16: pb_check_frames fills the stride in with
    it, the plain route then is not the windowed kernel (pb_aligned16) and pb_route answers SS_GENERIC, one n x frame of workspace.
    Returns the workspace bytes; plans without a fast path (deferred ones, double-fisheye sources) are generic by design."""
    ws = plan.supersample_workspace_bytes(n, src_ptr=dev.data_ptr())
    if plan.double_src or not plan.info()["fast_path"]:
        return ws
    if (3 * plan.src.height * plan.src.width) % 16:
        assert ws == 3 * plan.dst.height * plan.dst.width and _workspace(plan, n) == 0
    else:
        assert ws == 0 and _workspace(plan, n) == 0, "a prepared single-source plan with 16-byte aligned frames must take SS_FUSED"
    return ws


def _check_oracle(got, want):
    if H.live_numpy_is_the_goldens_numpy():
        assert np.array_equal(got, want), f"{int((got != want).any(axis=-1).sum())} pixels differ from the oracle"
    else:  # another host's libm: the n x samples keep the fragile-set allowance of the plain tests, so a few means may move
        d = np.abs(got.astype(np.int32) - want.astype(np.int32))
        assert int((d > 0).any(axis=-1).sum()) <= max(4, got.shape[0] * got.shape[1] // 500)


SMALL = [c for c in small_cases()] + [
    Case("S_chain9", pano(24, 48), cam(40, 40, "equidistant", 360, inscribed(40)), [(10, 20, 30), (-5, 7, 1)] * 4 + [(1, 2, 3)], mask=1)
]


@pytest.mark.parametrize("n", [2, 4])
@pytest.mark.parametrize("case", SMALL, ids=lambda c: c.name)
def test_small_cases_match_oracle(case, n):
    frame = H.case_frame(case)
    want = ss_ref.reference(case, n, frame)
    src, cm = _chain(case, n, frame)
    got = src.process_coordinate_map(cm)  # ndarray in -> ndarray out (the facade: a deferred plan's first use)
    assert isinstance(got, np.ndarray) and got.shape == want.shape
    _check_oracle(got, want)
    if len(case.rotations) <= nat.PB_MAX_ROTATIONS:
        # the prepared n x plan on the device: the fused kernel where it takes the plan, and the forced generic path
        plan = _ss_plan(case, n)
        dev = torch.from_numpy(frame).cuda()
        _assert_route(plan, n, dev)
        fused = plan.remap(dev, supersample=n).cpu().numpy()
        generic = plan.remap(dev, supersample=n, generic=True).cpu().numpy()
        assert np.array_equal(fused, got) and np.array_equal(generic, got)


@pytest.mark.parametrize("case", mid_cases(), ids=lambda c: c.name)
def test_mid_cases_match_oracle(case):
    n = 2
    frame = H.case_frame(case)
    want = ss_ref.reference(case, n, frame)
    plan = _ss_plan(case, n)
    assert _workspace(plan, n) == 0  # prepared single-source plans take the fused kernel
    got = plan.remap(torch.from_numpy(frame).cuda(), supersample=n).cpu().numpy()
    _check_oracle(got, want)


RANDOM = [random_case(np.random.default_rng(5000 + k), k) for k in range(24)]


@pytest.mark.parametrize("case", RANDOM, ids=lambda c: f"{c.name}:{c.dst[0]}<-{c.src[0]}:r{len(c.rotations)}")
def test_random_geometries_match_oracle(case):
    n = (2, 4)[int(case.name[4:]) % 2]
    frame = synth_frame(case.src[1], case.src[2], frame=3)
    want = ss_ref.reference(case, n, frame)
    plan = _ss_plan(case, n)
    dev = torch.from_numpy(frame).cuda()
    _assert_route(plan, n, dev)
    got = plan.remap(dev, supersample=n).cpu().numpy()
    assert np.array_equal(got, plan.remap(dev, supersample=n, generic=True).cpu().numpy())
    _check_oracle(got, want)


@pytest.mark.parametrize("n", [2, 4])
@pytest.mark.parametrize("name", ["c1", "c2", "c3"])
def test_fused_equals_generic_at_full_size(name, n):
    case = next(c for c in full_cases() if c.name == name)
    plan = _ss_plan(case, n)
    assert _workspace(plan, n) == 0 and _workspace(plan, n, flags=nat.SS_GENERIC) == 3 * plan.dst.height * plan.dst.width
    frames = torch.stack([nat.synth_frame(case.src[1], case.src[2], frame=k, circle_mask=case.mask) for k in range(3)])
    oh, ow = plan.out_shape(n)
    one = plan.remap(frames[0], supersample=n)
    assert tuple(one.shape) == (oh, ow, 3)
    assert torch.equal(one, plan.remap(frames[0], supersample=n, generic=True))
    many = plan.remap(frames, supersample=n)  # one launch for the batch
    assert torch.equal(many, plan.remap(frames, supersample=n, generic=True))
    assert torch.equal(many[0], one) and not torch.equal(many[1], many[2])
    # and the generic path is the block mean of the plain n x remap
    assert torch.equal(one, ss_ref.block_mean_torch(plan.remap(frames[0]), n))


@pytest.mark.parametrize("name", ["c5_180", "c5_195"])
def test_double_source_full_size(name):
    n = 2
    case = next(c for c in full_cases() if c.name == name)
    plan = _ss_plan(case, n)
    assert _workspace(plan, n) == 3 * plan.dst.height * plan.dst.width  # double-fisheye sources: the generic path
    frame = nat.synth_frame(case.src[1], case.src[2], frame=1, circle_mask=case.mask)
    got = plan.remap(frame, supersample=n)
    assert torch.equal(got, ss_ref.block_mean_torch(plan.remap(frame), n))


@pytest.mark.parametrize("n", [2, 4])
@pytest.mark.parametrize("name", ["A_photo_odd", "C_alter_ste_ort", "E_stitch_195_masked", "E_double_dst", "D_pano_chain"])
def test_bilinear_is_the_block_mean_of_bilinear(name, n):
    case = next(c for c in small_cases() if c.name == name)
    frame = H.case_frame(case)
    src, cm = _chain(case, n, frame)
    full = src.process_coordinate_map(cm, interpolation="bilinear", supersample=1)
    got = src.process_coordinate_map(cm, interpolation="bilinear")
    assert np.array_equal(got, ss_ref.block_mean(full, n))
    plan = _ss_plan(case, n)
    dev = torch.from_numpy(frame).cuda()
    assert np.array_equal(plan.remap(dev, interpolation="bilinear", supersample=n).cpu().numpy(), got)


def _layouts(h, w):
    rgb = synth_frame(h, w, frame=2)
    grey = rgb[..., 1].copy()
    rgba = np.concatenate([rgb, rgb[..., :1] ^ 0x5A], axis=2)
    u16 = rgb.astype(np.uint16) * 257 + np.arange(h * w * 3, dtype=np.uint16).reshape(h, w, 3) % 251
    return {"grey": grey, "rgba": rgba, "u16": u16, "grey16": u16[..., 0].copy()}


@pytest.mark.parametrize("interp", ["nearest", "bilinear"])
@pytest.mark.parametrize("name", ["A_photo_odd", "C_alter_rect_thoby", "E_stitch_195_raw"])
def test_other_sample_layouts(name, interp):
    case = next(c for c in small_cases() if c.name == name)
    n = 2
    for lname, img in _layouts(case.src[1], case.src[2]).items():
        if case.src[0] == "double" and img.ndim == 2:
            continue  # (the reference's blend cannot broadcast grey samples either)
        src, cm = _chain(case, n, img)
        full = src.process_coordinate_map(cm, interpolation=interp, supersample=1)
        got = src.process_coordinate_map(cm, interpolation=interp)
        assert got.dtype == full.dtype and np.array_equal(got, ss_ref.block_mean(full, n)), lname
        t = torch.from_numpy(img).cuda()
        src_t, cm_t = _chain(case, n, t)
        assert np.array_equal(src_t.process_coordinate_map(cm_t, interpolation=interp).cpu().numpy(), got), lname


@pytest.mark.parametrize("n", [2, 4])
def test_materialised_and_edited_map(n):
    case = next(c for c in small_cases() if c.name == "D_photo_rot")
    frame = H.case_frame(case)
    src, cm = _chain(case, n, frame)
    arr = np.array(np.asarray(cm))  # materialised: leaves the rotation as a plain ndarray, without its factor
    arr[: 3 * n, :, 1] += 0.25  # edited
    arr[5 * n : 6 * n, 2:7, 2] = 1.0
    full = src.process_coordinate_map(arr.copy())
    got = src.process_coordinate_map(arr.copy(), supersample=n)
    assert got.shape == (case.dst[1], case.dst[2], 3) and np.array_equal(got, ss_ref.block_mean(full, n))
    dmap = torch.from_numpy(arr.copy()).cuda()
    assert np.array_equal(src.process_coordinate_map(dmap, supersample=n), got)
    # a pano source zeroes invalid lat / lon in the caller's map, as the n = 1 call does
    a1, a2 = arr.copy(), arr.copy()
    p = pb.PanoramaImage(frame)
    p.process_coordinate_map(a1)
    p.process_coordinate_map(a2, supersample=n)
    assert np.array_equal(H.bits(a1), H.bits(a2))


def test_supersample_one_is_byte_identical():
    case = next(c for c in small_cases() if c.name == "D_photo_rot")
    frame = H.case_frame(case)
    for kw in ({}, {"interpolation": "bilinear"}):
        src, cm = _chain(case, 1, frame)
        a = src.process_coordinate_map(cm, **kw)
        src, cm = _chain(case, 1, frame)
        b = src.process_coordinate_map(cm, supersample=1, **kw)
        assert np.array_equal(a, b)
    plan = _ss_plan(case, 1)
    dev = torch.from_numpy(frame).cuda()
    assert torch.equal(plan.remap(dev), plan.remap(dev, supersample=1))


@pytest.mark.parametrize("n", [2, 4])
def test_ndarray_and_streamed_batches_equal_the_device_path(n):
    case = next(c for c in full_cases() if c.name == "c1")
    dst, src = H.pb_obj(case.dst), H.pb_obj(case.src, np.zeros((case.src[1], case.src[2], 3), np.uint8))
    plan = batch.plan_for(dst, [pb.Rotation(0.1, 0.2, 0.3)], src, supersample=n)
    frames = [synth_frame(case.src[1], case.src[2], frame=k, circle_mask=case.mask) for k in range(3)]
    want = [plan.remap(torch.from_numpy(f).cuda(), supersample=n).cpu().numpy() for f in frames]
    got = list(batch.remap_frames(plan, frames, supersample=n))
    assert all(np.array_equal(g, w) for g, w in zip(got, want))
    cm = pb.Rotation(0.1, 0.2, 0.3).rotate_coordinate_map(dst.get_coordinate_map(supersample=n))
    out = pb.CameraImage(frames[1], src.fov, pb.equidistant(), magnitude=src.magnitude).process_coordinate_map(cm)
    assert isinstance(out, np.ndarray) and np.array_equal(out, want[1])


@pytest.mark.parametrize("case", [c for c in __import__("tests.cases", fromlist=["cli_cases"]).cli_cases()
                                  if c[0] in ("photo_rot2", "pano_double_195", "alter_eqd_eqs_rot", "photo_rgba")], ids=lambda c: c[0])
def test_cli_supersample_equals_api(case, tmp_path):
    name, cmd, opts, spec = case
    h, w, mask, layout = (*spec, "RGB")[:4]
    inp, o1, o2 = tmp_path / "in.png", tmp_path / "a.png", tmp_path / "b.png"
    img = synth_image(h, w, layout, frame=5, circle_mask=mask)
    Image.fromarray(img).save(inp)
    res = CliRunner().invoke(cli.main, [cmd, str(inp), *opts, "--supersample", "2", str(o2)])
    assert res.exit_code == 0, (res.output, res.exception)
    got = np.asarray(Image.open(o2))
    # the API: the same objects the CLI builds, at n = 2
    orig = cli.run_chain
    seen = {}

    def spy(source, destiny, rotations, out, supersample=1):
        seen["args"] = (source, destiny, rotations)
        return orig(source, destiny, rotations, out, supersample)

    cli.run_chain = spy
    try:
        res = CliRunner().invoke(cli.main, [cmd, str(inp), *opts, str(o1)])
    finally:
        cli.run_chain = orig
    assert res.exit_code == 0
    source, destiny, rotations = seen["args"]
    cm = destiny.get_coordinate_map(supersample=2)
    for rot in rotations:
        cm = pb.Rotation(*map(rad, rot)).rotate_coordinate_map(cm)
    want = source.process_coordinate_map(cm)
    assert got.shape == np.asarray(Image.open(o1)).shape and np.array_equal(got, want)


def test_streamed_generic_route_keeps_no_workspace_per_call():
    """remap_frames on a double-fisheye source (the generic path: an n x workspace per call) many times: the workspace is the host
    pipeline's, checked out for the call and returned - device memory does not grow with the number of calls (each call makes fresh
    streams)."""
    from photonbend_amd import _hostpipe

    n = 2
    dst = pb.PanoramaImage(np.zeros((1024, 2048, 3), np.uint8))
    src = pb.DoubleCameraImage(np.zeros((972, 1944, 3), np.uint8), rad(195), pb.equidistant())
    plan = batch.plan_for(dst, [], src, supersample=n)
    frames = [synth_frame(972, 1944, frame=k, circle_mask=2) for k in range(2)]
    ws_bytes = plan.supersample_workspace_bytes(n)
    assert ws_bytes == 3 * 2048 * 4096  # the generic path
    want = [plan.remap(torch.from_numpy(f).cuda(), supersample=n).cpu().numpy() for f in frames]
    for interp in ("nearest", "bilinear"):  # (bilinear: the plan's tables are built on first use, before memory is measured)
        list(batch.remap_frames(plan, frames, supersample=n, interpolation=interp))
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    for _ in range(6):
        got = list(batch.remap_frames(plan, frames, supersample=n))
        assert all(np.array_equal(g, w) for g, w in zip(got, want))
        for interp in ("nearest", "bilinear"):
            assert src.process_coordinate_map(dst.get_coordinate_map(supersample=n), interpolation=interp).shape == (1024, 2048, 3)
    torch.cuda.synchronize()
    pipe = _hostpipe.pipe_for(torch.cuda.current_device())
    assert pipe._ws_idle is not None and pipe._ws_idle.nbytes >= ws_bytes
    grown = free0 - torch.cuda.mem_get_info()[0]
    assert grown < ws_bytes, f"device memory grew by {grown} bytes over 6 streamed calls (one workspace is {ws_bytes})"


def test_caller_owned_workspace():
    case = next(c for c in full_cases() if c.name == "c1")
    n = 2
    plan = _ss_plan(case, n)
    frame = nat.synth_frame(case.src[1], case.src[2], frame=2, circle_mask=case.mask)
    need = plan.supersample_workspace_bytes(n, generic=True)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    got = plan.remap(frame, supersample=n, generic=True, workspace=ws)
    assert torch.equal(got, plan.remap(frame, supersample=n))
    with pytest.raises(nat.PbError):
        plan.remap(frame, supersample=n, generic=True, workspace=ws[: need // 2])
