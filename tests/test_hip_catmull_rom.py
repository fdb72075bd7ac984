"""The opt-in Catmull-Rom mode on the device, against its written definition (tests/catmull_rom_ref.py; the reference has no
such mode).  The float64 kernels - the map kernel (pb_sample_map_catmull_rom_px) and the plan's float64 routes (PB_MODE_FAITHFUL, double
fisheye sources) - evaluate the definition's own expressions on the reference's coordinate bits: EQUAL, asserted wherever the live NumPy is
the goldens' (tests/helpers.py), 1 LSB elsewhere, like tests/test_hip_bilinear_map.py.  The tile kernel evaluates float32 coordinate models
certified to 1/1024 px and sums in float32: within 1 LSB on every pixel; black in one result and sampled in the other nowhere at full size
and, on the small and mid cases, only on a black rim (`_within_one`)."""

import numpy as np
import pytest
import torch
from click.testing import CliRunner
from PIL import Image

import photonbend_amd as pb
import photonbend_amd.batch  # noqa: F401  (pb.batch)
from oracle.synth import synth_frame, synth_image
from photonbend_amd import _native as nat
from photonbend_amd.scripts import cli
from tests import cases as tc
from tests import catmull_rom_ref as cr
from tests import helpers as H

pytestmark = pytest.mark.gpu
SMALL = tc.small_cases()
GENERIC = tc.generic_cases()
CR = "catmull-rom"


def _chain(case):
    cmap = H.pb_obj(case.dst).get_coordinate_map()
    for rot in case.rotations:
        cmap = pb.Rotation(*map(pb.utils.to_radians, rot)).rotate_coordinate_map(cmap)
    return cmap


def _oracle_map(case):
    from oracle import reference_path as orc

    m = orc.coordinate_map(H.orc_proj(case.dst))
    for rot in H.orc_rots(case):
        m = orc.rotate_map(orc.rotation_matrix(*rot), m)
    return m


def _want(case, img, cmap=None):
    return cr.remap(H.orc_proj(case.dst), H.orc_proj(case.src), img, H.orc_rots(case), cmap=cmap)


def _diff(got, want, double_src):
    d = np.abs(got.astype(np.int64) - want.astype(np.int64))
    if double_src:
        d = np.minimum(d, 256 - d)  # the blend's cast wraps mod 256 like the reference's
    return d


def _exact(got, want, double_src, name):
    assert got.shape == want.shape and got.dtype == want.dtype, (name, got.shape, got.dtype, want.shape, want.dtype)
    d = _diff(got, want, double_src)
    assert int(d.max(initial=0)) <= 1, f"{name}: {int((d > 1).sum())} samples beyond 1 LSB of the definition (max {int(d.max())})"
    if H.live_numpy_is_the_goldens_numpy():
        assert int((d != 0).sum()) == 0, f"{name}: {int((d != 0).sum())} samples differ from the float64 definition"


def _rim_of(black):
    """one pixel either side of a black / sampled edge of the definition's output (8-neighbourhood)"""
    rim = np.zeros_like(black)
    for dy, dx in ((0, 1), (1, 0), (0, -1), (-1, 0), (1, 1), (1, -1), (-1, 1), (-1, -1)):
        rim |= black != np.roll(np.roll(black, dy, axis=0), dx, axis=1)
    return rim


def _within_one(got, want, double_src, name, rim_flips=0):
    """No pixel beyond 1 LSB; no pixel black in one result and sampled in the other - except, up to `rim_flips` of them, on a black rim of
    the definition's output: the tile kernel takes its black / sampled decision from the bilinear mode's tile classes, whose models are
    certified to 1/1024 px, and a camera source's coordinate within that reach of the image's edge (f = -1e-5: live in the nearest mode,
    black in the interpolating modes' definition) can land either way (M_pano_thoby: one pixel of 1.2 M)."""
    assert got.shape == want.shape, name
    d = _diff(got, want, double_src).reshape(got.shape[0], got.shape[1], -1).max(axis=2)
    bw = (want.reshape(d.shape + (-1,)) == 0).all(axis=2)
    flips = (got.reshape(d.shape + (-1,)) == 0).all(axis=2) != bw
    off = d > 1
    assert int(off.sum()) == 0, f"{name}: {int(off.sum())} pixels beyond 1 LSB (max {int(d.max())}; {int((off & flips).sum())} of them flips)"
    assert int(flips.sum()) <= rim_flips and not (flips & ~_rim_of(bw)).any(), f"{name}: {int(flips.sum())} pixels black in one result and sampled in the other"
    return float((d > 0).mean())


# ---- the float64 kernels: the definition, to the bit -------------------------------------------------------------------------------
@pytest.mark.parametrize("case", SMALL, ids=lambda c: c.name)
def test_map_kernel_small_cases(case):
    frame = synth_frame(case.src[1], case.src[2], frame=0, seed=0, circle_mask=case.mask)
    host_map = np.array(np.asarray(_chain(case)))
    got = H.pb_obj(case.src, frame).process_coordinate_map(host_map, interpolation=CR)
    assert isinstance(got, np.ndarray)
    _exact(got, _want(case, frame), case.src[0] == "double", case.name)


@pytest.mark.parametrize("case", SMALL, ids=lambda c: c.name)
def test_float64_route_small_cases(case):
    """PB_MODE_FAITHFUL: the plan's float64 route (pb_interp_fix_kernel / pb_interp_double_kernel with the PbCatmullRom filter) from the device chain."""
    frame = synth_frame(case.src[1], case.src[2], frame=0, seed=0, circle_mask=case.mask)
    plan = H.pb_plan_private(case)
    plan.set_mode(nat.MODE_FAITHFUL)
    got = plan.remap(torch.from_numpy(frame).cuda(), interpolation=CR).cpu().numpy()
    _exact(got, _want(case, frame), case.src[0] == "double", case.name)


@pytest.mark.parametrize("name,case,layout", GENERIC, ids=[c[0] for c in GENERIC])
def test_generic_images_and_custom_lenses(name, case, layout):
    _, h, w, *_ = case.src
    img = synth_image(h, w, layout, frame=3, circle_mask=case.mask)
    src = H.pb_obj(case.src, img)
    if case.src[0] == "double" and img.ndim == 2:
        with pytest.raises(ValueError, match="broadcast"):
            src.process_coordinate_map(_chain(case), interpolation=CR)
        return
    want = _want(case, img, cmap=_oracle_map(case))
    got = src.process_coordinate_map(_chain(case), interpolation=CR)
    custom = lambda p: p[0] != "pano" and p[3] in ("custom", "thobylike")
    if layout == "RGB" and not custom(case.src) and not custom(case.dst) and case.src[0] != "double":
        _within_one(got, want, False, name)  # (uint8 RGB + built-in lenses + a lazy map: the tile kernel)
        return
    if layout == "RGB" and case.src[0] == "double" and not custom(case.src) and not custom(case.dst):
        _exact(got, want, True, name)  # (the double float64 route)
        return
    _exact(got, want, case.src[0] == "double", name)


def test_edited_map():
    case = tc.Case("edit", tc.cam(96, 96, "equisolid", 190, tc.inscribed(96)), tc.pano(64, 128), [(10, 20, 30)])
    frame = synth_frame(64, 128, frame=2, seed=0)
    m = np.array(np.asarray(_chain(case)))
    m[10:20, 30:50, 2] = 1.0
    m[40:60, :, 1] *= -1.0
    m[70, 5:9, 0] = np.nan
    want_map = m.copy()
    want = cr.remap(None, H.orc_proj(case.src), frame, cmap=want_map)
    got = pb.PanoramaImage(frame).process_coordinate_map(m, interpolation=CR)
    _exact(got, want, False, "edited map")
    assert np.array_equal(m.view(np.uint64), want_map.view(np.uint64)), "the caller's map must carry the reference's in-place zeroing"


# ---- the tile kernel: within 1 LSB ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", SMALL + tc.mid_cases(), ids=lambda c: c.name)
def test_tile_kernel_within_one_lsb(case):
    frame = synth_frame(case.src[1], case.src[2], frame=0, seed=0, circle_mask=case.mask)
    plan = H.pb_plan_private(case)
    got = plan.remap(torch.from_numpy(frame).cuda(), interpolation=CR).cpu().numpy()
    share = _within_one(got, _want(case, frame), case.src[0] == "double", case.name, rim_flips=2)
    print(f"{case.name}: {100 * share:.3f} % of the pixels 1 LSB off")


@pytest.mark.parametrize("name", ["c1", "c2", "c3"])
def test_tile_kernel_against_float64_route_at_full_size(name):
    """Every pixel of c1, c2 and c3 on the noise frame (255 LSB per pixel of coordinate error): the tile kernel against the float64 route
    of the same plan (equal to the definition: the tests above)."""
    case = next(c for c in tc.full_cases() if c.name == name)
    plan = H.pb_plan_private(case)
    assert plan.info()["fast_path"]
    frame = nat.synth_frame(case.src[1], case.src[2], frame=0, seed=0, circle_mask=case.mask)
    got = plan.remap(frame, interpolation=CR)
    plan.set_mode(nat.MODE_FAITHFUL)
    want = plan.remap(frame, interpolation=CR)
    d = (got.to(torch.int16) - want.to(torch.int16)).abs().amax(dim=2)
    flips = (got == 0).all(dim=2) != (want == 0).all(dim=2)
    share = float((d > 0).float().mean())
    print(f"{name}: {100 * share:.3f} % of the pixels 1 LSB off")
    assert int((d > 1).sum()) == 0, f"{int((d > 1).sum())} pixels beyond 1 LSB (max {int(d.max())})"
    assert int(flips.sum()) == 0, f"{int(flips.sum())} pixels black in one result and sampled in the other"
    assert share <= 0.05


def test_magnification_is_sharper_than_bilinear():
    """What the mode is for: a fisheye unwrapped into a larger panorama.  On a smooth pattern, Catmull-Rom stays closer to the continuous
    image than bilinear."""
    case = tc.Case("mag", tc.pano(384, 768), tc.cam(96, 96, "equidistant", 180, tc.inscribed(96)))
    yy, xx = np.mgrid[0:96, 0:96]
    f = lambda y, x: 127.5 + 100.0 * np.sin(x * 0.55) * np.cos(y * 0.45)
    frame = np.rint(np.stack([f(yy + 0.5, xx + 0.5)] * 3, axis=2)).astype(np.uint8)
    src, cmap = H.pb_chain(case, frame)
    from oracle import reference_path as orc

    cm = orc.coordinate_map(H.orc_proj(case.dst))
    with np.errstate(all="ignore"):
        _, _, fy, fx = orc.camera_positions(H.orc_proj(case.src), 96, 96, cm[:, :, 0], cm[:, :, 1])
    truth = f(fy, fx)
    inner = np.isfinite(fy) & (fy > 3) & (fy < 93) & (fx > 3) & (fx < 93)
    errs = {}
    for mode in ("bilinear", CR):
        got = src.process_coordinate_map(cmap, interpolation=mode)[:, :, 0].astype(np.float64)
        errs[mode] = float(np.abs(got - truth)[inner].mean())
    assert errs[CR] < 0.8 * errs["bilinear"], errs


# ---- batches, strides, host paths and the CLI: the same bytes ------------------------------------------------------------------------
def test_batches_strides_and_host_paths_agree():
    case = tc.case_by_name("D_photo_rot")
    plan = H.pb_plan_private(case)
    h, w = case.src[1], case.src[2]
    frames = [synth_frame(h, w, frame=k, seed=1) for k in range(3)]
    one = [plan.remap(torch.from_numpy(f).cuda(), interpolation=CR).cpu().numpy() for f in frames]
    batch = plan.remap(torch.from_numpy(np.stack(frames)).cuda(), interpolation=CR).cpu().numpy()
    assert all(np.array_equal(batch[k], one[k]) for k in range(3))
    # strided frames: every frame padded by 48 bytes in one buffer, outputs too
    H_, W_ = case.dst[1], case.dst[2]
    ss, ds = h * w * 3 + 48, H_ * W_ * 3 + 48
    sbuf = torch.zeros(3 * ss, dtype=torch.uint8, device="cuda")
    for k, f in enumerate(frames):
        sbuf[k * ss : k * ss + f.size] = torch.from_numpy(f.reshape(-1)).cuda()
    dbuf = torch.zeros(3 * ds, dtype=torch.uint8, device="cuda")
    plan.launch(sbuf.data_ptr(), dbuf.data_ptr(), 3, None, CR, src_stride=ss, dst_stride=ds)
    torch.cuda.synchronize()
    for k in range(3):
        assert np.array_equal(dbuf[k * ds : k * ds + H_ * W_ * 3].cpu().numpy().reshape(H_, W_, 3), one[k])
    # ndarrays: the facade's host path, remap_frames (list and generator)
    src, cmap = H.pb_chain(case, frames[0])
    assert np.array_equal(src.process_coordinate_map(cmap, interpolation=CR), one[0])
    bplan = pb.batch.plan_for(H.pb_obj(case.dst), [pb.Rotation(*map(pb.utils.to_radians, r)) for r in case.rotations], H.pb_obj(case.src))
    outs = [np.array(o) for o in pb.batch.remap_frames(bplan, frames, interpolation=CR)]
    assert all(np.array_equal(outs[k], one[k]) for k in range(3))
    outs = [np.array(o) for o in pb.batch.remap_frames(bplan, iter(frames), interpolation=CR)]
    assert all(np.array_equal(outs[k], one[k]) for k in range(3))


@pytest.mark.parametrize("case", [c for c in tc.cli_cases() if c[0] in ("photo_rot2", "pano_double_195", "alter_eqd_eqs_rot", "photo_rgba", "alter_rgba_double_in")],
                         ids=lambda c: c[0])
def test_cli_equals_api(case, tmp_path):
    name, cmd, opts, spec = case
    h, w, mask, layout = (*spec, "RGB")[:4]
    inp, out = tmp_path / "in.png", tmp_path / "o.png"
    img = synth_image(h, w, layout, frame=5, circle_mask=mask)
    Image.fromarray(img).save(inp)
    seen = {}
    orig = cli.run_chain

    def spy(source, destiny, rotations, out, supersample=1, interpolation="nearest"):
        seen["args"] = (source, destiny, rotations, interpolation)
        return orig(source, destiny, rotations, out, supersample, interpolation)

    cli.run_chain = spy
    try:
        res = CliRunner().invoke(cli.main, [cmd, str(inp), *opts, "--interpolation", CR, str(out)])
    finally:
        cli.run_chain = orig
    assert res.exit_code == 0, (res.output, res.exception)
    source, destiny, rotations, interp = seen["args"]
    assert interp == CR
    cm = destiny.get_coordinate_map()
    for rot in rotations:
        cm = pb.Rotation(*map(pb.utils.to_radians, rot)).rotate_coordinate_map(cm)
    want = source.process_coordinate_map(cm, interpolation=CR)
    got = np.asarray(Image.open(out))
    assert got.shape == want.shape and np.array_equal(got, want)
    near = CliRunner().invoke(cli.main, [cmd, str(inp), *opts, str(tmp_path / "n.png")])
    assert near.exit_code == 0 and not np.array_equal(np.asarray(Image.open(tmp_path / "n.png")), got)
