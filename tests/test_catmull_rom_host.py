"""CPU checks of the opt-in Catmull-Rom mode: properties of the test-side definition (tests/catmull_rom_ref.py), the C ABI's
new entries and their argument checks, and the refusals the Python API and the CLI make before anything needs a GPU."""

import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
from click.testing import CliRunner
from PIL import Image

import photonbend_amd as pb
import photonbend_amd.batch  # noqa: F401  (pb.batch)
from oracle import reference_path as orc
from photonbend_amd import _native as nat
from photonbend_amd.build import LIB_PATH
from photonbend_amd.scripts import cli
from tests import catmull_rom_ref as cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
rad = pb.utils.to_radians
NEW = ("pb_remap_catmull_rom_u8", "pb_sample_map_catmull_rom_px")


# ---- the definition -------------------------------------------------------------------------------------------------------------
def test_weights_at_zero_and_partition_of_unity():
    w = cr.weights(np.float64(0.0))
    assert [float(x) for x in w] == [0.0, 1.0, 0.0, 0.0]
    t = np.linspace(0.0, 1.0, 1001)
    assert np.allclose(sum(cr.weights(t)), 1.0, atol=1e-15)
    # the bound the precision budget uses: sum |w| <= 1.25 and sum |w'| <= 3, both reached at t = 1/2
    assert np.isclose(np.abs(np.stack(cr.weights(t))).sum(axis=0).max(), 1.25)
    d = (np.stack(cr.weights(t + 1e-7)) - np.stack(cr.weights(t - 1e-7))) / 2e-7
    assert np.abs(d).sum(axis=0).max() <= 3.0 + 1e-6


def _img(h, w, c=3, seed=0, dt=np.uint8):
    return np.random.default_rng(seed).integers(0, np.iinfo(dt).max + 1, size=(h, w, c)).astype(dt)


@pytest.mark.parametrize("wrap", [False, True])
def test_texel_centres_return_the_texel(wrap):
    img = _img(7, 9)
    yy, xx = np.mgrid[0:7, 0:9]
    got = cr.sample(img, yy + 0.5, xx + 0.5, np.ones((7, 9), bool), wrap)
    assert np.array_equal(got, img)


@pytest.mark.parametrize("dt", [np.uint8, np.uint16])
def test_constant_stays_constant(dt):
    img = np.full((6, 10, 2), 201, dt)
    rng = np.random.default_rng(1)
    fy, fx = rng.uniform(-1, 7, (50, 50)), rng.uniform(-2, 12, (50, 50))
    for wrap in (False, True):
        assert (cr.sample(img, fy, fx, np.ones(fy.shape, bool), wrap) == 201).all()


def test_ramp_is_reproduced():
    """A linear ramp in x and y (far from the edges, where clamping bends it) comes back to within rounding."""
    h, w = 40, 60
    yy, xx = np.mgrid[0:h, 0:w]
    img = np.stack([2 * xx + 10, 3 * yy + 5, xx + yy], axis=2).astype(np.uint8)
    rng = np.random.default_rng(2)
    fy, fx = rng.uniform(3, h - 3, 500), rng.uniform(3, w - 3, 500)
    got = cr.sample(img, fy, fx, np.ones(500, bool), False).astype(np.float64)
    sy, sx = fy - 0.5, fx - 0.5
    want = np.stack([2 * sx + 10, 3 * sy + 5, sx + sy], axis=1)
    assert np.abs(got - want).max() <= 1.0


def test_overshoot_is_clipped():
    img = np.zeros((4, 8, 1), np.uint8)
    img[:, 4:] = 255  # a step: the cubic rings on both sides
    fy = np.full(40, 2.0)
    fx = np.linspace(2.0, 6.0, 40)
    v = cr.sample(img, fy, fx, np.ones(40, bool), False)[:, 0].astype(int)
    assert v.min() == 0 and v.max() == 255 and (np.diff(v) >= 0).all()


def test_panorama_columns_wrap():
    """At a panorama's seam the taps of columns -1 and w come from the other side of the frame."""
    img = _img(5, 8, seed=3)
    fy, fx = np.array([2.5, 2.5, 2.7]), np.array([0.5 + 0.25, 0.2, 7.9])
    got = cr.sample(img, fy, fx, np.ones(3, bool), True).astype(np.float64)
    for n in range(3):
        sy, sx = fy[n] - 0.5, fx[n] - 0.5
        i0, j0 = int(np.floor(sy)), int(np.floor(sx))
        wy, wx = cr.weights(sy - i0), cr.weights(sx - j0)
        v = 0.0
        for k in range(4):
            r = min(max(i0 - 1 + k, 0), 4)
            v += wy[k] * sum(wx[l] * img[r, (j0 - 1 + l) % 8].astype(np.float64) for l in range(4))
        assert np.abs(np.clip(np.rint(v), 0, 255) - got[n]).max() <= 1e-9


def test_eyes_clamp_to_their_own_half():
    """A double fisheye: an eye's taps stay in its own half (the right one mirrored), so repainting one half changes no pixel that only the
    other eye samples - the pixels next to the halves' shared edge included, whose 4 x 4 footprint would cross it unclamped."""
    h, w = 24, 48
    src = orc.Proj("double", h, w, "equidistant", orc.to_radians(200.0))
    dst = orc.Proj("pano", 32, 64)
    left, right, w2 = orc._double_sides(src)
    cm = orc.coordinate_map(dst)
    _, _, lat_r = orc.double_weights(src, cm[:, :, 0])
    base = _img(h, w, seed=4)
    a = cr.remap(dst, src, base)
    for eye, lat, half in ((right, lat_r, np.s_[:, w2:]), (left, cm[:, :, 0], np.s_[:, :w2])):
        with np.errstate(all="ignore"):
            _, _, fy, fx = orc.camera_positions(eye, h, eye.width, lat, cm[:, :, 1])
            dead = ~(np.isfinite(fy) & np.isfinite(fx) & (fy >= 0) & (fy < h) & (fx >= 0) & (fx < eye.width))
        other = base.copy()
        other[half] = _img(h, w, seed=5)[half]
        b = cr.remap(dst, src, other)
        assert np.array_equal(a[dead], b[dead]) and not np.array_equal(a, b)


def test_grey_image_is_its_single_channel():
    img = _img(20, 40, c=1, seed=5)
    dst = orc.Proj("camera", 16, 16, "equidistant", orc.to_radians(180), None)
    src = orc.Proj("pano", 20, 40)
    assert np.array_equal(cr.remap(dst, src, img[:, :, 0]), cr.remap(dst, src, img)[:, :, 0])


def test_black_where_bilinear_is_black():
    img = np.full((30, 30, 3), 200, np.uint8)
    dst = orc.Proj("camera", 24, 24, "equisolid", orc.to_radians(190), 10.0)
    src = orc.Proj("camera", 30, 30, "equidistant", orc.to_radians(120), None)
    a, b = cr.remap(dst, src, img), orc.remap_bilinear(dst, src, img)
    assert np.array_equal((a == 0).all(axis=2), (b == 0).all(axis=2))
    assert (a[(b != 0).any(axis=2)] == 200).all()  # (a constant image: the samples are the constant)


# ---- C ABI --------------------------------------------------------------------------------------------------------------------------
def test_new_symbols_exported_and_declared():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "photonbend_hip.h")).read(), flags=re.S)
    lib = ctypes.CDLL(LIB_PATH)
    for name in NEW:
        assert re.search(rf"\b{name}\s*\(", text), name
        assert hasattr(lib, name) and name in nat.SIGNATURES, name
    assert nat.load().pb_abi_version() == nat.ABI_VERSION == 5
    nm = subprocess.run(["nm", "-D", "--defined-only", LIB_PATH], capture_output=True, text=True)
    if nm.returncode == 0:
        for name in NEW:
            assert re.search(rf"\bT {name}$", nm.stdout, re.M), name


def test_remap_refuses_like_bilinear_on_a_deferred_plan():
    lib = nat.load()
    V = ctypes.c_void_p
    dst = nat.make_proj(nat.KIND_CAMERA, 6, 10, 0, rad(180), 3.0, 3.0 / rad(90))
    plan = nat.Plan(dst, [], nat.make_proj(nat.KIND_PANO, 16, 32), defer=True)
    for args in ((V(16), None, 1), (None, V(16), 1), (V(16), V(16), -1)):
        assert lib.pb_remap_bilinear_u8(plan.handle, *args, 0, 0, None) == -1
        want = lib.pb_last_error().decode()
        assert lib.pb_remap_catmull_rom_u8(plan.handle, *args, 0, 0, None) == -1
        assert lib.pb_last_error().decode() == want, args
    assert "negative frame count" in want
    assert lib.pb_remap_catmull_rom_u8(None, V(16), V(16), 1, 0, 0, None) == -1
    assert lib.pb_remap_catmull_rom_u8(plan.handle, V(16), V(16), 0, 0, 0, None) == 0  # nothing to do
    assert lib.pb_remap_catmull_rom_u8(plan.handle, V(16), V(16), 2, 0, 5, None) == -1  # dst stride below a frame
    assert "dst_frame_stride" in lib.pb_last_error().decode()


def test_map_entry_refuses_like_bilinear():
    lib = nat.load()
    V = ctypes.c_void_p
    pano = nat.make_proj(nat.KIND_PANO, 16, 32)
    cam = nat.make_proj(nat.KIND_CAMERA, 16, 16, nat.LENS_CUSTOM, rad(180), 8.0, 8.0 / rad(90))
    cases = [(pano, None, 4, 4, V(16), V(16), 3, 1), (pano, V(16), 0, 4, V(16), V(16), 3, 1), (pano, V(16), 4, 4, V(16), V(16), 17, 1),
             (pano, V(16), 4, 4, V(16), V(16), 3, 4), (cam, V(16), 4, 4, V(16), V(16), 3, 1)]
    for src, m, hh, ww, img, out, ch, sb in cases:
        assert lib.pb_sample_map_bilinear_px(ctypes.byref(src), m, hh, ww, None, None, img, out, ch, sb, None) == -1
        want = lib.pb_last_error().decode()
        assert lib.pb_sample_map_catmull_rom_px(ctypes.byref(src), m, hh, ww, None, None, img, out, ch, sb, None) == -1
        assert lib.pb_last_error().decode() == want


def test_supersampled_entry_points_still_take_only_nearest_and_bilinear():
    lib = nat.load()
    dst = nat.make_proj(nat.KIND_CAMERA, 6, 10, 0, rad(180), 3.0, 3.0 / rad(90))
    plan = nat.Plan(dst, [], nat.make_proj(nat.KIND_PANO, 16, 32), defer=True)
    need = ctypes.c_size_t(0)
    assert lib.pb_remap_ss_workspace(plan.handle, 2, 2, 0, ctypes.byref(need)) == -1
    assert "catmull-rom" not in nat.INTERP_IDS


# ---- Python API -----------------------------------------------------------------------------------------------------------------------
def test_refusals_without_gpu():
    cm = pb.CameraImage(np.zeros((16, 16, 3), np.uint8), rad(180), pb.equidistant()).get_coordinate_map()
    src = pb.PanoramaImage(np.zeros((24, 48, 3), np.uint8))
    for bad in ("bicubic", "cubic", "Catmull-Rom", "catmull_rom"):
        with pytest.raises(ValueError):
            src.process_coordinate_map(cm, interpolation=bad)
    with pytest.raises(NotImplementedError):
        pb.PanoramaImage(np.zeros((24, 48, 3), np.float32)).process_coordinate_map(cm, interpolation="catmull-rom")
    with pytest.raises(NotImplementedError):
        pb.PanoramaImage(np.zeros((24, 48), np.int16)).process_coordinate_map(cm, interpolation="catmull-rom")
    # with supersampling: ValueError whatever else is wrong, before anything reaches the library
    cm2 = pb.CameraImage(np.zeros((16, 16, 3), np.uint8), rad(180), pb.equidistant()).get_coordinate_map(supersample=2)
    for img in (np.zeros((24, 48, 3), np.uint8), np.zeros((24, 48, 3), np.float32)):
        with pytest.raises(ValueError, match="catmull-rom"):
            pb.PanoramaImage(img).process_coordinate_map(cm2, interpolation="catmull-rom")
        with pytest.raises(ValueError, match="catmull-rom"):
            pb.PanoramaImage(img).process_coordinate_map(cm, interpolation="catmull-rom", supersample=4)
    dst = nat.make_proj(nat.KIND_CAMERA, 8, 8, 0, rad(180), 4.0, 4.0 / rad(90))
    plan = nat.Plan(dst, [], nat.make_proj(nat.KIND_PANO, 16, 32), defer=True)
    with pytest.raises(ValueError, match="catmull-rom"):
        plan.launch(16, 16, 1, None, "catmull-rom", supersample=2)
    with pytest.raises(ValueError, match="catmull-rom"):
        plan.remap(None, interpolation="catmull-rom", supersample=2)
    with pytest.raises(ValueError, match="catmull-rom"):
        pb.batch.remap_frames(plan, [], interpolation="catmull-rom", supersample=2)
    from photonbend_amd import _hostpipe

    with pytest.raises(ValueError, match="catmull-rom"):
        _hostpipe.remap_ndarray(plan, np.zeros((16, 32, 3), np.uint8), "catmull-rom", supersample=2)


# ---- CLI ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cmd", ["make-photo", "alter-photo", "make-pano"])
def test_cli_option(cmd):
    res = CliRunner().invoke(cli.main, [cmd, "--help"])
    assert res.exit_code == 0 and "--interpolation" in res.output and "catmull-rom" in res.output


def test_cli_refuses_catmull_rom_with_supersampling(tmp_path):
    inp = tmp_path / "in.png"
    Image.fromarray(np.zeros((40, 80, 3), np.uint8)).save(inp)
    for n in ("2", "4"):
        res = CliRunner().invoke(cli.main, ["make-photo", str(inp), "--type", "inscribed", "--lens", "equidistant", "--fov", "180",
                                            "--interpolation", "catmull-rom", "--supersample", n, str(tmp_path / "o.png")])
        assert res.exit_code == 2 and "--interpolation" in res.output and "supersample" in res.output, (res.exit_code, res.output)
        assert not (tmp_path / "o.png").exists()
    res = CliRunner().invoke(cli.main, ["make-pano", str(inp), "--type", "inscribed", "--lens", "equidistant", "--fov", "180",
                                        "--interpolation", "bicubic", str(tmp_path / "o.png")])
    assert res.exit_code == 2 and "--interpolation" in res.output


def test_cli_passes_the_sampler_and_keeps_the_default_call(monkeypatch, tmp_path):
    inp = tmp_path / "in.png"
    Image.fromarray(np.zeros((40, 80, 3), np.uint8)).save(inp)
    seen = []
    monkeypatch.setattr(cli, "run_chain", lambda *a, **k: seen.append((a[4:], k)))
    base = ["alter-photo", str(inp), "--itype", "inscribed", "--ilens", "equidistant", "--ifov", "180", "--otype", "inscribed", "--olens",
            "equisolid", "--ofov", "170", str(tmp_path / "o.png")]
    for extra, want in (([], ((1,), {})), (["--interpolation", "nearest"], ((1,), {})),
                        (["--interpolation", "catmull-rom"], ((1,), {"interpolation": "catmull-rom"})),
                        (["--interpolation", "bilinear", "--supersample", "2"], ((2,), {"interpolation": "bilinear"}))):
        seen.clear()
        res = CliRunner().invoke(cli.main, base + extra)
        assert res.exit_code == 0, res.output
        assert seen == [want], (extra, seen)
