"""CPU checks of the supersampled mode: the n x destination's projection (dimensions, magnitude, f_distance bits), the lazy
recipe carrying its factor, argument validation before anything needs a GPU, the test-side reference against a per-pixel brute force, and
the C ABI's new entries."""

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
from oracle.synth import synth_frame
from photonbend_amd import _native as nat
from photonbend_amd.build import LIB_PATH
from photonbend_amd.scripts import cli
from tests import helpers as H
from tests import ss_ref
from tests.cases import cam, dbl, inscribed, pano, small_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
rad = pb.utils.to_radians


def _bits(x):
    return np.float64(x).view(np.uint64)


@pytest.mark.parametrize("n", [2, 4])
@pytest.mark.parametrize("lens,fov,mag", [("equidistant", 360, None), ("equisolid", 180, 47.5), ("rectilinear", 120, 61.3), ("thoby", 170, 23.0),
                                           ("stereographic", 200, None), ("orthographic", 170, 33.3)])
def test_camera_projection_scales_exactly(n, lens, fov, mag):
    img = pb.CameraImage(np.zeros((48, 64, 3), np.uint8), rad(fov), getattr(pb, lens)(), magnitude=mag)
    p1, pn = img._proj("dst"), img._proj_ss(n)
    assert (pn.height, pn.width) == (n * 48, n * 64) and pn.kind == p1.kind and pn.lens == p1.lens and pn.fov == p1.fov
    assert _bits(pn.magnitude) == _bits(n * img.magnitude)
    fresh = (img.magnitude * n) / img.forward_lens(img.fov / 2)
    assert _bits(pn.f_distance) == _bits(fresh) == _bits(n * img.f_distance)
    cm = img.get_coordinate_map(supersample=n)
    assert cm.is_lazy and cm.supersample == n and cm.shape == (n * 48, n * 64, 3)
    assert cm.dst_proj.key() == pn.key()


@pytest.mark.parametrize("n", [2, 4])
def test_double_and_pano_projections_scale(n):
    d = pb.DoubleCameraImage(np.zeros((40, 81, 3), np.uint8), rad(195), pb.equidistant())
    pd = d._proj_ss(n)
    assert (pd.height, pd.width) == (n * 40, n * 80)  # the map of an odd-width double is 2 (W // 2) wide
    assert _bits(pd.magnitude) == _bits(n * 40 / 2.0)
    assert _bits(pd.f_distance) == _bits((n * 40 / 2.0) / d.forward_lens(d.sensor_fov / 2)) == _bits(n * d.f_distance)
    assert d.get_coordinate_map(supersample=n).shape == (n * 40, n * 80, 3)
    p = pb.PanoramaImage(np.zeros((31, 62, 3), np.uint8))
    pp = p._proj_ss(n)
    assert (pp.kind, pp.height, pp.width) == (nat.KIND_PANO, n * 31, n * 62)
    assert p.get_coordinate_map(supersample=n).shape == (n * 31, n * 62, 3)


def test_supersample_one_is_the_plain_map():
    img = pb.CameraImage(np.zeros((48, 48, 3), np.uint8), rad(180), pb.equisolid(), magnitude=23.5)
    a, b = img.get_coordinate_map(), img.get_coordinate_map(supersample=1)
    assert a.dst_proj.key() == b.dst_proj.key() and a.supersample == b.supersample == 1 and a.shape == b.shape


def test_supersample_survives_rotation_and_copy():
    cm = pb.PanoramaImage(np.zeros((20, 40, 3), np.uint8)).get_coordinate_map(supersample=4)
    r1 = pb.Rotation(0.1, 0.2, 0.3).rotate_coordinate_map(cm)
    r2 = pb.Rotation(-0.4, 0.0, 1.0).rotate_coordinate_map(r1)
    assert r2.is_lazy and r2.supersample == 4 and r2.shape == (80, 160, 3) and len(r2.rotations) == 2
    c = r2.copy()
    assert c.is_lazy and c.supersample == 4 and c.shape == (80, 160, 3) and len(c.rotations) == 2
    assert r2.rotated(np.eye(3)).supersample == 4
    assert "supersample 4" in repr(r2)


@pytest.mark.parametrize("bad", [3, 0, -2, 8, 2.0, True, "2"])
def test_bad_factors_raise_without_gpu(bad):
    img = pb.CameraImage(np.zeros((48, 48, 3), np.uint8), rad(180), pb.equidistant())
    with pytest.raises(ValueError):
        img.get_coordinate_map(supersample=bad)
    src = pb.PanoramaImage(np.zeros((24, 48, 3), np.uint8))
    with pytest.raises(ValueError):
        src.process_coordinate_map(np.zeros((8, 8, 3)), supersample=bad)
    with pytest.raises(ValueError):
        pb.batch.plan_for(img, [], src, supersample=bad)


def test_sample_types_and_divisibility_are_checked_without_gpu():
    cm = pb.CameraImage(np.zeros((16, 16, 3), np.uint8), rad(180), pb.equidistant()).get_coordinate_map(supersample=2)
    with pytest.raises(NotImplementedError):
        pb.PanoramaImage(np.zeros((24, 48, 3), np.float32)).process_coordinate_map(cm)
    with pytest.raises(NotImplementedError):
        pb.PanoramaImage(np.zeros((24, 48), np.int16)).process_coordinate_map(cm, interpolation="bilinear")
    with pytest.raises(ValueError):
        pb.PanoramaImage(np.zeros((24, 48, 3), np.uint8)).process_coordinate_map(cm, interpolation="cubic")
    src = pb.PanoramaImage(np.zeros((24, 48, 3), np.uint8))
    for shape, n in (((5, 6, 3), 2), ((8, 6, 3), 4), ((12, 9, 3), 2)):
        with pytest.raises(ValueError):
            src.process_coordinate_map(np.zeros(shape), supersample=n)
    with pytest.raises(ValueError):  # a lazy 2x map declared as 4x: 32 x 32 is divisible by 4, but a 2x recipe of 18 rows is not
        pb.PanoramaImage(np.zeros((24, 48, 3), np.uint8)).process_coordinate_map(
            pb.CameraImage(np.zeros((9, 9, 3), np.uint8), rad(180), pb.equidistant()).get_coordinate_map(supersample=2), supersample=4)


C5_DST = (4096, 8192)  # BASELINE c5: the 8192 x 4096 panorama made from a Gear-360 stitch


def test_c5_at_four_is_refused_at_every_layer(tmp_path):
    """n = 4 makes c5's destination a 32768 x 16384 map: 2^29 pixels, one past the projection limit (H W <= (2^31 - 1) / 4)."""
    h, w = C5_DST
    assert (4 * h) * (4 * w) == nat.MAX_PROJ_PIXELS + 1
    dst = pb.PanoramaImage(np.zeros((h, w, 3), np.uint8))
    with pytest.raises(ValueError, match="projection limit"):
        dst.get_coordinate_map(supersample=4)
    assert dst.get_coordinate_map(supersample=2).shape == (2 * h, 2 * w, 3)
    with pytest.raises(ValueError, match="projection limit"):
        pb.batch.plan_for(dst, [], pb.DoubleCameraImage(np.zeros((3888, 7776, 3), np.uint8), rad(195), pb.equidistant()), supersample=4)
    # C: a plan of that destination is refused (a deferred plan: no device work), and so is pb_box_reduce of a frame of that size
    big = nat.make_proj(nat.KIND_PANO, 4 * h, 4 * w)
    src = nat.make_proj(nat.KIND_DOUBLE, 3888, 7776, nat.LENS_IDS["equidistant"], rad(195), 1944.0, 1944.0 / rad(195 / 2))
    with pytest.raises(nat.PbError, match="out of range"):
        nat.Plan(big, [], src, defer=True)
    lib = nat.load()
    assert lib.pb_box_reduce(ctypes.c_void_p(16), ctypes.c_void_p(16), h, w, 3, 1, 4, 1, None) == -1
    assert "projection limit" in lib.pb_last_error().decode()
    # CLI: a clean usage error, no traceback
    inp = tmp_path / "in.png"
    Image.fromarray(np.zeros((40, 80, 3), np.uint8)).save(inp)
    res = CliRunner().invoke(cli.main, ["make-pano", str(inp), "--type", "double", "--lens", "equidistant", "--fov", "195", "-s", str(h),
                                        "--supersample", "4", str(tmp_path / "o.png")])
    assert res.exit_code == 2 and "projection limit" in res.output, (res.exit_code, res.output)
    res = CliRunner().invoke(cli.main, ["make-pano", str(inp), "--type", "double", "--lens", "equidistant", "--fov", "195",
                                        "--supersample", "3", str(tmp_path / "o.png")])
    assert res.exit_code == 2 and "--supersample" in res.output


def test_c_abi_validation_without_gpu():
    lib = nat.load()
    V = ctypes.c_void_p
    for n in (0, 1, 3, 8):
        assert lib.pb_box_reduce(V(16), V(16), 4, 4, 3, 1, n, 1, None) == -1
    assert lib.pb_box_reduce(V(16), V(16), 4, 4, 3, 4, 2, 1, None) == -1  # 4-byte samples
    assert lib.pb_box_reduce(None, V(16), 4, 4, 3, 1, 2, 1, None) == -1
    # a deferred plan of a 6 x 10 camera destination: divisible by 2, not by 4
    dst = nat.make_proj(nat.KIND_CAMERA, 6, 10, 0, rad(180), 3.0, 3.0 / rad(90))
    plan = nat.Plan(dst, [], nat.make_proj(nat.KIND_PANO, 16, 32), defer=True)
    need = ctypes.c_size_t(7)
    for n, interp, ok in ((2, 0, True), (2, 1, True), (4, 0, False), (3, 0, False), (1, 0, False), (2, 2, False)):
        rc = lib.pb_remap_ss_workspace(plan.handle, n, interp, 0, ctypes.byref(need))
        assert (rc == 0) == ok, (n, interp, rc)
    # a deferred plan runs the float64 kernel: never the fused path, the generic one needs one n x frame
    assert lib.pb_remap_ss_workspace(plan.handle, 2, 0, 0, ctypes.byref(need)) == 0 and need.value == 3 * 6 * 10
    assert lib.pb_remap_ss_u8(plan.handle, 4, 0, V(16), V(16), 1, 0, 0, None, 0, 0, None) == -1
    assert "divisible" in lib.pb_last_error().decode()
    assert lib.pb_remap_ss_u8(plan.handle, 2, 0, V(16), V(16), 1, 0, 0, None, 0, 0, None) == -1  # no workspace for the generic path
    assert "workspace" in lib.pb_last_error().decode()
    assert lib.pb_remap_ss_u8(plan.handle, 2, 0, V(16), V(16), -1, 0, 0, None, 0, 0, None) == -1
    assert lib.pb_remap_ss_u8(plan.handle, 2, 0, V(16), V(16), 0, 0, 0, None, 0, 0, None) == 0  # nothing to do
    with pytest.raises(ValueError):
        plan.out_shape(4)
    assert plan.out_shape(2) == (3, 5) and plan.out_shape(1) == (6, 10)


def test_new_symbols_exported_and_declared():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "photonbend_hip.h")).read(), flags=re.S)
    lib = ctypes.CDLL(LIB_PATH)
    for name in ("pb_remap_ss_u8", "pb_remap_ss_workspace", "pb_box_reduce"):
        assert re.search(rf"\b{name}\s*\(", text), name
        assert hasattr(lib, name) and name in nat.SIGNATURES, name
    assert "#define PB_SS_GENERIC" in text
    assert nat.load().pb_abi_version() == nat.ABI_VERSION == 5
    nm = subprocess.run(["nm", "-D", "--defined-only", LIB_PATH], capture_output=True, text=True)
    if nm.returncode == 0:
        for name in ("pb_remap_ss_u8", "pb_remap_ss_workspace", "pb_box_reduce"):
            assert re.search(rf"\bT {name}$", nm.stdout, re.M), name


def _brute(full: np.ndarray, n: int) -> np.ndarray:
    """Per pixel, per channel: Python's round() of the exact mean (N a power of two: sum / N is exact, round() ties to even)."""
    H, W = full.shape[0] // n, full.shape[1] // n
    out = np.zeros((H, W) + full.shape[2:], full.dtype)
    for i in range(H):
        for j in range(W):
            blk = full[n * i : n * i + n, n * j : n * j + n].reshape((n * n,) + full.shape[2:]).astype(np.int64)
            out[i, j] = np.vectorize(lambda s: round(s / (n * n)))(blk.sum(axis=0))
    return out


@pytest.mark.parametrize("n", [2, 4])
def test_block_mean_rule(n):
    rng = np.random.default_rng(n)
    for dt, hi in ((np.uint8, 256), (np.uint16, 65536)):
        a = rng.integers(0, hi, size=(4 * n, 3 * n, 3)).astype(dt)
        a[:n, :n] = np.array([0, 1, 2])[None, None, :]  # sums near the tie
        a[0, 0] = 1
        assert np.array_equal(ss_ref.block_mean(a, n), _brute(a, n))
    # ties: sum = q N + N / 2 goes to the even neighbour
    N = n * n
    for q in (0, 1, 2, 3, 254):
        blk = np.full((n, n), q, np.uint8)
        blk.flat[: N // 2] += 1  # sum = q N + N / 2
        assert int(ss_ref.block_mean(blk, n)[0, 0]) == (q if q % 2 == 0 else q + 1)


@pytest.mark.parametrize("name,n,bilinear", [("A_photo_odd", 2, False), ("B_pano_odd", 4, False), ("E_stitch_195_masked", 2, False),
                                             ("C_alter_ste_ort", 2, True), ("E_double_dst", 4, False)])
def test_reference_helper_against_brute_force(name, n, bilinear):
    case = next(c for c in small_cases() if c.name == name)
    frame = H.case_frame(case)
    od = ss_ref.orc_proj_ss(case.dst, n)
    with np.errstate(all="ignore"):
        full = (orc.remap_bilinear if bilinear else orc.remap)(od, H.orc_proj(case.src), frame, H.orc_rots(case))
    got = ss_ref.reference(case, n, frame, bilinear)
    kind, h, w = case.dst[:3]
    assert got.shape[:2] == (h, 2 * (w // 2) if kind == "double" else w)
    assert np.array_equal(got, _brute(full, n))
