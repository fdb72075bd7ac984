"""``remap-yuv`` and ``remap-nv12`` with ``--interpolation bilinear``: each command runs as a child ``python -m photonbend_amd``
process on two small frames through files, and the output file must hold what ``Plan.remap_planar`` / ``Plan.remap_nv12`` give with
``interpolation="bilinear"`` on the plan the command makes (the photo make-photo would make, after the -r rotation)."""

import os
import subprocess
import sys

import numpy as np
import pytest

import photonbend_amd as pb
from photonbend_amd import _native as nat
from photonbend_amd.core import rotation_track

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H_, W_, SIZE = 16, 32, 18
ROT = (5, -20, 33)


def child(command, *args):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, "-m", "photonbend_amd", command, *map(str, args)], capture_output=True, cwd=ROOT, env=env, timeout=300)


def the_plan():
    rad = pb.utils.to_radians
    dst = pb.CameraImage(np.zeros((SIZE, SIZE, 3), np.uint8), rad(180), pb.equidistant(), magnitude=SIZE / 2 - 0.5)
    dstp, srcp = dst.get_coordinate_map().dst_proj, pb.PanoramaImage(np.zeros((H_, W_, 3), np.uint8))._proj("src")
    mats = rotation_track(np.array([[rad(v) for v in ROT]], np.float64))
    return nat.Plan(dstp, [mats[0]], srcp, bilinear=True)


COMMON = ("--width", W_, "--height", H_, "--type", "inscribed", "--lens", "equidistant", "--fov", 180, "--size", SIZE, "-r", *ROT, "--chunk", 4)


@pytest.mark.parametrize("fmt", ["yuv420p", "yuv422p10le", "gbrp"])
def test_remap_yuv_bilinear_through_files(tmp_path, fmt):
    import torch

    dt, sub, fill = nat.PLANAR_FORMATS[fmt]
    top = 1023 if "10le" in fmt else np.iinfo(dt).max
    frames = np.random.default_rng(20).integers(0, top + 1, (2, nat.planar_frame_samples(H_, W_, sub)), dtype=dt)
    inp, out = tmp_path / "in.yuv", tmp_path / "out.yuv"
    frames.tofile(inp)
    res = child("remap-yuv", inp, out, *COMMON, "--pix-fmt", fmt, "--interpolation", "bilinear")
    assert res.returncode == 0, res.stderr.decode()
    plan = the_plan()
    want = plan.remap_planar(torch.from_numpy(frames).cuda(), sub, fill=fill, interpolation="bilinear").cpu().numpy()
    got = np.fromfile(out, dt)
    assert got.size == want.size and np.array_equal(got.reshape(want.shape), want)
    nearest = plan.remap_planar(torch.from_numpy(frames).cuda(), sub, fill=fill).cpu().numpy()
    assert not np.array_equal(want, nearest)  # (the option changed the sampler)
    res = child("remap-yuv", inp, out, *COMMON, "--pix-fmt", fmt)  # the default is nearest, as before
    assert res.returncode == 0 and np.array_equal(np.fromfile(out, dt).reshape(nearest.shape), nearest), res.stderr.decode()


@pytest.mark.parametrize("fmt,dt", [("nv12", np.uint8), ("p010", np.uint16)])
def test_remap_nv12_bilinear_through_files(tmp_path, fmt, dt):
    import torch

    S = np.dtype(dt).itemsize
    frames = np.random.default_rng(21).integers(0, 256, (2, 3 * H_ // 2, W_ * S), dtype=np.uint8).view(dt)
    inp, out = tmp_path / "in.yuv", tmp_path / "out.yuv"
    frames.tofile(inp)
    res = child("remap-nv12", inp, out, *COMMON, "--pix-fmt", fmt, "--interpolation", "bilinear")
    assert res.returncode == 0, res.stderr.decode()
    plan = the_plan()
    want = plan.remap_nv12(torch.from_numpy(frames).cuda(), interpolation="bilinear").cpu().numpy()
    got = np.fromfile(out, dt)
    assert got.size == want.size and np.array_equal(got.reshape(want.shape), want)
    assert not np.array_equal(want, plan.remap_nv12(torch.from_numpy(frames).cuda()).cpu().numpy())
