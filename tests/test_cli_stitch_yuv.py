"""The ``stitch-yuv`` command: raw packed video frames of a side-by-side double fisheye in, panorama frames of the same pixel
format out.  The GPU test runs the command as a child ``python -m photonbend_amd`` process and compares the output file with
``Plan.stitch_planar`` / ``Plan.stitch_nv12`` of the same chain.  (The usage errors, which need no GPU: tests/test_stitch_video_host.py.)"""

import os
import subprocess
import sys

import numpy as np
import pytest
from click.testing import CliRunner

import photonbend_amd as pb
from photonbend_amd import _native as nat
from photonbend_amd.scripts import cli

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H_, W_ = 40, 80
OUT_H, OUT_W = 34, 72
ROT = (3, 90, -7)


def frames_of(n, fmt, seed, h=H_, w=W_):
    dt, fam, _ = nat.VIDEO_FORMATS[fmt]
    nb = int(np.prod(fam.packed(h, w)[0])) * dt.itemsize
    return np.random.default_rng(seed).integers(0, 256, (n, nb), dtype=np.uint8).view(dt)


def child(*args):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, "-m", "photonbend_amd", "stitch-yuv", *map(str, args)], capture_output=True, cwd=ROOT, env=env, timeout=300)


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", ["nv12", "p010", "yuv420p", "yuv422p10le", "gbrp"])
def test_five_frames_in_chunks_of_four_equal_the_plan_s_stitch(tmp_path, fmt):
    import torch

    rad = pb.utils.to_radians
    dt, fam, fill = nat.VIDEO_FORMATS[fmt]
    frames = frames_of(5, fmt, 20)
    inp, out = tmp_path / "in.yuv", tmp_path / "out.yuv"
    frames.tofile(inp)
    common = (inp, out, "--width", W_, "--height", H_, "--pix-fmt", fmt, "--lens", "equidistant", "--fov", 195, "--out-width", OUT_W, "--out-height", OUT_H,
              "-r", *ROT, "--chunk", 4)
    res = child(*common)
    assert res.returncode == 0, res.stderr.decode()
    cmap = pb.Rotation(*map(rad, ROT)).rotate_coordinate_map(pb.PanoramaImage(np.zeros((OUT_H, OUT_W, 3), np.uint8)).get_coordinate_map())
    src = pb.DoubleCameraImage(np.zeros((H_, W_, 3), np.uint8), rad(195), pb.equidistant())
    plan = nat.Plan(cmap.dst_proj, list(cmap.rotations), src._proj(), bilinear=False)
    s = torch.from_numpy(frames.reshape((5,) + fam.packed(H_, W_)[0])).cuda()
    want = (plan.stitch_nv12(s) if fam.pairs else plan.stitch_planar(s, fam.sub, fill=fill)).cpu().numpy().reshape(5, -1)
    got = np.fromfile(out, dt)
    assert got.size == want.size and np.array_equal(got.reshape(want.shape), want)
    assert not np.array_equal(want[0], want[1])
    # through pipes (in this process): nothing but frames on stdout; a truncated last frame leaves whole frames only
    piped = ("-", "-", *map(str, common[2:]))
    res = CliRunner().invoke(cli.main, ["stitch-yuv", *piped], input=frames.tobytes())
    assert res.exit_code == 0 and res.stdout_bytes == want.tobytes(), res.stderr if res.stderr_bytes else res.exception
    res = CliRunner().invoke(cli.main, ["stitch-yuv", *piped], input=frames.tobytes()[:-6])
    assert res.exit_code == 1 and b"truncated" in res.stderr_bytes and res.stdout_bytes == want[:4].tobytes()
