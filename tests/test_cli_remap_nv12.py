"""The ``remap-nv12`` command: raw packed NV12 / P010 frames of an equirectangular panorama in, remapped frames out.  Its
usage errors need no GPU: they exit non-zero with a message and write nothing.  One GPU test runs the command as a child
``python -m photonbend_amd`` process and compares the output file with tests/nv12_ref.py of each frame's faithful index map."""

import os
import subprocess
import sys

import numpy as np
import pytest
from click.testing import CliRunner

import photonbend_amd as pb
from photonbend_amd import _native as nat
from photonbend_amd.core import rotation_track
from photonbend_amd.scripts import cli
from tests import nv12_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H_, W_ = 16, 32
TRACK = [(0, 0, 0), (-90, 0, 0), (30, 45, 10), (-3.5, 170, 12), (1, 2, 3)]  # the identity and the pole-crossing pitch lead
PLAN_ROT = (5, -20, 33)


def frames_of(n, dt, seed):
    S = np.dtype(dt).itemsize
    return np.random.default_rng(seed).integers(0, 256, (n, 3 * H_ // 2, W_ * S), dtype=np.uint8).view(dt)


def write_track(path, rows):
    path.write_text("# pitch yaw roll\n" + "".join(f"{p} {y} {r}\n" for p, y, r in rows) + "\n")
    return path


def run(*args):
    return CliRunner().invoke(cli.main, ["remap-nv12", *map(str, args)])


# ---- usage errors: no GPU -------------------------------------------------------------------------------------------------------------
def test_odd_sizes_exit_non_zero_with_a_message_and_write_nothing(tmp_path):
    inp, out = tmp_path / "in.yuv", tmp_path / "out.yuv"
    frames_of(2, np.uint8, 1).tofile(inp)
    for args in (("--width", 31, "--height", 16), ("--width", 32, "--height", 15), ("--width", 32, "--height", 16, "--size", 9),
                 ("--width", 32, "--height", 16, "--type", "inscribed", "--lens", "equidistant", "--fov", 180, "--size", 7)):
        res = run(inp, out, *args)
        assert res.exit_code != 0 and "even" in res.output and not out.exists(), (args, res.output)


def test_a_truncated_last_frame_exits_non_zero_and_leaves_no_partial_frame(tmp_path):
    inp, out = tmp_path / "in.yuv", tmp_path / "out.yuv"
    inp.write_bytes(frames_of(2, np.uint8, 2).tobytes()[:-10])
    res = run(inp, out, "--width", W_, "--height", H_)
    assert res.exit_code != 0 and "truncated" in res.output and not out.exists(), res.output
    inp.write_bytes(frames_of(3, np.uint16, 2).tobytes()[:-2])
    res = run(inp, out, "--width", W_, "--height", H_, "--pix-fmt", "p010")
    assert res.exit_code != 0 and "truncated" in res.output and not out.exists(), res.output


def test_more_frames_than_track_lines_exit_non_zero_and_write_nothing(tmp_path):
    inp, out = tmp_path / "in.yuv", tmp_path / "out.yuv"
    frames_of(5, np.uint8, 3).tofile(inp)
    res = run(inp, out, "--width", W_, "--height", H_, "--rotations", write_track(tmp_path / "track.txt", TRACK[:4]))
    assert res.exit_code != 0 and "5 frames" in res.output and "4 lines" in res.output and not out.exists(), res.output
    bad = tmp_path / "bad.txt"
    bad.write_text("0 0 0\n1 2\n")
    res = run(inp, out, "--width", W_, "--height", H_, "--rotations", bad)
    assert res.exit_code != 0 and "bad.txt:2" in res.output and not out.exists(), res.output


def test_missing_and_mismatched_options_are_usage_errors(tmp_path):
    inp, out = tmp_path / "in.yuv", tmp_path / "out.yuv"
    frames_of(1, np.uint8, 4).tofile(inp)
    for args, word in ((("--width", W_), "--height"), (("--height", H_), "--width"), ((), "--width"),
                       (("--width", W_, "--height", H_, "--lens", "equidistant"), "--type"),
                       (("--width", W_, "--height", H_, "--type", "inscribed", "--lens", "equidistant"), "--fov"),
                       (("--width", W_, "--height", H_, "--type", "double", "--lens", "equidistant", "--fov", 190), "double"),
                       (("--width", W_, "--height", H_, "--pix-fmt", "i420"), "i420"),
                       (("--width", W_, "--height", H_, "--chunk", 6), "multiple of 4"),
                       (("--width", W_, "--height", H_, "--rotations", tmp_path / "none.txt"), "none.txt")):
        res = run(inp, out, *args)
        assert res.exit_code != 0 and word in res.output and not out.exists(), (args, res.output)
    res = run(tmp_path / "absent.yuv", out, "--width", W_, "--height", H_)
    assert res.exit_code != 0 and "absent.yuv" in res.output and not out.exists(), res.output


# ---- the command itself -----------------------------------------------------------------------------------------------------------------
def child(*args):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, "-m", "photonbend_amd", "remap-nv12", *map(str, args)], capture_output=True, cwd=ROOT, env=env, timeout=300)


@pytest.mark.gpu
@pytest.mark.parametrize("fmt,dt", [("nv12", np.uint8), ("p010", np.uint16)])
def test_five_frames_with_a_five_line_track_in_chunks_of_four(tmp_path, fmt, dt):
    import torch

    rad = pb.utils.to_radians
    frames = frames_of(5, dt, 10)
    inp, out = tmp_path / "in.yuv", tmp_path / "out.yuv"
    frames.tofile(inp)
    track = write_track(tmp_path / "track.txt", TRACK)
    common = (inp, out, "--width", W_, "--height", H_, "--pix-fmt", fmt, "--type", "inscribed", "--lens", "equidistant", "--fov", 180, "--size", 18,
              "-r", *PLAN_ROT, "--chunk", 4)
    res = child(*common, "--rotations", track)
    assert res.returncode == 0, res.stderr.decode()
    # the photo make-photo would make: an 18 x 18 inscribed equidistant 180-degree fisheye; frame f's chain is -r, then line f
    dst = pb.CameraImage(np.zeros((18, 18, 3), np.uint8), rad(180), pb.equidistant(), magnitude=18 / 2 - 0.5)
    dstp, srcp = dst.get_coordinate_map().dst_proj, pb.PanoramaImage(np.zeros((H_, W_, 3), np.uint8))._proj("src")
    mats = rotation_track(np.array([[rad(v) for v in r] for r in [PLAN_ROT] + TRACK], np.float64))

    def faithful_index(chain):
        plan = nat.Plan(dstp, list(chain), srcp, defer=True)
        plan.set_mode(nat.MODE_FAITHFUL)
        idx = plan.index_map()
        torch.cuda.synchronize()
        return idx.cpu().numpy()

    want = np.stack([nv12_ref.remap_frame(frames[f], faithful_index([mats[0], mats[1 + f]]), H_, W_) for f in range(5)])
    got = np.fromfile(out, dt)
    assert got.size == want.size and np.array_equal(got.reshape(want.shape), want)
    assert bool((want[:, :18] != nv12_ref.default_fill(dt)[0]).any())
    tracked = want.tobytes()
    # the same run without --rotations: a prepared plan and Plan.remap_nv12
    res = child(*common)
    assert res.returncode == 0, res.stderr.decode()
    plan = nat.Plan(dstp, [mats[0]], srcp, bilinear=False)
    want = plan.remap_nv12(torch.from_numpy(frames).cuda()).cpu().numpy()
    got = np.fromfile(out, dt)
    assert got.size == want.size and np.array_equal(got.reshape(want.shape), want)
    # through pipes (in this process): nothing but frames on stdout; a truncated last frame leaves whole frames only
    piped = ("-", "-", *map(str, common[2:]), "--rotations", str(track))
    res = CliRunner().invoke(cli.main, ["remap-nv12", *piped], input=frames.tobytes())
    assert res.exit_code == 0 and res.stdout_bytes == tracked, res.stderr if res.stderr_bytes else res.exception
    res = CliRunner().invoke(cli.main, ["remap-nv12", *piped], input=frames.tobytes()[:-6])
    assert res.exit_code != 0 and b"truncated" in res.stderr_bytes and res.stdout_bytes == tracked[: 4 * 27 * 18 * np.dtype(dt).itemsize]
