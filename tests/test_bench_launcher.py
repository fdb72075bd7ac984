"""bench.py's own multi-rank launcher (`--gpus N` without RANK in the environment starts the N ranks itself), rehearsed on the ONE GPU a
test box has: the ranks share the card and talk over gloo (PB_DIST_BACKEND=gloo).  VERDICT r4 asked for eight ranks; the pool's boxes
kill a job with more than six GPU processes (the launcher counts), so the on-card rehearsal runs FIVE ranks - rendezvous, the broadcast
of the parameter block, shard_range, the `sharded` block's all-gather of first-frame hashes and rank 0's re-make - and the eight-rank
choreography runs on the CPU (tests/test_parallel_gloo.py::test_broadcast_sharding_and_gather_world8).  profiles/r05_bench_5ranks_gloo.json
is the kept line of such a run with the BASELINE share sizes (64 / 32 frames per rank)."""

import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def _run(extra_env, gpus):
    env = dict(os.environ, PB_DIST_BACKEND="gloo", PB_SHARD_FRAMES="8", **extra_env)
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(gpus), "--steps", "8", "--warmup", "2", "--no-cpu-baseline", "--full"],
                          env=env, cwd=ROOT, capture_output=True, text=True, timeout=900)


def test_five_ranks_share_one_gpu_through_bench_py():
    res = _run({}, 5)
    assert res.returncode == 0, res.stderr[-2000:]
    line = json.loads(res.stdout.strip().splitlines()[-1])
    assert line["n_gpus"] == 5 and line["ranks_seen"] == 5 and line["collective_backend"] == "gloo"
    sh = line["sharded"]
    assert sh["ranks_seen"] == 5
    for name in ("c4", "c5"):
        assert sh[name]["first_frames_identical_to_rank0"] == 5, sh[name]
        assert sh[name]["frames_total"] == 5 * sh[name]["frames_per_gpu"]


def test_a_dead_rank_fails_the_whole_command():
    res = _run({"PB_BENCH_FAIL_RANK": "1"}, 3)
    assert res.returncode != 0
    assert not any(l.startswith("{") and '"metric"' in l for l in res.stdout.splitlines()), "no line for fewer ranks than asked for"
