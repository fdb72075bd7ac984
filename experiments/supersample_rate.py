#!/usr/bin/env python3
"""Supersampled remapping: the fused kernel against the forced generic path and against the plain n x remap, measured in the
SAME process, alternating, per BASELINE config and factor; plus the n x plan's creation time and device memory.
    python experiments/supersample_rate.py [--reps 5] [--iters 20] [--out file.json]
Per round and way: `iters` launches between two HIP events, after a warm-up launch; the figure is the median over `reps` rounds.
Bytes are algorithmic (what the way must move at least): fused = source frame + H x W output; generic = source frame + n^2 H W written and
read back + H W output; plain = source frame + n^2 H W.  c5 (double-fisheye source) has no fused path: generic and plain only; c5 at n = 4
(a 2^29-pixel map) is refused and recorded as such."""

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from photonbend_amd import _native as nat  # noqa: E402
from tests import helpers as H  # noqa: E402
from tests.cases import full_cases  # noqa: E402


def plan_of(case, n):
    """(n x plan, its creation ms, device bytes it holds)."""
    src, cm = H.pb_chain(case, image=np.zeros((case.src[1], case.src[2], 3), np.uint8))
    dst = H.pb_obj(case.dst)
    proj = dst._proj_ss(n)
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    t0 = time.perf_counter()
    plan = nat.Plan(proj, cm.rotations, src._proj())
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3
    return plan, ms, free0 - torch.cuda.mem_get_info()[0]


def timed(fn, iters, stream):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    a.record(stream)
    for _ in range(iters):
        fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters  # us per launch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--configs", default="c1,c2,c3,c5_180")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    stream = torch.cuda.current_stream()
    rows = []
    for name in args.configs.split(","):
        case = next(c for c in full_cases() if c.name == name)
        frame = nat.synth_frame(case.src[1], case.src[2], frame=0, circle_mask=case.mask)
        src_bytes = frame.numel()
        for n in (2, 4):
            try:
                plan, create_ms, plan_bytes = plan_of(case, n)
            except (ValueError, nat.PbError) as exc:
                rows.append({"config": name, "n": n, "refused": str(exc)})
                print(json.dumps(rows[-1]), flush=True)
                continue
            oh, ow = plan.out_shape(n)
            out = torch.empty((oh, ow, 3), dtype=torch.uint8, device="cuda")
            full = torch.empty((plan.dst.height, plan.dst.width, 3), dtype=torch.uint8, device="cuda")
            out_b, full_b = out.numel(), full.numel()
            ways = {
                "fused": (lambda: plan.launch(frame.data_ptr(), out.data_ptr(), supersample=n), src_bytes + out_b),
                "generic": (lambda: plan.launch(frame.data_ptr(), out.data_ptr(), supersample=n, generic=True), src_bytes + 2 * full_b + out_b),
                "plain_nx": (lambda: plan.launch(frame.data_ptr(), full.data_ptr()), src_bytes + full_b),
            }
            if plan.double_src:
                del ways["fused"]  # (the generic path is what a double-fisheye source takes)
            times = {k: [] for k in ways}
            for _ in range(args.reps):
                for k, (fn, _) in ways.items():  # alternating: fused, generic, plain, fused, ...
                    times[k].append(timed(fn, args.iters, stream))
            row = {"config": name, "n": n, "out": [oh, ow], "nx": [plan.dst.height, plan.dst.width], "plan_create_ms": round(create_ms, 2),
                   "plan_device_mib": round(plan_bytes / 2**20, 1), "fast_path": plan.info()["fast_path"]}
            for k, (_, nbytes) in ways.items():
                us = statistics.median(times[k])
                row[k] = {"us": round(us, 1), "us_all": [round(t, 1) for t in times[k]], "alg_bytes": nbytes, "alg_GBps": round(nbytes / us / 1e3, 1)}
            if "fused" in row:
                row["generic_over_fused"] = round(row["generic"]["us"] / row["fused"]["us"], 2)
            rows.append(row)
            print(json.dumps(row), flush=True)
            del plan, out, full
            torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "reps": args.reps, "iters": args.iters, "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
