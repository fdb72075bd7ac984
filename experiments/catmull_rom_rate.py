#!/usr/bin/env python3
"""Catmull-Rom sampling: the tile kernel (pb_catmull_rom_hot_kernel) next to the bilinear tile kernel (pb_bilinear_hot_kernel) and
next to the mode's float64 route (pb_interp_fix_kernel<PbCatmullRom>, the same geometry's plan in PB_MODE_FAITHFUL), measured in the SAME process,
alternating, per BASELINE config.
    python experiments/catmull_rom_rate.py [--reps 5] [--iters 20] [--configs c1,c2,c3] [--out file.json]
Per round and way: `iters` launches between two HIP events, after a warm-up launch; the figure is the median over `reps` rounds."""

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from photonbend_amd import _native as nat  # noqa: E402
from tests import helpers as H  # noqa: E402
from tests.cases import full_cases  # noqa: E402


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
    ap.add_argument("--configs", default="c1,c2,c3")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    stream = torch.cuda.current_stream()
    rows = []
    for name in args.configs.split(","):
        case = next(c for c in full_cases() if c.name == name)
        frame = nat.synth_frame(case.src[1], case.src[2], frame=0, circle_mask=case.mask)
        plan = H.pb_plan_private(case)
        plan64 = H.pb_plan_private(case)
        plan64.set_mode(nat.MODE_FAITHFUL)
        out = torch.empty((case.dst[1], case.dst[2], 3), dtype=torch.uint8, device="cuda")
        ways = {
            "catmull_rom_tiles": lambda: plan.launch(frame.data_ptr(), out.data_ptr(), interpolation="catmull-rom"),
            "bilinear_tiles": lambda: plan.launch(frame.data_ptr(), out.data_ptr(), interpolation="bilinear"),
            "catmull_rom_float64": lambda: plan64.launch(frame.data_ptr(), out.data_ptr(), interpolation="catmull-rom"),
        }
        times = {k: [] for k in ways}
        for _ in range(args.reps):
            for k, fn in ways.items():  # alternating
                times[k].append(timed(fn, args.iters, stream))
        row = {"config": name, "dst": [case.dst[1], case.dst[2]], "src": [case.src[1], case.src[2]], "fast_path": plan.info()["fast_path"],
               "bilinear_float64_tiles": plan.info()["bilinear_float64_tiles"]}
        for k in ways:
            row[k] = {"us": round(statistics.median(times[k]), 1), "us_all": [round(t, 1) for t in times[k]]}
        row["float64_over_tiles"] = round(row["catmull_rom_float64"]["us"] / row["catmull_rom_tiles"]["us"], 2)
        row["tiles_over_bilinear"] = round(row["catmull_rom_tiles"]["us"] / row["bilinear_tiles"]["us"], 2)
        rows.append(row)
        print(json.dumps(row), flush=True)
        del plan, plan64, out
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "reps": args.reps, "iters": args.iters, "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
