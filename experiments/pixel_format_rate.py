#!/usr/bin/env python3
"""The rates of pb_remap_px, measured in ONE process, warm, alternating: medians of `reps` rounds of `iters` launches between
two HIP events, after a warm-up launch.
    python experiments/pixel_format_rate.py [--reps 5] [--iters 20] [--cases c2,c1] [--out file.json]
On each case's geometry, for each pixel size B in {1, 2, 4, 6, 8}, time per frame of
  (a)   pb_remap_px: one launch of pb_px_hot_kernel;
  (b)   what the library did for the same image before, on the same build: pb_index_map_i32 into a preallocated buffer, then pb_gather_px -
        measured twice (A / A) for that figure's own spread;
  (b')  pb_gather_px alone on a cached index map: the best a C caller could do before (4 bytes per output pixel resident per plan);
  (c)   pb_remap_u8 on the same plan (three-byte pixels), for scale.
Exit status 1 when (a)'s bytes differ from (b)'s, or when (a) is not faster than (b) by more than the A / A spread of (b) in the same run."""

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from photonbend_amd import _native as nat  # noqa: E402
from tests import helpers as H  # noqa: E402
from tests.cases import full_cases  # noqa: E402

SIZES = (1, 2, 4, 6, 8)


def timed(fn, iters, stream):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    a.record(stream)
    for _ in range(iters):
        fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters  # us per call


def alternate(ways, reps, iters, stream):
    times = {k: [] for k in ways}
    for _ in range(reps):
        for k, fn in ways.items():
            times[k].append(timed(fn, iters, stream))
    return {k: {"us": round(statistics.median(v), 1), "us_all": [round(t, 1) for t in v]} for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--cases", default="c2,c1")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    stream = torch.cuda.current_stream()
    st = nat.current_stream()
    L = nat.load()
    res = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "iters": args.iters, "rows": []}
    failures = []
    for name in args.cases.split(","):
        case = next(c for c in full_cases() if c.name == name)
        plan = H.pb_plan_private(case, bilinear=False)
        _, h, w, *_ = case.src
        Hd, Wd = case.dst[1], case.dst[2]
        npx = Hd * Wd
        idx = torch.empty((Hd, Wd), dtype=torch.int32, device="cuda")
        cached = plan.index_map()
        rgb = torch.randint(0, 256, (h, w, 3), dtype=torch.uint8, device="cuda")
        rgb_out = torch.empty((Hd, Wd, 3), dtype=torch.uint8, device="cuda")
        info = plan.info()
        for B in SIZES:
            assert plan.px_supported(B)
            src = torch.randint(0, 256, (h, w, B), dtype=torch.uint8, device="cuda")
            out_a = torch.empty((Hd, Wd, B), dtype=torch.uint8, device="cuda")
            out_b = torch.empty_like(out_a)

            def a():
                nat.check(L.pb_remap_px(plan.handle, src.data_ptr(), out_a.data_ptr(), 1, 0, 0, B, st))

            def b():
                nat.check(L.pb_index_map_i32(plan.handle, idx.data_ptr(), None, st))
                nat.check(L.pb_gather_px(idx.data_ptr(), src.data_ptr(), out_b.data_ptr(), npx, B, st))

            def b_cached():
                nat.check(L.pb_gather_px(cached.data_ptr(), src.data_ptr(), out_b.data_ptr(), npx, B, st))

            def c():
                nat.check(L.pb_remap_u8(plan.handle, rgb.data_ptr(), rgb_out.data_ptr(), 1, 0, 0, st))

            a()
            b()
            torch.cuda.synchronize()
            equal = bool(torch.equal(out_a, out_b))
            t = alternate({"b_1": b, "a": a, "b_cached": b_cached, "c": c, "b_2": b}, args.reps, args.iters, stream)
            b_all = t["b_1"]["us_all"] + t["b_2"]["us_all"]
            b_med, b_spread = statistics.median(b_all), max(b_all) - min(b_all)
            row = {"case": name, "bytes_per_px": B, "bytes_equal": equal, "a_remap_px": t["a"], "b_index_map_gather_1": t["b_1"], "b_index_map_gather_2": t["b_2"],
                   "b_us": round(b_med, 1), "b_spread_us": round(b_spread, 1), "b_cached_gather": t["b_cached"], "c_remap_u8": t["c"],
                   "b_over_a": round(b_med / t["a"]["us"], 2), "b_cached_over_a": round(t["b_cached"]["us"] / t["a"]["us"], 2),
                   "a_over_c": round(t["a"]["us"] / t["c"]["us"], 2), "a_GBps_out": round(npx * B / t["a"]["us"] * 1e-3, 1)}
            res["rows"].append(row)
            print(json.dumps(row), flush=True)
            if not equal:
                failures.append(f"{name} B={B}: pb_remap_px's bytes differ from pb_index_map_i32 + pb_gather_px's")
            if not t["a"]["us"] < b_med - b_spread:
                failures.append(f"{name} B={B}: pb_remap_px ({t['a']['us']} us) is not faster than index map + gather ({b_med:.1f} us) beyond its spread ({b_spread:.1f} us)")
            del src, out_a, out_b
        res.setdefault("mix", {})[name] = {k: info[k] for k in ("tiles", "fix_tiles", "fix_pixels", "lean_tiles", "direct_tiles", "black_tiles")}
        del plan, idx, cached, rgb, rgb_out
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    for msg in failures:
        print("FAILED: " + msg, file=sys.stderr)
    sys.exit(1 if failures else 0)


if __name__ == "__main__":
    main()
