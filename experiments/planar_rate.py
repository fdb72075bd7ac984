#!/usr/bin/env python3
"""The rates of pb_remap_planar, measured in ONE process, warm, alternating: medians of `reps` rounds of `iters` launches
between two HIP events, after a warm-up launch (the method of experiments/nv12_rate.py).
    python experiments/planar_rate.py [--reps 5] [--iters 20] [--cases c2,c1] [--formats yuv420p,yuv444p,yuv420p16le] [--out file.json]
On each case's geometry and for each pixel format, time per frame of
  (a)   pb_remap_planar: one launch of pb_video_hot_kernel, the three planes;
  (b)   what a caller could do for the same frame before, on the same build and with the same bytes: pb_remap_px of plane 0, plus
        pb_index_map_i32 into a preallocated buffer, the chroma index of the anchors from it (tensor arithmetic on the device) and
        two pb_gather_px, one per chroma plane - measured twice (A / A) for that figure's own spread;
  (c)   pb_remap_nv12 on the same plan and sample size, at 4:2:0 only, as the yardstick (the same bytes per frame; half the chroma gathers).
Fill (0, 0, 0), so that (a) and (b) write the same bytes.  Exit status 1 when (a)'s bytes differ from (b)'s, or when (a) is not faster than
(b) by more than the A / A spread of (b) in the same run - the only threshold.  The (a) / (c) ratio is reported."""

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

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from pixel_format_rate import alternate  # noqa: E402


def chroma_index(idx, w, cx, cy):
    """The anchors' index into a (h >> cy, w >> cx) chroma plane, -1 where the anchor is black."""
    a = idx[0 :: 1 << cy, 0 :: 1 << cx]
    r, c = torch.div(a, w, rounding_mode="floor"), torch.remainder(a, w)
    return torch.where(a < 0, a, (r >> cy) * (w >> cx) + (c >> cx)).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--cases", default="c2,c1")
    ap.add_argument("--formats", default="yuv420p,yuv444p,yuv420p16le")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    stream = torch.cuda.current_stream()
    st = nat.current_stream()
    L = nat.load()
    res = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "iters": args.iters, "rows": []}
    failures = []
    zero = (nat.C.c_uint16 * 3)(0, 0, 0)
    for name in args.cases.split(","):
        case = next(c for c in full_cases() if c.name == name)
        plan = H.pb_plan_private(case, bilinear=False)
        _, h, w, *_ = case.src
        Hd, Wd = case.dst[1], case.dst[2]
        idx = torch.empty((Hd, Wd), dtype=torch.int32, device="cuda")
        for fmt in args.formats.split(","):
            dt, sub, _ = nat.PLANAR_FORMATS[fmt]
            S = dt.itemsize
            cx, cy = nat.PLANAR_SHIFTS[sub]
            assert plan.planar_supported(sub, S) and plan.px_supported(S)
            n_src, n_dst = nat.planar_frame_samples(h, w, sub) * S, nat.planar_frame_samples(Hd, Wd, sub) * S
            src = torch.randint(0, 256, (n_src,), dtype=torch.uint8, device="cuda")
            out_a = torch.empty((n_dst,), dtype=torch.uint8, device="cuda")
            out_b = torch.empty_like(out_a)
            sc, dc = (h >> cy) * (w >> cx) * S, (Hd >> cy) * (Wd >> cx) * S  # a chroma plane's bytes
            n_chroma = (Hd >> cy) * (Wd >> cx)
            semi = sub == nat.PLANAR_420
            out_c = torch.empty_like(out_a) if semi else None

            def a():
                nat.check(L.pb_remap_planar(plan.handle, src.data_ptr(), out_a.data_ptr(), 1, None, None, sub, S, nat.C.addressof(zero), st))

            def b():
                nat.check(L.pb_remap_px(plan.handle, src.data_ptr(), out_b.data_ptr(), 1, 0, 0, S, st))
                nat.check(L.pb_index_map_i32(plan.handle, idx.data_ptr(), None, st))
                ci = chroma_index(idx, w, cx, cy)
                for k in (0, 1):
                    nat.check(L.pb_gather_px(ci.data_ptr(), src.data_ptr() + h * w * S + k * sc, out_b.data_ptr() + Hd * Wd * S + k * dc, n_chroma, S, st))

            def c():  # (the same buffer read as a semi-planar frame: the timing does not depend on what the bytes mean)
                nat.check(L.pb_remap_nv12(plan.handle, src.data_ptr(), out_c.data_ptr(), 1, None, None, S, nat.C.addressof(zero), st))

            a()
            b()
            torch.cuda.synchronize()
            equal = bool(torch.equal(out_a, out_b))
            ways = {"b_1": b, "a": a, **({"c": c} if semi else {}), "b_2": b}
            t = alternate(ways, args.reps, args.iters, stream)
            b_all = t["b_1"]["us_all"] + t["b_2"]["us_all"]
            b_med, b_spread = statistics.median(b_all), max(b_all) - min(b_all)
            row = {"case": name, "pixel_format": fmt, "bytes_per_sample": S, "bytes_equal": equal, "a_remap_planar": t["a"], "b_px_index_map_gathers_1": t["b_1"],
                   "b_px_index_map_gathers_2": t["b_2"], "b_us": round(b_med, 1), "b_spread_us": round(b_spread, 1), "b_over_a": round(b_med / t["a"]["us"], 2),
                   "c_remap_nv12": t.get("c"), "a_over_c": round(t["a"]["us"] / t["c"]["us"], 2) if semi else None,
                   "a_GBps_out": round(n_dst / t["a"]["us"] * 1e-3, 1)}
            res["rows"].append(row)
            print(json.dumps(row), flush=True)
            if not equal:
                failures.append(f"{name} {fmt}: pb_remap_planar's bytes differ from pb_remap_px + index map + two gathers'")
            if not t["a"]["us"] < b_med - b_spread:
                failures.append(f"{name} {fmt}: pb_remap_planar ({t['a']['us']} us) is not faster than the parent's route ({b_med:.1f} us) beyond its spread ({b_spread:.1f} us)")
            del src, out_a, out_b, out_c
        del plan, idx
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
