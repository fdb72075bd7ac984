#!/usr/bin/env python3
"""The rates of pb_remap_nv12, measured in ONE process, warm, alternating: medians of `reps` rounds of `iters` launches
between two HIP events, after a warm-up launch (the method of experiments/pixel_format_rate.py).
    python experiments/nv12_rate.py [--reps 5] [--iters 20] [--cases c2,c1] [--out file.json]
On each case's geometry, for NV12 (S = 1) and P010 (S = 2), time per frame of
  (a)   pb_remap_nv12: one launch of pb_video_hot_kernel (PAIRS), both planes;
  (b)   what a caller could do for the same frame before, on the same build and with the same bytes: pb_remap_px of the luma plane, plus
        pb_index_map_i32 into a preallocated buffer, the chroma index of the anchors from it (tensor arithmetic on the device) and
        pb_gather_px of the pairs - measured twice (A / A) for that figure's own spread;
  (b')  the same with the anchors' chroma index cached (pb_remap_px + one pb_gather_px; 1 byte per output pixel resident per plan);
  (c)   pb_remap_u8 on the same plan (RGB8: 3 bytes per pixel where the video frame has 1.5 S), as the yardstick.
Fill (0, 0, 0), so that (a) and (b) write the same bytes.  Exit status 1 when (a)'s bytes differ from (b)'s, or when (a) is not faster than
(b) by more than the A / A spread of (b) in the same run."""

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

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from pixel_format_rate import alternate  # noqa: E402


def chroma_index(idx, w):
    """The anchors' index into the (h/2, w/2) plane of pairs, -1 where the anchor is black."""
    a = idx[0::2, 0::2]
    r, c = torch.div(a, w, rounding_mode="floor"), torch.remainder(a, w)
    return torch.where(a < 0, a, (r >> 1) * (w // 2) + (c >> 1)).contiguous()


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
    zero = (nat.C.c_uint16 * 3)(0, 0, 0)
    for name in args.cases.split(","):
        case = next(c for c in full_cases() if c.name == name)
        plan = H.pb_plan_private(case, bilinear=False)
        _, h, w, *_ = case.src
        Hd, Wd = case.dst[1], case.dst[2]
        idx = torch.empty((Hd, Wd), dtype=torch.int32, device="cuda")
        cached = chroma_index(plan.index_map(), w)
        rgb = torch.randint(0, 256, (h, w, 3), dtype=torch.uint8, device="cuda")
        rgb_out = torch.empty((Hd, Wd, 3), dtype=torch.uint8, device="cuda")
        for S in (1, 2):
            assert plan.nv12_supported(S) and plan.px_supported(S)
            src = torch.randint(0, 256, (3 * h // 2, w * S), dtype=torch.uint8, device="cuda")
            out_a = torch.empty((3 * Hd // 2, Wd * S), dtype=torch.uint8, device="cuda")
            out_b = torch.empty_like(out_a)
            uv_src, uv_b = src.data_ptr() + h * w * S, out_b.data_ptr() + Hd * Wd * S
            n_pairs = Hd * Wd // 4

            def a():
                nat.check(L.pb_remap_nv12(plan.handle, src.data_ptr(), out_a.data_ptr(), 1, None, None, S, nat.C.addressof(zero), st))

            def b():
                nat.check(L.pb_remap_px(plan.handle, src.data_ptr(), out_b.data_ptr(), 1, 0, 0, S, st))
                nat.check(L.pb_index_map_i32(plan.handle, idx.data_ptr(), None, st))
                ci = chroma_index(idx, w)
                nat.check(L.pb_gather_px(ci.data_ptr(), uv_src, uv_b, n_pairs, 2 * S, st))

            def b_cached():
                nat.check(L.pb_remap_px(plan.handle, src.data_ptr(), out_b.data_ptr(), 1, 0, 0, S, st))
                nat.check(L.pb_gather_px(cached.data_ptr(), uv_src, uv_b, n_pairs, 2 * S, st))

            def c():
                nat.check(L.pb_remap_u8(plan.handle, rgb.data_ptr(), rgb_out.data_ptr(), 1, 0, 0, st))

            a()
            b()
            torch.cuda.synchronize()
            equal = bool(torch.equal(out_a, out_b))
            t = alternate({"b_1": b, "a": a, "b_cached": b_cached, "c": c, "b_2": b}, args.reps, args.iters, stream)
            b_all = t["b_1"]["us_all"] + t["b_2"]["us_all"]
            b_med, b_spread = statistics.median(b_all), max(b_all) - min(b_all)
            row = {"case": name, "bytes_per_sample": S, "bytes_equal": equal, "a_remap_nv12": t["a"], "b_px_index_map_gather_1": t["b_1"],
                   "b_px_index_map_gather_2": t["b_2"], "b_us": round(b_med, 1), "b_spread_us": round(b_spread, 1), "b_cached": t["b_cached"],
                   "c_remap_u8": t["c"], "b_over_a": round(b_med / t["a"]["us"], 2), "b_cached_over_a": round(t["b_cached"]["us"] / t["a"]["us"], 2),
                   "a_over_c": round(t["a"]["us"] / t["c"]["us"], 2), "a_GBps_out": round(3 * Hd * Wd * S / 2 / t["a"]["us"] * 1e-3, 1)}
            res["rows"].append(row)
            print(json.dumps(row), flush=True)
            if not equal:
                failures.append(f"{name} S={S}: pb_remap_nv12's bytes differ from pb_remap_px + index map + gather's")
            if not t["a"]["us"] < b_med - b_spread:
                failures.append(f"{name} S={S}: pb_remap_nv12 ({t['a']['us']} us) is not faster than the parent's route ({b_med:.1f} us) beyond its spread ({b_spread:.1f} us)")
            del src, out_a, out_b
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
