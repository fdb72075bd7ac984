#!/usr/bin/env python3
"""The rates of pb_stitch_nv12 / pb_stitch_planar, measured in ONE process, warm, alternating: medians of `reps` rounds of
`iters` launches between two HIP events, after a warm-up launch (experiments/nv12_rate.py's protocol).
    python experiments/stitch_video_rate.py [--reps 5] [--iters 20] [--formats nv12,p010,yuv420p,yuv444p] [--case c5_195] [--out file.json]
Geometry: c5, an 8192 x 4096 panorama from a 7776 x 3888 double fisheye, fov 195.  Per format, time per frame of
  (a)  the new launch: pb_stitch_video_kernel, every plane;
  (b)  the only route before it, on the same build: pb_index_map_i32 with weights into preallocated buffers, the chroma index maps and
       weights of the anchors derived from it on the device (tensor arithmetic), and pb_gather_blend_u8 once per plane (the pair plane of
       NV12 / P010 as one two-channel image) - measured twice (A / A) for that figure's own spread.  It writes uint8 whatever the sample;
  (c)  pb_remap_u8 on the same plan, as the RGB8 yardstick.
Fill (0, 0, 0).  Exit status 1 when the bytes of (a) and (b) differ (8-bit formats), or when (a) is not faster than (b) by more than (b)'s
own A / A spread.  How (a) stands against (c) is recorded, not required."""

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


def chroma_maps(idx2, w2, w, cx, cy):
    """The anchors' taps into the (h >> cy, w >> cx) plane (-1 where black) and their factors: (2, H >> cy, W >> cx) each."""
    a = idx2[:, 0 :: 1 << cy, 0 :: 1 << cx]
    r, c = torch.div(a, w, rounding_mode="floor"), torch.remainder(a, w)
    return torch.where(a < 0, a, (r >> cy) * (w >> cx) + (c >> cx)).contiguous(), w2[:, 0 :: 1 << cy, 0 :: 1 << cx].contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--formats", default="nv12,p010,yuv420p,yuv444p")
    ap.add_argument("--case", default="c5_195")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    stream = torch.cuda.current_stream()
    st = nat.current_stream()
    L = nat.load()
    res = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "iters": args.iters, "case": args.case, "rows": []}
    failures = []
    zero = (nat.C.c_uint16 * 3)(0, 0, 0)
    case = next(c for c in full_cases() if c.name == args.case)
    plan = H.pb_plan_private(case, bilinear=False)
    _, h, w, *_ = case.src
    Hd, Wd = case.dst[1], case.dst[2]
    res["tile_mix"] = plan.stitch_tile_mix()
    idx2 = torch.empty((2, Hd, Wd), dtype=torch.int32, device="cuda")
    w2 = torch.empty((2, Hd, Wd), dtype=torch.float64, device="cuda")
    rgb = torch.randint(0, 256, (h, w, 3), dtype=torch.uint8, device="cuda")
    rgb_out = torch.empty((Hd, Wd, 3), dtype=torch.uint8, device="cuda")
    for fmt in args.formats.split(","):
        dt, fam, _ = nat.VIDEO_FORMATS[fmt]
        S = dt.itemsize
        cx, cy = (1, 1) if fam.pairs else ((fam.sub != nat.PLANAR_444) * 1, (fam.sub == nat.PLANAR_420) * 1)
        n0, nc = h * w, (h >> cy) * (w >> cx)
        N0, NC = Hd * Wd, (Hd >> cy) * (Wd >> cx)
        assert plan.stitch_nv12_supported(S) if fam.pairs else plan.stitch_planar_supported(fam.sub, S)
        src = torch.randint(0, 256, ((n0 + 2 * nc) * S,), dtype=torch.uint8, device="cuda")
        out_a = torch.empty(((N0 + 2 * NC) * S,), dtype=torch.uint8, device="cuda")
        out_b = torch.zeros((N0 + 2 * NC,), dtype=torch.uint8, device="cuda")  # (pb_gather_blend_u8 writes uint8)

        def a():
            if fam.pairs:
                nat.check(L.pb_stitch_nv12(plan.handle, src.data_ptr(), out_a.data_ptr(), 1, None, None, S, nat.C.addressof(zero), st))
            else:
                nat.check(L.pb_stitch_planar(plan.handle, src.data_ptr(), out_a.data_ptr(), 1, None, None, fam.sub, S, nat.C.addressof(zero), st))

        def b():
            nat.check(L.pb_index_map_i32(plan.handle, idx2.data_ptr(), w2.data_ptr(), st))
            nat.check(L.pb_gather_blend_u8(idx2.data_ptr(), w2.data_ptr(), src.data_ptr(), out_b.data_ptr(), N0, 1, S, st))
            ci, cw = (idx2, w2) if (cx, cy) == (0, 0) else chroma_maps(idx2, w2, w, cx, cy)
            if fam.pairs:
                nat.check(L.pb_gather_blend_u8(ci.data_ptr(), cw.data_ptr(), src.data_ptr() + n0 * S, out_b.data_ptr() + N0, NC, 2, S, st))
            else:
                for k in (0, 1):
                    nat.check(L.pb_gather_blend_u8(ci.data_ptr(), cw.data_ptr(), src.data_ptr() + (n0 + k * nc) * S, out_b.data_ptr() + N0 + k * NC, NC, 1, S, st))

        def c():
            nat.check(L.pb_remap_u8(plan.handle, rgb.data_ptr(), rgb_out.data_ptr(), 1, 0, 0, st))

        a()
        b()
        torch.cuda.synchronize()
        equal = bool(torch.equal(out_a, out_b)) if S == 1 else None
        t = alternate({"b_1": b, "a": a, "c": c, "b_2": b}, args.reps, args.iters, stream)
        b_all = t["b_1"]["us_all"] + t["b_2"]["us_all"]
        b_med, b_spread = statistics.median(b_all), max(b_all) - min(b_all)
        row = {"format": fmt, "bytes_per_sample": S, "bytes_equal": equal, "a_stitch": t["a"], "b_index_map_gather_blend_1": t["b_1"], "b_index_map_gather_blend_2": t["b_2"],
               "b_us": round(b_med, 1), "b_spread_us": round(b_spread, 1), "c_remap_u8": t["c"], "b_over_a": round(b_med / t["a"]["us"], 2),
               "a_over_c": round(t["a"]["us"] / t["c"]["us"], 2), "a_GBps_out": round((N0 + 2 * NC) * S / t["a"]["us"] * 1e-3, 1)}
        res["rows"].append(row)
        print(json.dumps(row), flush=True)
        if equal is False:
            failures.append(f"{fmt}: the stitch launch's bytes differ from pb_index_map_i32 + pb_gather_blend_u8's")
        if not t["a"]["us"] < b_med - b_spread:
            failures.append(f"{fmt}: the stitch launch ({t['a']['us']} us) is not faster than the index-map route ({b_med:.1f} us) beyond its spread ({b_spread:.1f} us)")
        del src, out_a, out_b
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
