#!/usr/bin/env python3
"""The rate of pb_track_stitch_nv12 / pb_track_stitch_planar against what the library offered before, in ONE process, warm,
the ways alternating: medians of `reps` rounds of `iters` batches between two HIP events on the launch stream, after a warm-up batch
(experiments/rotation_track_rate.py's and stitch_video_rate.py's protocol).
    python experiments/stitch_track_rate.py [--reps 5] [--iters 20] [--frames 16] [--formats nv12,p010,yuv420p,yuv444p] [--out file.json]
Geometry: a 7776 x 3888 double fisheye at 195 degrees -> a 4096 x 2048 panorama.  N distinct frames, N distinct rotations.  Per format,
time per frame of
  (a)  the new launch: pb_track_stitch_kernel over the N frames, every plane;
  (b)  the only route without a plan per frame before it, on the same build: per frame a deferred plan's pb_index_map_i32 with weights
       into preallocated buffers, the chroma index maps and weights of the anchors derived from it on the device (tensor arithmetic), and
       pb_gather_blend_u8 once per plane (the pair plane of NV12 / P010 as one two-channel image) - measured twice (A / A) for that
       figure's own spread.  It writes uint8 whatever the sample.  The deferred plans are made beforehand: their creation is not timed;
  (c)  per frame a PREPARED plan of the whole chain plus pb_stitch_nv12 / pb_stitch_planar: WALL time, pb_plan_create included;
  (d)  pb_remap_track_u8 over N RGB8 frames of the same geometry: the same float64 chain and taps, as the yardstick.
Fill (0, 0, 0).  Exit status 1 when the bytes of (a) differ from (b)'s (8-bit formats) or from (c)'s.  How (a) stands against (b), (c)
and (d) is recorded, not required: nothing is fixed in advance."""

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

import photonbend_amd as pb  # noqa: E402
from photonbend_amd import _native as nat  # noqa: E402
from photonbend_amd.core import rotation_track  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from stitch_video_rate import chroma_maps  # noqa: E402

SRC_HW, DST_HW, FOV = (3888, 7776), (2048, 4096), 195


def events_us(fn, iters, stream):  # (rotation_track_rate.py's, which parses its own command line on import)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    a.record(stream)
    for _ in range(iters):
        fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def wall_us(fn, iters):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--formats", default="nv12,p010,yuv420p,yuv444p")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    stream, st, L = torch.cuda.current_stream(), nat.current_stream(), nat.load()
    n = args.frames
    (h, w), (Hd, Wd) = SRC_HW, DST_HW
    mats = rotation_track(np.random.default_rng(7).uniform(-np.pi, np.pi, (n, 3)))
    table = torch.from_numpy(mats).cuda()
    dstp = pb.PanoramaImage(np.zeros((Hd, Wd, 3), np.uint8))._proj_ss(1)
    srcp = pb.DoubleCameraImage(np.zeros((h, w, 3), np.uint8), pb.utils.to_radians(FOV), pb.equidistant())._proj("src")
    base = nat.Plan(dstp, [], srcp, defer=True)
    made = [nat.Plan(dstp, [mats[f]], srcp, defer=True) for f in range(n)]
    zero = (nat.C.c_uint16 * 3)(0, 0, 0)
    idx2 = torch.empty((2, Hd, Wd), dtype=torch.int32, device="cuda")
    w2 = torch.empty((2, Hd, Wd), dtype=torch.float64, device="cuda")
    res = {"device": torch.cuda.get_device_name(0), "library": nat.LIB_PATH, "reps": args.reps, "iters": args.iters, "frames": n,
           "geometry": f"{w} x {h} double fisheye at {FOV} degrees -> {Wd} x {Hd} panorama", "rows": []}
    failures = []

    # (d): the RGB8 track of the same geometry, timed once per format round like the other ways
    rgb = torch.randint(0, 256, (n, h, w, 3), dtype=torch.uint8, device="cuda")
    rgb_out = torch.empty((n, Hd, Wd, 3), dtype=torch.uint8, device="cuda")

    def d():
        nat.check(L.pb_remap_track_u8(base.handle, table.data_ptr(), 1, 0, rgb.data_ptr(), rgb_out.data_ptr(), n, 0, 0, st))

    for fmt in args.formats.split(","):
        dt, fam, _ = nat.VIDEO_FORMATS[fmt]
        S = dt.itemsize
        cx, cy = (1, 1) if fam.pairs else ((fam.sub != nat.PLANAR_444) * 1, (fam.sub == nat.PLANAR_420) * 1)
        n0, nc = h * w, (h >> cy) * (w >> cx)
        N0, NC = Hd * Wd, (Hd >> cy) * (Wd >> cx)
        fs, fd = (n0 + 2 * nc) * S, (N0 + 2 * NC) * S  # bytes of a packed source / destination frame
        src = torch.randint(0, 256, (n * fs,), dtype=torch.uint8, device="cuda")
        out_a = torch.zeros((n * fd,), dtype=torch.uint8, device="cuda")
        out_b = torch.zeros((n * (N0 + 2 * NC),), dtype=torch.uint8, device="cuda")  # (pb_gather_blend_u8 writes uint8)
        out_c = torch.zeros((n * fd,), dtype=torch.uint8, device="cuda")

        def a():
            if fam.pairs:
                nat.check(L.pb_track_stitch_nv12(base.handle, table.data_ptr(), 1, src.data_ptr(), out_a.data_ptr(), n, None, None, S, nat.C.addressof(zero), st))
            else:
                nat.check(L.pb_track_stitch_planar(base.handle, table.data_ptr(), 1, src.data_ptr(), out_a.data_ptr(), n, None, None, fam.sub, S, nat.C.addressof(zero), st))

        def b():
            for f in range(n):
                s, o = src.data_ptr() + f * fs, out_b.data_ptr() + f * (N0 + 2 * NC)
                nat.check(L.pb_index_map_i32(made[f].handle, idx2.data_ptr(), w2.data_ptr(), st))
                nat.check(L.pb_gather_blend_u8(idx2.data_ptr(), w2.data_ptr(), s, o, N0, 1, S, st))
                ci, cw = (idx2, w2) if (cx, cy) == (0, 0) else chroma_maps(idx2, w2, w, cx, cy)
                if fam.pairs:
                    nat.check(L.pb_gather_blend_u8(ci.data_ptr(), cw.data_ptr(), s + n0 * S, o + N0, NC, 2, S, st))
                else:
                    for k in (0, 1):
                        nat.check(L.pb_gather_blend_u8(ci.data_ptr(), cw.data_ptr(), s + (n0 + k * nc) * S, o + N0 + k * NC, NC, 1, S, st))

        def c_whole():
            for f in range(n):
                p = nat.Plan(dstp, [mats[f]], srcp, bilinear=False)
                s, o = src.data_ptr() + f * fs, out_c.data_ptr() + f * fd
                if fam.pairs:
                    nat.check(L.pb_stitch_nv12(p.handle, s, o, 1, None, None, S, nat.C.addressof(zero), st))
                else:
                    nat.check(L.pb_stitch_planar(p.handle, s, o, 1, None, None, fam.sub, S, nat.C.addressof(zero), st))

        a()
        b()
        c_whole()
        torch.cuda.synchronize()
        equal_b = bool(torch.equal(out_a, out_b)) if S == 1 else None
        equal_c = bool(torch.equal(out_a, out_c))
        kernel = {k: [] for k in ("b_1", "a", "d", "b_2")}
        wall = {k: [] for k in ("a", "c")}
        for _ in range(args.reps):
            kernel["b_1"].append(events_us(b, args.iters, stream) / n)
            kernel["a"].append(events_us(a, args.iters, stream) / n)
            kernel["d"].append(events_us(d, args.iters, stream) / n)
            kernel["b_2"].append(events_us(b, args.iters, stream) / n)
            wall["a"].append(wall_us(a, args.iters) / n)
            wall["c"].append(wall_us(c_whole, max(1, args.iters // 4)) / n)
        med = lambda v: round(statistics.median(v), 2)  # noqa: E731
        kb = kernel["b_1"] + kernel["b_2"]
        row = {"format": fmt, "bytes_per_sample": S, "bytes_equal_b": equal_b, "bytes_equal_c": equal_c,
               "kernel_us_per_frame": {k: {"median": med(v), "all": [round(t, 2) for t in v]} for k, v in kernel.items()},
               "wall_us_per_frame": {k: {"median": med(v), "all": [round(t, 2) for t in v]} for k, v in wall.items()},
               "a_us": med(kernel["a"]), "b_us": med(kb), "b_spread_us": round(max(kb) - min(kb), 2), "c_wall_us": med(wall["c"]), "d_us": med(kernel["d"]),
               "b_over_a": round(med(kb) / med(kernel["a"]), 2), "c_wall_over_a_wall": round(med(wall["c"]) / med(wall["a"]), 2),
               "a_over_d": round(med(kernel["a"]) / med(kernel["d"]), 3), "a_GBps_out": round(fd / med(kernel["a"]) * 1e-3, 1)}
        res["rows"].append(row)
        print(json.dumps(row), flush=True)
        if equal_b is False:
            failures.append(f"{fmt}: the track launch's bytes differ from pb_index_map_i32 + pb_gather_blend_u8's")
        if not equal_c:
            failures.append(f"{fmt}: the track launch's bytes differ from the prepared plans' pb_stitch call's")
        del src, out_a, out_b, out_c
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
