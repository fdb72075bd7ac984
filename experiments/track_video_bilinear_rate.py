#!/usr/bin/env python3
"""The rate of the bilinear rotation tracks for video frames (pb_remap_track_planar_bilinear / pb_remap_track_nv12_bilinear)
against what the library offered before, in ONE process, warm, the ways alternating: medians of `reps` rounds of `iters` batches, after a
warm-up batch (the protocol of experiments/rotation_track_rate.py).
    python experiments/track_video_bilinear_rate.py [--reps 5] [--iters 20] [--frames 16] [--geometries c2,stab] [--formats ...] [--out file.json]
Geometries: c2 = an 8192 x 4096 panorama -> 4096^2 equidistant-360; stab = a 4096 x 2048 panorama -> the same size panorama (stabilisation).
Formats: yuv420p, nv12, yuv444p, p010.  N distinct random frames, N distinct random rotations.  Per frame of a batch, in us:
  (a)  one bilinear tracked launch over the N frames: between two HIP events on the launch stream, and by the host's clock;
  (n)  the nearest tracked call on the same data, between events: (a) / (n) says what interpolation costs on a kernel bound by float64
       transcendentals - recorded, not required;
  (b)  the only route to smooth tracked video before: per frame a PREPARED plan of the whole chain with the bilinear mode's tables
       (pb_plan_create, bilinear=True), then pb_remap_planar_bilinear / pb_remap_nv12_bilinear - the host's clock around the N plan
       creations, the N launches and the stream's synchronise, taken twice (A / A) for its own spread.
Fill (0, 0, 0).  Exit status 1 when (a)'s wall time per frame does not beat (b)'s by more than (b)'s A / A spread at yuv420p or nv12, or
when (a) and (b) - the exact kernel and the tile kernel - differ by more than T(R) = 1 + R // 512 anywhere outside the edge band of DESIGN
3.18 (where exactly one of the two is fill), or that band holds more pixels than the geometry allows (none for a panorama source, which
has no liveness edge).  Nothing else is judged."""

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
from photonbend_amd.core import rotation_track  # noqa: E402

import photonbend_amd as pb  # noqa: E402


# (geometry, events_us and wall_us are experiments/rotation_track_rate.py's, which parses its command line on import)
def geometry(name):
    """-> (pb_proj dst, pb_proj src)"""
    if name == "c2":
        dst = pb.CameraImage(np.zeros((4096, 4096, 3), np.uint8), pb.utils.to_radians(360), pb.equidistant(), magnitude=4096 / 2 - 0.5)
        src = pb.PanoramaImage(np.zeros((4096, 8192, 3), np.uint8))
    elif name == "stab":
        dst = pb.PanoramaImage(np.zeros((2048, 4096, 3), np.uint8))
        src = pb.PanoramaImage(np.zeros((2048, 4096, 3), np.uint8))
    else:
        raise KeyError(name)
    return dst._proj_ss(1), src._proj("src")


def events_us(fn, iters, stream):
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


# name -> (bytes per sample, subsampling, interleaved pairs)
FORMATS = {"yuv420p": (1, nat.PLANAR_420, False), "nv12": (1, nat.PLANAR_420, True), "yuv444p": (1, nat.PLANAR_444, False), "p010": (2, nat.PLANAR_420, True)}
REQUIRED = ("yuv420p", "nv12")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--geometries", default="c2,stab")
    ap.add_argument("--formats", default=",".join(FORMATS))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    stream, st, L, C = torch.cuda.current_stream(), nat.current_stream(), nat.load(), nat.C
    n = args.frames
    mats = rotation_track(np.random.default_rng(7).uniform(-np.pi, np.pi, (n, 3)))
    table = torch.from_numpy(mats).cuda()
    zero = (C.c_uint16 * 3)(0, 0, 0)
    fz = C.addressof(zero)
    res = {"device": torch.cuda.get_device_name(0), "library": nat.LIB_PATH, "reps": args.reps, "iters": args.iters, "frames": n, "rows": []}
    failures = []
    for name in args.geometries.split(","):
        dstp, srcp = geometry(name)
        h, w, Hd, Wd = srcp.height, srcp.width, dstp.height, dstp.width
        base = nat.Plan(dstp, [], srcp, defer=True)
        band_bound = 0 if srcp.kind == nat.KIND_PANO else None  # (a panorama source has no liveness edge: DESIGN 3.18's band is empty)
        for fmt in args.formats.split(","):
            S, sub, pairs = FORMATS[fmt]
            n_src, n_dst = nat.planar_frame_samples(h, w, sub) * S, nat.planar_frame_samples(Hd, Wd, sub) * S
            src = torch.randint(0, 256, (n, n_src), dtype=torch.uint8, device="cuda")
            out_a, out_n, out_b = (torch.zeros((n, n_dst), dtype=torch.uint8, device="cuda") for _ in range(3))

            def a():
                if pairs:
                    nat.check(L.pb_remap_track_nv12_bilinear(base.handle, table.data_ptr(), 1, src.data_ptr(), out_a.data_ptr(), n, None, None, S, fz, st))
                else:
                    nat.check(L.pb_remap_track_planar_bilinear(base.handle, table.data_ptr(), 1, src.data_ptr(), out_a.data_ptr(), n, None, None, sub, S, fz, st))

            def nearest():
                if pairs:
                    nat.check(L.pb_remap_track_nv12(base.handle, table.data_ptr(), 1, src.data_ptr(), out_n.data_ptr(), n, None, None, S, fz, st))
                else:
                    nat.check(L.pb_remap_track_planar(base.handle, table.data_ptr(), 1, src.data_ptr(), out_n.data_ptr(), n, None, None, sub, S, fz, st))

            def b_whole():
                for f in range(n):
                    p = nat.Plan(dstp, [mats[f]], srcp, bilinear=True)
                    if pairs:
                        nat.check(L.pb_remap_nv12_bilinear(p.handle, src[f].data_ptr(), out_b[f].data_ptr(), 1, None, None, S, fz, st))
                    else:
                        nat.check(L.pb_remap_planar_bilinear(p.handle, src[f].data_ptr(), out_b[f].data_ptr(), 1, None, None, sub, S, fz, st))

            a()
            b_whole()
            torch.cuda.synchronize()
            T = 1 + (255 if S == 1 else 65535) // 512
            dtv = torch.uint8 if S == 1 else torch.int16
            ga, gb = out_a.view(dtv).to(torch.int32) & 0xFFFF, out_b.view(dtv).to(torch.int32) & 0xFFFF
            d = (ga - gb).abs()
            flips = (ga == 0) != (gb == 0)  # (fill in exactly one of the two: the edge band)
            beyond, band = int(((d > T) & ~flips).sum()), int(((d > T) & flips).sum())
            row = {"geometry": name, "pixel_format": fmt, "bytes_per_sample": S, "T": T, "max_abs_diff_outside_band": int(d[~flips].max()), "samples_beyond_T": beyond,
                   "band_samples": band, "band_bound": band_bound, "samples_differing": int((d != 0).sum()), "samples": int(d.numel())}
            del ga, gb, d, flips
            if beyond:
                failures.append(f"{name} {fmt}: {beyond} samples of the exact launch and the tile kernel differ by more than T = {T} outside the edge band")
            if band_bound is not None and band > band_bound:
                failures.append(f"{name} {fmt}: {band} samples are fill in exactly one of the two, the geometry allows {band_bound}")
            kernel = {k: [] for k in ("a", "n")}
            wall = {k: [] for k in ("b_1", "a", "b_2")}
            for _ in range(args.reps):
                wall["b_1"].append(wall_us(b_whole, args.iters) / n)
                kernel["a"].append(events_us(a, args.iters, stream) / n)
                kernel["n"].append(events_us(nearest, args.iters, stream) / n)
                wall["a"].append(wall_us(a, args.iters) / n)
                wall["b_2"].append(wall_us(b_whole, args.iters) / n)
            med = lambda v: round(statistics.median(v), 2)  # noqa: E731
            wb = wall["b_1"] + wall["b_2"]
            wb_spread = max(wb) - min(wb)
            row.update({"kernel_us_per_frame": {k: {"median": med(v), "all": [round(t, 2) for t in v]} for k, v in kernel.items()},
                        "wall_us_per_frame": {k: {"median": med(v), "all": [round(t, 2) for t in v]} for k, v in wall.items()},
                        "b_wall_us": med(wb), "b_wall_spread_us": round(wb_spread, 2), "a_over_n_kernel": round(med(kernel["a"]) / med(kernel["n"]), 3),
                        "b_over_a_wall": round(med(wb) / med(wall["a"]), 2), "a_GBps_out": round(n_dst / med(kernel["a"]) * 1e-3, 1)})
            res["rows"].append(row)
            print(json.dumps(row), flush=True)
            if fmt in REQUIRED and not med(wall["a"]) < med(wb) - wb_spread:
                failures.append(f"{name} {fmt}: the tracked launch ({med(wall['a'])} us per frame) does not beat a prepared plan per frame ({med(wb)} us) by more than "
                                f"its spread ({wb_spread:.2f} us)")
            del src, out_a, out_n, out_b
            torch.cuda.empty_cache()
        del base
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    for msg in failures:
        print("FAILED: " + msg, file=sys.stderr)
    sys.exit(1 if failures else 0)


if __name__ == "__main__":
    main()
