#!/usr/bin/env python3
"""The rate of pb_remap_track_nv12 against what the library offered before, in ONE process, warm, the ways alternating: medians
of `reps` rounds of `iters` batches between two HIP events on the launch stream, after a warm-up batch.
    python experiments/track_nv12_rate.py [--reps 5] [--iters 20] [--frames 16] [--geometries c2,stab] [--out file.json]
Geometries (experiments/rotation_track_rate.py's): c2 = an 8192 x 4096 panorama -> 4096^2 equidistant-360; stab = a 4096 x 2048 panorama ->
the same size panorama (stabilisation).  Both sample sizes.  N distinct random frames, N distinct rotations.  Per frame of a batch:
  (a)  one pb_remap_track_nv12 over the N frames;
  (b)  the equal-bytes route there was before, per frame: a deferred plan of that frame's rotation (made beforehand: its creation is not in
       the figure), pb_index_map_i32, pb_gather_px of luma, the anchors' chroma index, pb_gather_px of the pairs - taken twice (A / A) for
       its own spread;
  (c)  per frame a PREPARED plan (pb_plan_create) and pb_remap_nv12: wall time, plan creation included;
  (d)  pb_remap_track_u8 on the same geometry, RGB8 frames: the yardstick (the same float64 chain, 3 bytes per pixel instead of 1.5 S).
Fill (0, 0, 0), so that (a) and (b) write the same bytes.  Exit status 1 when (a)'s bytes differ from (b)'s, or when (a) is not faster than
(b) by more than the A / A spread of (b) in the same run."""

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

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from nv12_rate import chroma_index  # noqa: E402
from pixel_format_rate import alternate  # noqa: E402


def geometry(name):
    """-> (pb_proj dst, pb_proj src): experiments/rotation_track_rate.py's c2 and stab"""
    import photonbend_amd as pb

    if name == "c2":
        dst = pb.CameraImage(np.zeros((4096, 4096, 3), np.uint8), pb.utils.to_radians(360), pb.equidistant(), magnitude=4096 / 2 - 0.5)
        src = pb.PanoramaImage(np.zeros((4096, 8192, 3), np.uint8))
    elif name == "stab":
        dst = pb.PanoramaImage(np.zeros((2048, 4096, 3), np.uint8))
        src = pb.PanoramaImage(np.zeros((2048, 4096, 3), np.uint8))
    else:
        raise KeyError(name)
    return dst._proj_ss(1), src._proj("src")


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
    ap.add_argument("--geometries", default="c2,stab")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    stream, st, L = torch.cuda.current_stream(), nat.current_stream(), nat.load()
    n = args.frames
    mats = rotation_track(np.random.default_rng(7).uniform(-np.pi, np.pi, (n, 3)))
    table = torch.from_numpy(mats).cuda()
    zero = (nat.C.c_uint16 * 3)(0, 0, 0)
    res = {"device": torch.cuda.get_device_name(0), "library": nat.LIB_PATH, "reps": args.reps, "iters": args.iters, "frames": n, "rows": []}
    failures = []
    for name in args.geometries.split(","):
        dstp, srcp = geometry(name)
        h, w, Hd, Wd = srcp.height, srcp.width, dstp.height, dstp.width
        base = nat.Plan(dstp, [], srcp, defer=True)
        made = [nat.Plan(dstp, [mats[f]], srcp, defer=True) for f in range(n)]
        idx = torch.empty((Hd, Wd), dtype=torch.int32, device="cuda")
        rgb = torch.randint(0, 256, (n, h, w, 3), dtype=torch.uint8, device="cuda")
        rgb_out = torch.empty((n, Hd, Wd, 3), dtype=torch.uint8, device="cuda")

        def d():
            nat.check(L.pb_remap_track_u8(base.handle, table.data_ptr(), 1, 0, rgb.data_ptr(), rgb_out.data_ptr(), n, 0, 0, st))

        for S in (1, 2):
            fs, fd = 3 * h * w * S // 2, 3 * Hd * Wd * S // 2  # bytes of a packed frame
            src = torch.randint(0, 256, (n, fs), dtype=torch.uint8, device="cuda")
            out_a = torch.zeros((n, fd), dtype=torch.uint8, device="cuda")
            out_b, out_c = torch.zeros_like(out_a), torch.zeros_like(out_a)
            n_pairs = Hd * Wd // 4

            def a():
                nat.check(L.pb_remap_track_nv12(base.handle, table.data_ptr(), 1, src.data_ptr(), out_a.data_ptr(), n, None, None, S, nat.C.addressof(zero), st))

            def b():
                for f in range(n):
                    s, o = src[f].data_ptr(), out_b[f].data_ptr()
                    nat.check(L.pb_index_map_i32(made[f].handle, idx.data_ptr(), None, st))
                    nat.check(L.pb_gather_px(idx.data_ptr(), s, o, Hd * Wd, S, st))
                    ci = chroma_index(idx, w)
                    nat.check(L.pb_gather_px(ci.data_ptr(), s + h * w * S, o + Hd * Wd * S, n_pairs, 2 * S, st))

            def c():
                for f in range(n):
                    p = nat.Plan(dstp, [mats[f]], srcp, bilinear=False)
                    nat.check(L.pb_remap_nv12(p.handle, src[f].data_ptr(), out_c[f].data_ptr(), 1, None, None, S, nat.C.addressof(zero), st))

            a()
            b()
            torch.cuda.synchronize()
            equal = bool(torch.equal(out_a, out_b))
            t = alternate({"b_1": b, "a": a, "d": d, "b_2": b}, args.reps, args.iters, stream)
            c_wall = [wall_us(c, max(1, args.iters // 10)) / n for _ in range(args.reps)]
            a_wall = [wall_us(a, args.iters) / n for _ in range(args.reps)]
            b_all = [v / n for v in t["b_1"]["us_all"] + t["b_2"]["us_all"]]
            b_med, b_spread = statistics.median(b_all), max(b_all) - min(b_all)
            a_us, d_us = t["a"]["us"] / n, t["d"]["us"] / n
            row = {"geometry": name, "bytes_per_sample": S, "bytes_equal": equal, "us_per_frame": {
                       "a_track_nv12": round(a_us, 1), "a_all": [round(v / n, 1) for v in t["a"]["us_all"]], "b_index_map_two_gathers": round(b_med, 1),
                       "b_all": [round(v, 1) for v in b_all], "b_spread": round(b_spread, 1), "d_track_u8": round(d_us, 1),
                       "d_all": [round(v / n, 1) for v in t["d"]["us_all"]], "c_wall_plan_per_frame_nv12": round(statistics.median(c_wall), 1),
                       "a_wall": round(statistics.median(a_wall), 1)},
                   "b_over_a": round(b_med / a_us, 2), "a_over_d": round(a_us / d_us, 2), "c_wall_over_a_wall": round(statistics.median(c_wall) / statistics.median(a_wall), 2)}
            res["rows"].append(row)
            print(json.dumps(row), flush=True)
            if not equal:
                failures.append(f"{name} S={S}: pb_remap_track_nv12's bytes differ from the index map + two gathers'")
            if not a_us < b_med - b_spread:
                failures.append(f"{name} S={S}: pb_remap_track_nv12 ({a_us:.1f} us per frame) is not faster than the route before ({b_med:.1f} us) beyond its spread ({b_spread:.1f} us)")
            del src, out_a, out_b, out_c
        del rgb, rgb_out, idx, made, base
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
