#!/usr/bin/env python3
"""The rate of pb_remap_track_px against the only route the library had for a rotation per frame of grey, RGBA and 16-bit
frames, in ONE process, warm, the ways alternating: medians of `reps` rounds of `iters` batches between two HIP events on the launch
stream, after a warm-up batch.
    python experiments/track_px_rate.py [--reps 5] [--iters 20] [--frames 16] [--geometries stab,c2] [--out file.json]
Geometries: stab = a 4096 x 2048 panorama -> the same size panorama (stabilisation); c2 = an 8192 x 4096 panorama -> 4096^2 equidistant-360.
N distinct frames, N distinct rotations.  Rows: grey8, RGBA8, RGB16, RGBA16 nearest, RGBA8 bilinear.  Per frame of a batch, microseconds:
  (a)  one pb_remap_track_px over the N frames;
  (b)  per frame a deferred plan of the whole chain, pb_index_map_i32 into a preallocated buffer, pb_gather_px - the bilinear row:
       pb_coordmap_f64 + pb_rotate_f64 + pb_sample_map_bilinear_px into preallocated maps.  Taken twice (A / A) for its own spread.  Kernel
       time: the launches of plans made beforehand, between events; wall time: the host clock around plan creation + launches for the N
       frames and the stream's synchronise;
  (c)  pb_remap_track_u8 on the same geometry with RGB8 frames, twice (A / A): recorded, not required - whether the pixel size is free
       beside the float64 chain.
Exit status 1 when (a)'s bytes differ from (b)'s on any row, or when (a) is not faster than (b) by more than (b)'s A / A spread."""

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--geometries", default="stab,c2")
    ap.add_argument("--out", default=None)
    return ap.parse_args()


ARGS = parse()

import ctypes  # noqa: E402

import numpy as np  # noqa: E402
import torch  # noqa: E402

import photonbend_amd as pb  # noqa: E402
from photonbend_amd import _native as nat  # noqa: E402
from photonbend_amd.core import rotation_track  # noqa: E402

# name -> (channels, sample_bytes, interpolation)
ROWS = {"grey8": (1, 1, "nearest"), "rgba8": (4, 1, "nearest"), "rgb16": (3, 2, "nearest"), "rgba16": (4, 2, "nearest"), "rgba8_bilinear": (4, 1, "bilinear")}


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


def main():
    args = ARGS
    torch.cuda.set_device(0)
    stream, st, L = torch.cuda.current_stream(), nat.current_stream(), nat.load()
    n = args.frames
    rng = np.random.default_rng(7)
    mats = rotation_track(rng.uniform(-np.pi, np.pi, (n, 3)))
    table = torch.from_numpy(mats).cuda()
    mat_ptrs = [np.ascontiguousarray(mats[f]).ctypes.data_as(ctypes.POINTER(ctypes.c_double)) for f in range(n)]
    res = {"device": torch.cuda.get_device_name(0), "library": nat.LIB_PATH, "reps": args.reps, "iters": args.iters, "frames": n, "rows": []}
    failures = []
    med = lambda v: round(statistics.median(v), 2)  # noqa: E731
    for name in args.geometries.split(","):
        dstp, srcp = geometry(name)
        npx_d, npx_s = dstp.height * dstp.width, srcp.height * srcp.width
        base = nat.Plan(dstp, [], srcp, defer=True)
        made = [nat.Plan(dstp, [mats[f]], srcp, defer=True) for f in range(n)]
        idx = torch.empty((npx_d,), dtype=torch.int32, device="cuda")
        map0 = torch.empty((npx_d * 3,), dtype=torch.float64, device="cuda")
        map1 = torch.empty_like(map0)
        # (c): the RGB8 track on this geometry
        src3 = torch.randint(0, 256, (n, npx_s * 3), dtype=torch.uint8, device="cuda")
        out3 = torch.zeros((n, npx_d * 3), dtype=torch.uint8, device="cuda")

        def c():
            nat.check(L.pb_remap_track_u8(base.handle, table.data_ptr(), 1, 0, src3.data_ptr(), out3.data_ptr(), n, 0, 0, st))

        for row_name, (ch, sb, interp) in ROWS.items():
            B = ch * sb
            iid = nat.TRACK_INTERP_IDS[interp]
            src = torch.randint(0, 256, (n, npx_s * B), dtype=torch.uint8, device="cuda")
            out_a = torch.zeros((n, npx_d * B), dtype=torch.uint8, device="cuda")
            out_b = torch.zeros_like(out_a)

            def a():
                nat.check(L.pb_remap_track_px(base.handle, table.data_ptr(), 1, iid, src.data_ptr(), out_a.data_ptr(), n, 0, 0, ch, sb, st))

            def b_frame(plan, f):
                if interp == "nearest":
                    nat.check(L.pb_index_map_i32(plan.handle, idx.data_ptr(), None, st))
                    nat.check(L.pb_gather_px(idx.data_ptr(), src[f].data_ptr(), out_b[f].data_ptr(), npx_d, B, st))
                else:
                    nat.check(L.pb_coordmap_f64(ctypes.byref(dstp), map0.data_ptr(), st))
                    nat.check(L.pb_rotate_f64(mat_ptrs[f], map0.data_ptr(), map1.data_ptr(), dstp.height, dstp.width, st))
                    nat.check(L.pb_sample_map_bilinear_px(ctypes.byref(srcp), map1.data_ptr(), dstp.height, dstp.width, None, None, src[f].data_ptr(),
                                                          out_b[f].data_ptr(), ch, sb, st))

            def b_kernels():
                for f in range(n):
                    b_frame(made[f], f)

            def b_whole():
                for f in range(n):
                    b_frame(nat.Plan(dstp, [mats[f]], srcp, defer=True), f)

            a()
            b_kernels()
            torch.cuda.synchronize()
            equal = bool(torch.equal(out_a, out_b)) and bool(out_b.any())
            kernel = {k: [] for k in ("b_1", "a", "c_1", "b_2", "c_2")}
            wall = {k: [] for k in ("b_1", "a", "b_2")}
            for _ in range(args.reps):
                kernel["b_1"].append(events_us(b_kernels, args.iters, stream) / n)
                kernel["a"].append(events_us(a, args.iters, stream) / n)
                kernel["c_1"].append(events_us(c, args.iters, stream) / n)
                kernel["b_2"].append(events_us(b_kernels, args.iters, stream) / n)
                kernel["c_2"].append(events_us(c, args.iters, stream) / n)
                wall["b_1"].append(wall_us(b_whole, args.iters) / n)
                wall["a"].append(wall_us(a, args.iters) / n)
                wall["b_2"].append(wall_us(b_whole, args.iters) / n)
            kb, wb, kc = kernel["b_1"] + kernel["b_2"], wall["b_1"] + wall["b_2"], kernel["c_1"] + kernel["c_2"]
            kb_spread, wb_spread = abs(med(kernel["b_1"]) - med(kernel["b_2"])), abs(med(wall["b_1"]) - med(wall["b_2"]))
            kc_spread = abs(med(kernel["c_1"]) - med(kernel["c_2"]))
            row = {"geometry": name, "row": row_name, "channels": ch, "sample_bytes": sb, "interpolation": interp, "bytes_equal": equal,
                   "kernel_us_per_frame": {k: {"median": med(v), "all": [round(t, 2) for t in v]} for k, v in kernel.items()},
                   "wall_us_per_frame": {k: {"median": med(v), "all": [round(t, 2) for t in v]} for k, v in wall.items()},
                   "a_kernel_us": med(kernel["a"]), "a_wall_us": med(wall["a"]),
                   "b_kernel_us": med(kb), "b_kernel_spread_us": round(kb_spread, 2), "b_wall_us": med(wb), "b_wall_spread_us": round(wb_spread, 2),
                   "c_kernel_us": med(kc), "c_kernel_spread_us": round(kc_spread, 2),
                   "a_over_b_kernel": round(med(kernel["a"]) / med(kb), 3), "a_over_b_wall": round(med(wall["a"]) / med(wb), 3),
                   "a_over_c_kernel": round(med(kernel["a"]) / med(kc), 3),
                   "a_within_c_spread": bool(abs(med(kernel["a"]) - med(kc)) <= kc_spread)}
            res["rows"].append(row)
            print(json.dumps(row), flush=True)
            if not equal:
                failures.append(f"{name} {row_name}: the track's bytes differ from the per-frame route's (or every frame is black)")
            if not med(kernel["a"]) < med(kb) - kb_spread:
                failures.append(f"{name} {row_name}: the track's kernel time per frame ({med(kernel['a'])} us) is not below the per-frame route's ({med(kb)} us) by "
                                f"more than its A / A spread ({kb_spread:.2f} us)")
            if not med(wall["a"]) < med(wb) - wb_spread:
                failures.append(f"{name} {row_name}: the track's wall time per frame ({med(wall['a'])} us) is not below the per-frame route's ({med(wb)} us) by "
                                f"more than its A / A spread ({wb_spread:.2f} us)")
            del src, out_a, out_b
            torch.cuda.empty_cache()
        del src3, out3, made, base, idx, map0, map1
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
