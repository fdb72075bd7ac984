#!/usr/bin/env python3
"""The rate of pb_remap_track_u8 against what the library offered before, in ONE process, warm, the ways alternating: medians
of `reps` rounds of `iters` batches between two HIP events on the launch stream, after a warm-up batch.
    python experiments/rotation_track_rate.py [--reps 5] [--iters 20] [--frames 16] [--geometries c2,stab] [--sweep 1,2,4,8] [--out file.json]
Geometries: c2 = an 8192 x 4096 panorama -> 4096^2 equidistant-360; stab = a 4096 x 2048 panorama -> the same size panorama (stabilisation);
fish / cube / dfe = a fisheye, a cube map, a double fisheye -> a 4096 x 2048 panorama (the other source kinds: for A/B builds of the kernel,
loaded through PB_LIB_PATH).
N distinct frames, N distinct rotations.  Per frame of a batch:
  (a)  one pb_remap_track_u8 over the N frames;
  (b)  per frame a deferred pb_plan_create with that rotation, then pb_remap_u8 (the float64 kernel): one launch per frame - taken twice
       (A / A) for its own spread.  Kernel time: the N launches of plans made beforehand, between events; wall time: host clock around plan
       creation + launch for the N frames and the stream's synchronise;
  (c)  for reference only: per frame a PREPARED plan (pb_plan_create) and the tile kernel, wall time.
--sweep: the candidates for PB_TRACK_FRAMES (frames a work-item loops over), timed in the same alternation through the diagnostic build's
knob of that name (build/libphotonbend_hip_diag.so, loaded through PB_LIB_PATH unless the caller names another library).
Exit status 1 when (a)'s bytes differ from (b)'s, when (a)'s kernel time per frame exceeds (b)'s by more than (b)'s A / A spread, or when
(a)'s wall time per frame is not below (b)'s."""

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
    ap.add_argument("--geometries", default="c2,stab")
    ap.add_argument("--sweep", default="")
    ap.add_argument("--out", default=None)
    return ap.parse_args()


ARGS = parse()
SWEEP = [int(v) for v in ARGS.sweep.split(",") if v]
if SWEEP and not os.environ.get("PB_LIB_PATH"):
    os.environ["PB_LIB_PATH"] = os.path.join(ROOT, "build", "libphotonbend_hip_diag.so")

import numpy as np  # noqa: E402
import torch  # noqa: E402

import photonbend_amd as pb  # noqa: E402
from photonbend_amd import _native as nat  # noqa: E402
from photonbend_amd.core import rotation_track  # noqa: E402


def geometry(name):
    """-> (pb_proj dst, pb_proj src)"""
    if name == "c2":
        dst = pb.CameraImage(np.zeros((4096, 4096, 3), np.uint8), pb.utils.to_radians(360), pb.equidistant(), magnitude=4096 / 2 - 0.5)
        src = pb.PanoramaImage(np.zeros((4096, 8192, 3), np.uint8))
    elif name == "stab":
        dst = pb.PanoramaImage(np.zeros((2048, 4096, 3), np.uint8))
        src = pb.PanoramaImage(np.zeros((2048, 4096, 3), np.uint8))
    elif name == "fish":  # a fisheye source: 4096^2 equisolid 190 degrees -> a 4096 x 2048 panorama (a turntable)
        dst = pb.PanoramaImage(np.zeros((2048, 4096, 3), np.uint8))
        src = pb.CameraImage(np.zeros((4096, 4096, 3), np.uint8), pb.utils.to_radians(190), pb.equisolid(), magnitude=4096 / 2 - 0.5)
    elif name == "cube":  # a cube map of 1024-pixel faces -> a 4096 x 2048 panorama
        dst = pb.PanoramaImage(np.zeros((2048, 4096, 3), np.uint8))
        src = pb.CubemapImage(np.zeros((2048, 3072, 3), np.uint8))
    elif name == "dfe":  # a 195-degree double fisheye -> a 4096 x 2048 panorama
        dst = pb.PanoramaImage(np.zeros((2048, 4096, 3), np.uint8))
        src = pb.DoubleCameraImage(np.zeros((2048, 4096, 3), np.uint8), pb.utils.to_radians(195), pb.equidistant())
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
    res = {"device": torch.cuda.get_device_name(0), "library": nat.LIB_PATH, "reps": args.reps, "iters": args.iters, "frames": n, "rows": []}
    failures = []
    for name in args.geometries.split(","):
        dstp, srcp = geometry(name)
        src = torch.randint(0, 256, (n, srcp.height, srcp.width, 3), dtype=torch.uint8, device="cuda")
        out_a = torch.zeros((n, dstp.height, dstp.width, 3), dtype=torch.uint8, device="cuda")
        out_b = torch.zeros_like(out_a)
        base = nat.Plan(dstp, [], srcp, defer=True)
        made = [nat.Plan(dstp, [mats[f]], srcp, defer=True) for f in range(n)]

        def a():
            nat.check(L.pb_remap_track_u8(base.handle, table.data_ptr(), 1, 0, src.data_ptr(), out_a.data_ptr(), n, 0, 0, st))

        def b_kernels():
            for f in range(n):
                nat.check(L.pb_remap_u8(made[f].handle, src[f].data_ptr(), out_b[f].data_ptr(), 1, 0, 0, st))

        def b_whole():
            for f in range(n):
                p = nat.Plan(dstp, [mats[f]], srcp, defer=True)
                nat.check(L.pb_remap_u8(p.handle, src[f].data_ptr(), out_b[f].data_ptr(), 1, 0, 0, st))

        def c_whole():
            for f in range(n):
                p = nat.Plan(dstp, [mats[f]], srcp, bilinear=False)
                nat.check(L.pb_remap_u8(p.handle, src[f].data_ptr(), out_b[f].data_ptr(), 1, 0, 0, st))

        def a_with(F):
            def run():
                os.environ["PB_TRACK_FRAMES"] = str(F)
                a()
            return run

        os.environ.pop("PB_TRACK_FRAMES", None)
        a()
        b_kernels()
        torch.cuda.synchronize()
        equal = bool(torch.equal(out_a, out_b))
        for F in SWEEP:  # every candidate writes the same bytes
            out_a.zero_()
            a_with(F)()
            torch.cuda.synchronize()
            equal = equal and bool(torch.equal(out_a, out_b))
        os.environ.pop("PB_TRACK_FRAMES", None)
        kernel = {k: [] for k in ["b_1", "a", "b_2"] + [f"a_F{F}" for F in SWEEP]}
        wall = {k: [] for k in ("b_1", "a", "c", "b_2")}
        for _ in range(args.reps):
            kernel["b_1"].append(events_us(b_kernels, args.iters, stream) / n)
            os.environ.pop("PB_TRACK_FRAMES", None)
            kernel["a"].append(events_us(a, args.iters, stream) / n)
            for F in SWEEP:
                kernel[f"a_F{F}"].append(events_us(a_with(F), args.iters, stream) / n)
            os.environ.pop("PB_TRACK_FRAMES", None)
            kernel["b_2"].append(events_us(b_kernels, args.iters, stream) / n)
            wall["b_1"].append(wall_us(b_whole, args.iters) / n)
            wall["a"].append(wall_us(a, args.iters) / n)
            wall["c"].append(wall_us(c_whole, max(1, args.iters // 4)) / n)
            wall["b_2"].append(wall_us(b_whole, args.iters) / n)
        med = lambda v: round(statistics.median(v), 2)  # noqa: E731
        kb, wb = kernel["b_1"] + kernel["b_2"], wall["b_1"] + wall["b_2"]
        kb_spread = max(kb) - min(kb)
        row = {"geometry": name, "bytes_equal": equal,
               "kernel_us_per_frame": {k: {"median": med(v), "all": [round(t, 2) for t in v]} for k, v in kernel.items()},
               "wall_us_per_frame": {k: {"median": med(v), "all": [round(t, 2) for t in v]} for k, v in wall.items()},
               "b_kernel_us": med(kb), "b_kernel_spread_us": round(kb_spread, 2), "b_wall_us": med(wb),
               "a_over_b_kernel": round(med(kernel["a"]) / med(kb), 3), "a_over_b_wall": round(med(wall["a"]) / med(wb), 3)}
        res["rows"].append(row)
        print(json.dumps(row), flush=True)
        if not equal:
            failures.append(f"{name}: the track's bytes differ from the per-frame plans'")
        if med(kernel["a"]) > med(kb) + kb_spread:
            failures.append(f"{name}: the track's kernel time per frame ({med(kernel['a'])} us) exceeds the per-frame launches' ({med(kb)} us) by more than their spread ({kb_spread:.2f} us)")
        if not med(wall["a"]) < med(wb):
            failures.append(f"{name}: the track's wall time per frame ({med(wall['a'])} us) is not below the per-frame plans' ({med(wb)} us)")
        del src, out_a, out_b, made, base
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
