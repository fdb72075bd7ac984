#!/usr/bin/env python3
"""What the host side of one video call costs - the argument checks of the C library and the Python in front of them - on the CPU: a
deferred plan (no device) and ``n_frames = 0``, so every check runs, explicit layouts are resolved and the fills stored, and nothing is
launched or looked at:
    python experiments/video_call_overhead.py [--tree DIR] [--repeats 5] [--calls 20000] [--warmup 2000]
Times pb_remap_nv12, pb_remap_planar (4:2:0), pb_remap_track_nv12 and pb_remap_track_planar_bilinear, each through ctypes alone (layouts
and fills built once) and through the matching ``Plan.launch_*`` method (which builds them per call).  Per repeat the median of `calls`
calls after `warmup`; prints one JSON line with, per call, the repeats' medians (us), their median and their spread (max - min).
``--tree DIR``: time the package of another checkout (its Python; PB_LIB_PATH names the library to load)."""

import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x1000  # a non-null "device pointer": with no frames nothing reads it
H, W = 1080, 1920


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20000)
    ap.add_argument("--warmup", type=int, default=2000)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    from photonbend_amd import _native as nat

    lib = nat.load()
    p = nat.make_proj(nat.KIND_PANO, H, W)
    plan = nat.Plan(p, [], p, defer=True)
    h = plan._h
    nv12 = (2048, 2048 * H, 2048 * H * 3 // 2)  # pitched rows
    planar = (2048, 1024, 2048 * H, 2048 * H + 1024 * (H // 2), 2048 * H * 3 // 2)
    ln, lp, fill = nat.pb_nv12_layout(*nv12), nat.pb_planar_layout(*planar), (C.c_uint16 * 3)(16, 128, 128)
    an, ap_, af = C.addressof(ln), C.addressof(lp), C.addressof(fill)
    sub = nat.PLANAR_420
    cases = {
        "pb_remap_nv12": lambda: lib.pb_remap_nv12(h, FAKE, FAKE, 0, an, an, 1, af, None),
        "pb_remap_planar": lambda: lib.pb_remap_planar(h, FAKE, FAKE, 0, ap_, ap_, sub, 1, af, None),
        "pb_remap_track_nv12": lambda: lib.pb_remap_track_nv12(h, FAKE, 1, FAKE, FAKE, 0, an, an, 1, af, None),
        "pb_remap_track_planar_bilinear": lambda: lib.pb_remap_track_planar_bilinear(h, FAKE, 1, FAKE, FAKE, 0, ap_, ap_, sub, 1, af, None),
        "Plan.launch_nv12": lambda: plan.launch_nv12(FAKE, FAKE, 0, 0, 1, (16, 128, 128), nv12, nv12),
        "Plan.launch_planar": lambda: plan.launch_planar(FAKE, FAKE, sub, 0, 0, 1, (16, 128, 128), planar, planar),
        "Plan.launch_track_nv12": lambda: plan.launch_track_nv12(FAKE, 1, FAKE, FAKE, 0, 0, 1, (16, 128, 128), nv12, nv12),
        "Plan.launch_track_planar(bilinear)": lambda: plan.launch_track_planar(FAKE, 1, FAKE, FAKE, sub, 0, 0, 1, (16, 128, 128), planar, planar,
                                                                               interpolation="bilinear"),
    }
    out = {"package": os.path.dirname(nat.__file__), "library": nat.LIB_PATH, "calls": {}}
    for name, call in cases.items():
        assert call() in (0, None), (name, lib.pb_last_error())  # (every argument passes its checks; no frames: PB_OK)
        medians = []
        for _ in range(args.repeats):
            for _ in range(args.warmup):
                call()
            times = []
            for _ in range(args.calls):
                t0 = time.perf_counter()
                call()
                times.append(time.perf_counter() - t0)
            medians.append(round(statistics.median(times) * 1e6, 3))
        out["calls"][name] = {"us_per_call": medians, "median_us": statistics.median(medians), "spread_us": round(max(medians) - min(medians), 3)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
