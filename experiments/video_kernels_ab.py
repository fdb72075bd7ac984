#!/usr/bin/env python3
"""The times of the calls behind the nearest video kernels and the pixel-size kernel, for WHICHEVER LIBRARY IS LOADED (PB_LIB_PATH names
another build of the sources, e.g. the parent commit's made with build_library(out=...)): one process, warm, medians of `reps` rounds of
`iters` calls between two HIP events after a warm-up call (the method of experiments/nv12_rate.py).
    python experiments/video_kernels_ab.py [--reps 5] [--iters 20] [--frames 16] [--out file.json]
On c2 and c1: pb_remap_nv12 at S = 1 and 2, pb_remap_planar at 4:2:0 and 4:4:4, pb_remap_px at 1 and 4 bytes, and pb_remap_track_nv12 and
pb_remap_track_planar (4:2:0) on a batch of `frames` frames; on c5 (c5_195): pb_stitch_nv12.  Packed frames of random bytes; a track call's time is
per batch.  An A / B comparison alternates child processes of the two libraries and compares the rounds (experiments/README.md)."""

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from photonbend_amd import _native as nat  # noqa: E402
from photonbend_amd.core import rotation_track  # noqa: E402
from tests import helpers as H  # noqa: E402
from tests.cases import full_cases  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from pixel_format_rate import alternate  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    stream, st, L = torch.cuda.current_stream(), nat.current_stream(), nat.load()
    n = args.frames
    table = torch.from_numpy(rotation_track(np.random.default_rng(7).uniform(-np.pi, np.pi, (n, 3)))).cuda()
    zero = (nat.C.c_uint16 * 3)(0, 0, 0)
    fill = nat.C.addressof(zero)
    res = {"device": torch.cuda.get_device_name(0), "library": nat.LIB_PATH, "reps": args.reps, "iters": args.iters, "frames": n, "us": {}}
    for name in ("c2", "c1", "c5_195"):
        case = next(c for c in full_cases() if c.name == name)
        plan = H.pb_plan_private(case, bilinear=False)
        _, h, w, *_ = case.src
        Hd, Wd = case.dst[1], case.dst[2]
        src = torch.randint(0, 256, (n * 3 * h * w * 2,), dtype=torch.uint8, device="cuda")  # (the largest frame here: 4:4:4 or a batch of P010)
        out = torch.empty((n * 3 * Hd * Wd * 2,), dtype=torch.uint8, device="cuda")
        s, o, p = src.data_ptr(), out.data_ptr(), plan.handle
        if name == "c5_195":
            ways = {"stitch_nv12": lambda: nat.check(L.pb_stitch_nv12(p, s, o, 1, None, None, 1, fill, st))}
        else:
            ways = {
                "remap_nv12 S=1": lambda: nat.check(L.pb_remap_nv12(p, s, o, 1, None, None, 1, fill, st)),
                "remap_nv12 S=2": lambda: nat.check(L.pb_remap_nv12(p, s, o, 1, None, None, 2, fill, st)),
                "remap_planar 4:2:0": lambda: nat.check(L.pb_remap_planar(p, s, o, 1, None, None, nat.PLANAR_420, 1, fill, st)),
                "remap_planar 4:4:4": lambda: nat.check(L.pb_remap_planar(p, s, o, 1, None, None, nat.PLANAR_444, 1, fill, st)),
                "remap_px B=1": lambda: nat.check(L.pb_remap_px(p, s, o, 1, 0, 0, 1, st)),
                "remap_px B=4": lambda: nat.check(L.pb_remap_px(p, s, o, 1, 0, 0, 4, st)),
                f"remap_track_nv12 x{n}": lambda: nat.check(L.pb_remap_track_nv12(p, table.data_ptr(), 1, s, o, n, None, None, 1, fill, st)),
                f"remap_track_planar x{n}": lambda: nat.check(L.pb_remap_track_planar(p, table.data_ptr(), 1, s, o, n, None, None, nat.PLANAR_420, 1, fill, st)),
            }
        for k, t in alternate(ways, args.reps, args.iters, stream).items():
            res["us"][f"{name} {k}"] = t
            print(f"{name} {k}: {t['us']} us {t['us_all']}", flush=True)
        del plan, src, out
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
