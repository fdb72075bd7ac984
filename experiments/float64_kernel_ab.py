#!/usr/bin/env python3
"""The float64 remap kernel (what a deferred plan launches) and warm plan preparation for BUILT-IN lenses, as one process of whatever tree
it is started in measures them - to be run alternately in two checkouts (a parent and a change that touches the float64 chain) in one
GPU call.  Geometries: c2 (panorama source, no rotation), c1 (camera source, no rotation), c3 (camera source, one rotation) and c2 with
two rotations (the run-time rotation count) - the instantiations pb_remap_kernel<2, 0>, <0, 0>, <0, 1> and <2, -1>.
    python experiments/float64_kernel_ab.py [--reps 5] [--iters 20]
Per geometry: `iters` launches between two HIP events after a warm-up launch, the median over `reps` rounds; one JSON line."""

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
from tests.cases import Case, full_cases  # noqa: E402


def timed(fn, iters, stream):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    a.record(stream)
    for _ in range(iters):
        fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    stream = torch.cuda.current_stream()
    full = {c.name: c for c in full_cases()}
    c2 = full["c2"]
    cases = [c2, full["c1"], full["c3"], Case("c2_rot2", c2.dst, c2.src, [(10, 20, 30), (-5, 7, 1)])]
    row = {"tree": ROOT}
    for case in cases:
        frame = nat.synth_frame(case.src[1], case.src[2], frame=0, circle_mask=case.mask)
        out = torch.empty((case.dst[1], case.dst[2], 3), dtype=torch.uint8, device="cuda")
        plan = H.pb_plan_private(case, defer=True, bilinear=False)
        ts = [timed(lambda: plan.launch(frame.data_ptr(), out.data_ptr()), args.iters, stream) for _ in range(args.reps)]
        prep = [H.pb_plan_private(case, bilinear=False).timing()["prepare_ms"] for _ in range(6)]
        row[case.name] = {"float64_us": round(statistics.median(ts), 1), "float64_us_all": [round(t, 1) for t in ts],
                          "prepare_ms": round(statistics.median(prep[1:]), 3)}
        del plan, out, frame
        torch.cuda.empty_cache()
    print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
