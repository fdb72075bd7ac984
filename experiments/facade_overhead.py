#!/usr/bin/env python3
"""What one ``process_coordinate_map`` call costs on the smallest host-frame fused case - a 32 x 64 panorama from a 48 x 48 camera, uint8
RGB, lazy map, the geometry's plan prepared (second and later uses) - where the kernel is negligible and the facade's own Python shows:
    python experiments/facade_overhead.py [--tree DIR] [--repeats 5] [--calls 200] [--warmup 20]
Per repeat the median of `calls` calls after `warmup` calls; prints one JSON line with the repeats' medians (us), their median and their
spread (max - min).  ``--tree DIR``: time the package of another checkout (its Python; PB_LIB_PATH names the library to load)."""

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    import numpy as np

    import photonbend_amd as pb

    rng = np.random.default_rng(0)
    camera = pb.CameraImage(rng.integers(0, 256, (48, 48, 3), dtype=np.uint8), pb.utils.to_radians(180), pb.equidistant())
    cmap = pb.PanoramaImage(np.zeros((32, 64, 3), np.uint8)).get_coordinate_map()
    first = camera.process_coordinate_map(cmap)
    medians = []
    for _ in range(args.repeats):
        for _ in range(args.warmup):
            camera.process_coordinate_map(cmap)
        times = []
        for _ in range(args.calls):
            t0 = time.perf_counter()
            out = camera.process_coordinate_map(cmap)
            times.append(time.perf_counter() - t0)
        assert np.array_equal(out, first)
        medians.append(round(statistics.median(times) * 1e6, 2))
    print(json.dumps({"package": os.path.dirname(pb.__file__), "us_per_call": medians, "median_us": statistics.median(medians),
                      "spread_us": round(max(medians) - min(medians), 2)}))


if __name__ == "__main__":
    main()
