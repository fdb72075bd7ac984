#!/usr/bin/env python3
"""The polynomial (Kannala-Brandt) lens at the sizes of BASELINE's c2 (4096^2 fisheye <- 8192x4096 panorama) and c1
(4096x2048 panorama <- 3072^2 fisheye), one process, warm, alternating (the protocol of experiments/catmull_rom_rate.py: per round and
way `iters` launches between two HIP events on the launch stream after a warm-up launch; medians over `reps` rounds):

  parity   ZERO (all coefficients zero: geometrically the built-in equidistant lens, the same bytes) against the built-in equidistant
           plan AND a second built-in plan of the same geometry (A/A), nearest and bilinear - the hot kernels do not know lenses, so the
           polynomial median should lie inside the A/A spread; the tile mixes are printed next to the times.
  buys     CAL (an OpenCV-like calibration, max_theta 105 degrees; field of view 200 degrees) as the fisheye end: per-frame wall time
           ndarray -> ndarray through the device lens against the SAME lens as untagged Python callables (the host path, unchanged), and
           the device-resident kernel time per frame.
  costs    warm plan preparation and the float64 kernel per frame (a deferred plan), CAL against the built-in equidistant lens on the
           same geometry.

    python experiments/polynomial_lens_rate.py [--reps 5] [--iters 20] [--configs c2,c1] [--skip-host] [--out file.json]"""

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

rad = pb.utils.to_radians
CAL = dict(k1=-0.0357, k2=0.0031, k3=-0.00042, k4=0.00002, max_theta=rad(105))
# (fisheye side, panorama height, panorama width, the fisheye is the destination, circle mask of the synthetic source)
CONFIGS = {"c2": (4096, 4096, 8192, True, 0), "c1": (3072, 2048, 4096, False, 1)}
TILE_KEYS = ("tiles", "fix_tiles", "fix_pixels", "lean_tiles", "black_tiles", "direct_tiles", "bilinear_float64_tiles")


def timed(fn, iters, stream):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    a.record(stream)
    for _ in range(iters):
        fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters  # us per launch


def ends(name, lens, fov_deg, image=None):
    """(destination object, source object) of a config with `lens` on its fisheye end."""
    side, ph, pw, fisheye_is_dst, _ = CONFIGS[name]
    zeros = lambda h, w: np.zeros((h, w, 3), np.uint8)  # noqa: E731
    cam = lambda img: pb.CameraImage(img, rad(fov_deg), lens, magnitude=side / 2 - 0.5)  # noqa: E731
    if fisheye_is_dst:
        return cam(zeros(side, side)), pb.PanoramaImage(zeros(ph, pw) if image is None else image)
    return pb.PanoramaImage(zeros(ph, pw)), cam(zeros(side, side) if image is None else image)


def plan_of(name, lens, fov_deg, **kw):
    dst, src = ends(name, lens, fov_deg)
    kw.setdefault("bilinear", True)
    return nat.Plan(dst._proj("dst"), [], src._proj("src"), **kw)


def src_shape(name):
    side, ph, pw, fisheye_is_dst, _ = CONFIGS[name]
    return (ph, pw) if fisheye_is_dst else (side, side)


def dst_shape(name):
    side, ph, pw, fisheye_is_dst, _ = CONFIGS[name]
    return (side, side) if fisheye_is_dst else (ph, pw)


def medians(ways, reps, iters, stream):
    times = {k: [] for k in ways}
    for _ in range(reps):
        for k, fn in ways.items():  # alternating
            times[k].append(timed(fn, iters, stream))
    return {k: {"us": round(statistics.median(v), 2), "us_all": [round(t, 2) for t in v]} for k, v in times.items()}


def parity(name, args, stream):
    h, w = src_shape(name)
    frame = nat.synth_frame(h, w, frame=0, circle_mask=CONFIGS[name][4])
    out = torch.empty(dst_shape(name) + (3,), dtype=torch.uint8, device="cuda")
    plans = {"equidistant_a": plan_of(name, pb.equidistant(), 360), "equidistant_b": plan_of(name, pb.equidistant(), 360),
             "polynomial_zero": plan_of(name, pb.polynomial(), 360)}
    same = bool(torch.equal(plans["equidistant_a"].remap(frame), plans["polynomial_zero"].remap(frame)))
    row = {"measure": "parity", "config": name, "same_bytes": same, "tile_mix": {k: {t: p.info()[t] for t in TILE_KEYS} for k, p in plans.items()}}
    for interp in ("nearest", "bilinear"):
        ways = {k: (lambda p=p: p.launch(frame.data_ptr(), out.data_ptr(), interpolation=interp)) for k, p in plans.items()}
        m = medians(ways, args.reps, args.iters, stream)
        a, b, z = (m[k]["us"] for k in ("equidistant_a", "equidistant_b", "polynomial_zero"))
        every = m["equidistant_a"]["us_all"] + m["equidistant_b"]["us_all"]
        m["aa_spread_us"] = round(abs(a - b), 2)
        m["aa_range_us"] = [min(every), max(every)]
        m["polynomial_minus_mean_builtin_us"] = round(z - (a + b) / 2, 2)
        m["polynomial_inside_aa_range"] = bool(min(every) <= z <= max(every))
        row[interp] = m
    return row


def buys_and_costs(name, args, stream):
    h, w = src_shape(name)
    fov = 200
    tagged = pb.polynomial(**CAL)
    untagged = pb.Lens(lambda t: tagged.forward_function(t), lambda r: tagged.reverse_function(r))
    frame_dev = nat.synth_frame(h, w, frame=0, circle_mask=CONFIGS[name][4])
    frame = frame_dev.cpu().numpy()
    out = torch.empty(dst_shape(name) + (3,), dtype=torch.uint8, device="cuda")
    row = {"measure": "buys_and_costs", "config": name, "fov_degrees": fov, "lens": {k: (v if k != "max_theta" else 105.0) for k, v in CAL.items()},
           "src": list(src_shape(name)), "dst": list(dst_shape(name))}

    def wall(lens, calls):
        dst, src = ends(name, lens, fov, image=frame)
        t0 = time.perf_counter()
        cmap = dst.get_coordinate_map()
        t_map = time.perf_counter() - t0
        res, ts = None, []
        for _ in range(calls + 2):  # (the facade's first use of a geometry runs a deferred plan, the second prepares it: both left out)
            t0 = time.perf_counter()
            res = src.process_coordinate_map(cmap)
            ts.append(time.perf_counter() - t0)
        return res, {"map_ms": round(t_map * 1e3, 2), "frame_ms": round(statistics.median(ts[2:]) * 1e3, 3), "frame_ms_all": [round(t * 1e3, 3) for t in ts]}

    new, row["device_lens_wall"] = wall(tagged, 5)
    if not args.skip_host:
        old, row["host_callables_wall"] = wall(untagged, 3)
        row["same_bytes"] = bool(np.array_equal(new, old))
        row["wall_ratio"] = round(row["host_callables_wall"]["frame_ms"] / row["device_lens_wall"]["frame_ms"], 1)
    # device-resident: the prepared plan's kernel, the float64 kernel of a deferred plan, and plan preparation - CAL against equidistant
    for tag, lens in (("polynomial_cal", tagged), ("equidistant", pb.equidistant())):
        prep = []
        for _ in range(6):
            p = plan_of(name, lens, fov, bilinear=False)
            prep.append(p.timing()["prepare_ms"])
        deferred = plan_of(name, lens, fov, defer=True, bilinear=False)
        ways = {"tiles": lambda p=p: p.launch(frame_dev.data_ptr(), out.data_ptr()), "float64": lambda d=deferred: d.launch(frame_dev.data_ptr(), out.data_ptr())}
        m = medians(ways, args.reps, args.iters, stream)
        row[tag] = {"prepare_ms": round(statistics.median(prep[1:]), 3), "prepare_ms_all": [round(t, 3) for t in prep], "tile_kernel": m["tiles"],
                    "float64_kernel": m["float64"], "tile_mix": {t: p.info()[t] for t in TILE_KEYS}}
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--configs", default="c2,c1")
    ap.add_argument("--skip-host", action="store_true", help="leave out the user-callable host path (seconds per frame at these sizes)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    stream = torch.cuda.current_stream()
    rows = []
    for name in args.configs.split(","):
        for fn in (parity, buys_and_costs):
            row = fn(name, args, stream)
            rows.append(row)
            print(json.dumps(row), flush=True)
            torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "reps": args.reps, "iters": args.iters, "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
