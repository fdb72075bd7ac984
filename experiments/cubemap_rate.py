#!/usr/bin/env python3
"""The cube map's rates, measured in ONE process, warm, alternating: medians of `reps` rounds of `iters` launches between two
HIP events, after a warm-up launch.
    python experiments/cubemap_rate.py [--reps 5] [--iters 20] [--face 2048] [--out file.json]
  destination   the 4N x 2N panorama -> a cube of face size N in ONE launch, against the only way there was before: six prepared
                rectilinear N x N camera plans (fov 120 degrees, f_distance N / 2) behind the six face rotations, six launches, summed -
                measured twice (A / A) for that figure's own spread.  The bytes must be equal.
  source        the cube -> the 4N x 2N panorama on the prepared plan (the camera's tile kernels + the exact tables) against the same
                build's float64 route (PB_MODE_FAITHFUL); the share of tiles listed whole (face edges), and the warm preparation time of
                both plans next to BASELINE config c2's.
Exit status 1 when bytes differ either way, or when the one launch is slower than the six beyond the six-launch figure's own spread."""

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
from tests import helpers as H  # noqa: E402
from tests.cases import full_cases  # noqa: E402

KEYS = ("tiles", "fix_tiles", "fix_pixels", "lean_tiles", "direct_tiles", "black_tiles")


def timed(fn, iters, stream):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    a.record(stream)
    for _ in range(iters):
        fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters  # us per call


def alternate(ways, reps, iters, stream):
    times = {k: [] for k in ways}
    for _ in range(reps):
        for k, fn in ways.items():
            times[k].append(timed(fn, iters, stream))
    return {k: {"us": round(statistics.median(v), 1), "us_all": [round(t, 1) for t in v]} for k, v in times.items()}


def warm_prepare_ms(make, n=5):
    """Median wall time of creating (= preparing) a plan of a geometry this process has prepared before."""
    make()
    out = []
    for _ in range(n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        p = make()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
        del p
    return round(statistics.median(out), 3)


def mix(plan):
    info = plan.info()
    return {k: info[k] for k in KEYS}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--face", type=int, default=2048)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    stream = torch.cuda.current_stream()
    n = args.face
    res = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "iters": args.iters, "face": n}
    pano = nat.make_proj(nat.KIND_PANO, 2 * n, 4 * n)
    cube = nat.make_proj(nat.KIND_CUBE, 2 * n, 3 * n)

    # ---- destination: one cube launch against six face launches ------------------------------------------------------------------------
    frame = nat.synth_frame(2 * n, 4 * n, frame=0)
    plan = nat.Plan(cube, [], pano)
    fov = 2 * np.pi / 3
    face = nat.make_proj(nat.KIND_CAMERA, n, n, nat.LENS_IDS["rectilinear"], fov, n / 2 * np.tan(fov / 2), n / 2)
    faces = [nat.Plan(face, [pb.utils.cubemap_face_rotation(name)], pano) for name in pb.utils.CUBEMAP_FACES]
    out = torch.empty((2 * n, 3 * n, 3), dtype=torch.uint8, device="cuda")
    outs = [torch.empty((n, n, 3), dtype=torch.uint8, device="cuda") for _ in range(6)]
    plan.remap(frame, out=out)
    for p, o in zip(faces, outs):
        p.remap(frame, out=o)
    torch.cuda.synchronize()
    equal = all(bool(torch.equal(out[(k // 3) * n:(k // 3 + 1) * n, (k % 3) * n:(k % 3 + 1) * n], outs[k])) for k in range(6))

    def six():
        for p, o in zip(faces, outs):
            p.launch(frame.data_ptr(), o.data_ptr())

    t = alternate({"six_a": six, "cube": lambda: plan.launch(frame.data_ptr(), out.data_ptr()), "six_b": six}, args.reps, args.iters, stream)
    six_all = t["six_a"]["us_all"] + t["six_b"]["us_all"]
    res["destination"] = {
        "bytes_equal": equal, "cube": t["cube"], "six_a": t["six_a"], "six_b": t["six_b"],
        "six_spread_us": round(max(six_all) - min(six_all), 1), "six_aa_us": round(abs(t["six_a"]["us"] - t["six_b"]["us"]), 1),
        "cube_over_six": round(t["cube"]["us"] / statistics.median(six_all), 3),
        "cube_mix": mix(plan), "face_mix": [mix(p) for p in faces],
        "cube_prepare_ms_warm": warm_prepare_ms(lambda: nat.Plan(cube, [], pano)),
    }
    print(json.dumps({"destination": res["destination"]}), flush=True)
    del plan, faces, out, outs, frame
    torch.cuda.empty_cache()

    # ---- source: the prepared plan against the float64 route ---------------------------------------------------------------------------
    frame = nat.synth_frame(2 * n, 3 * n, frame=0)
    plan, plan64 = nat.Plan(pano, [], cube), nat.Plan(pano, [], cube)
    plan64.set_mode(nat.MODE_FAITHFUL)
    out = torch.empty((2 * n, 4 * n, 3), dtype=torch.uint8, device="cuda")
    out64 = torch.empty_like(out)
    plan.remap(frame, out=out)
    plan64.remap(frame, out=out64)
    torch.cuda.synchronize()
    t = alternate({"plan": lambda: plan.launch(frame.data_ptr(), out.data_ptr()), "float64": lambda: plan64.launch(frame.data_ptr(), out64.data_ptr())},
                  args.reps, args.iters, stream)
    m = mix(plan)
    c2 = next(c for c in full_cases() if c.name == "c2")
    res["source"] = {
        "bytes_equal": bool(torch.equal(out, out64)), "fast_path": plan.info()["fast_path"], "plan": t["plan"], "float64": t["float64"],
        "float64_over_plan": round(t["float64"]["us"] / t["plan"]["us"], 2), "mix": m, "fix_tile_share": round(m["fix_tiles"] / max(1, m["tiles"]), 4),
        "prepare_ms_warm": warm_prepare_ms(lambda: nat.Plan(pano, [], cube)),
        "c2_prepare_ms_warm": warm_prepare_ms(lambda: H.pb_plan_private(c2, bilinear=False)),
    }
    print(json.dumps({"source": res["source"]}), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    # what must hold (exit status 1 otherwise): equal bytes both ways, and one cube launch not slower than the six face launches by more
    # than the six-launch figure's own spread in this run
    d, failures = res["destination"], []
    if not d["bytes_equal"]:
        failures.append("the cube launch's bytes differ from the six face launches'")
    if not res["source"]["bytes_equal"]:
        failures.append("the cube source's prepared plan and float64 route give different bytes")
    six = statistics.median(d["six_a"]["us_all"] + d["six_b"]["us_all"])
    if d["cube"]["us"] > six + d["six_spread_us"]:
        failures.append(f"one cube launch ({d['cube']['us']} us) is slower than six face launches ({six:.1f} us) beyond their spread ({d['six_spread_us']} us)")
    for msg in failures:
        print("FAILED: " + msg, file=sys.stderr)
    sys.exit(1 if failures else 0)


if __name__ == "__main__":
    main()
