#!/usr/bin/env python3
"""The equi-angular cube map's rates next to the plain cube's on the same build, measured in ONE process, warm, ways
alternating: medians of `reps` rounds of `iters` launches between two HIP events, after a warm-up launch.
    python experiments/eac_rate.py [--reps 5] [--iters 20] [--face 2048] [--out file.json]
For each mapping (equiangular, gnomonic):
  destination   the 4N x 2N panorama -> the cube of face size N on the prepared plan and on the float64 route (PB_MODE_FAITHFUL)
  source        the cube -> the 4N x 2N panorama, likewise; the float64 route is measured twice (A / A) for its own spread
with the tile mix of every plan - tiles listed whole, fix pixels, LEAN / DIRECT - and the warm preparation time.
Exit status 1 when a prepared plan's bytes differ from the float64 route's, either mapping, either direction, or when the prepared
equi-angular source plan does not beat the float64 route by more than that route's own A / A spread.  Equi-angular against plain cube is
a finding, printed, not a bar.
A GPU step of a job that runs this is one process: give it a `timeout` of its own and chain the steps with `&&`."""

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from experiments.cubemap_rate import alternate, mix, warm_prepare_ms  # noqa: E402
from photonbend_amd import _native as nat  # noqa: E402


def direction(dst, src, reps, iters, stream):
    frame = nat.synth_frame(src.height, src.width, frame=0)
    plan, plan64 = nat.Plan(dst, [], src), nat.Plan(dst, [], src)
    plan64.set_mode(nat.MODE_FAITHFUL)
    out = torch.empty((dst.height, dst.width, 3), dtype=torch.uint8, device="cuda")
    out64 = torch.empty_like(out)
    plan.remap(frame, out=out)
    plan64.remap(frame, out=out64)
    torch.cuda.synchronize()
    f64 = lambda: plan64.launch(frame.data_ptr(), out64.data_ptr())  # noqa: E731
    t = alternate({"float64_a": f64, "plan": lambda: plan.launch(frame.data_ptr(), out.data_ptr()), "float64_b": f64}, reps, iters, stream)
    both = t["float64_a"]["us_all"] + t["float64_b"]["us_all"]
    m = mix(plan)
    return {
        "bytes_equal": bool(torch.equal(out, out64)), "fast_path": plan.info()["fast_path"], "plan": t["plan"], "float64_a": t["float64_a"],
        "float64_b": t["float64_b"], "float64_us": round(statistics.median(both), 1), "float64_spread_us": round(max(both) - min(both), 1),
        "float64_over_plan": round(statistics.median(both) / t["plan"]["us"], 2), "mix": m,
        "fix_tile_share": round(m["fix_tiles"] / max(1, m["tiles"]), 4), "prepare_ms_warm": warm_prepare_ms(lambda: nat.Plan(dst, [], src)),
    }


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
    for name, kind in (("equiangular", nat.KIND_EAC), ("gnomonic", nat.KIND_CUBE)):
        cube = nat.make_proj(kind, 2 * n, 3 * n)
        res[name] = {"destination": direction(cube, pano, args.reps, args.iters, stream)}
        torch.cuda.empty_cache()
        res[name]["source"] = direction(pano, cube, args.reps, args.iters, stream)
        torch.cuda.empty_cache()
        print(json.dumps({name: res[name]}), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    failures = [f"{name} {way}: the prepared plan's bytes differ from the float64 route's"
                for name in ("equiangular", "gnomonic") for way in ("destination", "source") if not res[name][way]["bytes_equal"]]
    s = res["equiangular"]["source"]
    if not s["plan"]["us"] < s["float64_us"] - s["float64_spread_us"]:
        failures.append(f"the prepared equi-angular source plan ({s['plan']['us']} us) does not beat the float64 route ({s['float64_us']} us) by more "
                        f"than that route's own spread ({s['float64_spread_us']} us)")
    e, g = res["equiangular"], res["gnomonic"]
    for way in ("destination", "source"):
        print(f"{way}: equi-angular plan {e[way]['plan']['us']} us (listed whole {100 * e[way]['fix_tile_share']:.2f} %), "
              f"plain cube {g[way]['plan']['us']} us (listed whole {100 * g[way]['fix_tile_share']:.2f} %)")
    for msg in failures:
        print("FAILED: " + msg, file=sys.stderr)
    sys.exit(1 if failures else 0)


if __name__ == "__main__":
    main()
