#!/usr/bin/env python3
"""The rates of the interpolating call for grey, RGBA and 16-bit frames (pb_remap_interp_px), measured in ONE process, warm,
alternating: medians of `reps` rounds of `iters` launches between two HIP events, after a warm-up launch (the method of
experiments/video_bilinear_rate.py).
    python experiments/px_interp_rate.py [--reps 5] [--iters 20] [--cases c1,c2] [--out file.json]
On each case's geometry, for grey8, RGBA8, grey16 and RGBA16 frames and both filters, time per frame of
  (a)   the new launch, one pb_px_interp_kernel;
  (b)   pb_sample_map_bilinear_px / pb_sample_map_catmull_rom_px on a device-resident float64 map - measured twice (A / A) for that figure's
        own spread;
  (c)   pb_remap_track_px with an identity rotation per frame;
  (d)   pb_remap_bilinear_u8 / pb_remap_catmull_rom_u8 on an RGB8 frame of the same plan: recorded, not judged.
Exit status 1 when (a)'s samples are further than the derived tolerance (tests/px_interp_cases.tolerance) from (b)'s anywhere - a pixel
that is black in exactly one of the two is excused only inside tests/interp_cases.edge_band(case, final, 1/512), which is empty for a
panorama source such as c1's and c2's -, or when (a) is not faster than the faster of (b) and (c) by more than the A / A spread of (b) in the same
run - the only thresholds."""

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from photonbend_amd import _native as nat  # noqa: E402
from tests import helpers as H  # noqa: E402
from tests import interp_cases as ic  # noqa: E402
from tests import px_interp_cases as pc  # noqa: E402
from tests.cases import full_cases  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from pixel_format_rate import alternate  # noqa: E402

FORMATS = {"grey8": (1, 1), "rgba8": (4, 1), "grey16": (1, 2), "rgba16": (4, 2)}  # name -> (channels, sample bytes)
FILTERS = ("bilinear", "catmull-rom")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--cases", default="c1,c2")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    stream = torch.cuda.current_stream()
    st = nat.current_stream()
    L = nat.load()
    C = nat.C
    res = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "iters": args.iters, "rows": []}
    failures = []
    eye = torch.from_numpy(np.eye(3).reshape(1, 1, 3, 3)).cuda()
    for name in args.cases.split(","):
        case = next(c for c in full_cases() if c.name == name)
        assert not case.rotations  # (the device map below is the destination's own)
        plan = H.pb_plan_private(case, bilinear=True)
        _, h, w, *_ = case.src
        Hd, Wd = case.dst[1], case.dst[2]
        srcp = plan.src
        # where (a) and (b) may disagree on black or sampled: tests/interp_cases.edge_band, empty for a panorama source (no map is computed for one)
        band = ic.edge_band(case, ic.final_map(case), pc.BAND).ravel() if case.src[0] == "camera" else np.zeros(Hd * Wd, bool)
        cmap = nat.coordmap(plan.dst)  # device-resident, float64 (Hd, Wd, 3)
        rgb = torch.randint(0, 256, (h, w, 3), dtype=torch.uint8, device="cuda")
        rgb_out = torch.empty((Hd, Wd, 3), dtype=torch.uint8, device="cuda")
        row = {"case": name, "tile_mix": plan.bilinear_tile_mix(), "map_bytes": int(cmap.numel() * cmap.element_size())}
        res["rows"].append(row)
        print(json.dumps(row), flush=True)
        for fmt, (ch, S) in FORMATS.items():
            B = ch * S
            R = 255 if S == 1 else 65535
            src = torch.randint(0, 256, (h * w * B,), dtype=torch.uint8, device="cuda")  # (every byte random: samples in [0, R])
            out_a, out_b, out_c = (torch.empty((Hd * Wd * B,), dtype=torch.uint8, device="cuda") for _ in range(3))
            for filt in FILTERS:
                mode = nat.TRACK_INTERP_IDS[filt]
                assert plan.px_interp_supported(ch, S, filt)
                sample_map = L.pb_sample_map_bilinear_px if filt == "bilinear" else L.pb_sample_map_catmull_rom_px
                rgb_call = L.pb_remap_bilinear_u8 if filt == "bilinear" else L.pb_remap_catmull_rom_u8
                a = lambda: nat.check(L.pb_remap_interp_px(plan.handle, src.data_ptr(), out_a.data_ptr(), 1, 0, 0, ch, S, mode, st))  # noqa: E731
                b = lambda: nat.check(sample_map(C.byref(srcp), cmap.data_ptr(), Hd, Wd, None, None, src.data_ptr(), out_b.data_ptr(), ch, S, st))  # noqa: E731
                c = lambda: nat.check(L.pb_remap_track_px(plan.handle, eye.data_ptr(), 1, mode, src.data_ptr(), out_c.data_ptr(), 1, 0, 0, ch, S, st))  # noqa: E731
                d = lambda: nat.check(rgb_call(plan.handle, rgb.data_ptr(), rgb_out.data_ptr(), 1, 0, 0, st))  # noqa: E731
                a()
                b()
                torch.cuda.synchronize()
                dt = np.uint8 if S == 1 else np.uint16
                ga, gb = (o.cpu().numpy().view(dt).reshape(Hd * Wd, ch).astype(np.int64) for o in (out_a, out_b))
                T = pc.tolerance(filt, R)
                diff = np.abs(ga - gb).max(axis=1)
                # black in exactly one of the two, inside the edge band of a camera source's frame: the only excuse (none for a panorama source)
                flips = band & ((ga == 0).all(axis=1) != (gb == 0).all(axis=1))
                beyond = int(((diff > T) & ~flips).sum())
                row = {"case": name, "pixel_format": fmt, "filter": filt, "T": T, "max_abs_diff_outside_flips": int(diff[~flips].max(initial=0)), "pixels_beyond_T": beyond,
                       "edge_band_pixels": int(band.sum()), "flips": int(((diff > T) & flips).sum()), "pixels_differing": int((diff != 0).sum()), "pixels": int(diff.size)}
                if beyond:
                    failures.append(f"{name} {fmt} {filt}: {beyond} pixels further than T = {T} from the materialised-map call")
                t = alternate({"b_1": b, "a": a, "c": c, "d": d, "b_2": b}, args.reps, args.iters, stream)
                b_all = t["b_1"]["us_all"] + t["b_2"]["us_all"]
                b_med, b_spread = statistics.median(b_all), max(b_all) - min(b_all)
                best = min(b_med, t["c"]["us"])
                row.update({"a_px_interp": t["a"], "b_sample_map_1": t["b_1"], "b_sample_map_2": t["b_2"], "b_us": round(b_med, 1), "b_spread_us": round(b_spread, 1),
                            "c_track_identity": t["c"], "d_rgb8": t["d"], "best_before_over_a": round(best / t["a"]["us"], 2), "a_over_rgb8": round(t["a"]["us"] / t["d"]["us"], 2),
                            "a_GBps_out": round(Hd * Wd * B / t["a"]["us"] * 1e-3, 1)})
                if not t["a"]["us"] < best - b_spread:
                    failures.append(f"{name} {fmt} {filt}: the new launch ({t['a']['us']} us) is not faster than the faster of the materialised-map call ({b_med:.1f} us) "
                                    f"and the identity track ({t['c']['us']} us) beyond the former's spread ({b_spread:.1f} us)")
                res["rows"].append(row)
                print(json.dumps(row), flush=True)
            del src, out_a, out_b, out_c
        del plan, cmap, rgb, rgb_out
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
