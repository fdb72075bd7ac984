#!/usr/bin/env python3
"""The rates of the bilinear video calls (pb_remap_planar_bilinear / pb_remap_nv12_bilinear), measured in ONE process, warm,
alternating: medians of `reps` rounds of `iters` launches between two HIP events, after a warm-up launch (the method of
experiments/planar_rate.py).
    python experiments/video_bilinear_rate.py [--reps 5] [--iters 20] [--cases c2,c1] [--out file.json]
On each case's geometry, time per frame of
  (a)   the new launch, one pb_planar_bilinear_kernel, for yuv420p, nv12, yuv444p and p010;
  (n)   the nearest call on the same plan and frame (pb_remap_planar / pb_remap_nv12), for scale;
  (r)   pb_remap_bilinear_u8 (LDS windows) and pb_remap_catmull_rom_u8 (global taps) on the same plan, RGB8 frames: where (a) lands between
        them is reported, not judged;
  (b)   at yuv444p: the only way to compute the same definition before - three pb_sample_map_bilinear_px calls, one per plane, on a
        device-resident float64 map - measured twice (A / A) for that figure's own spread.
Fill (0, 0, 0), so that (a) and (b) write the same planes.  Exit status 1 when (a)'s samples are further than T(R) = 1 + R // 512 from (b)'s
anywhere but where exactly one of the two is fill, or when (a) is not faster than (b) by more than the A / A spread of (b) in the same run -
the only thresholds."""

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
from tests.cases import full_cases  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from pixel_format_rate import alternate  # noqa: E402

# name -> (bytes per sample, subsampling, interleaved pairs)
FORMATS = {"yuv420p": (1, nat.PLANAR_420, False), "nv12": (1, nat.PLANAR_420, True), "yuv444p": (1, nat.PLANAR_444, False), "p010": (2, nat.PLANAR_420, True)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--cases", default="c2,c1")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    stream = torch.cuda.current_stream()
    st = nat.current_stream()
    L = nat.load()
    C = nat.C
    res = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "iters": args.iters, "rows": []}
    failures = []
    zero = (C.c_uint16 * 3)(0, 0, 0)
    for name in args.cases.split(","):
        case = next(c for c in full_cases() if c.name == name)
        assert not case.rotations  # (the device map below is the destination's own)
        plan = H.pb_plan_private(case, bilinear=True)
        _, h, w, *_ = case.src
        Hd, Wd = case.dst[1], case.dst[2]
        mix = plan.bilinear_tile_mix()
        # (r) the two interpolating RGB8 tile kernels on this plan
        rgb = torch.randint(0, 256, (h, w, 3), dtype=torch.uint8, device="cuda")
        rgb_out = torch.empty((Hd, Wd, 3), dtype=torch.uint8, device="cuda")
        ways = {"bilinear_u8": lambda: nat.check(L.pb_remap_bilinear_u8(plan.handle, rgb.data_ptr(), rgb_out.data_ptr(), 1, 0, 0, st)),
                "catmull_rom_u8": lambda: nat.check(L.pb_remap_catmull_rom_u8(plan.handle, rgb.data_ptr(), rgb_out.data_ptr(), 1, 0, 0, st))}
        rgb_t = alternate(ways, args.reps, args.iters, stream)
        row = {"case": name, "tile_mix": mix, "rgb8": rgb_t}
        res["rows"].append(row)
        print(json.dumps(row), flush=True)
        cmap = nat.coordmap(plan.dst)  # device-resident, float64 (Hd, Wd, 3)
        for fmt, (S, sub, pairs) in FORMATS.items():
            cx, cy = nat.PLANAR_SHIFTS[sub]
            assert plan.nv12_supported(S, interpolation="bilinear") if pairs else plan.planar_supported(sub, S, interpolation="bilinear")
            n_src, n_dst = nat.planar_frame_samples(h, w, sub) * S, nat.planar_frame_samples(Hd, Wd, sub) * S
            src = torch.randint(0, 256, (n_src,), dtype=torch.uint8, device="cuda")
            out_a, out_n = torch.empty((n_dst,), dtype=torch.uint8, device="cuda"), torch.empty((n_dst,), dtype=torch.uint8, device="cuda")
            fz = C.addressof(zero)
            if pairs:
                a = lambda: nat.check(L.pb_remap_nv12_bilinear(plan.handle, src.data_ptr(), out_a.data_ptr(), 1, None, None, S, fz, st))  # noqa: E731
                n = lambda: nat.check(L.pb_remap_nv12(plan.handle, src.data_ptr(), out_n.data_ptr(), 1, None, None, S, fz, st))  # noqa: E731
            else:
                a = lambda: nat.check(L.pb_remap_planar_bilinear(plan.handle, src.data_ptr(), out_a.data_ptr(), 1, None, None, sub, S, fz, st))  # noqa: E731
                n = lambda: nat.check(L.pb_remap_planar(plan.handle, src.data_ptr(), out_n.data_ptr(), 1, None, None, sub, S, fz, st))  # noqa: E731
            ways = {"a": a, "n": n}
            row = {"case": name, "pixel_format": fmt, "bytes_per_sample": S}
            if fmt == "yuv444p":
                out_b = torch.empty_like(out_a)
                srcp = plan.src

                def b():
                    for k in range(3):
                        nat.check(L.pb_sample_map_bilinear_px(C.byref(srcp), cmap.data_ptr(), Hd, Wd, None, None, src.data_ptr() + k * h * w * S,
                                                              out_b.data_ptr() + k * Hd * Wd * S, 1, S, st))

                a()
                b()
                torch.cuda.synchronize()
                ga, gb = out_a.cpu().numpy().astype(np.int64), out_b.cpu().numpy().astype(np.int64)
                T = 1 + (255 if S == 1 else 65535) // 512
                d = np.abs(ga - gb)
                flips = (ga == 0) != (gb == 0)  # (fill in exactly one of the two: the rim of a camera source)
                beyond = int(((d > T) & ~flips).sum())
                row.update({"T": T, "max_abs_diff_outside_flips": int(d[~flips].max(initial=0)), "samples_beyond_T": beyond, "flips": int(((d > T) & flips).sum()),
                            "samples_differing": int((d != 0).sum()), "samples": int(d.size)})
                if beyond:
                    failures.append(f"{name} {fmt}: {beyond} samples further than T = {T} from three pb_sample_map_bilinear_px calls")
                ways = {"b_1": b, "a": a, "n": n, "b_2": b}
            t = alternate(ways, args.reps, args.iters, stream)
            row.update({"a_video_bilinear": t["a"], "n_nearest": t["n"], "a_over_nearest": round(t["a"]["us"] / t["n"]["us"], 2),
                        "a_over_bilinear_u8": round(t["a"]["us"] / rgb_t["bilinear_u8"]["us"], 2), "a_over_catmull_rom_u8": round(t["a"]["us"] / rgb_t["catmull_rom_u8"]["us"], 2),
                        "a_GBps_out": round(n_dst / t["a"]["us"] * 1e-3, 1)})
            if fmt == "yuv444p":
                b_all = t["b_1"]["us_all"] + t["b_2"]["us_all"]
                b_med, b_spread = statistics.median(b_all), max(b_all) - min(b_all)
                row.update({"b_three_sample_map_1": t["b_1"], "b_three_sample_map_2": t["b_2"], "b_us": round(b_med, 1), "b_spread_us": round(b_spread, 1),
                            "b_over_a": round(b_med / t["a"]["us"], 2)})
                if not t["a"]["us"] < b_med - b_spread:
                    failures.append(f"{name} {fmt}: the new launch ({t['a']['us']} us) is not faster than three pb_sample_map_bilinear_px calls ({b_med:.1f} us) beyond "
                                    f"their spread ({b_spread:.1f} us)")
            res["rows"].append(row)
            print(json.dumps(row), flush=True)
            del src, out_a, out_n
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
