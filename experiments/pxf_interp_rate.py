#!/usr/bin/env python3
"""The rates of the interpolating call for float16 and float32 frames (pb_remap_interp_pxf), measured in ONE process, warm,
alternating: medians of `reps` rounds of `iters` launches between two HIP events, after a warm-up launch (the method of
experiments/px_interp_rate.py).
    python experiments/pxf_interp_rate.py [--reps 5] [--iters 20] [--cases c1,c2] [--out file.json]
On each case's geometry, for grey, RGB and RGBA frames of half and single samples and both filters, time per frame of
  (a)   the new launch, one pb_pxf_interp_kernel;
  (p)   where an integer format has the same pixel size - grey-half : grey16, RGBA-half : RGBA16, grey-single : RGBA8 -, pb_remap_interp_px
        (pb_px_interp_kernel) on the same plan, measured twice (A / A) for that figure's own spread: the same bytes loaded and stored.
No earlier route exists for these frames, so nothing is judged faster or slower: the figures are recorded.  Exit status 1 only when (a)'s
samples are further than the derived tolerance (tests/pxf_cases.tolerance) from the definition's on a strip of the frame - a pixel that
is black in exactly one of the two is excused only inside tests/interp_cases.edge_band(case, final, 1/512), which is empty for a panorama
source."""

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
from tests import pxf_cases as fc  # noqa: E402
from tests import pxf_ref  # noqa: E402
from tests.cases import full_cases  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from pixel_format_rate import alternate  # noqa: E402

FORMATS = {"grey_half": (1, 2), "rgb_half": (3, 2), "rgba_half": (4, 2), "grey_single": (1, 4), "rgb_single": (3, 4), "rgba_single": (4, 4)}
SAME_BYTES = {"grey_half": ("grey16", 1, 2), "rgba_half": ("rgba16", 4, 2), "grey_single": ("rgba8", 4, 1)}  # -> pb_remap_interp_px's (name, channels, sample bytes)
FILTERS = ("bilinear", "catmull-rom")
STRIP = 64  # destination rows compared with the definition: whole tile rows through the middle of the frame (the tests compare whole frames)


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
    res = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "iters": args.iters, "rows": []}
    failures = []
    for name in args.cases.split(","):
        case = next(c for c in full_cases() if c.name == name)
        assert not case.rotations
        plan = H.pb_plan_private(case, bilinear=True)
        _, h, w, *_ = case.src
        Hd, Wd = case.dst[1], case.dst[2]
        y0 = (Hd // 2) // 32 * 32  # a strip of whole tile rows through the middle of the frame
        final = ic.final_map(case)[y0 : y0 + STRIP].copy()
        band = ic.edge_band(case, final, fc.BAND)
        row = {"case": name, "tile_mix": plan.bilinear_tile_mix()}
        res["rows"].append(row)
        print(json.dumps(row), flush=True)
        for fmt, (ch, S) in FORMATS.items():
            B = ch * S
            image, (lo, hi) = fc.draw(h, w, ch, S, 0, 7 + B, squeeze=False)
            src = torch.from_numpy(image.view(np.uint8).ravel()).cuda()
            out_a = torch.empty((Hd * Wd * B,), dtype=torch.uint8, device="cuda")
            for filt in FILTERS:
                mode = nat.TRACK_INTERP_IDS[filt]
                assert plan.float_supported(ch, S, filt)
                a = lambda: nat.check(L.pb_remap_interp_pxf(plan.handle, src.data_ptr(), out_a.data_ptr(), 1, 0, 0, ch, S, mode, st))  # noqa: E731
                a()
                torch.cuda.synchronize()
                got = out_a.cpu().numpy().view(image.dtype).reshape(Hd, Wd, ch)[y0 : y0 + STRIP].astype(np.float64)
                V = pxf_ref.remap_f64(ic.src_proj(case), image, filt, np.copy(final))
                T = fc.tolerance(filt, lo, hi, S)
                diff = np.abs(got - V).max(axis=2)
                flips = band & ((got == 0).all(axis=2) != (V == 0).all(axis=2))
                beyond = int(((diff > T) & ~flips).sum())
                row = {"case": name, "pixel_format": fmt, "pixel_bytes": B, "filter": filt, "T": T, "max_abs_diff_outside_flips": float(diff[~flips].max(initial=0.0)),
                       "pixels_beyond_T": beyond, "edge_band_pixels": int(band.sum()), "pixels_compared": int(diff.size)}
                if beyond:
                    failures.append(f"{name} {fmt} {filt}: {beyond} pixels further than T = {T} from the definition")
                ways = {"a": a}
                if fmt in SAME_BYTES:
                    pname, pch, pS = SAME_BYTES[fmt]
                    assert pch * pS == B and plan.px_interp_supported(pch, pS, filt)
                    out_p = torch.empty_like(out_a)
                    p = lambda: nat.check(L.pb_remap_interp_px(plan.handle, src.data_ptr(), out_p.data_ptr(), 1, 0, 0, pch, pS, mode, st))  # noqa: E731
                    ways = {"p_1": p, "a": a, "p_2": p}
                t = alternate(ways, args.reps, args.iters, stream)
                row.update({"a_pxf_interp": t["a"], "a_GBps_out": round(Hd * Wd * B / t["a"]["us"] * 1e-3, 1)})
                if fmt in SAME_BYTES:
                    p_all = t["p_1"]["us_all"] + t["p_2"]["us_all"]
                    p_med = statistics.median(p_all)
                    row.update({"same_bytes_integer_format": SAME_BYTES[fmt][0], "p_px_interp_1": t["p_1"], "p_px_interp_2": t["p_2"], "p_us": round(p_med, 1),
                                "p_spread_us": round(max(p_all) - min(p_all), 1), "a_over_p": round(t["a"]["us"] / p_med, 3)})
                res["rows"].append(row)
                print(json.dumps(row), flush=True)
            del src, out_a
        del plan
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
