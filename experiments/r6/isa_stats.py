#!/usr/bin/env python3
"""Per-kernel register / scratch / occupancy figures of the product build's gfx950 code, read from the compiler's own assembly listing
(photonbend_amd.build: build_listing compiles it, parse_listing reads it) - and the SGPR-spill traffic (v_readlane / v_writelane),
which decides whether a tile kernel keeps its 64-dword tile entry in scalar registers or drags it through VGPR lanes at every use (round 6:
+40 % vector instructions per wave from the spelling of one `if`; tests/test_isa_budget.py pins the figures).
    python experiments/r6/isa_stats.py [-DNAME ...] [--out file.s] [--all] [--reuse]     (default: the hot kernels only)"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from photonbend_amd.build import build_listing, parse_listing  # noqa: E402

HOT = ("pb_hot_win_kernel", "pb_hot_double_kernel", "pb_bilinear_hot_kernel", "pb_bilinear_double_hot_kernel", "pb_certify_kernel")


def kernel_stats(defs=(), out="/tmp/pb_isa.s", reuse=False):
    """-> the rows of parse_listing for every kernel of the device code built with `defs` ("-DNAME" arguments), listing kept at `out`"""
    if not (reuse and os.path.exists(out)):
        build_listing(out, [d[2:] for d in defs])
    return parse_listing(open(out).read())


if __name__ == "__main__":
    defs = [a for a in sys.argv[1:] if a.startswith("-D")]
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else "/tmp/pb_isa.s"
    print(f"{'kernel':70s} vgpr agpr sgpr scratch occ  f64  valu  instr  v_readlane+v_writelane (SGPR spill traffic)")
    for r in kernel_stats(defs, out, "--reuse" in sys.argv):
        if "--all" in sys.argv or any(h in r["name"] for h in HOT):
            print(f"{r['name'][:70]:70s} {r['vgpr']:4d} {r['agpr']:4d} {r['sgpr']:4d} {r['scratch']:7d} {r['occupancy']:3d} {r['f64']:4d} {r['valu']:5d} {r['instr']:6d} {r['lane_traffic']:6d}")
