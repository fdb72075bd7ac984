"""Builds the HIP shared library in-tree with hipcc for gfx950 (cross-compiles
without a GPU).  ``python -m photonbend_amd.build`` or ``build_library()``."""

from __future__ import annotations

import os
import re
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
HEADER = os.path.join(os.path.dirname(HERE), "include", "photonbend_hip.h")
LIB_NAME = "libphotonbend_hip.so"
# the product library of the FIRST math flavour (what _native.py loads on a host with AVX512_SKX; PB_LIB_PATH there loads another build
# of the same sources - A/B experiments: -DPB_STAMPS, -DPB_ABLATION)
LIB_PATH = os.path.join(HERE, LIB_NAME)
LIBM_LIB_NAME = "libphotonbend_hip_libm.so"
LIBM_LIB_PATH = os.path.join(HERE, LIBM_LIB_NAME)
# NOT in the package directory: only the product libraries sit next to _native.py (build/ is git-ignored and travels to the GPU box)
DIAG_LIB_PATH = os.path.join(os.path.dirname(HERE), "build", "libphotonbend_hip_diag.so")

# -ffp-contract=off: the reference rounds every multiply and add separately; the
# kernels fuse only where they say fma() (see csrc/pb_stages.hpp).
# -mllvm -disable-machine-licm: the float64 kernels evaluate five table-and-polynomial transcendental kernels per pixel inside loops (16
# pixels per lane in certification); hoisting those kernels' hundred-odd float64 constants out of the loops made certification need 212
# VGPRs (two waves per SIMD) where 94 suffice (five): plan preparation c3 1.15 -> 1.02 ms, c5 1.52 -> 1.31.  The hot kernels keep their
# register counts and their times with or without it (experiments/README.md, round 4).
HIPCC_FLAGS = [
    "--offload-arch=gfx950",
    "-O3",
    "-std=c++17",
    "-ffp-contract=off",
    "-mllvm",
    "-disable-machine-licm",
    "-fPIC",
    "-shared",
    "-fvisibility=hidden",
    "-Wall",
    "-Wno-unused-function",
]


def hipcc() -> str:
    for cand in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found (looked at $HIPCC, PATH and /opt/rocm/bin/hipcc)")


def sources():
    return sorted(os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".hip"))


def stale(path: str) -> bool:
    """True when `path` is missing, or older than any file of csrc/ or the public header."""
    if not os.path.exists(path):
        return True
    t = os.path.getmtime(path)
    deps = [os.path.join(CSRC, f) for f in os.listdir(CSRC)]
    deps.append(HEADER)
    return any(os.path.getmtime(d) > t for d in deps)


def host_math_flavour() -> str:
    """Which code THIS host's NumPy runs for np.arcsin / arccos / arctan / tan - and so which bits the reference would print here:
    "svml" (NumPy's AVX-512 kernels: x86-64 Linux with AVX512_SKX) or "libm" (everything else: the platform's libm).  PB_MATH_FLAVOUR
    overrides.  The library is loaded in the same flavour (include/photonbend_hip.h, "MATH FLAVOURS")."""
    env = os.environ.get("PB_MATH_FLAVOUR", "").lower()
    if env in ("svml", "libm"):
        return env
    try:
        try:
            from numpy._core._multiarray_umath import __cpu_features__ as feats
        except ImportError:
            from numpy.core._multiarray_umath import __cpu_features__ as feats
    except Exception:
        return "svml"
    return "svml" if feats.get("AVX512_SKX") else "libm"


def variants() -> dict:
    """name -> (path, defines): the three libraries built from the same sources.
    product: what _native.py loads on a host with AVX512_SKX.
    libm: the SECOND MATH FLAVOUR (-DPB_MATH_LIBM, csrc/pb_math.hpp): np.arcsin / arccos / arctan / tan as an x86-64 host WITHOUT AVX512_SKX
    computes them (glibc's asin / acos / atan / tan instead of NumPy's AVX-512 kernels).  A product library like the first: _native.py loads
    the one that matches the host's own NumPy dispatch (PB_MATH_FLAVOUR overrides).
    diagnostic: the -DPB_ABLATION build (never the product: loaded only through PB_LIB_PATH by experiments/ and by the error-path test): it
    alone reads the experiment knobs and the allocation-failure hook from the environment.  In the HOST's math flavour, like the product
    library the tests compare it with."""
    return {
        "product": (LIB_PATH, ()),
        "libm": (LIBM_LIB_PATH, ("PB_MATH_LIBM",)),
        "diagnostic": (DIAG_LIB_PATH, ("PB_ABLATION",) + (("PB_MATH_LIBM",) if host_math_flavour() == "libm" else ())),
    }


def _run_hipcc(args, verbose: bool = False) -> None:
    cmd = [hipcc(), *args]
    if verbose:
        print(" ".join(cmd), file=sys.stderr)
    res = subprocess.run(cmd, capture_output=True, text=True)
    if res.returncode != 0:
        raise RuntimeError(f"hipcc failed ({res.returncode}):\n{res.stdout}\n{res.stderr}")
    if verbose and res.stderr:
        print(res.stderr, file=sys.stderr)


def _build(out: str, defines, force: bool, verbose: bool) -> str:
    """One library: `defines` compiled into `out`, unless it is up to date and nobody forces it."""
    if not force and not stale(out):
        return out
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)  # (build/ may not exist yet)
    _run_hipcc([*HIPCC_FLAGS, *[f"-D{d}" for d in defines], *sources(), "-o", out], verbose)
    return out


def build_library(force: bool = False, verbose: bool = False, out: str = None, defines=()) -> str:
    """The product library - or, with `out` another path, any build of the same sources (always compiled)."""
    product, _ = variants()["product"]
    out = out or product
    return _build(out, defines, force or out != product, verbose)


def build_libm_flavour(force: bool = False, verbose: bool = False) -> str:
    return _build(*variants()["libm"], force, verbose)


def build_diagnostic(force: bool = False, verbose: bool = False) -> str:
    return _build(*variants()["diagnostic"], force, verbose)


def build_listing(out: str, defines=()) -> str:
    """The assembly listing of the device code of the same build (parse_listing reads it): the libraries' flags without the ones
    that make a shared library."""
    flags = [f for f in HIPCC_FLAGS if f not in ("-shared", "-fPIC", "-fvisibility=hidden")]
    _run_hipcc([*flags, *[f"-D{d}" for d in defines], "-S", "--cuda-device-only", "-o", out, *sources()])
    return out


def parse_listing(text):
    """-> [{mangled, name, vgpr, agpr, sgpr, scratch, occupancy, f64, valu, instr, lane_traffic}] for every kernel of a listing: registers,
    scratch, occupancy, and the SGPR-spill traffic (v_readlane / v_writelane), which decides whether a tile kernel keeps its 64-dword tile
    entry in scalar registers or drags it through VGPR lanes at every use."""
    t = text
    rows = []
    for m in re.finditer(r"^(_Z\w+):\s*; @", t, re.M):
        end = t.find(".Lfunc_end", m.end())
        body, tail = t[m.end():end], t[end:end + 6000]

        def grab(pat):
            mm = re.search(pat, tail)
            return int(mm.group(1)) if mm else -1

        ops = [l.split()[0] for l in body.splitlines() if l.strip() and l.strip()[0] not in ".;" and not l.strip().endswith(":")]
        rows.append({"mangled": m.group(1), "vgpr": grab(r"; NumVgprs: (\d+)"), "agpr": grab(r"; NumAgprs: (\d+)"), "sgpr": grab(r"; TotalNumSgprs: (\d+)"),
                     "scratch": grab(r"; ScratchSize: (\d+)"), "occupancy": grab(r"; Occupancy: (\d+)"),
                     "f64": sum(1 for o in ops if o.startswith("v_") and "f64" in o), "valu": sum(1 for o in ops if o.startswith("v_")), "instr": len(ops),
                     "lane_traffic": sum(1 for o in ops if o in ("v_readlane_b32", "v_writelane_b32"))})
    names = subprocess.run(["c++filt"], input="\n".join(r["mangled"] for r in rows), capture_output=True, text=True).stdout.splitlines()
    for r, d in zip(rows, names):
        r["name"] = re.sub(r"\(.*", "", d).replace("void ", "")
    return rows


if __name__ == "__main__":
    print(build_library(force="--force" in sys.argv, verbose=True))
    if "--libm" in sys.argv or host_math_flavour() == "libm":  # (a host without AVX512_SKX loads the second flavour: build it without being asked)
        print(build_libm_flavour(force=True, verbose=True))
    if "--diag" in sys.argv:
        print(build_diagnostic(force=True, verbose=True))
