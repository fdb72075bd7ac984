"""Every refusal of the video calls, on the CPU: a grid over the twelve C entry points - pb_remap_nv12 / _planar, their
_bilinear, _track and _track_bilinear forms and the four _supported questions - and both sample sizes, and a second grid over the ``Plan``
methods on top of them.  Every plan is DEFERRED: it has no device, so each answer is the same with and without a GPU, and every call with
frames is refused before anything could be launched.  The expected statuses, ``pb_last_error()`` texts and Python exceptions
(``tests/golden/video_calls.json``) were recorded by this very recorder from the library as it was when each family of entry points had
its own copy of the checks: a difference is a behaviour change - a message, a status, or the ORDER of two checks.

``python tests/test_video_calls_host.py OUT.json`` records the grids of the package on the path into OUT.json."""

import contextlib
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np
import pytest

from photonbend_amd import _native as nat

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "video_calls.json")
FAKE = 0x1000  # a non-null "device pointer" for calls that must be refused before anything reads it
INVALID, UNSUPPORTED = -1, -3
SUBS = {"444": nat.PLANAR_444, "422": nat.PLANAR_422, "420": nat.PLANAR_420}
SHIFTS = {nat.PLANAR_444: (0, 0), nat.PLANAR_422: (1, 0), nat.PLANAR_420: (1, 1)}
SRC_HW, DST_HW = (4, 8), (6, 12)
DOUBLE = (nat.KIND_DOUBLE,) + SRC_HW + (nat.LENS_IDS["equidistant"], 3.3, 3.0, 2.0)

# name -> (family, tracked, bilinear)
CALLS = {
    "pb_remap_nv12": ("nv12", False, False), "pb_remap_nv12_bilinear": ("nv12", False, True),
    "pb_remap_planar": ("planar", False, False), "pb_remap_planar_bilinear": ("planar", False, True),
    "pb_remap_track_nv12": ("nv12", True, False), "pb_remap_track_nv12_bilinear": ("nv12", True, True),
    "pb_remap_track_planar": ("planar", True, False), "pb_remap_track_planar_bilinear": ("planar", True, True),
}
QUESTIONS = {"pb_remap_nv12_supported": "nv12", "pb_remap_nv12_bilinear_supported": "nv12", "pb_remap_planar_supported": "planar",
             "pb_remap_planar_bilinear_supported": "planar"}

# name -> (source, destination, the plan's own rotations); every one is created with PB_PLAN_DEFER
ODD = {"odd_5x8_4x8": ((5, 8), (4, 8)), "odd_4x7_4x8": ((4, 7), (4, 8)), "odd_4x8_3x8": ((4, 8), (3, 8)), "odd_4x8_4x9": ((4, 8), (4, 9)),
       "odd_3x5_7x9": ((3, 5), (7, 9))}
PLANS = {
    "base": ((nat.KIND_PANO,) + SRC_HW, (nat.KIND_PANO,) + DST_HW, 0),
    **{name: ((nat.KIND_PANO,) + s, (nat.KIND_PANO,) + d, 0) for name, (s, d) in ODD.items()},
    "rot1": ((nat.KIND_PANO,) + SRC_HW, (nat.KIND_PANO,) + DST_HW, 1),
    "rot7": ((nat.KIND_PANO,) + SRC_HW, (nat.KIND_PANO,) + DST_HW, 7),
    "rot8": ((nat.KIND_PANO,) + SRC_HW, (nat.KIND_PANO,) + DST_HW, 8),
    "double": (DOUBLE, (nat.KIND_PANO,) + DST_HW, 0),
    "cube": ((nat.KIND_CUBE, 8, 12), (nat.KIND_PANO,) + DST_HW, 0),
    "eac": ((nat.KIND_EAC, 8, 12), (nat.KIND_PANO,) + DST_HW, 0),
    "tall": ((nat.KIND_PANO, 32768, 4), (nat.KIND_PANO, 4, 8), 0),  # (a small frame: the side alone is refused)
}


def _create(spec):
    src, dst, n_rot = spec
    lib, h = nat.load(), C.c_void_p()
    s, d = nat.make_proj(*src), nat.make_proj(*dst)
    rots = (C.c_double * (9 * max(1, n_rot)))(*([1, 0, 0, 0, 1, 0, 0, 0, 1] * max(1, n_rot)))
    assert lib.pb_plan_create_ex(C.byref(d), rots if n_rot else None, n_rot, C.byref(s), nat.PLAN_DEFER, 0, C.byref(h)) == 0, lib.pb_last_error()
    return h


def is_deferred(h):
    """No table of the plan exists: nothing has prepared it, so it has no device."""
    fast, stats = C.c_int(-1), (C.c_longlong * 7)()
    assert nat.load().pb_plan_info(h, C.byref(fast), stats, None) == 0
    return fast.value == 0 and stats[0] == -1


@contextlib.contextmanager
def plans():
    made = {name: _create(spec) for name, spec in PLANS.items()}
    try:
        yield made
    finally:
        for h in made.values():
            nat.load().pb_plan_destroy(h)


# ---- the C grid -------------------------------------------------------------------------------------------------------------------------
def packed(family, hw, S, sub):
    """The packed defaults of the header, spelled out: (pitch, uv_offset, frame_stride) / (pitch, chroma_pitch, offset1, offset2, frame_stride)."""
    h, w = hw
    if family == "nv12":
        return S * w, S * w * h, S * w * h * 3 // 2
    cx, cy = SHIFTS[sub]
    p, cp = S * w, S * (w >> cx)
    o1 = p * h
    o2 = o1 + cp * (h >> cy)
    return p, cp, o1, o2, o2 + cp * (h >> cy)


def layouts(family, hw, S, sub):
    """-> (broken, huge, valid): every layout the host tests of the three families break a rule with, the members at or beyond 2^31, and
    the ones that pass - zeros, the packed defaults spelled out, a pitched frame, and (planar) planes 1 and 2 swapped."""
    b = packed(family, hw, S, sub)
    h, w = hw
    if family == "nv12":
        broken = [(b[0] - 2 * S, 0, 0), (0, b[1] - 2 * S, 0), (b[0] + 2 * S, b[1], 0), (0, 0, b[2] - 2 * S), (0, b[1] + 2 * S, b[2]), (b[0] + S, 0, 0),
                  (0, b[1] + S, 0), (0, 0, b[2] + S), (b[0] + 2 * S + 1, 0, 0),
                  (b[0] - 2 * S, b[1] - 2 * S, 1), (b[0] + S, 0, b[2] - 2 * S)]  # (two rules at once: the first one in the order of the checks answers)
        huge = [((1 << 63) + (1 << 20), 0, 0), (1 << 31, 0, 0), (0, 1 << 31, 0), (0, (1 << 64) - 2 * S, 0), (0, (1 << 64) - 2, 0),
                (b[0] - 2 * S, 1 << 31, 0)]
        valid = [(0, 0, 0), b, (256, 256 * 9, 256 * 16), (b[0] + 2 * S, 0, 0), (0, 0, 1 << 40)]
        return broken, huge, valid
    ce = b[3] - b[2]  # a packed chroma plane's bytes
    broken = [(b[0] - S, 0, 0, 0, 0), (0, b[1] - S, 0, 0, 0), (0, S, 0, 0, 0),
              (0, 0, b[2] - S, 0, 0), (0, 0, 0, b[2] - S, 0), (0, 0, 0, b[3] - S, 0), (0, 0, b[3] + ce - S, b[3], 0), (0, 0, 0, 0, b[4] - S),
              (0, 0, 0, b[3] + S, b[4]), (0, 0, b[4], 0, b[4] + ce - S), (0, 0, 0, 0, b[0] * h), (0, 0, b[3], b[3] + S, 0),
              *([(b[0] + 1, 0, 0, 0, 0), (0, b[1] + 1, 0, 0, 0), (b[0], b[1], b[2] + 1, b[3] + 2, 0), (0, 0, 0, b[3] + 1, 0), (0, 0, 0, 0, b[4] + 1),
                 (0, 0, 0, 0, 3 * b[0] * h + 1)] if S == 2 else []),  # by one byte: not a multiple of one sample
              (b[0] - S, b[1] - S, b[2] - S, 0, 1), (b[0] + 1, 0, b[2] - S, 0, 0), (0, b[1] - S, 0, b[2] - S, b[4] - S)]  # (several rules at once)
    huge = [tuple(v if i == pos else 0 for i in range(5)) for pos in range(4) for v in (1 << 31, (1 << 63) + (1 << 20), (1 << 64) - 2)]
    huge += [(b[0] - S, 1 << 31, 0, 0, 0)]
    valid = [(0,) * 5, b, (b[0], b[1], b[3], b[2], b[4]), (256, 128, 256 * 9, 256 * 16, 256 * 32), (S * w + S, S * w, S * (w + 1) * h + S, 1024, 0),
             (0, 0, 0, 0, 1 << 40)]
    return broken, huge, valid


def call_cases(family, tracked, bilinear, S, sub):
    """[(plan's name, keywords)] of one entry point at one sample size (and subsampling): each breaks a rule - or, where it says ``ok``,
    passes every argument check and is left to the plan, which refuses it (a tracked call is served on a deferred plan, so its passing
    arguments go to the double-fisheye plan, which no video call takes)."""
    good = "double" if tracked else "base"
    out = [(None, {}), ("base", dict(src=None)), ("base", dict(dst=None)), ("base", dict(src=None, dst=None)), ("base", dict(n=-1)),
           ("base", dict(n=-1, src=None)), ("base", dict(n=-1, S=3)), (None, dict(n=-1, S=3)), ("base", dict(n=-7, sl="broken0"))]
    out += [("base", dict(S=bad)) for bad in (-1, 0, 3, 4, 8)]
    out += [("odd_5x8_4x8", dict(S=3)), ("base", dict(S=3, sl="broken0")), ("base", dict(S=0, src=FAKE + 1)), ("base", dict(S=4, n=0)), ("base", dict(S=3, table=None))]
    if family == "planar":
        out += [("base", dict(sub=bad)) for bad in (-1, 3, 5, 420)]
        out += [("base", dict(sub=3, k=0)), ("base", dict(sub=5, S=3)), ("odd_3x5_7x9", dict(sub=5)), ("base", dict(sub=-1, sl="broken0")), ("base", dict(sub=420, n=0))]
    for name, dims in ODD.items():
        out += [(name, dict(k=0)), (name, dict(n=0)), (name, dict(table=None, dl="broken1"))]
        if not tracked or family == "nv12" or any((h & SHIFTS[sub][1]) | (w & SHIFTS[sub][0]) for h, w in dims):  # (a tracked call is served where the rule allows the plan)
            out += [(name, {}), (name, dict(sl="broken0")), (name, dict(src=FAKE + 1))]
    broken_s, huge_s, valid_s = layouts(family, SRC_HW, S, sub)
    broken_d, huge_d, valid_d = layouts(family, DST_HW, S, sub)
    for which, broken, huge in (("sl", broken_s, huge_s), ("dl", broken_d, huge_d)):
        out += [("base", {which: v}) for v in broken + huge]
        out += [("base", {which: broken[0], "k": 0}), ("base", {which: broken[0], "table": None}), ("base", {which: broken[0], "src": FAKE + 1}),
                ("base", {which: huge[0], "dst": FAKE + 1}), ("base", {which: broken[3], "n": 0}), ("base", {which: huge[1], "n": 0}),
                ("double", {which: broken[1]}), ("cube", {which: huge[0]}), ("tall", {which: huge[2]})]
    # the source is looked at before the destination, a member beyond 2^31 of a layout before its other rules
    out += [("base", dict(sl=broken_s[0], dl=broken_d[1])), ("base", dict(sl=broken_s[3], dl=huge_d[0])), ("base", dict(sl=huge_s[0], dl=broken_d[0])),
            ("base", dict(sl=valid_s[1], dl=broken_d[0])), ("base", dict(sl=broken_s[5], dl=valid_d[1], src=FAKE + 1, table=None, k=0))]
    out += [(good, dict(sl=s, dl=d, ok=True)) for s, d in list(zip(valid_s, valid_d)) + [(valid_s[1], None), (None, valid_d[2])]]
    out += [("base", dict(sl=s, dl=d, n=0)) for s, d in zip(valid_s, valid_d)]
    # the pointers: one chroma pair / one sample
    unit = 2 * S if family == "nv12" else S
    for kw in (dict(src=FAKE + S), dict(dst=FAKE + S), dict(src=FAKE + 1), dict(dst=FAKE + 1), dict(src=FAKE + S, dst=FAKE + 3 * S), dict(src=FAKE + 2 * S, dst=FAKE + 2 * S)):
        out += [("base", dict(kw, ok=not (kw.get("src", 0) % unit or kw.get("dst", 0) % unit)))]
    out += [("base", kw) for kw in (dict(src=FAKE + 1, table=None), dict(dst=FAKE + 1, k=0), dict(src=FAKE + 1, n=0), dict(src=FAKE + 1, table=FAKE + 4))]
    out = [(good if kw.get("ok") else p, kw) for p, kw in out]
    # the rotation table (the other calls take and ignore these keywords: the same grid for all)
    out += [("base", kw) for kw in (dict(table=None), dict(table=FAKE + 4), dict(k=0), dict(k=-1), dict(k=9), dict(table=None, k=0), dict(table=FAKE + 4, k=9),
                                    dict(table=None, n=0), dict(k=0, n=0), dict(k=9, n=0), dict(dst=None, table=None))]
    for name, n_rot in (("rot1", 1), ("rot7", 7), ("rot8", 8)):
        out += [(name, dict(k=8 - n_rot + 1)), (name, dict(k=8 - n_rot + 1, n=0)), (name, dict(k=9, table=None))]
        if n_rot < 8:
            out += [(name, dict(k=8 - n_rot, n=0))]
    # no frames: nothing to launch, with and without fills
    out += [("base", dict(n=0)), ("base", dict(n=0, fill=(1, 2, 3))), ("base", dict(n=0, fill=(0xFFFF,) * 3)), ("double", dict(n=0)), ("cube", dict(n=0, fill=(0, 0, 0))),
            ("tall", dict(n=0)), ("base", dict(n=0, k=8))]
    out += [(good, dict(fill=(1, 2, 3), ok=True)), (good, dict(fill=(0xFFFF, 0x1FF, 0), ok=True)), (good, dict(n=3, ok=True)), (good, dict(n=(1 << 31) - 1, ok=True))]
    # sources no video call, or no bilinear one, takes; frames of 2^31 bytes; a source of 32768 rows
    out += [("double", {}), ("double", dict(k=0)), ("double", dict(dl=(1 << 30,) + (0,) * (2 if family == "nv12" else 4))), ("double", dict(src=FAKE + 1))]
    for name in ("cube", "eac"):
        out += [(name, dict(k=0)), (name, dict(src=None)), (name, dict(sl=broken_s[0]))]
        if not tracked or bilinear:  # (the nearest tracked calls serve a cube source)
            out += [(name, {}), (name, dict(n=2, fill=(1, 2, 3))), (name, dict(dl=(1 << 30,) + (0,) * (2 if family == "nv12" else 4)))]
    for which in ("sl", "dl"):
        out += [("base", {which: (1 << 30,) + (0,) * (2 if family == "nv12" else 4)}), ("tall", {which: (1 << 30,) + (0,) * (2 if family == "nv12" else 4)})]
    out += [("tall", {}), ("tall", dict(k=0)), ("tall", dict(n=5)), ("tall", dict(dst=FAKE + 1))]
    named = {"broken0": broken_s[0], "broken1": broken_d[1]}
    return [(p, {k: named.get(v, v) if isinstance(v, str) else v for k, v in kw.items() if k != "ok"}) for p, kw in out]


def c_cells():
    """[(entry point, sample size, subsampling or None, plan's name, keywords)]: the whole C grid, in order."""
    cells = []
    for name, (family, tracked, bilinear) in CALLS.items():
        for S in (1, 2):
            for sub in (SUBS.values() if family == "planar" else (None,)):
                cells += [(name, S, sub, p, kw) for p, kw in call_cases(family, tracked, bilinear, S, sub)]
    for name, family in QUESTIONS.items():
        for plan in [None] + list(PLANS):
            for S in (-1, 0, 1, 2, 3, 4, 8):
                for sub in (tuple(SUBS.values()) + (-1, 3, 5, 420) if family == "planar" else (None,)):
                    cells.append((name, S, sub, plan, {}))
    return cells


def run_c_cell(lib, made, name, S, sub, plan, kw):
    """-> (n_frames or None for a question, status, pb_last_error() when the status is an error)."""
    h = None if plan is None else made[plan]
    S, sub = kw.get("S", S), kw.get("sub", sub)
    if name in QUESTIONS:
        rc = getattr(lib, name)(h, S) if QUESTIONS[name] == "nv12" else getattr(lib, name)(h, sub, S)
        return None, rc, lib.pb_last_error().decode() if rc < 0 else ""
    family, tracked, _ = CALLS[name]
    cls = nat.pb_nv12_layout if family == "nv12" else nat.pb_planar_layout
    sl, dl = (None if kw.get(w) is None else cls(*kw[w]) for w in ("sl", "dl"))
    fill = None if kw.get("fill") is None else (C.c_uint16 * 3)(*kw["fill"])
    n = kw.get("n", 1)
    args = [h] + ([kw.get("table", FAKE), kw.get("k", 1)] if tracked else []) + [kw.get("src", FAKE), kw.get("dst", FAKE), n,
            None if sl is None else C.addressof(sl), None if dl is None else C.addressof(dl)] + ([sub] if family == "planar" else []) + [
            S, None if fill is None else C.addressof(fill), None]
    rc = getattr(lib, name)(*args)
    return n, rc, lib.pb_last_error().decode() if rc != 0 else ""


def record_c():
    lib = nat.load()
    with plans() as made:
        assert all(is_deferred(h) for h in made.values())
        return [run_c_cell(lib, made, *cell) for cell in c_cells()]


# ---- the Python grid --------------------------------------------------------------------------------------------------------------------
class FakeDevice:
    """Passes nat.is_device_array's test without a device: the checks under test run before anything touches it."""

    def __init__(self, shape, dtype):
        self.shape, self.dtype = tuple(shape), np.dtype(dtype)

    def data_ptr(self):
        return FAKE


@contextlib.contextmanager
def stand_ins():
    mp = pytest.MonkeyPatch()
    mp.setattr(nat, "is_device_array", lambda a: isinstance(a, FakeDevice))
    mp.setattr(nat, "is_tensor", lambda a: False)
    mp.setattr(nat, "require_gpu", lambda: None)
    mp.setattr(nat, "device_index_of", lambda a: 0)
    mp.setattr(nat, "on_device", lambda d: contextlib.nullcontext())
    mp.setattr(nat, "current_stream", lambda: 0)
    mp.setattr(nat, "empty", lambda shape, dtype, like=None, device=None: FakeDevice(shape, dtype))
    try:
        yield
    finally:
        mp.undo()


def _outcome(fn):
    try:
        out = fn()
    except Exception as exc:  # (the facade's argument errors are part of its behaviour)
        return [type(exc).__name__, str(exc)]
    if isinstance(out, tuple):  # (the shared source helper's answer)
        return ["tuple"] + [[list(v.shape), v.dtype.name] if isinstance(v, FakeDevice) else (v.name if isinstance(v, np.dtype) else
                            list(v) if isinstance(v, tuple) else None if v is None else v if isinstance(v, (int, str, bool)) else type(v).__name__) for v in out]
    assert out is None or isinstance(out, bool), out  # (a question's answer, or a call without frames: nothing else gets through)
    return ["result", repr(out)]


def _rot(n, k=None, dtype=np.float64):
    return FakeDevice((n, 3, 3) if k is None else (n, k, 3, 3), dtype)


def py_cells():
    """[(label, thunk)]: the facade's grid.  Plans: pano 4 x 8 -> 6 x 12 for the plain calls and the same shapes from a double-fisheye
    source for the tracked ones (a tracked call is served on a deferred plan), and the odd-dimension plans."""
    pano = nat.Plan(nat.make_proj(nat.KIND_PANO, *DST_HW), [], nat.make_proj(nat.KIND_PANO, *SRC_HW), defer=True)
    double = nat.Plan(nat.make_proj(nat.KIND_PANO, *DST_HW), [], nat.make_proj(*DOUBLE), defer=True)
    odd = {name: nat.Plan(nat.make_proj(nat.KIND_PANO, *d), [], nat.make_proj(nat.KIND_PANO, *s), defer=True) for name, (s, d) in ODD.items()}
    (h, w), (Hd, Wd) = SRC_HW, DST_HW
    cells = []

    def add(label, fn):
        cells.append((label, fn))

    families = [("nv12", None)] + [("planar", s) for s in ("444", "422", "420", nat.PLANAR_420)]
    def family(fam, sub):  # (a function: its cells close over the family, not over a loop variable)
        sa = () if fam == "nv12" else (sub,)  # the subsampling argument, where the family has one
        tag = fam if sub is None else f"{fam}/{sub}"
        sid = None if sub is None else nat.planar_subsampling(sub)
        for plan_name, plan in [("pano", pano), ("double", double)] + list(odd.items()):
            for S in (1, 2, 3, 0):
                for interp in ("nearest", "bilinear"):
                    add(f"{tag} supported {plan_name} S={S} {interp}", lambda p=plan, S=S, i=interp: getattr(p, f"{fam}_supported")(*sa, S, interpolation=i))
        for interp in ("catmull-rom", "cubic", None):
            add(f"{tag} supported interpolation={interp}", lambda i=interp: getattr(pano, f"{fam}_supported")(*sa, interpolation=i))
            add(f"{tag} remap interpolation={interp}", lambda i=interp: getattr(pano, f"remap_{fam}")(FakeDevice((1,), np.uint8), *sa, interpolation=i))
            add(f"{tag} remap_track interpolation={interp}", lambda i=interp: getattr(double, f"remap_track_{fam}")(FakeDevice((1,), np.uint8), _rot(1), *sa, interpolation=i))
            add(f"{tag} launch interpolation={interp}", lambda i=interp: getattr(pano, f"launch_{fam}")(FAKE, FAKE, *sa, interpolation=i))
            add(f"{tag} launch_track interpolation={interp}", lambda i=interp: getattr(double, f"launch_track_{fam}")(FAKE, 1, FAKE, FAKE, *sa, interpolation=i))
        if fam == "nv12":
            ns, nd = None, None
            good = [(3 * h // 2, w), (3, 3 * h // 2, w), (1, 3 * h // 2, w)]
            bad = [(3 * h // 2 * w,), (3 * h // 2, w + 1), (2, 3, 3 * h // 2, w), (h, w), (), (3 * h // 2, w, 1)]
            src_layouts = [(16, 80, 256), {"pitch": 16}, (0, 0, 96), nat.pb_nv12_layout(16, 0, 0)]
            dst_layouts = [(32, 256, 512), {"frame_stride": 512}, (10, 0, 0), (0, 8, 0)]
            bad_layouts = [{"pich": 16}, {"chroma_pitch": 16}, (1, 2), (1, 2, 3, 4, 5)]
            span_s, span_d = 80 + 16 * 2, 256 + 32 * 3
        else:
            ns, nd = nat.planar_frame_samples(h, w, sid), nat.planar_frame_samples(Hd, Wd, sid)
            good = [(ns,), (3, ns), (1, ns)] + ([(3, h, w), (2, 3, h, w)] if sid == nat.PLANAR_444 else [])
            bad = [(h * 3 // 2, w), (ns - 1,), (ns + 1,), (3, h, w), (2 * ns,), (2, 3, h, w), (h, w, 3), (3, w, h), (), (1, 1, ns)]
            bad = [b for b in bad if b not in good]
            src_layouts = [(16, 8, 80, 128, 256), {"pitch": 16}, (0, 0, 0, 0, 512), nat.pb_planar_layout(16, 0, 0, 0, 0), (0, 0, 128, 64, 256)]
            dst_layouts = [(32, 16, 256, 384, 1024), {"frame_stride": 1024}, (10, 0, 0, 0, 0), (0, 0, 8, 0, 0), (0, 0, 0, 0, 8), (0, 2, 0, 0, 0)]
            bad_layouts = [{"uv_offset": 16}, {"pich": 16}, (1, 2, 3), (1, 2)]
            span_s = None
        def calls(tracked):
            plan = double if tracked else pano
            method = getattr(plan, f"remap_track_{fam}" if tracked else f"remap_{fam}")
            kind = "remap_track" if tracked else "remap"

            def remap(src, n=None, _m=method, _t=tracked, **kw):
                rot = kw.pop("rotations", None)
                return _m(src, *(((_rot(n) if rot is None else rot),) if _t else ()), *sa, **kw)

            def frames(shp):
                return shp[0] if len(shp) == (3 if fam == "nv12" else (4 if len(shp) >= 3 else 2)) else 1

            add(f"{tag} {kind} host array", lambda r=remap: r(np.zeros(good[0], np.uint8), 1))
            add(f"{tag} {kind} none", lambda r=remap: r(None, 1))
            for dt in (np.float32, np.int16, np.int8, np.uint32, np.float64):
                add(f"{tag} {kind} dtype {np.dtype(dt).name}", lambda r=remap, dt=dt: r(FakeDevice(good[0], dt), 1))
            for interp in ("nearest", "bilinear"):
                for dt in (np.uint8, np.uint16):
                    for shp in good:
                        add(f"{tag} {kind} {interp} {np.dtype(dt).name} good {shp}", lambda r=remap, dt=dt, shp=shp, i=interp: r(FakeDevice(shp, dt), frames(shp), interpolation=i))
                        add(f"{tag} {kind} {interp} {np.dtype(dt).name} good {shp} fill", lambda r=remap, dt=dt, shp=shp, i=interp: r(FakeDevice(shp, dt), frames(shp), interpolation=i, fill=(1, 2, 3)))
            for dt in (np.uint8, np.uint16):
                S = np.dtype(dt).itemsize
                for shp in bad:
                    add(f"{tag} {kind} {np.dtype(dt).name} bad {shp}", lambda r=remap, dt=dt, shp=shp: r(FakeDevice(shp, dt), 1))
                # frames at a layout: a 1-D buffer, counted by the stride; too short; not 1-D
                for li, l in enumerate(src_layouts):
                    for count in (1, 40, 139, 140, 256, 300, 700, 2000):
                        add(f"{tag} {kind} {np.dtype(dt).name} src_layout {li} x{count}", lambda r=remap, dt=dt, l=l, c=count: r(FakeDevice((c,), dt), 1, src_layout=l))
                    add(f"{tag} {kind} {np.dtype(dt).name} src_layout {li} 2-D", lambda r=remap, dt=dt, l=l: r(FakeDevice((3, 256), dt), 3, src_layout=l))
                    add(f"{tag} {kind} {np.dtype(dt).name} src_layout {li} out", lambda r=remap, dt=dt, l=l: r(FakeDevice((700,), dt), 1, src_layout=l, out=FakeDevice((5000,), dt), dst_layout=dst_layouts[0]))
                for li, l in enumerate(bad_layouts):
                    add(f"{tag} {kind} {np.dtype(dt).name} bad src_layout {li}", lambda r=remap, dt=dt, l=l: r(FakeDevice((700,), dt), 1, src_layout=l))
                    add(f"{tag} {kind} {np.dtype(dt).name} bad dst_layout {li}", lambda r=remap, dt=dt, l=l: r(FakeDevice(good[0], dt), 1, out=FakeDevice((5000,), dt), dst_layout=l))
                # out: the wrong shape, dtype, kind or size; a destination layout without it
                src1, srcN = good[0], good[1]
                outs = [(3 * Hd // 2, Wd), (3, 3 * Hd // 2, Wd), (1, 3 * Hd // 2, Wd), (nd or 7,), (3, nd or 7), (1, nd or 7), (3, Hd, Wd), (2, 3, Hd, Wd), (Hd, Wd),
                        (3 * Hd // 2 * Wd,), ()]
                for shp in outs:
                    add(f"{tag} {kind} {np.dtype(dt).name} out {shp}", lambda r=remap, dt=dt, shp=shp: r(FakeDevice(src1, dt), 1, out=FakeDevice(shp, dt)))
                    add(f"{tag} {kind} {np.dtype(dt).name} batched out {shp}", lambda r=remap, dt=dt, shp=shp: r(FakeDevice(srcN, dt), 3, out=FakeDevice(shp, dt)))
                if fam == "planar" and sid == nat.PLANAR_444:
                    for shp in outs:
                        add(f"{tag} {kind} {np.dtype(dt).name} cube out {shp}", lambda r=remap, dt=dt, shp=shp: r(FakeDevice((3, h, w), dt), 1, out=FakeDevice(shp, dt)))
                        add(f"{tag} {kind} {np.dtype(dt).name} batched cube out {shp}", lambda r=remap, dt=dt, shp=shp: r(FakeDevice((2, 3, h, w), dt), 2, out=FakeDevice(shp, dt)))
                other = np.uint16 if S == 1 else np.uint8
                add(f"{tag} {kind} {np.dtype(dt).name} out dtype", lambda r=remap, dt=dt, o=other: r(FakeDevice(src1, dt), 1, out=FakeDevice((3 * Hd // 2, Wd) if fam == "nv12" else (nd,), o)))
                add(f"{tag} {kind} {np.dtype(dt).name} out host", lambda r=remap, dt=dt: r(FakeDevice(src1, dt), 1, out=np.zeros((3 * Hd // 2, Wd) if fam == "nv12" else (nd,), dt)))
                for li, l in enumerate(dst_layouts):
                    add(f"{tag} {kind} {np.dtype(dt).name} dst_layout {li} no out", lambda r=remap, dt=dt, l=l: r(FakeDevice(src1, dt), 1, dst_layout=l))
                    for count in (1, 100, 351, 352, 700, 1500, 3000):
                        add(f"{tag} {kind} {np.dtype(dt).name} dst_layout {li} out x{count}", lambda r=remap, dt=dt, l=l, c=count: r(FakeDevice(src1, dt), 1, out=FakeDevice((c,), dt), dst_layout=l))
                        add(f"{tag} {kind} {np.dtype(dt).name} dst_layout {li} batched out x{count}", lambda r=remap, dt=dt, l=l, c=count: r(FakeDevice(srcN, dt), 3, out=FakeDevice((c,), dt), dst_layout=l))
                    add(f"{tag} {kind} {np.dtype(dt).name} dst_layout {li} 2-D out", lambda r=remap, dt=dt, l=l: r(FakeDevice(src1, dt), 1, out=FakeDevice((30, 100), dt), dst_layout=l))
            # the dimension rule, per plan
            for name, p in odd.items():
                m = getattr(p, f"remap_track_{fam}" if tracked else f"remap_{fam}")
                add(f"{tag} {kind} {name}", lambda m=m: m(FakeDevice((1,), np.uint8), *((_rot(1),) if tracked else ()), *sa))
                add(f"{tag} {kind} {name} host array", lambda m=m: m(np.zeros(1, np.uint8), *((_rot(1),) if tracked else ()), *sa))
            if tracked:  # a frame count that does not match the table; tables that are none
                for shp in good:
                    for n_tab in (0, 1, 2, 3, 4):
                        add(f"{tag} {kind} {shp} with {n_tab} rotations", lambda r=remap, shp=shp, n=n_tab: r(FakeDevice(shp, np.uint8), n))
                    add(f"{tag} {kind} {shp} with k=2", lambda r=remap, shp=shp: r(FakeDevice(shp, np.uint8), rotations=_rot(frames(shp), 2)))
                    add(f"{tag} {kind} {shp} with k=9", lambda r=remap, shp=shp: r(FakeDevice(shp, np.uint8), rotations=_rot(frames(shp), 9)))
                for rot in (_rot(1, dtype=np.float32), FakeDevice((1, 3, 4), np.float64), FakeDevice((3, 3), np.float64), np.zeros((2, 3, 3)), np.zeros((1, 2, 2)), 7, [],
                            [np.eye(3)] * 2):
                    add(f"{tag} {kind} rotations {type(rot).__name__} {getattr(rot, 'shape', None)} {getattr(rot, 'dtype', None)}", lambda r=remap, rot=rot: r(FakeDevice(good[0], np.uint8), rotations=rot))
                add(f"{tag} {kind} bad frames before a bad table", lambda r=remap: r(FakeDevice(bad[0], np.uint8), rotations=_rot(1, dtype=np.float32)))
                add(f"{tag} {kind} a bad table before a bad out", lambda r=remap: r(FakeDevice(good[0], np.uint8), 2, out=FakeDevice((1,), np.uint8)))
        calls(False)
        calls(True)
        if fam == "planar":
            for bad_sub in ("411", 7, -1, None, True, "4:2:1", 1.5):
                add(f"planar subsampling {bad_sub!r} [{sub}]", lambda b=bad_sub: pano.remap_planar(FakeDevice((1,), np.uint8), b))
                add(f"planar supported subsampling {bad_sub!r} [{sub}]", lambda b=bad_sub: pano.planar_supported(b))
                add(f"planar launch subsampling {bad_sub!r} [{sub}]", lambda b=bad_sub: pano.launch_planar(FAKE, FAKE, b))
                add(f"planar launch_track subsampling {bad_sub!r} [{sub}]", lambda b=bad_sub: double.launch_track_planar(FAKE, 1, FAKE, FAKE, b))
                add(f"planar remap_track subsampling {bad_sub!r} [{sub}]", lambda b=bad_sub: double.remap_track_planar(FakeDevice((1,), np.uint8), _rot(1), b))
        # the raw calls: refused by the library (a deferred plan; a double-fisheye source)
        for S in (1, 2, 3):
            for interp in ("nearest", "bilinear"):
                for li, (sl, dl) in enumerate([(None, None), (src_layouts[0], dst_layouts[0]), (src_layouts[1], None), (None, dst_layouts[2]), (dst_layouts[2], None),
                                               (bad_layouts[0], None), (None, bad_layouts[2])]):
                    for fill in (None, (1, 2, 3)):
                        add(f"{tag} launch S={S} {interp} layouts {li} fill={fill}", lambda S=S, i=interp, sl=sl, dl=dl, f=fill: getattr(pano, f"launch_{fam}")(
                            FAKE, FAKE, *sa, 1, 0, S, f, sl, dl, interpolation=i))
                        add(f"{tag} launch_track S={S} {interp} layouts {li} fill={fill}", lambda S=S, i=interp, sl=sl, dl=dl, f=fill: getattr(double, f"launch_track_{fam}")(
                            FAKE, 1, FAKE, FAKE, *sa, 1, 0, S, f, sl, dl, interpolation=i))
                add(f"{tag} launch S={S} {interp} no frames", lambda S=S, i=interp: getattr(pano, f"launch_{fam}")(FAKE, FAKE, *sa, 0, 0, S, interpolation=i))
                add(f"{tag} launch S={S} {interp} misaligned", lambda S=S, i=interp: getattr(pano, f"launch_{fam}")(FAKE + 1, FAKE, *sa, 1, 0, S, interpolation=i))
                add(f"{tag} launch_track S={S} {interp} k=0", lambda S=S, i=interp: getattr(double, f"launch_track_{fam}")(FAKE, 0, FAKE, FAKE, *sa, 1, 0, S, interpolation=i))
                add(f"{tag} launch_track S={S} {interp} no table", lambda S=S, i=interp: getattr(double, f"launch_track_{fam}")(None, 1, FAKE, FAKE, *sa, 1, 0, S, interpolation=i))
                add(f"{tag} launch_track S={S} {interp} no frames", lambda S=S, i=interp: getattr(double, f"launch_track_{fam}")(FAKE, 1, FAKE, FAKE, *sa, 0, 0, S, interpolation=i))

    for fam, sub in families:
        family(fam, sub)
    return cells, (pano, double, odd)


def record_py():
    with stand_ins():
        cells, keep = py_cells()
        assert all(is_deferred(p._h) for p in keep[:2] + tuple(keep[2].values()))
        out = [[label, _outcome(fn)] for label, fn in cells]
        del cells, keep
    return out


# ---- the fixture ------------------------------------------------------------------------------------------------------------------------
def _digest(labels):
    return hashlib.sha256(json.dumps(labels).encode()).hexdigest()


def c_labels():
    return [[name, S, sub, plan, {k: list(v) if isinstance(v, tuple) else v for k, v in sorted(kw.items())}] for name, S, sub, plan, kw in c_cells()]


def check_grid(c_results):
    """The two conditions on the C grid: every plan is deferred (``plans()``: PB_PLAN_DEFER, and no call here prepares one), and every call
    with frames comes back INVALID or UNSUPPORTED - a status of 0 or a HIP error there is a bug in the grid, not a result."""
    wrong = [(cell, r) for cell, r in zip(c_labels(), c_results) if r[0] is not None and r[0] > 0 and r[1] not in (INVALID, UNSUPPORTED)]
    assert not wrong, f"{len(wrong)} calls with frames were not refused by an argument or plan check; the first: {wrong[0]}"
    wrong = [(cell, r) for cell, r in zip(c_labels(), c_results) if r[1] not in (0, 1, INVALID, UNSUPPORTED)]
    assert not wrong, f"{len(wrong)} cells came back with another status; the first: {wrong[0]}"


def encode(c_results, py_results):
    check_grid(c_results)
    messages = {}
    c = [[n, rc, messages.setdefault(msg, len(messages))] for n, rc, msg in c_results]
    outcomes = {}
    py = [outcomes.setdefault(json.dumps(o), len(outcomes)) for _, o in py_results]
    return {"c_cells": _digest(c_labels()), "py_cells": _digest([l for l, _ in py_results]), "messages": list(messages), "c": c,
            "outcomes": [json.loads(o) for o in outcomes], "py": py}


def decode(rec):
    return [(n, rc, rec["messages"][m]) for n, rc, m in rec["c"]], [rec["outcomes"][o] for o in rec["py"]]


@pytest.fixture(scope="module")
def golden():
    return json.load(open(GOLDEN))


def test_every_c_call_of_the_grid_comes_back_with_the_recorded_status_and_message(golden):
    want, _ = decode(golden)
    labels = c_labels()
    assert golden["c_cells"] == _digest(labels) and len(want) == len(labels)  # no cell dropped, added or changed
    got = record_c()
    check_grid(got)
    wrong = [(cell, g, w) for cell, g, w in zip(labels, got, want) if tuple(g) != tuple(w)]
    assert not wrong, f"{len(wrong)} of {len(want)} cells differ; the first: {wrong[0][0]}\n got  {wrong[0][1]}\n want {wrong[0][2]}"


def test_every_facade_call_of_the_grid_ends_as_recorded(golden):
    _, want = decode(golden)
    got = json.loads(json.dumps(record_py()))
    assert golden["py_cells"] == _digest([l for l, _ in got]) and len(want) == len(got)
    wrong = [(label, g, w) for (label, g), w in zip(got, want) if g != w]
    assert not wrong, f"{len(wrong)} of {len(want)} cells differ; the first: {wrong[0][0]}\n got  {wrong[0][1]}\n want {wrong[0][2]}"


def test_the_recording_holds_every_message_of_the_video_calls(golden):
    msgs = golden["messages"]
    for exact in ("null argument", "negative frame count", "bytes_per_sample outside {1, 2}", "subsampling outside {PB_PLANAR_444, PB_PLANAR_422, PB_PLANAR_420}",
                  "4:2:0 frames need even source and destination dimensions", "4:2:2 frames need even source and destination widths", "null rotation table",
                  "the rotation table must be 8-byte aligned", "n_rot_per_frame must be at least 1", "the plan's 0 rotations and 9 per frame exceed PB_MAX_ROTATIONS (8)",
                  "the plan's 1 rotations and 8 per frame exceed PB_MAX_ROTATIONS (8)", "the plan's 8 rotations and 1 per frame exceed PB_MAX_ROTATIONS (8)"):
        assert exact in msgs, exact
    for part in ("pitch smaller than a row", "chroma_pitch smaller than a row", "uv_offset smaller than the luma plane", "planes overlap: plane 1 or 2 starts inside plane 0",
                 "planes overlap: planes 1 and 2", "frame_stride smaller than a frame", "frame_stride smaller than a frame: a plane ends beyond it",
                 "bytes (one chroma pair)", "bytes (one sample)", "frame pointers must be multiples of 2 bytes (one chroma pair)", "frame pointers must be multiples of 2 bytes (one sample)",
                 "pb_remap_nv12 takes frames whose planes span less than 2^31 bytes (source pitch or uv_offset)",
                 "pb_remap_nv12 takes frames whose planes span less than 2^31 bytes (destination pitch or uv_offset)",
                 "pb_remap_planar takes frames whose planes span less than 2^31 bytes (source pitch, chroma_pitch, offset1 or offset2)",
                 "pb_remap_planar takes frames whose planes span less than 2^31 bytes (destination pitch, chroma_pitch, offset1 or offset2)",
                 " takes single sources (a double fisheye's blend is sample-typed)", " takes panorama and camera sources (the bilinear definition of video frames covers no cube map)",
                 " takes frames whose planes span less than 2^31 bytes and sources below 32768 px a side",
                 "pb_remap_nv12 takes prepared plans of a single source in a tile mode", "pb_remap_planar takes prepared plans of a single source in a tile mode",
                 "pb_remap_nv12_bilinear takes prepared plans of a single source in a tile mode", "pb_remap_planar_bilinear takes prepared plans of a single source in a tile mode"):
        assert any(part in m for m in msgs), part
    # ... each of the plain ones for both sides, and the tracked refusals under each of the four names
    for side in ("source ", "destination "):
        for part in ("pitch smaller than a row", "chroma_pitch smaller than a row", "uv_offset smaller than the luma plane", "planes overlap: planes 1 and 2",
                     "frame_stride smaller than a frame"):
            assert any(m.startswith(side + part) for m in msgs), (side, part)
    for name in (n for n, (_, tracked, _) in CALLS.items() if tracked):
        assert any(m.startswith(name + " takes single sources") for m in msgs) and any(m.startswith(name + " takes frames whose planes span") for m in msgs), name
    assert {o[0] for o in golden["outcomes"]} == {"PbError", "ValueError", "result"}


if __name__ == "__main__":
    with open(sys.argv[1], "w") as f:
        json.dump(encode(record_c(), json.loads(json.dumps(record_py()))), f, separators=(",", ":"))
        f.write("\n")
