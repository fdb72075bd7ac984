"""CPU-only checks of bilinear rotation tracks for video frames (pb_remap_track_nv12_bilinear, pb_remap_track_planar_bilinear):
the two symbols and their signatures; every PB_ERR_INVALID of the nearest tracked calls comes back from the bilinear call with the same
code and message - on deferred plans with fake pointers: a deferred plan has no device, and every call here is refused (or has no
frames) before anything could be launched -; the refusals; and the ``interpolation`` keyword of the four Plan methods against the
stand-ins of tests/test_rotation_track_host.py."""

import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from photonbend_amd import _device
from photonbend_amd import _native as nat
from photonbend_amd.core import rotation_track
from tests.test_rotation_track_host import FakeTrackLib, env  # noqa: F401  (the stand-in library and its environment)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x1000  # a non-null, 8-byte aligned "device pointer" for calls that must be refused before anything reads it
INVALID, UNSUPPORTED = -1, -3
SUBS = {"444": nat.PLANAR_444, "422": nat.PLANAR_422, "420": nat.PLANAR_420}
NV12_DECLARATION = ("const pb_plan* plan, const double* rot3x3_dev, int n_rot_per_frame, const void* src_dev, void* dst_dev, int n_frames, "
                    "const pb_nv12_layout* src_layout, const pb_nv12_layout* dst_layout, int bytes_per_sample, const uint16_t fill_yuv[3], void* stream")
PLANAR_DECLARATION = ("const pb_plan* plan, const double* rot3x3_dev, int n_rot_per_frame, const void* src_dev, void* dst_dev, int n_frames, "
                      "const pb_planar_layout* src_layout, const pb_planar_layout* dst_layout, int subsampling, int bytes_per_sample, "
                      "const uint16_t fill[3], void* stream")


def _deferred(src=(nat.KIND_PANO, 4, 8), dst=(nat.KIND_PANO, 6, 12), n_rot=0):
    lib = nat.load()
    h = C.c_void_p()
    s, d = nat.make_proj(*src), nat.make_proj(*dst)
    rots = (C.c_double * (9 * max(1, n_rot)))(*([1, 0, 0, 0, 1, 0, 0, 0, 1] * max(1, n_rot)))
    assert lib.pb_plan_create_ex(C.byref(d), rots if n_rot else None, n_rot, C.byref(s), nat.PLAN_DEFER, 0, C.byref(h)) == 0, lib.pb_last_error()
    return lib, h


def nv12(lib, name, plan, table=FAKE, k=1, src=FAKE, dst=FAKE, n=1, sl=None, dl=None, S=1, fill=None):
    sl = None if sl is None else nat.pb_nv12_layout(*sl)
    dl = None if dl is None else nat.pb_nv12_layout(*dl)
    f = None if fill is None else (C.c_uint16 * 3)(*fill)
    rc = getattr(lib, name)(plan, table, k, src, dst, n, None if sl is None else C.addressof(sl), None if dl is None else C.addressof(dl), S,
                            None if f is None else C.addressof(f), None)
    return rc, lib.pb_last_error()


def planar(lib, name, plan, table=FAKE, k=1, src=FAKE, dst=FAKE, n=1, sl=None, dl=None, sub=nat.PLANAR_420, S=1, fill=None):
    sl = None if sl is None else nat.pb_planar_layout(*sl)
    dl = None if dl is None else nat.pb_planar_layout(*dl)
    f = None if fill is None else (C.c_uint16 * 3)(*fill)
    rc = getattr(lib, name)(plan, table, k, src, dst, n, None if sl is None else C.addressof(sl), None if dl is None else C.addressof(dl), sub, S,
                            None if f is None else C.addressof(f), None)
    return rc, lib.pb_last_error()


CALLS = {"nv12": (nv12, "pb_remap_track_nv12", "pb_remap_track_nv12_bilinear"), "planar": (planar, "pb_remap_track_planar", "pb_remap_track_planar_bilinear")}


def test_the_header_declares_the_two_calls_the_library_exports_them_and_the_signatures_bind_them():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "photonbend_hip.h")).read(), flags=re.S)
    # (the return type stands on a line of its own: DESIGN 3.18's header convention)
    decl = {m.group(1): " ".join(m.group(2).split()) for m in re.finditer(r"^int\n(pb_remap_track_\w+_bilinear)\s*\(([^)]*)\)\s*;", text, re.M)}
    assert decl == {"pb_remap_track_nv12_bilinear": NV12_DECLARATION, "pb_remap_track_planar_bilinear": PLANAR_DECLARATION}
    assert re.search(r"#define PB_ABI_VERSION 5\b", text)
    header = open(os.path.join(ROOT, "include", "photonbend_hip.h")).read()
    assert "the definition's bytes exactly" in " ".join(header.split())
    vp = C.c_void_p
    assert nat.SIGNATURES["pb_remap_track_nv12_bilinear"] == nat.SIGNATURES["pb_remap_track_nv12"] == (C.c_int, [vp, vp, C.c_int, vp, vp, C.c_int, vp, vp, C.c_int, vp, vp])
    assert nat.SIGNATURES["pb_remap_track_planar_bilinear"] == nat.SIGNATURES["pb_remap_track_planar"] == (
        C.c_int, [vp, vp, C.c_int, vp, vp, C.c_int, vp, vp, C.c_int, C.c_int, vp, vp])
    lib = nat.load()
    assert hasattr(lib, "pb_remap_track_nv12_bilinear") and hasattr(lib, "pb_remap_track_planar_bilinear")
    assert lib.pb_abi_version() == 5 == nat.ABI_VERSION


def _broken(kind, S):
    """Arguments that break one rule each (and some that break several) on a plan without rotations: null frames, a negative count, the
    layouts, the pointers' alignment, a null or misaligned table, n_rot_per_frame 0 and beyond PB_MAX_ROTATIONS.  EVERY entry must be
    refused: a deferred plan is served by these calls, so one that passed would launch on the fake pointers where there is a device."""
    out = [dict(src=None), dict(dst=None), dict(src=None, dst=None), dict(n=-1), dict(n=-1, table=None), dict(table=None), dict(table=FAKE + 4), dict(k=0),
           dict(k=nat.PB_MAX_ROTATIONS + 1), dict(k=-1), dict(table=None, k=0), dict(dst=None, table=None)]
    if kind == "nv12":
        ok_s, ok_d = (S * 8, S * 8 * 4, S * 8 * 6), (S * 12, S * 12 * 6, S * 12 * 9)
        out += [dict(src=FAKE + S), dict(dst=FAKE + S), dict(src=FAKE + 1)]
        for which, base in (("sl", ok_s), ("dl", ok_d)):
            out += [{which: v} for v in ((base[0] - 2 * S, 0, 0), (0, base[1] - 2 * S, 0), (base[0] + 2 * S, base[1], 0), (0, 0, base[2] - 2 * S),
                                         (0, base[1] + 2 * S, base[2]), (base[0] + S, 0, 0), (0, base[1] + S, 0), (0, 0, base[2] + S))]
            out += [{which: (base[0] - 2 * S, 0, 0), "k": 0}]
    else:
        for which, (h, w) in (("sl", (4, 8)), ("dl", (6, 12))):
            p = S * w
            out += [{which: v} for v in ((p - S, 0, 0, 0, 0), (0, S, 0, 0, 0), (0, 0, p * h - S, 0, 0), (0, 0, 0, p * h - S, 0), (0, 0, 0, 0, p * h))]
            out += [{which: (p - S, 0, 0, 0, 0), "table": None}]
            if S == 2:
                out += [{which: (p + 1, 0, 0, 0, 0)}, {which: (0, 0, 0, 0, 3 * p * h + 1)}]
        if S == 2:
            out += [dict(dst=FAKE + 1)]
    return out


@pytest.mark.parametrize("kind", ["nv12", "planar"])
def test_every_invalid_argument_of_the_nearest_tracked_call_comes_back_with_the_same_code_and_message(kind):
    call, nearest, bilinear = CALLS[kind]
    lib, h = _deferred()  # source 4 x 8, destination 6 x 12
    lib2, odd = _deferred(dst=(nat.KIND_PANO, 6, 11))
    seen = set()
    try:
        subs = [dict(sub=s) for s in SUBS.values()] if kind == "planar" else [{}]
        for S in (1, 2):
            for extra in subs:
                for kw in _broken(kind, S):
                    want = call(lib, nearest, h, S=S, **extra, **kw)
                    assert want[0] == INVALID, (S, extra, kw, want)
                    assert call(lib, bilinear, h, S=S, **extra, **kw) == want, (S, extra, kw)
                    seen.add(want[1])
        # a null plan; a bad sample size; a bad subsampling; odd dimensions (at 4:4:4 they are allowed: no check to compare)
        for plan, kw in [(None, {}), (h, dict(S=0)), (h, dict(S=3)), (h, dict(S=4)), (h, dict(S=3, n=-1)), (odd, {}), (odd, dict(k=0)), (odd, dict(S=3))] + (
                [(h, dict(sub=5)), (h, dict(sub=-1)), (h, dict(sub=3, k=0)), (odd, dict(sub=nat.PLANAR_422))] if kind == "planar" else []):
            want = call(lib2 if plan is odd else lib, nearest, plan, **kw)
            assert want[0] == INVALID, (kw, want)
            assert call(lib2 if plan is odd else lib, bilinear, plan, **kw) == want, kw
            seen.add(want[1])
        # the rotation limit counts the plan's own rotations: PB_MAX_ROTATIONS per frame behind one of the plan's, ...
        assert nat.PB_MAX_ROTATIONS == 8
        for n_rot in (1, 7, 8):
            lib3, p3 = _deferred(n_rot=n_rot)
            try:
                k = 8 - n_rot + 1
                want = (INVALID, f"the plan's {n_rot} rotations and {k} per frame exceed PB_MAX_ROTATIONS (8)".encode())
                assert call(lib3, nearest, p3, k=k) == want == call(lib3, bilinear, p3, k=k)
                if n_rot < 8:
                    assert call(lib3, bilinear, p3, k=k - 1, n=0)[0] == 0
            finally:
                lib3.pb_plan_destroy(p3)
    finally:
        lib.pb_plan_destroy(h)
        lib2.pb_plan_destroy(odd)
    for message in (b"null argument", b"negative frame count", b"bytes_per_sample outside {1, 2}", b"null rotation table", b"the rotation table must be 8-byte aligned",
                    b"n_rot_per_frame must be at least 1", b"the plan's 0 rotations and 9 per frame exceed PB_MAX_ROTATIONS (8)", b"4:2:0 frames need even source and destination dimensions"):
        assert message in seen, message
    assert any(b"pitch smaller than a row" in m for m in seen) and any(b"frame pointers must be multiples of" in m for m in seen)
    if kind == "planar":
        assert b"subsampling outside {PB_PLANAR_444, PB_PLANAR_422, PB_PLANAR_420}" in seen and b"4:2:2 frames need even source and destination widths" in seen


@pytest.mark.parametrize("kind", ["nv12", "planar"])
def test_no_frames_is_ok_with_no_launch_and_no_device(kind):
    call, _, bilinear = CALLS[kind]
    lib, h = _deferred()
    try:
        for S in (1, 2):
            for k in (1, 2, 8):
                assert call(lib, bilinear, h, k=k, n=0, S=S)[0] == 0
                assert call(lib, bilinear, h, k=k, n=0, S=S, fill=(1, 2, 3))[0] == 0
    finally:
        lib.pb_plan_destroy(h)


@pytest.mark.parametrize("kind", ["nv12", "planar"])
def test_double_fisheye_cube_and_equi_angular_cube_sources_and_frames_of_2_31_bytes_are_unsupported(kind):
    call, nearest, bilinear = CALLS[kind]
    sources = {
        "double": ((nat.KIND_DOUBLE, 6, 12, nat.LENS_IDS["equidistant"], 3.3, 3.0, 2.0), b" takes single sources (a double fisheye's blend is sample-typed): convert to RGB8 and use pb_remap_track_u8"),
        "cube": ((nat.KIND_CUBE, 8, 12), b" takes panorama and camera sources"),
        "eac": ((nat.KIND_EAC, 8, 12), b" takes panorama and camera sources"),
    }
    for what, (src, message) in sources.items():
        lib, h = _deferred(src=src)
        try:
            for S in (1, 2):
                rc, msg = call(lib, bilinear, h, S=S)
                assert rc == UNSUPPORTED and msg.startswith(bilinear.encode() + message), (what, msg)
                assert call(lib, bilinear, h, S=S, k=0)[0] == INVALID  # (the argument checks come first)
            if what == "double":  # the nearest tracked call's message, under its own name
                rc, msg = call(lib, nearest, h)
                assert rc == UNSUPPORTED and msg == nearest.encode() + message
        finally:
            lib.pb_plan_destroy(h)
    lib, h = _deferred()
    try:
        dl = ((1 << 30), 0, 0) if kind == "nv12" else ((1 << 30), 0, 0, 0, 0)
        rc, msg = call(lib, bilinear, h, dl=dl)
        assert rc == UNSUPPORTED and msg.startswith(bilinear.encode() + b" takes frames whose planes span less than 2^31 bytes and sources below 32768 px a side"), msg
        assert call(lib, nearest, h, dl=dl)[1] == msg.replace(bilinear.encode(), nearest.encode())
    finally:
        lib.pb_plan_destroy(h)
    lib, h = _deferred(src=(nat.KIND_PANO, 32768, 4), dst=(nat.KIND_PANO, 4, 8))  # (a small frame: the side alone is refused)
    try:
        rc, msg = call(lib, bilinear, h)
        assert rc == UNSUPPORTED and b"sources below 32768 px a side" in msg, msg
    finally:
        lib.pb_plan_destroy(h)


# ---- the four Plan methods against stand-ins --------------------------------------------------------------------------------------------
class FakeVideoTrackLib(FakeTrackLib):
    def _record(self, name, table, k, src, dst, n, S):
        self.calls.append({"fn": name, "table": int(table), "k": int(k), "src": int(src), "dst": int(dst), "n": int(n), "S": int(S)})
        return 0

    def pb_remap_track_nv12(self, plan, table, k, src, dst, n, sl, dl, S, fill, stream):
        return self._record("pb_remap_track_nv12", table, k, src, dst, n, S)

    def pb_remap_track_nv12_bilinear(self, plan, table, k, src, dst, n, sl, dl, S, fill, stream):
        return self._record("pb_remap_track_nv12_bilinear", table, k, src, dst, n, S)

    def pb_remap_track_planar(self, plan, table, k, src, dst, n, sl, dl, sub, S, fill, stream):
        return self._record("pb_remap_track_planar", table, k, src, dst, n, S)

    def pb_remap_track_planar_bilinear(self, plan, table, k, src, dst, n, sl, dl, sub, S, fill, stream):
        return self._record("pb_remap_track_planar_bilinear", table, k, src, dst, n, S)


@pytest.fixture
def video_env(env, monkeypatch):  # noqa: F811
    _, plans = env
    lib = FakeVideoTrackLib()
    monkeypatch.setattr(_device, "_lib", lambda: lib)
    monkeypatch.setattr(nat, "load", lambda: lib)
    return lib, plans


def test_the_four_methods_take_the_keyword_only_interpolation_with_the_nearest_default():
    for m in (nat.Plan.launch_track_nv12, nat.Plan.remap_track_nv12, nat.Plan.launch_track_planar, nat.Plan.remap_track_planar):
        p = inspect.signature(m).parameters["interpolation"]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default == "nearest", m.__name__


def test_the_default_calls_the_nearest_function_bilinear_the_new_one_and_anything_else_is_the_value_error(video_env):
    lib, plans = video_env
    plan = plans[0]  # 4 x 8 -> 4 x 8: packed NV12 frames are (6, 8), packed 4:2:0 planar frames 48 samples
    mats = rotation_track(np.arange(9.0).reshape(3, 3))
    for dt in (np.uint8, np.uint16):
        S = np.dtype(dt).itemsize
        semi, flat = _device.DeviceArray((3, 6, 8), dt), _device.DeviceArray((3, 48), dt)
        routes = [
            (lambda **kw: plan.remap_track_nv12(semi, mats, **kw), semi, "pb_remap_track_nv12"),
            (lambda **kw: plan.remap_track_planar(flat, mats, "420", **kw), flat, "pb_remap_track_planar"),
        ]
        for run, src, name in routes:
            for kw, want in (({}, name), (dict(interpolation="nearest"), name), (dict(interpolation="bilinear"), name + "_bilinear")):
                out = run(**kw)
                c = lib.calls[-1]
                assert (c["fn"], c["k"], c["src"], c["dst"], c["n"], c["S"]) == (want, 1, src.data_ptr(), out.data_ptr(), 3, S), (kw, c)
                assert out.shape == src.shape and out.dtype == np.dtype(dt)
            n_calls, n_log = len(lib.calls), len(lib.log)
            for bad in ("cubic", "catmull-rom", "linear", ""):
                with pytest.raises(ValueError, match="interpolation must be one of|video frames are sampled"):
                    run(interpolation=bad)
            with pytest.raises(ValueError, match="video frames are sampled with one of 'nearest', 'bilinear'"):
                run(interpolation="catmull-rom")
            with pytest.raises(ValueError, match="the table holds"):  # a table whose length is not the frame count
                (plan.remap_track_nv12(semi, mats[:2], interpolation="bilinear") if src is semi else plan.remap_track_planar(flat, mats[:2], "420", interpolation="bilinear"))
            assert len(lib.calls) == n_calls and len(lib.log) == n_log, "a refused call reached the library or the device"
        # the raw launches
        for launch, name in ((lambda **kw: plan.launch_track_nv12(FAKE, 1, FAKE, FAKE, 2, 0, S, **kw), "pb_remap_track_nv12"),
                             (lambda **kw: plan.launch_track_planar(FAKE, 1, FAKE, FAKE, "444", 2, 0, S, **kw), "pb_remap_track_planar")):
            launch()
            assert lib.calls[-1]["fn"] == name
            launch(interpolation="bilinear")
            assert (lib.calls[-1]["fn"], lib.calls[-1]["n"], lib.calls[-1]["S"]) == (name + "_bilinear", 2, S)
            n_calls = len(lib.calls)
            with pytest.raises(ValueError):
                launch(interpolation="cubic")
            assert len(lib.calls) == n_calls
