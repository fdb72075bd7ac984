"""CPU-only checks of pb_remap_interp_px / pb_remap_interp_px_supported: the symbols and their signatures, pb_remap_px's frame
checks and the later checks in their order - a deferred plan has no device and every call here is refused before anything could be
launched -, Plan.remap_px's ``interpolation`` keyword against a stand-in for the library (tests/test_host_memory.py's), the two derived
tolerances, and the cap on the edge band that keeps the GPU test's excuse rule (tests/test_hip_px_interp.py) from hiding a failure."""

import contextlib
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from photonbend_amd import _device, _hostpipe
from photonbend_amd import _native as nat
from tests import interp_cases as ic
from tests import px_interp_cases as pc
from tests.test_host_memory import FakePipeLib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x1000  # a non-null, 8-byte aligned "device pointer" for calls that must be refused before anything reads it
OK, INVALID, UNSUPPORTED = 0, -1, -3
BIL, CR = 1, 2  # PB_INTERP_BILINEAR, PB_INTERP_CATMULL_ROM
FORMATS = [(1, 1), (2, 1), (3, 1), (4, 1), (1, 2), (2, 2), (3, 2), (4, 2)]  # (channels, sample_bytes)


def _plan(kind=nat.KIND_PANO, fov=None):
    lib = nat.load()
    h = ctypes.c_void_p()
    p = nat.make_proj(nat.KIND_PANO, 4, 8)
    s = nat.make_proj(kind, 4, 8) if fov is None else nat.make_proj(kind, 4, 8, lens=0, fov=fov, f_distance=2.0)
    assert lib.pb_plan_create_ex(ctypes.byref(p), None, 0, ctypes.byref(s), nat.PLAN_DEFER, 0, ctypes.byref(h)) == 0, lib.pb_last_error()
    return lib, h


@pytest.fixture
def deferred():
    lib, h = _plan()
    yield lib, h
    lib.pb_plan_destroy(h)


@pytest.fixture
def deferred_double():
    lib, h = _plan(nat.KIND_DOUBLE, fov=3.4)
    yield lib, h
    lib.pb_plan_destroy(h)


def interp(lib, h, src=FAKE, dst=FAKE, n=1, ss=0, ds=0, ch=4, sb=1, mode=BIL):
    return lib.pb_remap_interp_px(h, src, dst, n, ss, ds, ch, sb, mode, None), lib.pb_last_error()


def test_the_two_symbols_exist_with_the_declared_signatures_and_the_abi_is_still_5():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "photonbend_hip.h")).read(), flags=re.S)
    decl = {m.group(1): " ".join(m.group(2).split()) for m in re.finditer(r"\bint\s+(pb_remap_interp_px\w*)\s*\(([^)]*)\)\s*;", text)}
    assert decl == {
        "pb_remap_interp_px": "const pb_plan* plan, const void* src_dev, void* dst_dev, int n_frames, size_t src_frame_stride, size_t dst_frame_stride, "
                              "int channels, int sample_bytes, int interpolation, void* stream",
        "pb_remap_interp_px_supported": "const pb_plan* plan, int channels, int sample_bytes, int interpolation",
    }
    assert re.search(r"^int\npb_remap_interp_px\(", text, flags=re.M) and re.search(r"^int\npb_remap_interp_px_supported\(", text, flags=re.M)  # (DESIGN 3.18's form)
    assert re.search(r"#define PB_ABI_VERSION 5\b", text)
    assert re.search(r"#define PB_INTERP_BILINEAR 1\b", text) and re.search(r"#define PB_INTERP_CATMULL_ROM 2\b", text)
    vp, C = ctypes.c_void_p, ctypes
    assert nat.SIGNATURES["pb_remap_interp_px"] == (C.c_int, [vp, vp, vp, C.c_int, C.c_size_t, C.c_size_t, C.c_int, C.c_int, C.c_int, vp])
    assert nat.SIGNATURES["pb_remap_interp_px_supported"] == (C.c_int, [vp, C.c_int, C.c_int, C.c_int])
    lib = nat.load()
    assert hasattr(lib, "pb_remap_interp_px") and hasattr(lib, "pb_remap_interp_px_supported") and lib.pb_abi_version() == 5 == nat.ABI_VERSION
    assert (nat.TRACK_INTERP_IDS["bilinear"], nat.TRACK_INTERP_IDS["catmull-rom"]) == (BIL, CR)


def test_every_frame_argument_refusal_of_pb_remap_px_comes_back_with_its_status_and_message(deferred):
    lib, h = deferred
    for ch, sb in FORMATS:
        B = ch * sb
        for args in ((h, None, None, 1), (h, None, FAKE, 1), (h, FAKE, None, 3), (h, None, None, 0), (h, None, None, -1), (None, None, None, -1),
                     (None, FAKE, FAKE, 1), (h, FAKE, FAKE, -1), (h, FAKE, FAKE, -7)):
            want = lib.pb_remap_px(*args, 0, 0, B, None), lib.pb_last_error()
            for mode in (BIL, CR, 0, 9):  # (the frame arguments come before the interpolation)
                got = lib.pb_remap_interp_px(*args, 0, 0, ch, sb, mode, None), lib.pb_last_error()
                assert got == want and got[0] == INVALID and got[1] in (b"null argument", b"negative frame count"), (ch, sb, args, mode, got, want)
        frame, a = 4 * 8 * B, nat.px_align(B)
        layouts = [(FAKE, FAKE, 1, 0, frame - a), (FAKE, FAKE, 2, frame - a, 0)]  # a stride smaller than a frame
        if a > 1:  # misaligned pointers and strides, per pixel size
            layouts += [(FAKE + 1, FAKE, 1, 0, 0), (FAKE, FAKE + a // 2, 1, 0, 0), (FAKE, FAKE, 1, frame + 1, 0), (FAKE, FAKE, 1, 0, frame + a // 2),
                        (FAKE, FAKE, 2, frame + a + 1, frame + a)]
        for s, d, n, ss, ds in layouts:
            want = lib.pb_remap_px(h, s, d, n, ss, ds, B, None), lib.pb_last_error()
            for mode in (BIL, CR, 0):
                got = interp(lib, h, src=s, dst=d, n=n, ss=ss, ds=ds, ch=ch, sb=sb, mode=mode)
                assert got == want and got[0] == INVALID, (ch, sb, (s, d, n, ss, ds), got, want)
                assert b"smaller than a frame" in got[1] or got[1] == f"frame pointers and strides must be multiples of {a} bytes for {B}-byte pixels".encode()


def test_the_later_checks_follow_in_their_order(deferred):
    lib, h = deferred
    # a format outside the sets is checked at the weakest alignment: odd pointers and strides pass the frame checks and meet the next one
    assert interp(lib, h, src=FAKE + 1, dst=FAKE + 3, ch=5, sb=1, mode=7) == (INVALID, b"interpolation must be PB_INTERP_BILINEAR or PB_INTERP_CATMULL_ROM")
    for mode in (-1, 3, 7, 100):
        for ch, sb in FORMATS + [(0, 1), (5, 2), (1, 3)]:  # the interpolation comes before the format
            assert interp(lib, h, ch=ch, sb=sb, mode=mode) == (INVALID, b"interpolation must be PB_INTERP_BILINEAR or PB_INTERP_CATMULL_ROM"), (mode, ch, sb)
            assert lib.pb_remap_interp_px_supported(h, ch, sb, mode) == INVALID
    # PB_INTERP_NEAREST is another call's: the message names it
    for ch, sb in FORMATS + [(0, 1)]:
        for n in (0, 1):
            rc, msg = interp(lib, h, ch=ch, sb=sb, mode=0, n=n)
            assert rc == INVALID and b"PB_INTERP_NEAREST" in msg and b"pb_remap_px" in msg, (ch, sb, msg)
        assert lib.pb_remap_interp_px_supported(h, ch, sb, 0) == INVALID and b"pb_remap_px" in lib.pb_last_error()
    # the format comes before the plan: INVALID on a deferred plan, which a valid format finds UNSUPPORTED
    for ch, sb in ((0, 1), (5, 1), (0, 2), (5, 2), (1, 0), (1, 3), (4, 0), (4, 3), (-1, 1), (2, 4), (6, 1), (2, 3)):
        for mode in (BIL, CR):
            for n in (0, 1):
                rc, msg = interp(lib, h, ch=ch, sb=sb, mode=mode, n=n)
                assert rc == INVALID and b"channels" in msg and b"sample_bytes" in msg, (ch, sb, n, msg)
            assert lib.pb_remap_interp_px_supported(h, ch, sb, mode) == INVALID, (ch, sb)
    assert lib.pb_remap_interp_px_supported(None, 4, 1, BIL) == INVALID and lib.pb_last_error() == b"null argument"


def test_deferred_and_double_fisheye_plans_are_unsupported(deferred, deferred_double):
    for lib, h in (deferred, deferred_double):
        for ch, sb in FORMATS:
            if (ch, sb) == (3, 1):
                continue
            for mode in (BIL, CR):
                assert lib.pb_remap_interp_px_supported(h, ch, sb, mode) == 0, (ch, sb, mode)
                rc, msg = interp(lib, h, ch=ch, sb=sb, mode=mode)
                assert rc == UNSUPPORTED and msg.startswith(b"pb_remap_interp_px takes prepared plans") and b"pb_sample_map_bilinear_px" in msg, (ch, sb, mode, msg)
                # pb_remap_px's refusal of the same plan, with this call's name and way out
                assert lib.pb_remap_px(h, FAKE, FAKE, 1, 0, 0, ch * sb, None) == UNSUPPORTED
                assert lib.pb_last_error().split(b":")[0].replace(b"pb_remap_px", b"pb_remap_interp_px") == msg.split(b":")[0]
        # three uint8 channels are pb_remap_bilinear_u8 / pb_remap_catmull_rom_u8 themselves, which take every plan
        assert lib.pb_remap_interp_px_supported(h, 3, 1, BIL) == 1 and lib.pb_remap_interp_px_supported(h, 3, 1, CR) == 1
    plan = nat.Plan(nat.make_proj(nat.KIND_PANO, 4, 8), [], nat.make_proj(nat.KIND_PANO, 4, 8), defer=True)
    assert not plan.px_interp_supported(4, 1, "bilinear") and not plan.px_interp_supported(1, 2, "catmull-rom") and plan.px_interp_supported(3, 1, "bilinear")
    with pytest.raises(nat.PbError):
        plan.px_interp_supported(5, 1, "bilinear")
    with pytest.raises(ValueError):
        plan.px_interp_supported(4, 1, "nearest")
    with pytest.raises(ValueError):
        plan.px_interp_supported(4, 1, "cubic")


def test_no_frames_is_ok_and_launches_nothing(deferred, deferred_double):
    for lib, h in (deferred, deferred_double):
        for ch, sb in FORMATS:
            for mode in (BIL, CR):
                assert lib.pb_remap_interp_px(h, FAKE, FAKE, 0, 0, 0, ch, sb, mode, None) == OK, (ch, sb, mode)
                assert lib.pb_remap_interp_px(h, None, None, 0, 0, 0, ch, sb, mode, None) == INVALID  # (pb_remap_px's rule: no null frames)


# ---- Plan.remap_px's keyword against a stand-in ---------------------------------------------------------------------------------------
class FakeInterpPxLib(FakePipeLib):
    """tests/test_host_memory.py's stand-in with the two px launches: they record their arguments."""

    def __init__(self):
        super().__init__()
        self.calls = []

    def pb_remap_px(self, plan, src, dst, n, ss, ds, bpp, stream):
        self.calls.append(("pb_remap_px", int(src), int(dst), int(n), int(ss), int(ds), int(bpp), int(stream or 0)))
        return 0

    def pb_remap_interp_px(self, plan, src, dst, n, ss, ds, channels, sample_bytes, interpolation, stream):
        self.calls.append(("pb_remap_interp_px", int(src), int(dst), int(n), int(ss), int(ds), int(channels), int(sample_bytes), int(interpolation), int(stream or 0)))
        return 0


@pytest.fixture
def env(monkeypatch):
    p = nat.make_proj(nat.KIND_PANO, 4, 8)
    plan = nat.Plan(p, [], p, defer=True)
    lib = FakeInterpPxLib()
    monkeypatch.setattr(_device, "_lib", lambda: lib)
    monkeypatch.setattr(nat, "load", lambda: lib)
    monkeypatch.setattr(nat, "require_gpu", lambda: None)
    monkeypatch.setattr(nat, "current_device", lambda: 0)
    monkeypatch.setattr(nat, "current_stream", lambda: 0x55)
    monkeypatch.setattr(nat, "on_device", lambda d: contextlib.nullcontext())
    monkeypatch.setattr(_device, "PINNED", _device._PinnedPool())
    monkeypatch.setattr(_hostpipe, "PINNED", _device.PINNED)
    monkeypatch.setattr(_hostpipe, "REGISTERED", _device._Registrations())
    monkeypatch.setattr(_hostpipe, "_TLS", __import__("threading").local())
    return lib, plan


def test_the_default_makes_the_call_it_made(env):
    lib, plan = env
    for shape, dt, bpp, n in (((4, 8), np.uint8, 1, 1), ((4, 8, 4), np.uint8, 4, 1), ((2, 4, 8), np.uint16, 2, 2), ((3, 4, 8, 4), np.uint16, 8, 3), ((4, 8, 2), np.float32, 8, 1)):
        src = _device.DeviceArray(shape, dt)
        for kw in ({}, {"interpolation": "nearest"}):
            out = plan.remap_px(src, **kw)
            assert out.shape == shape and out.dtype == dt
            assert lib.calls[-1] == ("pb_remap_px", src.data_ptr(), out.data_ptr(), n, 0, 0, bpp, 0x55), (shape, kw, lib.calls[-1])
    assert {c[0] for c in lib.calls} == {"pb_remap_px"}


@pytest.mark.parametrize("shape,dt,fmt,n", [((4, 8), np.uint8, (1, 1), 1), ((4, 8, 2), np.uint8, (2, 1), 1), ((4, 8, 4), np.uint8, (4, 1), 1), ((4, 8, 3), np.uint8, (3, 1), 1),
                                           ((4, 8), np.uint16, (1, 2), 1), ((4, 8, 3), np.uint16, (3, 2), 1), ((5, 4, 8), np.uint8, (1, 1), 5), ((2, 4, 8, 4), np.uint16, (4, 2), 2),
                                           ((3, 4, 8, 1), np.uint16, (1, 2), 3)],
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else getattr(v, "__name__", str(v)))
def test_the_keyword_passes_the_format_and_the_mode(env, shape, dt, fmt, n):
    lib, plan = env
    src = _device.DeviceArray(shape, dt)
    for name, mode in (("bilinear", BIL), ("catmull-rom", CR)):
        out = plan.remap_px(src, interpolation=name)
        assert isinstance(out, _device.DeviceArray) and out.shape == shape and out.dtype == dt
        assert lib.calls[-1] == ("pb_remap_interp_px", src.data_ptr(), out.data_ptr(), n, 0, 0, fmt[0], fmt[1], mode, 0x55)
        mine = _device.DeviceArray(shape, dt)
        assert plan.remap_px(src, mine, interpolation=name) is mine and plan.remap_px(src, out=mine, interpolation=name) is mine
        assert lib.calls[-1][2] == mine.data_ptr()
    plan.launch_px_interp(FAKE, FAKE + 64, 2, 4, 2, "catmull-rom", stream=0x77, src_stride=512, dst_stride=1024)
    assert lib.calls[-1] == ("pb_remap_interp_px", FAKE, FAKE + 64, 2, 512, 1024, 4, 2, CR, 0x77)


def test_the_keyword_is_keyword_only_and_a_bad_name_or_frame_is_refused_before_any_device_work(env):
    lib, plan = env
    sig = inspect.signature(nat.Plan.remap_px)
    assert sig.parameters["interpolation"].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters["interpolation"].default == "nearest"
    assert list(sig.parameters) == ["self", "src", "out", "interpolation"]
    src = _device.DeviceArray((4, 8, 4), np.uint8)
    with pytest.raises(TypeError):
        plan.remap_px(src, None, "bilinear")
    for name in ("cubic", "", "BILINEAR", None):
        with pytest.raises(ValueError) as e:
            plan.remap_px(src, interpolation=name)
        with pytest.raises(ValueError) as e2:
            nat.check_interpolation(name)
        assert str(e.value) == str(e2.value)
    with pytest.raises(ValueError):
        plan.launch_px_interp(FAKE, FAKE, 1, 4, 1, "nearest")
    with pytest.raises(ValueError):
        plan.launch_px_interp(FAKE, FAKE, 1, 4, 1, "cubic")
    bad = [
        dict(src=np.zeros((4, 8, 4), np.uint8)),                                            # a host ndarray
        dict(src=_device.DeviceArray((4, 8), np.float32)),                                  # float samples
        dict(src=_device.DeviceArray((2, 4, 8, 2), np.int16)),
        dict(src=_device.DeviceArray((4, 8, 5), np.uint8)),                                 # five channels
        dict(src=_device.DeviceArray((4, 8, 2, 2), np.uint8)),                              # a tail of two dimensions
        dict(src=_device.DeviceArray((4, 7, 4), np.uint8)),                                 # not the plan's source
        dict(src=src, out=_device.DeviceArray((4, 8, 3), np.uint8)),                        # a wrong out: shape, dtype, kind
        dict(src=src, out=_device.DeviceArray((4, 8, 4), np.uint16)),
        dict(src=src, out=np.zeros((4, 8, 4), np.uint8)),
    ]
    for kw in bad:
        for name in ("bilinear", "catmull-rom"):
            with pytest.raises(nat.PbError):
                plan.remap_px(interpolation=name, **kw)
    # the refusal for a dtype is remap_track_px's
    with pytest.raises(nat.PbError) as e:
        plan.remap_px(_device.DeviceArray((1, 4, 8), np.float32), interpolation="bilinear")
    with pytest.raises(nat.PbError) as e2:
        plan.remap_track_px(_device.DeviceArray((1, 4, 8), np.float32), np.zeros((1, 3, 3)), interpolation="bilinear")
    assert str(e.value) == str(e2.value) == "bilinear sampling takes uint8 or uint16 frames of 1 to 4 channels, got (1, 4, 8) float32"
    assert lib.calls == [] and not lib.log, "a refused call reached the library"
    # no frames: nothing is launched
    assert plan.remap_px(_device.DeviceArray((0, 4, 8), np.uint16), interpolation="bilinear").shape == (0, 4, 8) and lib.calls == []


# ---- the tolerances, derived ------------------------------------------------------------------------------------------------------------
def test_the_two_tolerances():
    """T(R) = 1 + floor(R / 512); T_cr(R) = 1 + floor(15 R / 4096 + R 2^-18): DESIGN 3.8's budget with R in place of 255."""
    assert [pc.tolerance("bilinear", R) for R in (255, 1023, 65535)] == [1, 2, 128]
    assert [pc.tolerance("catmull-rom", R) for R in (255, 1023, 65535)] == [1, 4, 241]
    for R in (1, 255, 256, 1023, 4095, 65535):
        assert pc.tolerance("catmull-rom", R) == 1 + int(np.floor((R / 2) * (1.25 * 3 + 3 * 1.25) / 1024 + R * 2.0**-18))
    # the float32 arithmetic's bound, on the kernel's order of operations (pb_kernels_px_interp.hpp), is inside its share R 2^-18
    u = 2.0**-24
    dw = [u / 2 + u / 4 + u / 4, 2 * u + 2.5 * u / 2 + u / 2, u + u + u / 2, u / 4 + 0.5 * u / 2 + u / 16]  # the four weights, rounding by rounding
    assert dw[0] == u and dw[1] == 3.75 * u and dw[2] == 2.5 * u and dw[3] <= u and sum(dw) <= 8.25 * u
    dr = 8.25 * u + 4 * 1.25 * u                                # weights' errors on taps of at most R; four roundings of partial sums <= 1.25 R
    dv = 1.25 * dr + 8.25 * u * 1.25 + 4 * 1.25 * 1.25 * u      # row sums' errors; weights' errors on row sums <= 1.25 R; four roundings <= 1.5625 R
    assert dr == 13.25 * u and dv == 33.125 * u and dv < 2.0**-18 and dv * 65535 < 0.25 and dv * 255 < 255 * 2.0**-18


def _fma32(a, b, c):
    """float32 fused multiply-add on arrays: the product of two float32 is exact in float64, the sum is rounded to 53 bits and then to 24 -
    a double rounding, which can exceed the single one by 2^-29 of an ulp at most: nothing beside the bound checked below."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def _weights32(t):
    """pb_pxi_weights, operation by operation"""
    f = np.float32
    t2 = (t * t).astype(f)
    return [(_fma32(_fma32(np.full_like(t, -0.5), t, np.full_like(t, 1.0)), t, np.full_like(t, -0.5)) * t).astype(f),
            _fma32(_fma32(np.full_like(t, 1.5), t, np.full_like(t, -2.5)), t2, np.full_like(t, 1.0)),
            (_fma32(_fma32(np.full_like(t, -1.5), t, np.full_like(t, 2.0)), t, np.full_like(t, 0.5)) * t).astype(f),
            (_fma32(np.full_like(t, 0.5), t, np.full_like(t, -0.5)) * t2).astype(f)]


def test_the_kernel_s_float32_order_of_operations_stays_inside_its_share_of_the_budget():
    """pb_pxi_px's Catmull-Rom arithmetic emulated in float32 on the CPU - the weights' Horner steps, a row sum as one product and three fused
    multiply-adds, the column sum the same way - against the definition's float64 expression on the same fractions and taps: random taps, and
    the taps that put R wherever a weight is positive (the largest sums).  The unrounded values differ by less than the derived 33.125 u R."""
    from tests import catmull_rom_ref as crr

    rng = np.random.default_rng(2310)
    n, R, u = 200000, 65535, 2.0**-24
    worst = 0.0
    for kind in ("random", "table", "signed"):
        tx = rng.random(n).astype(np.float32) if kind != "table" else (rng.integers(0, 4096, n) / 4096.0).astype(np.float32)
        ty = rng.random(n).astype(np.float32) if kind != "table" else (rng.integers(0, 4096, n) / 4096.0).astype(np.float32)
        wx, wy = _weights32(tx), _weights32(ty)
        wx64, wy64 = crr.weights(tx.astype(np.float64)), crr.weights(ty.astype(np.float64))
        for k, (a, b) in enumerate(zip(wx + wy, list(wx64) + list(wy64))):
            assert np.abs(a.astype(np.float64) - b).max() <= (u, 3.75 * u, 2.5 * u, u)[k % 4], (kind, k)
        if kind == "signed":  # R where the product of the two weights is positive, 0 elsewhere: the largest value the footprint can give
            taps = np.stack([np.stack([np.where(wy64[k] * wx64[l] > 0, R, 0) for l in range(4)]) for k in range(4)]).astype(np.float32)
        else:
            taps = rng.integers(0, R + 1, (4, 4, n)).astype(np.float32)
        acc, v64 = None, None
        for k in range(4):
            s = (wx[0] * taps[k, 0]).astype(np.float32)
            s64 = wx64[0] * taps[k, 0].astype(np.float64)
            for l in range(1, 4):
                s = _fma32(wx[l], taps[k, l], s)
                s64 = s64 + wx64[l] * taps[k, l].astype(np.float64)
            acc = (wy[0] * s).astype(np.float32) if k == 0 else _fma32(wy[k], s, acc)
            v64 = wy64[0] * s64 if k == 0 else v64 + wy64[k] * s64
        err = float(np.abs(acc.astype(np.float64) - v64).max())
        print(f"{kind}: largest float32 - float64 difference {err:.5f} LSB at R = {R} ({err / (u * R):.2f} u R; bound 33.125 u R = {33.125 * u * R:.3f}, budget {R * 2.0**-18:.3f})")
        worst = max(worst, err)
    assert worst <= 33.125 * u * R < R * 2.0**-18


# ---- the excuse rule cannot hide a failure ----------------------------------------------------------------------------------------------
def test_the_gpu_cases_are_the_issue_s():
    names = [c.name for c in pc.CASES]
    assert names == [c.name for c in ic.SWEEP + ic.TINY + ic.MAGNIFIED + [ic.ODD_DST] if c.name != "tiny_double_2x4"] and len(names) == 40
    assert all(c.src[0] in ("camera", "pano") for c in pc.CASES)
    assert set(pc.ALL_FORMAT_CASES) <= set(names) and len(pc.ALL_FORMAT_CASES) == 7
    assert pc.FORMATS == [(1, 1), (2, 1), (4, 1), (1, 2), (2, 2), (3, 2), (4, 2)]


@pytest.mark.parametrize("case", [c for c in pc.CASES if not c.name.startswith("sweep")], ids=lambda c: c.name)
def test_the_edge_band_of_a_fixed_case_is_capped(case):
    final = ic.final_map(case)
    band = ic.edge_band(case, final, pc.BAND)
    n = int(band.sum())
    print(f"{case.name}: {n} of {band.size} pixels within 1/512 px of the source frame's edge")
    if case.src[0] == "pano":
        assert n == 0
    if case.name == "tiny_cam_1x6":  # the only one-row source: every row of the output runs along the frame's two long edges
        assert (n, band.size) == (32, 512) == (pc.PINNED_BANDS[case.name], band.size)
    else:
        assert case.name not in pc.PINNED_BANDS and n * 200 <= band.size, f"{n} of {band.size} pixels lie in the edge band"
    if case.name == "tiny_cam_2x2":
        assert (n, band.size) == (24, 8192)
    if case.name == "mag_pano_from_cam":
        assert (n, band.size) == (23, 294912)


def test_the_sweep_s_edge_bands_are_capped_by_the_existing_test():
    """tests/test_interp_cases_host.py holds every sweep case to 1 / 10 000 of its pixels (and shares the computation with this module)."""
    from tests.test_interp_cases_host import BAND, _definition

    assert BAND == pc.BAND
    for k, case in enumerate(ic.SWEEP):
        _, in_band, n = _definition(k)
        assert in_band * 10000 <= n and in_band * 200 <= n, (case.name, in_band, n)


def test_the_route_diagnostic_says_nothing_is_launched_for_a_deferred_plan(deferred, deferred_double):
    """pb_plan_px_interp_route: 0 where the call is refused, 3 for three uint8 channels (the RGB8 call's), the call's own argument errors;
    the tile kernel (1) and the float64 chain (2) need a prepared plan: tests/test_hip_px_interp.py."""
    vp, C = ctypes.c_void_p, ctypes
    assert nat.SIGNATURES["pb_plan_px_interp_route"] == (C.c_int, [vp, C.c_int, C.c_int, C.c_int])
    for lib, h in (deferred, deferred_double):
        for ch, sb in FORMATS:
            for mode in (BIL, CR):
                assert lib.pb_plan_px_interp_route(h, ch, sb, mode) == (3 if (ch, sb) == (3, 1) else 0), (ch, sb, mode)
        assert lib.pb_plan_px_interp_route(h, 5, 1, BIL) == INVALID and lib.pb_plan_px_interp_route(h, 4, 1, 0) == INVALID
        assert lib.pb_plan_px_interp_route(None, 4, 1, BIL) == INVALID
    plan = nat.Plan(nat.make_proj(nat.KIND_PANO, 4, 8), [], nat.make_proj(nat.KIND_PANO, 4, 8), defer=True)
    assert plan.px_interp_route(4, 1, "bilinear") == "none" and plan.px_interp_route(3, 1, "catmull-rom") == "rgb8"
