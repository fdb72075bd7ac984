"""CPU-only checks of pb_remap_interp_pxf / pb_remap_interp_pxf_supported: the definition tests/pxf_ref.py against the integer
definitions it continues, the symbols and their signatures, the argument checks in contract order - a deferred plan has no device and every
call here is refused before anything could be launched -, Plan.remap_float / launch_float / float_supported against a stand-in for the
library, the kernel's float32 order of operations inside its share of the tolerance, and the conditions that keep the GPU test's NaN
containment masks (tests/test_hip_pxf_interp.py) from being trivial."""

import contextlib
import ctypes
import functools
import os
import re

import numpy as np
import pytest

from oracle import reference_path as orc
from photonbend_amd import _device, _hostpipe
from photonbend_amd import _native as nat
from tests import catmull_rom_ref as crr
from tests import interp_cases as ic
from tests import px_interp_cases as pc
from tests import pxf_cases as fc
from tests import pxf_ref
from tests.test_px_interp_host import FakeInterpPxLib, _fma32, _weights32

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x1000  # a non-null, 16-byte aligned "device pointer" for calls that must be refused before anything reads it
OK, INVALID, UNSUPPORTED = 0, -1, -3
BIL, CR = 1, 2  # PB_INTERP_BILINEAR, PB_INTERP_CATMULL_ROM
NAME = b"pb_remap_interp_pxf"


# ---- the definition ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _final(name):
    final = ic.final_map(ic.by_name(name))
    final.setflags(write=False)
    return final


def test_the_cases_and_formats_are_the_issue_s():
    assert [c.name for c in fc.CASES] == [c.name for c in pc.CASES if c.name != "tiny_pano_1x2"] and len(fc.CASES) == 39
    assert fc.ALL_FORMAT_CASES == pc.ALL_FORMAT_CASES and set(fc.ALL_FORMAT_CASES) <= {c.name for c in fc.CASES}
    assert fc.FORMATS == [(1, 2), (2, 2), (3, 2), (4, 2), (1, 4), (2, 4), (3, 4), (4, 4)]
    assert fc.BAND == 1.0 / 512.0
    for S in (2, 4):
        for k, (_, L, U) in enumerate(fc.DRAWS[S]):
            a, (lo, hi) = fc.draw(9, 11, 3, S, k, 5)
            assert a.dtype == fc.DTYPE[S] and a.shape == (9, 11, 3) and (lo, hi) == (L, U) and lo <= float(a.min()) and float(a.max()) <= hi
            assert fc.draw(9, 11, 1, S, k, 5)[0].shape == (9, 11)
    assert fc.DRAWS[4][1][1:] == (-1000.0, 1000.0) and fc.DRAWS[2][1][1:] == (-64.0, 64.0)


@pytest.mark.parametrize("case", fc.CASES, ids=lambda c: c.name)
def test_the_definition_on_a_frame_of_integers_is_the_integer_definition_byte_for_byte(case):
    """rint(clip(remap_f64, 0, 255)) on a float frame holding integers of [0, 255] is orc.remap_bilinear / catmull_rom_ref.remap on the uint8
    frame: both filters, one and four channels, float32 and float16 frames (every integer of [0, 255] is exact in both)."""
    _, h, w, *_ = case.src
    src = ic.src_proj(case)
    image = np.random.default_rng(77).integers(0, 256, size=(h, w, 4), dtype=np.uint8)
    for filt, integer in (("bilinear", orc.remap_bilinear), ("catmull-rom", crr.remap)):
        for u8, dt in ((image, np.float32), (np.ascontiguousarray(image[:, :, 2]), np.float16)):
            with np.errstate(all="ignore"):
                want = integer(None, src, u8, cmap=np.copy(_final(case.name)))
            v = pxf_ref.remap_f64(src, u8.astype(dt), filt, np.copy(_final(case.name)))
            got = np.clip(np.rint(v), 0, 255).astype(np.uint8)
            assert np.array_equal(got.reshape(want.shape), want), (case.name, filt, dt)
            narrowed = pxf_ref.remap(src, u8.astype(dt), filt, np.copy(_final(case.name)))
            assert narrowed.dtype == dt and narrowed.shape == want.shape
            with np.errstate(all="ignore"):
                assert np.array_equal(narrowed, v.astype(dt).reshape(want.shape))
            assert not np.signbit(narrowed[want == 0]).any() or filt == "catmull-rom"  # (a dead pixel is +0.0; the cubic may give -0.0 ... only where live)


def test_a_dead_pixel_is_plus_zero_and_the_cubic_s_overshoot_is_kept():
    case = ic.by_name("mag_pano_from_cam")
    src = ic.src_proj(case)
    _, h, w, *_ = case.src
    final = _final(case.name)
    _, _, live = pxf_ref.positions(src, np.copy(final))
    assert live.any() and not live.all()
    step = np.zeros((h, w), np.float32)
    step[:, w // 2:] = 1000.0
    for filt in pxf_ref.FILTERS:
        out = pxf_ref.remap(src, step, filt, np.copy(final))
        assert not out[~live].view(np.uint32).any()  # all bytes zero
        if filt == "catmull-rom":
            assert out.min() < -1.0 and out.max() > 1001.0  # neither clipped nor rounded
        else:
            assert out.min() == 0.0 and out.max() == 1000.0 and (out != np.rint(out)).any()
    big = np.full((h, w), 60000.0, np.float16)
    big[:, ::2] = -60000.0
    with np.errstate(all="ignore"):
        assert np.isinf(pxf_ref.remap(src, big, "catmull-rom", np.copy(final))).any()  # float16 overflow is IEEE's


# ---- the symbols ------------------------------------------------------------------------------------------------------------------------
def test_the_two_symbols_exist_with_the_declared_signatures_and_the_abi_is_still_5():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "photonbend_hip.h")).read(), flags=re.S)
    decl = {m.group(1): " ".join(m.group(2).split()) for m in re.finditer(r"\bint\s+(?:[A-Z_]+\s+)?(pb_remap_interp_pxf\w*)\s*\(([^)]*)\)\s*;", text)}
    assert decl == {
        "pb_remap_interp_pxf": "const pb_plan* plan, const void* src_dev, void* dst_dev, int n_frames, size_t src_frame_stride, size_t dst_frame_stride, "
                               "int channels, int sample_bytes, int interpolation, void* stream",
        "pb_remap_interp_pxf_supported": "const pb_plan* plan, int channels, int sample_bytes, int interpolation",
    }
    assert re.search(r"#define PB_ABI_VERSION 5\b", text)
    vp, C = ctypes.c_void_p, ctypes
    assert nat.SIGNATURES["pb_remap_interp_pxf"] == (C.c_int, [vp, vp, vp, C.c_int, C.c_size_t, C.c_size_t, C.c_int, C.c_int, C.c_int, vp])
    assert nat.SIGNATURES["pb_remap_interp_pxf_supported"] == (C.c_int, [vp, C.c_int, C.c_int, C.c_int])
    lib = nat.load()
    assert hasattr(lib, "pb_remap_interp_pxf") and hasattr(lib, "pb_remap_interp_pxf_supported") and lib.pb_abi_version() == 5 == nat.ABI_VERSION


# ---- the C call's argument checks, in contract order ------------------------------------------------------------------------------------
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


def pxf(lib, h, src=FAKE, dst=FAKE, n=1, ss=0, ds=0, ch=4, sb=2, mode=BIL):
    return lib.pb_remap_interp_pxf(h, src, dst, n, ss, ds, ch, sb, mode, None), lib.pb_last_error()


def test_the_frame_checks_come_first_with_pb_remap_px_s_messages_and_12_and_16_as_pixel_sizes(deferred):
    lib, h = deferred
    for ch, sb in fc.FORMATS:
        B = ch * sb
        a = min(4, B & -B)
        assert a == (4 if B in (12, 16) else nat.px_align(B))
        for args in ((h, None, None, 1), (h, None, FAKE, 1), (h, FAKE, None, 3), (h, None, None, 0), (None, FAKE, FAKE, 1)):
            for mode in (BIL, CR, 0, 9):  # (the frame arguments come before the interpolation)
                assert (lib.pb_remap_interp_pxf(*args, 0, 0, ch, sb, mode, None), lib.pb_last_error()) == (INVALID, b"null argument"), (ch, sb, args, mode)
        for mode in (BIL, CR, 0, 9):
            assert (lib.pb_remap_interp_pxf(h, FAKE, FAKE, -1, 0, 0, ch, sb, mode, None), lib.pb_last_error()) == (INVALID, b"negative frame count")
        frame = 4 * 8 * B
        for s, d, n, ss, ds in ((FAKE, FAKE, 1, 0, frame - a), (FAKE, FAKE, 2, frame - a, 0)):
            rc, msg = pxf(lib, h, src=s, dst=d, n=n, ss=ss, ds=ds, ch=ch, sb=sb, mode=0)
            assert rc == INVALID and b"smaller than a frame" in msg, (ch, sb, msg)
        for s, d, n, ss, ds in ((FAKE + a // 2, FAKE, 1, 0, 0), (FAKE, FAKE + a // 2, 1, 0, 0), (FAKE, FAKE, 1, frame + a // 2, 0), (FAKE, FAKE, 1, 0, frame + a // 2),
                                (FAKE, FAKE, 2, frame + a + 1, frame + a)):
            rc, msg = pxf(lib, h, src=s, dst=d, n=n, ss=ss, ds=ds, ch=ch, sb=sb, mode=7)
            assert (rc, msg) == (INVALID, f"frame pointers and strides must be multiples of {a} bytes for {B}-byte pixels".encode()), (ch, sb, msg)
        # aligned to A and no further: the frame checks pass, and the deferred plan is what is refused
        rc, msg = pxf(lib, h, src=FAKE + a, dst=FAKE + 3 * a, n=2, ss=frame + a, ds=frame + 3 * a, ch=ch, sb=sb)
        assert rc == UNSUPPORTED and msg.startswith(NAME + b" "), (ch, sb, msg)
    # the other calls keep their answers: 12 and 16 are no pixel sizes of pb_remap_px, 4 is no sample size of pb_remap_interp_px
    for B in (12, 16):
        assert lib.pb_remap_px_supported(h, B) == INVALID and lib.pb_last_error() == b"bytes_per_px outside {1, 2, 3, 4, 6, 8}"
        assert (lib.pb_remap_px(h, FAKE, FAKE, 1, 0, 0, B, None), lib.pb_last_error()) == (INVALID, b"bytes_per_px outside {1, 2, 3, 4, 6, 8}")
    for mode in (BIL, CR):
        assert lib.pb_remap_interp_px_supported(h, 1, 4, mode) == INVALID and lib.pb_remap_interp_px_supported(h, 3, 4, mode) == INVALID
        assert lib.pb_remap_interp_px(h, FAKE, FAKE, 1, 0, 0, 4, 4, mode, None) == INVALID


def test_the_later_checks_follow_in_their_order(deferred):
    lib, h = deferred
    # a format outside the sets is checked at the weakest alignment: odd pointers and strides pass the frame checks and meet the next one
    assert pxf(lib, h, src=FAKE + 1, dst=FAKE + 3, ch=5, sb=2, mode=7) == (INVALID, b"interpolation must be PB_INTERP_BILINEAR or PB_INTERP_CATMULL_ROM")
    for mode in (-1, 3, 7, 100):
        for ch, sb in fc.FORMATS + [(0, 2), (5, 4), (1, 1), (1, 8)]:  # the interpolation comes before the format
            assert pxf(lib, h, ch=ch, sb=sb, mode=mode) == (INVALID, b"interpolation must be PB_INTERP_BILINEAR or PB_INTERP_CATMULL_ROM"), (mode, ch, sb)
            assert lib.pb_remap_interp_pxf_supported(h, ch, sb, mode) == INVALID
    for ch, sb in fc.FORMATS + [(0, 2)]:  # PB_INTERP_NEAREST is another call's: the message names it
        for n in (0, 1):
            rc, msg = pxf(lib, h, ch=ch, sb=sb, mode=0, n=n)
            assert rc == INVALID and msg.startswith(NAME + b" ") and b"PB_INTERP_NEAREST" in msg and b"pb_remap_px" in msg, (ch, sb, msg)
        assert lib.pb_remap_interp_pxf_supported(h, ch, sb, 0) == INVALID and b"pb_remap_px" in lib.pb_last_error()
    # the format comes before the plan and before "no frames": INVALID on a deferred plan, which a valid format finds UNSUPPORTED
    for ch, sb in ((0, 2), (5, 2), (0, 4), (5, 4), (1, 0), (1, 1), (4, 1), (1, 3), (4, 8), (-1, 2), (2, 6)):
        for mode in (BIL, CR):
            for n in (0, 1):
                rc, msg = pxf(lib, h, ch=ch, sb=sb, mode=mode, n=n)
                assert rc == INVALID and b"channels" in msg and b"sample_bytes" in msg, (ch, sb, n, msg)
            assert lib.pb_remap_interp_pxf_supported(h, ch, sb, mode) == INVALID, (ch, sb)
    assert lib.pb_remap_interp_pxf_supported(None, 4, 2, BIL) == INVALID and lib.pb_last_error() == b"null argument"


def test_no_frames_is_ok_and_deferred_and_double_fisheye_plans_are_unsupported(deferred, deferred_double):
    for lib, h in (deferred, deferred_double):
        for ch, sb in fc.FORMATS:
            for mode in (BIL, CR):
                assert lib.pb_remap_interp_pxf(h, FAKE, FAKE, 0, 0, 0, ch, sb, mode, None) == OK, (ch, sb, mode)
                assert lib.pb_remap_interp_pxf(h, None, None, 0, 0, 0, ch, sb, mode, None) == INVALID  # (pb_remap_px's rule: no null frames)
                assert lib.pb_remap_interp_pxf_supported(h, ch, sb, mode) == 0, (ch, sb, mode)
                rc, msg = pxf(lib, h, ch=ch, sb=sb, mode=mode)
                assert rc == UNSUPPORTED and msg.startswith(NAME + b" takes prepared plans") and b"pb_plan_prepare" not in msg, (ch, sb, mode, msg)
    plan = nat.Plan(nat.make_proj(nat.KIND_PANO, 4, 8), [], nat.make_proj(nat.KIND_PANO, 4, 8), defer=True)
    assert not plan.float_supported(4, 2, "bilinear") and not plan.float_supported(3, 4, "catmull-rom")
    with pytest.raises(nat.PbError):
        plan.float_supported(5, 2, "bilinear")
    with pytest.raises(nat.PbError):
        plan.float_supported(1, 1, "bilinear")
    for name in ("nearest", "cubic"):
        with pytest.raises(ValueError):
            plan.float_supported(4, 2, name)


# ---- Plan.remap_float against a stand-in ------------------------------------------------------------------------------------------------
class FakeFloatLib(FakeInterpPxLib):
    """tests/test_px_interp_host.py's stand-in with the float launch: it records its arguments."""

    def pb_remap_interp_pxf(self, plan, src, dst, n, ss, ds, channels, sample_bytes, interpolation, stream):
        self.calls.append(("pb_remap_interp_pxf", int(src), int(dst), int(n), int(ss), int(ds), int(channels), int(sample_bytes), int(interpolation), int(stream or 0)))
        return 0


@pytest.fixture
def env(monkeypatch):
    p = nat.make_proj(nat.KIND_PANO, 4, 8)
    plan = nat.Plan(p, [], p, defer=True)
    lib = FakeFloatLib()
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


@pytest.mark.parametrize("shape,dt,fmt,n", [((4, 8), np.float16, (1, 2), 1), ((4, 8, 2), np.float16, (2, 2), 1), ((4, 8, 3), np.float32, (3, 4), 1), ((4, 8, 4), np.float32, (4, 4), 1),
                                           ((4, 8), np.float32, (1, 4), 1), ((5, 4, 8), np.float16, (1, 2), 5), ((2, 4, 8, 4), np.float16, (4, 2), 2),
                                           ((3, 4, 8, 1), np.float32, (1, 4), 3), ((2, 4, 8, 3), np.float16, (3, 2), 2)],
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else getattr(v, "__name__", str(v)))
def test_the_four_shapes_and_both_dtypes_reach_the_call_with_their_format(env, shape, dt, fmt, n):
    lib, plan = env
    src = _device.DeviceArray(shape, dt)
    for kw, mode in (({}, BIL), ({"interpolation": "bilinear"}, BIL), ({"interpolation": "catmull-rom"}, CR)):
        out = plan.remap_float(src, **kw)
        assert isinstance(out, _device.DeviceArray) and out.shape == shape and out.dtype == dt
        assert lib.calls[-1] == ("pb_remap_interp_pxf", src.data_ptr(), out.data_ptr(), n, 0, 0, fmt[0], fmt[1], mode, 0x55)
        mine = _device.DeviceArray(shape, dt)
        assert plan.remap_float(src, mine, **kw) is mine and plan.remap_float(src, out=mine, **kw) is mine
        assert lib.calls[-1][2] == mine.data_ptr()
    plan.launch_float(FAKE, FAKE + 64, 2, 3, 4, "catmull-rom", stream=0x77, src_stride=512, dst_stride=1024)
    assert lib.calls[-1] == ("pb_remap_interp_pxf", FAKE, FAKE + 64, 2, 512, 1024, 3, 4, CR, 0x77)
    assert {c[0] for c in lib.calls} == {"pb_remap_interp_pxf"}


def test_a_bad_name_or_frame_is_refused_before_any_device_work(env, monkeypatch):
    lib, plan = env
    src = _device.DeviceArray((4, 8, 4), np.float32)
    with pytest.raises(ValueError) as e:
        plan.remap_float(src, interpolation="nearest")
    assert "remap_px" in str(e.value)
    for name in ("cubic", "", "BILINEAR", None):
        with pytest.raises(ValueError):
            plan.remap_float(src, interpolation=name)
    for name in ("nearest", "cubic"):
        with pytest.raises(ValueError):
            plan.launch_float(FAKE, FAKE, 1, 4, 2, name)
    with pytest.raises(TypeError):
        plan.remap_float(src, None, "bilinear")  # (keyword-only, as remap_px's)
    bad = [dict(src=np.zeros((4, 8, 4), np.float32))]                                          # a host ndarray
    bad += [dict(src=_device.DeviceArray((4, 8, 2), dt)) for dt in (np.uint8, np.uint16, np.int16, np.int32, np.float64)]  # other dtypes
    bad += [
        dict(src=_device.DeviceArray((4, 8, 5), np.float16)),                                  # five channels
        dict(src=_device.DeviceArray((4, 8, 2, 2), np.float16)),                               # a tail of two dimensions
        dict(src=_device.DeviceArray((4, 7, 4), np.float32)),                                  # not the plan's source
        dict(src=src, out=_device.DeviceArray((4, 8, 3), np.float32)),                         # a wrong out: shape, dtype, kind
        dict(src=src, out=_device.DeviceArray((4, 8, 4), np.float16)),
        dict(src=src, out=np.zeros((4, 8, 4), np.float32)),
    ]
    for kw in bad:
        for name in ("bilinear", "catmull-rom"):
            with pytest.raises(nat.PbError):
                plan.remap_float(interpolation=name, **kw)
    for dt in (np.uint8, np.float64):
        with pytest.raises(nat.PbError) as e:
            plan.remap_float(_device.DeviceArray((4, 8), dt))
        assert "float16 or float32" in str(e.value)
    # bfloat16, which NumPy has no dtype for: a tensor the method takes for a device array (there is no GPU here to put one on)
    torch = pytest.importorskip("torch")
    with monkeypatch.context() as m:
        m.setattr(nat, "is_device_array", lambda x: True)
        with pytest.raises(nat.PbError) as e:
            plan.remap_float(torch.zeros((4, 8), dtype=torch.bfloat16))
        assert "float16 or float32" in str(e.value) and "bfloat16" in str(e.value)
    assert lib.calls == [] and not lib.log, "a refused call reached the library"
    # no frames: nothing is launched
    assert plan.remap_float(_device.DeviceArray((0, 4, 8), np.float16)).shape == (0, 4, 8) and lib.calls == []
    # remap_px keeps its refusal of float frames with an interpolating mode, and its message
    with pytest.raises(nat.PbError) as e:
        plan.remap_px(_device.DeviceArray((1, 4, 8), np.float32), interpolation="bilinear")
    assert str(e.value) == "bilinear sampling takes uint8 or uint16 frames of 1 to 4 channels, got (1, 4, 8) float32" and lib.calls == []


# ---- the tolerance and the kernel's float32 order of operations -------------------------------------------------------------------------
def test_the_two_tolerances():
    u = 2.0**-24
    for S, uo in ((2, 2.0**-11), (4, u)):
        for L, U in ((0.25, 1.0), (-1000.0, 1000.0), (-64.0, 64.0), (2.0**-8, 4096.0)):
            D, M = U - L, max(abs(L), abs(U))
            assert fc.tolerance("bilinear", L, U, S) == D / 512 + M * 2.0**-20 + M * uo
            assert fc.tolerance("catmull-rom", L, U, S) == 15 * D / 4096 + M * 2.0**-18 + 1.5625 * M * uo
            assert (D / 2) * (1.25 * 3 + 3 * 1.25) / 1024 == 15 * D / 4096  # DESIGN 3.8's coordinate budget with D for R
    # the arithmetic's shares, as the kernel header derives them
    assert 4 * u * 2 + 4 * u <= 12 * u < 16 * u == 2.0**-20 and 33.125 * u < 64 * u == 2.0**-18


def test_the_kernel_s_float32_order_of_operations_stays_inside_its_share_of_the_budget():
    """pb_pxf_px's arithmetic emulated in float32 on the CPU, operation by operation - bilinear: b - a, fmaf(tx, b - a, a), bot likewise,
    bot - top, fmaf(ty, bot - top, top); Catmull-Rom: pb_pxi_weights' Horner steps, a row sum as one product and three fused multiply-adds,
    the column sum the same way - against the definition's float64 expression on the same fractions and taps.  Taps: random in [L, U] for
    every draw's range, and the extremes - L and U alternating (bilinear), U wherever the product of the two weights is positive and L
    elsewhere (the largest sums).  The unrounded values differ by less than the derived 4 u D + 4 u M and 33.125 u M."""
    rng = np.random.default_rng(2410)
    n, u = 100000, 2.0**-24
    f32 = np.float32
    for L, U in ((0.25, 1.0), (-1000.0, 1000.0), (-64.0, 64.0), (2.0**-8, 4096.0)):
        D, M = U - L, max(abs(L), abs(U))
        for kind in ("random", "table", "extreme"):
            tx = rng.random(n).astype(f32) if kind != "table" else (rng.integers(0, 4096, n) / 4096.0).astype(f32)
            ty = rng.random(n).astype(f32) if kind != "table" else (rng.integers(0, 4096, n) / 4096.0).astype(f32)
            # bilinear
            taps = rng.uniform(L, U, (4, n)).astype(f32) if kind != "extreme" else np.where(rng.integers(0, 2, (4, n)) == 1, f32(U), f32(L))
            taps = np.clip(taps, f32(L), f32(U))
            a, b, c, d = taps
            top = _fma32(tx, (b - a).astype(f32), a)
            bot = _fma32(tx, (d - c).astype(f32), c)
            g = _fma32(ty, (bot - top).astype(f32), top)
            a64, b64, c64, d64 = taps.astype(np.float64)
            t64 = a64 + tx.astype(np.float64) * (b64 - a64)
            b64_ = c64 + tx.astype(np.float64) * (d64 - c64)
            v64 = t64 + ty.astype(np.float64) * (b64_ - t64)
            err = float(np.abs(g.astype(np.float64) - v64).max())
            print(f"bilinear [{L}, {U}] {kind}: float32 - float64 {err:.3e} ({err / (u * M):.2f} u M; bound {4 * u * D + 4 * u * M:.3e}, share {M * 2.0**-20:.3e})")
            assert err <= 4 * u * D + 4 * u * M <= 12 * u * M < M * 2.0**-20
            # Catmull-Rom
            wx, wy = _weights32(tx), _weights32(ty)
            wx64, wy64 = crr.weights(tx.astype(np.float64)), crr.weights(ty.astype(np.float64))
            if kind == "extreme":
                taps = np.stack([np.stack([np.where(wy64[k] * wx64[l] > 0, U, L) for l in range(4)]) for k in range(4)]).astype(f32)
            else:
                taps = np.clip(rng.uniform(L, U, (4, 4, n)).astype(f32), f32(L), f32(U))
            acc, v64 = None, None
            for k in range(4):
                s = (wx[0] * taps[k, 0]).astype(f32)
                s64 = wx64[0] * taps[k, 0].astype(np.float64)
                for l in range(1, 4):
                    s = _fma32(wx[l], taps[k, l], s)
                    s64 = s64 + wx64[l] * taps[k, l].astype(np.float64)
                acc = (wy[0] * s).astype(f32) if k == 0 else _fma32(wy[k], s, acc)
                v64 = wy64[0] * s64 if k == 0 else v64 + wy64[k] * s64
            err = float(np.abs(acc.astype(np.float64) - v64).max())
            print(f"catmull-rom [{L}, {U}] {kind}: float32 - float64 {err:.3e} ({err / (u * M):.2f} u M; bound 33.125 u M = {33.125 * u * M:.3e}, share {M * 2.0**-18:.3e})")
            assert err <= 33.125 * u * M < M * 2.0**-18
            assert float(np.abs(v64).max()) <= 1.5625 * M  # what the narrowing's share assumes


# ---- the NaN containment masks are not trivial ------------------------------------------------------------------------------------------
def test_the_nan_containment_masks_are_non_trivial():
    """The GPU test sets one source texel to NaN and holds every pixel OUTSIDE pxf_cases.poison_mask to the clean run's bits: a mask that
    covered the frame would check nothing, an empty one would say the texel is not in view."""
    case = ic.by_name(fc.POISON_PANO)
    mask = fc.poison_mask(ic.src_proj(case), _final(case.name), fc.POISON_TEXEL)
    n = int(mask.sum())
    print(f"{case.name} texel {fc.POISON_TEXEL}: {n} of {mask.size} pixels within 3 texels")
    assert mask.size == 131072 and 0 < n <= mask.size // 10
    assert n == 7637
    case = ic.by_name(fc.POISON_CAM)
    src, final = ic.src_proj(case), _final(case.name)
    texel = fc.centre_texel(src, final)
    mask = fc.poison_mask(src, final, texel)
    n = int(mask.sum())
    print(f"{case.name} texel {texel}: {n} of {mask.size} pixels within 3 texels")
    assert 0 < n <= mask.size // 10 and 3 <= texel[0] < case.src[1] - 3 and 3 <= texel[1] < case.src[2] - 3
    # the definition agrees: a NaN there changes pixels inside the mask, and only there
    _, h, w, *_ = case.src
    clean, _ = fc.draw(h, w, 1, 4, 0, 3)
    dirty = clean.copy()
    dirty[texel] = np.nan
    for filt in pxf_ref.FILTERS:
        a, b = pxf_ref.remap(src, clean, filt, np.copy(final)), pxf_ref.remap(src, dirty, filt, np.copy(final))
        changed = a.view(np.uint32) != b.view(np.uint32)
        assert changed.any() and not (changed & ~mask).any(), filt
