"""CPU-only checks of pb_remap_track_px / pb_remap_track_px_supported: the symbols and their signatures, pb_remap_px's frame
checks and pb_remap_track_u8's table checks in their order - a deferred plan has no device and every call here is refused before anything
could be launched -, Plan.remap_track_px against a stand-in for the library (tests/test_host_memory.py's), and the definition itself on the
CPU: the golden index maps of tests/golden/rotation_track.npz gather grey16 and RGBA8 frames to the oracle's bytes."""

import contextlib
import ctypes
import os
import re

import numpy as np
import pytest

from oracle import reference_path as orc
from photonbend_amd import _device, _hostpipe, batch
from photonbend_amd import _native as nat
from photonbend_amd.core import rotation_track
from tests import helpers as H
from tests import rotation_track_cases as rc
from tests.test_host_memory import FakePipeLib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x1000  # a non-null, 8-byte aligned "device pointer" for calls that must be refused before anything reads it
OK, INVALID, UNSUPPORTED = 0, -1, -3
FORMATS = [(1, 1), (2, 1), (3, 1), (4, 1), (1, 2), (2, 2), (3, 2), (4, 2)]  # (channels, sample_bytes)


def _plan(kind=nat.KIND_PANO, n_rot=0, fov=None):
    lib = nat.load()
    h = ctypes.c_void_p()
    p = nat.make_proj(nat.KIND_PANO, 4, 8)
    s = nat.make_proj(kind, 4, 8) if fov is None else nat.make_proj(kind, 4, 8, lens=0, fov=fov, f_distance=2.0)
    rots = (ctypes.c_double * (9 * max(1, n_rot)))(*([1, 0, 0, 0, 1, 0, 0, 0, 1] * max(1, n_rot)))
    assert lib.pb_plan_create_ex(ctypes.byref(p), rots if n_rot else None, n_rot, ctypes.byref(s), nat.PLAN_DEFER, 0, ctypes.byref(h)) == 0, lib.pb_last_error()
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


def track(lib, h, table=FAKE, k=1, interp=0, src=FAKE, dst=FAKE, n=1, ss=0, ds=0, ch=4, sb=1):
    return lib.pb_remap_track_px(h, table, k, interp, src, dst, n, ss, ds, ch, sb, None), lib.pb_last_error()


def test_the_two_symbols_exist_with_the_declared_signatures_and_the_abi_is_still_5():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "photonbend_hip.h")).read(), flags=re.S)
    decl = {m.group(1): " ".join(m.group(2).split()) for m in re.finditer(r"\bint (pb_remap_track_px\w*)\s*\(([^)]*)\)\s*;", text)}
    assert decl == {
        "pb_remap_track_px": "const pb_plan* plan, const double* rot3x3_dev, int n_rot_per_frame, int interpolation, const void* src_dev, void* dst_dev, "
                             "int n_frames, size_t src_frame_stride, size_t dst_frame_stride, int channels, int sample_bytes, void* stream",
        "pb_remap_track_px_supported": "const pb_plan* plan, int channels, int sample_bytes",
    }
    assert re.search(r"#define PB_ABI_VERSION 5\b", text)
    vp, C = ctypes.c_void_p, ctypes
    assert nat.SIGNATURES["pb_remap_track_px"] == (C.c_int, [vp, vp, C.c_int, C.c_int, vp, vp, C.c_int, C.c_size_t, C.c_size_t, C.c_int, C.c_int, vp])
    assert nat.SIGNATURES["pb_remap_track_px_supported"] == (C.c_int, [vp, C.c_int, C.c_int])
    lib = nat.load()
    assert hasattr(lib, "pb_remap_track_px") and hasattr(lib, "pb_remap_track_px_supported") and lib.pb_abi_version() == 5 == nat.ABI_VERSION


def test_every_frame_argument_refusal_of_pb_remap_px_comes_back_with_its_status_and_message(deferred):
    lib, h = deferred
    for ch, sb in FORMATS:
        B = ch * sb
        for args in ((h, None, None, 1), (h, None, FAKE, 1), (h, FAKE, None, 3), (h, None, None, 0), (h, None, None, -1), (None, None, None, -1),
                     (None, FAKE, FAKE, 1), (h, FAKE, FAKE, -1), (h, FAKE, FAKE, -7)):
            want = lib.pb_remap_px(*args, 0, 0, B, None), lib.pb_last_error()
            for interp in (0, 1, 2):
                got = lib.pb_remap_track_px(args[0], FAKE, 1, interp, *args[1:], 0, 0, ch, sb, None), lib.pb_last_error()
                assert got == want and got[0] == INVALID and got[1] in (b"null argument", b"negative frame count"), (ch, sb, args, interp, got, want)
        frame, a = 4 * 8 * B, nat.px_align(B)
        layouts = [(FAKE, FAKE, 1, 0, frame - a), (FAKE, FAKE, 2, frame - a, 0)]  # a stride smaller than a frame
        if a > 1:  # misaligned pointers and strides, per pixel size
            layouts += [(FAKE + 1, FAKE, 1, 0, 0), (FAKE, FAKE + a // 2, 1, 0, 0), (FAKE, FAKE, 1, frame + 1, 0), (FAKE, FAKE, 1, 0, frame + a // 2),
                        (FAKE, FAKE, 2, frame + a + 1, frame + a)]
        for s, d, n, ss, ds in layouts:
            want = lib.pb_remap_px(h, s, d, n, ss, ds, B, None), lib.pb_last_error()
            got = track(lib, h, src=s, dst=d, n=n, ss=ss, ds=ds, ch=ch, sb=sb)
            assert got == want and got[0] == INVALID, (ch, sb, (s, d, n, ss, ds), got, want)
            assert b"smaller than a frame" in got[1] or got[1] == f"frame pointers and strides must be multiples of {a} bytes for {B}-byte pixels".encode()
        # a frame-argument refusal comes before the table's
        assert track(lib, h, table=None, ds=frame - a, ch=ch, sb=sb) == (INVALID, b"dst_frame_stride smaller than a frame")


def test_every_table_count_and_interpolation_refusal_of_pb_remap_track_u8_follows_in_its_order(deferred):
    lib, h = deferred
    for ch, sb in FORMATS:
        kw = dict(ch=ch, sb=sb)
        assert track(lib, h, table=None, **kw) == (INVALID, b"null rotation table")
        for off in (1, 2, 4, 7):
            assert track(lib, h, table=FAKE + off, **kw) == (INVALID, b"the rotation table must be 8-byte aligned"), off
        for k in (0, -1, -100):
            assert track(lib, h, k=k, **kw) == (INVALID, b"n_rot_per_frame must be at least 1"), k
        for interp in (-1, 3, 7):
            assert track(lib, h, interp=interp, **kw) == (INVALID, b"interpolation must be PB_INTERP_NEAREST, PB_INTERP_BILINEAR or PB_INTERP_CATMULL_ROM"), interp
        assert track(lib, h, k=9, **kw) == (INVALID, b"the plan's 0 rotations and 9 per frame exceed PB_MAX_ROTATIONS (8)")
        # the same calls of pb_remap_track_u8, status and message
        for t, k, interp in ((None, 1, 0), (FAKE + 4, 1, 0), (FAKE, 0, 0), (FAKE, 1, 3), (FAKE, 9, 0), (None, 0, 7), (FAKE + 1, 9, 7), (FAKE, 0, 7)):
            want = lib.pb_remap_track_u8(h, t, k, interp, FAKE, FAKE, 1, 0, 0, None), lib.pb_last_error()
            assert track(lib, h, table=t, k=k, interp=interp, **kw) == want and want[0] == INVALID, (t, k, interp)
    # the table's and the interpolation's checks come before the format's
    assert track(lib, h, table=None, ch=5) == (INVALID, b"null rotation table")
    assert track(lib, h, interp=3, ch=0, sb=3)[1].startswith(b"interpolation must be")
    lib2, h2 = _plan(n_rot=7)
    try:
        assert track(lib2, h2, k=2) == (INVALID, b"the plan's 7 rotations and 2 per frame exceed PB_MAX_ROTATIONS (8)")
        assert track(lib2, h2, k=1, n=0)[0] == OK
    finally:
        lib2.pb_plan_destroy(h2)


def test_channels_and_sample_bytes_outside_their_sets_are_invalid(deferred):
    lib, h = deferred
    for ch, sb in ((0, 1), (5, 1), (0, 2), (5, 2), (1, 0), (1, 3), (4, 0), (4, 3), (-1, 1), (2, 4), (6, 1), (2, 3)):
        for n in (0, 1):
            rc_, msg = track(lib, h, ch=ch, sb=sb, n=n)
            assert rc_ == INVALID and b"channels" in msg and b"sample_bytes" in msg, (ch, sb, n, msg)
        assert lib.pb_remap_track_px_supported(h, ch, sb) == INVALID, (ch, sb)
    assert lib.pb_remap_track_px_supported(None, 4, 1) == INVALID and lib.pb_last_error() == b"null argument"
    for ch, sb in FORMATS:  # a deferred plan of a single source: every format
        assert lib.pb_remap_track_px_supported(h, ch, sb) == 1, (ch, sb)


def test_a_double_fisheye_with_16_bit_samples_is_unsupported_and_names_the_map_route(deferred_double):
    lib, h = deferred_double
    for ch in (1, 2, 3, 4):
        assert lib.pb_remap_track_px_supported(h, ch, 2) == 0 and lib.pb_remap_track_px_supported(h, ch, 1) == 1, ch
        for interp in (0, 1, 2):
            for n in (0, 1):
                rc_, msg = track(lib, h, interp=interp, ch=ch, sb=2, n=n)
                assert rc_ == UNSUPPORTED and b"pb_sample_map_" in msg and b"pb_gather_blend_u8" in msg, (ch, interp, n, msg)
    # the argument checks come first
    assert track(lib, h, table=None, ch=4, sb=2) == (INVALID, b"null rotation table")
    assert track(lib, h, interp=9, ch=4, sb=2)[0] == INVALID
    plan = nat.Plan(nat.make_proj(nat.KIND_PANO, 4, 8), [], nat.make_proj(nat.KIND_DOUBLE, 4, 8, lens=0, fov=3.4, f_distance=2.0), defer=True)
    assert plan.track_px_supported(4, 1) and not plan.track_px_supported(4, 2)
    with pytest.raises(nat.PbError):
        plan.track_px_supported(5, 1)


def test_no_frames_is_ok_and_launches_nothing(deferred, deferred_double):
    for lib, h in (deferred, deferred_double):
        for ch, sb in FORMATS:
            if sb == 2 and h is deferred_double[1]:
                continue
            for interp in (0, 1, 2):
                for k in (1, 2, 8):
                    assert lib.pb_remap_track_px(h, FAKE, k, interp, FAKE, FAKE, 0, 0, 0, ch, sb, None) == OK, (ch, sb, interp, k)


# ---- Plan.remap_track_px against a stand-in ----------------------------------------------------------------------------------------
class FakeTrackPxLib(FakePipeLib):
    """tests/test_host_memory.py's stand-in with the two track launches: they record their arguments."""

    def __init__(self):
        super().__init__()
        self.calls = []

    def pb_remap_track_px(self, plan, table, k, interp, src, dst, n, ss, ds, channels, sample_bytes, stream):
        mats = np.frombuffer((ctypes.c_double * (9 * int(k) * int(n))).from_address(int(table)), np.float64).reshape(int(n), int(k), 3, 3).copy()
        self.calls.append({"fn": "px", "table": int(table), "k": int(k), "interp": int(interp), "src": int(src), "dst": int(dst), "n": int(n), "ss": int(ss),
                           "ds": int(ds), "channels": int(channels), "sample_bytes": int(sample_bytes), "stream": int(stream or 0), "mats": mats})
        return 0

    def pb_remap_track_u8(self, plan, table, k, interp, src, dst, n, ss, ds, stream):
        self.calls.append({"fn": "u8"})
        return 0


@pytest.fixture
def env(monkeypatch):
    p = nat.make_proj(nat.KIND_PANO, 4, 8)
    d = nat.make_proj(nat.KIND_DOUBLE, 4, 8, lens=0, fov=3.4, f_distance=2.0)
    plans = {0: nat.Plan(p, [], p, defer=True), 7: nat.Plan(p, [np.eye(3)] * 7, p, defer=True), "double": nat.Plan(p, [], d, defer=True)}
    lib = FakeTrackPxLib()
    monkeypatch.setattr(_device, "_lib", lambda: lib)
    monkeypatch.setattr(nat, "load", lambda: lib)
    monkeypatch.setattr(nat, "require_gpu", lambda: None)
    monkeypatch.setattr(nat, "current_device", lambda: 0)
    monkeypatch.setattr(nat, "current_stream", lambda: 0)
    monkeypatch.setattr(nat, "on_device", lambda d: contextlib.nullcontext())
    monkeypatch.setattr(_device, "PINNED", _device._PinnedPool())
    monkeypatch.setattr(_hostpipe, "PINNED", _device.PINNED)
    monkeypatch.setattr(_hostpipe, "REGISTERED", _device._Registrations())
    monkeypatch.setattr(_hostpipe, "_TLS", __import__("threading").local())
    return lib, plans


@pytest.mark.parametrize("shape,dt,interp,fmt", [
    ((3, 4, 8), np.uint8, "nearest", (1, 1)), ((3, 4, 8), np.uint8, "bilinear", (1, 1)),
    ((3, 4, 8), np.uint16, "nearest", (2, 1)), ((3, 4, 8), np.uint16, "catmull-rom", (1, 2)),
    ((3, 4, 8, 4), np.uint8, "nearest", (4, 1)), ((3, 4, 8, 4), np.uint8, "bilinear", (4, 1)),
    ((3, 4, 8, 3), np.uint16, "nearest", (3, 2)), ((3, 4, 8, 3), np.uint16, "bilinear", (3, 2)),
    ((3, 4, 8), np.float32, "nearest", (4, 1)), ((3, 4, 8, 2), np.float32, "nearest", (4, 2)), ((3, 4, 8, 3), np.uint8, "nearest", (3, 1)),
], ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else getattr(v, "__name__", str(v)))
def test_plan_remap_track_px_passes_the_format_strides_and_stream(env, shape, dt, interp, fmt):
    """nearest on a single source never looks inside a pixel: B bytes go as (B, 1) up to four, else as (B / 2, 2); the interpolating modes
    pass the channels and the sample size"""
    lib, plans = env
    src = _device.DeviceArray(shape, dt)
    mats = rotation_track(np.arange(18.0).reshape(6, 3)).reshape(3, 2, 3, 3)
    out = plans[0].remap_track_px(src, mats, interpolation=interp, stream=0x77)
    assert isinstance(out, _device.DeviceArray) and out.shape == shape and out.dtype == dt
    c = lib.calls[-1]
    assert c["fn"] == "px" and (c["channels"], c["sample_bytes"]) == fmt
    assert (c["k"], c["interp"], c["src"], c["dst"], c["n"], c["ss"], c["ds"], c["stream"]) == (2, nat.TRACK_INTERP_IDS[interp], src.data_ptr(), out.data_ptr(), 3, 0, 0, 0x77)
    assert np.array_equal(H.bits(c["mats"]), H.bits(mats)) and [k for k, _ in lib.log].count("h2d") == 1
    # into a caller's output, from a device table used in place
    mine = _device.DeviceArray(shape, dt)
    tab = _device.DeviceArray((3, 3, 3), np.float64).copy_from_host(mats[:, 0])
    copies = [k for k, _ in lib.log].count("h2d")
    assert plans[7].remap_track_px(src, tab, out=mine, interpolation=interp) is mine
    c = lib.calls[-1]
    assert (c["table"], c["k"], c["dst"], c["stream"]) == (tab.data_ptr(), 1, mine.data_ptr(), 0) and [k for k, _ in lib.log].count("h2d") == copies


def test_plan_remap_track_px_on_a_double_fisheye_passes_uint8_channels(env):
    lib, plans = env
    for shape, fmt in (((2, 4, 8), (1, 1)), ((2, 4, 8, 2), (2, 1)), ((2, 4, 8, 4), (4, 1))):
        for interp in ("nearest", "bilinear"):
            out = plans["double"].remap_track_px(_device.DeviceArray(shape, np.uint8), np.zeros((2, 3, 3)), interpolation=interp)
            assert out.shape == shape and (lib.calls[-1]["channels"], lib.calls[-1]["sample_bytes"]) == fmt


def test_plan_remap_track_px_refuses_before_any_device_work(env):
    lib, plans = env
    plan = plans[0]
    src = _device.DeviceArray((3, 4, 8, 4), np.uint8)
    mats = rotation_track(np.arange(9.0).reshape(3, 3))
    grey_f32 = _device.DeviceArray((3, 4, 8), np.float32)
    bad_calls = [
        (nat.PbError, plan, dict(src=np.zeros((3, 4, 8, 4), np.uint8), rotations=mats)),                    # a host ndarray
        (nat.PbError, plan, dict(src=grey_f32, rotations=mats, interpolation="bilinear")),                  # float samples, interpolated
        (nat.PbError, plan, dict(src=grey_f32, rotations=mats, interpolation="catmull-rom")),
        (nat.PbError, plan, dict(src=_device.DeviceArray((3, 4, 8, 5), np.uint8), rotations=mats)),         # five bytes a pixel
        (nat.PbError, plan, dict(src=_device.DeviceArray((3, 4, 8, 5), np.uint8), rotations=mats, interpolation="bilinear")),
        (nat.PbError, plan, dict(src=_device.DeviceArray((3, 4, 8, 3), np.float32), rotations=mats)),       # twelve bytes a pixel
        (nat.PbError, plan, dict(src=_device.DeviceArray((4, 8, 4), np.uint8), rotations=mats)),            # not a batch of the plan's source
        (nat.PbError, plan, dict(src=_device.DeviceArray((3, 4, 7, 4), np.uint8), rotations=mats)),
        (nat.PbError, plan, dict(src=src, rotations=mats, out=_device.DeviceArray((3, 4, 8, 3), np.uint8))),  # a wrong out: shape, dtype, kind
        (nat.PbError, plan, dict(src=src, rotations=mats, out=_device.DeviceArray((3, 4, 8, 4), np.uint16))),
        (nat.PbError, plan, dict(src=src, rotations=mats, out=np.zeros((3, 4, 8, 4), np.uint8))),
        (ValueError, plan, dict(src=src, rotations=mats[:2])),                                               # a table of the wrong length
        (ValueError, plan, dict(src=src, rotations=mats.astype(np.float32))),
        (ValueError, plan, dict(src=src, rotations=np.zeros((3, 9, 3, 3)))),
        (ValueError, plan, dict(src=src, rotations=mats, interpolation="cubic")),
        (ValueError, plans[7], dict(src=src, rotations=np.zeros((3, 2, 3, 3)))),
        (nat.PbError, plans["double"], dict(src=_device.DeviceArray((3, 4, 8), np.uint16), rotations=mats)),  # a double fisheye blends uint8
        (nat.PbError, plans["double"], dict(src=grey_f32, rotations=mats)),
    ]
    for exc, p, kw in bad_calls:
        with pytest.raises(exc):
            p.remap_track_px(**kw)
    with pytest.raises(ValueError):
        plan.launch_track_px(FAKE, 1, FAKE, FAKE, 1, 4, 1, interpolation="cubic")
    assert lib.calls == [] and not lib.log, "a refused call reached the library"
    # no frames: nothing is launched
    assert plan.remap_track_px(_device.DeviceArray((0, 4, 8), np.uint16), np.empty((0, 3, 3))).shape == (0, 4, 8) and lib.calls == []


def test_the_existing_refusals_of_remap_track_and_remap_frames_are_unchanged(env):
    lib, plans = env
    mats = rotation_track(np.arange(9.0).reshape(3, 3))
    with pytest.raises(nat.PbError):  # a uint16 source
        plans[0].remap_track(_device.DeviceArray((3, 4, 8, 3), np.uint16), mats)
    with pytest.raises(nat.PbError):  # a four-channel out
        plans[0].remap_track(_device.DeviceArray((3, 4, 8, 3), np.uint8), mats, out=_device.DeviceArray((3, 4, 8, 4), np.uint8))
    with pytest.raises(ValueError):  # a grey frame with a track
        list(batch.remap_frames(plans[0], [np.zeros((4, 8), np.uint8)], rotations=np.zeros((1, 3, 3))))
    assert lib.calls == []


# ---- the definition on the CPU -------------------------------------------------------------------------------------------------------
GOLD = np.load(os.path.join(H.GOLD, "rotation_track.npz"))


def frames_of(case, f, rng):
    """grey16 and RGBA8 frames whose RGB is the case's synthetic frame f"""
    rgb = rc.case_frames(case)[f]
    rgba = np.concatenate([rgb, rng.integers(0, 256, rgb.shape[:2] + (1,), dtype=np.uint8)], axis=2)
    grey16 = (rgb[..., 0].astype(np.uint16) << 8) | rgb[..., 1]
    return grey16, rgba


@pytest.mark.parametrize("case", rc.golden_cases(), ids=lambda c: c.name)
def test_the_golden_index_maps_gather_grey16_and_rgba8_frames_to_the_oracle_s_bytes(case):
    """What pb_remap_track_px's nearest mode is defined as: np.where(idx < 0, 0, flat[idx]) with the real reference's per-frame index map -
    and the reference fancy-indexes whatever array it is given.  A double fisheye blends per byte: the first three channels of an RGBA
    frame are the RGB golden."""
    dst, src = H.orc_proj(case.dst), H.orc_proj(case.src)
    exact = H.live_numpy_is_the_goldens_numpy()
    rng = np.random.default_rng(20261020)
    for f in range(4):
        rots = [tuple(map(orc.to_radians, r)) for r in case.chain(f)]
        grey16, rgba = frames_of(case, f, rng)
        with np.errstate(all="ignore"):
            fragile = orc.fragile_mask(orc.pretrunc(dst, src, rots))
            want_rgba = orc.remap(dst, src, rgba, rots)
        if case.src[0] == "double":
            bad = (want_rgba[..., :3] != GOLD[f"{case.name}/{f}/u8"]).any(axis=2)
            assert want_rgba.dtype == np.uint8 and want_rgba[..., :3].any()
        else:
            idx = GOLD[f"{case.name}/{f}/idx"]
            with np.errstate(all="ignore"):
                want_grey = orc.remap(dst, src, grey16, rots)
            got_rgba = np.where((idx < 0)[..., None], 0, rgba.reshape(-1, 4)[np.where(idx < 0, 0, idx)]).astype(np.uint8)
            got_grey = np.where(idx < 0, 0, grey16.reshape(-1)[np.where(idx < 0, 0, idx)]).astype(np.uint16)
            assert want_grey.dtype == np.uint16 and want_grey.shape == idx.shape and want_rgba.shape == idx.shape + (4,) and got_rgba.any() and got_grey.any()
            bad = (got_rgba != want_rgba).any(axis=2) | (got_grey != want_grey) | (got_rgba[..., :3] != GOLD[f"{case.name}/{f}/u8"]).any(axis=2)
        assert int((bad & ~fragile).sum()) == 0, (case.name, f, int(bad.sum()))
        if exact:
            assert int(bad.sum()) == 0, (case.name, f, int(bad.sum()))
