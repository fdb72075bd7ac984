"""CPU-only checks of rotation tracks for NV12 / P010 video frames (pb_remap_track_nv12): the symbol and its signature, every
argument check in its order and with its message - on deferred plans with fake pointers: a deferred plan has no device, and every call here
is refused (or has no frames) before anything could be launched - and Plan.remap_track_nv12's own checks against the stand-ins of
tests/test_rotation_track_host.py."""

import ctypes as C
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
DECLARATION = ("const pb_plan* plan, const double* rot3x3_dev, int n_rot_per_frame, const void* src_dev, void* dst_dev, int n_frames, "
               "const pb_nv12_layout* src_layout, const pb_nv12_layout* dst_layout, int bytes_per_sample, const uint16_t fill_yuv[3], void* stream")


def _deferred(src=(nat.KIND_PANO, 4, 8), dst=(nat.KIND_PANO, 6, 12), n_rot=0):
    lib = nat.load()
    h = C.c_void_p()
    s, d = nat.make_proj(*src), nat.make_proj(*dst)
    rots = (C.c_double * (9 * max(1, n_rot)))(*([1, 0, 0, 0, 1, 0, 0, 0, 1] * max(1, n_rot)))
    assert lib.pb_plan_create_ex(C.byref(d), rots if n_rot else None, n_rot, C.byref(s), nat.PLAN_DEFER, 0, C.byref(h)) == 0, lib.pb_last_error()
    return lib, h


@pytest.fixture
def deferred():
    lib, h = _deferred()  # source 4 x 8, destination 6 x 12
    yield lib, h
    lib.pb_plan_destroy(h)


def call(lib, plan, table=FAKE, k=1, src=FAKE, dst=FAKE, n=1, sl=None, dl=None, S=1, fill=None):
    sl = None if sl is None else nat.pb_nv12_layout(*sl)
    dl = None if dl is None else nat.pb_nv12_layout(*dl)
    f = None if fill is None else (C.c_uint16 * 3)(*fill)
    rc = lib.pb_remap_track_nv12(plan, table, k, src, dst, n, None if sl is None else C.addressof(sl), None if dl is None else C.addressof(dl), S,
                                 None if f is None else C.addressof(f), None)
    return rc, lib.pb_last_error()


def test_the_symbol_exists_with_the_declared_signature_and_the_abi_is_still_5():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "photonbend_hip.h")).read(), flags=re.S)
    m = re.search(r"\bint pb_remap_track_nv12\s*\(([^)]*)\)\s*;", text)
    assert m and " ".join(m.group(1).split()) == DECLARATION
    assert re.search(r"#define PB_ABI_VERSION 5\b", text)
    vp = C.c_void_p
    assert nat.SIGNATURES["pb_remap_track_nv12"] == (C.c_int, [vp, vp, C.c_int, vp, vp, C.c_int, vp, vp, C.c_int, vp, vp])
    lib = nat.load()
    assert hasattr(lib, "pb_remap_track_nv12") and lib.pb_abi_version() == 5 == nat.ABI_VERSION
    assert callable(nat.Plan.launch_track_nv12) and callable(nat.Plan.remap_track_nv12)


def test_every_argument_check_in_its_order_with_its_message(deferred):
    """Each call breaks one rule and every rule AFTER it too: the message is the first broken rule's.  `worse` accumulates the later
    rules' violations, from the last check backwards."""
    lib, h = deferred
    worse = dict(n=0)  # (n_frames == 0 is the last decision: PB_OK)
    assert call(lib, h, **worse) == (0, lib.pb_last_error())
    steps = [  # from the last check to the first: (the arguments that break it, its message)
        (dict(k=9), b"the plan's 0 rotations and 9 per frame exceed PB_MAX_ROTATIONS (8)"),
        (dict(k=0), b"n_rot_per_frame must be at least 1"),
        (dict(table=FAKE + 4), b"the rotation table must be 8-byte aligned"),
        (dict(table=None), b"null rotation table"),
        (dict(dst=FAKE + 1), b"frame pointers must be multiples of 2 bytes (one chroma pair)"),
        (dict(dl=(10, 0, 0)), b"destination pitch smaller than a row"),
        (dict(sl=(0, 2, 0)), b"source uv_offset smaller than the luma plane"),
    ]
    for change, message in steps:
        worse.update(change)
        assert call(lib, h, **worse) == (INVALID, message), (change, lib.pb_last_error())
    # odd dimensions: a plan of its own, every later rule still broken
    lib2, odd = _deferred(dst=(nat.KIND_PANO, 6, 11))
    try:
        assert call(lib2, odd, **worse) == (INVALID, b"4:2:0 frames need even source and destination dimensions")
        for S in (0, 3, 4, -1):
            assert call(lib2, odd, **{**worse, "S": S}) == (INVALID, b"bytes_per_sample outside {1, 2}"), S
        assert call(lib2, odd, **{**worse, "S": 3, "n": -1}) == (INVALID, b"negative frame count")
        for nulls in (dict(src=None), dict(dst=None), dict(src=None, dst=None)):
            assert call(lib2, odd, **{**worse, "S": 3, "n": -1, **nulls}) == (INVALID, b"null argument"), nulls
        assert call(lib2, None, **{**worse, "S": 3, "n": -1}) == (INVALID, b"null argument")
    finally:
        lib2.pb_plan_destroy(odd)


def test_the_frame_checks_and_messages_are_pb_remap_nv12s(deferred):
    """The same arguments to both entry points: whatever pb_remap_nv12 refuses as invalid, pb_remap_track_nv12 refuses with the same message."""
    lib, h = deferred
    for S in (1, 2):
        ok_s, ok_d = (S * 8, S * 8 * 4, S * 8 * 6), (S * 12, S * 12 * 6, S * 12 * 9)
        broken = [dict(src=None), dict(dst=None), dict(n=-1), dict(src=FAKE + S), dict(dst=FAKE + S), dict(src=FAKE + 1)]
        for which, base in (("sl", ok_s), ("dl", ok_d)):
            broken += [{which: v} for v in ((base[0] - 2 * S, 0, 0), (0, base[1] - 2 * S, 0), (base[0] + 2 * S, base[1], 0), (0, 0, base[2] - 2 * S),
                                           (0, base[1] + 2 * S, base[2]), (base[0] + S, 0, 0), (0, base[1] + S, 0), (0, 0, base[2] + S))]
        for kw in broken:
            sl = None if kw.get("sl") is None else nat.pb_nv12_layout(*kw["sl"])
            dl = None if kw.get("dl") is None else nat.pb_nv12_layout(*kw["dl"])
            want = lib.pb_remap_nv12(h, kw.get("src", FAKE), kw.get("dst", FAKE), kw.get("n", 1), None if sl is None else C.addressof(sl),
                                     None if dl is None else C.addressof(dl), S, None, None), lib.pb_last_error()
            assert want[0] == INVALID
            assert call(lib, h, S=S, **kw) == want, (S, kw)
        # a pitch or an offset no frame below 2^31 bytes can have is refused before anything is multiplied
        for which in ("sl", "dl"):
            for huge in (((1 << 63) + (1 << 20), 0, 0), (1 << 31, 0, 0), (0, 1 << 31, 0), (0, (1 << 64) - 2 * S, 0)):
                rc, msg = call(lib, h, S=S, **{which: huge})
                assert rc == UNSUPPORTED and b"2^31" in msg, (S, which, huge, msg)
        # ... and a span that reaches 2^31 through the rows: refused with the way round, after every argument check
        rc, msg = call(lib, h, S=S, dl=((1 << 30), 0, 0))
        assert rc == UNSUPPORTED and b"2^31" in msg and b"pb_index_map_i32" in msg, msg
        assert call(lib, h, S=S, dl=((1 << 30), 0, 0), k=0) == (INVALID, b"n_rot_per_frame must be at least 1")


def test_the_rotation_limit_counts_the_plan_s_own_rotations():
    assert nat.PB_MAX_ROTATIONS == 8
    for n_rot in (1, 5, 7, 8):
        lib, h = _deferred(n_rot=n_rot)
        try:
            k = 8 - n_rot + 1
            assert call(lib, h, k=k) == (INVALID, f"the plan's {n_rot} rotations and {k} per frame exceed PB_MAX_ROTATIONS (8)".encode())
            if n_rot < 8:  # the boundary itself is accepted (no frames: nothing to launch)
                assert call(lib, h, k=k - 1, n=0)[0] == 0
        finally:
            lib.pb_plan_destroy(h)


def test_no_frames_is_ok_with_no_launch_and_no_device(deferred):
    lib, h = deferred
    for S in (1, 2):
        for k in (1, 2, 8):
            assert call(lib, h, k=k, n=0, S=S)[0] == 0
            assert call(lib, h, k=k, n=0, S=S, sl=(S * 8 + 6 * S, 0, 0), fill=(1, 2, 3))[0] == 0


def test_a_double_fisheye_source_is_unsupported_and_says_the_way_round():
    lib, h = _deferred(src=(nat.KIND_DOUBLE, 6, 12, nat.LENS_IDS["equidistant"], 3.3, 3.0, 2.0))
    try:
        for S in (1, 2):
            rc, msg = call(lib, h, S=S)
            assert rc == UNSUPPORTED and b"double fisheye" in msg and b"pb_remap_track_u8" in msg, msg
            assert call(lib, h, S=S, k=0)[0] == INVALID  # (the argument checks come first)
    finally:
        lib.pb_plan_destroy(h)


# ---- Plan.remap_track_nv12 against stand-ins -------------------------------------------------------------------------------------------
class FakeTrackNv12Lib(FakeTrackLib):
    def pb_remap_track_nv12(self, plan, table, k, src, dst, n, sl, dl, S, fill, stream):
        mats = np.frombuffer((C.c_double * (9 * int(k) * int(n))).from_address(int(table)), np.float64).reshape(int(n), int(k), 3, 3).copy()
        self.calls.append({"table": int(table), "k": int(k), "src": int(src), "dst": int(dst), "n": int(n), "sl": sl, "dl": dl, "S": int(S),
                           "fill": None if not fill else list((C.c_uint16 * 3).from_address(int(fill))), "stream": int(stream or 0), "mats": mats})
        return 0


@pytest.fixture
def video_env(env, monkeypatch):  # noqa: F811
    _, plans = env
    lib = FakeTrackNv12Lib()
    monkeypatch.setattr(_device, "_lib", lambda: lib)
    monkeypatch.setattr(nat, "load", lambda: lib)
    return lib, plans


def test_plan_remap_track_nv12_checks_shapes_dtypes_and_table_lengths_before_any_device_work(video_env):
    lib, plans = video_env
    plan = plans[0]  # 4 x 8 -> 4 x 8: packed frames are (6, 8)
    src = _device.DeviceArray((3, 6, 8), np.uint8)
    mats = rotation_track(np.arange(9.0).reshape(3, 3))
    bad_calls = [
        (nat.PbError, dict(src=np.zeros((3, 6, 8), np.uint8), rotations=mats)),                       # not a device array
        (nat.PbError, dict(src=_device.DeviceArray((3, 4, 8), np.uint8), rotations=mats)),            # luma only
        (nat.PbError, dict(src=_device.DeviceArray((3, 6, 8, 1), np.uint8), rotations=mats)),
        (nat.PbError, dict(src=_device.DeviceArray((3, 6, 8), np.float32), rotations=mats)),          # not a sample type
        (nat.PbError, dict(src=_device.DeviceArray((3, 6, 8), np.uint8), rotations=mats, src_layout=(16, 0, 0))),  # a layout wants a 1-D buffer
        (nat.PbError, dict(src=_device.DeviceArray((40,), np.uint8), rotations=mats[:1], src_layout=(16, 0, 0))),  # ... that holds a frame
        (ValueError, dict(src=src, rotations=mats[:2])),                                               # two rotations for three frames
        (ValueError, dict(src=_device.DeviceArray((6, 8), np.uint8), rotations=mats)),                 # three rotations for one frame
        (ValueError, dict(src=src, rotations=mats.astype(np.float32))),
        (ValueError, dict(src=src, rotations=np.zeros((3, 9)))),
        (ValueError, dict(src=src, rotations=np.zeros((3, 9, 3, 3)))),                                 # nine rotations per frame
        (nat.PbError, dict(src=src, rotations=mats, out=_device.DeviceArray((3, 6, 8), np.uint16))),   # the other sample type
        (nat.PbError, dict(src=src, rotations=mats, out=_device.DeviceArray((2, 6, 8), np.uint8))),
        (nat.PbError, dict(src=src, rotations=mats, out=np.zeros((3, 6, 8), np.uint8))),
        (nat.PbError, dict(src=src, rotations=mats, dst_layout=(16, 0, 0))),                            # a layout without its buffer
        (nat.PbError, dict(src=src, rotations=mats, out=_device.DeviceArray((100,), np.uint8), dst_layout=(16, 0, 0))),  # too small
    ]
    for exc, kw in bad_calls:
        with pytest.raises(exc):
            plan.remap_track_nv12(**kw)
    with pytest.raises(ValueError, match="PB_MAX_ROTATIONS"):
        plans[7].remap_track_nv12(src, np.zeros((3, 2, 3, 3)))
    assert lib.calls == [] and not lib.log, "a refused call reached the library"


def test_plan_remap_track_nv12_uploads_an_ndarray_uses_a_device_table_in_place_and_passes_layouts_and_fill(video_env):
    lib, plans = video_env
    plan = plans[0]
    for dt in (np.uint8, np.uint16):
        S = np.dtype(dt).itemsize
        src = _device.DeviceArray((3, 6, 8), dt)
        mats = rotation_track(np.arange(18.0).reshape(6, 3)).reshape(3, 2, 3, 3)
        copies = [k for k, _ in lib.log].count("h2d")
        out = plan.remap_track_nv12(src, mats, fill=(1, 2, 3), stream=0x77)
        assert isinstance(out, _device.DeviceArray) and out.shape == (3, 6, 8) and out.dtype == np.dtype(dt)
        c = lib.calls[-1]
        assert (c["k"], c["src"], c["dst"], c["n"], c["S"], c["fill"], c["stream"], c["sl"], c["dl"]) == (2, src.data_ptr(), out.data_ptr(), 3, S, [1, 2, 3], 0x77, None, None)
        assert np.array_equal(c["mats"], mats) and [k for k, _ in lib.log].count("h2d") == copies + 1
        # a float64 device table: the very pointer, no copy; a pitched 1-D source into a pitched `out`
        tab = _device.DeviceArray((2, 3, 3), np.float64).copy_from_host(mats[:2, 0])
        copies = [k for k, _ in lib.log].count("h2d")
        pitch = 8 * S + 6 * S
        buf, mine = _device.DeviceArray((2 * pitch * 6 // S,), dt), _device.DeviceArray((2 * pitch * 6 // S,), dt)
        assert plan.remap_track_nv12(buf, tab, out=mine, src_layout=(pitch, 0, 0), dst_layout={"pitch": pitch}) is mine
        c = lib.calls[-1]
        assert (c["table"], c["k"], c["n"], c["S"], c["fill"], c["dst"]) == (tab.data_ptr(), 1, 2, S, None, mine.data_ptr())
        assert c["sl"] and c["dl"] and [k for k, _ in lib.log].count("h2d") == copies
