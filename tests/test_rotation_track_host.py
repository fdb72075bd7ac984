"""CPU-only checks of rotation tracks: pb_remap_track_u8's symbol, signature and argument checks - a deferred plan has no
device and every call here is refused before anything could be launched -, core.rotation_track against Rotation, the golden fixture
against the oracle, and Plan.remap_track / batch.remap_frames(rotations=...) against stand-ins for the library (tests/test_host_memory.py's)."""

import contextlib
import ctypes
import os
import re

import numpy as np
import pytest

import photonbend_amd as pb
from oracle import reference_path as orc
from photonbend_amd import _device, _hostpipe, batch
from photonbend_amd import _native as nat
from photonbend_amd.core import rotation_track
from tests import helpers as H
from tests import rotation_track_cases as rc
from tests.test_host_memory import FakePipeLib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x1000  # a non-null, 8-byte aligned "device pointer" for calls that must be refused before anything reads it
INVALID = -1


def _deferred(n_rot=0):
    lib = nat.load()
    h = ctypes.c_void_p()
    p = nat.make_proj(nat.KIND_PANO, 4, 8)
    rots = (ctypes.c_double * (9 * max(1, n_rot)))(*([1, 0, 0, 0, 1, 0, 0, 0, 1] * max(1, n_rot)))
    assert lib.pb_plan_create_ex(ctypes.byref(p), rots if n_rot else None, n_rot, ctypes.byref(p), nat.PLAN_DEFER, 0, ctypes.byref(h)) == 0
    return lib, h


@pytest.fixture
def deferred():
    lib, h = _deferred()
    yield lib, h
    lib.pb_plan_destroy(h)


def track(lib, h, table=FAKE, k=1, interp=0, src=FAKE, dst=FAKE, n=1, ss=0, ds=0):
    return lib.pb_remap_track_u8(h, table, k, interp, src, dst, n, ss, ds, None), lib.pb_last_error()


def test_the_symbol_exists_with_the_declared_signature_and_the_abi_is_still_5():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "photonbend_hip.h")).read(), flags=re.S)
    m = re.search(r"\bint pb_remap_track_u8\s*\(([^)]*)\)\s*;", text)
    assert m and " ".join(m.group(1).split()) == ("const pb_plan* plan, const double* rot3x3_dev, int n_rot_per_frame, int interpolation, const uint8_t* src_dev, "
                                                  "uint8_t* dst_dev, int n_frames, size_t src_frame_stride, size_t dst_frame_stride, void* stream")
    assert re.search(r"#define PB_INTERP_NEAREST 0\b", text) and re.search(r"#define PB_INTERP_BILINEAR 1\b", text) and re.search(r"#define PB_INTERP_CATMULL_ROM 2\b", text)
    assert re.search(r"#define PB_ABI_VERSION 5\b", text)
    vp, C = ctypes.c_void_p, ctypes
    assert nat.SIGNATURES["pb_remap_track_u8"] == (C.c_int, [vp, vp, C.c_int, C.c_int, vp, vp, C.c_int, C.c_size_t, C.c_size_t, vp])
    assert nat.TRACK_INTERP_IDS == {"nearest": 0, "bilinear": 1, "catmull-rom": 2} and nat.TRACK_MATRIX_BYTES == 72
    lib = nat.load()
    assert hasattr(lib, "pb_remap_track_u8") and lib.pb_abi_version() == 5 == nat.ABI_VERSION


def test_frame_arguments_are_checked_like_pb_remap_u8s(deferred):
    lib, h = deferred
    for args in ((h, None, None, 1), (h, None, FAKE, 1), (h, FAKE, None, 3), (h, None, None, 0), (h, None, None, -1), (None, None, None, -1),
                 (None, FAKE, FAKE, 1), (h, FAKE, FAKE, -1), (h, FAKE, FAKE, -7)):
        want = lib.pb_remap_u8(*args, 0, 0, None), lib.pb_last_error()
        for interp in (0, 1, 2):
            got = lib.pb_remap_track_u8(args[0], FAKE, 1, interp, *args[1:], 0, 0, None), lib.pb_last_error()
            assert got == want and got[0] == INVALID and got[1] in (b"null argument", b"negative frame count"), (args, interp, got, want)
    frame = 3 * 4 * 8
    assert track(lib, h, ds=frame - 1) == (INVALID, b"dst_frame_stride smaller than a frame")
    assert track(lib, h, n=2, ss=frame - 1) == (INVALID, b"src_frame_stride smaller than a frame")


def test_every_invalid_table_count_and_interpolation_is_refused_with_its_message(deferred):
    lib, h = deferred
    assert track(lib, h, table=None) == (INVALID, b"null rotation table")
    for off in (1, 2, 4, 7):
        assert track(lib, h, table=FAKE + off) == (INVALID, b"the rotation table must be 8-byte aligned"), off
    for k in (0, -1, -100):
        assert track(lib, h, k=k) == (INVALID, b"n_rot_per_frame must be at least 1"), k
    for interp in (-1, 3, 7):
        assert track(lib, h, interp=interp) == (INVALID, b"interpolation must be PB_INTERP_NEAREST, PB_INTERP_BILINEAR or PB_INTERP_CATMULL_ROM"), interp
    # the plan's own rotations count: n_rot + n_rot_per_frame <= PB_MAX_ROTATIONS = 8
    assert nat.PB_MAX_ROTATIONS == 8
    assert track(lib, h, k=9)[0] == INVALID and b"exceed PB_MAX_ROTATIONS (8)" in lib.pb_last_error()
    for n_rot in (1, 5, 7, 8):
        lib2, h2 = _deferred(n_rot)
        try:
            rc_, msg = track(lib2, h2, k=8 - n_rot + 1)
            assert rc_ == INVALID and msg == f"the plan's {n_rot} rotations and {8 - n_rot + 1} per frame exceed PB_MAX_ROTATIONS (8)".encode(), (n_rot, msg)
            if n_rot < 8:  # the boundary itself is accepted (no frames: nothing to launch)
                assert track(lib2, h2, k=8 - n_rot, n=0)[0] == 0, n_rot
        finally:
            lib2.pb_plan_destroy(h2)


def test_no_frames_is_ok_and_launches_nothing(deferred):
    lib, h = deferred
    for interp in (0, 1, 2):
        for k in (1, 2, 8):
            assert lib.pb_remap_track_u8(h, FAKE, k, interp, FAKE, FAKE, 0, 0, 0, None) == 0 == lib.pb_remap_u8(h, FAKE, FAKE, 0, 0, 0, None)


def test_rotation_track_is_rotation_s_matrix_bit_for_bit():
    rng = np.random.default_rng(20261018)
    angles = np.concatenate([rng.uniform(-2 * np.pi, 2 * np.pi, (32, 3)),
                             [[pb.utils.to_radians(30), pb.utils.to_radians(45), pb.utils.to_radians(10)], [pb.utils.to_radians(-90), 0, 0], [0, 0, 0]]])
    tab = rotation_track(angles)
    assert tab.shape == (35, 3, 3) and tab.dtype == np.float64 and tab.flags.c_contiguous
    assert pb.core.rotation_track is rotation_track
    for k in range(35):
        want = pb.Rotation(*angles[k]).rotation_matrix
        assert np.array_equal(H.bits(tab[k]), H.bits(want)), k
        assert np.array_equal(H.bits(tab[k]), H.bits(pb.Rotation(float(angles[k, 0]), float(angles[k, 1]), float(angles[k, 2])).rotation_matrix)), k
    assert np.array_equal(tab[34], np.eye(3))
    assert rotation_track(np.empty((0, 3))).shape == (0, 3, 3)
    for bad in (np.zeros(3), np.zeros((2, 4)), np.zeros((2, 3, 3))):
        with pytest.raises(ValueError):
            rotation_track(bad)


def test_rotation_table_takes_arrays_and_rotation_objects_and_checks_them():
    mats = rotation_track(np.arange(12.0).reshape(4, 3))
    tab, n, k = nat.rotation_table(mats)
    assert (n, k) == (4, 1) and tab.shape == (4, 1, 3, 3) and tab.flags.c_contiguous and np.array_equal(tab[:, 0], mats)
    tab, n, k = nat.rotation_table(mats.reshape(2, 2, 3, 3), n_rot=6)
    assert (n, k) == (2, 2) and tab.shape == (2, 2, 3, 3)
    tab, n, k = nat.rotation_table([pb.Rotation(0.1 * f, 0.2, 0.3) for f in range(5)], n_rot=7)
    assert (n, k) == (5, 1) and all(np.array_equal(tab[f, 0], pb.Rotation(0.1 * f, 0.2, 0.3).rotation_matrix) for f in range(5))
    assert nat.rotation_table([])[1:] == (0, 1)
    for bad in (mats.astype(np.float32), mats.astype(np.int64), np.zeros((4, 9)), np.zeros((4, 3, 4)), np.zeros((3, 3)), np.zeros((2, 2, 2, 3, 3)), 7):
        with pytest.raises(ValueError):
            nat.rotation_table(bad)
    with pytest.raises(ValueError, match="PB_MAX_ROTATIONS"):
        nat.rotation_table(mats.reshape(2, 2, 3, 3), n_rot=7)
    with pytest.raises(ValueError, match="PB_MAX_ROTATIONS"):
        nat.rotation_table(mats, n_rot=8)
    with pytest.raises(ValueError):
        nat.rotation_table(np.zeros((4, 0, 3, 3)))


# ---- the golden fixture against the oracle ------------------------------------------------------------------------------------------
GOLD = np.load(os.path.join(H.GOLD, "rotation_track.npz"))


@pytest.mark.parametrize("case", rc.golden_cases(), ids=lambda c: c.name)
def test_the_fixture_is_the_oracle_s_chain_of_the_plan_s_rotations_then_the_frame_s(case):
    """The reference applied Rotation objects in turn; oracle/reference_path.py does the same with the concatenated chain.  On the goldens'
    platform every index and byte is equal; elsewhere the live oracle's last bits are this host's, and the fragile set is the allowance."""
    assert len(GOLD.files) == 56 and len(case.frames) == 4
    dst, src = H.orc_proj(case.dst), H.orc_proj(case.src)
    frames = rc.case_frames(case)
    exact = H.live_numpy_is_the_goldens_numpy()
    for f in range(4):
        rots = [tuple(map(orc.to_radians, r)) for r in case.chain(f)]
        with np.errstate(all="ignore"):
            idx = orc.remap_index(dst, src, rots)
            u8 = orc.remap(dst, src, frames[f], rots)
            fragile = orc.fragile_mask(orc.pretrunc(dst, src, rots))
        got_u8 = GOLD[f"{case.name}/{f}/u8"]
        assert got_u8.dtype == np.uint8 and got_u8.shape == (case.dst[1], case.dst[2], 3)
        pairs = [(GOLD[f"{case.name}/{f}/idx_l"], idx[0]), (GOLD[f"{case.name}/{f}/idx_r"], idx[1])] if case.src[0] == "double" else [(GOLD[f"{case.name}/{f}/idx"], idx)]
        bad = (got_u8 != u8).any(axis=2)
        for got, want in pairs:
            assert got.dtype == np.int32 and got.shape == want.shape
            bad |= got != want
        assert int((bad & ~fragile).sum()) == 0, (case.name, f, int(bad.sum()))
        if exact:
            assert int(bad.sum()) == 0, (case.name, f, int(bad.sum()))


# ---- Plan.remap_track and batch.remap_frames(rotations=...) against stand-ins --------------------------------------------------------
class FakeTrackLib(FakePipeLib):
    """tests/test_host_memory.py's stand-in with the track launch: it records its arguments and the table it finds behind the pointer."""

    def __init__(self):
        super().__init__()
        self.calls = []

    def pb_remap_track_u8(self, plan, table, k, interp, src, dst, n, ss, ds, stream):
        mats = np.frombuffer((ctypes.c_double * (9 * int(k) * int(n))).from_address(int(table)), np.float64).reshape(int(n), int(k), 3, 3).copy()
        self.calls.append({"table": int(table), "k": int(k), "interp": int(interp), "src": int(src), "dst": int(dst), "n": int(n), "ss": int(ss), "ds": int(ds),
                           "stream": int(stream or 0), "mats": mats})
        return 0


@pytest.fixture
def env(monkeypatch):
    p = nat.make_proj(nat.KIND_PANO, 4, 8)
    plans = {n_rot: nat.Plan(p, [np.eye(3)] * n_rot, p, defer=True) for n_rot in (0, 7)}  # (made by the real library, before the stand-in takes over)
    lib = FakeTrackLib()
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


def test_plan_remap_track_checks_shapes_dtypes_and_counts_before_any_device_work(env):
    lib, plans = env
    plan = plans[0]
    src = _device.DeviceArray((3, 4, 8, 3), np.uint8)
    mats = rotation_track(np.arange(9.0).reshape(3, 3))
    bad_calls = [
        (nat.PbError, dict(src=np.zeros((3, 4, 8, 3), np.uint8), rotations=mats)),                   # not a device array
        (nat.PbError, dict(src=_device.DeviceArray((4, 8, 3), np.uint8), rotations=mats)),           # not a batch
        (nat.PbError, dict(src=_device.DeviceArray((3, 4, 7, 3), np.uint8), rotations=mats)),        # not the plan's source
        (nat.PbError, dict(src=_device.DeviceArray((3, 4, 8, 3), np.uint16), rotations=mats)),       # not uint8
        (ValueError, dict(src=src, rotations=mats[:2])),                                              # two rotations for three frames
        (ValueError, dict(src=src, rotations=mats.astype(np.float32))),
        (ValueError, dict(src=src, rotations=_device.DeviceArray((3, 3, 3), np.float32))),
        (ValueError, dict(src=src, rotations=np.zeros((3, 9)))),
        (ValueError, dict(src=src, rotations=np.zeros((3, 9, 3, 3)))),                               # nine rotations per frame
        (ValueError, dict(src=src, rotations=mats, interpolation="cubic")),
        (nat.PbError, dict(src=src, rotations=mats, out=_device.DeviceArray((3, 4, 8, 4), np.uint8))),
        (nat.PbError, dict(src=src, rotations=mats, out=np.zeros((3, 4, 8, 3), np.uint8))),
    ]
    for exc, kw in bad_calls:
        with pytest.raises(exc):
            plan.remap_track(**kw)
    with pytest.raises(ValueError, match="PB_MAX_ROTATIONS"):
        plans[7].remap_track(src, np.zeros((3, 2, 3, 3)))
    assert lib.calls == [] and not lib.log, "a refused call reached the library"


def test_plan_remap_track_uploads_an_ndarray_and_uses_a_device_table_in_place(env):
    lib, plans = env
    plan = plans[0]
    src = _device.DeviceArray((3, 4, 8, 3), np.uint8)
    mats = rotation_track(np.arange(18.0).reshape(6, 3)).reshape(3, 2, 3, 3)
    out = plan.remap_track(src, mats, interpolation="catmull-rom", stream=0x77)
    assert isinstance(out, _device.DeviceArray) and out.shape == (3, 4, 8, 3) and out.dtype == np.uint8
    c = lib.calls[-1]
    assert (c["k"], c["interp"], c["src"], c["dst"], c["n"], c["ss"], c["ds"], c["stream"]) == (2, 2, src.data_ptr(), out.data_ptr(), 3, 0, 0, 0x77)
    assert np.array_equal(H.bits(c["mats"]), H.bits(mats)) and [k for k, _ in lib.log].count("h2d") == 1
    # Rotation objects, one per frame, into a caller's output
    rots = [pb.Rotation(0.1, 0.2 * f, -0.3) for f in range(3)]
    mine = _device.DeviceArray((3, 4, 8, 3), np.uint8)
    assert plan.remap_track(src, rots, out=mine, interpolation="bilinear") is mine
    c = lib.calls[-1]
    assert (c["k"], c["interp"], c["dst"], c["stream"]) == (1, 1, mine.data_ptr(), 0)
    assert all(np.array_equal(H.bits(c["mats"][f, 0]), H.bits(rots[f].rotation_matrix)) for f in range(3))
    # a float64 device array: the very pointer, no copy
    tab = _device.DeviceArray((3, 3, 3), np.float64).copy_from_host(mats[:, 0])
    copies = [k for k, _ in lib.log].count("h2d")
    plans[7].remap_track(src, tab)
    c = lib.calls[-1]
    assert c["table"] == tab.data_ptr() and (c["k"], c["interp"], c["n"]) == (1, 0, 3) and [k for k, _ in lib.log].count("h2d") == copies
    # no frames: nothing is launched
    n_calls = len(lib.calls)
    assert plan.remap_track(_device.DeviceArray((0, 4, 8, 3), np.uint8), np.empty((0, 3, 3))).shape == (0, 4, 8, 3) and len(lib.calls) == n_calls


@pytest.mark.parametrize("k", [1, 2])
def test_remap_frames_points_launch_f_at_entry_f_of_a_table_uploaded_once(env, k):
    lib, plans = env
    plan = plans[0]
    n = 5
    mats = rotation_track(np.random.default_rng(k).uniform(-3, 3, (n * k, 3))).reshape(n, k, 3, 3)
    frames = [np.full((4, 8, 3), f, np.uint8) for f in range(n)]
    # an ndarray: uploaded once, before the first frame's upload
    outs = list(batch.remap_frames(plan, frames, depth=2, interpolation="bilinear", rotations=mats if k == 2 else mats[:, 0]))
    assert len(outs) == n and all(o.shape == (4, 8, 3) and o.dtype == np.uint8 for o in outs)
    assert len(lib.calls) == n and lib.log[0][0] == "h2d" and [e[0] for e in lib.log].count("h2d") == 1 + n
    base = lib.calls[0]["table"]
    for f, c in enumerate(lib.calls):
        assert c["table"] == base + f * k * 72 and (c["k"], c["n"], c["interp"], c["ss"], c["ds"]) == (k, 1, 1, 0, 0), (f, c)
        assert np.array_equal(H.bits(c["mats"][0]), H.bits(mats[f]))
    assert len({c["stream"] for c in lib.calls}) == 1 and lib.calls[0]["stream"] != 0
    # a device table: used in place
    del lib.calls[:]
    tab = _device.DeviceArray((n, k, 3, 3), np.float64).copy_from_host(mats)
    assert len(list(batch.remap_frames(plan, iter(frames), rotations=tab))) == n
    assert [c["table"] for c in lib.calls] == [tab.data_ptr() + f * k * 72 for f in range(n)] and all(c["interp"] == 0 for c in lib.calls)


def test_remap_frames_refuses_a_frame_beyond_the_table_at_that_frame_and_supersampling_at_once(env):
    lib, plans = env
    plan = plans[0]
    frames = [np.full((4, 8, 3), f, np.uint8) for f in range(4)]
    gen = batch.remap_frames(plan, frames, depth=2, rotations=[pb.Rotation(0, 0.1 * f, 0) for f in range(3)])
    with pytest.raises(ValueError, match="frame 3 has no rotation: the table holds 3"):
        list(gen)
    assert len(lib.calls) == 3  # the three frames the table covers were launched
    for bad in (dict(supersample=2), dict(supersample=4, interpolation="bilinear")):
        with pytest.raises(ValueError):  # (before the generator is made: nothing to iterate)
            batch.remap_frames(plan, frames, rotations=np.zeros((4, 3, 3)), **bad)
    with pytest.raises(ValueError):
        batch.remap_frames(plan, frames, rotations=np.zeros((4, 3, 3), np.float32))
    with pytest.raises(ValueError, match="PB_MAX_ROTATIONS"):
        batch.remap_frames(plans[7], frames, rotations=np.zeros((4, 2, 3, 3)))
    with pytest.raises(ValueError):  # a grey frame with a track
        list(batch.remap_frames(plan, [np.zeros((4, 8), np.uint8)], rotations=np.zeros((1, 3, 3))))
    # rotations=None: the plain launch, as before
    del lib.calls[:]
    assert batch.remap_frames.__defaults__[-1] is None
