"""CPU-only checks of the NV12 / P010 remap (pb_remap_nv12): the definition on a hand-written example, the header and the
library's exports, the argument checks that come before any device is looked at, the host pipeline's ``pixel_format`` keyword over the
stand-ins of tests/test_host_memory.py, and the ``utils`` helpers.  A deferred plan has no device and every library call here fails its
checks: none could start a launch."""

import ctypes as C
import os
import re

import numpy as np
import pytest

import photonbend_amd as pb
from photonbend_amd import _native as nat
from photonbend_amd import batch
from tests import nv12_ref
from tests.test_host_memory import FakePlan, pipe_env  # noqa: F401  (the stand-ins of the streaming pipeline's tests)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x1000  # a non-null "device pointer" for calls that must be refused before anything reads it
INVALID, UNSUPPORTED = -1, -3


# ---- the definition ---------------------------------------------------------------------------------------------------------------------
HAND_IDX = np.array([[5, -1, -1, 3],
                     [-1, -1, 7, 7],
                     [-1, 10, 15, -1],
                     [2, 2, -1, -1]], np.int32)


@pytest.mark.parametrize("dt", [np.uint8, np.uint16])
def test_the_definition_on_a_hand_written_example(dt):
    """4 x 4 <- 4 x 4.  Block (0, 0): the anchor is valid and the other three pixels are black - it keeps its chroma.  Blocks (0, 1) and
    (1, 0): the anchor is black and other pixels are valid - the pair is the fill.  Block (1, 1): the anchor samples the source's last
    pixel, so the source's last pair."""
    y = (np.arange(16).reshape(4, 4) + 100).astype(dt)
    uv = np.array([[[1, 2], [3, 4]], [[5, 6], [7, 8]]], dt)
    yo, uvo = nv12_ref.remap_nv12(y, uv, HAND_IDX, 4, (9, 8, 7))
    assert yo.dtype == uvo.dtype == np.dtype(dt)
    assert yo.tolist() == [[105, 9, 9, 103], [9, 9, 107, 107], [9, 110, 115, 9], [102, 102, 9, 9]]
    assert uvo.tolist() == [[[1, 2], [8, 7]], [[8, 7], [7, 8]]]
    # the packed form and the default fill: video black in the sample type
    fy, fu, fv = nv12_ref.default_fill(dt)
    assert (fy, fu, fv) == ((16, 128, 128) if dt == np.uint8 else (16 << 8, 128 << 8, 128 << 8))
    packed = nv12_ref.remap_frame(pb.utils.nv12_frame(y, uv), HAND_IDX, 4, 4)
    assert packed.shape == (6, 4) and packed.dtype == np.dtype(dt)
    assert packed[:4].tolist() == np.where(HAND_IDX < 0, fy, yo).tolist()
    assert packed[4:].tolist() == [[1, 2, fu, fv], [fu, fv, 7, 8]]


def test_a_different_source_width_and_a_magnifying_map():
    """8 x 4 <- 2 x 6: r = idx // w with the SOURCE width; blocks whose anchors fall on one source block share its pair."""
    y = np.arange(12, dtype=np.uint8).reshape(2, 6)
    uv = np.array([[[10, 11], [20, 21], [30, 31]]], np.uint8)
    idx = np.array([[0, 1, 2, 3], [6, 7, 8, 9], [4, 5, 10, 11], [-1, 0, 0, -1]] * 2, np.int32)
    yo, uvo = nv12_ref.remap_nv12(y, uv, idx, 6, (0, 1, 2))
    assert yo[2].tolist() == [4, 5, 10, 11] and yo[3].tolist() == [0, 0, 0, 0]
    assert uvo.tolist() == [[[10, 11], [20, 21]], [[30, 31], [30, 31]]] * 2


# ---- the C ABI --------------------------------------------------------------------------------------------------------------------------
def test_the_header_declares_both_functions_and_the_struct_and_the_library_exports_them():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "photonbend_hip.h")).read(), flags=re.S)
    decl = {m.group(1): " ".join(m.group(2).split()) for m in re.finditer(r"\bint (pb_remap_nv12\w*)\s*\(([^)]*)\)\s*;", text)}
    assert decl == {
        "pb_remap_nv12": "const pb_plan* plan, const void* src_dev, void* dst_dev, int n_frames, const pb_nv12_layout* src_layout, "
                         "const pb_nv12_layout* dst_layout, int bytes_per_sample, const uint16_t fill_yuv[3], void* stream",
        "pb_remap_nv12_supported": "const pb_plan* plan, int bytes_per_sample",
    }
    assert re.search(r"typedef struct pb_nv12_layout \{ size_t pitch, uv_offset, frame_stride; \} pb_nv12_layout;", text)
    vp = C.c_void_p
    assert nat.SIGNATURES["pb_remap_nv12"] == (C.c_int, [vp, vp, vp, C.c_int, vp, vp, C.c_int, vp, vp])
    assert nat.SIGNATURES["pb_remap_nv12_supported"] == (C.c_int, [vp, C.c_int])
    assert [f[0] for f in nat.pb_nv12_layout._fields_] == ["pitch", "uv_offset", "frame_stride"] and C.sizeof(nat.pb_nv12_layout) == 3 * C.sizeof(C.c_size_t)
    lib = nat.load()
    assert hasattr(lib, "pb_remap_nv12") and hasattr(lib, "pb_remap_nv12_supported")
    assert lib.pb_abi_version() == 5  # additive


def _deferred(h, w, H=None, W=None):
    lib = nat.load()
    handle = C.c_void_p()
    src, dst = nat.make_proj(nat.KIND_PANO, h, w), nat.make_proj(nat.KIND_PANO, H or h, W or w)
    assert lib.pb_plan_create_ex(C.byref(dst), None, 0, C.byref(src), nat.PLAN_DEFER, 0, C.byref(handle)) == 0
    return lib, handle


def _call(lib, plan, S=1, src=FAKE, dst=FAKE, n=1, sl=None, dl=None, fill=None):
    sl = None if sl is None else nat.pb_nv12_layout(*sl)
    dl = None if dl is None else nat.pb_nv12_layout(*dl)
    rc = lib.pb_remap_nv12(plan, src, dst, n, None if sl is None else C.addressof(sl), None if dl is None else C.addressof(dl), S,
                           None if fill is None else C.addressof((C.c_uint16 * 3)(*fill)), None)
    return rc, lib.pb_last_error()


def test_argument_checks_come_before_any_device_and_say_what_is_wrong():
    lib, plan = _deferred(4, 8, 6, 12)  # source 4 x 8, destination 6 x 12
    try:
        assert _call(lib, None) == (INVALID, b"null argument")
        assert _call(lib, plan, src=None) == (INVALID, b"null argument") and _call(lib, plan, dst=None) == (INVALID, b"null argument")
        assert _call(lib, plan, n=-1) == (INVALID, b"negative frame count")
        for S in (-1, 0, 3, 4, 8):
            rc, msg = _call(lib, plan, S)
            assert rc == INVALID and b"bytes_per_sample" in msg, (S, msg)
            assert lib.pb_remap_nv12_supported(plan, S) == INVALID and b"bytes_per_sample" in lib.pb_last_error()
        assert lib.pb_remap_nv12_supported(None, 1) == INVALID and lib.pb_last_error() == b"null argument"
        for S in (1, 2):
            ok_s, ok_d = (S * 8, S * 8 * 4, S * 8 * 6), (S * 12, S * 12 * 6, S * 12 * 9)  # the packed defaults, spelled out
            # the defaults and their spelled-out form pass every argument check: what is left is the plan (deferred)
            for sl, dl in ((None, None), (ok_s, ok_d), ((0, 0, 0), (0, 0, 0)), ((S * 8 + 2 * S, 0, 0), (256, 256 * 9, 256 * 16))):
                rc, msg = _call(lib, plan, S, sl=sl, dl=dl)
                assert rc == UNSUPPORTED and b"pb_index_map_i32" in msg, (S, sl, dl, msg)
            assert lib.pb_remap_nv12_supported(plan, S) == 0
            assert _call(lib, plan, S, n=0)[0] == 0  # no frames: nothing to launch
            # each rule broken by one pair, on either side
            for which in ("sl", "dl"):
                base = ok_s if which == "sl" else ok_d
                name = b"source" if which == "sl" else b"destination"
                for broken, rule in (((base[0] - 2 * S, 0, 0), b"pitch smaller than a row"),
                                     ((0, base[1] - 2 * S, 0), b"uv_offset smaller than the luma plane"),
                                     ((base[0] + 2 * S, base[1], 0), b"uv_offset smaller than the luma plane"),  # (the pitched plane is larger)
                                     ((0, 0, base[2] - 2 * S), b"frame_stride smaller than a frame"),
                                     ((0, base[1] + 2 * S, base[2]), b"frame_stride smaller than a frame")):
                    rc, msg = _call(lib, plan, S, **{which: broken})
                    assert rc == INVALID and name in msg and rule in msg, (S, which, broken, msg)
                # ... and by one sample: not a multiple of one pair
                for broken in ((base[0] + S, 0, 0), (0, base[1] + S, 0), (0, 0, base[2] + S), (base[0] + 2 * S + 1, 0, 0)):
                    rc, msg = _call(lib, plan, S, **{which: broken})
                    assert rc == INVALID and b"multiples of" in msg and name in msg, (S, which, broken, msg)
            # a pitch or an offset no frame below 2^31 bytes can have - wrapping products included - is refused before anything is multiplied
            for which in ("sl", "dl"):
                for huge in (((1 << 63) + (1 << 20), 0, 0), (1 << 31, 0, 0), (0, 1 << 31, 0), (0, (1 << 64) - 2 * S, 0)):
                    rc, msg = _call(lib, plan, S, **{which: huge})
                    assert rc == UNSUPPORTED and b"2^31" in msg, (S, which, huge, msg)
            for kw in ({"src": FAKE + S}, {"dst": FAKE + S}, {"src": FAKE + 1}):
                rc, msg = _call(lib, plan, S, **kw)
                assert rc == INVALID and b"multiples of" in msg, (S, kw, msg)
    finally:
        lib.pb_plan_destroy(plan)


@pytest.mark.parametrize("dims", [(5, 8, 4, 8), (4, 7, 4, 8), (4, 8, 3, 8), (4, 8, 4, 9)])
def test_an_odd_dimension_is_invalid(dims):
    lib, plan = _deferred(*dims)
    try:
        for S in (1, 2):
            rc, msg = _call(lib, plan, S)
            assert rc == INVALID and b"even" in msg, (dims, S, msg)
            assert lib.pb_remap_nv12_supported(plan, S) == INVALID and b"even" in lib.pb_last_error()
    finally:
        lib.pb_plan_destroy(plan)


def test_plan_remap_nv12_checks_its_arguments_without_a_gpu():
    p = nat.make_proj(nat.KIND_PANO, 4, 8)
    plan = nat.Plan(p, [], p, defer=True)
    assert not plan.nv12_supported() and not plan.nv12_supported(2)
    with pytest.raises(nat.PbError, match="bytes_per_sample"):
        plan.nv12_supported(3)
    with pytest.raises(nat.PbError, match="device arrays"):
        plan.remap_nv12(np.zeros((6, 8), np.uint8))
    with pytest.raises(nat.PbError, match="pb_index_map_i32"):  # (the raw call: refused by the library, a deferred plan)
        plan.launch_nv12(FAKE, FAKE, 1, 0)
    assert nat.nv12_layout(None) is None
    l = nat.nv12_layout((256, 1024, 0))
    assert (l.pitch, l.uv_offset, l.frame_stride) == (256, 1024, 0) and nat.nv12_layout(l) is l
    l = nat.nv12_layout({"pitch": 64})
    assert (l.pitch, l.uv_offset, l.frame_stride) == (64, 0, 0)
    with pytest.raises(ValueError):
        nat.nv12_layout({"pich": 64})
    assert nat.nv12_frame_bytes(None, 4, 8, 2) == (96, 96) and nat.nv12_frame_bytes(nat.nv12_layout((32, 160, 512)), 4, 8, 2) == (224, 512)
    odd = nat.Plan(nat.make_proj(nat.KIND_PANO, 3, 8), [], p, defer=True)
    with pytest.raises(nat.PbError, match="even"):
        odd.nv12_supported()


# ---- the host pipeline ------------------------------------------------------------------------------------------------------------------
def test_remap_frames_without_a_pixel_format_is_what_it_was(pipe_env):  # noqa: F811
    """tests/test_host_memory.py's stand-ins, whose ``launch`` takes exactly the arguments of before: pixel_format=None adds nothing."""
    lib, hp = pipe_env
    rng = np.random.default_rng(7)
    frames = [rng.integers(0, 256, (24, 40, 3), dtype=np.uint8) for _ in range(4)]
    plan = FakePlan(24, 40, lib)
    outs = list(hp.remap_frames(plan, iter(frames), depth=3, pixel_format=None))
    assert len(outs) == 4 and plan.launches == [(plan.launches[0][0], "nearest")] * 4
    assert all(o.dtype == np.uint8 and np.array_equal(o, f[::-1]) for f, o in zip(frames, outs))
    one = hp.remap_ndarray(plan, frames[0], pixel_format=None)
    assert np.array_equal(one, frames[0][::-1])
    assert list(batch.remap_frames(plan, [], pixel_format=None)) == []
    del outs, one


class FakeVideoPlan(FakePlan):
    """... with the NV12 launch: 'remaps' a (3h/2, w) frame by flipping it upside down, and records the sample size."""

    def launch_nv12(self, src_ptr, dst_ptr, n_frames, stream, bytes_per_sample):
        n = self.src.height * 3 // 2 * self.src.width * bytes_per_sample
        a = np.frombuffer((C.c_ubyte * n).from_address(src_ptr), np.uint8).reshape(self.src.height * 3 // 2, -1)
        np.frombuffer((C.c_ubyte * n).from_address(dst_ptr), np.uint8).reshape(a.shape)[...] = a[::-1]
        self.launches.append((int(stream), "nv12", bytes_per_sample))
        self.lib.log.append(("run", int(stream)))


@pytest.mark.parametrize("fmt,dt", [("nv12", np.uint8), ("p010", np.uint16)])
def test_video_frames_take_the_same_pipeline(pipe_env, fmt, dt):  # noqa: F811
    lib, hp = pipe_env
    rng = np.random.default_rng(11)
    frames = [rng.integers(0, 256, (36, 40)).astype(dt) for _ in range(3)]
    plan = FakeVideoPlan(24, 40, lib)
    outs = list(hp.remap_frames(plan, frames, pixel_format=fmt))
    assert [l[1:] for l in plan.launches] == [("nv12", np.dtype(dt).itemsize)] * 3
    assert all(o.dtype == np.dtype(dt) and o.shape == (36, 40) and np.array_equal(o, f[::-1]) for f, o in zip(frames, outs))
    streams = {kind: {s for k, s in lib.log if k == kind} for kind in ("h2d", "run", "d2h")}
    assert len(streams["h2d"]) == 1 and len(streams["run"]) == 1 and streams["h2d"] != streams["run"] and not streams["d2h"]
    one = hp.remap_ndarray(plan, frames[1], pixel_format=fmt)
    assert one.dtype == np.dtype(dt) and np.array_equal(one, frames[1][::-1])
    # what is not such a frame, or not such a call, is a ValueError - before anything is launched
    n = len(plan.launches)
    for bad in (frames[0][:-1], frames[0].astype(np.float32), np.zeros((24, 40, 3), dt), frames[0].astype(np.uint16 if dt == np.uint8 else np.uint8)):
        with pytest.raises(ValueError):
            hp.remap_ndarray(plan, bad, pixel_format=fmt)
    with pytest.raises(ValueError):
        list(hp.remap_frames(plan, [frames[0], frames[0][:, :-2]], pixel_format=fmt))
    for kw in ({"interpolation": "bilinear"}, {"supersample": 2}, {"rotations": np.eye(3)[None]}):
        with pytest.raises(ValueError):
            batch.remap_frames(plan, frames, pixel_format=fmt, **kw)
    with pytest.raises(ValueError, match="pixel_format"):
        batch.remap_frames(plan, frames, pixel_format="i420")
    with pytest.raises(ValueError, match="pixel_format"):
        hp.remap_ndarray(plan, frames[0], pixel_format="yuv")
    with pytest.raises(ValueError, match="even"):
        hp.remap_ndarray(FakeVideoPlan(25, 40, lib), frames[0], pixel_format=fmt)
    assert len(plan.launches) == n + 1  # (the two-frame call above ran its first frame)
    del outs, one


# ---- utils ------------------------------------------------------------------------------------------------------------------------------
def test_the_plane_helpers_are_views_and_inverse_to_each_other():
    assert "nv12_planes" in pb.utils.__all__ and "nv12_frame" in pb.utils.__all__
    for dt in (np.uint8, np.uint16):
        frame = np.arange(6 * 8).reshape(6, 8).astype(dt)
        y, uv = pb.utils.nv12_planes(frame)
        assert y.shape == (4, 8) and uv.shape == (2, 4, 2) and y.base is not None and np.shares_memory(y, frame) and np.shares_memory(uv, frame)
        assert uv[1, 2].tolist() == [frame[5, 4], frame[5, 5]]  # the (U, V) pair of block (1, 2)
        back = pb.utils.nv12_frame(y, uv)
        assert back.dtype == frame.dtype and np.array_equal(back, frame) and not np.shares_memory(back, frame)
    for bad in ((5, 8), (6, 7), (6, 8, 1), (6,)):
        with pytest.raises(ValueError):
            pb.utils.nv12_planes(np.zeros(bad, np.uint8))
    with pytest.raises(ValueError):
        pb.utils.nv12_frame(np.zeros((4, 8), np.uint8), np.zeros((2, 4, 2), np.uint16))
    with pytest.raises(ValueError):
        pb.utils.nv12_frame(np.zeros((4, 8), np.uint8), np.zeros((2, 8), np.uint8))
