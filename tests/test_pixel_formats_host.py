"""CPU-only checks of pb_remap_px / pb_remap_px_supported: the symbols and their signatures, pb_remap_u8's argument checks
and messages, the pixel sizes, and the shape / dtype checks of Plan.remap_px.  A deferred plan has no device and every call here fails
its checks: none could start a launch."""

import ctypes
import os
import re

import numpy as np
import pytest

from photonbend_amd import _hostpipe
from photonbend_amd import _native as nat

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x1000  # a non-null "device pointer" for calls that must be refused before anything reads it


@pytest.fixture
def deferred():
    lib = nat.load()
    h = ctypes.c_void_p()
    p = nat.make_proj(nat.KIND_PANO, 4, 8)
    assert lib.pb_plan_create_ex(ctypes.byref(p), None, 0, ctypes.byref(p), nat.PLAN_DEFER, 0, ctypes.byref(h)) == 0
    yield lib, h
    lib.pb_plan_destroy(h)


def test_the_two_symbols_exist_with_the_declared_signatures():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "photonbend_hip.h")).read(), flags=re.S)
    decl = {m.group(1): " ".join(m.group(2).split()) for m in re.finditer(r"\bint (pb_remap_px\w*)\s*\(([^)]*)\)\s*;", text)}
    assert decl == {
        "pb_remap_px": "const pb_plan* plan, const void* src_dev, void* dst_dev, int n_frames, size_t src_frame_stride, size_t dst_frame_stride, "
                       "int bytes_per_px, void* stream",
        "pb_remap_px_supported": "const pb_plan* plan, int bytes_per_px",
    }
    vp, C = ctypes.c_void_p, ctypes
    assert nat.SIGNATURES["pb_remap_px"] == (C.c_int, [vp, vp, vp, C.c_int, C.c_size_t, C.c_size_t, C.c_int, vp])
    assert nat.SIGNATURES["pb_remap_px_supported"] == (C.c_int, [vp, C.c_int])
    lib = nat.load()
    assert hasattr(lib, "pb_remap_px") and hasattr(lib, "pb_remap_px_supported")
    assert lib.pb_abi_version() == 5  # additive


def test_argument_checks_and_messages_are_pb_remap_u8s(deferred):
    lib, h = deferred
    for B in nat.PX_SIZES:
        for args in ((h, None, None, 1), (h, None, FAKE, 1), (h, FAKE, None, 3), (h, None, None, 0), (h, None, None, -1), (None, None, None, -1),
                     (None, FAKE, FAKE, 1), (h, FAKE, FAKE, -1), (h, FAKE, FAKE, -7)):
            want = lib.pb_remap_u8(*args, 0, 0, None), lib.pb_last_error()
            got = lib.pb_remap_px(*args, 0, 0, B, None), lib.pb_last_error()
            assert got == want and got[0] == -1, (B, args, got, want)
            assert got[1] in (b"null argument", b"negative frame count")
        # no frames: nothing to launch
        assert lib.pb_remap_px(h, FAKE, FAKE, 0, 0, 0, B, None) == lib.pb_remap_u8(h, FAKE, FAKE, 0, 0, 0, None) == 0


def test_pixel_sizes(deferred):
    lib, h = deferred
    assert nat.PX_SIZES == (1, 2, 3, 4, 6, 8)
    for B in (-1, 0, 5, 7, 9, 12, 16, 64):
        assert lib.pb_remap_px(h, FAKE, FAKE, 1, 0, 0, B, None) == -1 and b"bytes_per_px" in lib.pb_last_error(), B
        assert lib.pb_remap_px_supported(h, B) == -1 and b"bytes_per_px" in lib.pb_last_error(), B
    assert lib.pb_remap_px_supported(None, 4) == -1 and lib.pb_last_error() == b"null argument"
    # a deferred plan: pb_remap_u8 takes it (three-byte pixels), the tile kernel of the other sizes does not - and says where to go
    for B in nat.PX_SIZES:
        assert lib.pb_remap_px_supported(h, B) == (1 if B == 3 else 0), B
        if B != 3:
            a = nat.px_align(B)
            assert a == min(4, B & -B)
            assert lib.pb_remap_px(h, FAKE, FAKE, 1, 0, 0, B, None) == -3, B
            msg = lib.pb_last_error()
            assert b"pb_index_map_i32" in msg and b"pb_gather_px" in msg, msg
            if a > 1:  # alignment is an argument error, reported before the plan is looked at
                for args in ((FAKE + 1, FAKE, 0, 0), (FAKE, FAKE + a // 2, 0, 0), (FAKE, FAKE, 4 * 8 * B + 1, 0), (FAKE, FAKE, 0, 4 * 8 * B + a // 2)):
                    assert lib.pb_remap_px(h, args[0], args[1], 1, args[2], args[3], B, None) == -1, (B, args)
                    assert b"multiples of" in lib.pb_last_error()
            assert lib.pb_remap_px(h, FAKE, FAKE, 1, 0, 4 * 8 * B - a, B, None) == -1 and lib.pb_last_error() == b"dst_frame_stride smaller than a frame"
            assert lib.pb_remap_px(h, FAKE, FAKE, 2, 4 * 8 * B - a, 0, B, None) == -1 and lib.pb_last_error() == b"src_frame_stride smaller than a frame"


def test_plan_remap_px_checks_shape_and_dtype_without_a_gpu():
    p = nat.make_proj(nat.KIND_PANO, 4, 8)
    plan = nat.Plan(p, [], p, defer=True)
    assert plan.px_supported(3) and not any(plan.px_supported(B) for B in (1, 2, 4, 6, 8))
    with pytest.raises(nat.PbError, match="bytes_per_px"):
        plan.px_supported(5)
    with pytest.raises(nat.PbError, match="device arrays"):
        plan.remap_px(np.zeros((4, 8, 4), np.uint8))
    with pytest.raises(ValueError):
        plan.launch(FAKE, FAKE, 1, None, "bilinear", bytes_per_px=4)
    with pytest.raises(ValueError):
        plan.launch(FAKE, FAKE, 1, None, "nearest", supersample=2, bytes_per_px=4)
    # which arrays are frames of a plan, and their pixel size
    hw = (4, 8)
    for shape, dt, want in (((4, 8), np.uint8, 1), ((4, 8), np.uint16, 2), ((4, 8, 2), np.uint8, 2), ((4, 8, 4), np.uint8, 4), ((4, 8, 3), np.uint16, 6),
                            ((4, 8, 4), np.uint16, 8), ((5, 4, 8, 4), np.uint8, 4), ((5, 4, 8), np.uint16, 2), ((4, 8, 3), np.float32, 12),
                            ((4, 8, 2, 2), np.uint8, 4), ((4, 7, 4), np.uint8, 0), ((8, 4), np.uint8, 0), ((4,), np.uint8, 0)):
        assert nat.pixel_bytes(shape, dt, hw) == want, (shape, dt)
    # the host pipe's format rule: uint8 RGB for every mode, the other pixel sizes for nearest without supersampling
    assert _hostpipe._px_format(plan, np.zeros((4, 8, 3), np.uint8), "bilinear", 2) == ((3,), np.uint8, 3)
    assert _hostpipe._px_format(plan, np.zeros((4, 8), np.uint16), "nearest", 1) == ((), np.uint16, 2)
    assert _hostpipe._px_format(plan, np.zeros((4, 8, 4), np.uint16), "nearest", 1) == ((4,), np.uint16, 8)
    for frame, interp, ss in ((np.zeros((4, 8, 4), np.uint8), "bilinear", 1), (np.zeros((4, 8, 4), np.uint8), "nearest", 2),
                              (np.zeros((4, 8, 3), np.float32), "nearest", 1), (np.zeros((4, 7, 3), np.uint8), "nearest", 1)):
        with pytest.raises(ValueError):
            _hostpipe._px_format(plan, frame, interp, ss)
