"""ctypes binding of include/photonbend_hip.h (the C ABI of the HIP library).

There is no fallback: if ``libphotonbend_hip.so`` is missing or a call fails,
this module raises.

PyTorch is OPTIONAL.  The reference needs numpy / Pillow / click (pyproject.toml:9-14) and so does this package: device memory,
streams and page-locked host memory come from the library itself (``_device.py`` over pb_malloc / pb_memcpy_* / pb_stream_* /
pb_host_*).  Where torch IS installed it is imported FIRST, on purpose - it ships its own ``libamdhip64.so`` (SONAME
libamdhip64.so.7); loading it before our library makes both share one HIP runtime, so torch device pointers and streams can be
handed straight to the kernels - and CUDA tensors are accepted wherever a device array is (frames that stay on the device).
"""

from __future__ import annotations

import contextlib
import ctypes as C
import os
import threading
import typing

import numpy as np

try:  # must precede the CDLL below - see module docstring
    import torch
except ImportError:  # the NumPy workflow needs no torch
    torch = None

from ._device import DeviceArray
from . import build as _build
from .build import host_math_flavour  # (the build picks the diagnostic library's flavour by it too)

MATH_FLAVOUR = host_math_flavour()
# PB_LIB_PATH: another build of the same sources (A/B experiments, the diagnostic build); else the product library of the host's flavour
LIB_PATH = os.environ.get("PB_LIB_PATH") or (_build.LIBM_LIB_PATH if MATH_FLAVOUR == "libm" else _build.LIB_PATH)

ABI_VERSION = 5
PB_MAX_ROTATIONS = 8
PLAN_DEFER, PLAN_TUNE, PLAN_MATH_SVML, PLAN_MATH_LIBM, PLAN_NO_BILINEAR, PLAN_BILINEAR = 1, 2, 4, 8, 16, 32
MODE_AUTO, MODE_FAITHFUL, MODE_FAST, MODE_FAST_DIRECT = 0, 1, 2, 3
INTERP_IDS = {"nearest": 0, "bilinear": 1}
INTERPOLATIONS = ("nearest", "bilinear", "catmull-rom")  # every mode a plain remap takes (INTERP_IDS: the supersampled ABI's ids)
SS_GENERIC = 1  # pb_remap_ss_u8: force the generic path (tests, A/B measurement)
SUPERSAMPLE_FACTORS = (1, 2, 4)
# the largest map any pb_proj may describe (photonbend_hip.hip, pb_end_ok): h * w <= (2^31 - 1) / 4
MAX_PROJ_PIXELS = 0x7FFFFFFF // 4
KIND_CAMERA, KIND_DOUBLE, KIND_PANO = 0, 1, 2
KIND_CUBE = 5  # a cube map (2N, 3N): no lens, like a panorama (3 and 4 are the library's own eye kinds)
KIND_EAC = 8  # an equi-angular cube map: the cube's frame and shape rule, face positions proportional to the angle
LENSLESS_KINDS = (KIND_PANO, KIND_CUBE, KIND_EAC)  # their pb_proj.lens / fov / magnitude / f_distance are ignored
LENS_IDS = {
    "equidistant": 0,
    "equisolid": 1,
    "rectilinear": 2,
    "stereographic": 3,
    "orthographic": 4,
    "thoby": 5,
}
LENS_CUSTOM = 6  # a Lens of user callables: the host evaluates it (pb_index_from_map_i32's distance planes)
LENS_POLYNOMIAL_BASE = 16  # ids of registered polynomial lenses (pb_lens_polynomial) start here; they are process-local


class PbError(RuntimeError):
    pass


class pb_proj(C.Structure):
    _fields_ = [
        ("kind", C.c_int32),
        ("lens", C.c_int32),
        ("height", C.c_int32),
        ("width", C.c_int32),
        ("fov", C.c_double),
        ("magnitude", C.c_double),
        ("f_distance", C.c_double),
    ]

    def key(self):
        """What identifies this projection in a cache - also one that outlives the process: a registered polynomial lens is named
        by its coefficients, never by its process-local id."""
        lens = self.lens
        if self.kind not in LENSLESS_KINDS and lens >= LENS_POLYNOMIAL_BASE:
            lens = ("polynomial",) + lens_polynomial_info(lens)
        return (self.kind, lens, self.height, self.width, self.fov, self.magnitude, self.f_distance)


# name -> (restype, argtypes); every symbol of include/photonbend_hip.h
_VP = C.c_void_p
SIGNATURES = {
    "pb_abi_version": (C.c_int, []),
    "pb_math_flavour": (C.c_int, []),
    "pb_last_error": (C.c_char_p, []),
    "pb_init": (C.c_int, [C.c_int]),
    "pb_shutdown": (C.c_int, []),
    "pb_device_name": (C.c_int, [C.c_char_p, C.c_size_t]),
    "pb_lens_polynomial": (C.c_int, [C.POINTER(C.c_double), C.c_double, C.POINTER(C.c_int)]),
    "pb_lens_polynomial_info": (C.c_int, [C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "pb_plan_create": (C.c_int, [C.POINTER(pb_proj), C.POINTER(C.c_double), C.c_int, C.POINTER(pb_proj), C.POINTER(_VP)]),
    "pb_plan_create_ex": (C.c_int, [C.POINTER(pb_proj), C.POINTER(C.c_double), C.c_int, C.POINTER(pb_proj), C.c_uint, C.c_int, C.POINTER(_VP)]),
    "pb_plan_prepare": (C.c_int, [_VP, C.c_uint, C.c_int]),
    "pb_plan_set_window_budget": (C.c_int, [_VP, C.c_int]),
    "pb_plan_timing": (C.c_int, [_VP, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "pb_plan_serialize": (C.c_int, [_VP, _VP, C.c_size_t, C.POINTER(C.c_size_t)]),
    "pb_plan_deserialize": (C.c_int, [_VP, C.c_size_t, C.POINTER(_VP)]),
    "pb_plan_destroy": (None, [_VP]),
    "pb_plan_set_mode": (C.c_int, [_VP, C.c_int]),
    "pb_plan_info": (C.c_int, [_VP, C.POINTER(C.c_int), C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]),
    "pb_plan_dst_shape": (C.c_int, [_VP, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "pb_plan_src_shape": (C.c_int, [_VP, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "pb_plan_window_budget": (C.c_int, [_VP]),
    "pb_plan_bilinear_float64_tiles": (C.c_int, [_VP]),
    "pb_plan_bilinear_tile_mix": (C.c_int, [_VP, C.POINTER(C.c_longlong)]),
    "pb_plan_bilinear_launch_shape": (C.c_int, [_VP, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "pb_plan_video_bilinear_mix": (C.c_int, [_VP, C.POINTER(C.c_longlong)]),
    "pb_plan_stitch_tile_mix": (C.c_int, [_VP, C.POINTER(C.c_longlong)]),
    "pb_stitch_nv12": (C.c_int, [_VP, _VP, _VP, C.c_int, _VP, _VP, C.c_int, _VP, _VP]),
    "pb_stitch_nv12_supported": (C.c_int, [_VP, C.c_int]),
    "pb_stitch_planar": (C.c_int, [_VP, _VP, _VP, C.c_int, _VP, _VP, C.c_int, C.c_int, _VP, _VP]),
    "pb_stitch_planar_supported": (C.c_int, [_VP, C.c_int, C.c_int]),
    "pb_plan_matches": (C.c_int, [_VP, C.POINTER(pb_proj), C.POINTER(C.c_double), C.c_int, C.POINTER(pb_proj)]),
    "pb_remap_u8": (C.c_int, [_VP, _VP, _VP, C.c_int, C.c_size_t, C.c_size_t, _VP]),
    "pb_remap_u8v": (C.c_int, [_VP, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_int, _VP]),
    "pb_remap_px": (C.c_int, [_VP, _VP, _VP, C.c_int, C.c_size_t, C.c_size_t, C.c_int, _VP]),
    "pb_remap_px_supported": (C.c_int, [_VP, C.c_int]),
    "pb_remap_nv12": (C.c_int, [_VP, _VP, _VP, C.c_int, _VP, _VP, C.c_int, _VP, _VP]),
    "pb_remap_nv12_supported": (C.c_int, [_VP, C.c_int]),
    "pb_remap_planar": (C.c_int, [_VP, _VP, _VP, C.c_int, _VP, _VP, C.c_int, C.c_int, _VP, _VP]),
    "pb_remap_planar_supported": (C.c_int, [_VP, C.c_int, C.c_int]),
    "pb_remap_planar_bilinear": (C.c_int, [_VP, _VP, _VP, C.c_int, _VP, _VP, C.c_int, C.c_int, _VP, _VP]),
    "pb_remap_nv12_bilinear": (C.c_int, [_VP, _VP, _VP, C.c_int, _VP, _VP, C.c_int, _VP, _VP]),
    "pb_remap_planar_bilinear_supported": (C.c_int, [_VP, C.c_int, C.c_int]),
    "pb_remap_nv12_bilinear_supported": (C.c_int, [_VP, C.c_int]),
    "pb_remap_bilinear_u8": (C.c_int, [_VP, _VP, _VP, C.c_int, C.c_size_t, C.c_size_t, _VP]),
    "pb_remap_catmull_rom_u8": (C.c_int, [_VP, _VP, _VP, C.c_int, C.c_size_t, C.c_size_t, _VP]),
    "pb_remap_track_u8": (C.c_int, [_VP, _VP, C.c_int, C.c_int, _VP, _VP, C.c_int, C.c_size_t, C.c_size_t, _VP]),
    "pb_remap_track_px": (C.c_int, [_VP, _VP, C.c_int, C.c_int, _VP, _VP, C.c_int, C.c_size_t, C.c_size_t, C.c_int, C.c_int, _VP]),
    "pb_remap_track_px_supported": (C.c_int, [_VP, C.c_int, C.c_int]),
    "pb_remap_interp_px": (C.c_int, [_VP, _VP, _VP, C.c_int, C.c_size_t, C.c_size_t, C.c_int, C.c_int, C.c_int, _VP]),
    "pb_remap_interp_px_supported": (C.c_int, [_VP, C.c_int, C.c_int, C.c_int]),
    "pb_remap_interp_pxf": (C.c_int, [_VP, _VP, _VP, C.c_int, C.c_size_t, C.c_size_t, C.c_int, C.c_int, C.c_int, _VP]),
    "pb_remap_interp_pxf_supported": (C.c_int, [_VP, C.c_int, C.c_int, C.c_int]),
    "pb_plan_px_interp_route": (C.c_int, [_VP, C.c_int, C.c_int, C.c_int]),
    "pb_remap_track_nv12": (C.c_int, [_VP, _VP, C.c_int, _VP, _VP, C.c_int, _VP, _VP, C.c_int, _VP, _VP]),
    "pb_remap_track_planar": (C.c_int, [_VP, _VP, C.c_int, _VP, _VP, C.c_int, _VP, _VP, C.c_int, C.c_int, _VP, _VP]),
    "pb_remap_track_nv12_bilinear": (C.c_int, [_VP, _VP, C.c_int, _VP, _VP, C.c_int, _VP, _VP, C.c_int, _VP, _VP]),
    "pb_remap_track_planar_bilinear": (C.c_int, [_VP, _VP, C.c_int, _VP, _VP, C.c_int, _VP, _VP, C.c_int, C.c_int, _VP, _VP]),
    "pb_track_stitch_nv12": (C.c_int, [_VP, _VP, C.c_int, _VP, _VP, C.c_int, _VP, _VP, C.c_int, _VP, _VP]),
    "pb_track_stitch_planar": (C.c_int, [_VP, _VP, C.c_int, _VP, _VP, C.c_int, _VP, _VP, C.c_int, C.c_int, _VP, _VP]),
    "pb_remap_ss_workspace": (C.c_int, [_VP, C.c_int, C.c_int, C.c_uint, C.POINTER(C.c_size_t)]),
    "pb_remap_ss_u8": (C.c_int, [_VP, C.c_int, C.c_int, _VP, _VP, C.c_int, C.c_size_t, C.c_size_t, _VP, C.c_size_t, C.c_uint, _VP]),
    "pb_box_reduce": (C.c_int, [_VP, _VP, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _VP]),
    "pb_index_map_i32": (C.c_int, [_VP, _VP, _VP, _VP]),
    "pb_coordmap_f64": (C.c_int, [C.POINTER(pb_proj), _VP, _VP]),
    "pb_rotate_f64": (C.c_int, [C.POINTER(C.c_double), _VP, _VP, C.c_int, C.c_int, _VP]),
    "pb_sample_map_u8": (C.c_int, [C.POINTER(pb_proj), _VP, C.c_int, C.c_int, _VP, _VP, _VP]),
    "pb_index_from_map_i32": (C.c_int, [C.POINTER(pb_proj), _VP, C.c_int, C.c_int, _VP, _VP, _VP, _VP, _VP]),
    "pb_sample_map_bilinear_px": (C.c_int, [C.POINTER(pb_proj), _VP, C.c_int, C.c_int, _VP, _VP, _VP, _VP, C.c_int, C.c_int, _VP]),
    "pb_sample_map_bilinear_u8": (C.c_int, [C.POINTER(pb_proj), _VP, C.c_int, C.c_int, _VP, _VP, _VP]),
    "pb_sample_map_catmull_rom_px": (C.c_int, [C.POINTER(pb_proj), _VP, C.c_int, C.c_int, _VP, _VP, _VP, _VP, C.c_int, C.c_int, _VP]),
    "pb_gather_px": (C.c_int, [_VP, _VP, _VP, C.c_size_t, C.c_int, _VP]),
    "pb_gather_blend_u8": (C.c_int, [_VP, _VP, _VP, _VP, C.c_size_t, C.c_int, C.c_int, _VP]),
    "pb_map_projection_u8": (C.c_int, [_VP, C.c_int, C.c_int, _VP, _VP, _VP]),
    "pb_synth_frame_u8": (C.c_int, [_VP, C.c_int, C.c_int, C.c_uint32, C.c_uint32, C.c_int, _VP]),
    "pb_malloc": (C.c_int, [C.POINTER(_VP), C.c_size_t]),
    "pb_free": (C.c_int, [_VP]),
    "pb_memcpy_h2d": (C.c_int, [_VP, _VP, C.c_size_t, _VP]),
    "pb_memcpy_d2h": (C.c_int, [_VP, _VP, C.c_size_t, _VP]),
    "pb_memset": (C.c_int, [_VP, C.c_int, C.c_size_t, _VP]),
    "pb_stream_create": (C.c_int, [C.POINTER(_VP)]),
    "pb_stream_destroy": (C.c_int, [_VP]),
    "pb_stream_sync": (C.c_int, [_VP]),
    "pb_event_create": (C.c_int, [C.POINTER(_VP)]),
    "pb_event_destroy": (C.c_int, [_VP]),
    "pb_event_record": (C.c_int, [_VP, _VP]),
    "pb_event_sync": (C.c_int, [_VP]),
    "pb_event_elapsed_ms": (C.c_int, [_VP, _VP, C.POINTER(C.c_float)]),
    "pb_stream_copy": (C.c_int, [_VP, _VP, C.c_size_t, _VP]),
    "pb_comm_unique_id": (C.c_int, [_VP]),
    "pb_comm_init": (C.c_int, [C.c_int, C.c_int, _VP, C.POINTER(_VP)]),
    "pb_comm_destroy": (C.c_int, [_VP]),
    "pb_comm_rank": (C.c_int, [_VP, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "pb_bcast_params": (C.c_int, [_VP, C.POINTER(pb_proj), C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(pb_proj), C.c_int, _VP]),
    "pb_shard_range": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "pb_remap_batch_sharded": (C.c_int, [_VP, _VP, _VP, _VP, C.c_int, C.c_size_t, C.c_size_t, C.POINTER(C.c_int), C.POINTER(C.c_int), _VP]),
    "pb_device_count": (C.c_int, [C.POINTER(C.c_int)]),
    "pb_set_device": (C.c_int, [C.c_int]),
    "pb_get_device": (C.c_int, [C.POINTER(C.c_int)]),
    "pb_device_sync": (C.c_int, []),
    "pb_stream_wait_event": (C.c_int, [_VP, _VP]),
    "pb_host_alloc": (C.c_int, [C.POINTER(_VP), C.c_size_t]),
    "pb_host_free": (C.c_int, [_VP]),
    "pb_host_register": (C.c_int, [_VP, C.c_size_t]),
    "pb_host_unregister": (C.c_int, [_VP]),
}

_lib = None
_lock = threading.Lock()


def load() -> C.CDLL:
    """dlopen the in-tree HIP library and bind every declared symbol."""
    global _lib, MATH_FLAVOUR
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise PbError(
                f"{LIB_PATH} is missing - build it with `python -m photonbend_amd.build{' --libm' if MATH_FLAVOUR == 'libm' else ''}` "
                "(hipcc --offload-arch=gfx950).  There is no CPU fallback."
            )
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)  # AttributeError if the ABI lost a symbol
            fn.restype = res
            fn.argtypes = args
        if lib.pb_abi_version() != ABI_VERSION:
            raise PbError(f"ABI version mismatch: library says {lib.pb_abi_version()}, binding expects {ABI_VERSION}")
        # the flavour a process runs in is the LIBRARY's: the plan cache's key and the fixtures the tests pick follow it.  A product library
        # must be the host's flavour; a library named by PB_LIB_PATH (A/B builds, the diagnostic build) says itself which one it is - and
        # must agree with an explicit PB_MATH_FLAVOUR.
        theirs = "libm" if lib.pb_math_flavour() == 1 else "svml"
        if theirs != MATH_FLAVOUR:
            if not os.environ.get("PB_LIB_PATH") or os.environ.get("PB_MATH_FLAVOUR", "").lower() in ("svml", "libm"):
                raise PbError(f"{LIB_PATH} is the {theirs} flavour of the library, this process wants {MATH_FLAVOUR}")
            MATH_FLAVOUR = theirs
        _lib = lib
    return _lib


def check_interpolation(interpolation: str, supersample: int = 1) -> int:
    """The one check of an interpolation name, made by every entry point before any library call (ValueError): one of INTERPOLATIONS,
    and catmull-rom is not supersampled (the supersampled ABI takes INTERP_IDS only).  Returns the supersample factor as an int."""
    if interpolation not in INTERPOLATIONS:
        raise ValueError(f"interpolation must be one of {', '.join(map(repr, INTERPOLATIONS))}, got {interpolation!r}")
    n = check_supersample(supersample)
    if n > 1 and interpolation not in INTERP_IDS:
        raise ValueError(f"{interpolation} sampling is not supersampled: pass supersample=1")
    return n


VIDEO_INTERPOLATIONS = ("nearest", "bilinear")  # what remap_nv12 / remap_planar sample with


def check_video_interpolation(interpolation: str) -> bool:
    """The interpolation name of a video call (``remap_nv12``, ``remap_planar`` and their ``_supported``): ``check_interpolation``'s
    ValueError for an unknown name, and one for a mode video frames do not have.  -> whether it is "bilinear"."""
    if interpolation == "nearest" or interpolation == "bilinear":  # (every launch asks: the two good answers first)
        return interpolation == "bilinear"
    check_interpolation(interpolation)
    if interpolation not in VIDEO_INTERPOLATIONS:
        raise ValueError(f"video frames are sampled with one of {', '.join(map(repr, VIDEO_INTERPOLATIONS))}, got {interpolation!r}")
    return interpolation == "bilinear"


TRACK_INTERP_IDS = {"nearest": 0, "bilinear": 1, "catmull-rom": 2}  # pb_remap_track_u8's PB_INTERP_* ids
TRACK_MATRIX_BYTES = 72  # one row-major 3 x 3 float64 matrix of a rotation table


def rotation_table(rotations, n_rot: int = 0):
    """A rotation track as pb_remap_track_u8 takes it -> (table, N, k): N frames of k rotations each, applied in order behind a plan's own
    ``n_rot``.  ``rotations``: a float64 ndarray (N, 3, 3) or (N, k, 3, 3) - returned C-contiguous as (N, k, 3, 3), for upload -, a device
    array of float64 of either shape (contiguous; returned as it is, used in place), or a sequence of ``Rotation`` objects / 3 x 3
    matrices (one per frame).  ValueError for any other shape or dtype, for k < 1 and for n_rot + k > PB_MAX_ROTATIONS.  Needs no GPU."""
    if is_device_array(rotations):
        tab = rotations
        dt = torch_dtype_np(tab.dtype) if is_tensor(tab) else np.dtype(tab.dtype)
        if is_tensor(tab) and not tab.is_contiguous():
            raise ValueError("a device rotation table must be contiguous")
    else:
        if not isinstance(rotations, np.ndarray):
            try:
                rotations = [getattr(r, "rotation_matrix", r) for r in rotations]
            except TypeError:
                raise ValueError(f"rotations must be an array (N, 3, 3) or (N, k, 3, 3) or a sequence of Rotation objects, got {type(rotations).__name__}") from None
            rotations = np.asarray(rotations) if len(rotations) else np.empty((0, 3, 3), np.float64)
        tab, dt = rotations, rotations.dtype
    shp = tuple(int(v) for v in tab.shape)
    if dt != np.float64:
        raise ValueError(f"a rotation table holds float64 matrices, got {dt}")
    if len(shp) not in (3, 4) or shp[-2:] != (3, 3):
        raise ValueError(f"a rotation table has shape (N, 3, 3) or (N, k, 3, 3), got {shp}")
    n, k = shp[0], (shp[1] if len(shp) == 4 else 1)
    if k < 1 or int(n_rot) + k > PB_MAX_ROTATIONS:
        raise ValueError(f"{k} rotations per frame behind the plan's {int(n_rot)}: between 1 and {PB_MAX_ROTATIONS - int(n_rot)} fit (PB_MAX_ROTATIONS = {PB_MAX_ROTATIONS})")
    if isinstance(tab, np.ndarray):
        tab = np.ascontiguousarray(tab).reshape(n, k, 3, 3)
    return tab, n, k


PX_SIZES = (1, 2, 3, 4, 6, 8)  # bytes per pixel pb_remap_px takes: grey8, grey16 / two uint8 channels, RGB8, RGBA8, RGB16, RGBA16


class pb_nv12_layout(C.Structure):
    """include/photonbend_hip.h: the plane layout of 4:2:0 semi-planar frames, in bytes; a 0 member is the packed default."""
    _fields_ = [("pitch", C.c_size_t), ("uv_offset", C.c_size_t), ("frame_stride", C.c_size_t)]


def nv12_layout(layout):
    """None, a pb_nv12_layout, a dict or a (pitch, uv_offset, frame_stride) tuple -> a pb_nv12_layout or None."""
    if layout is None or isinstance(layout, pb_nv12_layout):
        return layout
    if isinstance(layout, dict):
        extra = set(layout) - {"pitch", "uv_offset", "frame_stride"}
        if extra:
            raise ValueError(f"unknown layout members {sorted(extra)}")
        return pb_nv12_layout(int(layout.get("pitch", 0)), int(layout.get("uv_offset", 0)), int(layout.get("frame_stride", 0)))
    pitch, uv_offset, frame_stride = layout
    return pb_nv12_layout(int(pitch), int(uv_offset), int(frame_stride))


def nv12_frame_bytes(layout, height: int, width: int, bytes_per_sample: int) -> tuple:
    """(bytes one frame spans, frame stride) of a layout (None: packed) - the library's defaults, for buffer-size checks."""
    l = layout or pb_nv12_layout()
    pitch = l.pitch or bytes_per_sample * width
    uv = l.uv_offset or pitch * height
    span = uv + pitch * (height // 2)
    return span, (l.frame_stride or span)


PLANAR_444, PLANAR_422, PLANAR_420 = 0, 1, 2  # include/photonbend_hip.h: PB_PLANAR_*
PLANAR_SHIFTS = {PLANAR_444: (0, 0), PLANAR_422: (1, 0), PLANAR_420: (1, 1)}  # (cx, cy): planes 1 and 2 are (h >> cy, w >> cx)
_PLANAR_NAMES = {"444": PLANAR_444, "4:4:4": PLANAR_444, "422": PLANAR_422, "4:2:2": PLANAR_422, "420": PLANAR_420, "4:2:0": PLANAR_420}
_U8, _U16 = np.dtype(np.uint8), np.dtype(np.uint16)


def planar_subsampling(subsampling) -> int:
    """PLANAR_444 / PLANAR_422 / PLANAR_420, or "444" / "4:4:4" and so on -> the PB_PLANAR_* id.  ValueError otherwise."""
    if isinstance(subsampling, str) and subsampling in _PLANAR_NAMES:
        return _PLANAR_NAMES[subsampling]
    if not isinstance(subsampling, (str, bool)) and subsampling in PLANAR_SHIFTS:
        return int(subsampling)
    raise ValueError(f"subsampling must be PLANAR_444, PLANAR_422 or PLANAR_420 (or '444', '422', '420'), got {subsampling!r}")


def planar_dims_rule(subsampling: int, name: str | None = None) -> str:
    """The dimension rule of a subsampling, as the error messages say it - with a pixel format's name where there is one."""
    what = name or {PLANAR_444: "4:4:4", PLANAR_422: "4:2:2", PLANAR_420: "4:2:0"}[subsampling]
    return {PLANAR_444: f"{what} frames take any dimensions", PLANAR_422: f"{what} frames have even widths",
            PLANAR_420: f"{what} frames have even widths and heights"}[subsampling]


def planar_dims_ok(subsampling: int, *shapes) -> bool:
    """Whether every (height, width) obeys the subsampling's rule: widths multiples of 1 << cx, heights of 1 << cy."""
    cx, cy = PLANAR_SHIFTS[subsampling]
    return not any((int(h) & cy) | (int(w) & cx) for h, w in shapes)


def planar_frame_samples(height: int, width: int, subsampling: int) -> int:
    """Samples of one packed planar frame: plane 0 and two planes (h >> cy, w >> cx)."""
    cx, cy = PLANAR_SHIFTS[subsampling]
    return height * width + 2 * (height >> cy) * (width >> cx)


class pb_planar_layout(C.Structure):
    """include/photonbend_hip.h: the plane layout of planar frames, in bytes; a 0 member is the packed default."""
    _fields_ = [("pitch", C.c_size_t), ("chroma_pitch", C.c_size_t), ("offset1", C.c_size_t), ("offset2", C.c_size_t), ("frame_stride", C.c_size_t)]


_PLANAR_MEMBERS = ("pitch", "chroma_pitch", "offset1", "offset2", "frame_stride")


def planar_layout(layout):
    """None, a pb_planar_layout, a dict or a (pitch, chroma_pitch, offset1, offset2, frame_stride) tuple -> a pb_planar_layout or None."""
    if layout is None or isinstance(layout, pb_planar_layout):
        return layout
    if isinstance(layout, dict):
        extra = set(layout) - set(_PLANAR_MEMBERS)
        if extra:
            raise ValueError(f"unknown layout members {sorted(extra)}")
        return pb_planar_layout(*[int(layout.get(m, 0)) for m in _PLANAR_MEMBERS])
    pitch, chroma_pitch, offset1, offset2, frame_stride = layout
    return pb_planar_layout(int(pitch), int(chroma_pitch), int(offset1), int(offset2), int(frame_stride))


def planar_frame_bytes(layout, height: int, width: int, bytes_per_sample: int, subsampling: int) -> tuple:
    """(pitch, chroma_pitch, offset1, offset2, bytes one frame spans, frame stride) of a layout (None: packed) - the library's defaults and
    its layout checks (pb_planar_resolve), for buffer-size checks and plane views.  PbError for a pitch smaller than a row, planes that
    overlap, a plane beyond frame_stride and members that are no multiple of the sample size.  Needs no GPU."""
    l = layout or pb_planar_layout()
    S = int(bytes_per_sample)
    cx, cy = PLANAR_SHIFTS[subsampling]
    cw, ch = width >> cx, height >> cy
    pitch = l.pitch or S * width
    cpitch = l.chroma_pitch or S * cw
    if pitch < S * width or cpitch < S * cw:
        raise PbError("pitch smaller than a row")
    e0 = pitch * (height - 1) + S * width if height else 0
    ce = cpitch * (ch - 1) + S * cw if ch else 0
    o1 = l.offset1 or pitch * height
    o2 = l.offset2 or o1 + cpitch * ch
    if o1 < e0 or o2 < e0 or (ce and (o1 + ce > o2 if o1 < o2 else o2 + ce > o1)):
        raise PbError("the planes of a frame overlap")
    span = max(o1, o2) + ce
    stride = l.frame_stride or max(span, o2 + cpitch * ch)
    if stride < span:
        raise PbError("frame_stride smaller than a frame: a plane ends beyond it")
    if any(v % S for v in (pitch, cpitch, o1, o2, stride)):
        raise PbError(f"pitch, chroma_pitch, offsets and frame_stride must be multiples of {S} bytes (one sample)")
    return pitch, cpitch, o1, o2, span, stride


# (semi-planar?, rotation track?, bilinear?, the _supported question?) -> pb_remap[_track]_{nv12,planar}[_bilinear][_supported]
_VIDEO_FUNCTIONS = {(pairs, tracked, bilinear, question): f"pb_remap_{'track_' if tracked else ''}{'nv12' if pairs else 'planar'}{'_bilinear' if bilinear else ''}"
                                                          f"{'_supported' if question else ''}"
                    for pairs in (False, True) for tracked in (False, True) for bilinear in (False, True) for question in (False, True) if not (tracked and question)}
# ... and the stitch calls of a double-fisheye source: (semi-planar?, the _supported question?)
_STITCH_FUNCTIONS = {(pairs, question): f"pb_stitch_{'nv12' if pairs else 'planar'}{'_supported' if question else ''}" for pairs in (False, True) for question in (False, True)}
# ... and their rotation tracks: semi-planar?
_TRACK_STITCH_FUNCTIONS = {False: "pb_track_stitch_planar", True: "pb_track_stitch_nv12"}
_FILL = C.c_uint16 * 3  # the samples of black pixels, as the video calls take them


class VideoFamily(typing.NamedTuple):
    """What distinguishes the families of video frames (the library's PbVideoFmt): 4:2:0 semi-planar frames - NV12 / P010, planes 1 and 2
    as one plane of interleaved pairs (``NV12``) - or planar frames at a subsampling (``video_family``).  What ``Plan``'s video
    methods check differently for the two is said here; the library's functions are ``_VIDEO_FUNCTIONS``."""

    pairs: bool
    sub: int  # PLANAR_* (pairs: PLANAR_420)

    def layout(self, layout):
        return nv12_layout(layout) if self.pairs else planar_layout(layout)

    def frame_bytes(self, layout, height: int, width: int, bytes_per_sample: int) -> tuple:
        """(bytes one frame spans, frame stride) of a layout (None: packed); a planar layout is checked (``planar_frame_bytes``)."""
        if self.pairs:
            return nv12_frame_bytes(layout, height, width, bytes_per_sample)
        return planar_frame_bytes(layout, height, width, bytes_per_sample, self.sub)[4:]

    def check(self, h: int, w: int, Hd: int, Wd: int, dt) -> None:
        """The dimension rule for a plan's source and destination, and the sample type.  PbError."""
        if not planar_dims_ok(self.sub, (h, w), (Hd, Wd)):
            raise PbError("4:2:0 frames need even source and destination dimensions" if self.pairs
                          else f"{planar_dims_rule(self.sub)}, source and destination: the plan maps {h} x {w} to {Hd} x {Wd}")
        if dt not in (_U8, _U16):
            raise PbError(f"NV12 frames are uint8 and P010 / P016 frames uint16, got {dt}" if self.pairs else f"planar frames hold uint8 or uint16 samples, got {dt}")

    def packed(self, h: int, w: int) -> tuple:
        """The shapes of one packed (h, w) frame: (3h/2, w), or flat - a 4:2:0 or 4:2:2 frame is no rectangle - and at 4:4:4 also (3, h, w)."""
        if self.pairs:
            return ((3 * h // 2, w),)
        return ((planar_frame_samples(h, w, self.sub),),) + (((3, h, w),) if self.sub == PLANAR_444 else ())

    def packed_error(self, h: int, w: int, shp: tuple) -> str:
        if self.pairs:
            return f"packed source frames must be ({3 * h // 2}, {w}) or (N, {3 * h // 2}, {w}), got {shp}"
        ns = planar_frame_samples(h, w, self.sub)
        return f"packed source frames must be ({ns},) or (N, {ns})" + (f", or (3, {h}, {w}) / (N, 3, {h}, {w})" if self.sub == PLANAR_444 else "") + f", got {shp}"


NV12 = VideoFamily(True, PLANAR_420)


def video_family(subsampling) -> VideoFamily:
    """The planar family of a subsampling (``planar_subsampling``'s names and ValueError)."""
    return VideoFamily(False, planar_subsampling(subsampling))


# THE table of video pixel formats, by ffmpeg's -pix_fmt names: name -> (sample type, family, the samples of black; None: video black
# scaled to the sample size).  10-bit formats carry their value in the low bits of a 16-bit sample; gbrp is planar RGB in the order G, B, R
VIDEO_FORMATS = {
    "nv12": (_U8, NV12, None),
    "p010": (_U16, NV12, None),
    "yuv420p": (_U8, video_family(PLANAR_420), (16, 128, 128)),
    "yuv422p": (_U8, video_family(PLANAR_422), (16, 128, 128)),
    "yuv444p": (_U8, video_family(PLANAR_444), (16, 128, 128)),
    "yuv420p10le": (_U16, video_family(PLANAR_420), (64, 512, 512)),
    "yuv422p10le": (_U16, video_family(PLANAR_422), (64, 512, 512)),
    "yuv444p10le": (_U16, video_family(PLANAR_444), (64, 512, 512)),
    "yuv420p16le": (_U16, video_family(PLANAR_420), (16 << 8, 128 << 8, 128 << 8)),
    "yuv444p16le": (_U16, video_family(PLANAR_444), (16 << 8, 128 << 8, 128 << 8)),
    "gbrp": (_U8, video_family(PLANAR_444), (0, 0, 0)),
    "gbrp16le": (_U16, video_family(PLANAR_444), (0, 0, 0)),
}
# ... and its planar part as name -> (sample type, subsampling, the samples of black)
PLANAR_FORMATS = {name: (dt, fam.sub, fill) for name, (dt, fam, fill) in VIDEO_FORMATS.items() if not fam.pairs}


def px_align(bytes_per_px: int) -> int:
    """The alignment pb_remap_px asks of frame pointers and strides: min(4, B & -B) bytes."""
    return min(4, bytes_per_px & -bytes_per_px)


def tail_bytes(tail, dtype) -> int:
    """Bytes per pixel of frames whose shape after (h, w) is `tail`: the one place a trailing shape and a dtype become a byte count."""
    n = np.dtype(dtype).itemsize
    for v in tail:  # (no NumPy reduction: every facade call asks)
        n *= int(v)
    return n


def pixel_bytes(shape, dtype, hw) -> int:
    """Bytes per pixel of an (h, w, *tail) or (N, h, w, *tail) array of `dtype` for a plan whose source (or destination) is hw = (h, w);
    0 when the leading dimensions are not that."""
    shp = tuple(int(v) for v in shape)
    for lead in (2, 3):
        if len(shp) >= lead and shp[lead - 2:lead] == tuple(hw):
            return tail_bytes(shp[lead:], dtype)
    return 0


def check_supersample(n) -> int:
    """The supersample factor as an int: 1 (off), 2 or 4 (n x n subsamples per output pixel); anything else is a ValueError.  Needs no GPU."""
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or int(n) not in SUPERSAMPLE_FACTORS:
        raise ValueError(f"supersample must be one of {SUPERSAMPLE_FACTORS} (n x n subsamples per output pixel), got {n!r}")
    return int(n)


def check(status: int) -> None:
    if status != 0:
        msg = load().pb_last_error()
        raise PbError(f"photonbend_hip error {status}: {msg.decode() if msg else '?'}")


def is_tensor(x) -> bool:
    return torch is not None and isinstance(x, torch.Tensor)


def is_device_array(x) -> bool:
    """A CUDA tensor or a DeviceArray: something the kernels can be pointed at."""
    return isinstance(x, DeviceArray) or (is_tensor(x) and x.is_cuda)


def current_stream() -> int:
    """The stream launches go to: torch's current stream where torch is installed (its tensors are ordered on it), the
    default stream otherwise."""
    return int(torch.cuda.current_stream().cuda_stream) if (torch is not None and torch.cuda.is_available()) else 0


def device_count() -> int:
    n = C.c_int(0)
    check(load().pb_device_count(C.byref(n)))
    return int(n.value)


def current_device() -> int:
    if torch is not None and torch.cuda.is_available():
        return int(torch.cuda.current_device())
    d = C.c_int(0)
    check(load().pb_get_device(C.byref(d)))
    return int(d.value)


@contextlib.contextmanager
def on_device(index):
    """Runs the block with device `index` current (None: whatever is current)."""
    if index is None:
        yield
    elif torch is not None and torch.cuda.is_available():
        with torch.cuda.device(int(index)):
            yield
    else:
        prev = current_device()
        if prev != int(index):
            check(load().pb_set_device(int(index)))
        try:
            yield
        finally:
            if prev != int(index):
                check(load().pb_set_device(prev))


def device_index_of(x):
    """Device ordinal a device array lives on (DeviceArrays: the current device, where they were allocated)."""
    if is_tensor(x):
        return x.device.index if x.device.index is not None else current_device()
    return None


_gpu_ok = None


def require_gpu() -> None:
    global _gpu_ok
    if _gpu_ok is None:
        _gpu_ok = (torch.cuda.is_available() if torch is not None else False) or device_count() > 0
    if not _gpu_ok:
        raise PbError("no HIP device is visible; photonbend_amd has no CPU path")


def torch_dtype(dt):
    return torch.from_numpy(np.empty(0, np.dtype(dt))).dtype


def empty(shape, dtype, like=None, device=None):
    """Uninitialised device array: a CUDA tensor where torch is installed (on `like`'s device / `device` / the current one),
    else a DeviceArray.  `like` a DeviceArray forces a DeviceArray."""
    if isinstance(like, DeviceArray) or torch is None:
        return DeviceArray(shape, dtype)
    dev = like.device if is_tensor(like) else (device if device is not None else torch.device("cuda", torch.cuda.current_device()))
    return torch.empty(tuple(shape), dtype=torch_dtype(dtype), device=dev)


def to_host(x) -> np.ndarray:
    """Device array -> fresh ndarray (synchronous)."""
    return x.cpu().numpy() if is_tensor(x) else x.numpy()


def to_device(a: np.ndarray, device=None):
    """ndarray -> device array of the default kind (CUDA tensor with torch, DeviceArray without); synchronous."""
    a = np.ascontiguousarray(a)
    if torch is None:
        return DeviceArray(a.shape, a.dtype).copy_from_host(a)
    if not a.flags.writeable:
        a = a.copy()  # (torch refuses read-only arrays)
    return torch.from_numpy(a).to(device if device is not None else torch.device("cuda", torch.cuda.current_device()))


def _on(x):
    return on_device(device_index_of(x))


class _LaunchGate:
    """Launches of one plan (any number at a time) against the one rebuild of its tables a plan made for the reference's sampler may see -
    the opt-in bilinear mode's first use, on whichever thread of the host's plan cache that happens.  The C ABI's rule for
    pb_plan_prepare on a prepared plan is the caller's: no launch of the plan in flight or started during the call."""

    __slots__ = ("_cv", "_inside", "_closed")

    def __init__(self):
        self._cv = threading.Condition(threading.Lock())
        self._inside, self._closed = 0, False

    def enter(self) -> None:
        with self._cv:
            while self._closed:
                self._cv.wait()
            self._inside += 1

    def leave(self) -> None:
        with self._cv:
            self._inside -= 1
            if self._closed and not self._inside:
                self._cv.notify_all()

    def close(self) -> None:
        with self._cv:
            self._closed = True
            while self._inside:
                self._cv.wait()

    def open(self) -> None:
        with self._cv:
            self._closed = False
            self._cv.notify_all()


class Plan:
    """Owner of one pb_plan (dst projection, rotations, src projection)."""

    def __init__(self, dst: pb_proj, rotations, src: pb_proj, *, defer: bool = False, tune: bool = False, budget: int = 0, bilinear: bool = False):
        """``defer``: no device work now - launches run the faithful kernel until ``prepare()``;
        ``tune``: pick the LDS window budget by timing (opt-in, allocates scratch frames);
        ``budget``: explicit window budget in bytes (0 = library default);
        ``bilinear``: build the opt-in bilinear mode's tables now (0.2-0.3 ms of a c2 plan's 0.85) instead of at the first bilinear use
        (``ensure_bilinear``, called by ``remap`` / ``launch`` / the mode's diagnostics)."""
        lib = load()
        rots = np.ascontiguousarray(np.asarray(list(rotations), dtype=np.float64).reshape(-1, 9))
        if rots.shape[0] > PB_MAX_ROTATIONS:
            raise PbError(f"at most {PB_MAX_ROTATIONS} chained rotations are supported")
        self._h = _VP()
        rp = rots.ctypes.data_as(C.POINTER(C.c_double)) if rots.shape[0] else None
        flags = (PLAN_DEFER if defer else 0) | (PLAN_TUNE if tune else 0) | (0 if bilinear else PLAN_NO_BILINEAR)
        check(lib.pb_plan_create_ex(C.byref(dst), rp, rots.shape[0], C.byref(src), flags, int(budget), C.byref(self._h)))
        self.dst, self.src, self.n_rot = dst, src, rots.shape[0]
        self.double_src = src.kind == KIND_DOUBLE
        self._bilinear, self._deferred, self._bil_lock = bool(bilinear), bool(defer), threading.Lock()
        self._gate = None if (bilinear and not defer) else _LaunchGate()  # (None: the tables are final)

    @classmethod
    def _adopt(cls, handle, dst: pb_proj, src: pb_proj, n_rot: int) -> "Plan":
        self = cls.__new__(cls)
        self._h = handle
        self.dst, self.src, self.n_rot = dst, src, n_rot
        self.double_src = src.kind == KIND_DOUBLE
        self._bilinear, self._deferred, self._bil_lock = True, False, threading.Lock()  # (a restored plan rebuilds the mode's tables with everything else)
        self._gate = None
        return self

    def _rebuild(self, flags: int, budget: int) -> None:
        """pb_plan_prepare with this plan's launches held off: those inside the library leave first, the device drains (the tables the
        call rewrites may be in use by launches already queued, on any stream), new ones wait at the gate."""
        g = self._gate
        if g is not None:
            g.close()
        try:
            lib = load()
            if g is not None and not self._deferred:  # (a prepared plan: its tables may be in use by launches already queued, on any stream)
                check(lib.pb_device_sync())
            check(lib.pb_plan_prepare(self._h, flags, int(budget)))
        finally:
            if g is not None:
                g.open()

    def prepare(self, tune: bool = False, budget: int = 0) -> None:
        """Builds the fast path of a deferred plan on the current device (or re-applies ``budget``)."""
        with self._bil_lock:
            self._rebuild((PLAN_TUNE if tune else 0) | (PLAN_BILINEAR if self._bilinear else 0), budget)
            self._deferred = False
            if self._bilinear:
                self._gate = None

    def ensure_bilinear(self) -> None:
        """The opt-in bilinear mode's tables (which the Catmull-Rom mode reads too), built once when either mode is first used
        (synchronous: it waits for the device).  Launches of this plan made through
        this object on other threads wait while the tables are built; launches through the raw ``handle`` follow the C ABI's rule
        (none in flight, as for ``set_window_budget``).  A deferred plan stays deferred - its launches run the float64 kernels of
        either mode - and remembers the wish for ``prepare()``."""
        if self._bilinear:
            return
        with self._bil_lock:
            if not self._bilinear:
                if not self._deferred:
                    self._rebuild(PLAN_BILINEAR, 0)
                    self._gate = None
                self._bilinear = True

    def set_window_budget(self, budget: int) -> None:
        check(load().pb_plan_set_window_budget(self._h, int(budget)))

    def timing(self) -> dict:
        a, b = C.c_double(), C.c_double()
        check(load().pb_plan_timing(self._h, C.byref(a), C.byref(b)))
        return {"prepare_ms": a.value, "tune_ms": b.value}

    def serialize(self) -> bytes:
        """The prepared plan as a blob (``Plan.deserialize`` restores it without re-certifying)."""
        n = C.c_size_t()
        check(load().pb_plan_serialize(self._h, None, 0, C.byref(n)))
        buf = C.create_string_buffer(n.value)
        check(load().pb_plan_serialize(self._h, buf, n.value, C.byref(n)))
        return buf.raw[: n.value]

    @classmethod
    def deserialize(cls, blob: bytes, dst: pb_proj, rotations, src: pb_proj) -> "Plan":
        """Restores a serialized plan and checks that it was made for exactly this request (projections and rotation
        bits): a cache file name is not proof of what the file holds."""
        rots = np.ascontiguousarray(np.asarray(list(rotations), dtype=np.float64).reshape(-1, 9))
        h = _VP()
        raw = bytes(blob)
        check(load().pb_plan_deserialize(raw, len(raw), C.byref(h)))
        plan = cls._adopt(h, dst, src, rots.shape[0])  # (owns the handle: destroyed with `plan` if the check below raises)
        rp = rots.ctypes.data_as(C.POINTER(C.c_double)) if rots.shape[0] else None
        same = load().pb_plan_matches(h, C.byref(dst), rp, rots.shape[0], C.byref(src))
        if same < 0:
            check(same)
        if same != 1:
            raise PbError("the serialized plan belongs to another geometry")
        return plan

    @property
    def handle(self):
        return self._h

    def set_mode(self, mode: int) -> None:
        """MODE_AUTO (certified fast tiles, else faithful), MODE_FAITHFUL, MODE_FAST."""
        check(load().pb_plan_set_mode(self._h, int(mode)))

    def info(self) -> dict:
        fast = C.c_int()
        st = (C.c_longlong * 7)()
        thr = (C.c_longlong * 4)()
        check(load().pb_plan_info(self._h, C.byref(fast), st, thr))
        return {
            "fast_path": bool(fast.value),
            "tiles": int(st[0]),
            "fix_tiles": int(st[1]),
            "fix_pixels": int(st[2]),
            "model_diff_pixels": int(st[3]),
            "lean_tiles": int(st[4]),
            "black_tiles": int(st[5]),
            "direct_tiles": int(st[6]),
            "thresholds": [int(t) for t in thr],
            "window_budget": int(load().pb_plan_window_budget(self._h)),
            "bilinear_float64_tiles": int(load().pb_plan_bilinear_float64_tiles(self._h)),
        }

    def bilinear_launch_shape(self) -> dict:
        """The bilinear launch's workgroup LDS (bytes) and workgroups per frame - diagnostic."""
        self.ensure_bilinear()
        lds, wgs = C.c_int(), C.c_int()
        check(load().pb_plan_bilinear_launch_shape(self._h, C.byref(lds), C.byref(wgs)))
        return {"lds_bytes": lds.value, "workgroups": wgs.value}

    def bilinear_tile_mix(self) -> dict:
        """How the opt-in bilinear mode serves the plan's tiles (diagnostic, synchronous)."""
        self.ensure_bilinear()
        m = (C.c_longlong * 8)()
        check(load().pb_plan_bilinear_tile_mix(self._h, m))
        mix = dict(zip(("window", "direct", "table", "black", "td3", "entries", "half_windows", "table_plain"), (int(x) for x in m)))
        # what the video kernel's fix-pixel path meets (pb_plan_video_bilinear_mix): modelled tiles with fix pixels, their fix pixels, and
        # of those the chroma anchors at 4:2:2 and at 4:2:0
        v = (C.c_longlong * 4)()
        check(load().pb_plan_video_bilinear_mix(self._h, v))
        mix.update(zip(("fix_tiles", "fix_pixels", "fix_anchors_422", "fix_anchors_420"), (int(x) for x in v)))
        return mix

    def stitch_tile_mix(self) -> dict:
        """What the waves of a stitch launch (``stitch_planar`` / ``stitch_nv12``) meet in this plan, slot by slot of its launch-order table
        (pb_plan_stitch_tile_mix; diagnostic, synchronous): one-eye slots, two-eye tiles by weight class, failed tiles, two-eye tiles with
        fix pixels, those pixels, and of them the chroma anchors at 4:2:2 and at 4:2:0.  All zero without double-fisheye tile tables."""
        m = (C.c_longlong * 9)()
        check(load().pb_plan_stitch_tile_mix(self._h, m))
        return dict(zip(("solo", "unit", "row", "lat", "failed", "fix_tiles", "fix_pixels", "fix_anchors_422", "fix_anchors_420"), (int(x) for x in m)))

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h and _lib is not None:
            _lib.pb_plan_destroy(h)

    # -- launches (device arrays in, device arrays out: CUDA tensors or DeviceArrays; on the current stream unless told otherwise)
    def launch(self, src_ptr: int, dst_ptr: int, n_frames: int = 1, stream: int | None = None, interpolation: str = "nearest",
               src_stride: int = 0, dst_stride: int = 0, supersample: int = 1, generic: bool = False, workspace=None, bytes_per_px: int = 3) -> None:
        """The raw call: n_frames frames at src_ptr / dst_ptr (device addresses, strides in bytes, 0 = packed) on `stream`.
        ``supersample`` n in (2, 4): this plan is the n x destination's and each output frame is (H / n, W / n, 3), the n x n block
        means (pb_remap_ss_u8; ``generic`` forces its generic path).  ``workspace``: a device array of at least
        ``supersample_workspace_bytes(...)`` bytes the caller owns (allocate it outside a graph capture and keep it per stream); without
        one, a call that needs it takes a temporary buffer - from PyTorch's stream-ordered allocator where torch is installed, else a
        DeviceArray that is freed after the call (on a stream other than the default one the call then synchronises that stream).
        ``bytes_per_px``: the frames' pixel size, one of PX_SIZES (pb_remap_px; nearest, not supersampled); 3 is the uint8 RGB call."""
        n = check_interpolation(interpolation, supersample)
        if bytes_per_px != 3:
            if interpolation != "nearest" or n != 1:
                raise ValueError("frames of other than 3-byte pixels take nearest sampling without supersampling")
            self._gated(load().pb_remap_px, self._h, src_ptr, dst_ptr, int(n_frames), int(src_stride), int(dst_stride), int(bytes_per_px),
                        current_stream() if stream is None else stream)
            return
        if interpolation != "nearest":
            self.ensure_bilinear()  # (catmull-rom reads the bilinear mode's tables too)
        st = current_stream() if stream is None else stream
        if n == 1:
            fn = {"nearest": load().pb_remap_u8, "bilinear": load().pb_remap_bilinear_u8, "catmull-rom": load().pb_remap_catmull_rom_u8}[interpolation]
            self._gated(fn, self._h, src_ptr, dst_ptr, int(n_frames), int(src_stride), int(dst_stride), st)
            return
        interp, flags = INTERP_IDS[interpolation], (SS_GENERIC if generic else 0)
        nbytes = self.supersample_workspace_bytes(n, interpolation, generic, src_ptr, src_stride)
        args = (self._h, n, interp, src_ptr, dst_ptr, int(n_frames), int(src_stride), int(dst_stride))
        if nbytes == 0:
            self._gated(load().pb_remap_ss_u8, *args, None, 0, flags, st)
        elif workspace is not None:
            have = int(workspace.nbytes) if not is_tensor(workspace) else int(workspace.numel() * workspace.element_size())
            if have < nbytes:
                raise PbError(f"the supersample workspace holds {have} bytes, this call needs {nbytes}")
            self._gated(load().pb_remap_ss_u8, *args, workspace.data_ptr(), have, flags, st)
        else:
            with _temporary_workspace(nbytes, st) as ws:
                self._gated(load().pb_remap_ss_u8, *args, ws.data_ptr(), nbytes, flags, st)

    def supersample_workspace_bytes(self, supersample: int, interpolation: str = "nearest", generic: bool = False, src_ptr: int = 0,
                                    src_stride: int = 0) -> int:
        """Device bytes a supersampled launch of this plan needs as workspace (pb_remap_ss_workspace): 0 when the fused kernel takes it,
        else one n x frame.  ``src_ptr`` / ``src_stride``: the frames the call will pass (the fused kernel needs 16-byte aligned frames; a
        packed frame's size is its stride)."""
        n = check_supersample(supersample)
        if n == 1:
            return 0
        check_interpolation(interpolation, n)
        need = C.c_size_t(0)
        check(load().pb_remap_ss_workspace(self._h, n, INTERP_IDS[interpolation], SS_GENERIC if generic else 0, C.byref(need)))
        nbytes = int(need.value)
        if nbytes == 0 and (int(src_ptr) | (int(src_stride) or 3 * self.src.height * self.src.width)) & 15:
            nbytes = 3 * self.dst.height * self.dst.width
        return nbytes

    def out_shape(self, supersample: int = 1) -> tuple:
        """(H, W) of an output frame: the plan's destination, divided by the supersample factor."""
        n = check_supersample(supersample)
        if self.dst.height % n or self.dst.width % n:
            raise ValueError(f"the plan's destination {self.dst.height} x {self.dst.width} is not divisible by supersample={n}")
        return self.dst.height // n, self.dst.width // n

    def _gated(self, fn, *args) -> None:
        """One library call that launches this plan's kernels: through the gate while the plan's tables may still be rebuilt."""
        g = self._gate
        if g is None:
            check(fn(*args))
            return
        g.enter()
        try:
            check(fn(*args))
        finally:
            g.leave()

    def remap(self, src, out=None, interpolation: str = "nearest", supersample: int = 1, generic: bool = False, workspace=None):
        """src: uint8 device array (h, w, 3) or (N, h, w, 3) -> (H, W, 3) / (N, H, W, 3), of src's kind.
        interpolation: "nearest" (the reference's truncating sample), the opt-in "bilinear" or the opt-in "catmull-rom".
        supersample: n in (2, 4) on a plan of the n x destination -> (H / n, W / n, 3) frames of n x n block means (see ``launch``;
        nearest and bilinear only)."""
        ss = check_interpolation(interpolation, supersample)
        oh, ow = self.out_shape(ss)
        require_gpu()
        if not is_device_array(src):
            raise PbError(f"source frames must be uint8 device arrays (CUDA tensors or DeviceArrays), got {type(src).__name__}")
        tens = is_tensor(src)
        batched = len(src.shape) == 4
        shp = tuple(src.shape)
        n = shp[0] if batched else 1
        u8 = (src.dtype == torch.uint8) if tens else (src.dtype == np.uint8)
        if not u8 or shp[-3:] != (self.src.height, self.src.width, 3) or len(shp) not in (3, 4):
            raise PbError(f"source frames must be uint8 cuda (N, {self.src.height}, {self.src.width}, 3), got {shp} {src.dtype}")
        s = src.contiguous() if tens else src
        oshape = (n, oh, ow, 3)
        if out is None:
            o = empty(oshape, np.uint8, like=s)
        else:
            o = out
            if tuple(o.shape) not in (oshape, oshape[1:] if not batched else oshape):
                raise PbError("out must be a contiguous uint8 cuda tensor of the destination shape")
            if is_tensor(o) != tens or (tens and (o.dtype != torch.uint8 or not o.is_contiguous())) or (not tens and o.dtype != np.uint8):
                raise PbError("out must be a contiguous uint8 cuda tensor of the destination shape")
            if tens and (not o.is_cuda or o.device != s.device):
                raise PbError(f"out must live on the source's device ({s.device}), got {o.device}")
        with _on(s):
            self.launch(s.data_ptr(), o.data_ptr(), n, None, interpolation, supersample=ss, generic=generic, workspace=workspace)
        if out is not None:
            return out
        return o if batched else o[0]

    def launch_track(self, table_ptr: int, n_rot_per_frame: int, src_ptr: int, dst_ptr: int, n_frames: int = 1, stream: int | None = None,
                     interpolation: str = "nearest", src_stride: int = 0, dst_stride: int = 0) -> None:
        """The raw rotation-track call (pb_remap_track_u8): frame f of n_frames is remapped with this plan's own rotations followed by the
        ``n_rot_per_frame`` matrices at table_ptr + f * n_rot_per_frame * 72 (device memory, float64, row-major 3 x 3), in one launch on
        `stream`.  The table must stay alive and unchanged until the stream has run the launch."""
        if interpolation not in TRACK_INTERP_IDS:
            raise ValueError(f"interpolation must be one of {', '.join(map(repr, TRACK_INTERP_IDS))}, got {interpolation!r}")
        self._gated(load().pb_remap_track_u8, self._h, table_ptr, int(n_rot_per_frame), TRACK_INTERP_IDS[interpolation], src_ptr, dst_ptr, int(n_frames),
                    int(src_stride), int(dst_stride), current_stream() if stream is None else stream)

    def remap_track(self, src, rotations, out=None, interpolation: str = "nearest", stream: int | None = None):
        """A batch with a rotation per frame in ONE launch: src uint8 device array (N, h, w, 3) -> (N, H, W, 3); frame f is what a plan of
        this one's rotations followed by ``rotations[f]`` gives in MODE_FAITHFUL.  ``rotations``: see ``rotation_table`` - an ndarray
        (N, 3, 3) / (N, k, 3, 3) or a sequence of ``Rotation`` objects is uploaded; a float64 device array is used in place (keep it
        alive and unchanged until the stream has run the launch).  Shapes, dtypes and counts are checked before any device work."""
        if interpolation not in TRACK_INTERP_IDS:
            raise ValueError(f"interpolation must be one of {', '.join(map(repr, TRACK_INTERP_IDS))}, got {interpolation!r}")
        if not is_device_array(src):
            raise PbError(f"source frames must be uint8 device arrays (CUDA tensors or DeviceArrays), got {type(src).__name__}")
        tens = is_tensor(src)
        shp = tuple(int(v) for v in src.shape)
        u8 = (src.dtype == torch.uint8) if tens else (src.dtype == np.uint8)
        if not u8 or len(shp) != 4 or shp[1:] != (self.src.height, self.src.width, 3):
            raise PbError(f"source frames must be uint8 (N, {self.src.height}, {self.src.width}, 3), got {shp} {src.dtype}")
        n = shp[0]
        tab, n_tab, k = rotation_table(rotations, self.n_rot)
        if n_tab != n:
            raise ValueError(f"{n} frames need {n} rotations, the table holds {n_tab}")
        oshape = (n, self.dst.height, self.dst.width, 3)
        if out is not None:
            ok = is_device_array(out) and is_tensor(out) == tens and tuple(out.shape) == oshape
            ok = ok and ((out.dtype == torch.uint8 and out.is_contiguous()) if tens else out.dtype == np.uint8)
            if not ok:
                raise PbError(f"out must be a contiguous uint8 device array {oshape} of the source's kind")
            if tens and out.device != src.device:
                raise PbError(f"out must live on the source's device ({src.device}), got {out.device}")
        require_gpu()
        s = src.contiguous() if tens else src
        o = empty(oshape, np.uint8, like=s) if out is None else out
        if n == 0:
            return o
        with _on(s):
            st = current_stream() if stream is None else stream
            tab, release = self._track_table(tab, s, st)
            self.launch_track(tab.data_ptr(), k, s.data_ptr(), o.data_ptr(), n, st, interpolation)
            release()
        return o

    def launch_track_px(self, table_ptr: int, n_rot_per_frame: int, src_ptr: int, dst_ptr: int, n_frames: int, channels: int, sample_bytes: int,
                        stream: int | None = None, interpolation: str = "nearest", src_stride: int = 0, dst_stride: int = 0) -> None:
        """The raw rotation-track call for frames of ``channels`` samples of ``sample_bytes`` bytes a pixel (pb_remap_track_px):
        ``launch_track``'s table and frames, a pixel of channels * sample_bytes bytes.  The table must stay alive and unchanged until the
        stream has run the launch."""
        if interpolation not in TRACK_INTERP_IDS:
            raise ValueError(f"interpolation must be one of {', '.join(map(repr, TRACK_INTERP_IDS))}, got {interpolation!r}")
        self._gated(load().pb_remap_track_px, self._h, table_ptr, int(n_rot_per_frame), TRACK_INTERP_IDS[interpolation], src_ptr, dst_ptr, int(n_frames),
                    int(src_stride), int(dst_stride), int(channels), int(sample_bytes), current_stream() if stream is None else stream)

    def track_px_supported(self, channels: int, sample_bytes: int) -> bool:
        """Whether ``remap_track_px`` / ``launch_track_px`` takes this plan with this format (pb_remap_track_px_supported): every plan but a
        double-fisheye source's with 16-bit samples.  channels outside 1..4 or sample_bytes outside (1, 2) is a PbError.  Needs no GPU."""
        r = load().pb_remap_track_px_supported(self._h, int(channels), int(sample_bytes))
        if r < 0:
            check(r)
        return r == 1

    def remap_track_px(self, src, rotations, out=None, interpolation: str = "nearest", stream: int | None = None):
        """``remap_track`` for grey, RGBA and 16-bit frames in ONE launch (pb_remap_track_px): src is a device array (N, h, w)
        or (N, h, w, C) -> (N, H, W[, C]) of the same dtype and kind; frame f is what the materialised-map route gives for this plan's
        rotations followed by ``rotations[f]``.  An interpolating mode or a double-fisheye source looks inside the pixel: uint8 or uint16
        samples, 1 to 4 channels (uint8 for a double fisheye).  Nearest on a single source never does: any dtype whose pixel is 1, 2, 3, 4,
        6 or 8 bytes.  ``rotations``, ``out`` and ``stream`` follow ``remap_track``'s rules; shapes, dtypes, table and counts are checked
        before any device work."""
        if interpolation not in TRACK_INTERP_IDS:
            raise ValueError(f"interpolation must be one of {', '.join(map(repr, TRACK_INTERP_IDS))}, got {interpolation!r}")
        if not is_device_array(src):
            raise PbError(f"source frames must be device arrays (CUDA tensors or DeviceArrays), got {type(src).__name__}")
        tens = is_tensor(src)
        shp = tuple(int(v) for v in src.shape)
        dt = torch_dtype_np(src.dtype) if tens else np.dtype(src.dtype)
        sh = (self.src.height, self.src.width)
        if len(shp) not in (3, 4) or shp[1:3] != sh:
            raise PbError(f"source frames must be (N, {sh[0]}, {sh[1]}) or (N, {sh[0]}, {sh[1]}, C), got {shp} {dt}")
        tail = shp[3:]
        double = self.src.kind == KIND_DOUBLE
        if interpolation != "nearest" or double:
            fmt = (tail[0] if tail else 1, dt.itemsize)  # the sampler looks inside the pixel: (channels, sample bytes)
            if dt not in ((np.dtype(np.uint8),) if double else (np.dtype(np.uint8), np.dtype(np.uint16))) or not 1 <= fmt[0] <= 4:
                what = "a double-fisheye source takes uint8 frames" if double else f"{interpolation} sampling takes uint8 or uint16 frames"
                raise PbError(f"{what} of 1 to 4 channels, got {shp} {dt}")
        else:
            bpp = tail_bytes(tail, dt)  # the sampler never looks inside a pixel: B bytes as (B, 1), or (B / 2, 2) above four
            if bpp not in PX_SIZES:
                raise PbError(f"source frames must have pixels of {PX_SIZES} bytes, got {shp} {dt}")
            fmt = (bpp, 1) if bpp <= 4 else (bpp // 2, 2)
        n = shp[0]
        tab, n_tab, k = rotation_table(rotations, self.n_rot)
        if n_tab != n:
            raise ValueError(f"{n} frames need {n} rotations, the table holds {n_tab}")
        oshape = (n, self.dst.height, self.dst.width) + tail
        if out is not None:
            odt = (torch_dtype_np(out.dtype) if is_tensor(out) else np.dtype(out.dtype)) if is_device_array(out) else None
            if odt != dt or tuple(out.shape) != oshape or is_tensor(out) != tens or (tens and not out.is_contiguous()):
                raise PbError(f"out must be a contiguous device array {oshape} {dt} of the source's kind")
            if tens and out.device != src.device:
                raise PbError(f"out must live on the source's device ({src.device}), got {out.device}")
        require_gpu()
        s = src.contiguous() if tens else src
        o = empty(oshape, dt, like=s) if out is None else out
        if n == 0:
            return o
        with _on(s):
            st = current_stream() if stream is None else stream
            tab, release = self._track_table(tab, s, st)
            self.launch_track_px(tab.data_ptr(), k, s.data_ptr(), o.data_ptr(), n, fmt[0], fmt[1], st, interpolation)
            release()
        return o

    @staticmethod
    def _track_table(tab, like, st):
        """A rotation table on `like`'s device -> (table, release): an ndarray is uploaded (synchronously: it is on the device before the
        launch is queued) and ``release()``, called after the launch on stream `st` is queued, makes its memory safe to reuse; a device
        array is used in place."""
        if not isinstance(tab, np.ndarray):
            return tab, lambda: None
        tens = is_tensor(like)
        dev = torch.from_numpy(tab).to(like.device) if tens else DeviceArray(tab.shape, np.float64).copy_from_host(tab)

        def release():
            if tens and int(st or 0) != current_stream():
                check(load().pb_stream_sync(st))  # (the table goes back to torch's allocator, which orders its reuse on the current stream only)

        return dev, release

    def px_supported(self, bytes_per_px: int) -> bool:
        """Whether ``remap_px`` / ``launch(bytes_per_px=...)`` takes this plan with this pixel size (pb_remap_px_supported): a prepared plan
        of a single source in a tile mode.  A size outside PX_SIZES is a PbError.  Needs no GPU."""
        r = load().pb_remap_px_supported(self._h, int(bytes_per_px))
        if r < 0:
            check(r)
        return r == 1

    def launch_px_interp(self, src_ptr: int, dst_ptr: int, n_frames: int, channels: int, sample_bytes: int, interpolation: str, stream: int | None = None,
                         src_stride: int = 0, dst_stride: int = 0) -> None:
        """The raw interpolating call for frames of ``channels`` samples of ``sample_bytes`` bytes a pixel (pb_remap_interp_px):
        ``interpolation`` is "bilinear" or "catmull-rom" ("nearest" is ``launch(bytes_per_px=...)``).  The plan needs the bilinear mode's
        tables (``Plan(..., bilinear=True)`` or ``ensure_bilinear()``); a plan ``px_interp_supported`` refuses is a PbError."""
        check_interpolation(interpolation)
        if interpolation == "nearest":
            raise ValueError("launch_px_interp samples with 'bilinear' or 'catmull-rom': nearest sampling is launch(bytes_per_px=...)")
        self._gated(load().pb_remap_interp_px, self._h, src_ptr, dst_ptr, int(n_frames), int(src_stride), int(dst_stride), int(channels), int(sample_bytes),
                    TRACK_INTERP_IDS[interpolation], current_stream() if stream is None else stream)

    def px_interp_supported(self, channels: int, sample_bytes: int, interpolation: str) -> bool:
        """Whether ``launch_px_interp`` takes this plan with this format (pb_remap_interp_px_supported): a prepared plan of a camera or
        panorama source in a tile mode with the bilinear mode's tables; three uint8 channels are the RGB call's, which every plan takes.
        channels outside 1..4 or sample_bytes outside (1, 2) is a PbError.  Needs no GPU."""
        check_interpolation(interpolation)
        if interpolation == "nearest":
            raise ValueError("px_interp_supported asks about 'bilinear' or 'catmull-rom': nearest sampling is px_supported")
        r = load().pb_remap_interp_px_supported(self._h, int(channels), int(sample_bytes), TRACK_INTERP_IDS[interpolation])
        if r < 0:
            check(r)
        return r == 1

    def px_interp_route(self, channels: int, sample_bytes: int, interpolation: str) -> str:
        """Diagnostic (pb_plan_px_interp_route): what ``launch_px_interp`` launches on this plan - "tiles" (pb_px_interp_kernel), "float64"
        (the chain per pixel: a prepared plan whose coordinate tables cannot exist), "rgb8" (three uint8 channels) or "none"."""
        check_interpolation(interpolation)
        r = load().pb_plan_px_interp_route(self._h, int(channels), int(sample_bytes), TRACK_INTERP_IDS[interpolation])
        if r < 0:
            check(r)
        return ("none", "tiles", "float64", "rgb8")[r]

    def _remap_px_interp(self, src, out, interpolation: str):
        """``remap_px`` with an interpolating mode: the sampler looks inside the pixel - uint8 or uint16 samples, up to four channels."""
        sh, dh = (self.src.height, self.src.width), (self.dst.height, self.dst.width)
        if not is_device_array(src):
            raise PbError(f"source frames must be device arrays (CUDA tensors or DeviceArrays), got {type(src).__name__}")
        tens = is_tensor(src)
        shp = tuple(int(v) for v in src.shape)
        dt = torch_dtype_np(src.dtype) if tens else np.dtype(src.dtype)
        lead = 2 if shp[:2] == sh else 3  # (h, w[, C]), else (N, h, w[, C])
        if len(shp) not in (lead, lead + 1) or shp[lead - 2:lead] != sh:
            raise PbError(f"source frames must be ({sh[0]}, {sh[1]}), ({sh[0]}, {sh[1]}, C), (N, {sh[0]}, {sh[1]}) or (N, {sh[0]}, {sh[1]}, C), got {shp} {dt}")
        tail = shp[lead:]
        channels = tail[0] if tail else 1
        if dt not in (np.dtype(np.uint8), np.dtype(np.uint16)) or not 1 <= channels <= 4:
            raise PbError(f"{interpolation} sampling takes uint8 or uint16 frames of 1 to 4 channels, got {shp} {dt}")
        n = shp[0] if lead == 3 else 1
        oshape = ((n,) if lead == 3 else ()) + dh + tail
        if out is not None:
            odt = (torch_dtype_np(out.dtype) if is_tensor(out) else np.dtype(out.dtype)) if is_device_array(out) else None
            if odt != dt or tuple(out.shape) != oshape or is_tensor(out) != tens or (tens and not out.is_contiguous()):
                raise PbError(f"out must be a contiguous device array {oshape} {dt} of the source's kind")
            if tens and (not out.is_cuda or out.device != src.device):
                raise PbError(f"out must live on the source's device ({src.device}), got {out.device}")
        require_gpu()
        s = src.contiguous() if tens else src
        o = empty(oshape, dt, like=s) if out is None else out
        if n == 0:
            return o
        with _on(s):
            self.ensure_bilinear()  # (as ``remap`` does for uint8 RGB: the tables are built when an interpolating mode is first used)
            self.launch_px_interp(s.data_ptr(), o.data_ptr(), n, channels, dt.itemsize, interpolation)
        return o

    def launch_float(self, src_ptr: int, dst_ptr: int, n_frames: int, channels: int, sample_bytes: int, interpolation: str, stream: int | None = None,
                     src_stride: int = 0, dst_stride: int = 0) -> None:
        """The raw interpolating call for frames of ``channels`` float samples a pixel (pb_remap_interp_pxf): ``sample_bytes``
        2 is float16, 4 float32; ``interpolation`` is "bilinear" or "catmull-rom" ("nearest" moves bytes: ``launch(bytes_per_px=...)``).
        The plan needs the bilinear mode's tables (``Plan(..., bilinear=True)`` or ``ensure_bilinear()``); a plan ``float_supported``
        refuses is a PbError."""
        check_interpolation(interpolation)
        if interpolation == "nearest":
            raise ValueError("launch_float samples with 'bilinear' or 'catmull-rom': nearest sampling is launch(bytes_per_px=...)")
        self._gated(load().pb_remap_interp_pxf, self._h, src_ptr, dst_ptr, int(n_frames), int(src_stride), int(dst_stride), int(channels), int(sample_bytes),
                    TRACK_INTERP_IDS[interpolation], current_stream() if stream is None else stream)

    def float_supported(self, channels: int, sample_bytes: int, interpolation: str) -> bool:
        """Whether ``launch_float`` takes this plan with this format (pb_remap_interp_pxf_supported): a prepared plan of a camera or
        panorama source in a tile mode with the bilinear mode's coordinate tables.  channels outside 1..4 or sample_bytes outside (2, 4)
        is a PbError.  Needs no GPU."""
        check_interpolation(interpolation)
        if interpolation == "nearest":
            raise ValueError("float_supported asks about 'bilinear' or 'catmull-rom': nearest sampling is px_supported")
        r = load().pb_remap_interp_pxf_supported(self._h, int(channels), int(sample_bytes), TRACK_INTERP_IDS[interpolation])
        if r < 0:
            check(r)
        return r == 1

    def remap_float(self, src, out=None, *, interpolation: str = "bilinear"):
        """Bilinear or Catmull-Rom sampling of float16 / float32 frames - HDR panoramas, depth, flow, mattes - in ONE launch of the
        interpolating tile kernel (pb_remap_interp_pxf).  src: a device array (CUDA tensor or DeviceArray) (h, w), (h, w, C),
        (N, h, w) or (N, h, w, C) of float16 or float32, C <= 4 -> the same kind, dtype and shape at the destination size.  The value is
        the definition's sum narrowed once to the dtype: not rounded to an integer, not clipped (the cubic's overshoot is kept); +0.0 where
        the pixel is not live.  The bilinear mode's tables are built on first use; a plan ``float_supported`` then refuses is a PbError
        (no fallback).  "nearest" is a ValueError: ``remap_px`` moves float pixels as bytes."""
        check_interpolation(interpolation)
        if interpolation == "nearest":
            raise ValueError("remap_float samples with 'bilinear' or 'catmull-rom': nearest sampling of float frames is remap_px")
        sh, dh = (self.src.height, self.src.width), (self.dst.height, self.dst.width)
        if not is_device_array(src):
            raise PbError(f"source frames must be device arrays (CUDA tensors or DeviceArrays), got {type(src).__name__}")
        tens = is_tensor(src)
        shp = tuple(int(v) for v in src.shape)
        name = str(src.dtype).replace("torch.", "") if tens else np.dtype(src.dtype).name  # (bfloat16 has no NumPy dtype to convert to)
        if name not in ("float16", "float32"):
            raise PbError(f"remap_float takes float16 or float32 frames, got {shp} {name}")
        dt = np.dtype(name)
        lead = 2 if shp[:2] == sh else 3  # (h, w[, C]), else (N, h, w[, C])
        if len(shp) not in (lead, lead + 1) or shp[lead - 2:lead] != sh:
            raise PbError(f"source frames must be ({sh[0]}, {sh[1]}), ({sh[0]}, {sh[1]}, C), (N, {sh[0]}, {sh[1]}) or (N, {sh[0]}, {sh[1]}, C), got {shp} {dt}")
        tail = shp[lead:]
        channels = tail[0] if tail else 1
        if not 1 <= channels <= 4:
            raise PbError(f"remap_float takes frames of 1 to 4 channels, got {shp} {dt}")
        n = shp[0] if lead == 3 else 1
        oshape = ((n,) if lead == 3 else ()) + dh + tail
        if out is not None:
            odt = (str(out.dtype).replace("torch.", "") if is_tensor(out) else np.dtype(out.dtype).name) if is_device_array(out) else None
            if odt != name or tuple(out.shape) != oshape or is_tensor(out) != tens or (tens and not out.is_contiguous()):
                raise PbError(f"out must be a contiguous device array {oshape} {dt} of the source's kind")
            if tens and (not out.is_cuda or out.device != src.device):
                raise PbError(f"out must live on the source's device ({src.device}), got {out.device}")
        require_gpu()
        s = src.contiguous() if tens else src
        o = empty(oshape, dt, like=s) if out is None else out
        if n == 0:
            return o
        with _on(s):
            self.ensure_bilinear()  # (as ``remap_px`` does: the tables are built when an interpolating mode is first used)
            self.launch_float(s.data_ptr(), o.data_ptr(), n, channels, dt.itemsize, interpolation)
        return o

    def remap_px(self, src, out=None, *, interpolation: str = "nearest"):
        """The remap of frames of any pixel layout.  Nearest (pb_remap_px): src is a device array (h, w, *tail) or (N, h, w, *tail) of any
        dtype whose pixel - tail x itemsize - is 1, 2, 3, 4, 6 or 8 bytes (grey, grey16, RGB, RGBA, RGB16, RGBA16) -> (H, W, *tail) /
        (N, H, W, *tail) of the same dtype and kind, in ONE launch.  A plan ``px_supported`` refuses is a PbError (no fallback).
        ``interpolation`` "bilinear" or "catmull-rom" (pb_remap_interp_px) looks inside the pixel: (h, w), (h, w, C),
        (N, h, w) or (N, h, w, C) arrays of uint8 or uint16, C <= 4, the same kind back, in one launch of the interpolating tile kernel; the
        bilinear mode's tables are built on first use, and a plan ``px_interp_supported`` then refuses is a PbError (no fallback)."""
        if interpolation != "nearest":
            check_interpolation(interpolation)
            return self._remap_px_interp(src, out, interpolation)
        sh, dh = (self.src.height, self.src.width), (self.dst.height, self.dst.width)
        if not is_device_array(src):
            raise PbError(f"source frames must be device arrays (CUDA tensors or DeviceArrays), got {type(src).__name__}")
        tens = is_tensor(src)
        shp = tuple(int(v) for v in src.shape)
        dt = torch_dtype_np(src.dtype) if tens else np.dtype(src.dtype)
        bpp = pixel_bytes(shp, dt, sh)
        if bpp not in PX_SIZES:
            raise PbError(f"source frames must be ({sh[0]}, {sh[1]}, ...) or (N, {sh[0]}, {sh[1]}, ...) with pixels of {PX_SIZES} bytes, got {shp} {dt}")
        batched = shp[:2] != sh
        tail = shp[3:] if batched else shp[2:]
        n = shp[0] if batched else 1
        oshape = ((n,) if batched else ()) + dh + tail
        require_gpu()
        s = src.contiguous() if tens else src
        if out is None:
            o = empty(oshape, dt, like=s)
        else:
            o = out
            odt = (torch_dtype_np(o.dtype) if is_tensor(o) else np.dtype(o.dtype)) if is_device_array(o) else None
            if odt != dt or tuple(o.shape) != oshape or is_tensor(o) != tens or (tens and not o.is_contiguous()):
                raise PbError(f"out must be a contiguous device array {oshape} {dt} of the source's kind")
            if tens and (not o.is_cuda or o.device != s.device):
                raise PbError(f"out must live on the source's device ({s.device}), got {o.device}")
        with _on(s):
            self.launch(s.data_ptr(), o.data_ptr(), n, None, bytes_per_px=bpp)
        return o

    def nv12_supported(self, bytes_per_sample: int = 1, *, interpolation: str = "nearest") -> bool:
        """Whether ``remap_nv12`` takes this plan with samples of this size (pb_remap_nv12_supported): the plans ``px_supported`` takes,
        with even dimensions.  A size outside (1, 2) or an odd dimension is a PbError.  ``interpolation="bilinear"``: whether the
        bilinear call does (pb_remap_nv12_bilinear_supported): of those plans, the ones with the bilinear mode's tables.  Needs no GPU."""
        return self._video_supported(True, None, bytes_per_sample, interpolation)

    def launch_nv12(self, src_ptr: int, dst_ptr: int, n_frames: int = 1, stream: int | None = None, bytes_per_sample: int = 1, fill=None,
                    src_layout=None, dst_layout=None, *, interpolation: str = "nearest") -> None:
        """The raw call (pb_remap_nv12; ``interpolation="bilinear"``: pb_remap_nv12_bilinear): n_frames 4:2:0 semi-planar frames at src_ptr /
        dst_ptr on `stream`, layouts in bytes (None: packed), ``fill`` the (Y, U, V) samples of black pixels (None: video black)."""
        self._launch_video(True, None, None, src_ptr, dst_ptr, n_frames, stream, bytes_per_sample, fill, src_layout, dst_layout, interpolation)

    def remap_nv12(self, src, out=None, fill=None, src_layout=None, dst_layout=None, stream: int | None = None, *, interpolation: str = "nearest"):
        """The nearest remap of NV12 (uint8) or P010 / P016 (uint16) video frames in ONE launch (pb_remap_nv12): luma moves
        like a grey image, and the (U, V) pair of an output 2 x 2 block is the source pair at the block's top-left pixel's source position.
        src: a device array (3h/2, w) or (N, 3h/2, w), packed - or, with ``src_layout``, any 1-D uint8 / uint16 device buffer that holds
        the frames at that layout (then ``out`` is required with ``dst_layout``, or the result is packed).  -> (3H/2, W) / (N, 3H/2, W) of
        src's kind and dtype.  ``fill``: (Y, U, V) for black pixels (None: 16, 128, 128 scaled to the sample size).  Layouts: a
        (pitch, uv_offset, frame_stride) tuple, dict or pb_nv12_layout, in bytes, 0 = default.  A plan ``nv12_supported`` refuses is a
        PbError (no fallback).  ``interpolation="bilinear"`` (opt-in): luma is the bilinear mode's grey sample and a pair is
        sampled bilinearly on the pair plane at half its block's top-left pixel's coordinate; within 1 + R // 512 of the written definition
        (R the largest sample value), on plans prepared with ``bilinear=True``."""
        check_video_interpolation(interpolation)
        return self._remap_video(NV12, src, out, fill, src_layout, dst_layout, stream, interpolation)

    def launch_track_nv12(self, table_ptr: int, n_rot_per_frame: int, src_ptr: int, dst_ptr: int, n_frames: int = 1, stream: int | None = None,
                          bytes_per_sample: int = 1, fill=None, src_layout=None, dst_layout=None, *, interpolation: str = "nearest") -> None:
        """The raw rotation-track call for video frames (pb_remap_track_nv12; ``interpolation="bilinear"``: pb_remap_track_nv12_bilinear):
        ``launch_track``'s table, ``launch_nv12``'s frames, layouts and fill.  The table must stay alive and unchanged until the stream
        has run the launch."""
        self._launch_video(True, None, (table_ptr, n_rot_per_frame), src_ptr, dst_ptr, n_frames, stream, bytes_per_sample, fill, src_layout, dst_layout, interpolation)

    def remap_track_nv12(self, src, rotations, out=None, fill=None, src_layout=None, dst_layout=None, stream: int | None = None, *,
                         interpolation: str = "nearest"):
        """NV12 (uint8) or P010 / P016 (uint16) video frames with a rotation per frame in ONE launch (pb_remap_track_nv12):
        frame f is ``remap_nv12``'s definition with the index map of this plan's rotations followed by ``rotations[f]``.  ``src``, ``out``,
        ``fill`` and the layouts follow ``remap_nv12``'s rules, ``rotations`` follows ``rotation_table``'s as for ``remap_track``; the frame
        count must equal the table's (ValueError).  Any plan of a single source is served alike, a deferred one included.  Shapes, dtypes
        and counts are checked before any device work.  ``interpolation="bilinear"`` (opt-in, pb_remap_track_nv12_bilinear):
        frame f is ``remap_nv12``'s bilinear definition at the float64 coordinates of that chain - its bytes exactly, for either sample
        size; panorama and camera sources."""
        check_video_interpolation(interpolation)
        return self._remap_video(NV12, src, out, fill, src_layout, dst_layout, stream, interpolation, track=(rotations,))

    def planar_supported(self, subsampling, bytes_per_sample: int = 1, *, interpolation: str = "nearest") -> bool:
        """Whether ``remap_planar`` takes this plan with this subsampling and sample size (pb_remap_planar_supported): the plans
        ``px_supported`` takes.  A size outside (1, 2) or a dimension that breaks the subsampling's rule is a PbError.
        ``interpolation="bilinear"``: whether the bilinear call does (pb_remap_planar_bilinear_supported).  Needs no GPU."""
        return self._video_supported(False, subsampling, bytes_per_sample, interpolation)

    def launch_planar(self, src_ptr: int, dst_ptr: int, subsampling, n_frames: int = 1, stream: int | None = None, bytes_per_sample: int = 1, fill=None,
                      src_layout=None, dst_layout=None, *, interpolation: str = "nearest") -> None:
        """The raw call (pb_remap_planar; ``interpolation="bilinear"``: pb_remap_planar_bilinear): n_frames planar frames at src_ptr /
        dst_ptr on `stream`, layouts in bytes (None: packed), ``fill`` the samples of black pixels per plane (None: video black)."""
        self._launch_video(False, subsampling, None, src_ptr, dst_ptr, n_frames, stream, bytes_per_sample, fill, src_layout, dst_layout, interpolation)

    def remap_planar(self, src, subsampling, out=None, fill=None, src_layout=None, dst_layout=None, stream: int | None = None, *,
                     interpolation: str = "nearest"):
        """The nearest remap of PLANAR video frames - three planes of uint8 or uint16 samples at 4:4:4, 4:2:2 or 4:2:0 - in ONE launch
        (pb_remap_planar): plane 0 moves like a grey image, and a sample of planes 1 and 2 is the source sample at the source
        position of its block's top-left pixel.  src: a flat device array of one packed frame, or (N, frame_samples) - a 4:2:0 or 4:2:2
        frame is no rectangle; 4:4:4 also takes (3, h, w) / (N, 3, h, w) - or, with ``src_layout``, any 1-D buffer that holds the frames
        at that layout (then ``out`` is required with ``dst_layout``, or the result is packed).  -> the same shape for the destination.
        ``subsampling``: PLANAR_444 / PLANAR_422 / PLANAR_420 or "444" / "422" / "420".  ``fill``: the samples of black per plane (None:
        16, 128, 128 scaled to the sample size).  Layouts: a (pitch, chroma_pitch, offset1, offset2, frame_stride) tuple, dict or
        pb_planar_layout, in bytes, 0 = default.  A plan ``planar_supported`` refuses is a PbError (no fallback).
        ``interpolation="bilinear"`` (opt-in): plane 0 is the bilinear mode's grey sample; a sample of planes 1 and 2 is sampled
        bilinearly on its own plane at its block's top-left pixel's coordinate, halved where subsampled (chroma co-sited with that pixel);
        within 1 + R // 512 of the written definition (R the largest sample value), on plans prepared with ``bilinear=True``."""
        check_video_interpolation(interpolation)
        return self._remap_video(video_family(subsampling), src, out, fill, src_layout, dst_layout, stream, interpolation)

    def launch_track_planar(self, table_ptr: int, n_rot_per_frame: int, src_ptr: int, dst_ptr: int, subsampling, n_frames: int = 1, stream: int | None = None,
                            bytes_per_sample: int = 1, fill=None, src_layout=None, dst_layout=None, *, interpolation: str = "nearest") -> None:
        """The raw rotation-track call for planar frames (pb_remap_track_planar; ``interpolation="bilinear"``:
        pb_remap_track_planar_bilinear): ``launch_track``'s table, ``launch_planar``'s frames, layouts and fill.  The table must stay
        alive and unchanged until the stream has run the launch."""
        self._launch_video(False, subsampling, (table_ptr, n_rot_per_frame), src_ptr, dst_ptr, n_frames, stream, bytes_per_sample, fill, src_layout,
                           dst_layout, interpolation)

    def remap_track_planar(self, src, rotations, subsampling, out=None, fill=None, src_layout=None, dst_layout=None, stream: int | None = None, *,
                           interpolation: str = "nearest"):
        """Planar video frames with a rotation per frame in ONE launch (pb_remap_track_planar): frame f is ``remap_planar``'s
        definition with the index map of this plan's rotations followed by ``rotations[f]``.  ``src``, ``subsampling``, ``out``, ``fill``
        and the layouts follow ``remap_planar``'s rules, ``rotations`` follows ``rotation_table``'s as for ``remap_track``; the frame count
        must equal the table's (ValueError).  Any plan of a single source is served alike, a deferred one included.  Shapes, dtypes and
        counts are checked before any device work.  ``interpolation="bilinear"`` (opt-in, pb_remap_track_planar_bilinear):
        frame f is ``remap_planar``'s bilinear definition at the float64 coordinates of that chain - its bytes exactly, for either sample
        size; panorama and camera sources."""
        check_video_interpolation(interpolation)
        return self._remap_video(video_family(subsampling), src, out, fill, src_layout, dst_layout, stream, interpolation, track=(rotations,))

    def stitch_nv12_supported(self, bytes_per_sample: int = 1) -> bool:
        """Whether ``stitch_nv12`` takes this plan with samples of this size (pb_stitch_nv12_supported): prepared plans of a double-fisheye
        source in a tile mode, with even dimensions.  A size outside (1, 2) or an odd dimension is a PbError.  Needs no GPU."""
        return self._video_supported(True, None, bytes_per_sample, "nearest", stitch=True)

    def launch_stitch_nv12(self, src_ptr: int, dst_ptr: int, n_frames: int = 1, stream: int | None = None, bytes_per_sample: int = 1, fill=None,
                           src_layout=None, dst_layout=None) -> None:
        """The raw call (pb_stitch_nv12): ``launch_nv12``'s arguments, the source a side-by-side double fisheye."""
        self._launch_video(True, None, None, src_ptr, dst_ptr, n_frames, stream, bytes_per_sample, fill, src_layout, dst_layout, "nearest", stitch=True)

    def stitch_nv12(self, src, out=None, fill=None, src_layout=None, dst_layout=None, stream: int | None = None):
        """Stitches NV12 (uint8) or P010 / P016 (uint16) frames of a side-by-side DOUBLE FISHEYE in ONE launch (pb_stitch_nv12):
        every sample is the reference's blend of the two eyes' samples - luma at the pixel's two taps, the (U, V) pair of an output 2 x 2
        block at the taps of the block's top-left pixel, with that pixel's factors - exactly; ``fill`` only where neither eye is live.
        ``src``, ``out``, ``fill`` and the layouts follow ``remap_nv12``'s rules.  A plan ``stitch_nv12_supported`` refuses is a PbError
        (no fallback); a single source goes to ``remap_nv12``."""
        return self._remap_video(NV12, src, out, fill, src_layout, dst_layout, stream, "nearest", stitch=True)

    def stitch_planar_supported(self, subsampling, bytes_per_sample: int = 1) -> bool:
        """Whether ``stitch_planar`` takes this plan with this subsampling and sample size (pb_stitch_planar_supported).  Needs no GPU."""
        return self._video_supported(False, subsampling, bytes_per_sample, "nearest", stitch=True)

    def launch_stitch_planar(self, src_ptr: int, dst_ptr: int, subsampling, n_frames: int = 1, stream: int | None = None, bytes_per_sample: int = 1, fill=None,
                             src_layout=None, dst_layout=None) -> None:
        """The raw call (pb_stitch_planar): ``launch_planar``'s arguments, the source a side-by-side double fisheye."""
        self._launch_video(False, subsampling, None, src_ptr, dst_ptr, n_frames, stream, bytes_per_sample, fill, src_layout, dst_layout, "nearest", stitch=True)

    def stitch_planar(self, src, subsampling, out=None, fill=None, src_layout=None, dst_layout=None, stream: int | None = None):
        """Stitches PLANAR frames (4:4:4, 4:2:2 or 4:2:0; uint8 or uint16) of a side-by-side DOUBLE FISHEYE in ONE launch (pb_stitch_planar,
        DESIGN 3.20): plane 0 is the reference's stitch of a grey image, and a sample of planes 1 and 2 is the blend of the two eyes' samples
        at the taps of its block's top-left pixel, with that pixel's factors - exactly; at 4:4:4 with fill (0, 0, 0) the planes are the
        channels of ``remap`` of the RGB image built from the source planes.  ``src``, ``subsampling``, ``out``, ``fill`` and the layouts
        follow ``remap_planar``'s rules.  A plan ``stitch_planar_supported`` refuses is a PbError (no fallback)."""
        return self._remap_video(video_family(subsampling), src, out, fill, src_layout, dst_layout, stream, "nearest", stitch=True)

    def launch_stitch_track_nv12(self, table_ptr: int, n_rot_per_frame: int, src_ptr: int, dst_ptr: int, n_frames: int = 1, stream: int | None = None,
                                 bytes_per_sample: int = 1, fill=None, src_layout=None, dst_layout=None) -> None:
        """The raw rotation-track call for frames of a side-by-side double fisheye (pb_track_stitch_nv12): ``launch_track_nv12``'s
        arguments.  The table must stay alive and unchanged until the stream has run the launch."""
        self._launch_video(True, None, (table_ptr, n_rot_per_frame), src_ptr, dst_ptr, n_frames, stream, bytes_per_sample, fill, src_layout, dst_layout, "nearest",
                           stitch=True)

    def stitch_track_nv12(self, src, rotations, out=None, fill=None, src_layout=None, dst_layout=None, stream: int | None = None):
        """Stitches NV12 (uint8) or P010 / P016 (uint16) frames of a side-by-side DOUBLE FISHEYE with a rotation per frame in ONE launch
        (pb_track_stitch_nv12): frame f is ``stitch_nv12``'s definition with the taps and factors of this plan's rotations
        followed by ``rotations[f]`` - exactly what ``stitch_nv12`` writes from a prepared plan of that whole chain.  ``src``, ``out``,
        ``fill`` and the layouts follow ``remap_nv12``'s rules, ``rotations`` follows ``rotation_table``'s as for ``remap_track``; the frame
        count must equal the table's (ValueError).  Any plan of a double fisheye is served alike, a deferred one included; a single
        source goes to ``remap_track_nv12``."""
        return self._remap_video(NV12, src, out, fill, src_layout, dst_layout, stream, "nearest", track=(rotations,), stitch=True)

    def launch_stitch_track_planar(self, table_ptr: int, n_rot_per_frame: int, src_ptr: int, dst_ptr: int, subsampling, n_frames: int = 1,
                                   stream: int | None = None, bytes_per_sample: int = 1, fill=None, src_layout=None, dst_layout=None) -> None:
        """The raw rotation-track call for planar frames of a side-by-side double fisheye (pb_track_stitch_planar):
        ``launch_track_planar``'s arguments.  The table must stay alive and unchanged until the stream has run the launch."""
        self._launch_video(False, subsampling, (table_ptr, n_rot_per_frame), src_ptr, dst_ptr, n_frames, stream, bytes_per_sample, fill, src_layout, dst_layout,
                           "nearest", stitch=True)

    def stitch_track_planar(self, src, rotations, subsampling, out=None, fill=None, src_layout=None, dst_layout=None, stream: int | None = None):
        """Stitches PLANAR frames (4:4:4, 4:2:2 or 4:2:0; uint8 or uint16) of a side-by-side DOUBLE FISHEYE with a rotation per frame in
        ONE launch (pb_track_stitch_planar): frame f is ``stitch_planar``'s definition with the taps and factors of this
        plan's rotations followed by ``rotations[f]`` - exactly; at 4:4:4 uint8 with fill (0, 0, 0) the planes are the channels of
        ``remap_track``'s frame f.  ``src``, ``subsampling``, ``out``, ``fill`` and the layouts follow ``remap_planar``'s rules,
        ``rotations`` follows ``rotation_table``'s; the frame count must equal the table's (ValueError).  Any plan of a double fisheye
        is served alike, a deferred one included; a single source goes to ``remap_track_planar``."""
        return self._remap_video(video_family(subsampling), src, out, fill, src_layout, dst_layout, stream, "nearest", track=(rotations,), stitch=True)

    # the one path behind the video methods above (the stitch methods of a double-fisheye source included: `stitch`); `pairs`, `sub`: a VideoFamily's members - in the raw calls the subsampling as the caller
    # gave it, checked where the library's argument stands
    def _video_supported(self, pairs, sub, bytes_per_sample, interpolation, stitch=False) -> bool:
        fn = getattr(load(), _STITCH_FUNCTIONS[pairs, True] if stitch else _VIDEO_FUNCTIONS[pairs, False, check_video_interpolation(interpolation), True])
        r = fn(self._h, int(bytes_per_sample)) if pairs else fn(self._h, planar_subsampling(sub), int(bytes_per_sample))
        if r < 0:
            check(r)
        return r == 1

    def _launch_video(self, pairs, sub, table, src_ptr, dst_ptr, n_frames, stream, bytes_per_sample, fill, src_layout, dst_layout, interpolation, stitch=False) -> None:
        """The raw call; table: None, or the (pointer, rotations per frame) of a rotation track's table; stitch: the stitch calls' twin."""
        name = _VIDEO_FUNCTIONS[pairs, table is not None, check_video_interpolation(interpolation), False]
        if stitch:
            name = _STITCH_FUNCTIONS[pairs, False] if table is None else _TRACK_STITCH_FUNCTIONS[pairs]
        fn = getattr(load(), name)
        f = None if fill is None else _FILL(*[int(v) for v in fill])
        to_layout = nv12_layout if pairs else planar_layout
        sl, dl = to_layout(src_layout), to_layout(dst_layout)
        self._gated(fn, self._h, *(() if table is None else (table[0], int(table[1]))), src_ptr, dst_ptr, int(n_frames), None if sl is None else C.addressof(sl),
                    None if dl is None else C.addressof(dl), *(() if pairs else (planar_subsampling(sub),)), int(bytes_per_sample), None if f is None else C.addressof(f),
                    current_stream() if stream is None else stream)

    def _remap_video(self, fam, src, out, fill, src_layout, dst_layout, stream, interpolation, track=None, stitch=False):
        """``remap_nv12`` / ``remap_planar`` and, with track = (rotations,), their rotation tracks: the source checks, the table's, the
        ``out`` checks, one launch."""
        source = self._video_source(fam, src, src_layout)
        if track is not None:
            n = source[-1]
            tab, n_tab, k = rotation_table(track[0], self.n_rot)
            if n_tab != n:
                raise ValueError(f"{n} frames need {n} rotations, the table holds {n_tab}")
        s, o, n, S, sl, dl = self._video_out(*source, out, dst_layout)
        with _on(s):
            if track is None:
                self._launch_video(*fam, None, s.data_ptr(), o.data_ptr(), n, stream, S, fill, sl, dl, interpolation, stitch=stitch)
            else:
                st = current_stream() if stream is None else stream
                tab, release = self._track_table(tab, s, st)
                self._launch_video(*fam, (tab.data_ptr(), k), s.data_ptr(), o.data_ptr(), n, st, S, fill, sl, dl, interpolation, stitch=stitch)
                release()
        return o

    def _video_source(self, fam, src, src_layout):
        """The source checks of the video methods -> (src, family, its shape, dtype, layout, frame count).  Needs no GPU."""
        h, w = self.src.height, self.src.width
        if not is_device_array(src):
            raise PbError(f"source frames must be device arrays (CUDA tensors or DeviceArrays), got {type(src).__name__}")
        dt = torch_dtype_np(src.dtype) if is_tensor(src) else np.dtype(src.dtype)
        fam.check(h, w, self.dst.height, self.dst.width, dt)
        shp = tuple(int(v) for v in src.shape)
        S = dt.itemsize
        sl = fam.layout(src_layout)
        if sl is None:
            frames = fam.packed(h, w)
            if shp not in frames and shp[1:] not in frames:
                raise PbError(fam.packed_error(h, w, shp))
            n = 1 if shp in frames else shp[0]
        else:
            if len(shp) != 1:
                raise PbError(f"frames at a layout come as a 1-D buffer, got {shp}")
            span, stride = fam.frame_bytes(sl, h, w, S)
            n = 0 if shp[0] * S < span else (shp[0] * S - span) // stride + 1
            if n < 1:
                raise PbError(f"the source buffer holds {shp[0] * S} bytes, a frame at this layout spans {span}")
        return src, fam, shp, dt, sl, n

    def _video_out(self, src, fam, shp, dt, sl, n, out, dst_layout):
        """... and their ``out`` checks (allocating it when None) -> (source, out, frame count, sample size, the two layouts)."""
        h, w, Hd, Wd, S = self.src.height, self.src.width, self.dst.height, self.dst.width, dt.itemsize
        tens = is_tensor(src)
        dl = fam.layout(dst_layout)
        if dl is not None:
            fam.frame_bytes(dl, Hd, Wd, S)
        require_gpu()
        s = src.contiguous() if tens else src
        # the destination in the source's form: one frame or a batch of the same one of the family's packed shapes (frames at a layout: the first)
        frames, frames_out = fam.packed(h, w), fam.packed(Hd, Wd)
        batched = sl is None and shp not in frames
        form = 0 if sl is not None else frames.index(shp[1:] if batched else shp)
        packed_out = ((n,) if batched else ()) + frames_out[form]
        if out is None:
            if dl is not None:
                raise PbError("a destination layout needs the `out` buffer it describes")
            o = empty(packed_out if sl is None else (n,) + frames_out[0], dt, like=s)
        else:
            o = out
            odt = (torch_dtype_np(o.dtype) if is_tensor(o) else np.dtype(o.dtype)) if is_device_array(o) else None
            if odt != dt or is_tensor(o) != tens or (tens and not o.is_contiguous()):
                raise PbError(f"out must be a contiguous {dt} device array of the source's kind")
            oshp = tuple(int(v) for v in o.shape)
            if dl is None:
                if oshp not in (packed_out, (n,) + frames_out[0]):
                    raise PbError(f"out must be {packed_out}, got {oshp}")
            else:
                span, stride = fam.frame_bytes(dl, Hd, Wd, S)
                have = int(np.prod(oshp)) * S
                if have < (n - 1) * stride + span:
                    raise PbError(f"out holds {have} bytes, {n} frames at this layout span {(n - 1) * stride + span}")
            if tens and (not o.is_cuda or o.device != s.device):
                raise PbError(f"out must live on the source's device ({s.device}), got {o.device}")
        return s, o, n, S, sl, dl

    def remap_each(self, srcs, outs=None, stream: int | None = None):
        """A batch of SEPARATELY ALLOCATED frames (a ring of buffers) in one launch (``pb_remap_u8v``): srcs / outs are
        sequences of uint8 device arrays (h, w, 3) / (H, W, 3); returns the list of outputs (allocated when ``outs`` is None).
        Same bytes as one ``remap`` per frame, at the batch rate."""
        require_gpu()
        srcs = list(srcs)
        n = len(srcs)
        if n == 0:
            return []
        for s in srcs:
            u8 = is_device_array(s) and ((s.dtype == torch.uint8) if is_tensor(s) else (s.dtype == np.uint8))
            if not u8 or tuple(s.shape) != (self.src.height, self.src.width, 3) or (is_tensor(s) and not s.is_contiguous()):
                raise PbError(f"source frames must be contiguous uint8 device arrays ({self.src.height}, {self.src.width}, 3)")
        if outs is None:
            outs = [empty((self.dst.height, self.dst.width, 3), np.uint8, like=srcs[0]) for _ in range(n)]
        else:
            outs = list(outs)
            if len(outs) != n:
                raise PbError("outs must hold one array per source frame")
            for o in outs:
                u8 = is_device_array(o) and ((o.dtype == torch.uint8) if is_tensor(o) else (o.dtype == np.uint8))
                if not u8 or tuple(o.shape) != (self.dst.height, self.dst.width, 3) or (is_tensor(o) and not o.is_contiguous()):
                    raise PbError(f"outputs must be contiguous uint8 device arrays ({self.dst.height}, {self.dst.width}, 3)")
        sp = (C.c_void_p * n)(*[int(s.data_ptr()) for s in srcs])
        dp = (C.c_void_p * n)(*[int(o.data_ptr()) for o in outs])
        with _on(srcs[0]):
            self._gated(load().pb_remap_u8v, self._h, sp, dp, n, current_stream() if stream is None else stream)
        return outs

    def index_map(self, weights: bool = False, device=None):
        """int32 (H, W) index map, or for a double source (2, H, W) [+ float64 (2, H, W) weights]."""
        require_gpu()
        H, W = self.dst.height, self.dst.width
        shape = (2, H, W) if self.double_src else (H, W)
        idx = empty(shape, np.int32, device=device)
        w = empty((2, H, W), np.float64, like=idx) if (weights and self.double_src) else None
        with _on(idx):
            self._gated(load().pb_index_map_i32, self._h, idx.data_ptr(), w.data_ptr() if w is not None else None, current_stream())
        return (idx, w) if weights else idx


_WS_NULL: dict = {}  # device -> DeviceArray: the default stream's workspace when torch is absent (one per device, grown on demand)
_WS_LOCK = threading.Lock()


@contextlib.contextmanager
def _temporary_workspace(nbytes: int, stream: int):
    """A workspace for ONE launch on `stream` that the caller did not provide.  With torch: a block of its caching allocator, allocated on
    that stream - freed when the launch is queued, handed out again only to work ordered after it on the same stream (graph captures
    allocate from their own pool).  Without torch: the default stream shares one buffer per device (its work is ordered); any other stream
    gets a buffer of its own, released after the stream has drained."""
    if torch is not None and torch.cuda.is_available():
        cur = torch.cuda.current_stream()
        ts = cur if int(cur.cuda_stream) == int(stream or 0) else (torch.cuda.ExternalStream(int(stream)) if stream else torch.cuda.default_stream())
        with torch.cuda.stream(ts):
            buf = torch.empty((int(nbytes),), dtype=torch.uint8, device=torch.device("cuda", torch.cuda.current_device()))
        yield buf
        return
    if not stream:
        dev = current_device()
        with _WS_LOCK:
            buf = _WS_NULL.get(dev)
            if buf is None or buf.nbytes < nbytes:
                _WS_NULL.pop(dev, None)
                buf = _WS_NULL[dev] = DeviceArray((int(nbytes),), np.uint8)
        yield buf
        return
    buf = DeviceArray((int(nbytes),), np.uint8)
    try:
        yield buf
    finally:
        check(load().pb_stream_sync(stream))
        del buf


def box_reduce(x, n: int):
    """(n H, n W, *trailing) uint8 / uint16 device array -> (H, W, *trailing) of n x n block means, round half to even (pb_box_reduce)."""
    require_gpu()
    shp = tuple(int(v) for v in x.shape)
    dt = np.dtype(torch_dtype_np(x.dtype)) if is_tensor(x) else np.dtype(x.dtype)
    if dt not in (np.dtype(np.uint8), np.dtype(np.uint16)):
        raise NotImplementedError(f"supersampling takes 8- or 16-bit unsigned samples, got {dt}")
    if shp[0] % n or shp[1] % n:
        raise ValueError(f"a ({shp[0]}, {shp[1]}) sample array is not divisible by supersample={n}")
    H, W, tail = shp[0] // n, shp[1] // n, shp[2:]
    channels = int(np.prod(tail, dtype=np.int64)) if tail else 1
    if is_tensor(x):
        x = x.contiguous()
    out = empty((H, W) + tail, dt, like=x)
    with _on(x):
        check(load().pb_box_reduce(x.data_ptr(), out.data_ptr(), H, W, channels, dt.itemsize, int(n), 1, current_stream()))
    return out


def torch_dtype_np(tdt) -> np.dtype:
    return torch.empty(0, dtype=tdt).numpy().dtype


def make_proj(kind: int, height: int, width: int, lens: int = 0, fov: float = 0.0, magnitude: float = 0.0, f_distance: float = 0.0) -> pb_proj:
    return pb_proj(int(kind), int(lens), int(height), int(width), float(fov), float(magnitude), float(f_distance))


def lens_polynomial(k, max_theta: float) -> int:
    """Registers a polynomial (Kannala-Brandt) lens with the library and returns its pb_lens id (the same coefficients and max_theta give
    the same id; process-local).  The library validates like core.lens.polynomial: PbError on a set it refuses.  Needs no GPU."""
    kk = (C.c_double * 4)(*[float(v) for v in k])
    out = C.c_int()
    check(load().pb_lens_polynomial(kk, float(max_theta), C.byref(out)))
    return out.value


def lens_polynomial_info(lens: int) -> tuple:
    """(k1, k2, k3, k4, max_theta) of a registered polynomial lens id."""
    kk = (C.c_double * 4)()
    mt = C.c_double()
    check(load().pb_lens_polynomial_info(int(lens), kk, C.byref(mt)))
    return (kk[0], kk[1], kk[2], kk[3], mt.value)


def coordmap(dst: pb_proj, device=None):
    require_gpu()
    out = empty((dst.height, dst.width, 3), np.float64, device=device)
    with _on(out):
        check(load().pb_coordmap_f64(C.byref(dst), out.data_ptr(), current_stream()))
    return out


def rotate(matrix: np.ndarray, cmap):
    """cmap (H, W, 3) float64 device array, contiguous; invalid lat/lon are zeroed in it."""
    require_gpu()
    m = np.ascontiguousarray(matrix, dtype=np.float64).reshape(9)
    out = empty(tuple(cmap.shape), np.float64, like=cmap)
    with _on(cmap):
        check(load().pb_rotate_f64(m.ctypes.data_as(C.POINTER(C.c_double)), cmap.data_ptr(), out.data_ptr(), cmap.shape[0], cmap.shape[1], current_stream()))
    return out


def sample_map(src: pb_proj, cmap, image):
    require_gpu()
    out = empty((cmap.shape[0], cmap.shape[1], 3), np.uint8, like=cmap)
    with _on(cmap):
        check(load().pb_sample_map_u8(C.byref(src), cmap.data_ptr(), cmap.shape[0], cmap.shape[1], image.data_ptr(), out.data_ptr(), current_stream()))
    return out


def index_from_map(src: pb_proj, cmap, dist_l=None, dist_r=None):
    """cmap (H, W, 3) float64 device array -> (int32 indices (H, W) or (2, H, W) for a double source, float64 weights (2, H, W) or None).
    Zeroes invalid lat/lon in cmap for a panorama source, like the reference."""
    require_gpu()
    H, W = cmap.shape[0], cmap.shape[1]
    double = src.kind == KIND_DOUBLE
    idx = empty((2, H, W) if double else (H, W), np.int32, like=cmap)
    w = empty((2, H, W), np.float64, like=cmap) if double else None
    for d in (dist_l, dist_r):
        if d is None:
            continue
        if is_tensor(d):
            ok = d.is_cuda and d.dtype == torch.float64 and d.is_contiguous() and d.numel() == H * W and (not is_tensor(cmap) or d.device == cmap.device)
        else:
            ok = isinstance(d, DeviceArray) and d.dtype == np.float64 and d.size == H * W
        if not ok:
            raise PbError("distance planes must be contiguous float64 CUDA tensors of the map's size on the map's device")
    with _on(cmap):
        check(load().pb_index_from_map_i32(C.byref(src), cmap.data_ptr(), H, W, dist_l.data_ptr() if dist_l is not None else None,
                                           dist_r.data_ptr() if dist_r is not None else None, idx.data_ptr(), w.data_ptr() if w is not None else None, current_stream()))
    return idx, w


def sample_map_interp(interpolation: str, src: pb_proj, cmap, img, channels: int, dt: np.dtype, dist_l=None, dist_r=None):
    """An interpolating mode ("bilinear", "catmull-rom") from a materialised float64 map (H, W, 3) on the device: img = the image's samples
    as a device array (h, w, channels) of dtype dt (uint8 / uint16) -> (H, W, channels), uint8 for a double-fisheye source
    (pb_sample_map_bilinear_px / pb_sample_map_catmull_rom_px)."""
    require_gpu()
    fn = {"bilinear": load().pb_sample_map_bilinear_px, "catmull-rom": load().pb_sample_map_catmull_rom_px}[interpolation]
    H, W = int(cmap.shape[0]), int(cmap.shape[1])
    dt = np.dtype(dt)
    out_dt = np.dtype(np.uint8) if src.kind == KIND_DOUBLE else dt
    out = empty((H, W, channels), out_dt, like=cmap)
    with _on(cmap):
        check(fn(C.byref(src), cmap.data_ptr(), H, W, dist_l.data_ptr() if dist_l is not None else None,
                 dist_r.data_ptr() if dist_r is not None else None, img.data_ptr(), out.data_ptr(), int(channels), dt.itemsize, current_stream()))
    return out


def sample_map_bilinear(src: pb_proj, cmap, img, channels: int, dt: np.dtype, dist_l=None, dist_r=None):
    return sample_map_interp("bilinear", src, cmap, img, channels, dt, dist_l, dist_r)


def sample_map_catmull_rom(src: pb_proj, cmap, img, channels: int, dt: np.dtype, dist_l=None, dist_r=None):
    return sample_map_interp("catmull-rom", src, cmap, img, channels, dt, dist_l, dist_r)


def gather_px(idx, img_bytes):
    """idx int32 (H, W), img_bytes uint8 (h, w, bpp) -> uint8 (H, W, bpp): src[idx] or zeros where idx < 0."""
    require_gpu()
    bpp = img_bytes.shape[2]
    n = int(idx.shape[0]) * int(idx.shape[1])
    out = empty((idx.shape[0], idx.shape[1], bpp), np.uint8, like=idx)
    with _on(idx):
        check(load().pb_gather_px(idx.data_ptr(), img_bytes.data_ptr(), out.data_ptr(), n, bpp, current_stream()))
    return out


def gather_blend(idx2, w2, img_bytes, channels: int, sample_bytes: int):
    """The double-fisheye blend of arbitrary-width images: uint8 (H * W * channels)."""
    require_gpu()
    n = int(idx2.shape[1]) * int(idx2.shape[2])
    out = empty((n * channels,), np.uint8, like=idx2)
    with _on(idx2):
        check(load().pb_gather_blend_u8(idx2.data_ptr(), w2.data_ptr(), img_bytes.data_ptr(), out.data_ptr(), n, channels, sample_bytes, current_stream()))
    return out


def map_projection(cmap):
    """cmap (H, W, 3) float64 device array, contiguous -> uint8 (H, W, 3); invalid lat/lon are zeroed in cmap."""
    require_gpu()
    out = empty((cmap.shape[0], cmap.shape[1], 3), np.uint8, like=cmap)
    ws = empty((3,), np.int64, like=cmap)
    with _on(cmap):
        check(load().pb_map_projection_u8(cmap.data_ptr(), cmap.shape[0], cmap.shape[1], out.data_ptr(), ws.data_ptr(), current_stream()))
    if int(to_host(ws)[2]) == 0:
        raise ValueError("zero-size array to reduction operation minimum which has no identity")  # np.min of no valid pixel
    return out


def synth_frame(height: int, width: int, frame: int = 0, seed: int = 0, circle_mask: int = 0, device=None, out=None):
    require_gpu()
    if out is None:
        out = empty((height, width, 3), np.uint8, device=device)
    with _on(out):
        check(load().pb_synth_frame_u8(out.data_ptr(), height, width, frame & 0xFFFFFFFF, seed & 0xFFFFFFFF, circle_mask, current_stream()))
    return out


def device_name() -> str:
    buf = C.create_string_buffer(256)
    check(load().pb_device_name(buf, 256))
    return buf.value.decode()
