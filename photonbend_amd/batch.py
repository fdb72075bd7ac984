"""Streaming many host-resident frames through one plan.

The remap itself takes tens of microseconds per frame; for frames that live in host memory the wall time is
PCIe (an 8192x4096 source is 1.8 ms of H2D, its 4096x4096 result 0.9 ms of D2H).  ``remap_frames`` keeps both
directions of the link busy: while frame k+1 uploads (one DMA out of the caller's page-locked array), the remap
kernel of frame k stores its output over PCIe straight into frame k's result ndarray, through ``depth`` rotating
device input buffers.  Outputs are yielded in order as fresh (page-locked, recycled) ndarrays.
"""

from __future__ import annotations

from typing import Iterable, Iterator

import numpy as np

from . import _hostpipe
from . import _native as nat
from .core.projection import _plan_for


def plan_for(dst_image, rotations, src_image, supersample: int = 1) -> nat.Plan:
    """The plan of ``src_image.process_coordinate_map(rotations(dst_image.get_coordinate_map(supersample)))``.
    ``rotations``: sequence of ``Rotation`` objects (or 3x3 matrices), applied in order.  ``supersample`` n: the plan of the n x
    destination - pass the same n to ``remap_frames``."""
    mats = [getattr(r, "rotation_matrix", r) for r in rotations]
    return _plan_for(dst_image._proj_ss(nat.check_supersample(supersample)), mats, src_image._proj("src"))


def remap_frames(plan: nat.Plan, frames: Iterable[np.ndarray], depth: int = 3, interpolation: str = "nearest",
                 supersample: int = 1, rotations=None, pixel_format: str | None = None) -> Iterator[np.ndarray]:
    """Remaps an iterable of uint8 (h, w, 3) ndarrays with ``plan``; yields uint8 (H, W, 3) ndarrays in order
    (``_hostpipe.remap_frames``: upload stream + launch stream, page-locked results the kernel writes directly, no PyTorch).
    ``supersample`` n: ``plan`` came from ``plan_for(..., supersample=n)``; the frames are (H, W, 3) block means of its n x output.
    ``interpolation``: "nearest", "bilinear" or "catmull-rom" (not supersampled) - checked here, before the first frame.
    ``rotations``: a rotation track (``core.rotation_track``, an array (N, 3, 3) / (N, k, 3, 3), a float64 device array or a sequence
    of ``Rotation`` objects) - frame f is remapped with the plan's own rotations followed by entry f's (``Plan.remap_track``); the table
    is uploaded once, before the first frame; a frame beyond its length is a ValueError at that frame; not supersampled.
    ``pixel_format``: "nv12" (uint8) or "p010" (uint16) - the frames are 4:2:0 semi-planar video frames (3h/2, w), a luma plane over a
    plane of interleaved (U, V) pairs, and the results (3H/2, W), each in one launch (``Plan.remap_nv12``): nearest, not
    supersampled, no rotation track, even dimensions.  The keyword is needed - such an array looks like a grey image.  A planar format
    of ``nat.PLANAR_FORMATS`` ("yuv420p", "yuv422p", "yuv444p", "yuv420p10le", ..., "gbrp"): the frames are flat arrays of three planes'
    samples and so are the results (``Plan.remap_planar``), under the same conditions.  None: as above."""
    n = nat.check_interpolation(interpolation, supersample)
    if pixel_format is not None:  # (here, before the first frame: the pipeline below is a generator)
        _hostpipe.check_video_call(pixel_format, interpolation, n, rotations)
    table = None
    if rotations is not None:
        if n > 1:
            raise ValueError("a rotation track is not supersampled: pass supersample=1")
        table = nat.rotation_table(rotations, plan.n_rot)
    return _hostpipe.remap_frames(plan, frames, depth, interpolation, supersample, table, pixel_format)
