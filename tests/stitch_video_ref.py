"""The definition of the double-fisheye video stitch (pb_stitch_planar / pb_stitch_nv12), in NumPy only: what every stitch
test compares with, by equality.

A frame is tests/planar_ref.py's: three planes of one sample type, plane 0 (h, w), planes 1 and 2 (h >> cy, w >> cx); the source is the
side-by-side double fisheye.  For every output pixel the reference's DoubleCameraImage.process_coordinate_map uses two taps and two
factors (oracle.reference_path.source_index of a "double" projection; on the device Plan.index_map(weights=True)):
    il, ir   int32 indices r * w + c into the FULL frame (the right eye's already mirrored), -1 = that eye is black there;
    fl, fr   float64 factors.
    blend(a_l, a_r) = cast((il < 0 ? 0.0 : a_l) * fl + (ir < 0 ? 0.0 : a_r) * fr)
The cast is NumPy's astype to an 8-bit integer as x86-64 does it, widened to the sample: non-finite or |v| >= 2^31 gives 0, otherwise
truncate toward zero and keep the low 8 * S bits.  Plane 0 is blend at the pixel's own taps, fill[0] where both are -1.  A sample (i, j)
of planes 1 and 2 is decided by its ANCHOR, output pixel (i << cy, j << cx): blend of the plane's samples at (r >> cy, c >> cx) of the
anchor's taps with the anchor's factors, fill[k] where both of the anchor's taps are -1."""

import numpy as np

from tests.planar_ref import SHIFTS, default_fill, dims_ok, frame_samples, planes  # noqa: F401  (the frame is the planar one)


def cast(v, dtype):
    """float64 -> uint8 / uint16 as the definition says (pb_cvt_u8 widened): never NumPy's own astype, whose result for values outside the
    target's range is the platform's."""
    v = np.asarray(v, np.float64)
    bits = 8 * np.dtype(dtype).itemsize
    with np.errstate(all="ignore"):
        ok = np.abs(v) < 2147483648.0  # (False for NaN and the infinities)
        t = np.trunc(np.where(ok, v, 0.0)).astype(np.int64)
    return (t & ((1 << bits) - 1)).astype(dtype)


def blend(plane, il, ir, fl, fr, w, cx, cy, fill):
    """One output plane: `plane` is (h >> cy, w >> cx) of the source, il / ir / fl / fr the taps and factors of the deciding pixels."""
    plane = np.asarray(plane)
    rl, cl = np.divmod(np.where(il < 0, 0, il), w)
    rr, cr = np.divmod(np.where(ir < 0, 0, ir), w)
    a_l = np.where(il < 0, 0.0, plane[rl >> cy, cl >> cx].astype(np.float64))
    a_r = np.where(ir < 0, 0.0, plane[rr >> cy, cr >> cx].astype(np.float64))
    with np.errstate(all="ignore"):
        v = a_l * fl + a_r * fr
    return np.where((il < 0) & (ir < 0), np.asarray(fill, plane.dtype), cast(v, plane.dtype)).astype(plane.dtype)


def stitch_planar(p0, p1, p2, il, ir, fl, fr, w, sub, fill):
    """p0 (h, w), p1 and p2 (h >> cy, w >> cx); il, ir (H, W) int32; fl, fr (H, W) float64; w the source width; fill = (f0, f1, f2)
    -> the three output planes."""
    p0, p1, p2 = np.asarray(p0), np.asarray(p1), np.asarray(p2)
    il, ir, fl, fr = np.asarray(il), np.asarray(ir), np.asarray(fl, np.float64), np.asarray(fr, np.float64)
    cx, cy = SHIFTS[sub]
    H, W = il.shape
    h = p0.shape[0]
    assert p0.shape == (h, w) and p1.shape == p2.shape == (h >> cy, w >> cx) and p1.dtype == p2.dtype == p0.dtype
    assert il.shape == ir.shape == fl.shape == fr.shape
    assert dims_ok(sub, (h, w), (H, W)), "widths are multiples of 1 << cx, heights of 1 << cy"
    out0 = blend(p0, il, ir, fl, fr, w, 0, 0, fill[0])
    a = (slice(0, None, 1 << cy), slice(0, None, 1 << cx))  # the anchors
    return out0, blend(p1, il[a], ir[a], fl[a], fr[a], w, cx, cy, fill[1]), blend(p2, il[a], ir[a], fl[a], fr[a], w, cx, cy, fill[2])


def stitch_frame(frame, il, ir, fl, fr, h, w, sub, fill=None):
    """The same on a packed flat frame -> a packed flat frame of the destination."""
    frame = np.asarray(frame)
    outs = stitch_planar(*planes(frame, h, w, sub), il, ir, fl, fr, w, sub, default_fill(frame.dtype) if fill is None else fill)
    return np.concatenate([o.ravel() for o in outs])


def nv12_of(frame, h, w):
    """A packed yuv420p frame as NV12 / P010: the luma plane, then the chroma planes interleaved pair by pair."""
    p0, p1, p2 = planes(np.asarray(frame), h, w, "420")
    return np.concatenate([p0.ravel(), np.stack([p1, p2], axis=2).ravel()])


def oracle_taps(case):
    """(il, ir, fl, fr) of a tests.cases.Case with a double-fisheye source, from the CPU oracle."""
    from oracle import reference_path as orc
    from tests import helpers as H

    with np.errstate(all="ignore"):
        il, ir, fl, fr, _ = orc.remap_index(H.orc_proj(case.dst), H.orc_proj(case.src), H.orc_rots(case))
    return il, ir, fl, fr
