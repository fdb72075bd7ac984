"""The definition of the planar remap (pb_remap_planar), in NumPy only: what every planar test compares with, by equality.

A frame is three planes of one sample type.  Plane 0 is (h, w); planes 1 and 2 are (h >> cy, w >> cx) each, (cx, cy) = (0, 0) at 4:4:4,
(1, 0) at 4:2:2 and (1, 1) at 4:2:0.  idx is the reference's int32 index map of the plan, (H, W): an entry is r * w + c into the (h, w)
source, or -1 for black.  Plane 0 moves like a grey image.  A sample of planes 1 and 2 is the source sample at the source position of its
ANCHOR, the top-left pixel (i << cy, j << cx) of its block - whatever the block's other pixels are."""

import numpy as np

SHIFTS = {"444": (0, 0), "422": (1, 0), "420": (1, 1)}  # subsampling -> (cx, cy)
SUBSAMPLINGS = tuple(SHIFTS)


def dims_ok(sub, *shapes):
    """Widths are multiples of 1 << cx and heights of 1 << cy."""
    cx, cy = SHIFTS[sub]
    return not any((h & cy) | (w & cx) for h, w in shapes)


def frame_samples(h, w, sub):
    cx, cy = SHIFTS[sub]
    return h * w + 2 * (h >> cy) * (w >> cx)


def remap_planar(p0, p1, p2, idx, w, sub, fill):
    """p0 (h, w), p1 and p2 (h >> cy, w >> cx), idx (H, W) int32, w the source width, fill = (f0, f1, f2) -> the three output planes."""
    p0, p1, p2, idx = np.asarray(p0), np.asarray(p1), np.asarray(p2), np.asarray(idx)
    cx, cy = SHIFTS[sub]
    H, W = idx.shape
    h = p0.shape[0]
    assert p0.shape == (h, w) and p1.shape == p2.shape == (h >> cy, w >> cx) and p1.dtype == p2.dtype == p0.dtype
    assert dims_ok(sub, (h, w), (H, W)), "widths are multiples of 1 << cx, heights of 1 << cy"
    r, c = np.divmod(np.where(idx < 0, 0, idx), w)
    out0 = np.where(idx < 0, np.asarray(fill[0], p0.dtype), p0[r, c]).astype(p0.dtype)
    a = idx[0 :: 1 << cy, 0 :: 1 << cx]
    ra, ca = np.divmod(np.where(a < 0, 0, a), w)
    outs = [out0]
    for plane, f in ((p1, fill[1]), (p2, fill[2])):
        outs.append(np.where(a < 0, np.asarray(f, p0.dtype), plane[ra >> cy, ca >> cx]).astype(p0.dtype))
    return tuple(outs)


def default_fill(dtype):
    """pb_remap_nv12's video black in the sample type: (16, 128, 128) << 8 * (itemsize - 1)."""
    sh = 8 * (np.dtype(dtype).itemsize - 1)
    return 16 << sh, 128 << sh, 128 << sh


def planes(frame, h, w, sub):
    """The three plane views of a packed flat frame."""
    cx, cy = SHIFTS[sub]
    frame = np.asarray(frame)
    n0, nc = h * w, (h >> cy) * (w >> cx)
    assert frame.shape == (n0 + 2 * nc,)
    return frame[:n0].reshape(h, w), frame[n0 : n0 + nc].reshape(h >> cy, w >> cx), frame[n0 + nc :].reshape(h >> cy, w >> cx)


def remap_frame(frame, idx, h, w, sub, fill=None):
    """The same on a packed flat frame -> a packed flat frame of the destination."""
    frame = np.asarray(frame)
    outs = remap_planar(*planes(frame, h, w, sub), idx, w, sub, default_fill(frame.dtype) if fill is None else fill)
    return np.concatenate([o.ravel() for o in outs])
