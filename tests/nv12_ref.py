"""The definition of the 4:2:0 semi-planar remap (pb_remap_nv12), in NumPy only: what every NV12 / P010 test compares with.

idx is the reference's int32 index map of the plan, (H, W): an entry is r * w + c into the (h, w) source, or -1 for black.  H, W, h and w
are even.  Luma moves like a grey image.  The (U, V) pair of output block (i, j) is the source pair at the source position of the block's
ANCHOR, its top-left pixel (2i, 2j) - whatever the block's other three pixels are."""

import numpy as np


def remap_nv12(y, uv, idx, w, fill):
    """y (h, w), uv (h/2, w/2, 2), idx (H, W) int32, w the source width, fill = (fy, fu, fv) -> (Y_out (H, W), UV_out (H/2, W/2, 2))."""
    y, uv, idx = np.asarray(y), np.asarray(uv), np.asarray(idx)
    H, W = idx.shape
    h = y.shape[0]
    assert y.shape == (h, w) and uv.shape == (h // 2, w // 2, 2) and uv.dtype == y.dtype
    assert not (H | W | h | w) & 1, "4:2:0 frames have even dimensions"
    fy, fu, fv = fill
    r, c = np.divmod(np.where(idx < 0, 0, idx), w)
    y_out = np.where(idx < 0, np.asarray(fy, y.dtype), y[r, c]).astype(y.dtype)
    a = idx[0::2, 0::2]
    ra, ca = np.divmod(np.where(a < 0, 0, a), w)
    uv_out = uv[ra >> 1, ca >> 1].copy()
    uv_out[a < 0] = np.array([fu, fv], y.dtype)
    return y_out, uv_out


def default_fill(dtype):
    """Video black in the sample type: (16, 128, 128) << 8 * (itemsize - 1)."""
    sh = 8 * (np.dtype(dtype).itemsize - 1)
    return 16 << sh, 128 << sh, 128 << sh


def remap_frame(frame, idx, h, w, fill=None):
    """The same on a packed (3h/2, w) frame -> a packed (3H/2, W) frame."""
    frame = np.asarray(frame)
    y, uv = frame[:h], frame[h:].reshape(h // 2, w // 2, 2)
    yo, uvo = remap_nv12(y, uv, idx, w, default_fill(frame.dtype) if fill is None else fill)
    return np.concatenate([yo, uvo.reshape(yo.shape[0] // 2, yo.shape[1])], axis=0)
