"""The definition of BILINEAR sampling of video frames (pb_remap_planar_bilinear, pb_remap_nv12_bilinear), in NumPy only: what
every test of those calls compares with.  The reference samples nearest only, so this file IS the oracle of the mode.

A frame is what tests/planar_ref.py / tests/nv12_ref.py describe: plane 0 is (h, w), planes 1 and 2 are (h >> cy, w >> cx) each (NV12 /
P010 carry them interleaved), (cx, cy) = (0, 0) at 4:4:4, (1, 0) at 4:2:2, (1, 1) at 4:2:0.

For output pixel (y, x), (fy, fx) is the reference's pre-truncation source coordinate and `live` its liveness, to the letter that of
oracle/reference_path.py: remap_bilinear - a panorama source: not invalid and finite; a camera source: additionally 0 <= fy < h and
0 <= fx < w.

  plane 0       remap_bilinear's grey-image definition: s = f - 0.5, i0 = floor(s), t = s - i0, taps i0 and i0 + 1 per axis; rows clamped,
                a panorama's columns wrapped, a camera's clamped; float64, in _bilinear_camera's order: top = a + tx (b - a), bot likewise,
                rint(top + ty (bot - top)).  fill[0] where the pixel is not live.
  planes 1, 2   sample (i, j) has the ANCHOR (i << cy, j << cx), as in the nearest definition.  Chroma is CO-SITED with its block's top-left
                luma pixel, in source and destination alike, so the anchor's coordinate in chroma sample units is s_c = (f - 0.5) / (1 << c)
                per axis; the same bilinear expression on the (h >> cy, w >> cx) plane, rows clamped to that plane, a panorama's columns
                wrapped modulo w >> cx.  fill[k] where the anchor is not live.  Only the anchor decides.
At 4:4:4 this is plane 0's rule: gbrp is three grey bilinear remaps."""

import numpy as np

from tests.planar_ref import SHIFTS, default_fill, dims_ok, planes


def tolerance(R):
    """T(R) = 1 + floor(R / 512): the tile kernels' coordinates are certified to 1/1024 px per axis and a bilinear value moves by at most R
    (the largest sample value of the source frame and the fills) per pixel of coordinate per axis, so the unrounded values differ by at
    most R / 512 and the rounded ones by at most T."""
    return 1 + int(R) // 512


def _bilinear(plane, sy, sx, wrap):
    """The bilinear expression at tap coordinates (sy, sx) = s on one plane, float64 -> float64 (rounded, not cast)."""
    h, w = plane.shape
    r0 = np.floor(sy).astype(np.int64)
    c0 = np.floor(sx).astype(np.int64)
    ty, tx = sy - r0, sx - c0
    r1, c1 = r0 + 1, c0 + 1
    r0, r1 = np.clip(r0, 0, h - 1), np.clip(r1, 0, h - 1)
    if wrap:
        c0, c1 = c0 % w, c1 % w
    c0, c1 = np.clip(c0, 0, w - 1), np.clip(c1, 0, w - 1)
    img = plane.astype(np.float64)
    top = img[r0, c0] + tx * (img[r0, c1] - img[r0, c0])
    bot = img[r1, c0] + tx * (img[r1, c1] - img[r1, c0])
    return np.rint(top + ty * (bot - top))


def remap_planar_bilinear(p0, p1, p2, fy, fx, live, src_kind, sub, fill):
    """p0 (h, w), p1 and p2 (h >> cy, w >> cx); fy, fx (H, W) float64 pre-truncation coordinates, live (H, W) bool; src_kind "pano" or
    "camera"; fill = (f0, f1, f2) -> the three output planes."""
    p0, p1, p2 = np.asarray(p0), np.asarray(p1), np.asarray(p2)
    fy, fx, live = np.asarray(fy, np.float64), np.asarray(fx, np.float64), np.asarray(live, bool)
    assert src_kind in ("pano", "camera"), src_kind
    cx, cy = SHIFTS[sub]
    h, w = p0.shape
    H, W = live.shape
    assert p1.shape == p2.shape == (h >> cy, w >> cx) and p1.dtype == p2.dtype == p0.dtype
    assert dims_ok(sub, (h, w), (H, W)), "widths are multiples of 1 << cx, heights of 1 << cy"
    wrap = src_kind == "pano"
    with np.errstate(all="ignore"):
        sy, sx = np.where(live, fy, 0.5) - 0.5, np.where(live, fx, 0.5) - 0.5
        out0 = np.where(live, _bilinear(p0, sy, sx, wrap), fill[0]).astype(p0.dtype)
        # the anchors: output pixels (i << cy, j << cx); their coordinate in chroma sample units
        la = live[0 :: 1 << cy, 0 :: 1 << cx]
        say, sax = sy[0 :: 1 << cy, 0 :: 1 << cx] / (1 << cy), sx[0 :: 1 << cy, 0 :: 1 << cx] / (1 << cx)
        outs = [out0]
        for plane, f in ((p1, fill[1]), (p2, fill[2])):
            outs.append(np.where(la, _bilinear(plane, say, sax, wrap), f).astype(p0.dtype))
    return tuple(outs)


def remap_frame(frame, fy, fx, live, src_kind, h, w, sub, fill=None):
    """The same on a packed flat frame -> a packed flat frame of the destination."""
    frame = np.asarray(frame)
    outs = remap_planar_bilinear(*planes(frame, h, w, sub), fy, fx, live, src_kind, sub, default_fill(frame.dtype) if fill is None else fill)
    return np.concatenate([o.ravel() for o in outs])


def remap_nv12(frame, fy, fx, live, src_kind, h, w, fill=None):
    """An NV12 / P010 frame (3h/2, w): the luma plane over the plane of interleaved (U, V) pairs -> (3H/2, W).  The planar definition at
    4:2:0 on the de-interleaved planes, interleaved again."""
    frame = np.asarray(frame)
    assert frame.shape == (3 * h // 2, w) and not (h | w) & 1
    uv = frame[h:].reshape(h // 2, w // 2, 2)
    o0, o1, o2 = remap_planar_bilinear(frame[:h], uv[:, :, 0], uv[:, :, 1], fy, fx, live, src_kind, "420", default_fill(frame.dtype) if fill is None else fill)
    H, W = o0.shape
    return np.concatenate([o0, np.stack([o1, o2], axis=2).reshape(H // 2, W)], axis=0)
