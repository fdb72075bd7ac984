"""The written definition of the interpolating modes on float16 / float32 frames (pb_remap_interp_pxf): the integer modes'
definitions - oracle.reference_path.remap_bilinear and tests/catmull_rom_ref.remap - taken up to the sum, and
stopped there.

f is the reference's pre-truncation source coordinate, s = f - 0.5, i0 = floor(s), t = s - i0 per axis; rows clamped, a panorama's columns
wrapped modulo w, a camera's clamped.  Per channel, in float64:
  bilinear      top = a + tx (b - a), bot likewise, V = top + ty (bot - top).
  Catmull-Rom   Keys' weights with a = -0.5 (catmull_rom_ref.weights), the four row sums, then the column sum V.
No rounding to an integer and no clip: HDR samples have no range, and the cubic's overshoot and negative lobes are kept.  The result is V
narrowed once to the frame's sample type, round to nearest even (NumPy's astype); a float16 overflow is IEEE's infinity.  A pixel that is
not live is +0.0 in every channel.  A pixel whose taps hold a NaN or an infinity has an unspecified value; such a sample affects no other
pixel and never turns a dead pixel into anything but +0.0.

The coordinates and the liveness are the integer definitions' own code: orc.pano_positions for a panorama, orc.camera_positions with
_bilinear_camera's / catmull_rom_ref._camera's liveness test for a camera - the tap geometry cannot drift from theirs
(tests/test_pxf_host.py holds this file to them byte for byte on frames of integers)."""

from __future__ import annotations

import numpy as np

from oracle import reference_path as orc
from tests import catmull_rom_ref as crr

FILTERS = ("bilinear", "catmull-rom")
DTYPES = (np.dtype(np.float16), np.dtype(np.float32))


def positions(src_proj: orc.Proj, cmap: np.ndarray):
    """(fy, fx, live) of a materialised map on a panorama or camera source - remap_bilinear's / catmull_rom_ref.remap's coordinates and
    liveness; dead pixels sit at (0.5, 0.5) as there.  A panorama source zeroes the invalid lat / lon of `cmap` like the reference."""
    invalid = cmap[:, :, 2] != 0.0
    h, w = src_proj.height, src_proj.width
    with np.errstate(all="ignore"):
        if src_proj.kind == "camera":
            _, _, fy, fx = orc.camera_positions(src_proj, h, w, cmap[:, :, 0], cmap[:, :, 1])
            live = ~invalid & np.isfinite(fy) & np.isfinite(fx) & (fy >= 0) & (fy < h) & (fx >= 0) & (fx < w)
        elif src_proj.kind == "pano":
            _, _, _, fy, fx = orc.pano_positions(h, w, cmap)
            live = ~invalid & np.isfinite(fy) & np.isfinite(fx)
        else:
            raise ValueError(f"float frames are defined on panorama and camera sources, got {src_proj.kind!r}")
        return np.where(live, fy, 0.5), np.where(live, fx, 0.5), live


def tap_base(src_proj: orc.Proj, cmap: np.ndarray):
    """(i0, j0, ty, tx, live): the tap base floor(f - 0.5) per axis, unclamped and unwrapped, and the fractions."""
    fy, fx, live = positions(src_proj, cmap)
    sy, sx = fy - 0.5, fx - 0.5
    i0, j0 = np.floor(sy).astype(np.int64), np.floor(sx).astype(np.int64)
    return i0, j0, sy - i0, sx - j0, live


def remap_f64(src_proj: orc.Proj, image: np.ndarray, filt: str, cmap: np.ndarray) -> np.ndarray:
    """The float64 V, (H, W, C) - C = 1 for an (h, w) image -, zeros where the pixel is not live."""
    assert filt in FILTERS, filt
    assert image.dtype in DTYPES and image.ndim in (2, 3), (image.dtype, image.shape)
    img = (image[:, :, None] if image.ndim == 2 else image).astype(np.float64)
    h, w = src_proj.height, src_proj.width
    assert img.shape[:2] == (h, w), (img.shape, h, w)
    wrap = src_proj.kind == "pano"
    i0, j0, ty, tx, live = tap_base(src_proj, cmap)
    ty, tx = ty[..., None], tx[..., None]

    def col(j):
        return np.clip(j % w, 0, w - 1) if wrap else np.clip(j, 0, w - 1)

    with np.errstate(all="ignore"):
        if filt == "bilinear":
            r0, r1, c0, c1 = np.clip(i0, 0, h - 1), np.clip(i0 + 1, 0, h - 1), col(j0), col(j0 + 1)
            top = img[r0, c0] + tx * (img[r0, c1] - img[r0, c0])
            bot = img[r1, c0] + tx * (img[r1, c1] - img[r1, c0])
            v = top + ty * (bot - top)
        else:
            wy, wx = crr.weights(ty), crr.weights(tx)
            rows = [np.clip(i0 + k, 0, h - 1) for k in (-1, 0, 1, 2)]
            cols = [col(j0 + l) for l in (-1, 0, 1, 2)]
            v = None
            for k in range(4):
                r = wx[0] * img[rows[k], cols[0]]
                for l in range(1, 4):
                    r = r + wx[l] * img[rows[k], cols[l]]
                v = wy[0] * r if k == 0 else v + wy[k] * r
    v[~live] = 0.0
    return v


def remap(src_proj: orc.Proj, image: np.ndarray, filt: str, cmap: np.ndarray) -> np.ndarray:
    """V narrowed once to the image's dtype (round to nearest even), in the image's layout."""
    with np.errstate(all="ignore"):
        out = remap_f64(src_proj, image, filt, cmap).astype(image.dtype)
    return out[:, :, 0] if image.ndim == 2 else out
