"""Test-side definition of the opt-in Catmull-Rom mode: oracle.remap_bilinear's definition with a 4 x 4 footprint and Keys'
cubic weights (a = -0.5) in float64, in the order the device kernels evaluate them.  Shared by the Catmull-Rom test files."""

from __future__ import annotations

import warnings

import numpy as np

from oracle import reference_path as orc


def weights(t):
    """(w-1, w0, w1, w2) at fraction t, each evaluated in exactly this order."""
    return (((-0.5 * t + 1.0) * t - 0.5) * t, (1.5 * t - 2.5) * t * t + 1.0, ((-1.5 * t + 2.0) * t + 0.5) * t, (0.5 * t - 0.5) * t * t)


def sample(image: np.ndarray, fy, fx, live, wrap: bool) -> np.ndarray:
    """(h, w, C) samples at pre-truncation coordinates (fy, fx) where `live`, else 0: rows clamped, columns wrapped (wrap) or clamped;
    row sums, then the column sum, plain sequential adds; rint, clipped to the sample type's range."""
    h, w = image.shape[:2]
    with np.errstate(all="ignore"):
        fy = np.where(live, fy, 0.5)
        fx = np.where(live, fx, 0.5)
        sy, sx = fy - 0.5, fx - 0.5
        ry, rx = np.floor(sy), np.floor(sx)
        wy, wx = weights((sy - ry)[..., None]), weights((sx - rx)[..., None])
        i0, j0 = ry.astype(np.int64), rx.astype(np.int64)
        rows = [np.clip(i0 + k, 0, h - 1) for k in (-1, 0, 1, 2)]
        cols = [((j0 + l) % w) if wrap else np.clip(j0 + l, 0, w - 1) for l in (-1, 0, 1, 2)]
        img = image.astype(np.float64)
        v = None
        for k in range(4):
            r = wx[0] * img[rows[k], cols[0]]
            for l in range(1, 4):
                r = r + wx[l] * img[rows[k], cols[l]]
            v = wy[0] * r if k == 0 else v + wy[k] * r
        val = np.clip(np.rint(v), 0, np.iinfo(image.dtype).max).astype(image.dtype)
    val[~live] = 0
    return val


def _camera(p: orc.Proj, h: int, w: int, image: np.ndarray, lat, lon, invalid):
    """One fisheye (or one eye of a double frame) -> (values, live mask); bilinear's liveness."""
    with np.errstate(all="ignore"):
        _, _, fy, fx = orc.camera_positions(p, h, w, lat, lon)
        live = ~invalid & np.isfinite(fy) & np.isfinite(fx) & (fy >= 0) & (fy < h) & (fx >= 0) & (fx < w)
    return sample(image, fy, fx, live, False), live


def remap(dst: orc.Proj, src: orc.Proj, image: np.ndarray, rotations=(), cmap: np.ndarray = None) -> np.ndarray:
    """What process_coordinate_map(..., interpolation="catmull-rom") returns: remap_bilinear's structure (coordinates, liveness, the
    double-fisheye blend, grey / RGBA / 16-bit images) with the 4 x 4 sample.  `cmap`: a materialised (possibly edited) map instead of
    dst's and the rotations; a panorama source zeroes its invalid lat / lon in it like the reference."""
    if cmap is None:
        cmap = orc.coordinate_map(dst)
        for rot in rotations:
            cmap = orc.rotate_map(orc.rotation_matrix(*rot), cmap)
    if image.ndim == 2:
        if src.kind == "double":
            raise ValueError("operands could not be broadcast together")
        return remap(dst, src, image[:, :, None], rotations, cmap)[:, :, 0]
    invalid = cmap[:, :, 2] != 0.0
    h, w = src.height, src.width
    if src.kind == "double":
        left, right, w2 = orc._double_sides(src)
        lat = cmap[:, :, 0]
        fl, fr, lat_r = orc.double_weights(src, lat)
        l, _ = _camera(left, h, w2, image[:, :w2], lat, cmap[:, :, 1], invalid)
        r, _ = _camera(right, h, w - w2, np.copy(image[:, w2:])[:, ::-1], lat_r, cmap[:, :, 1], invalid)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            with np.errstate(all="ignore"):
                out = (l.astype(np.float64) * fl[..., None] + r.astype(np.float64) * fr[..., None]).astype(np.uint8)
        out[invalid] = 0
        return out
    if src.kind == "camera":
        val, _ = _camera(src, h, w, image, cmap[:, :, 0], cmap[:, :, 1], invalid)
        return val
    with np.errstate(all="ignore"):
        _, _, _, fy, fx = orc.pano_positions(h, w, cmap)
        live = ~invalid & np.isfinite(fy) & np.isfinite(fx)
    return sample(image, fy, fx, live, True)
