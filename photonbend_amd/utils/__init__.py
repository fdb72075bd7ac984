"""Angle helpers and the panorama -> photo size rule, with the reference's operation order
(photonbend/utils/__init__.py:27-118), the cube map's face layout and the planes of a 4:2:0 semi-planar video frame (no reference
counterparts).  Host scalars and array views only; nothing here computes a pixel."""

import math
from typing import Callable, Dict, Tuple

__all__ = ["to_radians", "to_degrees", "calculate_size_panorama_to_photo", "CUBEMAP_FACES", "cubemap_faces", "cubemap_from_faces",
           "cubemap_face_rotation", "nv12_planes", "nv12_frame", "planar_planes", "planar_frame"]

# the six faces of a cube map in frame order: face k occupies rows (k // 3) N ... and columns (k % 3) N ... of the (2N, 3N) image
CUBEMAP_FACES = ("left", "front", "right", "up", "back", "down")
# face -> its (right, forward, up) world unit vectors; world axes are the rotation's: +x the panorama's centre column, +y its zenith,
# +z 90 degrees to the right of centre
_CUBEMAP_TRIPLES = {
    "left": ((1, 0, 0), (0, 0, -1), (0, 1, 0)),
    "front": ((0, 0, 1), (1, 0, 0), (0, 1, 0)),
    "right": ((-1, 0, 0), (0, 0, 1), (0, 1, 0)),
    "up": ((0, 0, 1), (0, 1, 0), (-1, 0, 0)),
    "back": ((0, 0, -1), (-1, 0, 0), (0, 1, 0)),
    "down": ((0, 0, 1), (0, -1, 0), (1, 0, 0)),
}


def cubemap_face_rotation(name: str):
    """The 3 x 3 float64 matrix of a face: its right, forward and up vectors as columns (exact 0 and +-1, determinant +1).  A face of a
    cube map is a 120-degree rectilinear camera of focal distance N / 2 behind a rotation with this matrix."""
    import numpy as np

    if name not in _CUBEMAP_TRIPLES:
        raise KeyError(f"no cube map face {name!r}: the faces are {', '.join(CUBEMAP_FACES)}")
    return np.array(_CUBEMAP_TRIPLES[name], dtype=np.float64).T + 0.0  # (+ 0.0: no negative zeros)


def _cubemap_n(shape) -> int:
    h, w = (int(shape[0]), int(shape[1])) if len(shape) >= 2 else (0, 0)
    n = h // 2
    if n < 1 or h != 2 * n or w != 3 * n:
        raise ValueError(f"a cube map has shape (2N, 3N) + trailing: six N x N faces in a 3 x 2 grid, got {tuple(shape)}")
    return n


def cubemap_faces(image) -> Dict[str, "object"]:
    """name -> the face's N x N (+ trailing) VIEW of a cube map image (an ndarray or anything sliceable the same way)."""
    n = _cubemap_n(tuple(image.shape))
    return {name: image[(k // 3) * n:(k // 3 + 1) * n, (k % 3) * n:(k % 3 + 1) * n] for k, name in enumerate(CUBEMAP_FACES)}


def cubemap_from_faces(faces):
    """The (2N, 3N) + trailing cube map of six equal square faces (a mapping by name): cubemap_faces' inverse, in NumPy.  Other layouts
    (6 x 1, 1 x 6, a cross) are rearrangements of the same six arrays on the host."""
    import numpy as np

    missing = [name for name in CUBEMAP_FACES if name not in faces]
    if missing or len(faces) != 6:
        raise ValueError(f"a cube map needs exactly the faces {', '.join(CUBEMAP_FACES)}")
    arrs = [np.asarray(faces[name]) for name in CUBEMAP_FACES]
    first = arrs[0]
    if first.ndim < 2 or first.shape[0] != first.shape[1] or first.shape[0] < 1:
        raise ValueError(f"cube map faces are square, got {first.shape}")
    if any(a.shape != first.shape or a.dtype != first.dtype for a in arrs):
        raise ValueError("cube map faces must share one shape and sample type")
    return np.concatenate([np.concatenate(arrs[:3], axis=1), np.concatenate(arrs[3:], axis=1)], axis=0)


def nv12_planes(frame):
    """(y, uv) VIEWS of a packed 4:2:0 semi-planar frame (3h/2, w) - NV12 (uint8) or P010 / P016 (uint16), an ndarray or anything
    sliceable and reshapeable the same way: y is (h, w), uv is (h/2, w/2, 2) with uv[i, j] the (U, V) pair of luma block (2i, 2j)."""
    shape = tuple(int(v) for v in frame.shape)
    if len(shape) != 2 or shape[0] % 3 or shape[1] % 2 or shape[0] < 3 or (shape[0] // 3 * 2) % 2:
        raise ValueError(f"a 4:2:0 semi-planar frame has shape (3h/2, w) with h and w even, got {shape}")
    h, w = shape[0] // 3 * 2, shape[1]
    return frame[:h], frame[h:].reshape(h // 2, w // 2, 2)


def nv12_frame(y, uv):
    """The packed (3h/2, w) frame of a luma plane (h, w) and a chroma plane (h/2, w/2, 2) of the same sample type: nv12_planes'
    inverse, in NumPy."""
    import numpy as np

    y, uv = np.asarray(y), np.asarray(uv)
    if y.ndim != 2 or y.shape[0] % 2 or y.shape[1] % 2 or uv.shape != (y.shape[0] // 2, y.shape[1] // 2, 2) or uv.dtype != y.dtype:
        raise ValueError(f"a luma plane (h, w) with h and w even and a chroma plane (h/2, w/2, 2) of its sample type, got {y.shape} {y.dtype} and {uv.shape} {uv.dtype}")
    return np.concatenate([y, uv.reshape(y.shape[0] // 2, y.shape[1])], axis=0)


def planar_planes(frame, h: int, w: int, subsampling):
    """(p0, p1, p2) VIEWS of one packed planar frame - a flat array of h * w + 2 * (h >> cy) * (w >> cx) samples, an ndarray or anything
    sliceable and reshapeable the same way: p0 is (h, w), p1 and p2 are (h >> cy, w >> cx).  ``subsampling``: "444", "422", "420" or the
    PLANAR_* ids of ``Plan.remap_planar`` ((cx, cy) = (0, 0), (1, 0), (1, 1)).  A 4:4:4 frame may also come as (3, h, w)."""
    from .. import _native as nat

    sub = nat.planar_subsampling(subsampling)
    cx, cy = nat.PLANAR_SHIFTS[sub]
    h, w = int(h), int(w)
    if h < 1 or w < 1 or not nat.planar_dims_ok(sub, (h, w)):
        raise ValueError(f"{nat.planar_dims_rule(sub)}, got {h} x {w}")
    shape = tuple(int(v) for v in frame.shape)
    if sub == nat.PLANAR_444 and shape == (3, h, w):
        return frame[0], frame[1], frame[2]
    n0, nc = h * w, (h >> cy) * (w >> cx)
    if shape != (n0 + 2 * nc,):
        raise ValueError(f"a packed planar frame of {h} x {w} is a flat array of {n0 + 2 * nc} samples, got {shape}")
    return frame[:n0].reshape(h, w), frame[n0 : n0 + nc].reshape(h >> cy, w >> cx), frame[n0 + nc :].reshape(h >> cy, w >> cx)


def planar_frame(p0, p1, p2):
    """The packed flat frame of three planes of one sample type, p1 and p2 of one shape (h >> cy, w >> cx) for one of the three
    subsamplings: planar_planes' inverse, in NumPy."""
    import numpy as np

    p0, p1, p2 = np.asarray(p0), np.asarray(p1), np.asarray(p2)
    ok = p0.ndim == 2 and p1.shape == p2.shape and p1.dtype == p0.dtype and p2.dtype == p0.dtype
    if ok:
        h, w = p0.shape
        ok = p1.shape in ((h, w), (h, w >> 1), (h >> 1, w >> 1)) and (p1.shape == (h, w) or not w & 1) and (p1.shape[0] == h or not h & 1)
    if not ok:
        raise ValueError(f"a plane (h, w) and two planes (h >> cy, w >> cx) of its sample type, got {p0.shape} {p0.dtype}, {p1.shape} {p1.dtype} and {p2.shape} {p2.dtype}")
    return np.concatenate([p0.ravel(), p1.ravel(), p2.ravel()])


def to_radians(degrees: float) -> float:
    """degrees -> radians as ``degrees / 180 * pi`` (divide first; utils/__init__.py:37)."""
    return degrees / 180 * math.pi


def to_degrees(radians: float) -> float:
    """radians -> degrees as ``radians / pi * 180.0`` (utils/__init__.py:50)."""
    return radians / math.pi * 180.0


def _lens_ratio(lens_function: Callable[[float], float]) -> float:
    # radius of the 360-degree circle over the radius of the 180-degree circle (utils/__init__.py:58-60, :72-74)
    return lens_function(math.pi) / lens_function(math.pi / 2)


def calculate_size_panorama_to_photo(
    panorama_size: Tuple[int, int],
    lens_function: Callable[[float], float],
    preserve_vertical_resolution: bool = False,
) -> Tuple[int, int]:
    """(width, height) of the inscribed photo that keeps a panorama's pixel detail (utils/__init__.py:81-118).

    Horizontal rule (:53-64): the panorama's equator is ``width`` pixels long, so the 180-degree circle of the
    photo gets the diameter ``width / pi`` and the full circle that times the lens's 360 / 180 radius ratio,
    rounded up.  With ``preserve_vertical_resolution`` the vertical rule (:67-78) - ``height`` over the smaller of
    the ratio and one minus it - wins when it asks for more.  A panorama that is not 2:1 trips the same assertion."""
    width, height = panorama_size
    assert width == 2 * height, "Equirectangular panoramas should have width and height in a 2:1 proportion"
    ratio = _lens_ratio(lens_function)
    side = int(math.ceil(width / math.pi * ratio))
    if preserve_vertical_resolution:
        small_side_factor = 1.0 / (1.0 - ratio if ratio > 0.5 else ratio)
        v_side = abs(int(math.ceil(height * small_side_factor)))
        if v_side > side:
            side = v_side
    return (side, side)
