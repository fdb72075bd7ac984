"""TEST INFRASTRUCTURE ONLY - the equi-angular cube map's definition, written once in NumPy on top of the cube map's
(tests/cubemap_ref.py) and the stage functions of oracle/reference_path.py.

An equi-angular cube is the cube in everything - frame layout, world axes, face matrices, face selection, face camera (rectilinear,
fov 2 pi / 3, f_distance exactly N / 2), truncation with its (-1, 0) -> 0 quirk, per-face clamp of interpolating taps, black half-texel
strip - except that the position on a face is proportional to the ANGLE from the face centre instead of its tangent.  The only new things
are two functions of a centred face coordinate c in pixels, every operation rounded on its own in this nesting:

    warp(c)   = np.tan((c / half) * Q) * half          EAC face coordinate -> gnomonic face coordinate
    unwarp(c) = (np.arctan(c / half) * IQ) * half      and back

with half = N / 2, Q = math.pi / 4 and IQ = 4 / math.pi, evaluated on CONTIGUOUS float64 arrays (what reaches the NumPy loops that
csrc/pb_math_np.hpp / pb_math_libm.hpp restate).  `warp` and `unwarp` are module attributes looked up at call time: with both replaced by
the identity this module IS tests/cubemap_ref.py, bit for bit (tests/test_eac_host.py)."""

from __future__ import annotations

import contextlib
import math
import warnings

import numpy as np

from oracle import reference_path as orc
from tests import cubemap_ref as cr

Q = math.pi / 4  # 0x1.921fb54442d18p-1
IQ = 4 / math.pi  # 0x1.45f306dc9c883p+0
assert Q.hex() == "0x1.921fb54442d18p-1" and IQ.hex() == "0x1.45f306dc9c883p+0"

FACES, face_matrix, face_proj, face_size, select_face, _face_maps = cr.FACES, cr.face_matrix, cr.face_proj, cr.face_size, cr.select_face, cr._face_maps


def _arr(c) -> np.ndarray:
    a = np.ascontiguousarray(c, dtype=np.float64)
    return a if a.ndim else a.reshape(1)  # (never a Python or NumPy scalar: the array loops are the definition)


def warp(c, half: float) -> np.ndarray:
    with np.errstate(all="ignore"):
        return np.tan((_arr(c) / half) * Q) * half


def unwarp(c, half: float) -> np.ndarray:
    with np.errstate(all="ignore"):
        return (np.arctan(_arr(c) / half) * IQ) * half


def face_coordinate_map(n: int) -> np.ndarray:
    """One face's camera map (before its rotation): oracle.coordinate_map's camera branch with the mesh vectors warped."""
    p = face_proj(n)
    x = warp(np.linspace(-n / 2 + 0.5, n / 2 - 0.5, num=n), n / 2).reshape(n)[None, :]
    y = warp(np.linspace(n / 2 - 0.5, -n / 2 + 0.5, num=n), n / 2).reshape(n)[:, None]
    d = np.sqrt(x**2 + y**2) / p.f_distance
    lat = orc.lens_inverse(p.lens, d)
    lon = orc._atan2_via_clog(x, y)
    invalid = lat > p.fov / 2
    out = np.empty(lat.shape + (3,), np.float64)
    out[:, :, 0] = lat
    out[:, :, 1] = lon
    out[:, :, 2] = invalid
    return out


def coordinate_map(n: int) -> np.ndarray:
    """The EAC DESTINATION's coordinate map (2N, 3N, 3): per face the warped face camera's map after one rotate_map with M_face."""
    out = np.empty((2 * n, 3 * n, 3), np.float64)
    for k in range(6):
        out[(k // 3) * n:(k // 3 + 1) * n, (k % 3) * n:(k % 3 + 1) * n] = orc.rotate_map(face_matrix(k), face_coordinate_map(n))
    return out


def camera_positions(p: orc.Proj, h: int, w: int, lat, lon):
    """oracle.camera_positions up to z = exp(1j lon) dist; then the position on the face through unwarp."""
    cy, cx = h / 2 - 0.5, w / 2 - 0.5
    half = p.f_distance  # N / 2 exactly (face_proj)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with np.errstate(all="ignore"):
            dist = orc.lens_forward(p.lens, lat) * p.f_distance
            z = np.exp(lon * 1j) * dist
            pre_y = (unwarp(z.imag, half).reshape(z.shape) * (-1)) + cy
            pre_x = unwarp(z.real, half).reshape(z.shape) + cx
    return orc._to_int(pre_y), orc._to_int(pre_x), pre_y, pre_x


@contextlib.contextmanager
def _positions():
    """The camera definitions of the oracle and of tests/catmull_rom_ref.py with the position function substituted."""
    saved = orc.camera_positions
    orc.camera_positions = camera_positions
    try:
        yield
    finally:
        orc.camera_positions = saved


def source_index(n: int, cmap: np.ndarray) -> np.ndarray:
    """int32 linear index into the full (2N, 3N) frame per entry of the map, -1 where the output is black."""
    face = select_face(cmap)
    p = face_proj(n)
    out = np.full(cmap.shape[:2], -1, np.int64)
    with _positions():
        for k, fm in enumerate(_face_maps(cmap)):
            py, px, black, _, _ = orc.camera_index(p, n, n, fm)
            idx = (py + (k // 3) * n) * (3 * n) + px + (k % 3) * n
            idx[black] = -1
            out = np.where(face == k, idx, out)
    return out.astype(np.int32)


def pretrunc(n: int, cmap: np.ndarray):
    """(face, pre_y, pre_x): the selected face and the pre-truncation position on it (face-local pixels)."""
    face = select_face(cmap)
    p = face_proj(n)
    fy = np.zeros(cmap.shape[:2])
    fx = np.zeros(cmap.shape[:2])
    for k, fm in enumerate(_face_maps(cmap)):
        _, _, pre_y, pre_x = camera_positions(p, n, n, fm[:, :, 0], fm[:, :, 1])
        fy = np.where(face == k, pre_y, fy)
        fx = np.where(face == k, pre_x, fx)
    return face, fy, fx


def sample(image: np.ndarray, cmap: np.ndarray) -> np.ndarray:
    """eac.process_coordinate_map(cmap): image is (2N, 3N) + trailing, any sample type."""
    n = face_size(*image.shape[:2])
    idx = source_index(n, cmap)
    flat = image.reshape((-1,) + image.shape[2:])
    out = flat[np.maximum(idx, 0)]
    out[idx < 0] = 0
    return out


def remap_bilinear(image: np.ndarray, cmap: np.ndarray) -> np.ndarray:
    with _positions():
        return cr.remap_bilinear(image, cmap)


def remap_catmull_rom(image: np.ndarray, cmap: np.ndarray) -> np.ndarray:
    with _positions():
        return cr.remap_catmull_rom(image, cmap)


# ---- whole remaps: projections are tests/cases.py tuples with the kinds "cube" (tests/cubemap_ref.py) and "eac" = ("eac", 2N, 3N, ...) ----
def eac(n: int):
    return ("eac", 2 * n, 3 * n, "equidistant", 0.0, None)


def stages(case, lens_of=None):
    """The float64 maps after the destination's coordinate map and after each rotation."""
    kind, h, w = case.dst[:3]
    if kind != "eac":
        return cr.stages(case, lens_of)
    m = coordinate_map(face_size(h, w))
    out = [np.copy(m)]
    for rot in case.rotations:
        m = orc.rotate_map(orc.rotation_matrix(*map(orc.to_radians, rot)), m)
        out.append(np.copy(m))
    return out


def index_of(case, cmap, lens_of=None):
    kind, h, w = case.src[:3]
    if kind == "eac":
        return source_index(face_size(h, w), np.copy(cmap))
    return cr.index_of(case, cmap, lens_of)


def remap(case, image, lens_of=None, cmap=None):
    if cmap is None:
        cmap = stages(case, lens_of)[-1]
    if case.src[0] == "eac":
        return sample(image, np.copy(cmap))
    return cr.remap(case, image, lens_of, cmap)
