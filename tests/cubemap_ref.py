"""TEST INFRASTRUCTURE ONLY - the cube map's definition, written once in NumPy from the stage functions of
oracle/reference_path.py: a cube face IS a rectilinear camera behind a fixed rotation, so both directions are compositions of stages the
oracle already restates bit for bit.  tests/make_cubemap_goldens.py asserts these functions equal to the real reference while it writes
tests/golden/cubemap.npz.

Frame: a cube of face size N is an image (2N, 3N) + trailing; face k occupies rows (k // 3) N ... and columns (k % 3) N ...;
top row left, front, right - bottom row up, back, down; no padding, no mirroring.
World axes (the reference's rotation): v = (x, y, z) = (sin lat cos lon, cos lat, sin lat sin lon).
"""

from __future__ import annotations

import warnings

import numpy as np

from oracle import reference_path as orc

FACES = ("left", "front", "right", "up", "back", "down")
_X, _Y, _Z = np.eye(3)
# face -> (right, forward, up) world unit vectors
TRIPLES = {
    "left": (+_X, -_Z, +_Y),
    "front": (+_Z, +_X, +_Y),
    "right": (-_X, +_Z, +_Y),
    "up": (+_Z, +_Y, -_X),
    "back": (-_Z, -_X, +_Y),
    "down": (+_Z, -_Y, +_X),
}
FACE_FOV = 2 * np.pi / 3


def face_matrix(face) -> np.ndarray:
    """M_face: the 3 x 3 float64 matrix whose columns are the face's right, forward and up vectors (exact 0 and +-1, determinant +1)."""
    name = FACES[face] if isinstance(face, (int, np.integer)) else face
    return np.ascontiguousarray(np.stack(TRIPLES[name], axis=1) + 0.0)  # (+ 0.0: no negative zeros)


def face_proj(n: int) -> orc.Proj:
    """CameraImage(N x N, fov = 2 pi / 3, rectilinear()) whose f_distance attribute is then set to exactly N / 2."""
    p = orc.Proj("camera", n, n, "rectilinear", FACE_FOV)
    p.f_distance = n / 2
    return p


def face_size(height: int, width: int) -> int:
    n = height // 2
    if height < 2 or height != 2 * n or width != 3 * n:
        raise ValueError(f"a cube map has shape (2N, 3N), got ({height}, {width})")
    return n


def coordinate_map(n: int) -> np.ndarray:
    """The cube DESTINATION's coordinate map (2N, 3N, 3): per face the face camera's map after one rotate_map with M_face."""
    out = np.empty((2 * n, 3 * n, 3), np.float64)
    for k in range(6):
        m = orc.rotate_map(face_matrix(k), orc.coordinate_map(face_proj(n)))
        out[(k // 3) * n:(k // 3 + 1) * n, (k % 3) * n:(k % 3 + 1) * n] = m
    return out


def select_face(cmap: np.ndarray) -> np.ndarray:
    """The face index (order of FACES) each entry of a map samples; invalid entries are zeroed first as the reference's rotation does
    (in a copy: process_coordinate_map of a cube leaves the caller's map unmodified)."""
    invalid = cmap[:, :, 2] != 0.0
    lat = np.where(invalid, 0.0, cmap[:, :, 0])
    lon = np.where(invalid, 0.0, cmap[:, :, 1])
    vy = np.cos(lat)
    xz = np.exp(lon * 1j) * np.sin(lat)
    vx, vz = xz.real, xz.imag
    a, b, c = np.abs(vx), np.abs(vy), np.abs(vz)
    use_x = (a >= b) & (a >= c)
    use_y = ~use_x & (b >= c)
    neg_x, neg_y, neg_z = np.signbit(vx), np.signbit(vy), np.signbit(vz)
    # +x front, -x back, +y up, -y down, +z right, -z left
    return np.where(use_x, np.where(neg_x, 4, 1), np.where(use_y, np.where(neg_y, 5, 3), np.where(neg_z, 0, 2))).astype(np.int32)


def _face_maps(cmap: np.ndarray):
    """Per face k, one at a time: the map after one more rotate_map with M_k transposed (on a copy)."""
    for k in range(6):
        yield orc.rotate_map(np.ascontiguousarray(face_matrix(k).T), np.copy(cmap))


def source_index(n: int, cmap: np.ndarray) -> np.ndarray:
    """int32 linear index into the full (2N, 3N) frame per entry of the map, -1 where the output is black."""
    face = select_face(cmap)
    p = face_proj(n)
    out = np.full(cmap.shape[:2], -1, np.int64)
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
        _, _, pre_y, pre_x = orc.camera_positions(p, n, n, fm[:, :, 0], fm[:, :, 1])
        fy = np.where(face == k, pre_y, fy)
        fx = np.where(face == k, pre_x, fx)
    return face, fy, fx


def sample(image: np.ndarray, cmap: np.ndarray) -> np.ndarray:
    """cube.process_coordinate_map(cmap): image is (2N, 3N) + trailing, any sample type."""
    n = face_size(*image.shape[:2])
    idx = source_index(n, cmap)
    flat = image.reshape((-1,) + image.shape[2:])
    out = flat[np.maximum(idx, 0)]
    out[idx < 0] = 0
    return out


# ---- whole remaps with a cube at either end: projections are tests/cases.py tuples, kind "cube" = ("cube", 2N, 3N, ...) --------------
def cube(n: int):
    return ("cube", 2 * n, 3 * n, "equidistant", 0.0, None)


def orc_proj(p, lens_of=None) -> orc.Proj:
    kind, h, w, lens, fov, mag = p
    if kind == "pano":
        return orc.Proj("pano", h, w)
    if lens_of is not None:
        lens = lens_of(lens)
    return orc.Proj(kind, h, w, lens, orc.to_radians(fov), mag)


def stages(case, lens_of=None):
    """The float64 maps after the destination's coordinate map and after each rotation."""
    kind, h, w = case.dst[:3]
    m = coordinate_map(face_size(h, w)) if kind == "cube" else orc.coordinate_map(orc_proj(case.dst, lens_of))
    out = [np.copy(m)]
    for rot in case.rotations:
        m = orc.rotate_map(orc.rotation_matrix(*map(orc.to_radians, rot)), m)
        out.append(np.copy(m))
    return out


def index_of(case, cmap, lens_of=None):
    """The source's integer index map of a (final) coordinate map; a double source: the oracle's tuple."""
    kind, h, w = case.src[:3]
    if kind == "cube":
        return source_index(face_size(h, w), np.copy(cmap))
    return orc.source_index(orc_proj(case.src, lens_of), np.copy(cmap))


def remap(case, image, lens_of=None, cmap=None):
    if cmap is None:
        cmap = stages(case, lens_of)[-1]
    if case.src[0] == "cube":
        return sample(image, np.copy(cmap))
    return orc.sample(orc_proj(case.src, lens_of), image, np.copy(cmap))


# ---- the opt-in interpolated modes from a cube source: the camera definition on the selected face, taps clamped to
# that face's N x N rectangle (seams are not filtered across faces) ----------------------------------------------------------------
def remap_bilinear(image: np.ndarray, cmap: np.ndarray) -> np.ndarray:
    """Bilinear sampling of a cube source from a coordinate map, per oracle.reference_path._bilinear_camera on the selected face."""
    if image.ndim == 2:
        return remap_bilinear(image[:, :, None], cmap)[:, :, 0]
    n = face_size(*image.shape[:2])
    invalid = cmap[:, :, 2] != 0.0
    face = select_face(cmap)
    p = face_proj(n)
    out = np.zeros(cmap.shape[:2] + image.shape[2:], image.dtype)
    for k, fm in enumerate(_face_maps(cmap)):
        sub = image[(k // 3) * n:(k // 3 + 1) * n, (k % 3) * n:(k % 3 + 1) * n]
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            val, _ = orc._bilinear_camera(p, n, n, sub, fm[:, :, 0], fm[:, :, 1], invalid)
        out[face == k] = val[face == k]
    return out


def remap_catmull_rom(image: np.ndarray, cmap: np.ndarray) -> np.ndarray:
    """Catmull-Rom sampling of a cube source (tests/catmull_rom_ref.py's camera definition on the selected face)."""
    from tests import catmull_rom_ref as crr

    if image.ndim == 2:
        return remap_catmull_rom(image[:, :, None], cmap)[:, :, 0]
    n = face_size(*image.shape[:2])
    invalid = cmap[:, :, 2] != 0.0
    face = select_face(cmap)
    p = face_proj(n)
    out = np.zeros(cmap.shape[:2] + image.shape[2:], image.dtype)
    for k, fm in enumerate(_face_maps(cmap)):
        sub = image[(k // 3) * n:(k // 3 + 1) * n, (k % 3) * n:(k % 3 + 1) * n]
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            val, _ = crr._camera(p, n, n, sub, fm[:, :, 0], fm[:, :, 1], invalid)
        out[face == k] = val[face == k]
    return out
