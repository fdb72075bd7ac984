"""The cube map cases shared by tests/make_cubemap_goldens.py, the CPU tests and the GPU tests.

Projections are tests/cases.py tuples (kind, height, width, lens, fov_degrees, magnitude) with one more kind, "cube" = (2N, 3N); a lens
name of tests/polynomial_cases.LENSES is a ``photonbend_amd.polynomial(...)`` lens.  The definition the device is held to is
tests/cubemap_ref.py."""

from __future__ import annotations

import numpy as np

from oracle.synth import synth_frame
from tests import cubemap_ref as cr
from tests import polynomial_cases as pc
from tests.cases import Case, cam, dbl, full_frame, inscribed, pano

cube = cr.cube


def small_cases():
    rot = [(10, 20, 30)]
    return [
        # panorama -> cube, with and without rotations (N = 28: tiles of 32 straddle faces; N = 25: a centre pixel on every face)
        Case("K_pano_cube24", cube(24), pano(48, 96)),
        Case("K_pano_cube28", cube(28), pano(64, 128)),
        Case("K_pano_cube24_chain", cube(24), pano(50, 100), [(10, 20, 30), (-40, 5, 77)]),
        # each fisheye layout -> cube: inscribed, cropped (top and bottom cut), full frame; double fisheye -> cube
        Case("K_inscribed_cube24_rot", cube(24), cam(48, 48, "equidistant", 360, inscribed(48)), [(30, 45, 10)], mask=1),
        Case("K_cropped_cube24", cube(24), cam(36, 54, "equisolid", 200, inscribed(54))),
        Case("K_full_cube25", cube(25), cam(40, 60, "stereographic", 220, full_frame(40, 60))),
        Case("K_double_cube24_rot", cube(24), dbl(40, 80, "equidistant", 195), [(3, 90, -7)], mask=2),
        # cube -> panorama, camera (a fisheye destination with invalid corners), double fisheye, cube
        Case("K_cube_pano", pano(32, 64), cube(24)),
        Case("K_cube_pano_rot", pano(32, 64), cube(28), rot),
        Case("K_cube_camera_corners", cam(48, 48, "equisolid", 180, inscribed(48)), cube(32), rot),
        Case("K_cube_double_rot", dbl(32, 64, "equidistant", 195), cube(24), [(20, 30, 40)]),
        Case("K_cube_cube24_identity", cube(24), cube(24)),
        Case("K_cube_cube24_rot", cube(24), cube(32), [(12, 34, 56)]),
        # polynomial lens <-> cube
        Case("K_poly_cube24", cube(24), cam(48, 48, "EQS9", 190, 23.5), mask=1),
        Case("K_cube_poly", cam(40, 40, "CAL", 200, inscribed(40)), cube(32)),
    ]


def full_cases():
    """The full-size pair (tests/golden/cubemap_full.json): an 8192 x 4096 panorama into N = 2048 faces, and the way back."""
    return [Case("KF_pano_cube2048", cube(2048), pano(4096, 8192)), Case("KF_cube2048_pano", pano(4096, 8192), cube(2048))]


def case_by_name(name):
    for c in small_cases() + full_cases():
        if c.name == name:
            return c
    raise KeyError(name)


def lens_of(name):
    """What the oracle takes for a lens name: a built-in's name, or a polynomial lens's (forward, reverse) pair."""
    if name in pc.LENSES:
        L = pc.lens(name)
        return (L.forward_function, L.reverse_function)
    return name


def case_frame(case, frame: int = 0, layout: str = "RGB"):
    """The synthetic source frame of a case; layout: "RGB" uint8 (h, w, 3), "L" uint8 (h, w), "RGBA" uint8 (h, w, 4), "I;16" uint16 (h, w)."""
    _, h, w, *_ = case.src
    rgb = synth_frame(h, w, frame=frame, seed=0, circle_mask=case.mask)
    if layout == "RGB":
        return rgb
    if layout == "L":
        return np.ascontiguousarray(rgb[:, :, 1])
    if layout == "RGBA":
        return np.ascontiguousarray(np.concatenate([rgb, rgb[:, :, :1] ^ 0x5A], axis=2))
    if layout == "I;16":
        return (rgb[:, :, 0].astype(np.uint16) << 8) | rgb[:, :, 2].astype(np.uint16)
    raise KeyError(layout)


def map_key(case, k: int) -> str:
    """The fixture key of a case's map after k rotations: the unrotated map of a cube destination is stored once per face size."""
    if k == 0 and case.dst[0] == "cube":
        return f"cube{case.dst[1] // 2}/map0"
    return f"{case.name}/map{k}"


def pb_obj(p, image=None):
    import photonbend_amd as pb

    kind, h, w, name, fov, mag = p
    if kind == "cube":
        return pb.CubemapImage(np.zeros((h, w, 3), np.uint8) if image is None else image)
    return pc.pb_obj(p, image)


def pb_chain(case, image=None, supersample: int = 1):
    """dst.get_coordinate_map() -> rotations -> (src object, map)."""
    import photonbend_amd as pb

    dst = pb_obj(case.dst)
    cmap = dst.get_coordinate_map() if supersample == 1 else dst.get_coordinate_map(supersample=supersample)
    for rot in case.rotations:
        cmap = pb.Rotation(*map(pb.utils.to_radians, rot)).rotate_coordinate_map(cmap)
    return pb_obj(case.src, case_frame(case) if image is None else image), cmap


def ref_stages(case):
    return cr.stages(case, lens_of)


def ref_index(case, cmap):
    return cr.index_of(case, cmap, lens_of)


def ref_remap(case, image, cmap=None):
    return cr.remap(case, image, lens_of, cmap)
