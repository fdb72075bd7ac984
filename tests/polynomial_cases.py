"""The polynomial (Kannala-Brandt) lens cases shared by tests/make_polynomial_goldens.py, the CPU tests and the GPU tests.

Projections are tests/cases.py tuples (kind, height, width, lens, fov_degrees, magnitude) whose lens is a built-in's name or one of the
names of LENSES below - a ``photonbend_amd.polynomial(...)`` lens; the oracle takes its (forward, reverse) pair, and so does the
reference."""

from __future__ import annotations

import math

import numpy as np

from oracle import reference_path as orc
from oracle.synth import synth_frame
from tests.cases import Case, cam, dbl, inscribed, pano

# name -> ((k1, k2, k3, k4), max_theta in degrees): the series of 2 sin(theta / 2) and of 2 tan(theta / 2) to theta^9, an OpenCV-like
# calibration, and the identity
LENSES = {
    "EQS9": ((-1 / 24, 1 / 1920, -1 / 322560, 1 / 92897280), 110.0),
    "STE9": ((1 / 12, 1 / 120, 17 / 20160, 31 / 362880), 100.0),
    "CAL": ((-0.0357, 0.0031, -0.00042, 0.00002), 105.0),
    "ZERO": ((0.0, 0.0, 0.0, 0.0), 180.0),
}
ORTH9 = ((-1 / 6, 1 / 120, -1 / 5040, 1 / 362880), 85.0)  # the series of sin(theta): dp falls to 0.087 at 85 degrees


def lens(name):
    """The package's Lens for a name of LENSES (or a built-in's name)."""
    import photonbend_amd as pb

    if name in LENSES:
        k, deg = LENSES[name]
        return pb.polynomial(*k, max_theta=math.pi if deg == 180.0 else orc.to_radians(deg))
    return getattr(pb, name)()


def untagged(name):
    """The same lens as plain user callables: the package's host path (PB_LENS_CUSTOM)."""
    import photonbend_amd as pb

    L = lens(name)
    return pb.Lens(lambda t: L.forward_function(t), lambda r: L.reverse_function(r))


def small_cases():
    rot = [(10, 20, 30)]
    return [
        Case("P_dst_eqs9_rot", cam(40, 40, "EQS9", 190, 19.5), pano(32, 64), rot),
        Case("P_dst_cal", cam(48, 48, "CAL", 180, inscribed(48)), pano(32, 64)),
        # the image circle is the lens's whole domain (fov / 2 == max_theta): the corners lie beyond r_max
        Case("P_dst_beyond_rmax", cam(40, 40, "STE9", 200, inscribed(40)), pano(32, 64), rot),
        Case("P_src_eqs9_rot", pano(32, 64), cam(48, 48, "EQS9", 190, 23.5), rot, mask=1),
        # a panorama looks in every direction: most of it lies past the source lens's max_theta
        Case("P_src_past_max_theta", pano(32, 64), cam(48, 48, "CAL", 150, inscribed(48)), mask=1),
        Case("P_both_rot", cam(40, 40, "STE9", 180, inscribed(40)), cam(48, 48, "CAL", 200, inscribed(48)), [(-15, 100, 200)], mask=1),
        Case("P_both", cam(40, 40, "CAL", 200, inscribed(40)), cam(56, 56, "EQS9", 210, inscribed(56))),
        Case("P_builtin_dst_poly_src", cam(40, 40, "equisolid", 180, inscribed(40)), cam(48, 48, "CAL", 200, inscribed(48)), rot, mask=1),
        Case("P_double_src", pano(32, 64), dbl(40, 80, "EQS9", 195), mask=2),
        Case("P_double_src_rot", pano(33, 66), dbl(40, 80, "CAL", 200), [(3, 90, -7)], mask=2),
        Case("P_double_dst_rot", dbl(32, 64, "EQS9", 190), pano(48, 96), rot),
        Case("P_double_dst", dbl(32, 64, "STE9", 195), cam(48, 48, "equidistant", 360, inscribed(48)), mask=1),
        Case("P_zero", cam(48, 48, "ZERO", 360, inscribed(48)), pano(64, 128), rot),
    ]


def mid_cases():
    """About 1000 px a side, one per kind, with a rotation: sizes at which the windowed tile kernels run."""
    return [
        Case("PM_photo_cal", cam(1024, 1024, "CAL", 200, inscribed(1024)), pano(1024, 2048), [(12, -30, 7)]),
        Case("PM_pano_eqs9", pano(768, 1536), cam(1280, 1280, "EQS9", 210, inscribed(1280)), [(5, 60, -20)], mask=1),
        Case("PM_double_dst_cal", dbl(960, 1920, "CAL", 200), pano(1024, 2048), [(12, -30, 7)]),
        Case("PM_stitch_eqs9", pano(768, 1536), dbl(1024, 2048, "EQS9", 200), [(3, 90, -7)], mask=2),
    ]


def case_by_name(name):
    for c in small_cases() + mid_cases():
        if c.name == name:
            return c
    raise KeyError(name)


def orc_proj(p) -> orc.Proj:
    kind, h, w, name, fov, mag = p
    if kind == "pano":
        return orc.Proj("pano", h, w)
    if name in LENSES:
        L = lens(name)
        name = (L.forward_function, L.reverse_function)
    return orc.Proj(kind, h, w, name, orc.to_radians(fov), mag)


def orc_rots(case):
    return [tuple(map(orc.to_radians, r)) for r in case.rotations]


def case_frame(case, frame: int = 0):
    _, h, w, *_ = case.src
    return synth_frame(h, w, frame=frame, seed=0, circle_mask=case.mask)


def pb_obj(p, image=None, make_lens=lens):
    import photonbend_amd as pb

    kind, h, w, name, fov, mag = p
    if image is None:
        image = np.zeros((h, w, 3), np.uint8)
    if kind == "pano":
        return pb.PanoramaImage(image)
    if kind == "camera":
        return pb.CameraImage(image, pb.utils.to_radians(fov), make_lens(name), magnitude=mag)
    return pb.DoubleCameraImage(image, pb.utils.to_radians(fov), make_lens(name))


def pb_chain(case, image=None, make_lens=lens):
    """dst.get_coordinate_map() -> rotations -> (src object, map)."""
    import photonbend_amd as pb

    cmap = pb_obj(case.dst, make_lens=make_lens).get_coordinate_map()
    for rot in case.rotations:
        cmap = pb.Rotation(*map(pb.utils.to_radians, rot)).rotate_coordinate_map(cmap)
    return pb_obj(case.src, image if image is not None else case_frame(case), make_lens=make_lens), cmap


def orc_stages(case):
    """The oracle's float64 maps: after coordinate_map and after each rotation."""
    m = orc.coordinate_map(orc_proj(case.dst))
    out = [np.copy(m)]
    for rot in orc_rots(case):
        m = orc.rotate_map(orc.rotation_matrix(*rot), m)
        out.append(np.copy(m))
    return out
