"""The cases the two interpolating tile kernels (bilinear, Catmull-Rom: DESIGN 3.4 / 3.8) are swept with, shared by the CPU conditions on
them (tests/test_interp_cases_host.py) and the GPU tests (tests/test_hip_catmull_rom_tiles.py, tests/test_hip_bilinear.py).

Projections are the six-tuples of tests/cubemap_cases.py: (kind, height, width, lens, fov_degrees, magnitude), kind "cube" = (2N, 3N), a
lens name of tests/polynomial_cases.LENSES a ``photonbend_amd.polynomial(...)`` lens.  No source here is a double fisheye except where a
name says so: the Catmull-Rom mode serves those per pixel in float64, not by the tile kernel."""

from __future__ import annotations

import numpy as np

from oracle import reference_path as orc
from tests import cubemap_cases as cc
from tests import cubemap_ref as cr
from tests.cases import Case, cam, dbl, full_frame, inscribed, pano

cube = cc.cube

# the widest field of view a random camera is drawn with, per lens: the six built-in lenses (tests/test_hip_random.py's table) and two
# polynomial lenses of tests/polynomial_cases.LENSES (fov / 2 stays inside their max_theta of 105 and 110 degrees)
LENS_MAX_FOV = {"equidistant": 360, "equisolid": 360, "stereographic": 300, "orthographic": 180, "rectilinear": 170, "thoby": 200, "CAL": 205, "EQS9": 215}
POLYNOMIAL = ("CAL", "EQS9")
SCALE = 3  # every image dimension and magnitude of a drawn case is multiplied by this, as tests/test_hip_bilinear._noise_cases does
# Case k is drawn from seed SEED_BASE + k.  The base was found by a scan from 31000 on, in steps of 16, for sixteen draws that meet the
# conditions of tests/test_interp_cases_host.py and also hold a polynomial-lens source, three camera and two panorama destinations and two
# cases without a rotation (31000 itself: no double-fisheye destination, and an orthographic camera from an EQS9 source is all black).
SEED_BASE = 31192


def _draw(rng: np.random.Generator, k: int) -> Case:
    """tests/test_hip_random.random_case without double-fisheye sources, with the polynomial lenses and with cube destinations."""

    def rand_cam():
        lens = str(rng.choice(list(LENS_MAX_FOV)))
        fov = float(rng.uniform(60, LENS_MAX_FOV[lens]))
        h = int(rng.integers(40, 300))
        w = h if rng.random() < 0.6 else int(rng.integers(40, 300))
        mag = None if rng.random() < 0.3 else float(rng.uniform(0.4, 0.75) * min(h, w))
        return cam(h, w, lens, fov, mag)

    def rand_pano():
        h = int(rng.integers(24, 260))
        return pano(h, 2 * h)

    def rand_dbl():
        h = int(rng.integers(40, 200))
        return dbl(h, 2 * h, str(rng.choice(["equidistant", "equisolid", "stereographic"])), float(rng.uniform(180, 230)))

    def rand_cube():
        return cube(int(rng.integers(20, 121)))

    dk = str(rng.choice(["cam", "cam", "pano", "dbl", "cube"]))
    sk = str(rng.choice(["cam", "cam", "pano"]))
    dst = {"cam": rand_cam, "pano": rand_pano, "dbl": rand_dbl, "cube": rand_cube}[dk]()
    src = rand_cam() if sk == "cam" else rand_pano()
    nrot = int(rng.choice([0, 0, 1, 2]))
    rots = [tuple(float(v) for v in rng.uniform(-180, 180, 3)) for _ in range(nrot)]
    return Case(f"sweep{k}", dst, src, rots, mask=0)


def _up(p):
    kind, h, w, lens, fov, mag = p
    return (kind, h * SCALE, w * SCALE, lens, fov, None if mag is None else mag * SCALE)


def single_source_case(k: int, seed_base: int = SEED_BASE) -> Case:
    """The k-th seeded random geometry: a camera or panorama source, a camera, panorama, double-fisheye or cube destination, 0-2 rotations."""
    c = _draw(np.random.default_rng(seed_base + k), k)
    return Case(c.name, _up(c.dst), _up(c.src), c.rotations, c.mask)


def sweep(seed_base: int = SEED_BASE):
    return [single_source_case(k, seed_base) for k in range(16)]


SWEEP = sweep()

# frames of a few pixels: tests/test_hip_bilinear.py's nine ...
TINY_BILINEAR = [
    Case("tiny_pano_2x4", cam(33, 35, "equidistant", 180), pano(2, 4)),
    Case("tiny_pano_3x6", cam(40, 40, "equidistant", 360, inscribed(40)), pano(3, 6)),
    Case("tiny_cam_3x3", pano(5, 9), cam(3, 3, "equisolid", 180, inscribed(3))),
    Case("tiny_cam_2x2", pano(64, 128), cam(2, 2, "equidistant", 180, inscribed(2))),
    Case("tiny_double_2x4", pano(40, 80), dbl(2, 4, "equidistant", 190)),
    Case("tiny_dst_1x1", cam(1, 1, "equidistant", 180, 0.5), pano(8, 16)),
    Case("tiny_dst_1x2", pano(1, 2), pano(8, 16), [(10, 20, 30)]),
    Case("tiny_pano_1x2", pano(70, 140), pano(1, 2)),
    Case("tiny_pano_2x3", cam(64, 64, "rectilinear", 100, inscribed(64)), pano(2, 3)),
]
TINY = TINY_BILINEAR + [
    # ... and, for a 4 x 4 footprint: sources with a side of 1 to 5 px (under 4 px every tap of that axis clamps or wraps; a 2 x 4
    # panorama wraps a tap twice), cube destinations of 2 and 3 px faces, a 1 x 1 destination and one of 33 x 35 (partial tiles both ways)
    Case("tiny_cam_3x5", pano(24, 48), cam(3, 5, "equidistant", 180, full_frame(3, 5))),
    Case("tiny_cam_4x4", cam(40, 40, "equisolid", 160, inscribed(40)), cam(4, 4, "equidistant", 180, inscribed(4)), [(10, 20, 30)]),
    Case("tiny_cam_5x3", pano(20, 40), cam(5, 3, "stereographic", 200, full_frame(5, 3)), [(-40, 5, 77)]),
    Case("tiny_cam_1x6", pano(16, 32), cam(1, 6, "equidistant", 180, 3.0)),
    Case("tiny_pano_2x4_rot", pano(33, 66), pano(2, 4), [(10, 20, 30)]),
    Case("tiny_pano_3x6_rot", cam(35, 33, "equidistant", 200), pano(3, 6), [(30, 45, 10)]),
    Case("tiny_pano_4x8_pole", pano(40, 80), pano(4, 8), [(90, 0, 0)]),
    Case("tiny_cube2", cube(2), pano(8, 16)),
    Case("tiny_cube3_rot", cube(3), cam(5, 5, "equidistant", 360, inscribed(5)), [(12, 34, 56)]),
    Case("tiny_dst_1x1_cam4", cam(1, 1, "equidistant", 180, 0.5), cam(4, 4, "equidistant", 180, inscribed(4))),
    Case("tiny_dst_33x35", cam(33, 35, "equidistant", 180), pano(4, 8), [(3, 90, -7)]),
]

# sources magnified 8 to 20 times: most tiles have clamped or wrapped taps
MAGNIFIED = [
    Case("mag_pano_from_cam", pano(384, 768), cam(48, 64, "equidistant", 180, full_frame(48, 64))),
    Case("mag_cube_from_pano", cube(96), pano(16, 32), [(10, 20, 30)]),
    Case("mag_pano_pole_and_seam", pano(256, 512), pano(24, 48), [(90, 0, 0)]),  # the pole and the seam across tiles
    Case("mag_stereo_from_cal", cam(400, 400, "stereographic", 200, inscribed(400)), cam(20, 20, "CAL", 200, inscribed(20))),
]

# a destination whose width is no multiple of 4 (a lane stores four pixels) and whose height is no multiple of the tile's 32
ODD_DST = Case("odd_dst_61x35", cam(61, 35, "equidistant", 180, full_frame(61, 35)), pano(40, 80), [(10, 20, 30)])


def by_name(name: str) -> Case:
    for c in SWEEP + TINY + MAGNIFIED + [ODD_DST]:
        if c.name == name:
            return c
    raise KeyError(name)


def label(c: Case) -> str:
    lens = lambda p: f"{p[0]}{p[1]}x{p[2]}" + (f"_{p[3]}" if p[0] in ("camera", "double") else "")  # noqa: E731
    return f"{c.name}:{lens(c.dst)}<-{lens(c.src)}:r{len(c.rotations)}"


def noise_frame(case: Case, seed: int = 0) -> np.ndarray:
    """Independent random texels: 255 LSB per pixel of coordinate error, every pixel on an interpolation edge."""
    return np.random.default_rng(seed).integers(0, 256, size=(case.src[1], case.src[2], 3), dtype=np.uint8)


def src_proj(case: Case) -> orc.Proj:
    return cr.orc_proj(case.src, cc.lens_of)


def final_map(case: Case) -> np.ndarray:
    """The definition's float64 coordinate map after the destination's stage and every rotation."""
    with np.errstate(all="ignore"):
        return cc.ref_stages(case)[-1]


def edge_band(case: Case, final: np.ndarray, B: float) -> np.ndarray:
    """The output pixels whose float64 source position in the definition lies within B px of a liveness boundary of a camera source - fy = 0
    or h, fx = 0 or w, along the frame's rectangle: the only place where a tile kernel, whose coordinates are certified to 1/1024 px, may
    disagree with the definition on black or sampled.  Empty for a panorama source (every finite position is live)."""
    out = np.zeros(final.shape[:2], bool)
    if case.src[0] != "camera":
        return out
    _, h, w, *_ = case.src
    with np.errstate(all="ignore"):
        _, _, fy, fx = orc.camera_positions(src_proj(case), h, w, final[:, :, 0], final[:, :, 1])
        near_y = (np.abs(fy) <= B) | (np.abs(fy - h) <= B)
        near_x = (np.abs(fx) <= B) | (np.abs(fx - w) <= B)
        out = (near_y & (fx >= -B) & (fx <= w + B)) | (near_x & (fy >= -B) & (fy <= h + B))
    return out & (final[:, :, 2] == 0.0)
