"""The cases the bilinear video kernel (pb_planar_bilinear_kernel) is compared with its definition on, shared by the CPU
condition on them (tests/test_video_interp_cases_host.py) and the GPU tests (tests/test_hip_video_bilinear.py).  Every size is even, so
4:2:0 applies to all of them: four of the random sweep and the four magnified cases of tests/interp_cases.py, and five fixed ones - tiny
sources whose chroma planes are one or two samples wide, a 2 x 2 destination, a destination whose width is no multiple of 4 and whose
height is no multiple of the tile's 32."""

from __future__ import annotations

import numpy as np

from oracle import reference_path as orc
from tests import interp_cases as ic
from tests.cases import Case, cam, full_frame, inscribed, pano

BAND = 1.0 / 512.0  # twice the certified coordinate bound: where a tile kernel may decide black / sampled differently (interp_cases.edge_band)
BAND_SHARE = 0.005  # ... and the largest share of a case's output pixels that band may hold

FIXED = [
    Case("video_cam_34x36_pano_2x4", cam(34, 36, "equidistant", 180), pano(2, 4)),
    Case("video_pano_2x2_rot", pano(2, 2), pano(8, 16), [(10, 20, 30)]),
    Case("video_odd_dst_36x62", cam(36, 62, "equidistant", 180, full_frame(36, 62)), pano(40, 80), [(10, 20, 30)]),
    Case("video_pano_from_cam_2x2", pano(64, 128), cam(2, 2, "equidistant", 180, inscribed(2))),
    Case("video_pano_from_cam_4x6", pano(24, 48), cam(4, 6, "equidistant", 180, full_frame(4, 6))),
]
CASES = [ic.by_name(n) for n in ("sweep3", "sweep5", "sweep10", "sweep12")] + list(ic.MAGNIFIED) + FIXED


def by_name(name: str) -> Case:
    for c in CASES:
        if c.name == name:
            return c
    raise KeyError(name)


def coords(case: Case, final: np.ndarray):
    """(fy, fx, live, src_kind) of the definition (tests/video_bilinear_ref.py) from the float64 map interp_cases.final_map(case) gives:
    the pre-truncation source coordinate and liveness of oracle.reference_path.remap_bilinear."""
    cmap = np.copy(final)
    invalid = cmap[:, :, 2] != 0.0
    kind, h, w, *_ = case.src
    with np.errstate(all="ignore"):
        if kind == "pano":
            _, _, _, fy, fx = orc.pano_positions(h, w, cmap)
            live = ~invalid & np.isfinite(fy) & np.isfinite(fx)
        else:
            assert kind == "camera", kind
            _, _, fy, fx = orc.camera_positions(ic.src_proj(case), h, w, cmap[:, :, 0], cmap[:, :, 1])
            live = ~invalid & np.isfinite(fy) & np.isfinite(fx) & (fy >= 0) & (fy < h) & (fx >= 0) & (fx < w)
    return fy, fx, live, kind
