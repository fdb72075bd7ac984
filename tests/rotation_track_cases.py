"""The rotation-track cases shared by tests/make_rotation_track_goldens.py, the CPU test of the fixture and the GPU tests.

A case is a geometry (tests/cases.py projection tuples), the plan's own rotations and, per frame, the rotations of that frame (degrees:
pitch, yaw, roll, as the CLI's ``-r``): frame f's chain is ``plan_rot + frames[f]``, applied one after another."""

from __future__ import annotations

from dataclasses import dataclass, field
from typing import List, Tuple

from oracle.synth import synth_frame
from tests.cases import P, cam, dbl, inscribed, pano

Rot = Tuple[float, float, float]
IDENTITY, POLE = (0.0, 0.0, 0.0), (-90.0, 0.0, 0.0)  # no rotation at all; a pitch that carries the poles onto the horizon


@dataclass
class TrackCase:
    name: str
    dst: P
    src: P
    plan_rot: List[Rot] = field(default_factory=list)
    frames: List[List[Rot]] = field(default_factory=list)
    mask: int = 0  # the synthetic frames' circle mask (0 none, 1 single, 2 double)

    def chain(self, f: int) -> List[Rot]:
        return list(self.plan_rot) + list(self.frames[f])


def golden_cases() -> List[TrackCase]:
    """Six geometries x four frames (tests/golden/rotation_track.npz): every source kind the reference has, k = 1 and 2 rotations per
    frame behind 0 or 1 of the plan's, the identity and the pole-crossing pitch among them, an odd destination."""
    one = [[IDENTITY], [POLE], [(30, 45, 10)], [(-3.5, 170, 12)]]
    two = [[(10, 20, 30), IDENTITY], [POLE, (0, 90, 0)], [(1, 2, 3), (-40, 5, 77)], [(0, 0, 45), (0, 0, -45)]]
    return [
        TrackCase("T_stabilise_pano", pano(24, 48), pano(24, 48), [], one),
        TrackCase("T_reframe_odd", cam(35, 33, "equidistant", 180), pano(32, 64), [(5, -20, 33)], one),
        TrackCase("T_fisheye_src_k2", pano(20, 40), cam(40, 40, "equisolid", 190, inscribed(40)), [], two, mask=1),
        TrackCase("T_double_195", cam(32, 32, "equidistant", 360, inscribed(32)), dbl(32, 64, "equidistant", 195), [], one, mask=2),
        TrackCase("T_double_180_seam", pano(24, 48), dbl(24, 48, "equidistant", 180), [(3, 90, -7)], one, mask=2),
        TrackCase("T_alter_k2", cam(28, 28, "stereographic", 140, inscribed(28)), cam(36, 36, "thoby", 180, inscribed(36)), [(12, 34, 56)], two, mask=1),
    ]


def case_frames(case: TrackCase):
    """The synthetic source frames of a case, one per track entry: uint8 (N, h, w, 3)."""
    import numpy as np

    _, h, w, *_ = case.src
    return np.stack([synth_frame(h, w, frame=f, seed=0, circle_mask=case.mask) for f in range(len(case.frames))])
