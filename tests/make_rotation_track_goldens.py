#!/usr/bin/env python3
"""TEST INFRASTRUCTURE ONLY - writes tests/golden/rotation_track.npz.

Like tests/make_cubemap_goldens.py it runs only where the real reference can be imported (read-only, never copied).  For every case of
tests/rotation_track_cases.golden_cases() and every frame f it runs the reference's own classes: the destination's
``get_coordinate_map()``, then one ``Rotation(...).rotate_coordinate_map`` per rotation of frame f's chain - the plan's own, then the
frame's, in turn -, then the source's ``process_coordinate_map``.  Kept per frame: the int32 source-index map (the reference sampling an
int32 'image' whose pixel value is its linear index + 1; both eyes' maps for a double fisheye) and the uint8 output on the synthetic frame.

Usage:  python tests/make_rotation_track_goldens.py
"""

from __future__ import annotations

import os
import sys
import warnings

sys.dont_write_bytecode = True
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, "/root/reference")

import numpy as np  # noqa: E402

from tests import rotation_track_cases as rc  # noqa: E402

import photonbend.core.lens as ref_lens  # noqa: E402
from photonbend.core.projection import CameraImage, DoubleCameraImage, PanoramaImage  # noqa: E402
from photonbend.core.rotation import Rotation  # noqa: E402
from photonbend.utils import to_radians  # noqa: E402

GOLD = os.path.join(REPO, "tests", "golden")
warnings.simplefilter("ignore")
np.seterr(all="ignore")


def ref_obj(p, image=None):
    kind, h, w, name, fov, mag = p
    if image is None:
        image = np.zeros((h, w, 3), np.uint8)
    if kind == "pano":
        return PanoramaImage(image)
    if kind == "camera":
        return CameraImage(image, to_radians(fov), getattr(ref_lens, name)(), magnitude=mag)
    return DoubleCameraImage(image, to_radians(fov), getattr(ref_lens, name)())


def ref_map(case, f):
    m = ref_obj(case.dst).get_coordinate_map()
    for rot in case.chain(f):
        m = Rotation(*map(to_radians, rot)).rotate_coordinate_map(m)
    return m


def ref_index(case, cmap):
    kind, h, w, name, fov, mag = case.src
    ids = (np.arange(h * w, dtype=np.int32) + 1).reshape(h, w)
    if kind != "double":
        return ((ref_obj(case.src, ids).process_coordinate_map(np.copy(cmap)) - 1).astype(np.int32),)
    L = getattr(ref_lens, name)()
    w2 = w // 2
    left = CameraImage(ids[:, :w2], to_radians(fov), L)
    right = CameraImage(np.copy(ids[:, w2:])[:, ::-1], to_radians(fov), L)
    rmap = np.copy(cmap)
    rmap[:, :, 0] *= -1
    rmap[:, :, 0] += np.pi
    return (left.process_coordinate_map(np.copy(cmap)) - 1).astype(np.int32), (right.process_coordinate_map(rmap) - 1).astype(np.int32)


def main():
    out = {}
    for case in rc.golden_cases():
        frames = rc.case_frames(case)
        for f in range(len(case.frames)):
            m = ref_map(case, f)
            idx = ref_index(case, m)
            if len(idx) == 2:
                out[f"{case.name}/{f}/idx_l"], out[f"{case.name}/{f}/idx_r"] = idx
            else:
                out[f"{case.name}/{f}/idx"] = idx[0]
            u8 = ref_obj(case.src, frames[f]).process_coordinate_map(np.copy(m))
            assert u8.dtype == np.uint8 and u8.shape == (case.dst[1], case.dst[2], 3), (case.name, f, u8.dtype, u8.shape)
            out[f"{case.name}/{f}/u8"] = u8
            print(f"  {case.name} frame {f}: {int((~u8.any(axis=2)).sum())} black of {u8.shape[0] * u8.shape[1]}")
    path = os.path.join(GOLD, "rotation_track.npz")
    np.savez_compressed(path, **out)
    print(f"rotation_track.npz written, {len(out)} arrays, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
