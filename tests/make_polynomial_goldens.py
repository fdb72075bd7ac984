#!/usr/bin/env python3
"""TEST INFRASTRUCTURE ONLY - writes tests/golden/polynomial.npz.

Like oracle/make_goldens.py it runs only where the real reference can be imported (read-only, never copied): the cases of
tests/polynomial_cases.py go through the reference's public API with the package's polynomial lens handed over as a Lens of two
callables - which is all the reference knows of a lens -, the oracle (oracle/reference_path.py with the same pair) is asserted equal
on every array while writing, and per case the fixture keeps: the float64 map after get_coordinate_map and after every rotation
(bits), the integer source-index map(s) (and a double source's blend weights) and the output bytes on the synthetic frame.

Usage:  python tests/make_polynomial_goldens.py
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

from oracle import reference_path as orc  # noqa: E402
from tests import polynomial_cases as pc  # noqa: E402

import photonbend.core.lens as ref_lens  # noqa: E402
from photonbend.core.projection import CameraImage, DoubleCameraImage, PanoramaImage  # noqa: E402
from photonbend.core.rotation import Rotation  # noqa: E402
from photonbend.utils import to_radians  # noqa: E402

GOLD = os.path.join(REPO, "tests", "golden")
warnings.simplefilter("ignore")
np.seterr(all="ignore")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and bool(((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))).all())


def ref_lens_obj(name):
    if name in pc.LENSES:
        L = pc.lens(name)
        return ref_lens.Lens(L.forward_function, L.reverse_function)
    return getattr(ref_lens, name)()


def ref_obj(p, image=None):
    kind, h, w, name, fov, mag = p
    if image is None:
        image = np.zeros((h, w, 3), np.uint8)
    if kind == "pano":
        return PanoramaImage(image)
    if kind == "camera":
        return CameraImage(image, to_radians(fov), ref_lens_obj(name), magnitude=mag)
    return DoubleCameraImage(image, to_radians(fov), ref_lens_obj(name))


def ref_index(case, cmap):
    """The integer source-index map from the reference itself: an int32 'image' whose pixel value is its own linear index + 1."""
    kind, h, w, name, fov, mag = case.src
    ids = (np.arange(h * w, dtype=np.int32) + 1).reshape(h, w)
    if kind != "double":
        return (ref_obj(case.src, ids).process_coordinate_map(np.copy(cmap)) - 1).astype(np.int32)
    L = ref_lens_obj(name)
    w2 = w // 2
    left = CameraImage(ids[:, :w2], to_radians(fov), L)
    right = CameraImage(np.copy(ids[:, w2:])[:, ::-1], to_radians(fov), L)
    rmap = np.copy(cmap)
    rmap[:, :, 0] *= -1
    rmap[:, :, 0] += np.pi
    il = left.process_coordinate_map(np.copy(cmap)) - 1
    ir = right.process_coordinate_map(rmap) - 1
    return il.astype(np.int32), ir.astype(np.int32)


def main():
    out = {}
    for case in pc.small_cases():
        n = case.name
        m = ref_obj(case.dst).get_coordinate_map()
        stages = [np.copy(m)]
        for rot in case.rotations:
            m = Rotation(*map(to_radians, rot)).rotate_coordinate_map(m)
            stages.append(np.copy(m))
        for k, (st, want) in enumerate(zip(stages, pc.orc_stages(case))):
            assert same_bits(st, want), f"{n}: oracle map stage {k} != reference"
            out[f"{n}/map{k}"] = bits(st)
        frame = pc.case_frame(case)
        idx = ref_index(case, m)
        u8 = ref_obj(case.src, frame).process_coordinate_map(np.copy(m))
        od, os_, rots = pc.orc_proj(case.dst), pc.orc_proj(case.src), pc.orc_rots(case)
        oidx = orc.remap_index(od, os_, rots)
        if case.src[0] == "double":
            assert np.array_equal(oidx[0], idx[0]) and np.array_equal(oidx[1], idx[1]), n
            out[f"{n}/idx_l"], out[f"{n}/idx_r"] = idx
            out[f"{n}/w_l"], out[f"{n}/w_r"] = bits(oidx[2]), bits(oidx[3])
        else:
            assert np.array_equal(oidx, idx), n
            out[f"{n}/idx"] = idx
        assert np.array_equal(orc.remap(od, os_, frame, rots), u8), n
        out[f"{n}/u8"] = u8
        black = int((~u8.reshape(-1, u8.shape[-1]).any(axis=1)).sum())
        print(f"  {n}: ok ({u8.shape[0]}x{u8.shape[1]}, {black} black pixels)")
    path = os.path.join(GOLD, "polynomial.npz")
    np.savez_compressed(path, **out)
    print(f"polynomial.npz written, {len(out)} arrays, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
