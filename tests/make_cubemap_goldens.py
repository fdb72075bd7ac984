#!/usr/bin/env python3
"""TEST INFRASTRUCTURE ONLY - writes tests/golden/cubemap.npz and tests/golden/cubemap_full.json.

Like tests/make_polynomial_goldens.py it runs only where the real reference can be imported (read-only, never copied).  The reference
has no cube map; the cube map is DEFINED through it: face k of a cube of face size N is the reference's
``CameraImage(N x N, fov = 2 pi / 3, rectilinear())`` whose ``f_distance`` attribute is then set to exactly N / 2, behind one
``rotate_coordinate_map`` of a ``Rotation`` whose ``rotation_matrix`` attribute is set to M_k (a destination) or its transpose (a source,
on the face the selection rule picks).  This script runs exactly that composition through the reference's classes, asserts
tests/cubemap_ref.py equal to it on every array while writing, and keeps per small case: the float64 map after get_coordinate_map and
after every rotation (bits; a cube destination's unrotated map once per face size), the integer source-index map(s) (and a double
source's blend weights) and the output bytes on the synthetic frame.  The full-size pair goes into the JSON as SHA-256 plus samples.

Usage:  python tests/make_cubemap_goldens.py [--full]
"""

from __future__ import annotations

import hashlib
import json
import os
import sys
import warnings

sys.dont_write_bytecode = True
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, "/root/reference")

import numpy as np  # noqa: E402

from oracle import reference_path as orc  # noqa: E402
from tests import cubemap_cases as cc  # noqa: E402
from tests import cubemap_ref as cr  # noqa: E402
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


def ref_face_camera(pixels):
    """The reference's camera of one face: CameraImage(N x N, 2 pi / 3, rectilinear()) with f_distance injected."""
    n = pixels.shape[0]
    cam = CameraImage(pixels, 2 * np.pi / 3, ref_lens.rectilinear())
    cam.f_distance = n / 2
    return cam


def ref_face_rotation(matrix):
    rot = Rotation(0.0, 0.0, 0.0)
    rot.rotation_matrix = np.ascontiguousarray(matrix, dtype=np.float64)
    return rot


def ref_cube_map(n):
    out = np.empty((2 * n, 3 * n, 3), np.float64)
    for k in range(6):
        m = ref_face_camera(np.zeros((n, n, 3), np.uint8)).get_coordinate_map()
        out[(k // 3) * n:(k // 3 + 1) * n, (k % 3) * n:(k % 3 + 1) * n] = ref_face_rotation(cr.face_matrix(k)).rotate_coordinate_map(m)
    return out


def ref_cube_sample(image, cmap):
    """cube.process_coordinate_map(cmap) through the reference: per face its camera on the map after M_k transposed, the face by the rule."""
    n = cr.face_size(*image.shape[:2])
    face = cr.select_face(cmap)
    out = None
    for k in range(6):
        sub = np.ascontiguousarray(image[(k // 3) * n:(k // 3 + 1) * n, (k % 3) * n:(k % 3 + 1) * n])
        o = ref_face_camera(sub).process_coordinate_map(ref_face_rotation(cr.face_matrix(k).T).rotate_coordinate_map(np.copy(cmap)))
        if out is None:
            out = np.zeros_like(o)
        out[face == k] = o[face == k]
    return out


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
    if kind == "cube":
        return (ref_cube_sample(ids, cmap) - 1).astype(np.int32)
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


def ref_run(case, frame):
    """(map stages, final map, output bytes) of a case through the reference."""
    kind, h, w = case.dst[:3]
    m = ref_cube_map(cr.face_size(h, w)) if kind == "cube" else ref_obj(case.dst).get_coordinate_map()
    stages = [np.copy(m)]
    for rot in case.rotations:
        m = Rotation(*map(to_radians, rot)).rotate_coordinate_map(m)
        stages.append(np.copy(m))
    u8 = ref_cube_sample(frame, m) if case.src[0] == "cube" else ref_obj(case.src, frame).process_coordinate_map(np.copy(m))
    return stages, m, u8


def small(out):
    for case in cc.small_cases():
        n = case.name
        frame = cc.case_frame(case)
        stages, m, u8 = ref_run(case, frame)
        for k, (st, want) in enumerate(zip(stages, cc.ref_stages(case))):
            assert same_bits(st, want), f"{n}: cubemap_ref map stage {k} != reference"
            key = cc.map_key(case, k)
            if key in out:
                assert np.array_equal(out[key], bits(st)), key
            out[key] = bits(st)
        idx = ref_index(case, m)
        oidx = cc.ref_index(case, m)
        if case.src[0] == "double":
            assert np.array_equal(oidx[0], idx[0]) and np.array_equal(oidx[1], idx[1]), n
            out[f"{n}/idx_l"], out[f"{n}/idx_r"] = idx
            out[f"{n}/w_l"], out[f"{n}/w_r"] = bits(oidx[2]), bits(oidx[3])
        else:
            assert np.array_equal(oidx, idx), n
            out[f"{n}/idx"] = idx
        assert np.array_equal(cc.ref_remap(case, frame), u8), n
        if case.src[0] == "cube":  # process_coordinate_map of a cube leaves the caller's map unmodified
            keep = np.copy(m)
            cr.sample(frame, keep)
            assert same_bits(keep, m), n
        out[f"{n}/u8"] = u8
        black = int((~u8.reshape(-1, u8.shape[-1]).any(axis=1)).sum())
        invalid = int((stages[0][:, :, 2] != 0).sum())
        print(f"  {n}: ok ({u8.shape[0]}x{u8.shape[1]}, {invalid} invalid, {black} black pixels)")


def samples_of(a, count=64):
    """A fixed scatter of pixels: [[row, col, values...], ...]."""
    h, w = a.shape[:2]
    rng = np.random.RandomState(20260)
    rows, cols = rng.randint(0, h, count), rng.randint(0, w, count)
    return [[int(r), int(c)] + [int(v) for v in np.atleast_1d(a[r, c])] for r, c in zip(rows, cols)]


def full():
    """The full-size pair through tests/cubemap_ref.py (asserted equal to the reference on the small cases above and, here, on one face
    and one band of rows through the reference itself)."""
    res = {}
    for case in cc.full_cases():
        frame = cc.case_frame(case)
        stages = cc.ref_stages(case)
        m = stages[-1]
        if case.dst[0] == "cube":
            n = case.dst[1] // 2
            cam_map = ref_face_camera(np.zeros((n, n, 3), np.uint8)).get_coordinate_map()
            assert same_bits(ref_face_rotation(cr.face_matrix(4)).rotate_coordinate_map(cam_map), m[n:, n:2 * n]), "full: back face != reference"
        idx = cc.ref_index(case, m)
        u8 = cc.ref_remap(case, frame, m)
        if case.src[0] == "cube":
            band = slice(1000, 1016)
            assert np.array_equal(ref_cube_sample(frame, np.copy(m[band])), u8[band]), "full: rows 1000-1015 != reference"
        res[case.name] = {
            "shape": list(u8.shape),
            "sha256_u8": hashlib.sha256(np.ascontiguousarray(u8).tobytes()).hexdigest(),
            "sha256_idx": hashlib.sha256(np.ascontiguousarray(idx, dtype=np.int32).tobytes()).hexdigest(),
            "black": int((idx < 0).sum()),
            "samples_u8": samples_of(u8),
            "samples_idx": samples_of(idx),
        }
        print(f"  {case.name}: {u8.shape}, {res[case.name]['black']} black, sha256 {res[case.name]['sha256_u8'][:16]}...")
    with open(os.path.join(GOLD, "cubemap_full.json"), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


def main():
    out = {}
    small(out)
    path = os.path.join(GOLD, "cubemap.npz")
    np.savez_compressed(path, **out)
    print(f"cubemap.npz written, {len(out)} arrays, {os.path.getsize(path)} bytes")
    if "--full" in sys.argv:
        full()


if __name__ == "__main__":
    main()
