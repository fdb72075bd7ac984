"""Conditions on the inputs of tests/test_hip_catmull_rom_tiles.py (tests/interp_cases.py), checked on the CPU from the definitions alone:
the sweep is what its name says - deterministic, with every kind of destination and lens the tile kernels meet, pictures that are not
black - and the one place where a tile kernel may legitimately disagree with the definition on black or sampled, the band of 1/512 px
either side of a camera source's frame, holds next to no pixel.  1/512 px is twice the tile models' certified bound PB_COARSE_PX = 1/1024
(which also covers the coordinate tables' quantum of 1/4096 px)."""

import functools

import numpy as np
import pytest

from tests import catmull_rom_ref as crr
from tests import interp_cases as ic

BAND = 1.0 / 512.0


def _is_polynomial(p):
    return p[0] in ("camera", "double") and p[3] in ic.POLYNOMIAL


def test_sweep_is_deterministic():
    again = ic.sweep()
    assert len(ic.SWEEP) == 16 and [c.name for c in ic.SWEEP] == [f"sweep{k}" for k in range(16)]
    for a, b in zip(ic.SWEEP, again):
        assert (a.name, a.dst, a.src, a.rotations, a.mask) == (b.name, b.dst, b.src, b.rotations, b.mask)
    assert ic.single_source_case(5).src == ic.SWEEP[5].src and ic.single_source_case(5).rotations == ic.SWEEP[5].rotations


def test_sweep_holds_every_kind():
    S = ic.SWEEP
    assert all(c.src[0] in ("camera", "pano") for c in S), "a double-fisheye or cube source is not the tile kernel's"
    assert sum(c.dst[0] == "cube" for c in S) >= 3
    assert sum(c.dst[0] == "double" for c in S) >= 2
    assert sum(_is_polynomial(p) for c in S for p in (c.dst, c.src)) >= 3
    assert sum(c.src[0] == "pano" for c in S) >= 5
    assert sum(c.src[0] == "camera" for c in S) >= 6
    assert all(0 <= len(c.rotations) <= 2 for c in S) and any(len(c.rotations) == 2 for c in S)
    for c in S:
        for kind, h, w, lens, fov, mag in (c.dst, c.src):
            assert h % ic.SCALE == 0 and w % ic.SCALE == 0 and max(h, w) <= 1400, c
            if kind == "cube":
                assert 20 * ic.SCALE <= h // 2 <= 120 * ic.SCALE and w == 3 * (h // 2), c
            if kind in ("camera", "double"):
                assert lens in ic.LENS_MAX_FOV and 60 <= fov <= max(230, ic.LENS_MAX_FOV[lens]), c


def test_fixed_cases_are_what_the_gpu_tests_need():
    names = [c.name for c in ic.SWEEP + ic.TINY + ic.MAGNIFIED + [ic.ODD_DST]]
    assert len(set(names)) == len(names)
    src_shapes = {(c.src[0], c.src[1], c.src[2]) for c in ic.TINY}
    assert {("camera", 3, 5), ("camera", 4, 4), ("camera", 5, 3), ("camera", 1, 6), ("pano", 2, 4), ("pano", 3, 6), ("pano", 4, 8)} <= src_shapes
    dst_shapes = {(c.dst[0], c.dst[1], c.dst[2]) for c in ic.TINY}
    assert {("cube", 4, 6), ("cube", 6, 9), ("camera", 1, 1), ("camera", 33, 35)} <= dst_shapes
    assert len(ic.MAGNIFIED) == 4 and all(c.dst[1] >= 8 * c.src[1] or c.dst[0] == "cube" for c in ic.MAGNIFIED)
    assert ic.ODD_DST.dst[2] % 4 != 0 and ic.ODD_DST.dst[1] % 32 != 0


@functools.lru_cache(maxsize=None)
def _definition(k):
    """(share of non-black pixels of the Catmull-Rom definition on the noise frame, pixels in the edge band, pixels) of SWEEP[k]"""
    case = ic.SWEEP[k]
    final = ic.final_map(case)
    with np.errstate(all="ignore"):
        out = crr.remap(None, ic.src_proj(case), ic.noise_frame(case), cmap=np.copy(final))
    band = ic.edge_band(case, final, BAND)
    assert out.shape == (case.dst[1], case.dst[2], 3) and band.shape == out.shape[:2]
    return float((out != 0).any(axis=2).mean()), int(band.sum()), band.size


@pytest.mark.parametrize("k", range(16), ids=[ic.label(c) for c in ic.SWEEP])
def test_sweep_pictures_are_not_black_and_the_edge_band_is_thin(k):
    lit, in_band, n = _definition(k)
    print(f"{ic.label(ic.SWEEP[k])}: {100 * lit:.1f} % non-black, {in_band} of {n} pixels within 1/512 px of the source frame's edge")
    assert lit >= 0.10, f"only {100 * lit:.1f} % of the picture is not black"
    assert in_band * 10000 <= n, f"{in_band} of {n} pixels lie in the edge band"
    if ic.SWEEP[k].src[0] == "pano":
        assert in_band == 0


def test_edge_band_marks_the_pixels_next_to_the_frame():
    """A camera copied onto itself: pixel (i, j)'s source position is (i, j) to rounding, so row 0 and column 0 sit ON the boundaries f = 0
    and the last row and column one pixel inside f = h and f = w."""
    from tests.cases import Case, cam, full_frame

    case = Case("id", cam(24, 24, "equidistant", 180, full_frame(24, 24)), cam(24, 24, "equidistant", 180, full_frame(24, 24)))
    final = ic.final_map(case)
    valid = final[:, :, 2] == 0.0
    want = np.zeros((24, 24), bool)
    want[0, :] = want[:, 0] = True
    assert np.array_equal(ic.edge_band(case, final, 1e-6), want & valid) and (want & valid).any()
    want[[1, 23], :] = want[:, [1, 23]] = True
    assert np.array_equal(ic.edge_band(case, final, 1.0 + 1e-6), want & valid)
    assert not ic.edge_band(Case("p", case.dst, ("pano", 12, 24, "equidistant", 0.0, None)), final, 1.0).any()
