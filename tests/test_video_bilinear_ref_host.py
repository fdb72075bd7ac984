"""tests/video_bilinear_ref.py, the written definition of bilinear video sampling, checked against what it is defined by - no
GPU: plane 0 is oracle.reference_path.remap_bilinear on the grey plane; at 4:4:4 planes 1 and 2 follow plane 0's rule; a constant plane
stays constant; a chroma ramp comes back as the ramp of s_c (which pins the siting); the NV12 wrapper is the planar one interleaved."""

import functools

import numpy as np
import pytest

from oracle import reference_path as orc
from tests import interp_cases as ic
from tests import planar_ref as pr
from tests import video_bilinear_ref as vb
from tests import video_interp_cases as vc

# a panorama source under a rotation (the seam and a pole inside), a camera source with a rim, a tiny panorama (every tap wraps or clamps)
NAMES = ["video_odd_dst_36x62", "video_pano_from_cam_4x6", "video_cam_34x36_pano_2x4", "mag_pano_pole_and_seam"]


@functools.lru_cache(maxsize=None)
def _coords(name):
    case = vc.by_name(name)
    final = ic.final_map(case)
    fy, fx, live, kind = vc.coords(case, final)
    for a in (final, fy, fx, live):
        a.setflags(write=False)
    return case, final, fy, fx, live, kind


def _frame(case, sub, dtype, seed=0, top=None):
    top = np.iinfo(dtype).max if top is None else top
    return np.random.default_rng(seed).integers(0, top + 1, size=pr.frame_samples(case.src[1], case.src[2], sub), dtype=dtype)


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16], ids=["u8", "u16"])
@pytest.mark.parametrize("name", NAMES)
def test_plane_0_is_remap_bilinear_of_the_grey_plane(name, dtype):
    case, final, fy, fx, live, kind = _coords(name)
    h, w = case.src[1:3]
    for sub in pr.SUBSAMPLINGS:
        frame = _frame(case, sub, dtype)
        p0, p1, p2 = pr.planes(frame, h, w, sub)
        o0, _, _ = vb.remap_planar_bilinear(p0, p1, p2, fy, fx, live, kind, sub, (0, 7, 9))
        with np.errstate(all="ignore"):
            want = orc.remap_bilinear(None, ic.src_proj(case), p0, cmap=np.copy(final))
        assert o0.dtype == dtype and np.array_equal(o0, want), (name, sub)


@pytest.mark.parametrize("name", NAMES)
def test_at_444_planes_1_and_2_follow_plane_0_s_rule(name):
    case, final, fy, fx, live, kind = _coords(name)
    h, w = case.src[1:3]
    frame = _frame(case, "444", np.uint16, seed=1)
    p0, p1, p2 = pr.planes(frame, h, w, "444")
    _, o1, o2 = vb.remap_planar_bilinear(p0, p1, p2, fy, fx, live, kind, "444", (0, 0, 0))
    with np.errstate(all="ignore"):
        assert np.array_equal(o1, orc.remap_bilinear(None, ic.src_proj(case), p1, cmap=np.copy(final)))
        assert np.array_equal(o2, orc.remap_bilinear(None, ic.src_proj(case), p2, cmap=np.copy(final)))
    # ... and equal planes give equal planes
    q0, q1, q2 = vb.remap_planar_bilinear(p1, p1, p1, fy, fx, live, kind, "444", (5, 5, 5))
    assert np.array_equal(q0, q1) and np.array_equal(q0, q2)


@pytest.mark.parametrize("sub", pr.SUBSAMPLINGS)
@pytest.mark.parametrize("name", NAMES)
def test_a_constant_plane_stays_constant(name, sub):
    case, _, fy, fx, live, kind = _coords(name)
    h, w = case.src[1:3]
    cx, cy = pr.SHIFTS[sub]
    p0, pc = np.full((h, w), 77, np.uint8), np.full((h >> cy, w >> cx), 201, np.uint8)
    o0, o1, o2 = vb.remap_planar_bilinear(p0, pc, pc + 1, fy, fx, live, kind, sub, (1, 2, 3))
    la = live[0 :: 1 << cy, 0 :: 1 << cx]
    assert np.array_equal(o0, np.where(live, 77, 1)) and np.array_equal(o1, np.where(la, 201, 2)) and np.array_equal(o2, np.where(la, 202, 3))


@pytest.mark.parametrize("sub", ["422", "420"])
def test_a_chroma_ramp_comes_back_as_the_ramp_of_s_c(sub):
    """A camera source (no wrap) whose planes 1 and 2 hold 8 x their own column and row number: away from the clamped border an output
    sample is 8 x the anchor's coordinate in CHROMA sample units, s_c = (f - 0.5) / (1 << c) - top-left siting, and no other."""
    case = vc.by_name("mag_pano_from_cam")  # pano 384 x 768 from a 48 x 64 camera
    _, _, fy, fx, live, kind = _coords(case.name)
    h, w = case.src[1:3]
    cx, cy = pr.SHIFTS[sub]
    ch, cw = h >> cy, w >> cx
    cols = np.broadcast_to(8 * np.arange(cw, dtype=np.uint16), (ch, cw))
    rows = np.broadcast_to(8 * np.arange(ch, dtype=np.uint16)[:, None], (ch, cw))
    _, o1, o2 = vb.remap_planar_bilinear(np.zeros((h, w), np.uint16), cols, rows, fy, fx, live, kind, sub, (0, 0, 0))
    say = (fy[0 :: 1 << cy, 0 :: 1 << cx] - 0.5) / (1 << cy)
    sax = (fx[0 :: 1 << cy, 0 :: 1 << cx] - 0.5) / (1 << cx)
    la = live[0 :: 1 << cy, 0 :: 1 << cx]
    inside = la & (say >= 0) & (say <= ch - 1) & (sax >= 0) & (sax <= cw - 1)
    assert inside.sum() > 1000
    # (rint of an exact linear interpolation: within half a unit of 8 s_c)
    assert np.abs(o1[inside] - 8.0 * sax[inside]).max() <= 0.5 + 1e-9 and np.abs(o2[inside] - 8.0 * say[inside]).max() <= 0.5 + 1e-9
    # centre siting would read (f / 2 - 0.5) = s_c - 0.25 along a halved axis: 2 units away, far outside the half unit above
    assert np.abs(o1[inside] - 8.0 * (sax[inside] - 0.25)).max() > 1.0
    # outside the camera's frame the anchor is dead: the fill
    assert np.all(o1[~la] == 0) and np.all(o2[~la] == 0)


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16], ids=["nv12", "p010"])
@pytest.mark.parametrize("name", NAMES)
def test_the_nv12_wrapper_is_the_planar_definition_deinterleaved(name, dtype):
    case, _, fy, fx, live, kind = _coords(name)
    h, w = case.src[1:3]
    H, W = case.dst[1:3]
    frame = _frame(case, "420", dtype, seed=2)
    p0, p1, p2 = pr.planes(frame, h, w, "420")
    nv = np.concatenate([p0, np.stack([p1, p2], axis=2).reshape(h // 2, w)], axis=0)
    got = vb.remap_nv12(nv, fy, fx, live, kind, h, w)
    want = vb.remap_frame(frame, fy, fx, live, kind, h, w, "420")
    w0, w1, w2 = pr.planes(want, H, W, "420")
    assert got.shape == (3 * H // 2, W) and got.dtype == dtype
    uv = got[H:].reshape(H // 2, W // 2, 2)
    assert np.array_equal(got[:H], w0) and np.array_equal(uv[:, :, 0], w1) and np.array_equal(uv[:, :, 1], w2)


def test_the_tolerance_of_the_issue():
    assert [vb.tolerance(R) for R in (255, 511, 512, 1023, 65535)] == [1, 1, 2, 2, 128]
