"""The planar definition (tests/planar_ref.py) against the two definitions it extends, and the conditions the planar edge
cases rely on, asserted from the oracle alone - so the coverage of tests/test_hip_planar.py cannot go silently.  No GPU."""

import numpy as np
import pytest

from oracle import reference_path as orc
from tests import cases as tc
from tests import helpers as H
from tests import nv12_ref, planar_ref
from tests.cases import Case, cam, inscribed, pano

SMALL = H.load_small()
GOLDEN_CASES = ("D_photo_rot", "D_pano_pano_rot", "A_photo_odd")  # (the last one is odd both ways: 4:4:4 only)

# the edge geometries of the planar GPU tests that carry a condition (tests/test_hip_nv12.py's, and two odd ones of this feature)
EDGE_CASES = {
    "edge_34x36_src2x2": Case("edge_34x36_src2x2", cam(34, 36, "equidistant", 180), pano(2, 2), [(10, 20, 30)]),
    "edge_36x34_src4x6": Case("edge_36x34_src4x6", pano(36, 34), pano(4, 6), [(12, 34, 56)]),
    "edge_34x36_cam_src": Case("edge_34x36_cam_src", cam(34, 36, "equisolid", 190), cam(48, 48, "equidistant", 360, inscribed(48)), [(30, 45, 10)]),
    "edge_66x66_inscribed": Case("edge_66x66_inscribed", cam(66, 66, "equidistant", 360, inscribed(66)), pano(64, 128), [(30, 45, 10)]),
    "edge_pano_2x_last_pixel": Case("edge_pano_2x_last_pixel", pano(64, 128), pano(32, 64)),
    "edge_odd_33x36_src3x6": Case("edge_odd_33x36_src3x6", cam(33, 36, "equidistant", 180), pano(3, 6), [(10, 20, 30)]),  # odd heights: 4:2:2, 4:4:4
    "edge_odd_33x35_src3x5": Case("edge_odd_33x35_src3x5", cam(33, 35, "equidistant", 180), pano(3, 5), [(10, 20, 30)]),  # odd both ways: 4:4:4
}
# (blocks with a valid anchor and a black partner, blocks with a black anchor and a valid partner): 1 x 2 blocks (4:2:2) / 2 x 2 blocks
MIXED_1x2 = {"edge_34x36_src2x2": (20, 20), "edge_34x36_cam_src": (22, 22), "edge_66x66_inscribed": (38, 38), "edge_odd_33x36_src3x6": (13, 13)}
MIXED_2x2 = {"edge_34x36_src2x2": (16, 18), "edge_34x36_cam_src": (19, 19), "edge_66x66_inscribed": (32, 44)}
LAST_SAMPLES = ("edge_36x34_src4x6", "edge_pano_2x_last_pixel")  # the source's last pixel and, at 4:2:2, the last chroma sample of the last row


def oracle_index(case):
    with np.errstate(all="ignore"):
        return orc.remap_index(H.orc_proj(case.dst), H.orc_proj(case.src), H.orc_rots(case))


def random_planes(h, w, sub, dt, seed):
    cx, cy = planar_ref.SHIFTS[sub]
    rng = np.random.default_rng(seed)
    hi = np.iinfo(dt).max + 1
    return [rng.integers(0, hi, shp).astype(dt) for shp in ((h, w), (h >> cy, w >> cx), (h >> cy, w >> cx))]


def mixed(idx, by, bx):
    """(blocks of by x bx pixels with a valid anchor among black pixels, blocks with a black anchor among valid ones)."""
    Hd, Wd = idx.shape
    blocks = (idx >= 0).reshape(Hd // by, by, Wd // bx, bx).transpose(0, 2, 1, 3).reshape(-1, by * bx)
    m = blocks.any(axis=1) & ~blocks.all(axis=1)
    return int((m & blocks[:, 0]).sum()), int((m & ~blocks[:, 0]).sum())


@pytest.mark.parametrize("name", GOLDEN_CASES[:2])
@pytest.mark.parametrize("dt", (np.uint8, np.uint16))
def test_at_420_the_interleaved_chroma_planes_are_the_nv12_definition_s_pairs(name, dt):
    case = tc.case_by_name(name)
    idx = SMALL[f"{name}/idx"]
    _, h, w, *_ = case.src
    p0, p1, p2 = random_planes(h, w, "420", dt, seed=11)
    for fill in (planar_ref.default_fill(dt), (1, 2, 3)):
        o0, o1, o2 = planar_ref.remap_planar(p0, p1, p2, idx, w, "420", fill)
        y, uv = nv12_ref.remap_nv12(p0, np.stack([p1, p2], axis=2), idx, w, fill)
        assert np.array_equal(o0, y) and np.array_equal(np.stack([o1, o2], axis=2), uv)
        assert o0.dtype == o1.dtype == o2.dtype == np.dtype(dt)
    assert planar_ref.default_fill(dt) == nv12_ref.default_fill(dt)


@pytest.mark.parametrize("name", GOLDEN_CASES)
def test_at_444_every_plane_is_a_grey_remap(name):
    case = tc.case_by_name(name)
    idx = SMALL[f"{name}/idx"]
    _, h, w, *_ = case.src
    assert int((idx < 0).sum()) > 0 or name != "A_photo_odd"
    for dt in (np.uint8, np.uint16):
        ps = random_planes(h, w, "444", dt, seed=12)
        fill = (5, 6, 7)
        outs = planar_ref.remap_planar(*ps, idx, w, "444", fill)
        for p, o, f in zip(ps, outs, fill):
            want = p.ravel()[np.where(idx < 0, 0, idx)]
            want[idx < 0] = f
            assert np.array_equal(o, want)
        # the packed flat frame is the three planes one after another
        flat = planar_ref.remap_frame(np.concatenate([p.ravel() for p in ps]), idx, h, w, "444", fill)
        assert np.array_equal(flat, np.concatenate([o.ravel() for o in outs]))


def test_at_422_a_sample_follows_the_anchor_of_its_1x2_block():
    name = "D_photo_rot"
    case = tc.case_by_name(name)
    idx = SMALL[f"{name}/idx"]
    _, h, w, *_ = case.src
    p0, p1, p2 = random_planes(h, w, "422", np.uint8, seed=13)
    o0, o1, o2 = planar_ref.remap_planar(p0, p1, p2, idx, w, "422", (1, 2, 3))
    Hd, Wd = idx.shape
    assert o1.shape == o2.shape == (Hd, Wd // 2)
    for i in range(Hd):
        for j in range(Wd // 2):
            a = int(idx[i, 2 * j])
            assert (o1[i, j], o2[i, j]) == ((2, 3) if a < 0 else (p1[a // w, (a % w) >> 1], p2[a // w, (a % w) >> 1]))


def test_the_dimension_rule():
    assert planar_ref.dims_ok("444", (33, 35), (1, 1)) and planar_ref.dims_ok("422", (33, 36)) and planar_ref.dims_ok("420", (34, 36))
    assert not planar_ref.dims_ok("422", (33, 35)) and not planar_ref.dims_ok("420", (33, 36)) and not planar_ref.dims_ok("420", (34, 35))
    assert planar_ref.frame_samples(4, 6, "444") == 72 and planar_ref.frame_samples(4, 6, "422") == 48 and planar_ref.frame_samples(4, 6, "420") == 36
    with pytest.raises(AssertionError):
        planar_ref.remap_planar(np.zeros((3, 5), np.uint8), np.zeros((3, 2), np.uint8), np.zeros((3, 2), np.uint8), np.zeros((2, 2), np.int32), 5, "422", (0, 0, 0))


@pytest.mark.parametrize("name", sorted(EDGE_CASES))
def test_the_edge_cases_hold_what_the_gpu_tests_rely_on(name):
    case = EDGE_CASES[name]
    idx = oracle_index(case)
    _, h, w, *_ = case.src
    assert idx.shape == (case.dst[1], case.dst[2])
    if name in MIXED_1x2:
        assert mixed(idx, 1, 2) == MIXED_1x2[name]
    if name in MIXED_2x2:
        assert mixed(idx, 2, 2) == MIXED_2x2[name]
    if name == "edge_34x36_src2x2":
        assert int(idx.max()) == 3  # the source's last sample of every plane, at every subsampling
    if name in LAST_SAMPLES:
        assert int(idx.max()) == h * w - 1
        a = idx[:, 0::2]  # the anchors at 4:2:2
        r, c = np.divmod(np.where(a < 0, 0, a), w)
        assert bool(((a >= 0) & (r == h - 1) & ((c >> 1) == w // 2 - 1)).any())  # the last chroma sample of the last row
    if name == "edge_odd_33x36_src3x6":
        assert int(idx.max()) == 17 and planar_ref.dims_ok("422", (h, w), idx.shape) and not planar_ref.dims_ok("420", (h, w), idx.shape)
    if name == "edge_odd_33x35_src3x5":
        assert int((idx < 0).sum()) == 294 and int(idx.max()) == 14
        assert not planar_ref.dims_ok("422", (h, w), idx.shape) and planar_ref.dims_ok("444", (h, w), idx.shape)
