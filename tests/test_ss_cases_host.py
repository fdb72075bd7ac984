"""The conditions on the inputs of tests/test_hip_supersample_tiles.py (tests/ss_cases.py), from the oracle alone: what each edge case is
there to reach is really reached, so the GPU tests cannot go vacuous.  The counts are the goldens' platform's; elsewhere the booleans
and ">= 1" hold."""

import numpy as np
import pytest

from tests import helpers as H
from tests import ss_cases as sc
from tests import ss_ref

CASES = [(c, n) for c in sc.ALL_EDGES for n in sc.NS]
IDS = [f"{c.name}-n{n}" for c, n in CASES]


def test_the_edge_cases_are_the_nine_specified_shapes():
    assert [c.name for c in sc.EDGES] == ["ss_edge_17x19", "ss_edge_tiny_src", "ss_edge_33_inscribed", "ss_edge_identity", "ss_edge_1x1",
                                          "ss_edge_cam_src", "ss_edge_1x40", "ss_edge_40x1", "ss_edge_last_px"]
    assert [(c.dst[1], c.dst[2]) for c in sc.EDGES] == [(17, 19), (9, 18), (33, 33), (16, 32), (1, 1), (17, 18), (1, 40), (40, 1), (20, 36)]
    assert [(c.src[1], c.src[2]) for c in sc.EDGES] == [(16, 32), (2, 2), (16, 32), (32, 64), (4, 8), (48, 48), (8, 16), (8, 16), (4, 6)]
    assert sc.edge_by_name("ss_edge_cam_src").src[0] == "camera" and all(c.src[0] == "pano" for c in sc.EDGES if c.name != "ss_edge_cam_src")
    # two packed sources are no multiple of 16 bytes (the generic route); their twins are, and are otherwise the same cases
    for case, twin in zip((sc.edge_by_name("ss_edge_tiny_src"), sc.edge_by_name("ss_edge_last_px")), sc.FUSED_TWINS):
        assert (3 * case.src[1] * case.src[2]) % 16 != 0 and (3 * twin.src[1] * twin.src[2]) % 16 == 0
        assert twin.dst == case.dst and twin.rotations == case.rotations and twin.src[1] * twin.src[2] < 32 * 32
    assert all((3 * c.src[1] * c.src[2]) % 16 == 0 for c in sc.EDGES if c.name not in ("ss_edge_tiny_src", "ss_edge_last_px"))
    # the mid cases are used AS the n x plans: both factors divide their sides
    assert len(sc.MID) == 4 and all(c.dst[1] % 4 == 0 and c.dst[2] % 4 == 0 for c in sc.MID)


@pytest.mark.parametrize("case,n", CASES, ids=IDS)
def test_index_maps_have_the_n_x_shape_and_stay_inside_the_source(case, n):
    idx, fragile = sc.edge_index(case, n)
    assert idx.shape == fragile.shape == (n * case.dst[1], n * case.dst[2])
    assert int(idx.min()) >= -1 and int(idx.max()) < case.src[1] * case.src[2]
    assert not idx.flags.writeable and not fragile.flags.writeable  # shared among the tests: nobody edits them


@pytest.mark.parametrize("name", sorted(sc.SAMPLES_LAST_PIXEL))
def test_the_last_source_pixel_is_sampled(name):
    case = sc.edge_by_name(name)
    last = case.src[1] * case.src[2] - 1
    for n, expected in zip(sc.NS, sc.SAMPLES_LAST_PIXEL[name]):
        if expected:
            assert int(sc.edge_index(case, n)[0].max()) == last, (name, n)


@pytest.mark.parametrize("name", sorted(sc.MIXED_BLOCKS))
def test_blocks_mix_valid_and_black_subsamples_and_some_are_all_black(name):
    case = sc.edge_by_name(name)
    for k, n in enumerate(sc.NS):
        mixed, black = sc.mixed_and_black_blocks(sc.edge_index(case, n)[0], n)
        assert mixed >= 1 and black >= 1, (name, n, mixed, black)
        if H.live_numpy_is_the_goldens_numpy():
            assert (mixed, black) == (sc.MIXED_BLOCKS[name][k], sc.BLACK_BLOCKS[name][k]), (name, n)


@pytest.mark.parametrize("n", sc.NS)
def test_block_sums_hold_ties_rounded_up_and_ties_rounded_down(n):
    up = down = 0
    for case in sc.EDGES:
        u, d = sc.ties(sc.gather(sc.edge_frame(case), sc.edge_index(case, n)[0]), n)
        up, down = up + u, down + d
    assert up >= 1 and down >= 1, (n, up, down)
    if H.live_numpy_is_the_goldens_numpy():
        assert (up, down) == {2: (879, 806), 4: (457, 424)}[n]  # (hundreds of each: both branches of the tie rule decide output bytes)


@pytest.mark.parametrize("case,n", CASES, ids=IDS)
def test_the_fragile_blocks_leave_most_of_a_case_compared(case, n):
    """On another host's libm an output pixel may differ where its block holds a fragile pixel: that allowance must stay small."""
    idx, fragile = sc.edge_index(case, n)
    share = sc.fragile_share(sc.want(sc.edge_frame(case), idx, n), fragile, n)
    assert share <= sc.FRAGILE_SHARE_MAX, (case.name, n, share)
    if H.live_numpy_is_the_goldens_numpy() and case.name == "ss_edge_17x19" and n == 4:
        assert round(share, 3) == 0.136  # the largest of the eighteen


def test_frames_of_a_case_differ_and_are_reproducible():
    case = sc.edge_by_name("ss_edge_17x19")
    assert np.array_equal(sc.edge_frame(case, 1), sc.edge_frame(case, 1)) and not np.array_equal(sc.edge_frame(case, 1), sc.edge_frame(case, 2))


def test_want_is_the_block_mean_of_the_gather_with_black_misses():
    """The reference written out on a hand-made index map: misses are black subsamples that count in the mean."""
    img = np.arange(2 * 2 * 3, dtype=np.uint8).reshape(2, 2, 3) * 20
    idx = np.array([[0, 1, -1, -1], [2, 3, -1, 3]], dtype=np.int32)
    S = sc.gather(img, idx)
    assert S.shape == (2, 4, 3) and not S[0, 2].any() and np.array_equal(S[1, 3], img[1, 1])
    got = sc.want(img, idx, 2)
    # block 0: channel 0 of pixels 0..3 = 0, 60, 120, 180 -> 90; block 1: (0 + 0 + 0 + 180) / 4 = 45
    assert got.shape == (1, 2, 3) and got[0, 0, 0] == 90 and got[0, 1, 0] == 45
    assert np.array_equal(got, ss_ref.block_mean(S, 2))
    assert sc.mixed_and_black_blocks(idx, 2) == (1, 0) and sc.mixed_and_black_blocks(np.full((2, 4), -1), 2) == (0, 2)
    # a tie rounds to even: 4 x 2 + 2 = sum 10 -> q 2, r 2 -> 2; sum 14 -> q 3, r 2 -> 4
    assert sc.ties(np.array([[[2], [2]], [[3], [3]]], dtype=np.uint8), 2) == (0, 1)
    assert sc.ties(np.array([[[3], [3]], [[4], [4]]], dtype=np.uint8), 2) == (1, 0)
