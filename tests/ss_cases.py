"""The inputs of the fused supersample kernel's tests (tests/test_hip_supersample_tiles.py, tests/test_ss_cases_host.py), and
the reference they are held to - exact integers:

    idx  = the oracle's index map of the n x destination
    S    = img.reshape(-1, 3)[where(idx < 0, 0, idx)];  S[idx < 0] = 0
    want = ss_ref.block_mean(S, n)

Nothing here needs a GPU to import."""

from __future__ import annotations

import functools

import numpy as np

from oracle import reference_path as orc
from tests import cubemap_cases as cc
from tests import cubemap_ref as cr
from tests import helpers as H
from tests import ss_ref
from tests.cases import Case, cam, inscribed, pano
from tests.test_hip_pixel_formats import MID, _mid_plan, fancy  # noqa: F401  (the four mid cases of the pixel-format tests, each used AS the n x plan)

NS = (2, 4)

# The 1 x destination, the source, the rotations; each used at n = 2 and n = 4.  The smallest shapes that still reach each edge of
# pb_ss_reduce_store / pb_ss_put.
EDGES = [
    # partial tiles on both axes; an odd output width, so rows start off a dword boundary; the last store of a row holds 3 pixels
    Case("ss_edge_17x19", cam(17, 19, "equidistant", 172), pano(16, 32), [(10, 20, 30)]),
    # a tile holds more pixels than the source; the last source pixel in every tile
    Case("ss_edge_tiny_src", pano(9, 18), pano(2, 2), [(10, 20, 30)]),
    # black corners, and blocks that mix black and sampled subsamples
    Case("ss_edge_33_inscribed", cam(33, 33, "equidistant", 360, inscribed(33)), pano(16, 32), [(30, 45, 10)]),
    # n = 2 is the identity map and n = 4 a 2 x one; every coordinate sits on an integer
    Case("ss_edge_identity", pano(16, 32), pano(32, 64)),
    # one output pixel (count == 1)
    Case("ss_edge_1x1", pano(1, 1), pano(4, 8), [(12, 34, 56)]),
    # a camera source (PB_NT_DEFAULT: non-temporal stores); source misses
    Case("ss_edge_cam_src", cam(17, 18, "equisolid", 190), cam(48, 48, "equidistant", 360, inscribed(48)), [(30, 45, 10)]),
    # one output row
    Case("ss_edge_1x40", pano(1, 40), pano(8, 16), [(12, 34, 56)]),
    # one output column: every store is a single pixel
    Case("ss_edge_40x1", cam(40, 1, "equidistant", 172), pano(8, 16), [(12, 34, 56)]),
    # the source's last pixel sampled at both n
    Case("ss_edge_last_px", pano(20, 36), pano(4, 6), [(12, 34, 56)]),
]

# A packed frame of 3 h w bytes that is no multiple of 16 is not served fused (pb_aligned16 looks at the stride, which pb_check_frames
# fills in with the frame size): ss_edge_tiny_src (12 bytes) and ss_edge_last_px (72).  Their twins are the smallest sources of the
# same kind whose packed frames are (48 and 96 bytes): still far fewer pixels than a tile, the last one sampled at both n.
FUSED_TWINS = [
    Case("ss_edge_tiny_src_4x4", pano(9, 18), pano(4, 4), [(10, 20, 30)]),
    Case("ss_edge_last_px_4x8", pano(20, 36), pano(4, 8), [(12, 34, 56)]),
]
ALL_EDGES = EDGES + FUSED_TWINS

# what the oracle's index says of the edge cases (tests/test_ss_cases_host.py), as (n = 2, n = 4)
SAMPLES_LAST_PIXEL = {"ss_edge_tiny_src": (True, True), "ss_edge_33_inscribed": (True, True), "ss_edge_last_px": (True, True),
                      "ss_edge_identity": (False, True), "ss_edge_tiny_src_4x4": (True, True), "ss_edge_last_px_4x8": (True, True)}
MIXED_BLOCKS = {"ss_edge_17x19": (28, 44), "ss_edge_33_inscribed": (68, 96), "ss_edge_cam_src": (38, 62)}
BLACK_BLOCKS = {"ss_edge_17x19": (82, 74), "ss_edge_33_inscribed": (244, 236), "ss_edge_cam_src": (56, 44)}
FRAGILE_SHARE_MAX = 0.20  # of a case's blocks: those left out on another host's libm that are not all-black in `want`


def edge_by_name(name: str) -> Case:
    return next(c for c in ALL_EDGES if c.name == name)


def mid_by_name(name: str) -> Case:
    return next(c for c in MID if c.name == name)


def random_frame(h: int, w: int, seed: int) -> np.ndarray:
    """An (h, w, 3) frame of independent random bytes: a wrong index shows."""
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def edge_frame(case: Case, k: int = 0) -> np.ndarray:
    """Frame k of an edge case: the fixed seeds the host test's tie counts are taken on."""
    return random_frame(case.src[1], case.src[2], seed=7000 + 16 * [c.name for c in ALL_EDGES].index(case.name) + k)


@functools.lru_cache(maxsize=None)
def _edge_index(name: str, n: int):
    case = edge_by_name(name)
    od, os_, rots = ss_ref.orc_proj_ss(case.dst, n), H.orc_proj(case.src), H.orc_rots(case)
    with np.errstate(all="ignore"):
        idx = orc.remap_index(od, os_, rots)
        fragile = orc.fragile_mask(orc.pretrunc(od, os_, rots))
    idx.setflags(write=False)
    fragile.setflags(write=False)
    return idx, fragile


def edge_index(case: Case, n: int):
    """(the oracle's index map of the n x destination (n H, n W), its fragile mask): computed once per (case, n), read-only."""
    return _edge_index(case.name, n)


@functools.lru_cache(maxsize=None)
def _mid_index(name: str):
    case = mid_by_name(name)
    with np.errstate(all="ignore"):
        cmap = cc.ref_stages(case)[-1]
        idx = cc.ref_index(case, cmap)
        if case.src[0] == "cube":
            fragile = orc.fragile_mask(cr.pretrunc(cr.face_size(case.src[1], case.src[2]), np.copy(cmap)))
        else:
            fragile = orc.fragile_mask(orc.pretrunc(H.orc_proj(case.dst), H.orc_proj(case.src), H.orc_rots(case)))
    idx = np.ascontiguousarray(idx)
    idx.setflags(write=False)
    fragile.setflags(write=False)
    return idx, fragile


def mid_index(case: Case):
    """(index map, fragile mask) of a mid case's own destination - the n x destination of the supersampled call - as
    test_mid_cases_equal_fancy_indexing_with_the_oracle_index takes them: once per case, read-only."""
    return _mid_index(case.name)


gather = fancy  # S: NumPy fancy indexing of an (h, w, 3) frame with an index map, black where the index is negative


def want(img: np.ndarray, idx: np.ndarray, n: int) -> np.ndarray:
    return ss_ref.block_mean(gather(img, idx), n)


def blocks_any(mask: np.ndarray, n: int) -> np.ndarray:
    """(n H, n W) booleans -> (H, W): the n x n block holds a True."""
    Hh, Ww = mask.shape[0] // n, mask.shape[1] // n
    return mask.reshape(Hh, n, Ww, n).any(axis=(1, 3))


def blocks_all(mask: np.ndarray, n: int) -> np.ndarray:
    return ~blocks_any(~mask, n)


def mixed_and_black_blocks(idx: np.ndarray, n: int):
    """(blocks that hold valid and black subsamples together, blocks that are all black) of an index map."""
    valid = idx >= 0
    some, every = blocks_any(valid, n), blocks_all(valid, n)
    return int((some & ~every).sum()), int((~some).sum())


def block_sums(S: np.ndarray, n: int) -> np.ndarray:
    Hh, Ww = S.shape[0] // n, S.shape[1] // n
    return S.reshape(Hh, n, Ww, n, -1).astype(np.int64).sum(axis=(1, 3))


def ties(S: np.ndarray, n: int):
    """(block sums that are ties rounded up: r == N/2 with q odd, ties rounded down: q even)."""
    N = n * n
    s = block_sums(S, n)
    q, r = s // N, s % N
    tie = r == N // 2
    return int((tie & (q % 2 == 1)).sum()), int((tie & (q % 2 == 0)).sum())


def fragile_share(want_: np.ndarray, fragile: np.ndarray, n: int) -> float:
    """The share of a case's blocks that the other-host rule leaves out and that are not all-black in `want`."""
    out = blocks_any(fragile, n) & want_.any(axis=-1)
    return float(out.sum()) / out.size


def check(got: np.ndarray, want_: np.ndarray, fragile: np.ndarray, n: int, what: str) -> None:
    """The comparison with the oracle: equality where this host's NumPy is the goldens'; elsewhere an output pixel may differ only if
    its n x n block holds a pixel of the fragile mask."""
    assert got.shape == want_.shape and got.dtype == want_.dtype, (what, got.shape, want_.shape, got.dtype)
    bad = (got != want_).any(axis=-1)
    if H.live_numpy_is_the_goldens_numpy():
        assert int(bad.sum()) == 0, f"{what}: {int(bad.sum())} of {bad.size} output pixels differ from the oracle, first at {tuple(np.argwhere(bad)[0])}"
    else:
        outside = bad & ~blocks_any(fragile, n)
        assert int(outside.sum()) == 0, f"{what}: {int(outside.sum())} output pixels differ outside the fragile blocks"
