"""Test-side reference of the supersampled mode: the oracle's remap of the n x destination, then the n x n block mean with the
integer round-half-to-even rule.  Shared by the supersample test files."""

from __future__ import annotations

import numpy as np

from oracle import reference_path as orc


def block_mean(a: np.ndarray, n: int) -> np.ndarray:
    """(n H, n W, *trailing) unsigned samples -> (H, W, *trailing): q = sum >> k, r = sum & (N - 1), q + (r > N/2 or (r == N/2 and q odd))."""
    H, W = a.shape[0] // n, a.shape[1] // n
    assert a.shape[0] == n * H and a.shape[1] == n * W
    s = a.reshape((H, n, W, n) + a.shape[2:]).astype(np.uint64).sum(axis=(1, 3))
    N = n * n
    k = N.bit_length() - 1
    q, r = s >> np.uint64(k), s & np.uint64(N - 1)
    up = (r > N // 2) | ((r == N // 2) & ((q & np.uint64(1)) == 1))
    return (q + up.astype(np.uint64)).astype(a.dtype)


def block_mean_torch(t, n: int):
    """block_mean of a uint8 (n H, n W, C) CUDA tensor, on the device (full-size frames)."""
    import torch

    H, W = t.shape[0] // n, t.shape[1] // n
    s = t.view(H, n, W, n, *t.shape[2:]).to(torch.int32).sum(dim=(1, 3))
    N = n * n
    k = N.bit_length() - 1
    q, r = s >> k, s & (N - 1)
    up = (r > N // 2) | ((r == N // 2) & ((q & 1) == 1))
    return (q + up.to(torch.int32)).to(t.dtype)


def orc_proj_ss(p, n: int) -> orc.Proj:
    """The oracle's n x destination of a case tuple: image (n H, n W) - a double fisheye's map width 2 (W // 2) - and n x the magnitude."""
    kind, h, w, lens, fov, mag = p
    if kind == "pano":
        return orc.Proj("pano", n * h, n * w)
    if kind == "double":
        return orc.Proj("double", n * h, n * 2 * (w // 2), lens, orc.to_radians(fov))
    return orc.Proj("camera", n * h, n * w, lens, orc.to_radians(fov), (h / 2.0 if mag is None else mag) * n)


def reference(case, n: int, frame: np.ndarray, bilinear: bool = False) -> np.ndarray:
    """What the supersampled call must return for a case (tests/cases.py) at factor n."""
    from tests import helpers as H

    od, os_ = orc_proj_ss(case.dst, n), H.orc_proj(case.src)
    rots = H.orc_rots(case)
    with np.errstate(all="ignore"):
        full = orc.remap_bilinear(od, os_, frame, rots) if bilinear else orc.remap(od, os_, frame, rots)
    return block_mean(full, n)
