"""The RGB8 double-fisheye stitch (pb_remap_u8 of a double source: pb_hot_double_kernel, pb_sep_double_kernel, pb_remap_kernel) against
the CPU oracle's bytes: the definition, the frames and the case lists of tests/test_double_cases_host.py (which shows, on the CPU, that
the oracle alone meets every condition the GPU tests rely on) and tests/test_hip_double_tiles.py.  No GPU.

stitch_rgb is tests/stitch_video_ref.blend per channel with fill 0 - no second arithmetic.  Two frames: independent random bytes,
unmasked (sums that wrap, negative sums, NaN sums), and a frame that is CONSTANT per channel, the factor probe: with both taps equal
c * fl + c * fr sits on an integer wherever fl + fr is 1, so the truncation follows the factors' last bit."""

from __future__ import annotations

import os

import numpy as np

from tests import helpers as H
from tests import stitch_video_ref as ref
from tests.cases import Case, cam, dbl, inscribed, pano

PROBE = (255, 128, 1)  # the constant frame's channels: the largest byte, a power of two, the smallest that is not black
PROBE16 = (65535, 32768, 1)  # ... of a 16-bit plane


def stitch_rgb(image, il, ir, fl, fr, w):
    """(h, w, 3) uint8 image, the taps and factors of an (H, W) destination, the source width -> (H, W, 3) uint8."""
    image = np.asarray(image)
    assert image.dtype == np.uint8 and image.ndim == 3 and image.shape[1:] == (w, 3)
    return np.stack([ref.blend(image[..., c], il, ir, fl, fr, w, 0, 0, 0) for c in range(3)], axis=2)


def random_rgb(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def constant_rgb(h, w, rgb=PROBE):
    return np.broadcast_to(np.array(rgb, np.uint8), (h, w, 3)).copy()


EDGES = [
    Case("edge_1x1", pano(1, 1), dbl(40, 80, "equidistant", 195)),  # smallest destination
    Case("edge_2x2", pano(2, 2), dbl(40, 80, "equidistant", 195)),
    Case("edge_33x65_rot", pano(33, 65), dbl(40, 80, "equidistant", 195), [(3, 90, -7)]),  # partial tiles on both axes; a row's dword alignment changes from row to row
    Case("edge_34x66_src2x4", pano(34, 66), dbl(2, 4, "equidistant", 195)),  # a 2 x 4 source: its last pixel (index 7) is sampled
    Case("edge_45x91_src41x82", pano(45, 91), dbl(41, 82, "equisolid", 200), [(20, 30, 40)]),  # odd source height, odd eye width
    Case("edge_66x66_inscribed", cam(66, 66, "equidistant", 360, inscribed(66)), dbl(40, 80, "equidistant", 195), [(20, 30, 40)]),  # black destination pixels
    Case("edge_96x192_row_band", pano(96, 192), dbl(96, 192, "equidistant", 195)),  # a ROW band
    Case("edge_96x192_lat_band", pano(96, 192), dbl(100, 200, "equidistant", 195), [(3, 90, -7)]),  # a LAT band
    # fov 180: the factor's divisor is 0.  The oracle gives this destination NO non-finite factor - its rows lie pi / 126 either side of
    # the equator, the band is 0.5 degrees wide -, so the two cases after it reach them: an odd height puts a row ON the equator
    # (0 / 0: 64 NaN factors, NaN sums), a rotation puts 48 pixels inside the band (infinite factors, sums of -inf)
    Case("edge_64x128_fov180", pano(64, 128), dbl(48, 96, "equidistant", 180)),
    Case("edge_33x64_fov180_nan", pano(33, 64), dbl(48, 96, "equidistant", 180)),
    Case("edge_64x128_fov180_inf", pano(64, 128), dbl(48, 96, "equidistant", 180), [(3, 90, -7)]),
    # every factor is exactly 1 and the plan is rotated: neither row weights nor stored latitudes (the tile kernel's WMODE 0)
    Case("edge_34x34_unit_only", cam(34, 34, "equidistant", 150, inscribed(34)), dbl(40, 80, "equidistant", 195), [(0, 180, 0)]),
]
UNIT_ONLY = ("edge_34x34_unit_only",)
SAMPLES_LAST_PIXEL = ("edge_34x66_src2x4",)
BLACK_PIXELS = {"edge_66x66_inscribed": 1056}
BAND_PIXELS = {"edge_96x192_row_band": 1536, "edge_96x192_lat_band": 1600}
NON_FINITE = {"edge_33x64_fov180_nan": (64, 64), "edge_64x128_fov180_inf": (48, 0), "stitch_180": (2048, 1)}  # name -> (non-finite factors, NaN sums at least)
ALL_FINITE = ("edge_64x128_fov180",)

MID_NAMES = ("stitch_180", "stitch_195_aligned", "stitch_195_rot", "stitch_200_chain", "fisheye_from_double", "double_from_double",
             "stitch_220_raw", "odd_sizes")


def _mid():
    from tests.test_hip_double import CASES  # (needs torch to import, no GPU)

    by_name = {c.name: c for c in CASES}
    return [by_name[n] for n in MID_NAMES]


MID = _mid()  # tests/test_hip_double.CASES, by name


def case_by_name(name):
    return next(c for c in EDGES + MID if c.name == name)


FIXTURE = os.path.join(H.GOLD, "double_tiles.npz")
_TAPS = {}


def oracle_taps(case):
    """(il, ir, fl, fr) of the live CPU oracle, computed once per case and shared: callers leave the arrays unchanged."""
    if case.name not in _TAPS:
        _TAPS[case.name] = ref.oracle_taps(case)
    return _TAPS[case.name]


def fixture_taps(case, gold=None):
    """(il, ir, fl, fr) of an EDGES case as tests/make_double_goldens.py stored them: the oracle's on the goldens' platform."""
    g = np.load(FIXTURE) if gold is None else gold
    n = case.name
    return g[f"{n}/il"], g[f"{n}/ir"], g[f"{n}/fl"].view(np.float64), g[f"{n}/fr"].view(np.float64)


def black(il, ir):
    return (il < 0) & (ir < 0)


def band(il, ir, fl, fr):
    """The merge band: pixels where both eyes are live and a factor is finite and not exactly 1 - where the blend depends on the factors'
    bits.  (A non-finite factor, fov 180's, has no last bit to show: the sum stays outside the cast's range whatever it is nudged to.)"""
    return (il >= 0) & (ir >= 0) & ((fl != 1.0) | (fr != 1.0)) & np.isfinite(fl) & np.isfinite(fr)


def sums(image, il, ir, fl, fr, w):
    """The float64 sums a_l * fl + a_r * fr before the cast, (H, W, 3): what the frames make the blend meet."""
    image = np.asarray(image)
    rl, cl = np.divmod(np.where(il < 0, 0, il), w)
    rr, cr = np.divmod(np.where(ir < 0, 0, ir), w)
    a_l = np.where((il < 0)[..., None], 0.0, image[rl, cl].astype(np.float64))
    a_r = np.where((ir < 0)[..., None], 0.0, image[rr, cr].astype(np.float64))
    with np.errstate(all="ignore"):
        return a_l * fl[..., None] + a_r * fr[..., None]


def frames_of(case):
    """{"random": ..., "constant": ...} for a case's source."""
    _, h, w, *_ = case.src
    return {"random": random_rgb(h, w, seed=7000 + [c.name for c in EDGES + MID].index(case.name)), "constant": constant_rgb(h, w)}
