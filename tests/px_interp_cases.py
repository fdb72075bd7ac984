"""What tests/test_hip_px_interp.py runs pb_remap_interp_px on and how far a sample may lie from its definition, shared with
the CPU conditions on both (tests/test_px_interp_host.py)."""

from tests import interp_cases as ic
from tests import video_bilinear_ref as vb

# every case of tests/interp_cases.py whose source the tile kernels serve (a double-fisheye source is refused)
CASES = [c for c in ic.SWEEP + ic.TINY + ic.MAGNIFIED + [ic.ODD_DST] if c.src[0] != "double"]
# the cases that run every format: a camera and a panorama source of the sweep, a panorama that wraps a tap twice, a source smaller than the
# footprint, partial tiles both ways, the pole and the seam across tiles, a destination of odd width
ALL_FORMAT_CASES = ("sweep3", "sweep5", "tiny_pano_2x4_rot", "tiny_cam_3x5", "tiny_dst_33x35", "mag_pano_pole_and_seam", "odd_dst_61x35")
FORMATS = [(1, 1), (2, 1), (4, 1), (1, 2), (2, 2), (3, 2), (4, 2)]  # (channels, sample_bytes) of pb_px_interp_kernel; (3, 1) is the RGB8 kernels'
BAND = 1.0 / 512.0  # twice the tile models' certified bound PB_COARSE_PX = 1/1024 px
# The edge band may excuse a pixel that is black in one result only.  It holds at most 0.5 % of a case's pixels, except here: the only
# one-row source, whose every output row runs along the frame's two long edges - its count is pinned, and nothing outside it is excused.
PINNED_BANDS = {"tiny_cam_1x6": 32}


def tolerance(interpolation: str, R: int) -> int:
    """How far a sample may lie from its definition when R is the largest sample value of the source frame: the tile coordinates are
    certified to 1/1024 px per axis.
      bilinear      video_bilinear_ref.tolerance: T(R) = 1 + floor(R / 512).
      catmull-rom   DESIGN 3.8's budget with R in place of 255: sum |w| <= 1.25 and sum |w'| <= 3, taps at most R / 2 from mid-range, so the
                    unrounded values differ by at most (R / 2) (1.25 x 3 + 3 x 1.25) / 1024 = 15 R / 4096; the float32 arithmetic has R 2^-18
                    (pb_kernels_px_interp.hpp shows its own bound below that).  T_cr(R) = 1 + floor(15 R / 4096 + R 2^-18)."""
    if interpolation == "bilinear":
        return vb.tolerance(R)
    assert interpolation == "catmull-rom", interpolation
    return 1 + (15 * int(R) * 64 + int(R)) // (1 << 18)  # (15 R / 4096 = 960 R / 2^18: exact in integers)
