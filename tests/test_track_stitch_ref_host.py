"""The definition the tracked double-fisheye video stitch uses (pb_track_stitch_planar / pb_track_stitch_nv12) against the
reference's own output for a rotation track: tests/stitch_video_ref.py fed with the CPU oracle's taps and factors of the chain "the plan's
own rotations, then frame f's" gives, at 4:4:4 uint8 with fill (0, 0, 0), the three channels the rotation-track fixture holds
(tests/golden/rotation_track.npz, written from the reference) - for both double-fisheye cases, eight frames.  The CPU oracle only: no GPU,
no library.  It pins the definition the GPU tests compare with."""

import os

import numpy as np
import pytest

from oracle import reference_path as orc
from tests import helpers as H
from tests import rotation_track_cases as rc
from tests import stitch_video_ref as ref

GOLD = np.load(os.path.join(H.GOLD, "rotation_track.npz"))
DOUBLE = {c.name: c for c in rc.golden_cases() if c.src[0] == "double"}


def chain_taps(dst, src, chain):
    """(il, ir, fl, fr) of a chain of rotations in degrees, from the CPU oracle."""
    with np.errstate(all="ignore"):
        il, ir, fl, fr, _ = orc.remap_index(H.orc_proj(dst), H.orc_proj(src), [tuple(map(orc.to_radians, r)) for r in chain])
    return il, ir, fl, fr


def test_the_fixture_holds_two_double_fisheye_cases_of_four_frames():
    assert sorted(DOUBLE) == ["T_double_180_seam", "T_double_195"] and all(len(c.frames) == 4 for c in DOUBLE.values())
    assert DOUBLE["T_double_195"].plan_rot == [] and len(DOUBLE["T_double_180_seam"].plan_rot) == 1
    assert all(len(fr) == 1 for c in DOUBLE.values() for fr in c.frames)


@pytest.mark.parametrize("name", sorted(DOUBLE))
def test_at_444_uint8_fill_0_the_planes_are_the_channels_of_the_reference_s_track(name):
    case = DOUBLE[name]
    _, h, w, *_ = case.src
    frames = rc.case_frames(case)
    exact = H.live_numpy_is_the_goldens_numpy()
    two_eyes = none = 0
    for f in range(4):
        il, ir, fl, fr = chain_taps(case.dst, case.src, case.chain(f))
        assert il.dtype == ir.dtype == np.int32 and fl.dtype == fr.dtype == np.float64
        image = frames[f]
        outs = ref.stitch_planar(image[..., 0], image[..., 1], image[..., 2], il, ir, fl, fr, w, "444", (0, 0, 0))
        got = np.stack(outs, axis=2)
        want, want_l, want_r = GOLD[f"{name}/{f}/u8"], GOLD[f"{name}/{f}/idx_l"], GOLD[f"{name}/{f}/idx_r"]
        if exact:
            assert np.array_equal(il, want_l) and np.array_equal(ir, want_r), (name, f)
            assert np.array_equal(got, want), (name, f)
        else:  # (the fixture is the goldens' platform's: a last-bit difference of this host's NumPy may move a fragile pixel's tap)
            with np.errstate(all="ignore"):
                fragile = orc.fragile_mask(orc.pretrunc(H.orc_proj(case.dst), H.orc_proj(case.src), [tuple(map(orc.to_radians, r)) for r in case.chain(f)]))
            assert not ((il != want_l) & ~fragile).any() and not ((ir != want_r) & ~fragile).any(), (name, f)
            same_taps = (il == want_l) & (ir == want_r)
            assert np.array_equal(got[same_taps & (fl == 1.0) & (fr == 1.0)], want[same_taps & (fl == 1.0) & (fr == 1.0)]), (name, f)
        two_eyes += int(((il >= 0) & (ir >= 0)).sum())
        none += int(((il < 0) & (ir < 0)).sum())
    # the cases are not trivial: both eyes live somewhere; the fisheye destination has invalid pixels
    assert two_eyes > 0 and (none > 0 or name != "T_double_195")
