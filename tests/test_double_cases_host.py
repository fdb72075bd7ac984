"""What tests/test_hip_double_tiles.py takes for granted, shown on the CPU with the oracle alone (tests/double_cases.py): the definition
IS the oracle's remap, the fixture IS the oracle's run, the named cases hold what their names say, and the constant frame shows the last
bit of a blend factor.  Without these the GPU comparisons would prove nothing."""

import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import reference_path as orc
from tests import double_cases as dc
from tests import helpers as H

ALL = dc.EDGES + dc.MID


def test_the_lists_are_the_specified_ones():
    assert len(dc.EDGES) == 12 and len({c.name for c in ALL}) == len(ALL)
    assert tuple(c.name for c in dc.MID) == dc.MID_NAMES and {"stitch_195_aligned", "stitch_195_rot"} <= set(dc.MID_NAMES)
    assert all(c.src[0] == "double" for c in ALL)
    assert max(c.dst[1] * c.dst[2] for c in dc.EDGES) == 18432
    assert [c.dst[1:3] for c in dc.EDGES[:2]] == [(1, 1), (2, 2)]


@pytest.mark.parametrize("case", ALL, ids=lambda c: c.name)
def test_the_definition_is_the_oracle_s_remap_on_both_frames(case):
    taps = dc.oracle_taps(case)
    w = case.src[2]
    for what, frame in dc.frames_of(case).items():
        want = orc.remap(H.orc_proj(case.dst), H.orc_proj(case.src), frame.copy(), H.orc_rots(case))
        got = dc.stitch_rgb(frame, *taps, w)
        assert got.dtype == want.dtype == np.uint8 and got.shape == want.shape == (case.dst[1], case.dst[2], 3)
        assert np.array_equal(got, want), (case.name, what, int((got != want).sum()))


def test_the_frames_are_what_they_are_called():
    a, b = dc.random_rgb(40, 80, 1), dc.random_rgb(40, 80, 2)
    assert a.dtype == np.uint8 and a.shape == (40, 80, 3) and not np.array_equal(a, b) and np.array_equal(a, dc.random_rgb(40, 80, 1))
    assert len(np.unique(a)) == 256  # unmasked, every byte value
    c = dc.constant_rgb(3, 5)
    assert c.dtype == np.uint8 and c.shape == (3, 5, 3) and c.flags.writeable and bool((c == np.array(dc.PROBE, np.uint8)).all())


def test_the_fixture_is_a_live_oracle_run():
    if not H.live_numpy_is_the_goldens_numpy():
        pytest.skip("the live oracle's last bits are this host's NumPy's: the fixture holds the goldens' platform's")
    gold = np.load(dc.FIXTURE)
    assert sorted(gold.files) == sorted(f"{c.name}/{k}" for c in dc.EDGES for k in ("il", "ir", "fl", "fr"))
    for case in dc.EDGES:
        for got, want in zip(dc.fixture_taps(case, gold), dc.oracle_taps(case)):
            assert got.dtype == want.dtype and got.shape == want.shape
            assert np.array_equal(got.view(np.int32 if got.dtype == np.int32 else np.uint64), want.view(np.int32 if want.dtype == np.int32 else np.uint64)), case.name


def test_the_generator_writes_the_committed_fixture_byte_for_byte(tmp_path):
    if not H.live_numpy_is_the_goldens_numpy():
        pytest.skip("the generator runs on the goldens' platform only")
    out = tmp_path / "double_tiles.npz"
    subprocess.run([sys.executable, "tests/make_double_goldens.py", str(out)], check=True, cwd=os.path.dirname(os.path.dirname(H.GOLD)), capture_output=True)
    with open(dc.FIXTURE, "rb") as f:
        assert out.read_bytes() == f.read()


@pytest.mark.parametrize("case", dc.EDGES, ids=lambda c: c.name)
def test_the_fixture_s_taps_are_in_bounds(case):
    """On any host: what the GPU tests feed the definition with."""
    il, ir, fl, fr = dc.fixture_taps(case)
    _, h, w, *_ = case.src
    for idx in (il, ir):
        assert idx.dtype == np.int32 and idx.shape == (case.dst[1], case.dst[2]) and int(idx.min()) >= -1 and int(idx.max()) < h * w
    assert bool((il[il >= 0] % w < w // 2).all()) and bool((ir[ir >= 0] % w >= w // 2).all())  # each eye's taps stay in its half


def test_the_named_cases_hold_what_they_are_named_for():
    for name in dc.SAMPLES_LAST_PIXEL:
        case = dc.case_by_name(name)
        il, ir, _, _ = dc.oracle_taps(case)
        assert max(int(il.max()), int(ir.max())) == case.src[1] * case.src[2] - 1, name
    for name, n in dc.BLACK_PIXELS.items():
        il, ir, _, _ = dc.oracle_taps(dc.case_by_name(name))
        assert int(dc.black(il, ir).sum()) == n, name
    for name, n in dc.BAND_PIXELS.items():
        assert int(dc.band(*dc.oracle_taps(dc.case_by_name(name))).sum()) == n, name
    for name, (n_factors, n_nan_sums) in dc.NON_FINITE.items():
        case = dc.case_by_name(name)
        assert case.src[4] == 180.0
        il, ir, fl, fr = dc.oracle_taps(case)
        assert int((~np.isfinite(fl) | ~np.isfinite(fr)).sum()) == n_factors >= 1, name
        s = dc.sums(dc.frames_of(case)["random"], il, ir, fl, fr, case.src[2])
        assert int(np.isnan(s).any(axis=2).sum()) >= n_nan_sums, name
    assert any(n >= 1 for _, n in dc.NON_FINITE.values())
    for name in dc.ALL_FINITE:
        _, _, fl, fr = dc.oracle_taps(dc.case_by_name(name))
        assert bool(np.isfinite(fl).all() and np.isfinite(fr).all()), name
    for name in dc.UNIT_ONLY:
        case = dc.case_by_name(name)
        il, ir, fl, fr = dc.oracle_taps(case)
        assert case.rotations and bool((fl == 1.0).all() and (fr == 1.0).all()) and int(((il >= 0) & (ir >= 0)).sum()) > 0, name
    # the odd sizes: a destination row of 65 * 3 bytes changes its dword alignment from row to row; odd source height, odd eye width
    assert (dc.case_by_name("edge_33x65_rot").dst[2] * 3) % 4 and dc.case_by_name("edge_45x91_src41x82").src[1] & 1 and (dc.case_by_name("edge_45x91_src41x82").src[2] // 2) & 1


@pytest.mark.parametrize("case", dc.MID, ids=lambda c: c.name)
def test_the_random_frame_makes_the_blend_wrap_and_at_fov_180_go_negative(case):
    il, ir, fl, fr = dc.oracle_taps(case)
    s = dc.sums(dc.frames_of(case)["random"], il, ir, fl, fr, case.src[2])
    with np.errstate(all="ignore"):
        wraps, negative = int((s >= 256.0).any(axis=2).sum()), int((s < 0.0).any(axis=2).sum())
    print(f"{case.name}: {wraps} pixels whose sum wraps, {negative} with a negative sum, {int(np.isnan(s).any(axis=2).sum())} with a NaN sum")
    assert wraps >= 1000, case.name
    if case.name == "stitch_180":
        assert negative >= 1000


BANDED = [c for c in ALL if int(dc.band(*dc.oracle_taps(c)).sum()) >= 100]


def test_the_probe_covers_the_row_and_the_latitude_bands():
    names = {c.name for c in BANDED}
    assert set(dc.BAND_PIXELS) <= names and {"stitch_195_aligned", "stitch_195_rot"} <= names and len(names) >= 10, names


@pytest.mark.parametrize("case", BANDED, ids=lambda c: c.name)
def test_the_constant_frame_shows_a_one_ulp_error_of_a_factor(case):
    """fl one ulp toward zero on the band's pixels only: at least a quarter of those pixels change on the constant frame (and next to none
    of a random frame's - printed, the reason the constant frame exists)."""
    il, ir, fl, fr = dc.oracle_taps(case)
    w = case.src[2]
    band = dc.band(il, ir, fl, fr)
    n = int(band.sum())
    with np.errstate(all="ignore"):
        off = np.where(band, np.nextafter(fl, 0.0), fl)
    frames = dc.frames_of(case)
    moved = {k: (dc.stitch_rgb(f, il, ir, off, fr, w) != dc.stitch_rgb(f, il, ir, fl, fr, w)) for k, f in frames.items()}
    assert not bool((moved["constant"].any(axis=2) & ~band).any())
    pixels = int(moved["constant"].any(axis=2).sum())
    print(f"{case.name}: band {n} pixels; fl one ulp off moves {pixels} pixels ({100.0 * pixels / n:.0f} %), {int(moved['constant'].sum())} bytes of the "
          f"constant frame, {int(moved['random'].sum())} bytes of the random frame")
    assert 4 * pixels >= n, (case.name, pixels, n)
