"""The definition of the double-fisheye video stitch (tests/stitch_video_ref.py) against the reference's own stitch, and the
rules it adds for subsampled planes, wider samples and fills.  The CPU oracle only: no GPU, no library."""

import numpy as np
import pytest

from oracle import reference_path as orc
from tests import cases as tc
from tests import helpers as H
from tests import stitch_video_ref as ref

CASES = ("E_stitch_195_raw", "E_stitch_180_masked", "E_stitch_eqs_rot")


def random_planes(h, w, sub, dt, seed):
    cx, cy = ref.SHIFTS[sub]
    rng = np.random.default_rng(seed)
    hi = np.iinfo(dt).max + 1
    return [rng.integers(0, hi, shp).astype(dt) for shp in ((h, w), (h >> cy, w >> cx), (h >> cy, w >> cx))]


@pytest.fixture(scope="module")
def taps():
    return {name: ref.oracle_taps(tc.case_by_name(name)) for name in CASES}


def oracle_stitch(case, image):
    with np.errstate(all="ignore"):
        return orc.remap(H.orc_proj(case.dst), H.orc_proj(case.src), image, H.orc_rots(case))


@pytest.mark.parametrize("name", CASES)
def test_at_444_uint8_fill_0_the_planes_are_the_channels_of_the_reference_s_stitch(name, taps):
    case = tc.case_by_name(name)
    _, h, w, *_ = case.src
    il, ir, fl, fr = taps[name]
    assert il.dtype == ir.dtype == np.int32 and fl.dtype == fr.dtype == np.float64
    for seed, image in ((0, H.case_frame(case)), (21, np.stack(random_planes(h, w, "444", np.uint8, 21), axis=2))):
        want = oracle_stitch(case, image)
        outs = ref.stitch_planar(image[..., 0], image[..., 1], image[..., 2], il, ir, fl, fr, w, "444", (0, 0, 0))
        assert np.array_equal(np.stack(outs, axis=2), want), (name, seed)
    # the cases are not trivial: both eyes live somewhere, one eye alone somewhere, nothing live somewhere or a factor off 1 somewhere
    assert int(((il >= 0) & (ir >= 0)).sum()) > 0 and int(((il >= 0) ^ (ir >= 0)).sum()) > 0
    if "180" not in name:  # (at 180 degrees the merge band is empty: no pixel of a 32-row panorama lies in it)
        assert int(((fl != 1.0) | (fr != 1.0)).sum()) > 0


@pytest.mark.parametrize("name", CASES[:2])  # (E_stitch_eqs_rot's destination is 33 rows: 4:2:2 only)
@pytest.mark.parametrize("sub", ("420", "422"))
def test_plane_0_is_the_stitch_of_a_grey_image_and_chroma_is_that_stitch_at_the_anchors(name, sub, taps):
    case = tc.case_by_name(name)
    _, h, w, *_ = case.src
    il, ir, fl, fr = taps[name]
    cx, cy = ref.SHIFTS[sub]
    p0, p1, p2 = random_planes(h, w, sub, np.uint8, 22)
    o0, o1, o2 = ref.stitch_planar(p0, p1, p2, il, ir, fl, fr, w, sub, (0, 0, 0))
    assert np.array_equal(o0, oracle_stitch(case, np.stack([p0] * 3, axis=2))[..., 0])
    Hd, Wd = il.shape
    assert o1.shape == o2.shape == (Hd >> cy, Wd >> cx)
    # the anchor rule, sample by sample, written out without the definition's own helpers
    for plane, out in ((p1, o1), (p2, o2)):
        for i in range(Hd >> cy):
            for j in range(Wd >> cx):
                y, x = i << cy, j << cx
                l, r = int(il[y, x]), int(ir[y, x])
                if l < 0 and r < 0:
                    assert out[i, j] == 0
                    continue
                a = 0.0 if l < 0 else float(plane[(l // w) >> cy, (l % w) >> cx])
                b = 0.0 if r < 0 else float(plane[(r // w) >> cy, (r % w) >> cx])
                with np.errstate(all="ignore"):
                    v = np.float64(a) * fl[y, x] + np.float64(b) * fr[y, x]
                want = (int(v) & 0xFF) if np.isfinite(v) and abs(v) < 2.0**31 else 0
                assert int(out[i, j]) == want, (i, j)


def test_at_422_the_odd_destination_height_is_allowed():
    case = tc.case_by_name("E_stitch_eqs_rot")
    _, h, w, *_ = case.src
    il, ir, fl, fr = ref.oracle_taps(case)
    assert il.shape == (33, 66)
    p0, p1, p2 = random_planes(h, w, "422", np.uint8, 23)
    o0, o1, o2 = ref.stitch_planar(p0, p1, p2, il, ir, fl, fr, w, "422", (0, 0, 0))
    assert o1.shape == (33, 33) and np.array_equal(o0, oracle_stitch(case, np.stack([p0] * 3, axis=2))[..., 0])
    with pytest.raises(AssertionError):
        ref.stitch_planar(*random_planes(h, w, "420", np.uint8, 23), il, ir, fl, fr, w, "420", (0, 0, 0))


def test_the_cast_is_the_definition_s_at_both_widths():
    v = np.array([0.0, 255.9, 256.0, 300.0, -1.0, -0.5, 65535.5, 65536.0, 70000.0, 2.0**31 - 1, 2.0**31, -(2.0**31), np.nan, np.inf, -np.inf])
    assert ref.cast(v, np.uint8).tolist() == [0, 255, 0, 44, 255, 0, 255, 0, 112, 255, 0, 0, 0, 0, 0]
    assert ref.cast(v, np.uint16).tolist() == [0, 255, 256, 300, 65535, 0, 65535, 0, 4464, 65535, 0, 0, 0, 0, 0]


@pytest.mark.parametrize("name", CASES)
def test_uint16_samples_wrap_at_two_to_the_sixteen(name, taps):
    case = tc.case_by_name(name)
    _, h, w, *_ = case.src
    il, ir, fl, fr = taps[name]
    sub = "422" if il.shape[0] & 1 else "420"
    p0, p1, p2 = random_planes(h, w, sub, np.uint16, 24)
    o0, o1, o2 = ref.stitch_planar(p0, p1, p2, il, ir, fl, fr, w, sub, (0, 0, 0))
    assert o0.dtype == o1.dtype == o2.dtype == np.uint16
    live = (il >= 0) | (ir >= 0)
    l = np.where(il < 0, 0.0, p0.ravel()[np.where(il < 0, 0, il)].astype(np.float64))
    r = np.where(ir < 0, 0.0, p0.ravel()[np.where(ir < 0, 0, ir)].astype(np.float64))
    with np.errstate(all="ignore"):
        v = l * fl + r * fr
    fin = live & np.isfinite(v)
    assert np.array_equal(o0[fin].astype(np.int64), np.trunc(v[fin]).astype(np.int64) & 0xFFFF)
    # a 10-bit sample stored low wraps at 2^16, not at 2^10: where both eyes add with unit factors the sum exceeds 1023 and is kept
    q0, q1, q2 = (p & 1023 for p in (p0, p1, p2))
    s0, _, _ = ref.stitch_planar(q0, q1, q2, il, ir, fl, fr, w, sub, (0, 0, 0))
    both_unit = (il >= 0) & (ir >= 0) & (fl == 1.0) & (fr == 1.0)
    if both_unit.any():
        assert int(s0[both_unit].max()) > 1023
    assert int(s0.max()) < 4096


@pytest.mark.parametrize("name", CASES)
def test_the_fill_goes_only_where_both_taps_are_black(name, taps):
    case = tc.case_by_name(name)
    _, h, w, *_ = case.src
    il, ir, fl, fr = taps[name]
    sub = "422"
    cx, cy = ref.SHIFTS[sub]
    ps = random_planes(h, w, sub, np.uint8, 25)
    zero = ref.stitch_planar(*ps, il, ir, fl, fr, w, sub, (0, 0, 0))
    fill = (201, 202, 203)
    outs = ref.stitch_planar(*ps, il, ir, fl, fr, w, sub, fill)
    none = (il < 0) & (ir < 0)
    for k, (z, o) in enumerate(zip(zero, outs)):
        m = none if k == 0 else none[:: 1 << cy, :: 1 << cx]
        assert np.array_equal(o[~m], z[~m]) and (o[m] == fill[k]).all()
    # one eye black beside a live one contributes 0.0: the live eye's sample times its factor, never the fill
    one = (il >= 0) & (ir < 0) & (fl == 1.0)
    assert one.any() and np.array_equal(outs[0][one], ps[0].ravel()[il[one]])
    # the packed-frame form and the NV12 interleave
    flat = ref.stitch_frame(np.concatenate([p.ravel() for p in ps]), il, ir, fl, fr, h, w, sub, fill)
    assert np.array_equal(flat, np.concatenate([o.ravel() for o in outs])) and flat.size == ref.frame_samples(*il.shape, sub)
    if not il.shape[0] & 1:
        f420 = np.concatenate([p.ravel() for p in random_planes(h, w, "420", np.uint8, 26)])
        nv = ref.nv12_of(f420, h, w)
        assert nv.size == f420.size and np.array_equal(nv[: h * w], f420[: h * w]) and np.array_equal(nv[h * w :: 2], f420[h * w : h * w + h * w // 4])
