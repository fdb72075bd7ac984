"""pb_remap_planar: planar video frames - three planes at 4:4:4, 4:2:2 or 4:2:0, uint8 or uint16 samples - through the tile
kernel pb_video_hot_kernel: the bytes of the definition (tests/planar_ref.py) with the reference's index map, for both sample sizes and
the three subsamplings, every tile class, edge, layout and launch shape.  Every comparison is exact equality; frames are independent
random bytes per plane (a wrong index or a wrong plane shows), destinations sit between sentinel bytes that must survive, and so must the
padding bytes inside pitched frames."""

import os

import numpy as np
import pytest
import torch

from oracle import reference_path as orc
from photonbend_amd import _hostpipe, batch
from photonbend_amd import _native as nat
from tests import cases as tc
from tests import cubemap_cases as cc
from tests import cubemap_ref as cr
from tests import helpers as H
from tests import planar_ref
from tests import polynomial_cases as pc
from tests.cases import Case, cam, pano
from tests.test_hip_nv12 import EDGES, GUARD, SENTINEL, _fix_pixels, guarded, guards_intact, nv12_call
from tests.test_hip_pixel_formats import MID, _mid_plan  # (the four mid cases of the pixel-format tests, and their plans)
from tests.test_planar_ref_host import EDGE_CASES

pytestmark = pytest.mark.gpu

SAMPLES = ((1, np.uint8), (2, np.uint16))
SUBS = {"444": nat.PLANAR_444, "422": nat.PLANAR_422, "420": nat.PLANAR_420}
INVALID, UNSUPPORTED = -1, -3
SMALL = H.load_small()
GOLD_CUBE = np.load(os.path.join(H.GOLD, "cubemap.npz"))
GOLD_POLY = np.load(os.path.join(H.GOLD, "polynomial.npz"))


def dims_ok(case, sub):
    return planar_ref.dims_ok(sub, case.src[1:3], case.dst[1:3])


def random_frame(h, w, sub, dt, seed):
    """A packed flat frame of independent random bytes."""
    n = planar_ref.frame_samples(h, w, sub) * np.dtype(dt).itemsize
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).view(dt)


def planar_call(plan, src_ptr, dst_ptr, sub, S, n=1, sl=None, dl=None, fill=None, stream=None):
    sl = None if sl is None else nat.pb_planar_layout(*sl)
    dl = None if dl is None else nat.pb_planar_layout(*dl)
    f = None if fill is None else (nat.C.c_uint16 * 3)(*fill)
    return nat.load().pb_remap_planar(plan.handle, src_ptr, dst_ptr, n, None if sl is None else nat.C.addressof(sl), None if dl is None else nat.C.addressof(dl),
                                      SUBS[sub], S, None if f is None else nat.C.addressof(f), nat.current_stream() if stream is None else stream)


def run_planar(plan, frame, sub, fill=None):
    """One packed pb_remap_planar launch of a flat frame -> the destination's flat frame; the guards around it must survive."""
    S = frame.dtype.itemsize
    src = torch.from_numpy(frame.view(np.uint8)).cuda()
    buf = guarded(planar_ref.frame_samples(plan.dst.height, plan.dst.width, sub) * S)
    assert planar_call(plan, src.data_ptr(), buf.data_ptr() + GUARD, sub, S, fill=fill) == 0, nat.load().pb_last_error()
    torch.cuda.synchronize()
    assert guards_intact(buf), "pb_remap_planar wrote outside the destination frame"
    return buf[GUARD:-GUARD].cpu().numpy().view(frame.dtype)


def assert_equal(got, want, Hd, Wd, sub, fragile, exact, what):
    """The treatment of tests/test_hip_nv12.py: nothing differs outside the fragile set (for planes 1 and 2: the anchors'), and nothing
    at all where the index is the goldens' platform's."""
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    cx, cy = planar_ref.SHIFTS[sub]
    bad = [g != w for g, w in zip(planar_ref.planes(got, Hd, Wd, sub), planar_ref.planes(want, Hd, Wd, sub))]
    if fragile is not None:
        fa = fragile[0 :: 1 << cy, 0 :: 1 << cx]
        out = [int((bad[0] & ~fragile).sum()), int((bad[1] & ~fa).sum()), int((bad[2] & ~fa).sum())]
        assert out == [0, 0, 0], f"{what}: {out} samples of planes 0, 1, 2 differ outside the fragile set"
    if exact:
        assert [int(b.sum()) for b in bad] == [0, 0, 0], f"{what}: {[int(b.sum()) for b in bad]} samples of planes 0, 1, 2 differ"


def check(plan, case, idx, fragile, exact, seed, subs=planar_ref.SUBSAMPLINGS):
    """Both sample sizes, the subsamplings the case's dimensions allow, the default fill and (1, 2, 3)."""
    _, h, w, *_ = case.src
    Hd, Wd = idx.shape
    ran = 0
    for sub in subs:
        if not dims_ok(case, sub):
            continue
        for S, dt in SAMPLES:
            assert plan.planar_supported(sub, S), (case.name, sub, S)
            frame = random_frame(h, w, sub, dt, seed + 10 * S + SUBS[sub])
            for fill in (None, (1, 2, 3)):
                assert_equal(run_planar(plan, frame, sub, fill), planar_ref.remap_frame(frame, idx, h, w, sub, fill), Hd, Wd, sub, fragile, exact,
                             f"{case.name} {sub} S={S} fill={fill}")
                ran += 1
    return ran


# ---- 1. the small case matrices against the reference's golden index maps -------------------------------------------------------------
def _small_plans():
    out = []
    for c in tc.small_cases():
        if c.src[0] != "double":
            fragile = np.unpackbits(SMALL[f"{c.name}/fragile"])[: c.dst[1] * c.dst[2]].reshape(c.dst[1], c.dst[2]).astype(bool)
            out.append((c, lambda c=c: H.pb_plan_private(c, bilinear=False), SMALL[f"{c.name}/idx"], fragile))
    for mod, gold in ((cc, GOLD_CUBE), (pc, GOLD_POLY)):
        for c in mod.small_cases():
            if c.src[0] != "double":
                def make(c=c, mod=mod):
                    src, cmap = mod.pb_chain(c, image=np.zeros((c.src[1], c.src[2], 3), np.uint8))
                    return nat.Plan(cmap.dst_proj, cmap.rotations, src._proj("src"), bilinear=False)
                out.append((c, make, gold[f"{c.name}/idx"], None))
    return out


SMALL_PLANS = _small_plans()
ODD = ("A_photo_odd", "B_pano_odd")  # 33 x 35 and 31 x 63: served at 4:4:4, invalid at 4:2:0


def test_the_small_cases_cover_every_subsampling_and_the_two_odd_ones():
    names = {p[0].name for p in SMALL_PLANS}
    assert set(ODD) <= names
    for sub in planar_ref.SUBSAMPLINGS:
        assert sum(dims_ok(p[0], sub) for p in SMALL_PLANS) >= 49, sub
    assert all(dims_ok(tc.case_by_name(n), "444") and not dims_ok(tc.case_by_name(n), "420") for n in ODD)


@pytest.mark.parametrize("case,make_plan,idx,fragile", SMALL_PLANS, ids=[p[0].name for p in SMALL_PLANS])
def test_small_cases_equal_the_definition_with_the_golden_index(case, make_plan, idx, fragile):
    plan = make_plan()
    assert check(plan, case, idx, fragile, True, seed=100) >= 4  # (4:4:4 takes every case)
    if case.name in ODD:
        _, h, w, *_ = case.src
        for S, dt in SAMPLES:
            src = torch.zeros(4 * h * w * S, dtype=torch.uint8, device="cuda")
            buf = guarded(4 * case.dst[1] * case.dst[2] * S)
            assert planar_call(plan, src.data_ptr(), buf.data_ptr() + GUARD, "420", S) == INVALID and b"even" in nat.load().pb_last_error()
            torch.cuda.synchronize()
            assert bool((buf == SENTINEL).all())
            with pytest.raises(nat.PbError, match="even"):
                plan.planar_supported("420", S)
    # through Plan.remap_planar with the typed array: same dtype back, into `out`; 4:4:4 also as (3, h, w)
    _, h, w, *_ = case.src
    sub = next(s for s in ("420", "422", "444") if dims_ok(case, s))
    frame = random_frame(h, w, sub, np.uint16, seed=150)
    want = planar_ref.remap_frame(frame, idx, h, w, sub, (1, 2, 3))
    buf = guarded(want.nbytes)
    out = buf[GUARD:-GUARD].view(nat.torch_dtype(np.uint16))
    assert plan.remap_planar(torch.from_numpy(frame).cuda(), sub, out=out, fill=(1, 2, 3)) is out
    torch.cuda.synchronize()
    assert guards_intact(buf)
    assert_equal(out.cpu().numpy(), want, *idx.shape, sub, fragile, True, f"{case.name} remap_planar")
    frame = random_frame(h, w, "444", np.uint8, seed=151)
    got = plan.remap_planar(torch.from_numpy(frame.reshape(3, h, w)).cuda(), nat.PLANAR_444).cpu().numpy()
    assert got.shape == (3,) + idx.shape
    assert_equal(got.ravel(), planar_ref.remap_frame(frame, idx, h, w, "444"), *idx.shape, "444", fragile, True, f"{case.name} (3, h, w)")


# ---- 2. every tile class at mid size, against the oracle --------------------------------------------------------------------------------
def test_mid_cases_contain_every_tile_class_and_fix_pixels_that_are_anchors():
    """The coverage of the test below cannot go silently: its plans hold failed tiles, fix pixels, LEAN, DIRECT and BLACK tiles, a fix
    pixel on an even row and an even column (an anchor at every subsampling) - and one on an ODD row and an even column, an anchor at
    4:2:2 but not at 4:2:0."""
    total = {"fix_tiles": 0, "fix_pixels": 0, "lean_tiles": 0, "direct_tiles": 0, "black_tiles": 0}
    even_even = odd_even = 0
    for case in MID:
        assert dims_ok(case, "420"), case.name
        plan = _mid_plan(case)
        info = plan.info()
        assert info["fast_path"], case.name
        for k in total:
            total[k] += info[k]
        px = _fix_pixels(plan)
        assert len(px) == info["fix_pixels"], case.name
        y, x = np.divmod(px, case.dst[2])
        even_even += int((((y | x) & 1) == 0).sum())
        odd_even += int((((y & 1) == 1) & ((x & 1) == 0)).sum())
    assert all(v >= 1 for v in total.values()), total
    assert even_even >= 1 and odd_even >= 1, (even_even, odd_even)


@pytest.mark.parametrize("case", MID, ids=lambda c: c.name)
def test_mid_cases_equal_the_definition_with_the_oracle_index(case):
    with np.errstate(all="ignore"):
        cmap = cc.ref_stages(case)[-1]
        idx = cc.ref_index(case, cmap)
        if case.src[0] == "cube":
            fragile = orc.fragile_mask(cr.pretrunc(cr.face_size(case.src[1], case.src[2]), np.copy(cmap)))
        else:
            fragile = orc.fragile_mask(orc.pretrunc(H.orc_proj(case.dst), H.orc_proj(case.src), H.orc_rots(case)))
    exact = H.live_numpy_is_the_goldens_numpy()  # (else the live oracle's last bits are this host's: the fragile set is the allowance)
    assert check(_mid_plan(case), case, idx, fragile, exact, seed=200) == 12


# ---- 3. edges ---------------------------------------------------------------------------------------------------------------------------
ALL_EDGES = EDGES + [EDGE_CASES["edge_odd_33x36_src3x6"], EDGE_CASES["edge_odd_33x35_src3x5"],
                     Case("edge_1x2", cam(1, 2, "equidistant", 172), pano(16, 32)),  # one chroma sample at 4:2:2
                     Case("edge_1x1", cam(1, 1, "equidistant", 172), pano(16, 32))]  # ... at 4:4:4
EDGE_RUNS = {"edge_odd_33x36_src3x6": 8, "edge_odd_33x35_src3x5": 4, "edge_1x2": 8, "edge_1x1": 4}  # launches checked (default: 12, all three)


def test_the_edges_are_test_hip_nv12_s_nine_and_four_more():
    assert len(EDGES) == 9 and len(ALL_EDGES) == 13
    for e in EDGES:  # (the conditions asserted by tests/test_planar_ref_host.py hold for these very geometries)
        if e.name in EDGE_CASES:
            assert (e.dst, e.src, e.rotations) == (EDGE_CASES[e.name].dst, EDGE_CASES[e.name].src, EDGE_CASES[e.name].rotations), e.name


@pytest.mark.parametrize("case", ALL_EDGES, ids=lambda c: c.name)
def test_edges_partial_tiles_tiny_sources_mixed_blocks_odd_sizes_and_the_last_sample(case):
    with np.errstate(all="ignore"):
        idx = orc.remap_index(H.orc_proj(case.dst), H.orc_proj(case.src), H.orc_rots(case))
        fragile = orc.fragile_mask(orc.pretrunc(H.orc_proj(case.dst), H.orc_proj(case.src), H.orc_rots(case)))
    plan = H.pb_plan_private(case, bilinear=False)
    assert check(plan, case, idx, fragile, H.live_numpy_is_the_goldens_numpy(), seed=300) == EDGE_RUNS.get(case.name, 12)


# ---- 4. layouts -------------------------------------------------------------------------------------------------------------------------
LAYOUT_CASE = tc.case_by_name("D_photo_rot")


def layouts(h, w, S, sub):
    """name -> (pitch, chroma_pitch, offset1, offset2) of the layouts under test for an h x w frame."""
    cx, cy = planar_ref.SHIFTS[sub]
    cw, ch = w >> cx, h >> cy
    p1, c1 = w * S + 3 * S, cw * S + 5 * S  # a chroma pitch of its own
    p2, c2 = -(-w * S // 256) * 256, -(-cw * S // 64) * 64
    return {
        "pitched": (p1, c1, p1 * h, p1 * h + c1 * ch),
        "pitch_256_64": (p2, c2, p2 * h, p2 * h + c2 * ch),
        "padding_rows_between_the_planes": (p1, c1, p1 * (h + 3), p1 * (h + 3) + c1 * (ch + 2)),
        "planes_1_and_2_swapped": (w * S, cw * S, w * S * h + cw * S * ch, w * S * h),  # YV12
    }


def span(l, h, w, S, sub):
    cx, cy = planar_ref.SHIFTS[sub]
    return max(l[2], l[3]) + l[1] * ((h >> cy) - 1) + (w >> cx) * S


def rows_of(l, h, w, S, sub):
    """(offset, bytes) of every row of the three planes at a layout, in the packed frame's order."""
    cx, cy = planar_ref.SHIFTS[sub]
    out = [(y * l[0], w * S) for y in range(h)]
    for o in (l[2], l[3]):
        out += [(o + y * l[1], (w >> cx) * S) for y in range(h >> cy)]
    return out


def scatter(frame, l, h, w, S, sub, fill_byte=None, seed=0):
    """The packed frame laid out at `l` in a byte buffer whose padding is random (a source) or `fill_byte` (a destination)."""
    flat = frame.view(np.uint8)
    n = span(l, h, w, S, sub)
    buf = np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8) if fill_byte is None else np.full(n, fill_byte, np.uint8)
    at = 0
    for off, nb in rows_of(l, h, w, S, sub):
        buf[off : off + nb] = flat[at : at + nb]
        at += nb
    assert at == len(flat)
    return buf


def gather(buf, l, h, w, dt, sub):
    """(the packed frame found at `l` in a byte buffer, the buffer's bytes outside that frame)."""
    S = np.dtype(dt).itemsize
    pay = np.zeros(len(buf), bool)
    parts = []
    for off, nb in rows_of(l, h, w, S, sub):
        parts.append(buf[off : off + nb])
        assert not pay[off : off + nb].any()
        pay[off : off + nb] = True
    return np.concatenate(parts).view(dt), buf[~pay]


@pytest.mark.parametrize("sub", planar_ref.SUBSAMPLINGS)
@pytest.mark.parametrize("S,dt", SAMPLES)
def test_pitched_planes_padding_rows_swapped_planes_and_a_base_off_dword_alignment(S, dt, sub):
    case = LAYOUT_CASE
    plan = H.pb_plan_private(case, bilinear=False)
    _, h, w, *_ = case.src
    Hd, Wd = case.dst[1], case.dst[2]
    frame = random_frame(h, w, sub, dt, seed=400 + S)
    want = run_planar(plan, frame, sub)
    assert np.array_equal(want, planar_ref.remap_frame(frame, SMALL[f"{case.name}/idx"], h, w, sub))
    A = S  # one sample off dword alignment - 1 byte (S = 1) or 2 bytes (S = 2): the sample-by-sample store path runs
    for (name, sl), dl in zip(layouts(h, w, S, sub).items(), layouts(Hd, Wd, S, sub).values()):
        for off in (0, A):
            ns, nd = span(sl, h, w, S, sub), span(dl, Hd, Wd, S, sub)
            src = torch.zeros(ns + 512, dtype=torch.uint8, device="cuda")
            s_off = (-src.data_ptr()) % 256 + off
            src[s_off : s_off + ns] = torch.from_numpy(scatter(frame, sl, h, w, S, sub, seed=401)).cuda()
            buf = guarded(nd + 512)
            d_off = GUARD + (-(buf.data_ptr() + GUARD)) % 256 + off
            assert (src.data_ptr() + s_off) % 256 == off and (buf.data_ptr() + d_off) % 256 == off
            assert planar_call(plan, src.data_ptr() + s_off, buf.data_ptr() + d_off, sub, S, sl=sl + (0,), dl=dl + (0,)) == 0, (name, nat.load().pb_last_error())
            torch.cuda.synchronize()
            host = buf.cpu().numpy()
            got, padding = gather(host[d_off : d_off + nd], dl, Hd, Wd, dt, sub)
            assert np.array_equal(got, want), (name, off)
            assert bool((padding == SENTINEL).all()) and bool((host[:d_off] == SENTINEL).all()) and bool((host[d_off + nd :] == SENTINEL).all()), (name, off)
    # overlapping planes and a plane beyond frame_stride: PB_ERR_INVALID before any launch, the rule in the message, nothing written
    sl, dl = layouts(h, w, S, sub)["pitched"], layouts(Hd, Wd, S, sub)["pitched"]
    src = torch.zeros(span(sl, h, w, S, sub) + 256, dtype=torch.uint8, device="cuda")
    nd = span(dl, Hd, Wd, S, sub)
    for change, message in (({"dl": (dl[0], dl[1], dl[2], dl[2] + S, 0)}, b"planes overlap"), ({"dl": (dl[0], dl[1], dl[2] - 4 * S, dl[3], 0)}, b"planes overlap"),
                            ({"sl": (sl[0], sl[1], sl[3], sl[3] + S, 0)}, b"planes overlap"), ({"dl": dl + (nd - S,)}, b"frame_stride smaller than a frame"),
                            ({"sl": (sl[0], sl[1], sl[2], sl[3], sl[3])}, b"frame_stride smaller than a frame")):
        kw = {"sl": sl + (0,), "dl": dl + (0,), **change}
        fresh = guarded(nd + 64)
        rc = planar_call(plan, src.data_ptr(), fresh.data_ptr() + GUARD, sub, S, 2, kw["sl"], kw["dl"])
        assert rc == INVALID and message in nat.load().pb_last_error(), (change, rc, nat.load().pb_last_error())
        torch.cuda.synchronize()
        assert bool((fresh == SENTINEL).all()), change


@pytest.mark.parametrize("sub", planar_ref.SUBSAMPLINGS)
def test_three_frames_at_padded_strides_equal_three_single_launches(sub):
    case = LAYOUT_CASE
    plan = H.pb_plan_private(case, bilinear=False)
    _, h, w, *_ = case.src
    Hd, Wd = case.dst[1], case.dst[2]
    for S, dt in SAMPLES:
        sb, db = planar_ref.frame_samples(h, w, sub) * S, planar_ref.frame_samples(Hd, Wd, sub) * S
        for pad in (S, 48):
            ss, ds = sb + pad, db + pad
            src_host = np.random.default_rng(500 + S + pad).integers(0, 256, 3 * ss, dtype=np.uint8)  # (random bytes in the padding too)
            src = torch.from_numpy(src_host).cuda()
            buf = guarded(3 * ds)
            assert planar_call(plan, src.data_ptr(), buf.data_ptr() + GUARD, sub, S, 3, (0, 0, 0, 0, ss), (0, 0, 0, 0, ds)) == 0, nat.load().pb_last_error()
            torch.cuda.synchronize()
            assert guards_intact(buf)
            got = buf[GUARD:-GUARD].cpu().numpy()
            for f in range(3):
                single = run_planar(plan, src_host[f * ss : f * ss + sb].view(dt), sub)
                assert np.array_equal(got[f * ds : f * ds + db].view(dt), single), (sub, S, pad, f)
                assert bool((got[f * ds + db : (f + 1) * ds] == SENTINEL).all()), (sub, S, pad, f)  # the padding is intact
    # ... and through Plan.remap_planar: (N, frame_samples) in and out
    frames = np.stack([random_frame(h, w, sub, np.uint8, seed=510 + f) for f in range(3)])
    got = plan.remap_planar(torch.from_numpy(frames).cuda(), sub).cpu().numpy()
    assert got.shape == (3, planar_ref.frame_samples(Hd, Wd, sub)) and all(np.array_equal(got[f], run_planar(plan, frames[f], sub)) for f in range(3))


# ---- 5. consistency with pb_remap_px and pb_remap_nv12 ----------------------------------------------------------------------------------
def test_plane_0_is_pb_remap_px_of_the_plane_and_420_is_pb_remap_nv12_de_interleaved():
    case = tc.case_by_name("M_photo_stereographic")
    plan = _mid_plan(case)
    _, h, w, *_ = case.src
    Hd, Wd = case.dst[1], case.dst[2]
    for S, dt in SAMPLES:
        for sub in planar_ref.SUBSAMPLINGS:
            frame = random_frame(h, w, sub, dt, seed=600 + S)
            got = planar_ref.planes(run_planar(plan, frame, sub, fill=(0, 7, 9)), Hd, Wd, sub)
            p0 = plan.remap_px(torch.from_numpy(np.ascontiguousarray(frame[: h * w].reshape(h, w))).cuda()).cpu().numpy()
            assert np.array_equal(got[0], p0), (S, sub)
            if sub == "420":
                s0, s1, s2 = planar_ref.planes(frame, h, w, sub)
                semi = np.concatenate([s0, np.stack([s1, s2], axis=2).reshape(h // 2, w)], axis=0)
                src = torch.from_numpy(np.ascontiguousarray(semi).view(np.uint8)).cuda()
                buf = guarded(3 * Hd * Wd * S // 2)
                assert nv12_call(plan, src.data_ptr(), buf.data_ptr() + GUARD, S, fill=(0, 7, 9)) == 0
                torch.cuda.synchronize()
                out = buf[GUARD:-GUARD].cpu().numpy().view(dt).reshape(3 * Hd // 2, Wd)
                uv = out[Hd:].reshape(Hd // 2, Wd // 2, 2)
                assert np.array_equal(out[:Hd], got[0]) and np.array_equal(uv[..., 0], got[1]) and np.array_equal(uv[..., 1], got[2]), S


# ---- 6. plans the kernel does not serve -------------------------------------------------------------------------------------------------
def test_unsupported_plans_say_so_and_write_nothing():
    L = nat.load()
    single, double = tc.case_by_name("D_photo_rot"), tc.case_by_name("E_stitch_195_raw")
    faithful = H.pb_plan_private(single, bilinear=False)
    faithful.set_mode(nat.MODE_FAITHFUL)
    for what, case, plan in (("deferred", single, H.pb_plan_private(single, defer=True, bilinear=False)), ("faithful", single, faithful),
                             ("double-fisheye", double, H.pb_plan_private(double, bilinear=False))):
        _, h, w, *_ = case.src
        Hd, Wd = case.dst[1], case.dst[2]
        for sub in planar_ref.SUBSAMPLINGS:
            assert dims_ok(case, sub), what
            for S, dt in SAMPLES:
                assert L.pb_remap_planar_supported(plan.handle, SUBS[sub], S) == 0 and not plan.planar_supported(sub, S), (what, sub, S)
                assert not plan.px_supported(S) and not plan.nv12_supported(S)  # (exactly the plans pb_remap_px and pb_remap_nv12 refuse)
                frame = torch.from_numpy(random_frame(h, w, sub, dt, seed=700 + S)).cuda()
                buf = guarded(planar_ref.frame_samples(Hd, Wd, sub) * S)
                assert planar_call(plan, frame.data_ptr(), buf.data_ptr() + GUARD, sub, S) == UNSUPPORTED, (what, sub, S)
                assert b"pb_index_map_i32" in L.pb_last_error()
                torch.cuda.synchronize()
                assert bool((buf == SENTINEL).all()), (what, sub, S)
                with pytest.raises(nat.PbError):
                    plan.remap_planar(frame, sub)


# ---- 7. graph capture, streams and the host pipeline ------------------------------------------------------------------------------------
@pytest.mark.parametrize("sub", planar_ref.SUBSAMPLINGS)
@pytest.mark.parametrize("S,dt", SAMPLES)
def test_a_captured_launch_and_launches_on_three_streams_give_the_plain_bytes(S, dt, sub):
    case = tc.case_by_name("M_pano_thoby")
    plan = _mid_plan(case)
    _, h, w, *_ = case.src
    nd = planar_ref.frame_samples(case.dst[1], case.dst[2], sub) * S
    src = torch.from_numpy(random_frame(h, w, sub, dt, seed=800 + S)).cuda()
    want = plan.remap_planar(src, sub).view(torch.uint8)
    torch.cuda.synchronize()
    # never allocates or synchronises: the call captures into a graph, and a replay writes the frame again
    g_out = torch.zeros(nd, dtype=torch.uint8, device="cuda")
    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            assert planar_call(plan, src.data_ptr(), g_out.data_ptr(), sub, S, stream=int(side.cuda_stream)) == 0
    torch.cuda.current_stream().wait_stream(side)
    g_out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(g_out, want)
    # one launch on each of three streams
    streams = [torch.cuda.Stream() for _ in range(3)]
    outs = [torch.zeros(nd, dtype=torch.uint8, device="cuda") for _ in streams]
    torch.cuda.synchronize()
    for s, o in zip(streams, outs):
        assert planar_call(plan, src.data_ptr(), o.data_ptr(), sub, S, stream=int(s.cuda_stream)) == 0
    torch.cuda.synchronize()
    assert all(torch.equal(o, want) for o in outs)


@pytest.mark.parametrize("fmt", sorted(nat.PLANAR_FORMATS))
def test_remap_ndarray_and_remap_frames_take_every_pixel_format_name(fmt):
    case = tc.case_by_name("D_photo_rot")
    plan = H.pb_plan_private(case, bilinear=False)
    idx = SMALL[f"{case.name}/idx"]
    assert int((idx < 0).sum()) > 0  # (black pixels: the format's own black shows)
    _, h, w, *_ = case.src
    dt, sid, fill = nat.PLANAR_FORMATS[fmt]
    sub = {v: k for k, v in SUBS.items()}[sid]
    frames = [random_frame(h, w, sub, dt, seed=900 + k) for k in (0, 1, 0)]  # (the middle one differs)
    wants = [planar_ref.remap_frame(f, idx, h, w, sub, fill) for f in frames]
    one = _hostpipe.remap_ndarray(plan, frames[0], pixel_format=fmt)
    assert one.dtype == dt and np.array_equal(one, wants[0])
    outs = [np.array(o) for o in batch.remap_frames(plan, frames, pixel_format=fmt)]
    assert len(outs) == 3 and all(o.dtype == dt and np.array_equal(o, want) for o, want in zip(outs, wants))
    assert not np.array_equal(outs[1], outs[0])
    with pytest.raises(ValueError):
        list(batch.remap_frames(plan, [frames[0], frames[0][:-2]], pixel_format=fmt))
    with pytest.raises(ValueError):
        batch.remap_frames(plan, frames, pixel_format=fmt, rotations=np.eye(3)[None])
