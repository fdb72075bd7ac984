"""pb_remap_interp_pxf: bilinear and Catmull-Rom sampling of float16 and float32 frames through the tile kernel
pb_pxf_interp_kernel, against the written definition tests/pxf_ref.py on the float64 map tests/cubemap_cases.ref_stages gives.

A result g is compared with the definition's FLOAT64 value V (pxf_ref.remap_f64), so only the kernel's own narrowing is in the budget: with
a frame's samples in [L, U], EVERY sample must be within pxf_cases.tolerance(filter, L, U, S) of V - bilinear D / 512 + M 2^-20 + M u_out,
Catmull-Rom 15 D / 4096 + M 2^-18 + 1.5625 M u_out.  A pixel may be excused only if it is black in exactly one of the two results AND lies in
interp_cases.edge_band(case, final, 1/512); the excused pixels are counted and may not outnumber the band's, so a panorama source excuses
nothing (tests/test_px_interp_host.py caps the band for these very cases).  What needs no tolerance has none: a channel against the grey remap
of its plane, a half frame against the single one narrowed, a poisoned texel's reach, and how the frames reach the kernel - unaligned bases,
padded strides, batches, a captured graph, several streams."""

import functools

import numpy as np
import pytest
import torch

from photonbend_amd import _native as nat
from tests import cases as tc
from tests import cubemap_cases as cc
from tests import helpers as H
from tests import interp_cases as ic
from tests import pxf_cases as fc
from tests import pxf_ref
from tests.cases import Case, pano
from tests.test_hip_nv12 import GUARD, SENTINEL, guarded, guards_intact
from tests.test_hip_px_interp import BLACK_CASE, COV_RIM

pytestmark = pytest.mark.gpu

BIL, CR = "bilinear", "catmull-rom"
FILTERS = (BIL, CR)
UNSUPPORTED = -3
NAME = b"pb_remap_interp_pxf "
WORST = {}  # (filter, sample bytes, draw) -> the largest deviation from V seen in this run, as a fraction of T (printed; recorded in DESIGN 3.24)


def _plan(case, **kw):
    src, cmap = cc.pb_chain(case, image=np.zeros((case.src[1], case.src[2], 3), np.uint8))
    kw.setdefault("bilinear", True)
    return nat.Plan(cmap.dst_proj, cmap.rotations, src._proj("src"), **kw)


def _case(name):
    return COV_RIM if name == COV_RIM.name else ic.by_name(name)


@functools.lru_cache(maxsize=None)
def _geom(name):
    """The definition's float64 map of a case and its edge band, computed once and shared (read-only)."""
    case = _case(name)
    final = ic.final_map(case)
    band = ic.edge_band(case, final, fc.BAND)
    final.setflags(write=False)
    band.setflags(write=False)
    return final, band


def definition(case, image, filt):
    """The float64 V, (H, W, C)."""
    final, _ = _geom(case.name)
    return pxf_ref.remap_f64(ic.src_proj(case), image, filt, np.copy(final))


def fmt_of(image):
    return (1 if image.ndim == 2 else image.shape[2]), image.dtype.itemsize


def call(plan, src_ptr, dst_ptr, C, S, filt, n=1, ss=0, ds=0, stream=None):
    return nat.load().pb_remap_interp_pxf(plan.handle, src_ptr, dst_ptr, n, ss, ds, C, S, nat.TRACK_INTERP_IDS[filt], nat.current_stream() if stream is None else stream)


def run(plan, image, filt):
    """One packed launch of one frame -> the destination frame; the guards around the destination must survive."""
    C, S = fmt_of(image)
    Hd, Wd = plan.dst.height, plan.dst.width
    src = torch.from_numpy(np.ascontiguousarray(image).view(np.uint8).ravel()).cuda()
    buf = guarded(Hd * Wd * C * S)
    assert call(plan, src.data_ptr(), buf.data_ptr() + GUARD, C, S, filt) == 0, nat.load().pb_last_error()
    torch.cuda.synchronize()
    assert guards_intact(buf), "pb_remap_interp_pxf wrote outside the destination frame"
    out = buf[GUARD:-GUARD].cpu().numpy().view(image.dtype)
    return out.reshape((Hd, Wd) if image.ndim == 2 else (Hd, Wd, C))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint16 if a.dtype.itemsize == 2 else np.uint32)


def check(got, V, band, T, what, key):
    """The comparison rule of this file -> the number of excused pixels.  got: the kernel's frame; V: the definition's float64 (H, W, C)."""
    g3 = got[..., None] if got.ndim == 2 else got
    assert g3.shape == V.shape, (what, got.shape, V.shape)
    assert np.isfinite(g3).all(), f"{what}: a non-finite result on a finite frame"
    d = np.abs(g3.astype(np.float64) - V).max(axis=2)
    flip = (bits(g3) == 0).all(axis=2) != (V == 0).all(axis=2)  # black in exactly one of the two results
    ok = band & flip
    WORST[key] = max(WORST.get(key, 0.0), float(d[~ok].max(initial=0.0)) / T)
    off = (d > T) & ~ok
    where = np.argwhere(off)[:4].tolist()
    assert not off.any(), (f"{what}: {int(off.sum())} pixels beyond T = {T:.6g} of the definition (max {float(d[off].max()):.6g}; {int((off & flip).sum())} of them black in "
                           f"one result only, outside the edge band), first at {where}: got {[g3[y, x].tolist() for y, x in where]}, want {[V[y, x].tolist() for y, x in where]}")
    return int(((d > T) & ok).sum())


def against_the_definition(case, plan, forms, seed=0):
    """forms: (channels, sample bytes, draw) triples; both filters."""
    _, band = _geom(case.name)
    _, h, w, *_ = case.src
    for C, S, k in forms:
        assert plan.float_supported(C, S, BIL) and plan.float_supported(C, S, CR), (case.name, C, S)
        image, (L, U) = fc.draw(h, w, C, S, k, seed + 16 * C + S + 64 * k)
        for filt in FILTERS:
            T = fc.tolerance(filt, L, U, S)
            excused = check(run(plan, image, filt), definition(case, image, filt), band, T, f"{case.name} {filt} {C} x float{8 * S} draw {fc.DRAWS[S][k][0]}", (filt, S, k))
            assert excused <= int(band.sum()), f"{case.name} {filt} ({C}, {S}): {excused} pixels excused, the edge band holds {int(band.sum())}"
            if case.src[0] == "pano":
                assert excused == 0
            if case.name in fc.PINNED_BANDS:
                assert int(band.sum()) == fc.PINNED_BANDS[case.name]
            print(f"{case.name} {filt} ({C}, {S}) draw {fc.DRAWS[S][k][0]}: T = {T:.6g}, largest deviation so far {WORST[(filt, S, k)]:.4f} T, excused {excused} of {int(band.sum())} band px")


# ---- 1. parity ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", fc.CASES, ids=lambda c: c.name)
def test_every_case_on_rgba_half_and_grey_single_against_the_definition(case):
    against_the_definition(case, _plan(case), [(4, 2, 0), (1, 4, 0)])


@pytest.mark.parametrize("C,S", fc.FORMATS, ids=lambda v: str(v))
@pytest.mark.parametrize("name", fc.ALL_FORMAT_CASES)
def test_every_format_and_every_draw_against_the_definition(name, C, S):
    case = ic.by_name(name)
    against_the_definition(case, _plan(case), [(C, S, k) for k in range(3)], seed=100)


# ---- 2. what the kernel branches on is all there ------------------------------------------------------------------------------------------
COVERAGE_FORMATS = ((4, 2), (1, 4), (3, 4), (4, 4))  # the 12- and 16-byte paths meet every tile class


def test_the_rim_case_meets_every_tile_class_the_kernel_has_a_path_for():
    keys = ("window", "direct", "table", "black", "td3", "fix_tiles", "fix_pixels")
    rim, black = _plan(COV_RIM).bilinear_tile_mix(), _plan(ic.by_name(BLACK_CASE)).bilinear_tile_mix()
    for name, mix in ((COV_RIM.name, rim), (BLACK_CASE, black)):
        print(f"{name:26s} " + " ".join(f"{k} {mix[k]}" for k in keys))
    model = rim["window"] + rim["direct"]
    assert model - rim["td3"] > 0 and rim["td3"] > 0 and rim["table"] > 0, rim
    assert rim["fix_tiles"] > 0 and rim["fix_pixels"] > 0, rim
    assert black["black"] > 0 and black["window"] + black["direct"] > 0, black


@pytest.mark.parametrize("name", (COV_RIM.name, BLACK_CASE))
def test_the_coverage_cases_against_the_definition(name):
    case = _case(name)
    against_the_definition(case, _plan(case), [(C, S, 1) for C, S in COVERAGE_FORMATS], seed=40)


# ---- 3. exact: no tolerance ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("sweep5", BLACK_CASE, COV_RIM.name))
def test_a_channel_is_the_grey_remap_of_its_plane_and_a_half_frame_is_the_single_one_narrowed(name):
    case = _case(name)
    plan = _plan(case)
    _, h, w, *_ = case.src
    half, _ = fc.draw(h, w, 4, 2, 2, 300)
    frames = {2: half, 4: half.astype(np.float32)}  # the same values widened: exact
    for filt in FILTERS:
        full = {}
        for S, image in frames.items():
            grey = [run(plan, np.ascontiguousarray(image[:, :, k]), filt) for k in range(4)]
            assert any(g.any() for g in grey)
            for C in (2, 3, 4):
                got = run(plan, np.ascontiguousarray(image[:, :, :C]), filt)
                for k in range(C):
                    assert np.array_equal(bits(got[:, :, k]), bits(grey[k])), (name, filt, C, S, k)
                full[S] = got
        # float32 arithmetic and ONE narrowing: the half result is the single result rounded to nearest even
        assert np.array_equal(bits(full[2]), bits(full[4].astype(np.float16))), (name, filt)


# ---- 4. NaN containment -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", (fc.POISON_PANO, fc.POISON_CAM))
def test_a_poisoned_texel_in_view_spoils_only_the_pixels_whose_footprint_can_hold_it(name):
    case = ic.by_name(name)
    plan = _plan(case)
    final, _ = _geom(name)
    src = ic.src_proj(case)
    texel = fc.POISON_TEXEL if name == fc.POISON_PANO else fc.centre_texel(src, final)
    mask = fc.poison_mask(src, final, texel)
    assert 0 < int(mask.sum()) <= mask.size // 10
    _, h, w, *_ = case.src
    for C, S in ((3, 4), (4, 2)):
        clean, _ = fc.draw(h, w, C, S, 0, 600 + C)
        for filt in FILTERS:
            want = run(plan, clean, filt)
            for poison in (np.nan, np.inf):
                dirty = clean.copy()
                dirty[texel[0], texel[1], :] = poison
                got = run(plan, dirty, filt)
                same = (bits(got) == bits(want)).all(axis=2)
                assert same[~mask].all(), (name, C, S, filt, poison, int((~same & ~mask).sum()), np.argwhere(~same & ~mask)[:4].tolist())
                assert not same[mask].all(), (name, C, S, filt, poison, "the poisoned texel is not in view")


def test_a_nan_at_texel_0_0_reaches_no_dead_pixel():
    """A dead pixel reads pixel 0 and is zeroed by a select: a multiplication by zero would leave the NaN."""
    case = ic.by_name(BLACK_CASE)
    plan = _plan(case)
    final, band = _geom(case.name)
    _, _, live = pxf_ref.positions(ic.src_proj(case), np.copy(final))
    dead = ~live & ~band
    assert dead.any()
    _, h, w, *_ = case.src
    for C, S in ((3, 4), (4, 2), (1, 4)):
        image, _ = fc.draw(h, w, C, S, 0, 650 + C, squeeze=False)
        image[0, 0, :] = np.nan
        for filt in FILTERS:
            got = run(plan, image, filt)
            assert not bits(got)[dead].any(), (C, S, filt, int((bits(got)[dead] != 0).sum()))


# ---- 5. layouts -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("C,S", fc.FORMATS, ids=lambda v: str(v))
def test_unaligned_bases_and_padded_strides_give_the_bytes_of_the_aligned_single_launches(C, S, filt):
    """Frame bases at odd multiples of A = min(4, B & -B) from 256-byte alignment; three frames at strides padded by A and by 48 bytes, between
    random bytes (the source's padding) and sentinels (the destination's).  A destination of odd width: rows of 2- and 6-byte pixels start off
    dword alignment, and rows of every size off 16-byte alignment."""
    case = ic.ODD_DST
    plan = _plan(case)
    _, h, w, *_ = case.src
    B = C * S
    A = min(4, B & -B)
    image, _ = fc.draw(h, w, C, S, 1, 400 + B, squeeze=False)
    want = run(plan, image, filt)
    sb, db = image.nbytes, want.nbytes
    for off in (A, 3 * A):
        src = torch.zeros(sb + 512, dtype=torch.uint8, device="cuda")
        s_off = (-src.data_ptr()) % 256 + off
        src[s_off : s_off + sb] = torch.from_numpy(image.view(np.uint8).ravel()).cuda()
        buf = guarded(db + 512)
        d_off = GUARD + (-(buf.data_ptr() + GUARD)) % 256 + off
        assert call(plan, src.data_ptr() + s_off, buf.data_ptr() + d_off, C, S, filt) == 0, nat.load().pb_last_error()
        torch.cuda.synchronize()
        host = buf.cpu().numpy()
        assert np.array_equal(host[d_off : d_off + db], want.view(np.uint8).ravel()), off
        assert bool((host[:d_off] == SENTINEL).all()) and bool((host[d_off + db :] == SENTINEL).all()), off
    for pad in (A, 48):
        ss, ds = sb + pad, db + pad
        frames = [fc.draw(h, w, C, S, k, 500 + B + pad + k, squeeze=False)[0] for k in range(3)]
        src_host = np.random.default_rng(500 + B + pad).integers(0, 256, 3 * ss, dtype=np.uint8)  # (random bytes in the padding)
        for f in range(3):
            src_host[f * ss : f * ss + sb] = frames[f].view(np.uint8).ravel()
        buf = guarded(3 * ds)
        src = torch.from_numpy(src_host).cuda()
        assert call(plan, src.data_ptr(), buf.data_ptr() + GUARD, C, S, filt, 3, ss, ds) == 0, nat.load().pb_last_error()
        torch.cuda.synchronize()
        assert guards_intact(buf)
        got = buf[GUARD:-GUARD].cpu().numpy()
        for f in range(3):
            single = run(plan, frames[f], filt)
            assert np.array_equal(got[f * ds : f * ds + db], single.view(np.uint8).ravel()), (pad, f)
            assert bool((got[f * ds + db : (f + 1) * ds] == SENTINEL).all()), (pad, f)


# ---- 6. a captured graph, three streams -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("filt", FILTERS)
def test_a_captured_launch_and_launches_on_three_streams_give_the_plain_bytes(filt):
    case = ic.by_name("sweep10")
    plan = _plan(case)
    _, h, w, *_ = case.src
    for C, S in ((4, 2), (1, 4), (3, 4)):
        image, _ = fc.draw(h, w, C, S, 0, 800 + C * S)
        src = torch.from_numpy(image.view(np.uint8).ravel()).cuda()
        nd = case.dst[1] * case.dst[2] * C * S

        def go(dst, stream=None):
            return call(plan, src.data_ptr(), dst.data_ptr(), C, S, filt, stream=stream)

        want = torch.zeros(nd, dtype=torch.uint8, device="cuda")
        assert go(want) == 0
        torch.cuda.synchronize()
        assert bool(want.any())
        # never allocates or synchronises: the call captures into a graph, and a replay writes the frame again
        g_out = torch.zeros(nd, dtype=torch.uint8, device="cuda")
        graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            with torch.cuda.graph(graph, stream=side):
                assert go(g_out, int(side.cuda_stream)) == 0
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
            assert go(o, int(s.cuda_stream)) == 0
        torch.cuda.synchronize()
        assert all(torch.equal(o, want) for o in outs)


# ---- 7. plans the kernel does not serve ---------------------------------------------------------------------------------------------------------
def test_unsupported_plans_say_so_and_write_nothing():
    L = nat.load()
    single, double = tc.case_by_name("D_photo_rot"), tc.case_by_name("E_stitch_195_raw")
    cube = Case("cube_source", pano(32, 64), cc.cube(16))
    tiny = ic.by_name(fc.REFUSED)
    faithful = H.pb_plan_private(single, bilinear=True)
    faithful.set_mode(nat.MODE_FAITHFUL)
    plans = (("deferred", single, H.pb_plan_private(single, defer=True), b"prepared plans"), ("faithful", single, faithful, b"prepared plans"),
             ("double-fisheye", double, H.pb_plan_private(double, bilinear=True), b"prepared plans"), ("cube", cube, _plan(cube), b"cube source"),
             ("bilinear=False", single, H.pb_plan_private(single, bilinear=False), b"pb_plan_prepare(plan, PB_PLAN_BILINEAR)"),
             ("no tables", tiny, _plan(tiny), b"tables cannot exist"))
    for what, case, plan, message in plans:
        _, h, w, *_ = case.src
        Hd, Wd = case.dst[1], case.dst[2]
        for C, S in fc.FORMATS:
            image, _ = fc.draw(h, w, C, S, 0, 700 + C * S)
            src = torch.from_numpy(image.view(np.uint8).ravel()).cuda()
            for filt in FILTERS:
                assert L.pb_remap_interp_pxf_supported(plan.handle, C, S, nat.TRACK_INTERP_IDS[filt]) == 0 and not plan.float_supported(C, S, filt), (what, C, S, filt)
                buf = guarded(Hd * Wd * C * S)
                rc = call(plan, src.data_ptr(), buf.data_ptr() + GUARD, C, S, filt)
                assert rc == UNSUPPORTED and message in L.pb_last_error() and L.pb_last_error().startswith(NAME), (what, C, S, filt, rc, L.pb_last_error())
                if what == "no tables":  # ("call pb_plan_prepare" is a false answer for a plan that WAS prepared)
                    assert b"pb_plan_prepare" not in L.pb_last_error()
                torch.cuda.synchronize()
                assert bool((buf == SENTINEL).all()), (what, C, S, filt)
    # the integer call serves the two-pixel source from the float64 chain, and the nearest call moves float pixels of up to 8 bytes
    assert plans[5][2].px_interp_route(4, 1, BIL) == "float64" and plans[5][2].px_supported(8)
    # Plan.remap_float builds the tables of a plan made without them; what it cannot serve then is a PbError, never a fallback
    for what, case, plan, _ in plans[:4]:
        with pytest.raises(nat.PbError):
            plan.remap_float(torch.zeros((case.src[1], case.src[2], 4), dtype=torch.float16, device="cuda"))


# ---- 8. the Python method -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("filt", FILTERS)
def test_plan_remap_float_takes_the_four_shapes_and_both_dtypes(filt):
    case = ic.by_name("sweep5")
    plan = _plan(case, bilinear=False)  # (the tables are built on first use)
    _, h, w, *_ = case.src
    Hd, Wd = case.dst[1], case.dst[2]
    for S in (2, 4):
        frames = np.stack([fc.draw(h, w, 4, S, f, 900 + S + f)[0] for f in range(2)])
        for src in (frames[0, :, :, 0], frames[0], frames[:, :, :, 1], frames, frames[:, :, :, :3]):
            src = np.ascontiguousarray(src)
            got = plan.remap_float(torch.from_numpy(src).cuda(), interpolation=filt)
            assert isinstance(got, torch.Tensor) and got.dtype == torch.from_numpy(src).dtype
            batched = src.shape[0] == 2
            assert tuple(got.shape) == ((2,) if batched else ()) + (Hd, Wd) + src.shape[(3 if batched else 2):]
            one = [run(plan, f, filt) for f in (src if batched else [src])]
            assert np.array_equal(bits(got.cpu().numpy()), bits(np.stack(one) if batched else one[0])), (filt, S, src.shape)
            out = torch.empty_like(got)
            assert plan.remap_float(torch.from_numpy(src).cuda(), out=out, interpolation=filt) is out
            assert np.array_equal(bits(out.cpu().numpy()), bits(got.cpu().numpy()))
        assert got.cpu().numpy().any()
    if filt == BIL:  # the default
        src = torch.from_numpy(np.ascontiguousarray(frames[0])).cuda()
        assert torch.equal(plan.remap_float(src), plan.remap_float(src, interpolation=BIL))
    with pytest.raises(ValueError):
        plan.remap_float(torch.from_numpy(frames).cuda(), interpolation="nearest")
    with pytest.raises(nat.PbError):
        plan.remap_float(torch.from_numpy(frames.astype(np.float64)).cuda(), interpolation=filt)
    with pytest.raises(nat.PbError):
        plan.remap_float(torch.from_numpy(frames).cuda().to(torch.bfloat16), interpolation=filt)


def test_the_largest_deviations_seen():
    """Not a check of its own: prints what the tests above saw, as fractions of T, for DESIGN 3.24 (run after them, in file order)."""
    print("largest deviation from the definition per (filter, sample bytes, draw), as a fraction of T:",
          {(f, S, fc.DRAWS[S][k][0]): round(v, 4) for (f, S, k), v in sorted(WORST.items())})
    for key, worst in WORST.items():
        assert worst <= 1.0, key
