"""pb_remap_interp_px: bilinear and Catmull-Rom sampling of grey, RGBA and 16-bit frames through the tile kernel
pb_px_interp_kernel, against the written definitions oracle.reference_path.remap_bilinear and tests/catmull_rom_ref.remap on the float64 map
tests/cubemap_cases.ref_stages gives.

Frames are independent random samples in [0, R]: a coordinate error of e px moves a sample by up to e x R.  The tile kernels' coordinates are
certified to 1/1024 px per axis, so EVERY sample must be within px_interp_cases.tolerance(filter, R) of the definition - bilinear
1 + R // 512, Catmull-Rom 1 + floor(15 R / 4096 + R 2^-18).  A pixel may be excused only if it is black in exactly one of the two results AND
lies in interp_cases.edge_band(case, final, 1/512); the excused pixels are counted and may not outnumber the band's, so a panorama source
excuses nothing (tests/test_px_interp_host.py caps the band).  How the frames reach the kernel - unaligned bases, padded strides, batches, a
captured graph, several streams - never moves a byte."""

import functools

import numpy as np
import pytest
import torch

from oracle import reference_path as orc
from photonbend_amd import _native as nat
from tests import cases as tc
from tests import catmull_rom_ref as crr
from tests import cubemap_cases as cc
from tests import helpers as H
from tests import interp_cases as ic
from tests import px_interp_cases as pc
from tests.cases import Case, cam, inscribed, pano
from tests.test_hip_nv12 import GUARD, SENTINEL, guarded, guards_intact

pytestmark = pytest.mark.gpu

BIL, CR = "bilinear", "catmull-rom"
FILTERS = (BIL, CR)
UNSUPPORTED = -3
# a 360-degree equisolid rim under a rotation (tests/test_hip_video_bilinear.py): window, table and TD3 entries and hundreds of fix pixels
COV_RIM = Case("cov_rim", cam(512, 512, "equisolid", 360, inscribed(512)), cam(512, 512, "equidistant", 360, inscribed(512)), [(30, 45, 10)])
WORST = {}  # (filter, sample bytes, R) -> the largest deviation from the definition seen in this run (printed; recorded in DESIGN 3.23)


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
    band = ic.edge_band(case, final, pc.BAND)
    final.setflags(write=False)
    band.setflags(write=False)
    return final, band


def definition(case, image, filt):
    final, _ = _geom(case.name)
    with np.errstate(all="ignore"):
        fn = orc.remap_bilinear if filt == BIL else crr.remap
        return fn(None, ic.src_proj(case), image, cmap=np.copy(final))


def draw(h, w, C, S, R, seed, squeeze=True):
    """An (h, w, C) frame - (h, w) for one channel - of independent random samples in [0, R]."""
    a = np.random.default_rng(seed).integers(0, R + 1, size=(h, w, C), dtype=np.uint8 if S == 1 else np.uint16)
    return a[:, :, 0].copy() if C == 1 and squeeze else a


def fmt_of(image):
    return (1 if image.ndim == 2 else image.shape[2]), image.dtype.itemsize


def call(plan, src_ptr, dst_ptr, C, S, filt, n=1, ss=0, ds=0, stream=None):
    return nat.load().pb_remap_interp_px(plan.handle, src_ptr, dst_ptr, n, ss, ds, C, S, nat.TRACK_INTERP_IDS[filt], nat.current_stream() if stream is None else stream)


def run(plan, image, filt):
    """One packed launch of one frame -> the destination frame; the guards around the destination must survive."""
    C, S = fmt_of(image)
    Hd, Wd = plan.dst.height, plan.dst.width
    src = torch.from_numpy(np.ascontiguousarray(image).view(np.uint8).ravel()).cuda()
    buf = guarded(Hd * Wd * C * S)
    assert call(plan, src.data_ptr(), buf.data_ptr() + GUARD, C, S, filt) == 0, nat.load().pb_last_error()
    torch.cuda.synchronize()
    assert guards_intact(buf), "pb_remap_interp_px wrote outside the destination frame"
    out = buf[GUARD:-GUARD].cpu().numpy().view(image.dtype)
    return out.reshape((Hd, Wd) if image.ndim == 2 else (Hd, Wd, C))


def check(got, want, band, T, what, key):
    """The comparison rule of this file -> the number of excused pixels."""
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, got.dtype, want.shape, want.dtype)
    g3, w3 = (got[..., None], want[..., None]) if got.ndim == 2 else (got, want)
    d = np.abs(g3.astype(np.int64) - w3.astype(np.int64)).max(axis=2)
    flip = (g3 == 0).all(axis=2) != (w3 == 0).all(axis=2)  # black in exactly one of the two results
    ok = band & flip
    WORST[key] = max(WORST.get(key, 0), int(d[~ok].max(initial=0)))
    off = (d > T) & ~ok
    where = np.argwhere(off)[:4].tolist()
    assert not off.any(), (f"{what}: {int(off.sum())} pixels beyond T = {T} of the definition (max {int(d[off].max())}; {int((off & flip).sum())} of them black in one "
                           f"result only, outside the edge band), first at {where}: got {[g3[y, x].tolist() for y, x in where]}, want {[w3[y, x].tolist() for y, x in where]}")
    return int(((d > T) & ok).sum())


def against_the_definition(case, plan, forms, seed=0):
    """forms: (channels, sample bytes, R) triples; both filters."""
    _, band = _geom(case.name)
    _, h, w, *_ = case.src
    for C, S, R in forms:
        assert plan.px_interp_supported(C, S, BIL) and plan.px_interp_supported(C, S, CR), (case.name, C, S)
        image = draw(h, w, C, S, R, seed + 16 * C + S)
        for filt in FILTERS:
            T = pc.tolerance(filt, R)
            excused = check(run(plan, image, filt), definition(case, image, filt), band, T, f"{case.name} {filt} {C}x{8 * S} bit R={R}", (filt, S, R))
            assert excused <= int(band.sum()), f"{case.name} {filt} ({C}, {S}): {excused} pixels excused, the edge band holds {int(band.sum())}"
            if case.src[0] == "pano":
                assert excused == 0
            if case.name in pc.PINNED_BANDS:
                assert int(band.sum()) == pc.PINNED_BANDS[case.name]
            print(f"{case.name} {filt} ({C}, {S}) R = {R}: T = {T}, largest deviation so far {WORST[(filt, S, R)]}, excused {excused} of {int(band.sum())} band px")


# ---- 1. parity ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", pc.CASES, ids=lambda c: c.name)
def test_every_case_on_rgba8_and_grey16_against_the_definitions(case):
    against_the_definition(case, _plan(case), [(4, 1, 255), (1, 2, 65535)])


@pytest.mark.parametrize("C,S", pc.FORMATS, ids=lambda v: str(v))
@pytest.mark.parametrize("name", pc.ALL_FORMAT_CASES)
def test_every_format_against_the_definitions(name, C, S):
    """16-bit samples both at full range and at R = 1023 (10-bit samples stored low)."""
    case = ic.by_name(name)
    against_the_definition(case, _plan(case), [(C, S, 255)] if S == 1 else [(C, S, 65535), (C, S, 1023)], seed=100)


# ---- 2. what the kernel branches on is all there ------------------------------------------------------------------------------------------
BLACK_CASE = "mag_pano_from_cam"  # a camera source inside a panorama: the rim case has no all-black tile (its corners are invalid pixels of sampled tiles)


def test_the_rim_case_meets_every_tile_class_the_kernel_has_a_path_for():
    """On the one plan of the 360-degree equisolid rim under a rotation: model tiles plain and TD3, table tiles, modelled tiles with fix
    pixels - the classes that take different code.  That plan has no all-black tile, so the BLACK path is met on a case of its own.  Both plans
    are run against the definitions below, a 6-byte format among theirs.  A missing class is a failure."""
    keys = ("window", "direct", "table", "black", "td3", "fix_tiles", "fix_pixels")
    rim, black = _plan(COV_RIM).bilinear_tile_mix(), _plan(ic.by_name(BLACK_CASE)).bilinear_tile_mix()
    for name, mix in ((COV_RIM.name, rim), (BLACK_CASE, black)):
        print(f"{name:26s} " + " ".join(f"{k} {mix[k]}" for k in keys))
    model = rim["window"] + rim["direct"]
    assert model - rim["td3"] > 0 and rim["td3"] > 0 and rim["table"] > 0, rim
    assert rim["fix_tiles"] > 0 and rim["fix_pixels"] > 0, rim
    assert black["black"] > 0 and black["window"] + black["direct"] > 0, black


@pytest.mark.parametrize("name", (COV_RIM.name, BLACK_CASE))
def test_the_coverage_cases_against_the_definitions(name):
    case = _case(name)
    against_the_definition(case, _plan(case), [(4, 1, 255), (1, 2, 65535), (3, 2, 1023)], seed=40)


# ---- 2b. which route a plan takes -------------------------------------------------------------------------------------------------------------
def test_ordinary_plans_take_the_tile_kernel_and_a_two_pixel_source_the_float64_chain():
    """pb_plan_px_interp_route: every case but the one whose coordinate tables cannot exist (a source of two pixels) runs pb_px_interp_kernel;
    three uint8 channels are the RGB8 call's; a plan the call refuses launches nothing."""
    L = nat.load()
    for case in [c for c in pc.CASES if not c.name.startswith("sweep") or c.name in pc.ALL_FORMAT_CASES]:  # (every fixed case, two of the sweep)
        plan = _plan(case)
        want = "float64" if case.src[1] * case.src[2] < 3 else "tiles"
        for C, S in pc.FORMATS:
            for filt in FILTERS:
                assert plan.px_interp_route(C, S, filt) == want, (case.name, C, S, filt)
                assert L.pb_plan_px_interp_route(plan.handle, C, S, nat.TRACK_INTERP_IDS[filt]) == {"tiles": 1, "float64": 2}[want]
        assert plan.px_interp_route(3, 1, BIL) == "rgb8"
    assert [c.name for c in pc.CASES if c.src[1] * c.src[2] < 3] == ["tiny_pano_1x2"]
    assert _plan(ic.by_name("sweep5"), bilinear=False).px_interp_route(4, 1, BIL) == "none"
    with pytest.raises(nat.PbError):
        _plan(ic.by_name("sweep5")).px_interp_route(5, 1, BIL)


@pytest.mark.parametrize("filt", FILTERS)
def test_the_float64_route_takes_batches_and_padded_strides_and_is_the_materialised_map_call(filt):
    """A source of two pixels: three frames at strides padded by A and by 48 bytes between random bytes and sentinels give the bytes of the
    single launches, and a single launch gives pb_sample_map_*_px's bytes on the plan's own map - the definition on the device."""
    case = ic.by_name("tiny_pano_1x2")
    plan = _plan(case)
    _, h, w, *_ = case.src
    Hd, Wd = case.dst[1], case.dst[2]
    for C, S in ((4, 1), (1, 2), (3, 2)):
        assert plan.px_interp_route(C, S, filt) == "float64"
        B, A = C * S, nat.px_align(C * S)
        image = draw(h, w, C, S, 255 if S == 1 else 65535, 950 + B, squeeze=False)
        want = run(plan, image, filt)
        sb, db = image.nbytes, want.nbytes
        cmap = nat.coordmap(plan.dst)
        ref = nat.sample_map_interp(filt, plan.src, cmap, torch.from_numpy(image).cuda(), C, image.dtype)
        assert np.array_equal(nat.to_host(ref).reshape(want.shape), want) and want.any(), (C, S)
        for pad in (A, 48):
            ss, ds = sb + pad, db + pad
            src_host = np.random.default_rng(960 + B + pad).integers(0, 256, 3 * ss + 64, dtype=np.uint8)
            buf = guarded(3 * ds)
            src = torch.from_numpy(src_host).cuda()
            assert call(plan, src.data_ptr(), buf.data_ptr() + GUARD, C, S, filt, 3, ss, ds) == 0, nat.load().pb_last_error()
            torch.cuda.synchronize()
            assert guards_intact(buf)
            got = buf[GUARD:-GUARD].cpu().numpy()
            for f in range(3):
                single = run(plan, src_host[f * ss : f * ss + sb].view(image.dtype).reshape(image.shape), filt)
                assert np.array_equal(got[f * ds : f * ds + db], single.view(np.uint8).ravel()), (C, S, pad, f)
                assert bool((got[f * ds + db : (f + 1) * ds] == SENTINEL).all()), (C, S, pad, f)


# ---- 3. exact: no tolerance ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("sweep5", "mag_pano_from_cam", COV_RIM.name))
def test_a_channel_is_the_grey_remap_of_its_plane_and_rgb8_is_the_rgb8_call(name):
    case = _case(name)
    plan = _plan(case)
    _, h, w, *_ = case.src
    for filt in FILTERS:
        for S, R in ((1, 255), (2, 65535)):
            image = draw(h, w, 4, S, R, 300 + S)
            grey = [run(plan, np.ascontiguousarray(image[:, :, k]), filt) for k in range(4)]
            assert any(g.any() for g in grey)
            for C in (1, 2, 3, 4):
                if (C, S) == (3, 1):
                    continue
                got = run(plan, np.ascontiguousarray(image[:, :, :C]), filt)
                for k in range(C):
                    assert np.array_equal(got[:, :, k], grey[k]), (name, filt, C, S, k)
        # three uint8 channels: the RGB8 tile kernels, through this call
        rgb = draw(h, w, 3, 1, 255, 310)
        want = plan.remap(torch.from_numpy(rgb).cuda(), interpolation=filt).cpu().numpy()
        assert np.array_equal(run(plan, rgb, filt), want) and want.any(), (name, filt)
        assert plan.px_interp_supported(3, 1, filt)


# ---- 4. layouts -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("C,S", pc.FORMATS, ids=lambda v: str(v))
def test_unaligned_bases_and_padded_strides_give_the_bytes_of_the_aligned_single_launches(C, S, filt):
    """Frame bases at odd multiples of A = min(4, B & -B) from 256-byte alignment; three frames at strides padded by A and by 48 bytes, between
    random bytes (source) and sentinels (destination).  A destination of odd width: rows of 1-, 2- and 6-byte pixels start off dword alignment."""
    case = ic.ODD_DST
    plan = _plan(case)
    _, h, w, *_ = case.src
    Hd, Wd = case.dst[1], case.dst[2]
    B = C * S
    A = nat.px_align(B)
    R = 255 if S == 1 else 65535
    image = draw(h, w, C, S, R, 400 + B, squeeze=False)
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
        src_host = np.random.default_rng(500 + B + pad).integers(0, 256, 3 * ss, dtype=np.uint8)  # (random bytes in the padding too)
        buf = guarded(3 * ds)
        src = torch.from_numpy(src_host).cuda()
        assert call(plan, src.data_ptr(), buf.data_ptr() + GUARD, C, S, filt, 3, ss, ds) == 0, nat.load().pb_last_error()
        torch.cuda.synchronize()
        assert guards_intact(buf)
        got = buf[GUARD:-GUARD].cpu().numpy()
        for f in range(3):
            single = run(plan, src_host[f * ss : f * ss + sb].view(image.dtype).reshape(image.shape), filt)
            assert np.array_equal(got[f * ds : f * ds + db], single.view(np.uint8).ravel()), (pad, f)
            assert bool((got[f * ds + db : (f + 1) * ds] == SENTINEL).all()), (pad, f)


# ---- 5. a captured graph, three streams -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("filt", FILTERS)
def test_a_captured_launch_and_launches_on_three_streams_give_the_plain_bytes(filt):
    case = ic.by_name("sweep10")
    plan = _plan(case)
    _, h, w, *_ = case.src
    for C, S in ((4, 1), (1, 2), (3, 2)):
        image = draw(h, w, C, S, 255 if S == 1 else 65535, 800 + C * S)
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


# ---- 6. plans the kernel does not serve ---------------------------------------------------------------------------------------------------------
def test_unsupported_plans_say_so_and_write_nothing():
    L = nat.load()
    single, double = tc.case_by_name("D_photo_rot"), tc.case_by_name("E_stitch_195_raw")
    cube = Case("cube_source", pano(32, 64), cc.cube(16))
    faithful = H.pb_plan_private(single, bilinear=True)
    faithful.set_mode(nat.MODE_FAITHFUL)
    plans = (("deferred", single, H.pb_plan_private(single, defer=True), b"prepared plans"), ("faithful", single, faithful, b"prepared plans"),
             ("double-fisheye", double, H.pb_plan_private(double, bilinear=True), b"prepared plans"), ("cube", cube, _plan(cube), b"pb_sample_map_"),
             ("bilinear=False", single, H.pb_plan_private(single, bilinear=False), b"pb_plan_prepare(plan, PB_PLAN_BILINEAR)"))
    for what, case, plan, message in plans:
        _, h, w, *_ = case.src
        Hd, Wd = case.dst[1], case.dst[2]
        for C, S in pc.FORMATS:
            image = draw(h, w, C, S, 255 if S == 1 else 65535, 700 + C * S)
            src = torch.from_numpy(image.view(np.uint8).ravel()).cuda()
            for filt in FILTERS:
                assert L.pb_remap_interp_px_supported(plan.handle, C, S, nat.TRACK_INTERP_IDS[filt]) == 0 and not plan.px_interp_supported(C, S, filt), (what, C, S, filt)
                buf = guarded(Hd * Wd * C * S)
                rc = call(plan, src.data_ptr(), buf.data_ptr() + GUARD, C, S, filt)
                assert rc == UNSUPPORTED and message in L.pb_last_error() and L.pb_last_error().startswith(b"pb_remap_interp_px "), (what, C, S, filt, rc, L.pb_last_error())
                torch.cuda.synchronize()
                assert bool((buf == SENTINEL).all()), (what, C, S, filt)
        if what == "cube":
            assert b"cube source" in L.pb_last_error()
    # the nearest call serves the plans this call refuses for its tables' sake
    assert plans[3][2].px_supported(4) and plans[4][2].px_supported(4)
    # Plan.remap_px builds the tables of a plan made without them, as Plan.remap does; what it cannot serve then is a PbError, never a fallback
    for what, case, plan, _ in plans[:4]:
        with pytest.raises(nat.PbError):
            plan.remap_px(torch.zeros((case.src[1], case.src[2], 4), dtype=torch.uint8, device="cuda"), interpolation=BIL)


# ---- 7. the Python method -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("filt", FILTERS)
def test_plan_remap_px_with_the_keyword_takes_the_four_shapes_and_both_dtypes(filt):
    case = ic.by_name("sweep5")
    plan = _plan(case, bilinear=False)  # (the tables are built on first use)
    _, h, w, *_ = case.src
    Hd, Wd = case.dst[1], case.dst[2]
    for S, R in ((1, 255), (2, 65535)):
        frames = np.stack([draw(h, w, 4, S, R, 900 + S + f) for f in range(2)])
        for src in (frames[0, :, :, 0], frames[0], frames[:, :, :, 1], frames, frames[:, :, :, :2]):
            src = np.ascontiguousarray(src)
            got = plan.remap_px(torch.from_numpy(src).cuda(), interpolation=filt)
            assert isinstance(got, torch.Tensor) and got.dtype == torch.from_numpy(src).dtype
            batched = src.shape[0] == 2
            assert tuple(got.shape) == ((2,) if batched else ()) + (Hd, Wd) + src.shape[(3 if batched else 2):]
            one = [run(plan, f, filt) for f in (src if batched else [src])]
            assert np.array_equal(got.cpu().numpy(), np.stack(one) if batched else one[0]), (filt, S, src.shape)
            out = torch.empty_like(got)
            assert plan.remap_px(torch.from_numpy(src).cuda(), out=out, interpolation=filt) is out
            assert np.array_equal(out.cpu().numpy(), got.cpu().numpy())
        want = np.stack([run(plan, frames[f], filt) for f in range(2)])
        assert np.array_equal(plan.remap_px(torch.from_numpy(frames).cuda(), interpolation=filt).cpu().numpy(), want) and want.any()
        assert not np.array_equal(plan.remap_px(torch.from_numpy(frames).cuda()).cpu().numpy(), want)  # (the default samples nearest)
    with pytest.raises(ValueError):
        plan.remap_px(torch.from_numpy(frames).cuda(), interpolation="cubic")
    with pytest.raises(nat.PbError):
        plan.remap_px(torch.from_numpy(frames.astype(np.float32)).cuda(), interpolation=filt)


def test_the_largest_deviations_seen():
    """Not a check of its own: prints what the tests above saw, for DESIGN 3.23 (run after them, in file order)."""
    print("largest deviation from the definition per (filter, sample bytes, R):", {k: (v, pc.tolerance(k[0], k[2])) for k, v in sorted(WORST.items())})
    for (filt, _, R), worst in WORST.items():
        assert worst <= pc.tolerance(filt, R)
