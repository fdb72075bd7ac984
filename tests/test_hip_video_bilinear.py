"""pb_remap_planar_bilinear / pb_remap_nv12_bilinear: bilinear sampling of planar and NV12 / P010 video frames through the tile
kernel pb_planar_bilinear_kernel, against the written definition tests/video_bilinear_ref.py.

Frames are independent random samples: a coordinate error of e px moves a sample by up to e x R, R the largest sample value.  The tile
kernels' coordinates are certified to 1/1024 px per axis, so EVERY sample must be within T(R) = 1 + R // 512 of the definition
(video_bilinear_ref.tolerance) - 1 for 8-bit samples, 2 for 10-bit samples stored low, 128 for full 16-bit ones.  A sample may be excused
only if it is fill in exactly one of the two results AND its pixel (for planes 1 and 2: its anchor) lies in
interp_cases.edge_band(case, final, 1/512); the excused samples are counted and may not outnumber the band's pixels, so a panorama source
excuses nothing (tests/test_video_interp_cases_host.py caps the band at 0.5 % of a case's pixels).
How the frames reach the kernel - pitches, padding rows, swapped planes, unaligned bases, batches, a captured graph, several streams - never
moves a byte."""

import functools

import numpy as np
import pytest
import torch

from photonbend_amd import _native as nat
from tests import cases as tc
from tests import cubemap_cases as cc
from tests import helpers as H
from tests import interp_cases as ic
from tests import planar_ref as pr
from tests import video_bilinear_ref as vb
from tests import video_interp_cases as vc
from tests.cases import Case, cam, inscribed, pano
from tests.test_hip_nv12 import GUARD, SENTINEL, guarded, guards_intact
from tests.test_hip_planar import gather, layouts, scatter, span

pytestmark = pytest.mark.gpu

SUBS = {"444": nat.PLANAR_444, "422": nat.PLANAR_422, "420": nat.PLANAR_420}
UNSUPPORTED = -3
# sample type -> (dtype, the largest sample value drawn: R)
FORMS = {"u8": (np.uint8, 255), "u10": (np.uint16, 1023), "u16": (np.uint16, 65535)}
LAYOUTS = ("444", "422", "420", "nv12")
# a 360-degree equisolid rim under a rotation (tests/test_hip_catmull_rom_tiles.py): window, table and TD3 entries and hundreds of fix pixels
COV_RIM = Case("cov_rim", cam(512, 512, "equisolid", 360, inscribed(512)), cam(512, 512, "equidistant", 360, inscribed(512)), [(30, 45, 10)])
WORST = {}  # sample type -> the largest deviation from the definition seen in this run (printed; recorded in DESIGN 3.18)


def _plan(case, **kw):
    src, cmap = cc.pb_chain(case, image=np.zeros((case.src[1], case.src[2], 3), np.uint8))
    kw.setdefault("bilinear", True)
    return nat.Plan(cmap.dst_proj, cmap.rotations, src._proj("src"), **kw)


def _case(name):
    return COV_RIM if name == COV_RIM.name else vc.by_name(name)


@functools.lru_cache(maxsize=None)
def _ref(name):
    """The definition's coordinates of a case, computed once and shared (read-only): fy, fx, live, source kind, edge band."""
    case = _case(name)
    final = ic.final_map(case)
    fy, fx, live, kind = vc.coords(case, final)
    band = ic.edge_band(case, final, vc.BAND)
    for a in (fy, fx, live, band):
        a.setflags(write=False)
    return fy, fx, live, kind, band


def draw(h, w, sub, form, seed):
    """A packed flat frame of independent random samples in [0, R]."""
    dt, top = FORMS[form]
    return np.random.default_rng(seed).integers(0, top + 1, size=pr.frame_samples(h, w, sub), dtype=dt)


def to_nv12(frame, h, w):
    p0, p1, p2 = pr.planes(frame, h, w, "420")
    return np.ascontiguousarray(np.concatenate([p0, np.stack([p1, p2], axis=2).reshape(h // 2, w)], axis=0))


def from_nv12(semi, h, w):
    uv = semi[h:].reshape(h // 2, w // 2, 2)
    return np.concatenate([semi[:h].ravel(), uv[:, :, 0].ravel(), uv[:, :, 1].ravel()])


def planar_call(plan, src_ptr, dst_ptr, sub, S, n=1, sl=None, dl=None, fill=None, stream=None):
    sl = None if sl is None else nat.pb_planar_layout(*sl)
    dl = None if dl is None else nat.pb_planar_layout(*dl)
    f = None if fill is None else (nat.C.c_uint16 * 3)(*fill)
    return nat.load().pb_remap_planar_bilinear(plan.handle, src_ptr, dst_ptr, n, None if sl is None else nat.C.addressof(sl), None if dl is None else nat.C.addressof(dl),
                                               SUBS[sub], S, None if f is None else nat.C.addressof(f), nat.current_stream() if stream is None else stream)


def nv12_call(plan, src_ptr, dst_ptr, S, n=1, sl=None, dl=None, fill=None, stream=None):
    sl = None if sl is None else nat.pb_nv12_layout(*sl)
    dl = None if dl is None else nat.pb_nv12_layout(*dl)
    f = None if fill is None else (nat.C.c_uint16 * 3)(*fill)
    return nat.load().pb_remap_nv12_bilinear(plan.handle, src_ptr, dst_ptr, n, None if sl is None else nat.C.addressof(sl), None if dl is None else nat.C.addressof(dl), S,
                                             None if f is None else nat.C.addressof(f), nat.current_stream() if stream is None else stream)


def run(plan, frame, layout, fill=None):
    """One packed launch of a flat planar frame (layout "444" / "422" / "420") or of that 4:2:0 frame interleaved (layout "nv12") -> the
    destination's flat PLANAR frame; the guards around the destination must survive."""
    S = frame.dtype.itemsize
    h, w, Hd, Wd = plan.src.height, plan.src.width, plan.dst.height, plan.dst.width
    sub = "420" if layout == "nv12" else layout
    src = torch.from_numpy((to_nv12(frame, h, w) if layout == "nv12" else frame).view(np.uint8).ravel()).cuda()
    buf = guarded(pr.frame_samples(Hd, Wd, sub) * S)
    if layout == "nv12":
        rc = nv12_call(plan, src.data_ptr(), buf.data_ptr() + GUARD, S, fill=fill)
    else:
        rc = planar_call(plan, src.data_ptr(), buf.data_ptr() + GUARD, sub, S, fill=fill)
    assert rc == 0, nat.load().pb_last_error()
    torch.cuda.synchronize()
    assert guards_intact(buf), "the bilinear video call wrote outside the destination frame"
    out = buf[GUARD:-GUARD].cpu().numpy().view(frame.dtype)
    return from_nv12(out.reshape(3 * Hd // 2, Wd), Hd, Wd) if layout == "nv12" else out


def check(got, want, live, band, sub, fill, T, what, form):
    """The comparison rule of this file, plane by plane -> the number of excused samples."""
    Hd, Wd = live.shape
    cx, cy = pr.SHIFTS[sub]
    excused = 0
    for k, (g, w) in enumerate(zip(pr.planes(got, Hd, Wd, sub), pr.planes(want, Hd, Wd, sub))):
        lv, bd = (live, band) if k == 0 else (live[0 :: 1 << cy, 0 :: 1 << cx], band[0 :: 1 << cy, 0 :: 1 << cx])
        d = np.abs(g.astype(np.int64) - w.astype(np.int64))
        flip = (g == fill[k]) != ~lv  # fill in exactly one of the two results (the definition's is fill exactly where the anchor is dead)
        ok = bd & flip
        WORST[form] = max(WORST.get(form, 0), int(d[~ok].max(initial=0)))
        off = (d > T) & ~ok
        where = np.argwhere(off)[:4].tolist()
        assert not off.any(), (f"{what} plane {k}: {int(off.sum())} samples beyond T = {T} of the definition (max {int(d[off].max())}; {int((off & flip).sum())} of them "
                               f"fill in one result only, outside the edge band), first at {where}: got {[int(g[y, x]) for y, x in where]}, "
                               f"want {[int(w[y, x]) for y, x in where]}")
        excused += int(((d > T) & ok).sum())
    return excused


def against_the_definition(case, plan, form, layouts_=LAYOUTS, seed=0):
    fy, fx, live, kind, band = _ref(case.name)
    dt, top = FORMS[form]
    _, h, w, *_ = case.src
    S = np.dtype(dt).itemsize
    fill = (top, 0, top // 2 + 1)  # (inside [0, R]: R is the largest sample value of the frame and the fills)
    T = vb.tolerance(top)
    worst0 = WORST.get(form, 0)
    for layout in layouts_:
        sub = "420" if layout == "nv12" else layout
        assert plan.nv12_supported(S, interpolation="bilinear") if layout == "nv12" else plan.planar_supported(sub, S, interpolation="bilinear"), (case.name, layout, S)
        frame = draw(h, w, sub, form, seed + 7 * LAYOUTS.index(layout))
        want = vb.remap_frame(frame, fy, fx, live, kind, h, w, sub, fill)
        excused = check(run(plan, frame, layout, fill), want, live, band, sub, fill, T, f"{case.name} {layout} {form}", form)
        assert excused <= int(band.sum()), f"{case.name} {layout} {form}: {excused} samples excused, the edge band holds {int(band.sum())} pixels"
        if kind == "pano":
            assert excused == 0
    print(f"{case.name} {form}: T = {T}, largest deviation so far {max(worst0, WORST.get(form, 0))}, edge band {int(band.sum())} px")


# ---- 1. every case, every form, against the definition --------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("case", vc.CASES, ids=lambda c: c.name)
def test_every_case_in_every_form_against_the_definition(case, form):
    against_the_definition(case, _plan(case), form)


def test_the_default_fill_is_video_black_and_the_python_methods_make_the_same_launch():
    case = vc.by_name("video_pano_from_cam_4x6")  # (a camera source: dead pixels around the frame)
    plan = _plan(case)
    fy, fx, live, kind, band = _ref(case.name)
    _, h, w, *_ = case.src
    assert int((~live).sum()) > 0
    for form in ("u8", "u16"):
        for sub in pr.SUBSAMPLINGS:
            frame = draw(h, w, sub, form, 11)
            got = run(plan, frame, sub)
            check(got, vb.remap_frame(frame, fy, fx, live, kind, h, w, sub), live, band, sub, pr.default_fill(frame.dtype), vb.tolerance(FORMS[form][1]), f"default fill {sub} {form}", form)
            assert np.array_equal(plan.remap_planar(torch.from_numpy(frame).cuda(), sub, interpolation="bilinear").cpu().numpy(), got)
            assert not np.array_equal(plan.remap_planar(torch.from_numpy(frame).cuda(), sub).cpu().numpy(), got)  # (the default samples nearest)
        frame = draw(h, w, "420", form, 12)
        semi = plan.remap_nv12(torch.from_numpy(to_nv12(frame, h, w)).cuda(), interpolation="bilinear").cpu().numpy()
        assert np.array_equal(from_nv12(semi, case.dst[1], case.dst[2]), run(plan, frame, "nv12"))
    with pytest.raises(ValueError):
        plan.remap_planar(torch.from_numpy(frame).cuda(), "420", interpolation="cubic")


# ---- 2. what the kernel branches on is all there ----------------------------------------------------------------------------------------
CLASS_CASES = [c.name for c in vc.CASES if c.dst[1] * c.dst[2] >= 10000] + [COV_RIM.name]


def test_the_cases_cover_every_tile_class_the_kernel_has_a_path_for():
    """Model tiles plain and TD3, table tiles, black tiles, modelled tiles with fix pixels, fix pixels that are anchors (at 4:2:0, so at
    every subsampling).  A missing class is a failure."""
    keys = ("window", "direct", "table", "black", "td3", "fix_tiles", "fix_pixels", "fix_anchors_422", "fix_anchors_420")
    total = dict.fromkeys(keys, 0)
    for name in CLASS_CASES:
        mix = _plan(_case(name)).bilinear_tile_mix()
        print(f"{name:26s} " + " ".join(f"{k} {mix[k]}" for k in keys))
        for k in keys:
            total[k] += mix[k]
    model = total["window"] + total["direct"]
    assert model - total["td3"] > 0 and total["td3"] > 0 and total["table"] > 0 and total["black"] > 0, total
    assert total["fix_tiles"] > 0 and total["fix_anchors_420"] > 0 and total["fix_anchors_422"] > total["fix_anchors_420"], total


@pytest.mark.parametrize("form", FORMS)
def test_the_coverage_case_against_the_definition(form):
    against_the_definition(COV_RIM, _plan(COV_RIM), form, seed=40)


# ---- 3. layouts -------------------------------------------------------------------------------------------------------------------------
LAYOUT_CASES = {"420": "video_odd_dst_36x62", "422": "sweep5", "444": "video_pano_from_cam_4x6", "nv12": "sweep3"}
SAMPLES = ((1, "u8"), (2, "u16"))


@pytest.mark.parametrize("S,form", SAMPLES)
@pytest.mark.parametrize("sub", pr.SUBSAMPLINGS)
def test_planar_layouts_give_the_bytes_of_the_packed_launch_and_leave_the_padding(sub, S, form):
    """Pitched planes with padding rows, swapped chroma planes, a base one sample off 256-byte alignment (1 byte at S = 1, 2 at S = 2: off
    dword alignment, the sample-by-sample stores run)."""
    case = vc.by_name(LAYOUT_CASES[sub])
    plan = _plan(case)
    _, h, w, *_ = case.src
    Hd, Wd = case.dst[1], case.dst[2]
    frame = draw(h, w, sub, form, 400 + S)
    dt = frame.dtype
    want = run(plan, frame, sub)
    for (name, sl), dl in zip(layouts(h, w, S, sub).items(), layouts(Hd, Wd, S, sub).values()):
        for off in (0, S):
            ns, nd = span(sl, h, w, S, sub), span(dl, Hd, Wd, S, sub)
            src = torch.zeros(ns + 512, dtype=torch.uint8, device="cuda")
            s_off = (-src.data_ptr()) % 256 + off
            src[s_off : s_off + ns] = torch.from_numpy(scatter(frame, sl, h, w, S, sub, seed=401)).cuda()
            buf = guarded(nd + 512)
            d_off = GUARD + (-(buf.data_ptr() + GUARD)) % 256 + off
            assert planar_call(plan, src.data_ptr() + s_off, buf.data_ptr() + d_off, sub, S, sl=sl + (0,), dl=dl + (0,)) == 0, (name, nat.load().pb_last_error())
            torch.cuda.synchronize()
            host = buf.cpu().numpy()
            got, padding = gather(host[d_off : d_off + nd], dl, Hd, Wd, dt, sub)
            assert np.array_equal(got, want), (name, off)
            assert bool((padding == SENTINEL).all()) and bool((host[:d_off] == SENTINEL).all()) and bool((host[d_off + nd :] == SENTINEL).all()), (name, off)
    # three frames at padded strides
    sb, db = frame.nbytes, want.nbytes
    for pad in (S, 48):
        ss, ds = sb + pad, db + pad
        src_host = np.random.default_rng(500 + S + pad).integers(0, 256, 3 * ss, dtype=np.uint8)  # (random bytes in the padding too)
        buf = guarded(3 * ds)
        src = torch.from_numpy(src_host).cuda()
        assert planar_call(plan, src.data_ptr(), buf.data_ptr() + GUARD, sub, S, 3, (0, 0, 0, 0, ss), (0, 0, 0, 0, ds)) == 0
        torch.cuda.synchronize()
        assert guards_intact(buf)
        got = buf[GUARD:-GUARD].cpu().numpy()
        for f in range(3):
            single = run(plan, src_host[f * ss : f * ss + sb].view(dt), sub)
            assert np.array_equal(got[f * ds : f * ds + db].view(dt), single), (sub, S, pad, f)
            assert bool((got[f * ds + db : (f + 1) * ds] == SENTINEL).all()), (sub, S, pad, f)


@pytest.mark.parametrize("S,form", SAMPLES)
def test_nv12_layouts_give_the_bytes_of_the_packed_launch_and_leave_the_padding(S, form):
    """A pitch with padding, padding rows between the two planes, a base one pair off 256-byte alignment (2 bytes at S = 1: off dword
    alignment; 4 bytes at S = 2: off 8-byte alignment - a P010 pointer is pair-aligned), three frames at padded strides."""
    case = vc.by_name(LAYOUT_CASES["nv12"])
    plan = _plan(case)
    _, h, w, *_ = case.src
    Hd, Wd = case.dst[1], case.dst[2]
    frame = draw(h, w, "420", form, 450 + S)
    dt = frame.dtype
    semi = to_nv12(frame, h, w)
    want = to_nv12(run(plan, frame, "nv12"), Hd, Wd)

    def lay(hh, ww):
        p = ww * S + 6 * S
        return p, p * (hh + 3)  # pitch, uv_offset

    def put(rows2d, pitch, uv, hh, ww, fill_byte=None):
        n = uv + pitch * (hh // 2 - 1) + ww * S
        b = np.random.default_rng(451).integers(0, 256, n, dtype=np.uint8) if fill_byte is None else np.full(n, fill_byte, np.uint8)
        pay = np.zeros(n, bool)
        raw = rows2d.view(np.uint8).reshape(3 * hh // 2, ww * S)
        for y in range(3 * hh // 2):
            o = y * pitch if y < hh else uv + (y - hh) * pitch
            b[o : o + ww * S] = raw[y]
            pay[o : o + ww * S] = True
        return b, pay

    (sp, suv), (dp, duv) = lay(h, w), lay(Hd, Wd)
    sbuf, _ = put(semi, sp, suv, h, w)
    dref, pay = put(want, dp, duv, Hd, Wd, SENTINEL)
    for off in (0, 2 * S):
        src = torch.zeros(len(sbuf) + 512, dtype=torch.uint8, device="cuda")
        s_off = (-src.data_ptr()) % 256 + off
        src[s_off : s_off + len(sbuf)] = torch.from_numpy(sbuf).cuda()
        buf = guarded(len(dref) + 512)
        d_off = GUARD + (-(buf.data_ptr() + GUARD)) % 256 + off
        assert nv12_call(plan, src.data_ptr() + s_off, buf.data_ptr() + d_off, S, sl=(sp, suv, 0), dl=(dp, duv, 0)) == 0, nat.load().pb_last_error()
        torch.cuda.synchronize()
        host = buf.cpu().numpy()
        assert np.array_equal(host[d_off : d_off + len(dref)], dref), off  # (the payload and, around it, the sentinels of the padding)
        assert bool((host[:d_off] == SENTINEL).all()) and bool((host[d_off + len(dref) :] == SENTINEL).all()), off
    assert int((~pay).sum()) > 0
    sb, db = semi.nbytes, want.nbytes
    for pad in (2 * S, 48):
        ss, ds = sb + pad, db + pad
        src_host = np.random.default_rng(460 + S + pad).integers(0, 256, 3 * ss, dtype=np.uint8)
        buf = guarded(3 * ds)
        src = torch.from_numpy(src_host).cuda()
        assert nv12_call(plan, src.data_ptr(), buf.data_ptr() + GUARD, S, 3, (0, 0, ss), (0, 0, ds)) == 0
        torch.cuda.synchronize()
        assert guards_intact(buf)
        got = buf[GUARD:-GUARD].cpu().numpy()
        for f in range(3):
            one = from_nv12(src_host[f * ss : f * ss + sb].view(dt).reshape(3 * h // 2, w), h, w)
            single = to_nv12(run(plan, one, "nv12"), Hd, Wd)
            assert np.array_equal(got[f * ds : f * ds + db].view(dt), single.ravel()), (S, pad, f)
            assert bool((got[f * ds + db : (f + 1) * ds] == SENTINEL).all()), (S, pad, f)


# ---- 4. cross-checks --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,form", SAMPLES)
def test_444_planes_are_gbrp_remaps_of_themselves_and_nv12_is_420_interleaved(S, form):
    for name in ("sweep10", "mag_pano_from_cam"):
        case = vc.by_name(name)
        plan = _plan(case)
        _, h, w, *_ = case.src
        Hd, Wd = case.dst[1], case.dst[2]
        frame = draw(h, w, "444", form, 600 + S)
        got = pr.planes(run(plan, frame, "444", fill=(0, 0, 0)), Hd, Wd, "444")
        for k, plane in enumerate(pr.planes(frame, h, w, "444")):
            gbrp = np.concatenate([plane.ravel()] * 3)
            out = pr.planes(run(plan, gbrp, "444", fill=(0, 0, 0)), Hd, Wd, "444")
            assert np.array_equal(out[0], got[k]) and np.array_equal(out[1], got[k]) and np.array_equal(out[2], got[k]), (name, k)
        frame = draw(h, w, "420", form, 610 + S)
        assert np.array_equal(run(plan, frame, "nv12"), run(plan, frame, "420")), name
        assert np.array_equal(run(plan, frame, "nv12", fill=(1, 2, 3)), run(plan, frame, "420", fill=(1, 2, 3))), name


@pytest.mark.parametrize("layout", LAYOUTS)
def test_a_captured_launch_and_launches_on_three_streams_give_the_plain_bytes(layout):
    case = vc.by_name("sweep10")
    plan = _plan(case)
    _, h, w, *_ = case.src
    sub = "420" if layout == "nv12" else layout
    for S, form in SAMPLES:
        frame = draw(h, w, sub, form, 800 + S)
        host = to_nv12(frame, h, w) if layout == "nv12" else frame
        src = torch.from_numpy(host.view(np.uint8).ravel()).cuda()
        nd = pr.frame_samples(case.dst[1], case.dst[2], sub) * S

        def call(dst, stream=None):
            if layout == "nv12":
                return nv12_call(plan, src.data_ptr(), dst.data_ptr(), S, stream=stream)
            return planar_call(plan, src.data_ptr(), dst.data_ptr(), sub, S, stream=stream)

        want = torch.zeros(nd, dtype=torch.uint8, device="cuda")
        assert call(want) == 0
        torch.cuda.synchronize()
        # never allocates or synchronises: the call captures into a graph, and a replay writes the frame again
        g_out = torch.zeros(nd, dtype=torch.uint8, device="cuda")
        graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            with torch.cuda.graph(graph, stream=side):
                assert call(g_out, int(side.cuda_stream)) == 0
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
            assert call(o, int(s.cuda_stream)) == 0
        torch.cuda.synchronize()
        assert all(torch.equal(o, want) for o in outs)


# ---- 5. plans the kernel does not serve -------------------------------------------------------------------------------------------------
def test_unsupported_plans_say_so_and_write_nothing():
    L = nat.load()
    single, double = tc.case_by_name("D_photo_rot"), tc.case_by_name("E_stitch_195_raw")
    cube = Case("cube_source", pano(32, 64), cc.cube(16))
    faithful = H.pb_plan_private(single, bilinear=True)
    faithful.set_mode(nat.MODE_FAITHFUL)
    plans = (("deferred", single, H.pb_plan_private(single, defer=True), b"prepared plans"), ("faithful", single, faithful, b"prepared plans"),
             ("double-fisheye", double, H.pb_plan_private(double, bilinear=True), b"prepared plans"), ("cube", cube, _plan(cube), b"cube source"),
             ("bilinear=False", single, H.pb_plan_private(single, bilinear=False), b"pb_plan_prepare(plan, PB_PLAN_BILINEAR)"))
    for what, case, plan, message in plans:
        _, h, w, *_ = case.src
        Hd, Wd = case.dst[1], case.dst[2]
        for S, form in SAMPLES:
            for layout in LAYOUTS:
                sub = "420" if layout == "nv12" else layout
                assert pr.dims_ok(sub, (h, w), (Hd, Wd)), what
                if layout == "nv12":
                    assert L.pb_remap_nv12_bilinear_supported(plan.handle, S) == 0 and not plan.nv12_supported(S, interpolation="bilinear"), (what, S)
                else:
                    assert L.pb_remap_planar_bilinear_supported(plan.handle, SUBS[sub], S) == 0 and not plan.planar_supported(sub, S, interpolation="bilinear"), (what, sub, S)
                frame = draw(h, w, sub, form, 700 + S)
                src = torch.from_numpy((to_nv12(frame, h, w) if layout == "nv12" else frame).view(np.uint8).ravel()).cuda()
                buf = guarded(pr.frame_samples(Hd, Wd, sub) * S)
                rc = nv12_call(plan, src.data_ptr(), buf.data_ptr() + GUARD, S) if layout == "nv12" else planar_call(plan, src.data_ptr(), buf.data_ptr() + GUARD, sub, S)
                assert rc == UNSUPPORTED and message in L.pb_last_error(), (what, layout, S, rc, L.pb_last_error())
                torch.cuda.synchronize()
                assert bool((buf == SENTINEL).all()), (what, layout, S)
        with pytest.raises(nat.PbError):
            plan.remap_planar(torch.from_numpy(draw(h, w, "444", "u8", 1)).cuda(), "444", interpolation="bilinear")
    # the nearest calls serve the plans the bilinear call refuses for its tables' sake
    assert plans[3][2].planar_supported("420") and plans[4][2].planar_supported("420") and plans[4][2].nv12_supported()


def test_the_largest_deviations_seen():
    """Not a check of its own: prints what the tests above saw, for DESIGN 3.18 (run after them, in file order)."""
    print("largest deviation from the definition per sample type:", {k: (v, vb.tolerance(FORMS[k][1])) for k, v in sorted(WORST.items())})
    for form, worst in WORST.items():
        assert worst <= vb.tolerance(FORMS[form][1])
