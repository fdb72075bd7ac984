"""pb_stitch_planar / pb_stitch_nv12: video frames of a double-fisheye source through the tile kernel pb_stitch_video_kernel -
the bytes of the definition (tests/stitch_video_ref.py) fed with the plan's own taps and factors (Plan.index_map(weights=True)) and, for
the three small cases, with the CPU oracle's; both sample sizes, the three subsamplings and NV12, every tile path (Plan.stitch_tile_mix
proves the list reaches them), layouts and launch shapes.  Every comparison is exact equality on independent random samples; destinations
sit between sentinel bytes that must survive, and so must the padding inside pitched frames."""

import numpy as np
import pytest
import torch

from photonbend_amd import _native as nat
from tests import cases as tc
from tests import helpers as H
from tests import stitch_video_ref as ref
from tests.cases import Case, dbl, pano
from tests.test_hip_double import CASES as DOUBLE_CASES
from tests.test_hip_nv12 import GUARD, SENTINEL, guarded, guards_intact
from tests.test_hip_planar import gather, layouts, random_frame, scatter, span

pytestmark = pytest.mark.gpu

SAMPLES = ((1, np.uint8), (2, np.uint16))
SUBS = {"444": nat.PLANAR_444, "422": nat.PLANAR_422, "420": nat.PLANAR_420}
FORMATS = ("444", "422", "420", "nv12")
UNSUPPORTED = -3
SMALL = ("E_stitch_195_raw", "E_stitch_180_masked", "E_stitch_eqs_rot")
MID = ("stitch_195_aligned", "stitch_195_rot", "stitch_200_chain", "fisheye_from_double", "double_from_double", "stitch_220_raw")
GEOMETRIES = [tc.case_by_name(n) for n in SMALL] + [
    Case("odd_half_width_40x82", pano(32, 64), dbl(40, 82, "equidistant", 195)),  # w // 2 = 41: a chroma block straddles the seam between the eyes
    Case("pano_48x96", pano(48, 96), dbl(40, 80, "equidistant", 195)),  # partial tiles
    Case("odd_destination_45x91", pano(45, 91), dbl(40, 80, "equidistant", 195), [(3, 90, -7)]),  # 4:4:4 only
] + [c for c in DOUBLE_CASES if c.name in MID]
assert len(GEOMETRIES) == 12
MIX = {}  # geometry -> Plan.stitch_tile_mix(), filled by the geometry test and read by the coverage test after it


def sub_of(fmt):
    return "420" if fmt == "nv12" else fmt


def dims_ok(case, fmt):
    return ref.dims_ok(sub_of(fmt), case.src[1:3], case.dst[1:3])


def plan_of(case):
    return H.pb_plan_private(case, bilinear=False)


def taps_of(plan):
    Hd, Wd = plan.dst.height, plan.dst.width
    idx, wts = plan.index_map(weights=True)
    idx, wts = idx.reshape(2, Hd, Wd).cpu().numpy(), wts.reshape(2, Hd, Wd).cpu().numpy()
    assert idx.dtype == np.int32 and wts.dtype == np.float64
    return idx[0], idx[1], wts[0], wts[1]


def stitch_call(plan, src_ptr, dst_ptr, fmt, S, n=1, sl=None, dl=None, fill=None, stream=None):
    """The raw C call: pb_stitch_nv12 for "nv12", pb_stitch_planar for a subsampling."""
    cls = nat.pb_nv12_layout if fmt == "nv12" else nat.pb_planar_layout
    sl, dl = (None if l is None else cls(*l) for l in (sl, dl))
    f = None if fill is None else (nat.C.c_uint16 * 3)(*fill)
    args = [plan.handle, src_ptr, dst_ptr, n, None if sl is None else nat.C.addressof(sl), None if dl is None else nat.C.addressof(dl)]
    args += ([] if fmt == "nv12" else [SUBS[fmt]]) + [S, None if f is None else nat.C.addressof(f), nat.current_stream() if stream is None else stream]
    return (nat.load().pb_stitch_nv12 if fmt == "nv12" else nat.load().pb_stitch_planar)(*args)


def run(plan, frame, fmt, fill=None):
    """One packed launch of a flat PLANAR frame -> the destination's flat planar frame ("nv12": interleaved on the way in, taken apart on
    the way out); the guards around the destination must survive."""
    h, w, Hd, Wd, S = plan.src.height, plan.src.width, plan.dst.height, plan.dst.width, frame.dtype.itemsize
    sub = sub_of(fmt)
    host = ref.nv12_of(frame, h, w) if fmt == "nv12" else frame
    src = torch.from_numpy(np.ascontiguousarray(host).view(np.uint8)).cuda()
    buf = guarded(ref.frame_samples(Hd, Wd, sub) * S)
    assert stitch_call(plan, src.data_ptr(), buf.data_ptr() + GUARD, fmt, S, fill=fill) == 0, nat.load().pb_last_error()
    torch.cuda.synchronize()
    assert guards_intact(buf), "the stitch wrote outside the destination frame"
    out = buf[GUARD:-GUARD].cpu().numpy().view(frame.dtype)
    if fmt == "nv12":
        uv = out[Hd * Wd :].reshape(Hd // 2, Wd // 2, 2)
        out = np.concatenate([out[: Hd * Wd], uv[..., 0].ravel(), uv[..., 1].ravel()])
    return out


def differing(got, want, Hd, Wd, sub):
    return [int((g != w).sum()) for g, w in zip(ref.planes(got, Hd, Wd, sub), ref.planes(want, Hd, Wd, sub))]


# ---- 1. every geometry x format x sample size x fill, exactly the definition --------------------------------------------------------------
@pytest.mark.parametrize("case", GEOMETRIES, ids=lambda c: c.name)
def test_every_format_equals_the_definition_fed_with_the_plan_s_taps(case):
    plan = plan_of(case)
    _, h, w, *_ = case.src
    Hd, Wd = case.dst[1], case.dst[2]
    taps = taps_of(plan)
    MIX[case.name] = plan.stitch_tile_mix()
    oracle = ref.oracle_taps(case) if case.name in SMALL and H.live_numpy_is_the_goldens_numpy() else None
    ran = 0
    for fmt in FORMATS:
        if not dims_ok(case, fmt):
            assert (Hd | Wd | h | w) & 1
            continue
        sub = sub_of(fmt)
        for S, dt in SAMPLES:
            assert (plan.stitch_nv12_supported(S) if fmt == "nv12" else plan.stitch_planar_supported(sub, S)), (case.name, fmt, S)
            frame = random_frame(h, w, sub, dt, seed=1000 + 10 * S + FORMATS.index(fmt))
            for fill in ((0, 0, 0), (201, 77, 1 << (8 * S - 1))):
                got = run(plan, frame, fmt, fill)
                want = ref.stitch_frame(frame, *taps, h, w, sub, fill)
                assert got.dtype == want.dtype and differing(got, want, Hd, Wd, sub) == [0, 0, 0], (case.name, fmt, S, fill, differing(got, want, Hd, Wd, sub))
                if oracle is not None:
                    assert np.array_equal(got, ref.stitch_frame(frame, *oracle, h, w, sub, fill)), (case.name, fmt, S, fill, "oracle")
                ran += 1
            if fmt == "nv12":  # NV12 is yuv420p interleaved
                assert np.array_equal(run(plan, frame, "nv12", (1, 2, 3)), run(plan, frame, "420", (1, 2, 3))), (case.name, S)
    assert ran == 4 * (1 + (not (w | Wd) & 1) + 2 * (not (h | w | Hd | Wd) & 1)), (case.name, ran)  # 4:4:4 always; 4:2:2: even widths; 4:2:0 and NV12: all even
    # 4:4:4 uint8, fill 0: the three planes are the three channels of the RGB8 stitch of the image built from the source planes
    frame = random_frame(h, w, "444", np.uint8, seed=1100)
    rgb = torch.from_numpy(np.ascontiguousarray(frame.reshape(3, h, w).transpose(1, 2, 0))).cuda()
    want = plan.remap(rgb).permute(2, 0, 1).contiguous().cpu().numpy().ravel()
    assert np.array_equal(run(plan, frame, "444", (0, 0, 0)), want), case.name
    # ... and the planes of a 4:4:4 frame are gbrp frames of themselves: Plan.stitch_planar on (3, h, w)
    got = plan.stitch_planar(torch.from_numpy(frame.reshape(3, h, w)).cuda(), "444", fill=(0, 0, 0)).cpu().numpy()
    assert got.shape == (3, Hd, Wd) and np.array_equal(got.ravel(), want)


def test_the_geometries_reach_every_path_of_the_kernel():
    """Runs after the geometry test (file order) and reads what it recorded; a geometry it did not run is classified here."""
    for case in GEOMETRIES:
        if case.name not in MIX:
            MIX[case.name] = plan_of(case).stitch_tile_mix()
    total = {k: sum(m[k] for m in MIX.values()) for k in next(iter(MIX.values()))}
    print("stitch_tile_mix per geometry:")
    for name, m in MIX.items():
        print(f"  {name:28s} {m}")
    print(f"  {'total':28s} {total}")
    for path in ("solo", "unit", "row", "lat", "failed", "fix_tiles", "fix_pixels", "fix_anchors_422", "fix_anchors_420"):
        assert total[path] > 0, f"no geometry of the list reaches the kernel's {path} path: {total}"
    assert MIX["stitch_195_aligned"]["row"] > 0 and MIX["stitch_195_rot"]["lat"] > 0


# ---- 2. layouts ------------------------------------------------------------------------------------------------------------------------------
LAYOUT_CASE = Case("layout_stitch_195_rot", pano(96, 192), dbl(100, 200, "equidistant", 195), [(3, 90, -7)])


@pytest.mark.parametrize("sub", ("444", "422", "420"))
@pytest.mark.parametrize("S,dt", SAMPLES)
def test_pitched_planes_padding_rows_swapped_planes_and_a_base_off_dword_alignment(S, dt, sub):
    case = LAYOUT_CASE
    plan = plan_of(case)
    _, h, w, *_ = case.src
    Hd, Wd = case.dst[1], case.dst[2]
    frame = random_frame(h, w, sub, dt, seed=1200 + S)
    want = run(plan, frame, sub)
    assert np.array_equal(want, ref.stitch_frame(frame, *taps_of(plan), h, w, sub))
    for (name, sl), dl in zip(layouts(h, w, S, sub).items(), layouts(Hd, Wd, S, sub).values()):
        for off in (0, S):  # one sample off dword alignment: the sample-by-sample store path runs
            ns, nd = span(sl, h, w, S, sub), span(dl, Hd, Wd, S, sub)
            src = torch.zeros(ns + 512, dtype=torch.uint8, device="cuda")
            s_off = (-src.data_ptr()) % 256 + off
            src[s_off : s_off + ns] = torch.from_numpy(scatter(frame, sl, h, w, S, sub, seed=1201)).cuda()
            buf = guarded(nd + 512)
            d_off = GUARD + (-(buf.data_ptr() + GUARD)) % 256 + off
            assert stitch_call(plan, src.data_ptr() + s_off, buf.data_ptr() + d_off, sub, S, sl=sl + (0,), dl=dl + (0,)) == 0, (name, nat.load().pb_last_error())
            torch.cuda.synchronize()
            host = buf.cpu().numpy()
            got, padding = gather(host[d_off : d_off + nd], dl, Hd, Wd, dt, sub)
            assert np.array_equal(got, want), (name, off)
            assert bool((padding == SENTINEL).all()) and bool((host[:d_off] == SENTINEL).all()) and bool((host[d_off + nd :] == SENTINEL).all()), (name, off)


@pytest.mark.parametrize("S,dt", SAMPLES)
def test_nv12_at_a_pitch_and_a_uv_offset_of_its_own(S, dt):
    case = LAYOUT_CASE
    plan = plan_of(case)
    _, h, w, *_ = case.src
    Hd, Wd = case.dst[1], case.dst[2]
    frame = random_frame(h, w, "420", dt, seed=1300 + S)
    want = ref.nv12_of(run(plan, frame, "nv12"), Hd, Wd).view(np.uint8)
    semi = ref.nv12_of(frame, h, w).view(np.uint8).reshape(3 * h // 2, w * S)
    sp, dp = w * S + 6 * S, Wd * S + 10 * S
    sl, dl = (sp, sp * (h + 2), 0), (dp, dp * (Hd + 3), 0)
    src_host = np.random.default_rng(1301).integers(0, 256, sl[1] + sp * (h // 2), dtype=np.uint8)
    src_host[: sp * h].reshape(h, sp)[:, : w * S] = semi[:h]
    src_host[sl[1] :].reshape(h // 2, sp)[:, : w * S] = semi[h:]
    nd = dl[1] + dp * (Hd // 2)
    for off in (0, 2 * S):  # one pair off dword alignment at S = 1
        src = torch.zeros(len(src_host) + 512, dtype=torch.uint8, device="cuda")
        s_off = (-src.data_ptr()) % 256 + off
        src[s_off : s_off + len(src_host)] = torch.from_numpy(src_host).cuda()
        buf = guarded(nd + 512)
        d_off = GUARD + (-(buf.data_ptr() + GUARD)) % 256 + off
        assert stitch_call(plan, src.data_ptr() + s_off, buf.data_ptr() + d_off, "nv12", S, sl=sl, dl=dl) == 0, nat.load().pb_last_error()
        torch.cuda.synchronize()
        host = buf.cpu().numpy()
        body = host[d_off : d_off + nd]
        pay = np.zeros(nd, bool)
        pay[: dp * Hd].reshape(Hd, dp)[:, : Wd * S] = True
        pay[dl[1] :].reshape(Hd // 2, dp)[:, : Wd * S] = True
        assert np.array_equal(body[pay], want), off
        assert bool((body[~pay] == SENTINEL).all()) and bool((host[:d_off] == SENTINEL).all()) and bool((host[d_off + nd :] == SENTINEL).all()), off


@pytest.mark.parametrize("fmt", FORMATS)
def test_three_frames_at_padded_strides_equal_three_single_launches(fmt):
    case = LAYOUT_CASE
    plan = plan_of(case)
    _, h, w, *_ = case.src
    Hd, Wd = case.dst[1], case.dst[2]
    sub = sub_of(fmt)
    zeros = (0,) * (2 if fmt == "nv12" else 4)
    for S, dt in SAMPLES:
        sb, db = ref.frame_samples(h, w, sub) * S, ref.frame_samples(Hd, Wd, sub) * S
        for pad in (2 * S, 48):
            ss, ds = sb + pad, db + pad
            src_host = np.random.default_rng(1400 + S + pad).integers(0, 256, 3 * ss, dtype=np.uint8)  # (random bytes in the padding too)
            src = torch.from_numpy(src_host).cuda()
            buf = guarded(3 * ds)
            assert stitch_call(plan, src.data_ptr(), buf.data_ptr() + GUARD, fmt, S, 3, zeros + (ss,), zeros + (ds,)) == 0, nat.load().pb_last_error()
            torch.cuda.synchronize()
            assert guards_intact(buf)
            got = buf[GUARD:-GUARD].cpu().numpy()
            for f in range(3):
                one = torch.from_numpy(src_host[f * ss : f * ss + sb].copy()).cuda()
                single = guarded(db)
                assert stitch_call(plan, one.data_ptr(), single.data_ptr() + GUARD, fmt, S) == 0
                torch.cuda.synchronize()
                assert np.array_equal(got[f * ds : f * ds + db], single[GUARD:-GUARD].cpu().numpy()), (fmt, S, pad, f)
                assert bool((got[f * ds + db : (f + 1) * ds] == SENTINEL).all()), (fmt, S, pad, f)  # the padding is intact
    # ... and through the Plan methods: (N, frame) in and out
    frames = np.stack([random_frame(h, w, sub, np.uint8, seed=1410 + f) for f in range(3)])
    if fmt == "nv12":
        semi = np.stack([ref.nv12_of(f, h, w).reshape(3 * h // 2, w) for f in frames])
        got = plan.stitch_nv12(torch.from_numpy(semi).cuda()).cpu().numpy()
        assert got.shape == (3, 3 * Hd // 2, Wd)
        assert all(np.array_equal(got[f].ravel(), ref.nv12_of(run(plan, frames[f], "nv12"), Hd, Wd)) for f in range(3))
    else:
        got = plan.stitch_planar(torch.from_numpy(frames).cuda(), sub).cpu().numpy()
        assert got.shape == (3, ref.frame_samples(Hd, Wd, sub)) and all(np.array_equal(got[f], run(plan, frames[f], sub)) for f in range(3))


# ---- 3. graph capture and streams ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FORMATS)
def test_a_captured_launch_and_launches_on_three_streams_give_the_plain_bytes(fmt):
    case = LAYOUT_CASE
    plan = plan_of(case)
    _, h, w, *_ = case.src
    sub, S = sub_of(fmt), 1
    nd = ref.frame_samples(case.dst[1], case.dst[2], sub) * S
    src = torch.from_numpy(random_frame(h, w, sub, np.uint8, seed=1500)).cuda()
    want = torch.zeros(nd, dtype=torch.uint8, device="cuda")
    assert stitch_call(plan, src.data_ptr(), want.data_ptr(), fmt, S) == 0
    torch.cuda.synchronize()
    g_out = torch.zeros(nd, dtype=torch.uint8, device="cuda")
    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            assert stitch_call(plan, src.data_ptr(), g_out.data_ptr(), fmt, S, stream=int(side.cuda_stream)) == 0
    torch.cuda.current_stream().wait_stream(side)
    g_out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(g_out, want)
    streams = [torch.cuda.Stream() for _ in range(3)]
    outs = [torch.zeros(nd, dtype=torch.uint8, device="cuda") for _ in streams]
    torch.cuda.synchronize()
    for s, o in zip(streams, outs):
        assert stitch_call(plan, src.data_ptr(), o.data_ptr(), fmt, S, stream=int(s.cuda_stream)) == 0
    torch.cuda.synchronize()
    assert all(torch.equal(o, want) for o in outs)


# ---- 4. plans the kernel does not serve ----------------------------------------------------------------------------------------------------
def test_unsupported_plans_say_so_and_write_nothing():
    L = nat.load()
    double, single = tc.case_by_name("E_stitch_195_raw"), Case("pano_from_pano", pano(32, 64), pano(40, 80))
    faithful = plan_of(double)
    faithful.set_mode(nat.MODE_FAITHFUL)
    for what, case, plan, word in (("deferred", double, H.pb_plan_private(double, defer=True, bilinear=False), b"prepared double-fisheye plans"),
                                   ("faithful", double, faithful, b"prepared double-fisheye plans"),
                                   ("single source", single, plan_of(single), b"takes double-fisheye sources")):
        _, h, w, *_ = case.src
        Hd, Wd = case.dst[1], case.dst[2]
        for fmt in FORMATS:
            sub = sub_of(fmt)
            for S, dt in SAMPLES:
                assert not (plan.stitch_nv12_supported(S) if fmt == "nv12" else plan.stitch_planar_supported(sub, S)), (what, fmt, S)
                frame = torch.from_numpy(random_frame(h, w, sub, dt, seed=1600 + S)).cuda()
                buf = guarded(ref.frame_samples(Hd, Wd, sub) * S)
                assert stitch_call(plan, frame.data_ptr(), buf.data_ptr() + GUARD, fmt, S) == UNSUPPORTED, (what, fmt, S)
                msg = L.pb_last_error()
                assert word in msg and (b"pb_stitch_nv12" if fmt == "nv12" else b"pb_stitch_planar") in msg, (what, msg)
                if what == "single source":
                    assert (b"pb_remap_nv12" if fmt == "nv12" else b"pb_remap_planar") in msg
                torch.cuda.synchronize()
                assert bool((buf == SENTINEL).all()), (what, fmt, S)
                with pytest.raises(nat.PbError):
                    plan.stitch_planar(frame, sub) if fmt != "nv12" else plan.stitch_nv12(frame.reshape(3 * h // 2, w))
    # the served plan keeps refusing the single-source calls, and the double plan is what the stitch takes
    served = plan_of(double)
    assert served.stitch_planar_supported("420", 1) and served.stitch_nv12_supported(2) and not served.planar_supported("420", 1) and not served.nv12_supported(1)
    assert all(v == 0 for v in plan_of(single).stitch_tile_mix().values())
