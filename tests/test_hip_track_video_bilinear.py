"""pb_remap_track_planar_bilinear / pb_remap_track_nv12_bilinear: video frames with a rotation per frame in one launch,
sampled bilinearly.  Frame f must be, byte for byte, tests/video_bilinear_ref.py's definition at the (fy, fx, live) of the float64 chain
"the plan's own rotations, then frame f's" (tests/video_interp_cases.coords of tests/interp_cases.final_map).  Every comparison is exact
equality, for uint8 and uint16 samples alike: the kernel holds the float64 coordinate and evaluates the definition's own float64
expression.  Planes hold independent random bytes; destinations sit between sentinel bytes that must survive, and so must every padding
byte of pitched frames.  Shapes are tens of pixels a side."""

import functools

import numpy as np
import pytest
import torch

from photonbend_amd import _native as nat
from tests import interp_cases as ic
from tests import planar_ref
from tests import test_hip_track_nv12 as tn
from tests import test_hip_track_planar as tp
from tests import video_bilinear_ref as vbr
from tests import video_interp_cases as vic
from tests.cases import Case, cam, inscribed, pano
from tests.test_hip_track_nv12 import DEGREES, F, GUARD, PLAN_DEGREES, SENTINEL, cube, eac, mats_of, projections, track_mats

pytestmark = pytest.mark.gpu

SAMPLES = ((1, np.uint8), (2, np.uint16))
FORMS = ("444", "422", "420", "nv12")
SUBS = tp.SUBS
UNSUPPORTED = -3
HALF_QUAD = (cam(34, 30, "equidistant", 180), pano(16, 32))                        # W % 4 == 2: a half quad ends every row
CAMERA_RIM = (pano(20, 40), cam(40, 40, "equisolid", 190, inscribed(40)))          # a camera source with a liveness rim
ODD = (cam(33, 35, "equidistant", 180), pano(3, 5))                                # odd sizes, a quad of one: 4:4:4 only
ONE_CHROMA_SAMPLE = [(pano(2, 2), pano(2, 2)), (pano(4, 6), pano(2, 2))]           # a 1 x 1 chroma plane: wrap and clamp do all the work


def forms_of(dst, src):
    subs = [s for s in planar_ref.SUBSAMPLINGS if planar_ref.dims_ok(s, dst[1:3], src[1:3])]
    return subs + (["nv12"] if "420" in subs else [])


def random_frames(form, n, h, w, dt, seed):
    return tn.random_frames(n, h, w, dt, seed) if form == "nv12" else tp.random_frames(n, h, w, form, dt, seed)


@functools.lru_cache(maxsize=None)
def chain_coords(dst, src, n, k, n_rot):
    """[(fy, fx, live, kind)] per frame: the definition's coordinates of the chain PLAN_DEGREES[:n_rot] + frame f's k of DEGREES, on the
    host, computed once per geometry and shared by every form, sample size and fill."""
    out = []
    for f in range(n):
        case = Case("track", dst, src, list(PLAN_DEGREES[:n_rot]) + list(DEGREES[f * k : (f + 1) * k]))
        out.append(vic.coords(case, ic.final_map(case)))
    return out


def expected(form, coords, frames, h, w, fill=None):
    if form == "nv12":
        return np.stack([vbr.remap_nv12(frames[f], *coords[f], h, w, fill) for f in range(len(frames))])
    return np.stack([vbr.remap_frame(frames[f], *coords[f], h, w, form, fill) for f in range(len(frames))])


def call(form, plan, table_ptr, k, src_ptr, dst_ptr, n, S, sl=None, dl=None, fill=None, stream=None, bilinear=True):
    """The C call of a form: pb_remap_track_nv12[_bilinear] or pb_remap_track_planar[_bilinear]."""
    L = nat.load()
    f = None if fill is None else (nat.C.c_uint16 * 3)(*fill)
    st = nat.current_stream() if stream is None else stream
    if form == "nv12":
        sl, dl = (None if v is None else nat.pb_nv12_layout(*v) for v in (sl, dl))
        fn = L.pb_remap_track_nv12_bilinear if bilinear else L.pb_remap_track_nv12
        return fn(plan.handle, table_ptr, k, src_ptr, dst_ptr, n, None if sl is None else nat.C.addressof(sl), None if dl is None else nat.C.addressof(dl), S,
                  None if f is None else nat.C.addressof(f), st)
    sl, dl = (None if v is None else nat.pb_planar_layout(*v) for v in (sl, dl))
    fn = L.pb_remap_track_planar_bilinear if bilinear else L.pb_remap_track_planar
    return fn(plan.handle, table_ptr, k, src_ptr, dst_ptr, n, None if sl is None else nat.C.addressof(sl), None if dl is None else nat.C.addressof(dl), SUBS[form], S,
              None if f is None else nat.C.addressof(f), st)


def layouts(form, plan, S, src_kw, dst_kw):
    h, w, Hd, Wd = plan.src.height, plan.src.width, plan.dst.height, plan.dst.width
    if form == "nv12":
        return tn.Layout(h, w, S, **(src_kw or {})), tn.Layout(Hd, Wd, S, **(dst_kw or {}))
    return tp.Layout(h, w, S, form, **(src_kw or {})), tp.Layout(Hd, Wd, S, form, **(dst_kw or {}))


def run(form, plan, mats, frames, fill=None, src_kw=None, dst_kw=None, dst_off=0):
    """ONE bilinear launch of packed frames laid out as src_kw / dst_kw say (the keywords of the nearest tests' Layout classes), the
    destination dst_off bytes into its guarded buffer -> packed frames.  Guards, the offset bytes and every padding byte keep their
    sentinel (run_track of tests/test_hip_track_nv12.py and tests/test_hip_track_planar.py, for the bilinear entry points)."""
    n, dt = len(frames), frames.dtype
    S = dt.itemsize
    sl, dl = layouts(form, plan, S, src_kw, dst_kw)
    src = torch.from_numpy(sl.scatter(frames, seed=1)).cuda()
    table = torch.from_numpy(np.ascontiguousarray(mats)).cuda()
    nbytes = (n - 1) * dl.stride + dl.span
    buf = torch.full((nbytes + dst_off + 2 * GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
    rc = call(form, plan, table.data_ptr(), mats.shape[1], src.data_ptr(), buf.data_ptr() + GUARD + dst_off, n, S, sl.arg, dl.arg, fill)
    assert rc == 0, nat.load().pb_last_error()
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert (got[: GUARD + dst_off] == SENTINEL).all() and (got[GUARD + dst_off + nbytes :] == SENTINEL).all(), "the launch wrote outside its frames"
    out, padding = dl.gather(got[GUARD + dst_off :], n, dt)
    assert (padding == SENTINEL).all(), "the launch wrote into the padding between rows, planes or frames"
    return out


def assert_same(got, want, what=""):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    bad = int((got != want).sum())
    assert bad == 0, f"{what}: {bad} of {got.size} samples differ, by up to {int(np.abs(got.astype(np.int64) - want.astype(np.int64)).max())}"


def plan_of(dst, src, n_rot, **kw):
    dstp, srcp = projections(dst, src)
    return nat.Plan(dstp, list(mats_of(PLAN_DEGREES[:n_rot])) if n_rot else [], srcp, **(kw or dict(defer=True)))


# ---- 1. against the definition ----------------------------------------------------------------------------------------------------------
SHAPES = {"half_quad": HALF_QUAD, "camera_rim": CAMERA_RIM, "odd_444": ODD, "chroma_1x1_2x2": ONE_CHROMA_SAMPLE[0], "chroma_1x1_4x6": ONE_CHROMA_SAMPLE[1]}


def test_the_shapes_reach_what_they_are_for():
    assert DEGREES[0] == (0, 0, 0) and DEGREES[1] == (-90, 0, 0)  # the identity and the pole-crossing pitch are among the rotations
    assert F + 1 == 5 and HALF_QUAD[0][2] % 4 == 2
    assert forms_of(*HALF_QUAD) == list(FORMS) == forms_of(*CAMERA_RIM) and forms_of(*ODD) == ["444"]
    for dst, src in ONE_CHROMA_SAMPLE:
        assert forms_of(dst, src) == list(FORMS) and (src[1] >> 1, src[2] >> 1) == (1, 1)


@pytest.mark.parametrize("k,n_rot", [(1, 0), (2, 0), (1, 1), (2, 1)])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_five_frames_in_one_launch_equal_the_definition(shape, k, n_rot):
    dst, src = SHAPES[shape]
    n = F + 1  # the last chunk is short
    forms = forms_of(dst, src) if not shape.startswith("chroma") else ["420", "nv12"]
    _, h, w, *_ = src
    coords = chain_coords(dst, src, n, k, n_rot)
    if shape == "camera_rim":  # blocks whose anchor is dead beside live pixels, and the reverse: an "any pixel decides" kernel cannot pass
        dead_anchor = live_anchor = 0
        for _, _, live, _ in coords:
            blocks = live.reshape(dst[1] // 2, 2, dst[2] // 2, 2).transpose(0, 2, 1, 3).reshape(-1, 4)
            mixed = blocks.any(axis=1) & ~blocks.all(axis=1)
            dead_anchor, live_anchor = dead_anchor + int((mixed & ~blocks[:, 0]).sum()), live_anchor + int((mixed & blocks[:, 0]).sum())
        assert dead_anchor >= 1 and live_anchor >= 1, (dead_anchor, live_anchor)
    plan = plan_of(dst, src, n_rot)
    mats = track_mats(n, k)
    for form in forms:
        for S, dt in SAMPLES:
            frames = random_frames(form, n, h, w, dt, seed=100 + S)
            for fill in (None, (1, 2, 3)):
                want = expected(form, coords, frames, h, w, fill)
                fills = planar_ref.default_fill(dt) if fill is None else fill
                assert bool((want.reshape(n, -1)[:, : dst[1] * dst[2]] != fills[0]).any()), "the expectation is all fill: the test shows nothing"
                assert_same(run(form, plan, mats, frames, fill), want, f"{shape} {form} S={S} fill={fill} k={k} n_rot={n_rot}")


# ---- 2. a pin that needs no host math: the device's own float64 map and its per-pixel bilinear sampler ----------------------------------
@pytest.mark.parametrize("shape", ["half_quad", "camera_rim"])
def test_every_plane_equals_pb_sample_map_bilinear_px_on_the_device_s_float64_map_of_the_chain(shape):
    dst, src = SHAPES[shape]
    n, k, n_rot = F + 1, 2, 1
    _, h, w, *_ = src
    Hd, Wd = dst[1], dst[2]
    dstp, srcp = projections(dst, src)
    plan_mats = list(mats_of(PLAN_DEGREES[:n_rot]))
    plan = nat.Plan(dstp, plan_mats, srcp, defer=True)
    mats = track_mats(n, k)
    maps = []
    for f in range(n):
        cmap = nat.coordmap(dstp)  # pb_coordmap_f64, then one pb_rotate_f64 per rotation of the whole chain
        for m in plan_mats + list(mats[f]):
            cmap = nat.rotate(m, cmap)
        maps.append(cmap)

    def sampled(plane, f, dt):
        img = torch.from_numpy(np.ascontiguousarray(plane).reshape(h, w, 1)).cuda()
        out = nat.sample_map_bilinear(srcp, maps[f].clone(), img, 1, dt)  # (a panorama source's call zeroes invalid entries of its map)
        torch.cuda.synchronize()
        return out.cpu().numpy().reshape(Hd, Wd)

    for S, dt in SAMPLES:
        for form in ("444", "nv12"):
            frames = random_frames(form, n, h, w, dt, seed=200 + S)
            got = run(form, plan, mats, frames, (0, 0, 0))
            for f in range(n):
                if form == "nv12":
                    assert np.array_equal(got[f, :Hd], sampled(frames[f, :h], f, dt)), (shape, S, f)
                else:
                    for p, (g, s) in enumerate(zip(planar_ref.planes(got[f], Hd, Wd, form), planar_ref.planes(frames[f], h, w, form))):
                        assert np.array_equal(g, sampled(s, f, dt)), (shape, S, f, p)


# ---- 3. against the RGB8 track ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["half_quad", "camera_rim"])
def test_the_three_planes_of_a_yuv444p_uint8_frame_equal_the_three_channels_of_the_rgb8_bilinear_track(shape):
    dst, src = SHAPES[shape]
    n, k = F + 1, 1
    _, h, w, *_ = src
    Hd, Wd = dst[1], dst[2]
    plan = plan_of(dst, src, 1)
    mats = track_mats(n, k)
    frames = random_frames("444", n, h, w, np.uint8, seed=300)
    got = run("444", plan, mats, frames, (0, 0, 0)).reshape(n, 3, Hd, Wd)
    rgb = torch.from_numpy(np.ascontiguousarray(frames.reshape(n, 3, h, w).transpose(0, 2, 3, 1))).cuda()
    table = torch.from_numpy(np.ascontiguousarray(mats)).cuda()
    out = torch.zeros((n, Hd, Wd, 3), dtype=torch.uint8, device="cuda")
    assert nat.load().pb_remap_track_u8(plan.handle, table.data_ptr(), k, nat.TRACK_INTERP_IDS["bilinear"], rgb.data_ptr(), out.data_ptr(), n, 0, 0, nat.current_stream()) == 0
    torch.cuda.synchronize()
    assert_same(got, np.ascontiguousarray(out.cpu().numpy().transpose(0, 3, 1, 2)), f"{shape} against pb_remap_track_u8")


# ---- 4. against each other ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["half_quad", "camera_rim", "chroma_1x1_4x6"])
def test_nv12_equals_the_420_planar_result_interleaved(shape):
    dst, src = SHAPES[shape]
    n = F + 1
    _, h, w, *_ = src
    Hd, Wd = dst[1], dst[2]
    plan = plan_of(dst, src, 1)
    mats = track_mats(n, 1)
    for S, dt in SAMPLES:
        flat = random_frames("420", n, h, w, dt, seed=400 + S)
        semi = np.stack([np.concatenate([p0, np.stack([p1, p2], axis=2).reshape(h // 2, w)], axis=0) for p0, p1, p2 in (planar_ref.planes(fr, h, w, "420") for fr in flat)])
        for fill in (None, (1, 2, 3)):
            a, b = run("420", plan, mats, flat, fill), run("nv12", plan, mats, semi, fill)
            for f in range(n):
                p0, p1, p2 = planar_ref.planes(a[f], Hd, Wd, "420")
                uv = b[f, Hd:].reshape(Hd // 2, Wd // 2, 2)
                assert np.array_equal(b[f, :Hd], p0) and np.array_equal(uv[..., 0], p1) and np.array_equal(uv[..., 1], p2), (shape, S, fill, f)


# ---- 5. layouts ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
def test_pitches_gaps_swapped_chroma_frame_strides_and_a_destination_off_a_wide_store(form):
    dst, src = HALF_QUAD
    n = F + 1
    plan = plan_of(dst, src, 0)
    mats = track_mats(n, 1)
    for S, dt in SAMPLES:
        frames = random_frames(form, n, 16, 32, dt, seed=500 + S)
        want = run(form, plan, mats, frames)  # the packed launch's bytes
        assert_same(want, expected(form, chain_coords(dst, src, n, 1, 0), frames, 16, 32), f"packed {form} S={S}")
        if form == "nv12":
            cases = {name: (skw(16, 32), dkw(34, 30), off) for name, (skw, dkw, off) in tn._layouts(S).items()}
        else:
            pitched = dict(pitch_pad=6 * S, cpitch_pad=3 * S, gap1=5 * S, gap2=S, stride_pad=7 * S)
            cases = {"pitched": (pitched, pitched, 0), "padded_frame_stride": (dict(stride_pad=2 * S), dict(stride_pad=14 * S), 0),
                     "one_sample_off": (None, None, S), "three_samples_off_pitched": (pitched, pitched, 3 * S)}
        for name, (skw, dkw, off) in cases.items():
            assert_same(run(form, plan, mats, frames, None, skw, dkw, off), want, f"{name} {form} S={S}")
        if form != "nv12":  # planes 1 and 2 in the other order (YV12's) in both frames: the chroma offsets swapped.  The default fills of
            # planes 1 and 2 are equal, so each plane of the buffers is remapped in its place: the packed launch's bytes
            sl, dl = layouts(form, plan, S, None, None)
            swap = lambda l: (l.pitch, l.cpitch, l.o2, l.o1, l.stride)  # noqa: E731
            assert planar_ref.default_fill(dt)[1] == planar_ref.default_fill(dt)[2] and sl.o1 != sl.o2
            src_t = torch.from_numpy(np.ascontiguousarray(frames)).cuda()
            table = torch.from_numpy(np.ascontiguousarray(mats)).cuda()
            out = torch.full((n * dl.stride + 2 * GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
            assert call(form, plan, table.data_ptr(), 1, src_t.data_ptr(), out.data_ptr() + GUARD, n, S, swap(sl), swap(dl)) == 0, nat.load().pb_last_error()
            torch.cuda.synchronize()
            o = out.cpu().numpy()
            assert (o[:GUARD] == SENTINEL).all() and (o[GUARD + n * dl.stride :] == SENTINEL).all()
            assert_same(o[GUARD : GUARD + n * dl.stride].view(dt).reshape(n, -1), want, f"swapped chroma offsets {form} S={S}")


# ---- 6. plan states -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["420", "nv12"])
def test_deferred_prepared_tableless_and_faithful_plans_give_identical_bytes(form):
    dst, src = HALF_QUAD
    n = 3
    mats = track_mats(n, 1)
    faithful = plan_of(dst, src, 1, bilinear=True)
    faithful.set_mode(nat.MODE_FAITHFUL)
    states = {"deferred": plan_of(dst, src, 1, defer=True), "prepared with the bilinear tables": plan_of(dst, src, 1, bilinear=True),
              "prepared without them": plan_of(dst, src, 1, bilinear=False), "faithful": faithful}
    coords = chain_coords(dst, src, n, 1, 1)
    for S, dt in SAMPLES:
        frames = random_frames(form, n, 16, 32, dt, seed=600 + S)
        want = expected(form, coords, frames, 16, 32)
        for what, plan in states.items():
            assert_same(run(form, plan, mats, frames), want, f"{what} {form} S={S}")


# ---- 7. a captured launch -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,dt", SAMPLES)
@pytest.mark.parametrize("form", ["420", "nv12"])
def test_a_captured_launch_replayed_once_gives_the_plain_launch_s_bytes(form, S, dt):
    """never allocates, never synchronises, never copies the table: ONE kernel node, a linear capture on one stream"""
    dst, src = HALF_QUAD
    n = F + 1
    plan = plan_of(dst, src, 0)
    mats, frames = track_mats(n, 1), random_frames(form, n, 16, 32, dt, seed=700 + S)
    want = run(form, plan, mats, frames)
    table, src_t = torch.from_numpy(mats).cuda(), torch.from_numpy(frames).cuda()
    out = torch.zeros(want.shape, dtype=nat.torch_dtype(dt), device="cuda")
    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            assert call(form, plan, table.data_ptr(), 1, src_t.data_ptr(), out.data_ptr(), n, S) == 0  # (the current stream: the capturing one)
    torch.cuda.current_stream().wait_stream(side)
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), want)


# ---- 8. the Python methods ----------------------------------------------------------------------------------------------------------------
def test_the_plan_methods_return_the_c_call_s_bytes_with_the_host_s_dtype():
    dst, src = HALF_QUAD
    n = F + 1
    plan = plan_of(dst, src, 1)
    for S, dt in SAMPLES:
        for k in (1, 2):
            mats = track_mats(n, k)
            for form in FORMS:
                frames = random_frames(form, n, 16, 32, dt, seed=800 + S)
                src_t = torch.from_numpy(frames).cuda()
                want = run(form, plan, mats, frames, (1, 2, 3))
                rot = mats if k == 2 else mats[:, 0]
                if form == "nv12":
                    got = plan.remap_track_nv12(src_t, rot, fill=(1, 2, 3), interpolation="bilinear")
                    nearest = plan.remap_track_nv12(src_t, rot, fill=(1, 2, 3))
                else:
                    got = plan.remap_track_planar(src_t, rot, form, fill=(1, 2, 3), interpolation="bilinear")
                    nearest = plan.remap_track_planar(src_t, rot, form, fill=(1, 2, 3))
                assert isinstance(got, torch.Tensor) and got.is_cuda and got.dtype == nat.torch_dtype(dt) and np.array_equal(got.cpu().numpy(), want), (form, S, k)
                assert not np.array_equal(nearest.cpu().numpy(), want), "the default samples nearest"
        with pytest.raises(ValueError, match="the table holds"):
            plan.remap_track_nv12(torch.from_numpy(random_frames("nv12", n, 16, 32, dt, seed=1)).cuda(), track_mats(n - 1, 1), interpolation="bilinear")
        with pytest.raises(ValueError, match="the table holds"):
            plan.remap_track_planar(torch.from_numpy(random_frames("420", n, 16, 32, dt, seed=1)).cuda(), track_mats(n - 1, 1), "420", interpolation="bilinear")


# ---- 9. the refusals ----------------------------------------------------------------------------------------------------------------------
def test_double_fisheye_cube_and_equi_angular_cube_sources_are_refused_and_nothing_is_written():
    L = nat.load()
    dst = pano(20, 40)
    double = [c for c in tp.GOLDEN.values() if c.name == "T_double_195"][0].src
    sources = {"double": (double, b"single sources"), "cube": (cube(12), b"panorama and camera sources"), "eac": (eac(12), b"panorama and camera sources")}
    table = torch.from_numpy(track_mats(1, 1)).cuda()
    for what, (src, message) in sources.items():
        dstp, srcp = projections(dst, src)
        plan = nat.Plan(dstp, [], srcp, defer=True)
        src_t = torch.zeros(3 * src[1] * src[2] * 2, dtype=torch.uint8, device="cuda")
        buf = torch.full((3 * dst[1] * dst[2] * 2,), SENTINEL, dtype=torch.uint8, device="cuda")
        for form in FORMS:
            for S, _ in SAMPLES:
                assert call(form, plan, table.data_ptr(), 1, src_t.data_ptr(), buf.data_ptr(), 1, S) == UNSUPPORTED, (what, form, S)
                name = b"pb_remap_track_nv12_bilinear" if form == "nv12" else b"pb_remap_track_planar_bilinear"
                assert L.pb_last_error().startswith(name) and message in L.pb_last_error(), (what, form, L.pb_last_error())
        torch.cuda.synchronize()
        assert bool((buf == SENTINEL).all()), what
