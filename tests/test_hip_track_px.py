"""pb_remap_track_px: a rotation per frame in one launch for grey, RGBA and 16-bit frames.  The yardstick of every test is
the EXISTING materialised-map route, frame by frame: pb_coordmap_f64, pb_rotate_f64 by the plan's rotations and then the frame's, then
pb_index_from_map_i32 + pb_gather_px (a double fisheye: pb_gather_blend_u8) for nearest, pb_sample_map_bilinear_px /
pb_sample_map_catmull_rom_px for the interpolating modes.  Every comparison is byte equality, and the expected frames are never all
black.  Frames are independent random samples (a wrong index or a swapped byte shows); destinations sit between sentinel bytes.  Shapes
are tests/test_hip_rotation_track.py's: partial last quads, rows that start off a dword, more than one workgroup, frame counts around
the kernel's chunk of PB_TRACK_FRAMES frames."""

import os

import numpy as np
import pytest
import torch

from oracle import reference_path as orc
from photonbend_amd import _native as nat
from tests import eac_cases as ec
from tests import helpers as H
from tests import rotation_track_cases as rc
from tests.cases import Case, cam, dbl, inscribed, pano
from tests.test_hip_rotation_track import PLAN_DEGREES, mats_of, track_mats

pytestmark = pytest.mark.gpu

F = 4  # PB_TRACK_FRAMES (csrc/pb_kernels_track.hpp): frames a work-item loops over
GUARD = 64
SENTINEL = 0xA5
UNSUPPORTED = -3
cube, eac = ec.cube, ec.eac
INTERPOLATIONS = ("nearest", "bilinear", "catmull-rom")

# (channels, sample_bytes) -> the frames' dtype and trailing shape
DTYPES = {1: np.uint8, 2: np.uint16}
ALL_FORMATS = [(1, 1), (1, 2), (2, 1), (4, 1), (3, 2), (4, 2)]
DOUBLE_FORMATS = [(1, 1), (2, 1), (4, 1)]
INTERP_FORMATS = [(1, 1), (4, 1), (3, 2)]
INTERP_DOUBLE_FORMATS = [(1, 1), (4, 1)]

SOURCES = {
    "pano": pano(24, 48),
    "camera": cam(40, 40, "equisolid", 190, inscribed(40)),
    "cube": cube(12),
    "eac": eac(12),
    "double": dbl(24, 48, "equidistant", 195),
}
DESTINATIONS = {
    "pano": pano(20, 40),
    "camera_odd": cam(35, 33, "equidistant", 180),  # 1155 px: a partial last quad; rows of 33 px start off a dword for B = 1, 2, 6
    "cube": cube(14),                               # (28, 42): 1176 px, two workgroups of 256 quads
}


def projections(dst, src):
    s, cmap = ec.pb_chain(Case("track_px", dst, src), image=np.zeros((src[1], src[2], 3), np.uint8))
    return cmap.dst_proj, s._proj("src")


def random_frames(n, h, w, fmt, seed):
    ch, sb = fmt
    dt = DTYPES[sb]
    return np.random.default_rng(seed).integers(0, np.iinfo(dt).max + 1, (n, h, w) + ((ch,) if ch > 1 else ()), dtype=dt)


_MAPS = {}  # the rotated float64 map of (dst, chain) on the device, computed once and shared (its consumers leave it as it is)


def frame_map(dstp, key, chain):
    k = (key, tuple(np.asarray(m, np.float64).tobytes() for m in chain))
    if k not in _MAPS:
        cmap = nat.coordmap(dstp)
        for m in chain:
            cmap = nat.rotate(np.asarray(m, np.float64), cmap)
        _MAPS[k] = cmap
    return _MAPS[k]


def expected(dstp, srcp, key, plan_mats, mats, frames, fmt, interpolation="nearest"):
    """Frame f through the existing map-stage calls: the yardstick."""
    ch, sb = fmt
    n = len(frames)
    Hd, Wd = dstp.height, dstp.width
    out_dt = np.uint8 if srcp.kind == nat.KIND_DOUBLE else DTYPES[sb]
    out = np.empty((n, Hd, Wd) + ((ch,) if ch > 1 else ()), out_dt)
    for f in range(n):
        cmap = frame_map(dstp, key, list(plan_mats) + list(mats[f]))
        img = torch.from_numpy(np.ascontiguousarray(frames[f])).cuda()
        if interpolation != "nearest":
            got = nat.sample_map_interp(interpolation, srcp, cmap, img, ch, DTYPES[sb])
        else:
            idx, w = nat.index_from_map(srcp, cmap)
            if srcp.kind == nat.KIND_DOUBLE:
                got = nat.gather_blend(idx, w, img, ch, sb)
            else:
                got = nat.gather_px(idx, img.view(torch.uint8).reshape(frames.shape[1], frames.shape[2], ch * sb))
        torch.cuda.synchronize()
        out[f] = got.cpu().numpy().reshape(-1).view(out_dt).reshape(out.shape[1:])
    return out


def track_call(plan, table, k, interpolation, src_ptr, dst_ptr, n, fmt, ss=0, ds=0, stream=None):
    return nat.load().pb_remap_track_px(plan.handle, table.data_ptr(), k, nat.TRACK_INTERP_IDS[interpolation], src_ptr, dst_ptr, n, ss, ds, fmt[0], fmt[1],
                                        nat.current_stream() if stream is None else stream)


def run_track(plan, mats, frames, fmt, interpolation="nearest", src_pad=0, dst_pad=0, dst_off=0, stream=None):
    """One pb_remap_track_px launch; frames at strides of a frame + pad bytes, the destination dst_off bytes into its guarded buffer.
    Guards, the offset bytes and the padding between destination frames must keep their sentinel."""
    n = frames.shape[0]
    B = fmt[0] * fmt[1]
    Hd, Wd = plan.dst.height, plan.dst.width
    sb, db = frames[0].nbytes, Hd * Wd * B
    ss, ds = sb + src_pad, db + dst_pad
    host = np.random.default_rng(1).integers(0, 256, n * ss, dtype=np.uint8)  # (random bytes in the source padding too)
    for f in range(n):
        host[f * ss : f * ss + sb] = np.ascontiguousarray(frames[f]).reshape(-1).view(np.uint8)
    src = torch.from_numpy(host).cuda()
    table = torch.from_numpy(np.ascontiguousarray(mats)).cuda()
    buf = torch.full((n * ds + dst_off + 2 * GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    rc_ = track_call(plan, table, mats.shape[1], interpolation, src.data_ptr(), buf.data_ptr() + GUARD + dst_off, n, fmt, ss if src_pad else 0, ds if dst_pad else 0,
                     stream)
    assert rc_ == 0, nat.load().pb_last_error()
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert (got[: GUARD + dst_off] == SENTINEL).all() and (got[GUARD + dst_off + n * ds :] == SENTINEL).all(), "the launch wrote outside its frames"
    body = got[GUARD + dst_off : GUARD + dst_off + n * ds].reshape(n, ds)
    assert (body[:, db:] == SENTINEL).all(), "the launch wrote into the padding between destination frames"
    dt = DTYPES[fmt[1]]
    return np.ascontiguousarray(body[:, :db]).view(dt).reshape((n, Hd, Wd) + ((fmt[0],) if fmt[0] > 1 else ()))


def n_diff(got, want):
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    d = got != want
    return int((d.any(axis=-1) if d.ndim == 4 else d).sum())


def check(d, s, fmt, n=3, k=1, n_rot=0, interpolation="nearest", seed=0, **layout):
    dst = DESTINATIONS.get(d, d)
    src = SOURCES.get(s, s)
    dstp, srcp = projections(dst, src)
    plan_mats = list(mats_of(PLAN_DEGREES[:n_rot])) if n_rot else []
    mats = track_mats(n, k)
    frames = random_frames(n, src[1], src[2], fmt, seed)
    plan = nat.Plan(dstp, plan_mats, srcp, defer=True)
    got = run_track(plan, mats, frames, fmt, interpolation, **layout)
    want = expected(dstp, srcp, (d, s) if isinstance(d, str) else repr((dst, src)), plan_mats, mats, frames, fmt, interpolation)
    bad = n_diff(got, want)
    assert bad == 0, f"{bad} of {want.shape[0] * want.shape[1] * want.shape[2]} pixels differ from the map-stage calls ({fmt}, {interpolation})"
    assert want.any(), "the geometry samples nothing: a test of black frames shows nothing"
    return got


# ---- 1. nearest: every source kind x {panorama, odd camera, cube} destination x every format ------------------------------------------
KINDS = [(s, d) for s in SOURCES for d in DESTINATIONS]


@pytest.mark.parametrize("s,d", KINDS, ids=[f"{s}_to_{d}" for s, d in KINDS])
def test_nearest_from_every_source_kind_into_every_destination_kind_in_every_format(s, d):
    """five frames cross a chunk of F = 4"""
    for fmt in (DOUBLE_FORMATS if s == "double" else ALL_FORMATS):
        check(d, s, fmt, n=F + 1, k=1, n_rot=0, seed=10 + fmt[0] * fmt[1])


# ---- 2. the three interpolations ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", list(SOURCES))
@pytest.mark.parametrize("interpolation", INTERPOLATIONS)
def test_the_three_interpolations_on_every_source_kind(s, interpolation):
    for fmt in (INTERP_DOUBLE_FORMATS if s == "double" else INTERP_FORMATS):
        check("camera_odd", s, fmt, n=F + 1, k=1, n_rot=1, seed=20 + fmt[0], interpolation=interpolation)
        if interpolation != "catmull-rom":  # (the cubic on one destination only: the suite stays short)
            check("pano", s, fmt, n=2, k=2, seed=21 + fmt[0], interpolation=interpolation)


# ---- 3. the real reference --------------------------------------------------------------------------------------------------------------
GOLD = np.load(os.path.join(H.GOLD, "rotation_track.npz"))


@pytest.mark.parametrize("case", rc.golden_cases(), ids=lambda c: c.name)
def test_the_nearest_track_is_the_reference_s_output_whatever_the_pixel_holds(case):
    """tests/golden/rotation_track.npz, six cases x four frames: an RGBA8 frame whose RGB is the case's frame gives the reference's RGB in
    its first three channels; for single sources grey16 and RGBA16 random frames are np.where(idx < 0, 0, flat[idx]) with the reference's
    own index map.  No tolerance on the goldens' platform; elsewhere the library of this host's flavour keeps the fragile-set allowance."""
    dstp, srcp = projections(case.dst, case.src)
    plan = nat.Plan(dstp, list(mats_of(case.plan_rot)) if case.plan_rot else [], srcp, defer=True)
    n, k = len(case.frames), len(case.frames[0])
    mats = mats_of([r for fr in case.frames for r in fr]).reshape(n, k, 3, 3)
    rgb = rc.case_frames(case)
    rng = np.random.default_rng(120)
    rgba = np.concatenate([rgb, rng.integers(0, 256, rgb.shape[:3] + (1,), dtype=np.uint8)], axis=3)
    got = run_track(plan, mats, rgba, (4, 1))
    exact = H.live_numpy_is_the_goldens_numpy()
    fragile = []
    for f in range(n):
        rots = [tuple(map(orc.to_radians, r)) for r in case.chain(f)]
        with np.errstate(all="ignore"):
            fragile.append(np.zeros(got.shape[1:3], bool) if exact else orc.fragile_mask(orc.pretrunc(H.orc_proj(case.dst), H.orc_proj(case.src), rots)))
        want = GOLD[f"{case.name}/{f}/u8"]
        assert want.any()
        bad = (got[f][..., :3] != want).any(axis=2)
        assert int((bad & ~fragile[f]).sum()) == 0, (case.name, f, int(bad.sum()))
    if case.src[0] == "double":
        return
    for fmt in ((1, 2), (4, 2)):
        frames = random_frames(n, case.src[1], case.src[2], fmt, 121 + fmt[0])
        got = run_track(plan, mats, frames, fmt)
        for f in range(n):
            idx = GOLD[f"{case.name}/{f}/idx"]
            flat = frames[f].reshape((-1,) + frames.shape[3:])
            want = flat[np.where(idx < 0, 0, idx)]
            want[idx < 0] = 0
            assert want.any()
            d = got[f] != want
            bad = d.any(axis=-1) if d.ndim == 3 else d
            assert int((bad & ~fragile[f]).sum()) == 0, (case.name, fmt, f, int(bad.sum()))


# ---- 4. three one-byte channels are pb_remap_track_u8 -----------------------------------------------------------------------------------
@pytest.mark.parametrize("interpolation", INTERPOLATIONS)
def test_three_one_byte_channels_write_pb_remap_track_u8_s_bytes(interpolation):
    for s in ("pano", "double"):
        src = SOURCES[s]
        dstp, srcp = projections(DESTINATIONS["camera_odd"], src)
        plan = nat.Plan(dstp, list(mats_of(PLAN_DEGREES[:1])), srcp, defer=True)
        n = F + 1
        mats, frames = track_mats(n, 1), random_frames(n, src[1], src[2], (3, 1), 40)
        got = run_track(plan, mats, frames, (3, 1), interpolation, dst_off=1)
        table, src_t = torch.from_numpy(mats).cuda(), torch.from_numpy(frames).cuda()
        want = torch.zeros((n, 35, 33, 3), dtype=torch.uint8, device="cuda")
        assert nat.load().pb_remap_track_u8(plan.handle, table.data_ptr(), 1, nat.TRACK_INTERP_IDS[interpolation], src_t.data_ptr(), want.data_ptr(), n, 0, 0,
                                            nat.current_stream()) == 0
        torch.cuda.synchronize()
        assert n_diff(got, want.cpu().numpy()) == 0 and bool(want.any()), (s, interpolation)


# ---- 5. layouts -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", [(1, 1), (1, 2), (3, 2), (4, 1)], ids=lambda v: f"{v[0]}x{v[1]}")
def test_padded_strides_and_destinations_off_a_dword_boundary(fmt):
    """strides that are multiples of A = min(4, B & -B); the destination A and 2 A bytes into its buffer (B = 1, 2, 6: off a dword, the
    stores go in units of A); random bytes in the source padding; sentinels before, after and between the frames"""
    A = nat.px_align(fmt[0] * fmt[1])
    for layout in (dict(src_pad=5 * A), dict(dst_pad=A), dict(src_pad=12 * A, dst_pad=3 * A), dict(dst_off=A), dict(dst_off=2 * A, dst_pad=A, src_pad=A)):
        for interpolation in ("nearest", "bilinear"):
            check("camera_odd", pano(16, 32), fmt, n=F + 1, k=1, seed=50, interpolation=interpolation, **layout)
    if fmt[1] == 1:
        for layout in (dict(src_pad=3 * A, dst_pad=A), dict(dst_off=A, dst_pad=2 * A)):
            for interpolation in ("nearest", "bilinear"):
                check("pano", "double", fmt, n=3, seed=51, interpolation=interpolation, **layout)


def test_a_misaligned_frame_is_refused_and_nothing_is_written():
    dstp, srcp = projections(DESTINATIONS["pano"], SOURCES["pano"])
    plan = nat.Plan(dstp, [], srcp, defer=True)
    table = torch.from_numpy(track_mats(1, 1)).cuda()
    src = torch.zeros(24 * 48 * 8 + 8, dtype=torch.uint8, device="cuda")
    buf = torch.full((20 * 40 * 8 + 2 * GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
    for fmt in ((1, 2), (4, 1), (3, 2), (4, 2)):
        a = nat.px_align(fmt[0] * fmt[1])
        assert track_call(plan, table, 1, "nearest", src.data_ptr(), buf.data_ptr() + GUARD + a // 2, 1, fmt) == -1
        assert b"multiples of" in nat.load().pb_last_error()
    torch.cuda.synchronize()
    assert bool((buf == SENTINEL).all())


# ---- 6. frame counts and rotation counts ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, F + 1, 2 * F + 1])
@pytest.mark.parametrize("k,n_rot", [(1, 0), (2, 0), (1, 1), (2, 1)])
def test_frame_counts_and_rotation_counts(n, k, n_rot):
    check("camera_odd", pano(16, 32), (3, 2), n=n, k=k, n_rot=n_rot, seed=60 + n)
    check("cube", pano(16, 32), (1, 1), n=n, k=k, n_rot=n_rot, seed=61 + n, interpolation="bilinear")


# ---- 7. every plan state is served alike ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", ["pano", "double"])
def test_deferred_prepared_and_faithful_plans_give_identical_bytes(s):
    src = SOURCES[s]
    dstp, srcp = projections(DESTINATIONS["camera_odd"], src)
    plan_mats = list(mats_of(PLAN_DEGREES[:1]))
    fmt = (4, 1)
    mats, frames = track_mats(3, 1), random_frames(3, src[1], src[2], fmt, 70)
    for interpolation in INTERPOLATIONS:
        want = expected(dstp, srcp, ("camera_odd", s), plan_mats, mats, frames, fmt, interpolation)
        assert want.any()
        faithful = nat.Plan(dstp, plan_mats, srcp, bilinear=True)
        faithful.set_mode(nat.MODE_FAITHFUL)
        states = {"deferred": nat.Plan(dstp, plan_mats, srcp, defer=True), "prepared": nat.Plan(dstp, plan_mats, srcp, bilinear=True), "faithful": faithful}
        for what, plan in states.items():
            assert n_diff(run_track(plan, mats, frames, fmt, interpolation), want) == 0, (what, interpolation)


def test_a_double_fisheye_with_16_bit_samples_is_unsupported_and_nothing_is_written():
    src = SOURCES["double"]
    dstp, srcp = projections(DESTINATIONS["pano"], src)
    plan = nat.Plan(dstp, [], srcp)
    assert plan.track_px_supported(4, 1) and not plan.track_px_supported(1, 2)
    table = torch.from_numpy(track_mats(1, 1)).cuda()
    frames = torch.from_numpy(random_frames(1, src[1], src[2], (1, 2), 71)).cuda()
    buf = torch.full((20 * 40 * 2 + 2 * GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
    for interpolation in INTERPOLATIONS:
        assert track_call(plan, table, 1, interpolation, frames.data_ptr(), buf.data_ptr() + GUARD, 1, (1, 2)) == UNSUPPORTED
        assert b"pb_gather_blend_u8" in nat.load().pb_last_error()
    torch.cuda.synchronize()
    assert bool((buf == SENTINEL).all())


# ---- 8. graph capture -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("interpolation", ["nearest", "bilinear"])
def test_a_captured_launch_replayed_once_gives_the_same_bytes(interpolation):
    """never allocates, never synchronises, never copies the table: ONE kernel node, captured on one stream, no parallel branches"""
    fmt = (3, 2)
    dstp, srcp = projections(DESTINATIONS["camera_odd"], pano(16, 32))
    n = F + 1
    mats, frames = track_mats(n, 1), random_frames(n, 16, 32, fmt, 80)
    plan = nat.Plan(dstp, [], srcp, defer=True)
    want = run_track(plan, mats, frames, fmt, interpolation)
    table, src_t = torch.from_numpy(mats).cuda(), torch.from_numpy(frames).cuda()
    out = torch.zeros((n, 35, 33, 3), dtype=torch.uint16, device="cuda")
    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            assert track_call(plan, table, 1, interpolation, src_t.data_ptr(), out.data_ptr(), n, fmt) == 0  # (the current stream: the capturing one)
    torch.cuda.current_stream().wait_stream(side)
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert n_diff(out.cpu().numpy(), want) == 0 and want.any()


# ---- 9. a second stream -----------------------------------------------------------------------------------------------------------------
def test_a_launch_on_a_second_stream_gives_the_default_stream_s_bytes():
    fmt = (4, 1)
    dstp, srcp = projections(DESTINATIONS["camera_odd"], SOURCES["camera"])
    mats, frames = track_mats(F + 1, 1), random_frames(F + 1, 40, 40, fmt, 90)
    plan = nat.Plan(dstp, [], srcp, defer=True)
    for interpolation in ("nearest", "catmull-rom"):
        want = run_track(plan, mats, frames, fmt, interpolation)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        got = run_track(plan, mats, frames, fmt, interpolation, stream=int(side.cuda_stream))
        assert n_diff(got, want) == 0 and want.any(), interpolation


# ---- 10. the facade ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", [(1, 2), (4, 1)], ids=lambda v: f"{v[0]}x{v[1]}")
def test_plan_remap_track_px_returns_the_c_call_s_bytes(fmt):
    dstp, srcp = projections(DESTINATIONS["camera_odd"], pano(16, 32))
    n = F + 2
    frames = random_frames(n, 16, 32, fmt, 100)
    plan = nat.Plan(dstp, list(mats_of(PLAN_DEGREES[:1])), srcp, defer=True)
    for k in (1, 2):
        mats = track_mats(n, k)
        for interpolation in INTERPOLATIONS:
            want = run_track(plan, mats, frames, fmt, interpolation)
            src_t = torch.from_numpy(frames).cuda()
            got = plan.remap_track_px(src_t, mats if k == 2 else mats[:, 0], interpolation=interpolation)  # an uploaded table
            assert isinstance(got, torch.Tensor) and got.is_cuda and got.dtype == src_t.dtype
            torch.cuda.synchronize()
            assert n_diff(got.cpu().numpy(), want) == 0 and want.any(), (k, interpolation)
            out = torch.zeros_like(got)
            assert plan.remap_track_px(src_t, torch.from_numpy(mats).cuda(), out=out, interpolation=interpolation) is out  # a device table, in place
            torch.cuda.synchronize()
            assert n_diff(out.cpu().numpy(), want) == 0, (k, interpolation)
    # nearest never looks inside a pixel: float32 grey frames travel as four bytes
    f32 = np.random.default_rng(101).standard_normal((n, 16, 32)).astype(np.float32)
    mats = track_mats(n, 1)
    want = run_track(plan, mats, f32.view(np.uint8).reshape(n, 16, 32, 4), (4, 1))
    got = plan.remap_track_px(torch.from_numpy(f32).cuda(), mats)
    torch.cuda.synchronize()
    assert got.dtype == torch.float32 and np.array_equal(got.cpu().numpy().view(np.uint8).reshape(want.shape), want) and want.any()
