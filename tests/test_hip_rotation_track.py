"""pb_remap_track_u8: a rotation per frame in one launch.  Frame f must be, byte for byte, what the EXISTING entry points
write for frame f alone from a private plan of the full chain - the plan's own rotations, then the frame's - in PB_MODE_FAITHFUL.  Every
comparison is exact equality; frames are independent random bytes (a wrong index shows); destinations sit between sentinel bytes that must
survive.  Shapes are the smallest that still reach each way to go wrong: partial last quads, rows that start off a 4-byte boundary, more
than one workgroup, frame counts around the kernel's chunk of PB_TRACK_FRAMES frames."""

import os

import numpy as np
import pytest
import torch

import photonbend_amd as pb
from oracle import reference_path as orc
from photonbend_amd import batch
from photonbend_amd import _native as nat
from photonbend_amd.core import rotation_track
from tests import cubemap_cases as cc
from tests import helpers as H
from tests import rotation_track_cases as rc
from tests.cases import Case, cam, dbl, inscribed, pano

pytestmark = pytest.mark.gpu

F = 4  # PB_TRACK_FRAMES (csrc/pb_kernels_track.hpp): frames a work-item loops over
GUARD = 64
SENTINEL = 0xA5
INVALID = -1
cube = cc.cube

# per-frame rotations in degrees: the identity, the pole-crossing pitch, then arbitrary ones
DEGREES = [(0, 0, 0), (-90, 0, 0), (30, 45, 10), (-3.5, 170, 12), (77, -120, 200), (1, 2, 3), (-40, 5, 77), (0, 90, 0), (12, 34, 56),
           (180, 0, 0), (0, 0, 45), (-15, 100, 200), (5, -20, 33), (89, 1, -1), (-60, -60, -60), (0.001, 0, 0), (45, 45, 45), (10, 20, 30)]
PLAN_DEGREES = [(3, 90, -7), (20, 30, 40), (-40, 5, 77), (10, 20, 30), (1, -2, 3), (60, 0, 0), (0, -45, 0), (0, 0, 15)]


def mats_of(degrees):
    return rotation_track(np.array([[pb.utils.to_radians(v) for v in d] for d in degrees], dtype=np.float64).reshape(-1, 3))


def track_mats(n, k):
    """(n, k, 3, 3): frame f's k rotations; the identity and the pole-crossing pitch lead."""
    assert n * k <= len(DEGREES)
    return mats_of(DEGREES[: n * k]).reshape(n, k, 3, 3)


def projections(dst, src):
    """tests/cases.py projection tuples (and "cube", and polynomial lens names) -> the facade's pb_proj pair"""
    s, cmap = cc.pb_chain(Case("track", dst, src), image=np.zeros((src[1], src[2], 3), np.uint8))
    return cmap.dst_proj, s._proj("src")


def random_frames(n, h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (n, h, w, 3), dtype=np.uint8)


CALLS = {"nearest": "pb_remap_u8", "bilinear": "pb_remap_bilinear_u8", "catmull-rom": "pb_remap_catmull_rom_u8"}


def expected(dstp, srcp, plan_mats, mats, frames, interpolation="nearest"):
    """Frame f from the existing single-plan entry point: a private plan of the whole chain, PB_MODE_FAITHFUL."""
    L = nat.load()
    out = torch.empty((len(frames), dstp.height, dstp.width, 3), dtype=torch.uint8, device="cuda")
    for f in range(len(frames)):
        plan = nat.Plan(dstp, list(plan_mats) + list(mats[f]), srcp, defer=True, bilinear=True)
        plan.set_mode(nat.MODE_FAITHFUL)
        src = torch.from_numpy(frames[f]).cuda()
        assert getattr(L, CALLS[interpolation])(plan.handle, src.data_ptr(), out[f].data_ptr(), 1, 0, 0, nat.current_stream()) == 0, L.pb_last_error()
        torch.cuda.synchronize()
    return out.cpu().numpy()


def track_call(plan, table, k, interpolation, src_ptr, dst_ptr, n, ss=0, ds=0, stream=None):
    return nat.load().pb_remap_track_u8(plan.handle, table.data_ptr(), k, nat.TRACK_INTERP_IDS[interpolation], src_ptr, dst_ptr, n, ss, ds,
                                        nat.current_stream() if stream is None else stream)


def run_track(plan, mats, frames, interpolation="nearest", src_pad=0, dst_pad=0, dst_off=0):
    """One pb_remap_track_u8 launch; frames at strides of a frame + pad bytes, the destination dst_off bytes into its guarded buffer.
    Guards, the offset bytes and the padding between destination frames must keep their sentinel."""
    n, h, w, _ = frames.shape
    Hd, Wd = plan.dst.height, plan.dst.width
    sb, db = h * w * 3, Hd * Wd * 3
    ss, ds = sb + src_pad, db + dst_pad
    host = np.random.default_rng(1).integers(0, 256, n * ss, dtype=np.uint8)  # (random bytes in the source padding too)
    for f in range(n):
        host[f * ss : f * ss + sb] = frames[f].reshape(-1)
    src = torch.from_numpy(host).cuda()
    table = torch.from_numpy(np.ascontiguousarray(mats)).cuda()
    buf = torch.full((n * ds + dst_off + 2 * GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
    rc_ = track_call(plan, table, mats.shape[1], interpolation, src.data_ptr(), buf.data_ptr() + GUARD + dst_off, n, ss if src_pad else 0, ds if dst_pad else 0)
    assert rc_ == 0, nat.load().pb_last_error()
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert (got[: GUARD + dst_off] == SENTINEL).all() and (got[GUARD + dst_off + n * ds :] == SENTINEL).all(), "the launch wrote outside its frames"
    body = got[GUARD + dst_off : GUARD + dst_off + n * ds].reshape(n, ds)
    assert (body[:, db:] == SENTINEL).all(), "the launch wrote into the padding between destination frames"
    return body[:, :db].reshape(n, Hd, Wd, 3)


def n_diff(got, want):
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape)
    return int((got != want).any(axis=-1).sum())


def check(dst, src, n=3, k=1, n_rot=0, interpolation="nearest", seed=0, **layout):
    dstp, srcp = projections(dst, src)
    plan_mats = list(mats_of(PLAN_DEGREES[:n_rot])) if n_rot else []
    mats = track_mats(n, k)
    frames = random_frames(n, src[1], src[2], seed)
    plan = nat.Plan(dstp, plan_mats, srcp, defer=True)
    got = run_track(plan, mats, frames, interpolation, **layout)
    want = expected(dstp, srcp, plan_mats, mats, frames, interpolation)
    bad = n_diff(got, want)
    assert bad == 0, f"{bad} of {got.shape[0] * got.shape[1] * got.shape[2]} pixels differ from the single-plan calls"
    assert want.any(), "the geometry samples nothing: a test of black frames shows nothing"
    return got


# ---- 1. every source kind x {panorama, camera, cube} destination ------------------------------------------------------------------
SOURCES = {
    "pano": pano(24, 48),
    "camera": cam(40, 40, "equisolid", 190, inscribed(40)),
    "cube": cube(12),
    "double": dbl(24, 48, "equidistant", 195),
}
DESTINATIONS = {
    "pano": pano(20, 40),
    "camera_odd": cam(35, 33, "equidistant", 180),  # 1155 px: a partial last quad; rows start at 99 i bytes, off a 4-byte boundary
    "cube": cube(14),                               # (28, 42): 1176 px, two workgroups of 256 quads
}
KINDS = [(s, d) for s in SOURCES for d in DESTINATIONS]


@pytest.mark.parametrize("s,d", KINDS, ids=[f"{s}_to_{d}" for s, d in KINDS])
def test_every_source_kind_into_every_destination_kind(s, d):
    check(DESTINATIONS[d], SOURCES[s], n=3, k=1, n_rot=0, seed=10)


def test_a_two_by_two_source_and_a_destination_of_less_than_a_quad():
    check(cam(35, 33, "equidistant", 180), pano(2, 2), n=3, seed=11)
    check(pano(1, 3), pano(2, 2), n=2, seed=12)


# ---- 2. frame counts around the chunk, rotations per frame, the plan's own rotations ------------------------------------------------
@pytest.mark.parametrize("n", [1, 3, 5, 2 * F + 1])
@pytest.mark.parametrize("k,n_rot", [(1, 0), (2, 0), (1, 1), (2, 1)])
def test_frame_counts_and_rotation_counts(n, k, n_rot):
    check(cam(35, 33, "equidistant", 180), pano(16, 32), n=n, k=k, n_rot=n_rot, seed=20 + n)


def test_a_cube_destination_runs_its_face_rotation_before_the_plan_s_and_the_frame_s():
    check(cube(14), pano(16, 32), n=5, k=2, n_rot=1, seed=21)
    check(cube(14), cube(12), n=3, k=1, n_rot=1, seed=22)


def test_the_rotation_limit_is_the_plan_s_and_the_frame_s_together():
    dst, src = cam(35, 33, "equidistant", 180), pano(16, 32)
    check(dst, src, n=2, k=2, n_rot=nat.PB_MAX_ROTATIONS - 2, seed=30)
    check(dst, src, n=2, k=nat.PB_MAX_ROTATIONS, n_rot=0, seed=31)
    # one more: PB_ERR_INVALID, and nothing is written
    dstp, srcp = projections(dst, src)
    plan = nat.Plan(dstp, list(mats_of(PLAN_DEGREES[:7])), srcp, defer=True)
    table = torch.from_numpy(track_mats(2, 2)).cuda()
    frames = torch.from_numpy(random_frames(2, 16, 32, 32)).cuda()
    buf = torch.full((2 * 35 * 33 * 3 + 2 * GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
    assert track_call(plan, table, 2, "nearest", frames.data_ptr(), buf.data_ptr() + GUARD, 2) == INVALID
    assert b"exceed PB_MAX_ROTATIONS" in nat.load().pb_last_error()
    torch.cuda.synchronize()
    assert bool((buf == SENTINEL).all())


# ---- 3. strides and alignment -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", [dict(src_pad=5), dict(dst_pad=4), dict(src_pad=48, dst_pad=7), dict(dst_off=1), dict(dst_off=3, dst_pad=1, src_pad=1)],
                         ids=lambda v: "_".join(f"{k}{n}" for k, n in v.items()))
def test_padded_strides_and_destinations_off_a_dword_boundary(layout):
    """dst_pad 4 keeps the dword stores; an odd stride or offset takes the byte stores"""
    for interpolation in ("nearest", "bilinear"):
        check(cam(35, 33, "equidistant", 180), pano(16, 32), n=F + 1, k=1, seed=40, interpolation=interpolation, **layout)
    check(pano(20, 40), dbl(24, 48, "equidistant", 195), n=3, seed=41, **layout)


# ---- 4. double fisheyes at 180 and 195 degrees (the seam row's quirk included), polynomial lenses ----------------------------------
@pytest.mark.parametrize("fov", [180, 195])
@pytest.mark.parametrize("interpolation", ["nearest", "bilinear", "catmull-rom"])
def test_double_fisheye_sources_at_180_and_195_degrees(fov, interpolation):
    check(pano(24, 48), dbl(24, 48, "equidistant", fov), n=3, k=1, n_rot=1, seed=50 + fov, interpolation=interpolation)


@pytest.mark.parametrize("interpolation", ["nearest", "bilinear", "catmull-rom"])
def test_polynomial_lenses_as_source_and_as_destination(interpolation):
    check(pano(20, 40), cam(48, 48, "EQS9", 190, 23.5), n=3, seed=60, interpolation=interpolation)
    check(cam(40, 40, "CAL", 200, inscribed(40)), pano(24, 48), n=3, seed=61, interpolation=interpolation)


# ---- 5. the three interpolations on each source kind ------------------------------------------------------------------------------
@pytest.mark.parametrize("s", list(SOURCES))
@pytest.mark.parametrize("interpolation", ["bilinear", "catmull-rom"])
def test_the_interpolating_modes_on_every_source_kind(s, interpolation):
    check(cam(35, 33, "equidistant", 180), SOURCES[s], n=F + 1, k=1, n_rot=1, seed=70, interpolation=interpolation)
    check(cube(14), SOURCES[s], n=2, k=2, seed=71, interpolation=interpolation)


# ---- 6. every plan state is served alike -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", ["pano", "double"])
def test_deferred_prepared_and_tableless_plans_in_any_mode_give_identical_bytes(s):
    dst, src = cam(35, 33, "equidistant", 180), SOURCES[s]
    dstp, srcp = projections(dst, src)
    plan_mats = list(mats_of(PLAN_DEGREES[:1]))
    mats, frames = track_mats(3, 1), random_frames(3, src[1], src[2], 80)
    for interpolation in ("nearest", "bilinear", "catmull-rom"):
        want = expected(dstp, srcp, plan_mats, mats, frames, interpolation)
        states = {"deferred": nat.Plan(dstp, plan_mats, srcp, defer=True), "prepared": nat.Plan(dstp, plan_mats, srcp, bilinear=True),
                  "no bilinear tables": nat.Plan(dstp, plan_mats, srcp, bilinear=False)}
        for mode in (nat.MODE_FAITHFUL, nat.MODE_FAST, nat.MODE_FAST_DIRECT):
            p = nat.Plan(dstp, plan_mats, srcp, bilinear=True)
            p.set_mode(mode)
            states[f"mode {mode}"] = p
        for what, plan in states.items():
            assert n_diff(run_track(plan, mats, frames, interpolation), want) == 0, (what, interpolation)


# ---- 7. graph capture -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("interpolation", ["nearest", "catmull-rom"])
def test_a_captured_launch_replayed_once_gives_the_same_bytes(interpolation):
    """never allocates, never synchronises, never copies the table: ONE kernel node, captured on the current stream"""
    dst, src = cam(35, 33, "equidistant", 180), pano(16, 32)
    dstp, srcp = projections(dst, src)
    n = F + 1
    mats, frames = track_mats(n, 1), random_frames(n, 16, 32, 90)
    plan = nat.Plan(dstp, [], srcp, defer=True)
    want = run_track(plan, mats, frames, interpolation)
    table, src_t = torch.from_numpy(mats).cuda(), torch.from_numpy(frames).cuda()
    out = torch.zeros((n, 35, 33, 3), dtype=torch.uint8, device="cuda")
    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            assert track_call(plan, table, 1, interpolation, src_t.data_ptr(), out.data_ptr(), n) == 0  # (the current stream: the capturing one)
    torch.cuda.current_stream().wait_stream(side)
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert n_diff(out.cpu().numpy(), want) == 0


# ---- 8. the facade ----------------------------------------------------------------------------------------------------------------
def test_plan_remap_track_and_remap_frames_return_the_c_call_s_bytes():
    dst, src = cam(35, 33, "equidistant", 180), pano(16, 32)
    dstp, srcp = projections(dst, src)
    n = F + 2
    frames = random_frames(n, 16, 32, 100)
    plan = nat.Plan(dstp, list(mats_of(PLAN_DEGREES[:1])), srcp, defer=True)
    for k in (1, 2):
        mats = track_mats(n, k)
        for interpolation in ("nearest", "bilinear", "catmull-rom"):
            want = run_track(plan, mats, frames, interpolation)
            src_t = torch.from_numpy(frames).cuda()
            got = plan.remap_track(src_t, mats if k == 2 else mats[:, 0], interpolation=interpolation)
            assert isinstance(got, torch.Tensor) and got.is_cuda and n_diff(got.cpu().numpy(), want) == 0, (k, interpolation)
            out = torch.zeros_like(got)
            assert plan.remap_track(src_t, torch.from_numpy(mats).cuda(), out=out, interpolation=interpolation) is out  # a device table, in place
            torch.cuda.synchronize()
            assert n_diff(out.cpu().numpy(), want) == 0, (k, interpolation)
            streamed = np.stack([np.array(o) for o in batch.remap_frames(plan, list(frames), interpolation=interpolation, rotations=mats)])
            assert n_diff(streamed, want) == 0, (k, interpolation)
    # Rotation objects, one per frame
    rots = [pb.Rotation(*(pb.utils.to_radians(v) for v in d)) for d in DEGREES[:n]]
    want = run_track(plan, track_mats(n, 1), frames)
    assert n_diff(plan.remap_track(torch.from_numpy(frames).cuda(), rots).cpu().numpy(), want) == 0
    assert n_diff(np.stack([np.array(o) for o in batch.remap_frames(plan, iter(frames), depth=2, rotations=rots)]), want) == 0
    with pytest.raises(ValueError, match=f"frame {n - 1} has no rotation"):
        list(batch.remap_frames(plan, list(frames), rotations=rots[:-1]))


# ---- 9. the reference's own output ---------------------------------------------------------------------------------------------------
GOLD = np.load(os.path.join(H.GOLD, "rotation_track.npz"))


@pytest.mark.parametrize("case", rc.golden_cases(), ids=lambda c: c.name)
def test_the_nearest_track_is_the_reference_s_output_with_rotations_applied_in_turn(case):
    """tests/golden/rotation_track.npz: the real reference, Rotation objects applied one after another.  The fixture is the goldens'
    platform's; a host whose NumPy gives other last bits loads the library of ITS flavour and keeps the fragile-set allowance."""
    dstp, srcp = projections(case.dst, case.src)
    plan = nat.Plan(dstp, list(mats_of(case.plan_rot)) if case.plan_rot else [], srcp, defer=True)
    n, k = len(case.frames), len(case.frames[0])
    mats = mats_of([r for fr in case.frames for r in fr]).reshape(n, k, 3, 3)
    frames = rc.case_frames(case)
    got = run_track(plan, mats, frames)
    exact = H.live_numpy_is_the_goldens_numpy()
    for f in range(n):
        bad = (got[f] != GOLD[f"{case.name}/{f}/u8"]).any(axis=2)
        if exact:
            assert int(bad.sum()) == 0, (case.name, f, int(bad.sum()))
        else:
            rots = [tuple(map(orc.to_radians, r)) for r in case.chain(f)]
            with np.errstate(all="ignore"):
                fragile = orc.fragile_mask(orc.pretrunc(H.orc_proj(case.dst), H.orc_proj(case.src), rots))
            assert int((bad & ~fragile).sum()) == 0, (case.name, f, int(bad.sum()))
        # ... and through random bytes with the golden index map, where the source is a single image
        if case.src[0] != "double":
            idx = GOLD[f"{case.name}/{f}/idx"]
            img = random_frames(1, case.src[1], case.src[2], 110 + f)[0]
            want = img.reshape(-1, 3)[np.where(idx < 0, 0, idx)]
            want[idx < 0] = 0
            one = run_track(plan, mats[f : f + 1], img[None])[0]
            bad = (one != want).any(axis=2)
            assert int(bad.sum()) == 0 if exact else int((bad & ~fragile).sum()) == 0, (case.name, f, int(bad.sum()))
