"""pb_remap_track_nv12: NV12 and P010 video frames with a rotation per frame in one launch.  Frame f must be, byte for byte,
tests/nv12_ref.py's definition with the index map of the chain "the plan's own rotations, then frame f's" - the reference's own map where
the fixture holds it (tests/golden/rotation_track.npz), else pb_index_map_i32 of a private PB_MODE_FAITHFUL plan of that chain.  Every
comparison is exact equality; planes hold independent random bytes (a wrong index shows); destinations sit between sentinel bytes that
must survive, and so must every padding byte of pitched frames and the gaps between planes and frames.  Shapes are tens of pixels a side:
the smallest that still reach half quads (W % 4 == 2), rows off a dword, more than one workgroup and frame counts around the chunk."""

import os

import numpy as np
import pytest
import torch

import photonbend_amd as pb
from oracle import reference_path as orc
from photonbend_amd import _native as nat
from photonbend_amd.core import rotation_track
from tests import eac_cases as ec
from tests import helpers as H
from tests import nv12_ref
from tests import rotation_track_cases as rc
from tests.cases import Case, cam, inscribed, pano

pytestmark = pytest.mark.gpu

F = 4  # PB_TRACK_FRAMES (csrc/pb_kernels_track.hpp): frames a work-item loops over
SAMPLES = ((1, np.uint8), (2, np.uint16))
GUARD = 64
SENTINEL = 0xA5
GOLD = np.load(os.path.join(H.GOLD, "rotation_track.npz"))
cube, eac = ec.cube, ec.eac

# per-frame rotations in degrees: the identity, the pole-crossing pitch, then arbitrary ones (tests/test_hip_rotation_track.py's)
DEGREES = [(0, 0, 0), (-90, 0, 0), (30, 45, 10), (-3.5, 170, 12), (77, -120, 200), (1, 2, 3), (-40, 5, 77), (0, 90, 0), (12, 34, 56),
           (180, 0, 0), (0, 0, 45), (-15, 100, 200), (5, -20, 33), (89, 1, -1), (-60, -60, -60), (0.001, 0, 0), (45, 45, 45), (10, 20, 30)]
PLAN_DEGREES = [(3, 90, -7), (20, 30, 40)]


def mats_of(degrees):
    return rotation_track(np.array([[pb.utils.to_radians(v) for v in d] for d in degrees], dtype=np.float64).reshape(-1, 3))


def track_mats(n, k):
    """(n, k, 3, 3): frame f's k rotations; the identity and the pole-crossing pitch lead."""
    assert n * k <= len(DEGREES)
    return mats_of(DEGREES[: n * k]).reshape(n, k, 3, 3)


def projections(dst, src):
    s, cmap = ec.pb_chain(Case("track", dst, src), image=np.zeros((src[1], src[2], 3), np.uint8))
    return cmap.dst_proj, s._proj("src")


def random_frames(n, h, w, dt, seed):
    """n packed (3h/2, w) frames of independent random bytes."""
    S = np.dtype(dt).itemsize
    return np.random.default_rng(seed).integers(0, 256, (n, 3 * h // 2, w * S), dtype=np.uint8).view(dt)


def faithful_index(dstp, srcp, chain):
    """The index map of a private PB_MODE_FAITHFUL deferred plan of a whole chain (pb_index_map_i32): the float64 chain per pixel."""
    plan = nat.Plan(dstp, list(chain), srcp, defer=True)
    plan.set_mode(nat.MODE_FAITHFUL)
    idx = plan.index_map()
    torch.cuda.synchronize()
    return idx.cpu().numpy()


def chain_indices(dstp, srcp, plan_mats, mats):
    """frame f's index map: the plan's own rotations, then the frame's (computed once, shared by every sample size and fill)"""
    return [faithful_index(dstp, srcp, list(plan_mats) + list(m)) for m in mats]


def expected(idx, srcp, frames, fill=None):
    return np.stack([nv12_ref.remap_frame(frames[f], idx[f], srcp.height, srcp.width, fill) for f in range(len(frames))])


def span(pitch, uv, h):
    return uv + pitch * (h // 2)


class Layout:
    """A frame layout in bytes for n frames of h x w samples of S bytes: (pitch, uv_offset, frame_stride), 0 = the packed default."""

    def __init__(self, h, w, S, pitch=0, uv_gap=0, stride_pad=0):
        self.h, self.w, self.S = h, w, S
        self.pitch = pitch or w * S
        self.uv = self.pitch * h + uv_gap
        self.span = span(self.pitch, self.uv, h)
        self.stride = self.span + stride_pad
        self.packed = not (pitch or uv_gap or stride_pad)
        self.arg = None if self.packed else (self.pitch, self.uv, self.stride)

    def payload(self, n):
        """bool mask over n frames' bytes ((n - 1) strides + a span): the bytes that belong to a plane's row."""
        m = np.zeros((n - 1) * self.stride + self.span, bool)
        rb = self.w * self.S
        for f in range(n):
            for y in range(self.h):
                m[f * self.stride + y * self.pitch : f * self.stride + y * self.pitch + rb] = True
            for y in range(self.h // 2):
                m[f * self.stride + self.uv + y * self.pitch : f * self.stride + self.uv + y * self.pitch + rb] = True
        return m

    def scatter(self, frames, seed):
        """packed frames (n, 3h/2, w) laid out in a byte buffer whose padding is random"""
        n = len(frames)
        m = self.payload(n)
        buf = np.random.default_rng(seed).integers(0, 256, len(m), dtype=np.uint8)
        buf[m] = np.ascontiguousarray(frames).view(np.uint8).reshape(-1)  # (row by row, frame by frame: the mask's order)
        return buf

    def gather(self, buf, n, dt):
        m = self.payload(n)
        return buf[: len(m)][m].view(dt).reshape(n, 3 * self.h // 2, self.w), buf[: len(m)][~m]


def track_call(plan, table, k, src_ptr, dst_ptr, n, S, sl=None, dl=None, fill=None, stream=None):
    sl = None if sl is None else nat.pb_nv12_layout(*sl)
    dl = None if dl is None else nat.pb_nv12_layout(*dl)
    f = None if fill is None else (nat.C.c_uint16 * 3)(*fill)
    return nat.load().pb_remap_track_nv12(plan.handle, table.data_ptr(), k, src_ptr, dst_ptr, n, None if sl is None else nat.C.addressof(sl),
                                          None if dl is None else nat.C.addressof(dl), S, None if f is None else nat.C.addressof(f),
                                          nat.current_stream() if stream is None else stream)


def run_track(plan, mats, frames, fill=None, src_kw=None, dst_kw=None, dst_off=0):
    """One pb_remap_track_nv12 launch of packed frames (n, 3h/2, w) laid out as src_kw / dst_kw say (Layout's keywords), the destination
    dst_off bytes into its guarded buffer -> packed (n, 3H/2, W).  Guards, the offset bytes and every padding byte keep their sentinel."""
    n, dt = len(frames), frames.dtype
    S = dt.itemsize
    h, w, Hd, Wd = plan.src.height, plan.src.width, plan.dst.height, plan.dst.width
    sl, dl = Layout(h, w, S, **(src_kw or {})), Layout(Hd, Wd, S, **(dst_kw or {}))
    src = torch.from_numpy(sl.scatter(frames, seed=1)).cuda()
    table = torch.from_numpy(np.ascontiguousarray(mats)).cuda()
    nbytes = (n - 1) * dl.stride + dl.span
    buf = torch.full((nbytes + dst_off + 2 * GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
    if dst_off:  # a multiple of one pair that is not a multiple of a wide store
        assert (buf.data_ptr() + GUARD + dst_off) % (4 * S) == 2 * S
    rc_ = track_call(plan, table, mats.shape[1], src.data_ptr(), buf.data_ptr() + GUARD + dst_off, n, S, sl.arg, dl.arg, fill)
    assert rc_ == 0, nat.load().pb_last_error()
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert (got[: GUARD + dst_off] == SENTINEL).all() and (got[GUARD + dst_off + nbytes :] == SENTINEL).all(), "the launch wrote outside its frames"
    out, padding = dl.gather(got[GUARD + dst_off :], n, dt)
    assert (padding == SENTINEL).all(), "the launch wrote into the padding between rows, planes or frames"
    return out


def differing(got, want, Hd):
    """(luma pixels that differ (n, H, W), pairs that differ (n, H/2, W/2))"""
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    n, _, Wd = got.shape
    return got[:, :Hd] != want[:, :Hd], (got[:, Hd:] != want[:, Hd:]).reshape(n, Hd // 2, Wd // 2, 2).any(axis=3)


def assert_same(got, want, Hd, what=""):
    by, buv = differing(got, want, Hd)
    assert int(by.sum()) == 0 and int(buv.sum()) == 0, f"{what}: {int(by.sum())} luma pixels and {int(buv.sum())} pairs differ"


def check(dst, src, n=3, k=1, n_rot=0, seed=0, fills=(None,), **layout):
    dstp, srcp = projections(dst, src)
    plan_mats = list(mats_of(PLAN_DEGREES[:n_rot])) if n_rot else []
    mats = track_mats(n, k)
    plan = nat.Plan(dstp, plan_mats, srcp, defer=True)
    idx = chain_indices(dstp, srcp, plan_mats, mats)
    for S, dt in SAMPLES:
        frames = random_frames(n, src[1], src[2], dt, seed + S)
        for fill in fills:
            want = expected(idx, srcp, frames, fill)
            fy, fu, fv = nv12_ref.default_fill(dt) if fill is None else fill
            assert bool((want[:, : dst[1]] != fy).any()), "the geometry samples nothing: a test of fill shows nothing"
            assert_same(run_track(plan, mats, frames, fill, **layout), want, dst[1], f"S={S} fill={fill}")


# ---- 1. the reference's own index maps ----------------------------------------------------------------------------------------------
GOLDEN = [c for c in rc.golden_cases() if c.name in ("T_stabilise_pano", "T_fisheye_src_k2", "T_alter_k2")]
CHROMA_RULE = ("T_fisheye_src_k2", "T_alter_k2")  # every frame holds blocks with a black anchor beside valid pixels, and the other way round


@pytest.mark.parametrize("case", GOLDEN, ids=lambda c: c.name)
def test_the_reference_s_own_index_maps_in_one_four_frame_launch(case):
    assert len(GOLDEN) == 3 and len(case.frames) == 4
    _, h, w, *_ = case.src
    Hd, Wd = case.dst[1], case.dst[2]
    assert not (h | w | Hd | Wd) & 1
    idx = [GOLD[f"{case.name}/{f}/idx"] for f in range(4)]
    for f in range(4):
        blocks = (idx[f] >= 0).reshape(Hd // 2, 2, Wd // 2, 2).transpose(0, 2, 1, 3).reshape(-1, 4)
        mixed = blocks.any(axis=1) & ~blocks.all(axis=1)
        black_anchor, valid_anchor = int((mixed & ~blocks[:, 0]).sum()), int((mixed & blocks[:, 0]).sum())
        print(f"{case.name} frame {f}: {black_anchor} blocks with a black anchor beside valid pixels, {valid_anchor} the other way round")
        if case.name in CHROMA_RULE:  # an "any pixel decides" kernel cannot pass
            assert black_anchor >= 1 and valid_anchor >= 1, (case.name, f, black_anchor, valid_anchor)
    dstp, srcp = projections(case.dst, case.src)
    plan = nat.Plan(dstp, list(mats_of(case.plan_rot)) if case.plan_rot else [], srcp, defer=True)
    k = len(case.frames[0])
    mats = mats_of([r for fr in case.frames for r in fr]).reshape(4, k, 3, 3)
    exact = H.live_numpy_is_the_goldens_numpy()
    fragile = None
    if not exact:  # (the fixture is the goldens' platform's: the fragile set is the allowance, for chroma the anchors')
        with np.errstate(all="ignore"):
            fragile = np.stack([orc.fragile_mask(orc.pretrunc(H.orc_proj(case.dst), H.orc_proj(case.src), [tuple(map(orc.to_radians, r)) for r in case.chain(f)]))
                                for f in range(4)])
    for S, dt in SAMPLES:
        frames = random_frames(4, h, w, dt, seed=100 + S)
        for fill in (None, (1, 2, 3)):
            want = np.stack([nv12_ref.remap_frame(frames[f], idx[f], h, w, fill) for f in range(4)])
            got = run_track(plan, mats, frames, fill)  # ONE launch of the four frames
            by, buv = differing(got, want, Hd)
            if exact:
                assert int(by.sum()) == 0 and int(buv.sum()) == 0, (case.name, S, fill, int(by.sum()), int(buv.sum()))
            else:
                assert int((by & ~fragile).sum()) == 0 and int((buv & ~fragile[:, 0::2, 0::2]).sum()) == 0, (case.name, S, fill)


# ---- 2. every source kind x {panorama, camera, cube} destination --------------------------------------------------------------------
SOURCES = {
    "pano": pano(24, 48),
    "camera": cam(40, 40, "equisolid", 190, inscribed(40)),
    "cube": cube(12),
    "eac": eac(12),
}
DESTINATIONS = {
    "pano": pano(20, 40),
    "camera": cam(34, 30, "equidistant", 180),  # W % 4 == 2: a half quad ends every row; NV12 rows start off a dword on odd rows
    "cube": cube(14),                           # (28, 42): W % 4 == 2 again, 308 quads: two workgroups
}
KINDS = [(s, d) for s in SOURCES for d in DESTINATIONS]


@pytest.mark.parametrize("s,d", KINDS, ids=[f"{s}_to_{d}" for s, d in KINDS])
def test_every_source_kind_into_every_destination_kind(s, d):
    check(DESTINATIONS[d], SOURCES[s], n=3, k=1, n_rot=0, seed=10)


# ---- 3. frame counts around the chunk, rotations per frame, the plan's own rotations ------------------------------------------------
@pytest.mark.parametrize("n", [1, 3, 5, 2 * F + 1])
@pytest.mark.parametrize("k,n_rot", [(1, 0), (2, 0), (1, 1), (2, 1)])
def test_frame_counts_and_rotation_counts(n, k, n_rot):
    assert DEGREES[0] == (0, 0, 0) and DEGREES[1] == (-90, 0, 0)  # the identity and the pole-crossing pitch are among the rotations
    check(cam(34, 30, "equidistant", 180), pano(16, 32), n=n, k=k, n_rot=n_rot, seed=20 + n)


# ---- 4. layouts ---------------------------------------------------------------------------------------------------------------------
def _layouts(S):
    pitched = lambda w: dict(pitch=w * S + 6 * S)  # noqa: E731
    out = {
        "pitch_plus_6_samples": (lambda h, w: pitched(w), lambda h, w: pitched(w), 0),
        "gap_before_the_uv_plane": (lambda h, w: dict(uv_gap=10 * S), lambda h, w: dict(uv_gap=6 * S), 0),
        "padded_frame_stride": (lambda h, w: dict(stride_pad=2 * S), lambda h, w: dict(stride_pad=14 * S), 0),
        "destination_one_pair_off": (lambda h, w: {}, lambda h, w: {}, 2 * S),
        "everything_at_once": (lambda h, w: dict(pitch=w * S + 6 * S, uv_gap=4 * S, stride_pad=2 * S), lambda h, w: dict(pitch=w * S + 6 * S, uv_gap=2 * S, stride_pad=6 * S), 2 * S),
    }
    if S == 1:  # NV12 at a pitch of W + 2: no row but the first starts on a dword
        out["pitch_w_plus_2"] = (lambda h, w: dict(pitch=w + 2), lambda h, w: dict(pitch=w + 2), 0)
    return out


@pytest.mark.parametrize("S,dt", SAMPLES)
def test_pitches_plane_gaps_frame_strides_and_a_destination_one_pair_off_a_wide_store(S, dt):
    dst, src = cam(34, 30, "equidistant", 180), pano(16, 32)
    dstp, srcp = projections(dst, src)
    n = F + 1
    mats, frames = track_mats(n, 1), random_frames(n, 16, 32, dt, seed=40 + S)
    plan = nat.Plan(dstp, [], srcp, defer=True)
    want = expected(chain_indices(dstp, srcp, [], mats), srcp, frames)
    for name, (skw, dkw, off) in _layouts(S).items():
        assert off % (2 * S) == 0 and (off == 0 or off % (4 * S))
        assert_same(run_track(plan, mats, frames, None, skw(16, 32), dkw(34, 30), off), want, 34, name)


# ---- 5. the smallest shapes -----------------------------------------------------------------------------------------------------------
def test_one_pair_less_than_a_quad_and_a_full_quad_with_a_half_quad_per_row():
    check(pano(2, 2), pano(2, 2), n=3, seed=50)
    check(pano(4, 6), pano(2, 2), n=3, seed=51)
    check(pano(4, 6), pano(8, 16), n=F + 1, k=2, seed=52, fills=(None, (1, 2, 3)))


# ---- 6. against the tile kernel -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", ["pano", "camera", "cube", "eac"])
def test_each_frame_equals_pb_remap_nv12_of_a_prepared_plan_of_its_chain(s):
    dst, src = pano(20, 40), SOURCES[s]
    dstp, srcp = projections(dst, src)
    plan_mats = list(mats_of(PLAN_DEGREES[:1]))
    mats = track_mats(3, 1)
    plan = nat.Plan(dstp, plan_mats, srcp, defer=True)
    compared = 0
    for S, dt in SAMPLES:
        frames = random_frames(3, src[1], src[2], dt, seed=60 + S)
        got = run_track(plan, mats, frames, (1, 2, 3))
        for f in range(3):
            tiles = nat.Plan(dstp, plan_mats + list(mats[f]), srcp, bilinear=False)
            if not tiles.nv12_supported(S):  # (a geometry without a tile path has no single-plan counterpart)
                continue
            one = tiles.remap_nv12(torch.from_numpy(frames[f]).cuda(), fill=(1, 2, 3)).cpu().numpy()
            assert np.array_equal(got[f], one), (s, S, f)
            compared += 1
    assert compared >= 1, "no frame had a prepared plan the tile kernel serves: the comparison showed nothing"


# ---- 7. every plan state is served alike ----------------------------------------------------------------------------------------------
def test_deferred_prepared_and_tableless_plans_in_any_mode_give_identical_bytes():
    dst, src = cam(34, 30, "equidistant", 180), pano(24, 48)
    dstp, srcp = projections(dst, src)
    plan_mats = list(mats_of(PLAN_DEGREES[:1]))
    mats = track_mats(3, 1)
    states = {"deferred": nat.Plan(dstp, plan_mats, srcp, defer=True), "prepared": nat.Plan(dstp, plan_mats, srcp, bilinear=True),
              "no bilinear tables": nat.Plan(dstp, plan_mats, srcp, bilinear=False)}
    for mode in (nat.MODE_FAITHFUL, nat.MODE_FAST, nat.MODE_FAST_DIRECT):
        p = nat.Plan(dstp, plan_mats, srcp, bilinear=True)
        p.set_mode(mode)
        states[f"mode {mode}"] = p
    idx = chain_indices(dstp, srcp, plan_mats, mats)
    for S, dt in SAMPLES:
        frames = random_frames(3, 24, 48, dt, seed=70 + S)
        want = expected(idx, srcp, frames)
        for what, plan in states.items():
            assert_same(run_track(plan, mats, frames), want, 34, f"{what} S={S}")


# ---- 8. graph capture -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,dt", SAMPLES)
def test_a_captured_launch_replayed_once_gives_the_same_bytes(S, dt):
    """never allocates, never synchronises, never copies the table: ONE kernel node, a linear capture on one stream"""
    dst, src = cam(34, 30, "equidistant", 180), pano(16, 32)
    dstp, srcp = projections(dst, src)
    n = F + 1
    mats, frames = track_mats(n, 1), random_frames(n, 16, 32, dt, seed=80 + S)
    plan = nat.Plan(dstp, [], srcp, defer=True)
    want = run_track(plan, mats, frames)
    table, src_t = torch.from_numpy(mats).cuda(), torch.from_numpy(frames).cuda()
    out = torch.zeros((n, 51, 30 * S), dtype=torch.uint8, device="cuda")
    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            assert track_call(plan, table, 1, src_t.data_ptr(), out.data_ptr(), n, S) == 0  # (the current stream: the capturing one)
    torch.cuda.current_stream().wait_stream(side)
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy().view(dt), want)


# ---- 9. the facade --------------------------------------------------------------------------------------------------------------------
def test_plan_remap_track_nv12_returns_the_c_call_s_bytes_with_the_host_s_dtype():
    dst, src = cam(34, 30, "equidistant", 180), pano(16, 32)
    dstp, srcp = projections(dst, src)
    n = F + 2
    plan = nat.Plan(dstp, list(mats_of(PLAN_DEGREES[:1])), srcp, defer=True)
    for S, dt in SAMPLES:
        frames = random_frames(n, 16, 32, dt, seed=90 + S)
        src_t = torch.from_numpy(frames).cuda()
        for k in (1, 2):
            mats = track_mats(n, k)
            want = run_track(plan, mats, frames, (1, 2, 3))
            got = plan.remap_track_nv12(src_t, mats if k == 2 else mats[:, 0], fill=(1, 2, 3))
            assert isinstance(got, torch.Tensor) and got.is_cuda and got.dtype == nat.torch_dtype(dt) and np.array_equal(got.cpu().numpy(), want), (S, k)
            out = torch.zeros_like(got)
            assert plan.remap_track_nv12(src_t, torch.from_numpy(mats).cuda(), out=out, fill=(1, 2, 3)) is out  # a device table, in place
            torch.cuda.synchronize()
            assert np.array_equal(out.cpu().numpy(), want), (S, k)
        # Rotation objects, one per frame; a pitched 1-D source into a pitched `out`
        rots = [pb.Rotation(*(pb.utils.to_radians(v) for v in d)) for d in DEGREES[:n]]
        want = run_track(plan, track_mats(n, 1), frames)
        assert np.array_equal(plan.remap_track_nv12(src_t, rots).cpu().numpy(), want), S
        sl, dl = Layout(16, 32, S, pitch=32 * S + 6 * S), Layout(34, 30, S, pitch=30 * S + 6 * S, stride_pad=2 * S)
        buf = torch.from_numpy(sl.scatter(frames, seed=2).view(dt)).cuda()
        mine = torch.full(((n - 1) * dl.stride + dl.span,), SENTINEL, dtype=torch.uint8, device="cuda").view(nat.torch_dtype(dt))
        assert plan.remap_track_nv12(buf, rots, out=mine, src_layout=sl.arg, dst_layout=dl.arg) is mine
        torch.cuda.synchronize()
        got, padding = dl.gather(mine.cpu().numpy().view(np.uint8), n, dt)
        assert np.array_equal(got, want) and bool((padding == SENTINEL).all()), S
    with pytest.raises(ValueError, match="the table holds"):
        plan.remap_track_nv12(src_t, track_mats(n - 1, 1))
