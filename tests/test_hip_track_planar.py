"""pb_remap_track_planar: planar video frames - 4:4:4, 4:2:2, 4:2:0, uint8 or uint16 samples - with a rotation per frame in
one launch.  Frame f must be, byte for byte, tests/planar_ref.py's definition with the index map of the chain "the plan's own rotations,
then frame f's" - the reference's own map where the fixture holds it (tests/golden/rotation_track.npz), else pb_index_map_i32 of a
private PB_MODE_FAITHFUL plan of that chain.  Every comparison is exact equality; planes hold independent random bytes; destinations sit
between sentinel bytes that must survive, and so must every padding byte of pitched frames.  Shapes are tens of pixels a side."""

import numpy as np
import pytest
import torch

from oracle import reference_path as orc
from photonbend_amd import _native as nat
from tests import helpers as H
from tests import planar_ref
from tests import rotation_track_cases as rc
from tests.cases import cam, pano
from tests.test_hip_track_nv12 import F, GOLD, GUARD, PLAN_DEGREES, SENTINEL, chain_indices, mats_of, projections, track_mats
from tests.test_hip_track_nv12 import track_call as nv12_track_call

pytestmark = pytest.mark.gpu

SAMPLES = ((1, np.uint8), (2, np.uint16))
SUBS = {"444": nat.PLANAR_444, "422": nat.PLANAR_422, "420": nat.PLANAR_420}
INVALID, UNSUPPORTED = -1, -3


def random_frames(n, h, w, sub, dt, seed):
    """n packed flat frames of independent random bytes."""
    nb = planar_ref.frame_samples(h, w, sub) * np.dtype(dt).itemsize
    return np.random.default_rng(seed).integers(0, 256, (n, nb), dtype=np.uint8).view(dt)


def expected(idx, h, w, sub, frames, fill=None):
    return np.stack([planar_ref.remap_frame(frames[f], idx[f], h, w, sub, fill) for f in range(len(frames))])


def track_call(plan, table, k, src_ptr, dst_ptr, n, sub, S, sl=None, dl=None, fill=None, stream=None):
    sl = None if sl is None else nat.pb_planar_layout(*sl)
    dl = None if dl is None else nat.pb_planar_layout(*dl)
    f = None if fill is None else (nat.C.c_uint16 * 3)(*fill)
    return nat.load().pb_remap_track_planar(plan.handle, table.data_ptr(), k, src_ptr, dst_ptr, n, None if sl is None else nat.C.addressof(sl),
                                            None if dl is None else nat.C.addressof(dl), SUBS[sub], S, None if f is None else nat.C.addressof(f),
                                            nat.current_stream() if stream is None else stream)


class Layout:
    """A frame layout in bytes for frames of h x w samples of S bytes; every gap 0: packed."""

    def __init__(self, h, w, S, sub, pitch_pad=0, cpitch_pad=0, gap1=0, gap2=0, stride_pad=0):
        cx, cy = planar_ref.SHIFTS[sub]
        self.rows = [(h, w * S), (h >> cy, (w >> cx) * S), (h >> cy, (w >> cx) * S)]  # per plane: rows, bytes of a row
        self.pitch, self.cpitch = w * S + pitch_pad, (w >> cx) * S + cpitch_pad
        self.o1 = self.pitch * h + gap1
        self.o2 = self.o1 + self.cpitch * (h >> cy) + gap2
        self.span = self.o2 + self.cpitch * ((h >> cy) - 1) + (w >> cx) * S
        self.stride = self.o2 + self.cpitch * (h >> cy) + stride_pad
        self.arg = (self.pitch, self.cpitch, self.o1, self.o2, self.stride) if (pitch_pad or cpitch_pad or gap1 or gap2 or stride_pad) else None

    def payload(self, n):
        m = np.zeros((n - 1) * self.stride + self.span, bool)
        for f in range(n):
            for (rows, nb), off, pitch in zip(self.rows, (0, self.o1, self.o2), (self.pitch, self.cpitch, self.cpitch)):
                for y in range(rows):
                    m[f * self.stride + off + y * pitch : f * self.stride + off + y * pitch + nb] = True
        return m

    def scatter(self, frames, seed):
        m = self.payload(len(frames))
        buf = np.random.default_rng(seed).integers(0, 256, len(m), dtype=np.uint8)
        buf[m] = np.ascontiguousarray(frames).view(np.uint8).reshape(-1)  # (row by row, plane by plane, frame by frame: the mask's order)
        return buf

    def gather(self, buf, n, dt):
        m = self.payload(n)
        return buf[: len(m)][m].view(dt).reshape(n, -1), buf[: len(m)][~m]


def run_track(plan, mats, frames, sub, fill=None, src_kw=None, dst_kw=None, dst_off=0):
    """One pb_remap_track_planar launch of packed flat frames laid out as src_kw / dst_kw say, the destination dst_off bytes into its
    guarded buffer -> packed flat frames.  Guards, the offset bytes and every padding byte keep their sentinel."""
    n, dt = len(frames), frames.dtype
    S = dt.itemsize
    h, w, Hd, Wd = plan.src.height, plan.src.width, plan.dst.height, plan.dst.width
    sl, dl = Layout(h, w, S, sub, **(src_kw or {})), Layout(Hd, Wd, S, sub, **(dst_kw or {}))
    src = torch.from_numpy(sl.scatter(frames, seed=1)).cuda()
    table = torch.from_numpy(np.ascontiguousarray(mats)).cuda()
    nbytes = (n - 1) * dl.stride + dl.span
    buf = torch.full((nbytes + dst_off + 2 * GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
    rc_ = track_call(plan, table, mats.shape[1], src.data_ptr(), buf.data_ptr() + GUARD + dst_off, n, sub, S, sl.arg, dl.arg, fill)
    assert rc_ == 0, nat.load().pb_last_error()
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert (got[: GUARD + dst_off] == SENTINEL).all() and (got[GUARD + dst_off + nbytes :] == SENTINEL).all(), "the launch wrote outside its frames"
    out, padding = dl.gather(got[GUARD + dst_off :], n, dt)
    assert (padding == SENTINEL).all(), "the launch wrote into the padding between rows, planes or frames"
    return out


def assert_same(got, want, what=""):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape)
    assert int((got != want).sum()) == 0, f"{what}: {int((got != want).sum())} samples differ"


def subs_of(dst, src):
    return [s for s in planar_ref.SUBSAMPLINGS if planar_ref.dims_ok(s, dst[1:3], src[1:3])]


# ---- 1. six geometries x four frames: the shapes of the rotation-track fixture --------------------------------------------------------
GOLDEN = {c.name: c for c in rc.golden_cases()}
# the four single-source cases with the reference's own index maps; the two double-fisheye shapes with a panorama of the same size in
# the double fisheye's place (pb_remap_track_planar refuses a double fisheye: test_the_refusals), their index maps from pb_index_map_i32
GEOMETRIES = ["T_stabilise_pano", "T_reframe_odd", "T_fisheye_src_k2", "T_alter_k2", "T_double_195", "T_double_180_seam"]


def _geometry(name):
    case = GOLDEN[name]
    src = pano(case.src[1], case.src[2]) if case.src[0] == "double" else case.src
    dstp, srcp = projections(case.dst, src)
    plan_mats = list(mats_of(case.plan_rot)) if case.plan_rot else []
    k = len(case.frames[0])
    mats = mats_of([r for fr in case.frames for r in fr]).reshape(4, k, 3, 3)
    if case.src[0] == "double":
        idx, fragile, exact = chain_indices(dstp, srcp, plan_mats, mats), None, True
    else:
        idx = [GOLD[f"{name}/{f}/idx"] for f in range(4)]
        exact, fragile = H.live_numpy_is_the_goldens_numpy(), None
        if not exact:  # (the fixture is the goldens' platform's: the fragile set is the allowance, for planes 1 and 2 the anchors')
            with np.errstate(all="ignore"):
                fragile = [orc.fragile_mask(orc.pretrunc(H.orc_proj(case.dst), H.orc_proj(case.src), [tuple(map(orc.to_radians, r)) for r in case.chain(f)]))
                           for f in range(4)]
    return case, src, dstp, srcp, plan_mats, mats, idx, fragile, exact


def test_the_geometries_are_the_fixture_s_six():
    assert sorted(GEOMETRIES) == sorted(GOLDEN) and all(len(c.frames) == 4 for c in GOLDEN.values())
    assert subs_of(GOLDEN["T_reframe_odd"].dst, GOLDEN["T_reframe_odd"].src) == ["444"]  # 35 x 33: odd both ways
    assert all(len(subs_of(GOLDEN[n].dst, GOLDEN[n].src)) == 3 for n in GEOMETRIES if n != "T_reframe_odd")


@pytest.mark.parametrize("name", GEOMETRIES)
def test_four_frames_in_one_launch_equal_the_definition_the_tile_kernel_and_the_nv12_track(name):
    case, src, dstp, srcp, plan_mats, mats, idx, fragile, exact = _geometry(name)
    _, h, w, *_ = src
    Hd, Wd = case.dst[1], case.dst[2]
    plan = nat.Plan(dstp, plan_mats, srcp, defer=True)  # a deferred plan: the plan's tables are never read
    tiles = [nat.Plan(dstp, plan_mats + list(mats[f]), srcp, bilinear=False) for f in range(4)]  # prepared plans of the whole chains
    compared = 0
    for sub in subs_of(case.dst, src):
        cx, cy = planar_ref.SHIFTS[sub]
        for S, dt in SAMPLES:
            frames = random_frames(4, h, w, sub, dt, seed=100 + S + SUBS[sub])
            for fill in (None, (1, 2, 3)):
                want = expected(idx, h, w, sub, frames, fill)
                got = run_track(plan, mats, frames, sub, fill)  # ONE launch of the four frames
                for f in range(4):
                    bad = [g != x for g, x in zip(planar_ref.planes(got[f], Hd, Wd, sub), planar_ref.planes(want[f], Hd, Wd, sub))]
                    if exact:
                        assert [int(b.sum()) for b in bad] == [0, 0, 0], (name, sub, S, fill, f)
                    else:
                        fa = fragile[f][0 :: 1 << cy, 0 :: 1 << cx]
                        assert int((bad[0] & ~fragile[f]).sum()) == 0 and int((bad[1] & ~fa).sum()) == 0 and int((bad[2] & ~fa).sum()) == 0, (name, sub, S, fill, f)
            # ... equals pb_remap_planar of a prepared plan of the whole chain, wherever it is served
            got = run_track(plan, mats, frames, sub, (1, 2, 3))
            for f in range(4):
                if tiles[f].planar_supported(sub, S):
                    one = tiles[f].remap_planar(torch.from_numpy(frames[f]).cuda(), sub, fill=(1, 2, 3)).cpu().numpy()
                    assert np.array_equal(got[f], one), (name, sub, S, f)
                    compared += 1
            # ... and, at 4:2:0, pb_remap_track_nv12 de-interleaved
            if sub == "420":
                semi = np.stack([np.concatenate([p0, np.stack([p1, p2], axis=2).reshape(h // 2, w)], axis=0)
                                 for p0, p1, p2 in (planar_ref.planes(fr, h, w, sub) for fr in frames)])
                s_t, tab = torch.from_numpy(np.ascontiguousarray(semi)).cuda(), torch.from_numpy(np.ascontiguousarray(mats)).cuda()
                out = torch.zeros((4, 3 * Hd // 2, Wd * S), dtype=torch.uint8, device="cuda")
                assert nv12_track_call(plan, tab, mats.shape[1], s_t.data_ptr(), out.data_ptr(), 4, S, fill=(1, 2, 3)) == 0
                torch.cuda.synchronize()
                o = out.cpu().numpy().view(dt)
                for f in range(4):
                    p0, p1, p2 = planar_ref.planes(got[f], Hd, Wd, sub)
                    uv = o[f, Hd:].reshape(Hd // 2, Wd // 2, 2)
                    assert np.array_equal(o[f, :Hd], p0) and np.array_equal(uv[..., 0], p1) and np.array_equal(uv[..., 1], p2), (name, S, f)
    assert compared >= 1, "no frame had a prepared plan the tile kernel serves: the comparison showed nothing"


# ---- 2. a five-frame batch (the last chunk is short), pitched frames, a destination off a wide store ----------------------------------
@pytest.mark.parametrize("sub", planar_ref.SUBSAMPLINGS)
def test_a_five_frame_batch_pitched_frames_and_every_plan_state(sub):
    # 34 x 30: W % 4 == 2, a half quad ends every row; 4:4:4 also 33 x 35 <- 3 x 5, a quad of three and odd rows
    shapes = [(cam(34, 30, "equidistant", 180), pano(16, 32))] + ([(cam(33, 35, "equidistant", 180), pano(3, 5))] if sub == "444" else [])
    n = F + 1
    assert n == 5
    for dst, src in shapes:
        dstp, srcp = projections(dst, src)
        plan_mats = list(mats_of(PLAN_DEGREES[:1]))
        mats = track_mats(n, 1)
        idx = chain_indices(dstp, srcp, plan_mats, mats)
        faithful = nat.Plan(dstp, plan_mats, srcp, bilinear=False)
        faithful.set_mode(nat.MODE_FAITHFUL)
        states = {"deferred": nat.Plan(dstp, plan_mats, srcp, defer=True), "prepared": nat.Plan(dstp, plan_mats, srcp, bilinear=False), "faithful": faithful}
        for S, dt in SAMPLES:
            frames = random_frames(n, src[1], src[2], sub, dt, seed=200 + S)
            want = expected(idx, src[1], src[2], sub, frames)
            assert bool((want != planar_ref.default_fill(dt)[0]).any())
            for what, plan in states.items():
                assert_same(run_track(plan, mats, frames, sub), want, f"{what} {sub} S={S}")
            plan = states["deferred"]
            pitched = dict(pitch_pad=6 * S, cpitch_pad=3 * S, gap1=5 * S, gap2=S, stride_pad=7 * S)
            assert_same(run_track(plan, mats, frames, sub, None, pitched, pitched), want, f"pitched {sub} S={S}")
            assert_same(run_track(plan, mats, frames, sub, None, None, None, S), want, f"one sample off {sub} S={S}")
            # the facade: typed arrays in and out
            got = plan.remap_track_planar(torch.from_numpy(frames).cuda(), mats[:, 0], sub)
            assert got.dtype == nat.torch_dtype(dt) and np.array_equal(got.cpu().numpy(), want), (sub, S)
        with pytest.raises(ValueError, match="the table holds"):
            states["deferred"].remap_track_planar(torch.from_numpy(frames).cuda(), track_mats(n - 1, 1), sub)


# ---- 3. the refusals --------------------------------------------------------------------------------------------------------------------
def test_the_refusals():
    L = nat.load()
    dst, src = pano(24, 48), pano(24, 48)
    dstp, srcp = projections(dst, src)
    plan = nat.Plan(dstp, list(mats_of(PLAN_DEGREES[:1])), srcp, defer=True)
    frames = torch.from_numpy(random_frames(2, 24, 48, "444", np.uint8, seed=300)).cuda()
    table = torch.from_numpy(track_mats(2, 1)).cuda()
    for sub in planar_ref.SUBSAMPLINGS:
        buf = torch.full((2 * 3 * 24 * 48,), SENTINEL, dtype=torch.uint8, device="cuda")

        def call(tab_ptr=table.data_ptr(), k=1, S=1, subsampling=SUBS[sub]):
            return L.pb_remap_track_planar(plan.handle, tab_ptr, k, frames.data_ptr(), buf.data_ptr(), 2, None, None, subsampling, S, None, nat.current_stream())

        # the table's checks are pb_remap_track_u8's
        assert call(tab_ptr=None) == INVALID and L.pb_last_error() == b"null rotation table"
        assert call(tab_ptr=table.data_ptr() + 4) == INVALID and b"8-byte aligned" in L.pb_last_error()
        assert call(k=0) == INVALID and b"n_rot_per_frame" in L.pb_last_error()
        assert call(k=nat.PB_MAX_ROTATIONS) == INVALID and b"PB_MAX_ROTATIONS" in L.pb_last_error()
        assert call(S=3) == INVALID and call(subsampling=5) == INVALID
        torch.cuda.synchronize()
        assert bool((buf == SENTINEL).all()), sub
    # a double-fisheye source, from the fixture's shapes
    case = GOLDEN["T_double_195"]
    dstp, srcp = projections(case.dst, case.src)
    double = nat.Plan(dstp, [], srcp, defer=True)
    src_t = torch.zeros(3 * case.src[1] * case.src[2], dtype=torch.uint8, device="cuda")
    buf = torch.full((3 * case.dst[1] * case.dst[2],), SENTINEL, dtype=torch.uint8, device="cuda")
    for sub in planar_ref.SUBSAMPLINGS:
        assert track_call(double, table, 1, src_t.data_ptr(), buf.data_ptr(), 1, sub, 1) == UNSUPPORTED and b"single sources" in L.pb_last_error()
    torch.cuda.synchronize()
    assert bool((buf == SENTINEL).all())
