"""pb_track_stitch_planar / pb_track_stitch_nv12: video frames of a double fisheye with a rotation per frame in one launch.
Frame f must be, byte for byte, tests/stitch_video_ref.py's definition with the taps and factors of the chain "the plan's own rotations,
then frame f's" - the CPU oracle's (on a host whose NumPy is not the goldens' NumPy: pb_index_map_i32 with weights of a PB_MODE_FAITHFUL plan
of that chain) -, what pb_stitch_planar / pb_stitch_nv12 write from a prepared plan of the whole chain, and, at 4:4:4 uint8 with fill 0,
pb_remap_track_u8's channels and the reference's own output (tests/golden/rotation_track.npz).  Every comparison is exact equality on
independent random samples over the full range of the sample type; destinations sit between sentinel bytes that must survive, and so must
every padding byte of pitched frames.  Shapes are tens of pixels a side: the smallest that reach invalid pixels, two-eye and one-eye
pixels, non-finite factors, a row's last quad of three pixels, rows that straddle waves and a chroma block across the seam between the eyes;
the counts come from the CPU oracle and are asserted."""

import os

import numpy as np
import pytest
import torch
from click.testing import CliRunner

import photonbend_amd as pb
from photonbend_amd import _native as nat
from photonbend_amd.scripts import cli
from tests import helpers as H
from tests import rotation_track_cases as rc
from tests import stitch_video_ref as ref
from tests.cases import cam, dbl, inscribed, pano
from tests.test_hip_track_nv12 import DEGREES, F, GUARD, PLAN_DEGREES, SENTINEL, mats_of, projections
from tests.test_track_stitch_ref_host import chain_taps

pytestmark = pytest.mark.gpu

SAMPLES = ((1, np.uint8), (2, np.uint16))
SUBS = {"444": nat.PLANAR_444, "422": nat.PLANAR_422, "420": nat.PLANAR_420}
FORMATS = ("444", "422", "420", "nv12")
INVALID, UNSUPPORTED = -1, -3
N = F + 1  # five frames: a chunk of four and a short one
GOLD = np.load(os.path.join(H.GOLD, "rotation_track.npz"))
GOLDEN = {c.name: c for c in rc.golden_cases() if c.src[0] == "double"}

# name -> (destination, source, the plan's own rotations in degrees)
GEOMETRIES = {
    "T_double_195": (GOLDEN["T_double_195"].dst, GOLDEN["T_double_195"].src, []),  # a fisheye destination: invalid pixels
    "T_double_180_seam": (GOLDEN["T_double_180_seam"].dst, GOLDEN["T_double_180_seam"].src, list(GOLDEN["T_double_180_seam"].plan_rot)),
    "odd_half_width_40x82": (pano(40, 80), dbl(40, 82, "equidistant", 195), []),  # w // 2 = 41: a chroma block straddles the seam between the eyes
    "odd_destination_33x67": (pano(33, 67), dbl(24, 48, "equidistant", 180), []),  # 4:4:4 only: a row's last quad holds 3 pixels; non-finite factors
    "stereographic_36x36": (cam(36, 36, "stereographic", 140, inscribed(36)), dbl(32, 64, "equidistant", 190), [PLAN_DEGREES[0]]),  # 9 quads a row: rows straddle waves
    "half_quad_20x30": (pano(20, 30), dbl(24, 48, "equidistant", 195), []),  # every format: a row's last quad holds 2 pixels and, subsampled, one anchor
}


def sub_of(fmt):
    return "420" if fmt == "nv12" else fmt


def formats_of(dst, src):
    return [f for f in FORMATS if ref.dims_ok(sub_of(f), src[1:3], dst[1:3])]


def track_degrees(n, k):
    """frame f's k rotations in degrees; the identity and the pole-crossing pitch lead (tests/test_hip_track_nv12.py's list)."""
    assert n * k <= len(DEGREES)
    return [DEGREES[f * k : (f + 1) * k] for f in range(n)]


def mats_of_track(track):
    return mats_of([r for fr in track for r in fr]).reshape(len(track), len(track[0]), 3, 3)


def random_frames(n, h, w, sub, dt, seed):
    """n packed flat planar frames of independent random bytes: every sample anywhere in its type's range."""
    nb = ref.frame_samples(h, w, sub) * np.dtype(dt).itemsize
    return np.random.default_rng(seed).integers(0, 256, (n, nb), dtype=np.uint8).view(dt)


class Geometry:
    """A geometry with its deferred plan and, per track, the definition's taps of every frame - computed once and shared."""

    def __init__(self, name):
        self.name = name
        self.dst, self.src, self.plan_rot = GEOMETRIES[name]
        self.dstp, self.srcp = projections(self.dst, self.src)
        self.plan_mats = list(mats_of(self.plan_rot)) if self.plan_rot else []
        self.plan = nat.Plan(self.dstp, self.plan_mats, self.srcp, defer=True)  # a deferred plan: the plan's tables are never read
        self.h, self.w, self.Hd, self.Wd = self.src[1], self.src[2], self.dst[1], self.dst[2]
        self._taps = {}

    def taps(self, track):
        key = repr(track)
        if key not in self._taps:
            if H.live_numpy_is_the_goldens_numpy():
                self._taps[key] = [chain_taps(self.dst, self.src, list(self.plan_rot) + list(fr)) for fr in track]
            else:  # (this host's NumPy may differ from the device's restated functions in the last bit: the float64 chain's own taps)
                self._taps[key] = [self.device_taps(list(m)) for m in mats_of_track(track)]
        return self._taps[key]

    def device_taps(self, frame_mats):
        plan = nat.Plan(self.dstp, self.plan_mats + frame_mats, self.srcp, defer=True)
        plan.set_mode(nat.MODE_FAITHFUL)
        idx, wts = plan.index_map(weights=True)
        torch.cuda.synchronize()
        idx, wts = idx.cpu().numpy(), wts.cpu().numpy()
        return idx[0], idx[1], wts[0], wts[1]

    def expected(self, track, frames, sub, fill):
        return np.stack([ref.stitch_frame(frames[f], *t, self.h, self.w, sub, fill) for f, t in enumerate(self.taps(track))])


_GEOMETRIES = {}


def geometry(name):
    if name not in _GEOMETRIES:
        _GEOMETRIES[name] = Geometry(name)
    return _GEOMETRIES[name]


class Layout:
    """A frame layout in bytes for frames of h x w samples of S bytes in format `fmt`; every keyword 0 / False: packed.  The planes of a
    frame in their logical order: (byte offset, rows, payload bytes of a row, pitch)."""

    def __init__(self, fmt, h, w, S, pitch_pad=0, cpitch_pad=0, gap1=0, gap2=0, stride_pad=0, swap=False):
        cx, cy = ref.SHIFTS[sub_of(fmt)]
        pitch = w * S + pitch_pad
        if fmt == "nv12":  # one pitch for both planes; pairs of 2 * S bytes
            uv = pitch * h + gap1
            self.planes = [(0, h, w * S, pitch), (uv, h // 2, w * S, pitch)]
            arg = (pitch, uv)
        else:
            cpitch = (w >> cx) * S + cpitch_pad
            o1 = pitch * h + gap1
            o2 = o1 + cpitch * (h >> cy) + gap2
            if swap:
                o1, o2 = o2, o1
            self.planes = [(0, h, w * S, pitch), (o1, h >> cy, (w >> cx) * S, cpitch), (o2, h >> cy, (w >> cx) * S, cpitch)]
            arg = (pitch, cpitch, o1, o2)
        self.span = max(off + (rows - 1) * p + nb for off, rows, nb, p in self.planes)
        self.stride = max(off + rows * p for off, rows, nb, p in self.planes) + stride_pad
        self.arg = arg + (self.stride,) if (pitch_pad or cpitch_pad or gap1 or gap2 or stride_pad or swap) else None

    def _rows(self, n):
        """(start byte, payload bytes) of every row, frame by frame, plane by plane in logical order"""
        for f in range(n):
            for off, rows, nb, p in self.planes:
                for y in range(rows):
                    yield f * self.stride + off + y * p, nb

    def scatter(self, frames, seed):
        """packed frames (n, samples) laid out in a byte buffer whose padding is random"""
        data = np.ascontiguousarray(frames).view(np.uint8).reshape(-1)
        buf = np.random.default_rng(seed).integers(0, 256, (len(frames) - 1) * self.stride + self.span, dtype=np.uint8)
        at = 0
        for start, nb in self._rows(len(frames)):
            buf[start : start + nb] = data[at : at + nb]
            at += nb
        assert at == data.size
        return buf

    def gather(self, buf, n, dt):
        """-> packed frames (n, samples), the padding bytes"""
        pad = np.ones((n - 1) * self.stride + self.span, bool)
        parts = []
        for start, nb in self._rows(n):
            parts.append(buf[start : start + nb])
            pad[start : start + nb] = False
        return np.concatenate(parts).view(dt).reshape(n, -1), buf[: len(pad)][pad]


def track_call(plan, table, k, src_ptr, dst_ptr, n, fmt, S, sl=None, dl=None, fill=None, stream=None):
    """The raw C call: pb_track_stitch_nv12 for "nv12", pb_track_stitch_planar for a subsampling."""
    cls = nat.pb_nv12_layout if fmt == "nv12" else nat.pb_planar_layout
    sl, dl = (None if l is None else cls(*l) for l in (sl, dl))
    f = None if fill is None else (nat.C.c_uint16 * 3)(*fill)
    args = [plan.handle, table.data_ptr(), k, src_ptr, dst_ptr, n, None if sl is None else nat.C.addressof(sl), None if dl is None else nat.C.addressof(dl)]
    args += ([] if fmt == "nv12" else [SUBS[fmt]]) + [S, None if f is None else nat.C.addressof(f), nat.current_stream() if stream is None else stream]
    return (nat.load().pb_track_stitch_nv12 if fmt == "nv12" else nat.load().pb_track_stitch_planar)(*args)


def interleaved(frames, h, w):
    return np.stack([ref.nv12_of(f, h, w) for f in frames])


def planar_of(semi, Hd, Wd):
    """packed NV12 frames (n, samples) -> packed yuv420p frames"""
    uv = semi[:, Hd * Wd :].reshape(len(semi), Hd // 2, Wd // 2, 2)
    return np.concatenate([semi[:, : Hd * Wd], uv[..., 0].reshape(len(semi), -1), uv[..., 1].reshape(len(semi), -1)], axis=1)


def run(plan, mats, frames, fmt, fill=None, src_kw=None, dst_kw=None, dst_off=0):
    """ONE launch of packed flat PLANAR frames ("nv12": interleaved on the way in, taken apart on the way out) laid out as src_kw / dst_kw
    say, the destination dst_off bytes into its guarded buffer -> packed flat planar frames.  The guards, the offset bytes and every
    padding byte keep their sentinel."""
    n, dt = len(frames), frames.dtype
    S = dt.itemsize
    h, w, Hd, Wd = plan.src.height, plan.src.width, plan.dst.height, plan.dst.width
    sl, dl = Layout(fmt, h, w, S, **(src_kw or {})), Layout(fmt, Hd, Wd, S, **(dst_kw or {}))
    src = torch.from_numpy(sl.scatter(interleaved(frames, h, w) if fmt == "nv12" else frames, seed=1)).cuda()
    table = torch.from_numpy(np.ascontiguousarray(mats)).cuda()
    nbytes = (n - 1) * dl.stride + dl.span
    buf = torch.full((nbytes + dst_off + 2 * GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
    rc_ = track_call(plan, table, mats.shape[1], src.data_ptr(), buf.data_ptr() + GUARD + dst_off, n, fmt, S, sl.arg, dl.arg, fill)
    assert rc_ == 0, nat.load().pb_last_error()
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert (got[: GUARD + dst_off] == SENTINEL).all() and (got[GUARD + dst_off + nbytes :] == SENTINEL).all(), "the launch wrote outside its frames"
    out, padding = dl.gather(got[GUARD + dst_off :], n, dt)
    assert (padding == SENTINEL).all(), "the launch wrote into the padding between rows, planes or frames"
    return planar_of(out, Hd, Wd) if fmt == "nv12" else out


def assert_same(got, want, what=""):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    assert int((got != want).sum()) == 0, f"{what}: {int((got != want).sum())} samples differ"


# ---- 1. every geometry x format x sample size x fill x k, exactly the definition and the tile kernel's frame --------------------------------
def test_the_geometries_reach_every_class_of_pixel():
    """From the CPU oracle (host arithmetic only): per frame, the pixels with both eyes live, one eye live, none, and non-finite factors."""
    counts = {}
    for name, (dst, src, plan_rot) in GEOMETRIES.items():
        rows = []
        for k in (1, 2):
            for fr in track_degrees(N, k):
                il, ir, fl, fr_ = chain_taps(dst, src, list(plan_rot) + list(fr))
                rows.append((int(((il >= 0) & (ir >= 0)).sum()), int(((il >= 0) ^ (ir >= 0)).sum()), int(((il < 0) & (ir < 0)).sum()),
                             int((~np.isfinite(fl) | ~np.isfinite(fr_)).sum())))
        counts[name] = np.array(rows)
        print(name, "two-eye / one-eye / none / non-finite per frame:", counts[name].tolist())
    assert all((c[:, 0] > 0).all() and (c[:, 1] > 0).all() for c in counts.values())  # two-eye and one-eye pixels in every frame of every geometry
    assert (counts["T_double_195"][:, 2] > 0).all() and (counts["stereographic_36x36"][:, 2] == 344).all()  # invalid pixels
    assert (counts["odd_destination_33x67"][:, 3] > 0).all()  # the cast's zero rule
    assert formats_of(*GEOMETRIES["odd_destination_33x67"][:2]) == ["444"] and GEOMETRIES["odd_destination_33x67"][0][2] % 4 == 3
    assert all(formats_of(*g[:2]) == list(FORMATS) for n, g in GEOMETRIES.items() if n != "odd_destination_33x67")
    assert (GEOMETRIES["odd_half_width_40x82"][1][2] // 2) & 1 and -(-GEOMETRIES["stereographic_36x36"][0][2] // 4) == 9
    assert GEOMETRIES["half_quad_20x30"][0][2] % 4 == 2  # a row's last quad holds two pixels, at every subsampling


@pytest.mark.parametrize("k", (1, 2))
@pytest.mark.parametrize("name", sorted(GEOMETRIES))
def test_five_frames_in_one_launch_equal_the_definition_and_the_tile_kernel(name, k):
    g = geometry(name)
    track = track_degrees(N, k)
    mats = mats_of_track(track)
    tiles = [nat.Plan(g.dstp, g.plan_mats + list(mats[f]), g.srcp, bilinear=False) for f in range(N)]  # prepared plans of the whole chains
    compared = ran = 0
    for fmt in formats_of(g.dst, g.src):
        sub = sub_of(fmt)
        for S, dt in SAMPLES:
            frames = random_frames(N, g.h, g.w, sub, dt, seed=100 + 10 * S + FORMATS.index(fmt))
            for fill in ((0, 0, 0), (201, 77, 1 << (8 * S - 1))):
                got = run(g.plan, mats, frames, fmt, fill)  # ONE launch of the five frames
                want = g.expected(track, frames, sub, fill)
                for f in range(N):
                    bad = [int((a != b).sum()) for a, b in zip(ref.planes(got[f], g.Hd, g.Wd, sub), ref.planes(want[f], g.Hd, g.Wd, sub))]
                    assert got.dtype == want.dtype and bad == [0, 0, 0], (name, k, fmt, S, fill, f, bad)
                ran += 1
            # ... equals pb_stitch_planar / pb_stitch_nv12 of a prepared plan of the whole chain, wherever it is served
            fill = (201, 77, 1 << (8 * S - 1))
            for f in range(N):
                if fmt == "nv12" and tiles[f].stitch_nv12_supported(S):
                    one = tiles[f].stitch_nv12(torch.from_numpy(ref.nv12_of(frames[f], g.h, g.w).reshape(3 * g.h // 2, g.w)).cuda(), fill=fill).cpu().numpy()
                    assert np.array_equal(got[f], planar_of(one.reshape(1, -1), g.Hd, g.Wd)[0]), (name, k, fmt, S, f)
                    compared += 1
                elif fmt != "nv12" and tiles[f].stitch_planar_supported(sub, S):
                    one = tiles[f].stitch_planar(torch.from_numpy(frames[f]).cuda(), sub, fill=fill).cpu().numpy()
                    assert np.array_equal(got[f], one), (name, k, fmt, S, f)
                    compared += 1
            if fmt == "nv12":  # NV12 is yuv420p interleaved
                assert_same(run(g.plan, mats, frames, "nv12", (1, 2, 3)), run(g.plan, mats, frames, "420", (1, 2, 3)), f"{name} nv12 S={S}")
    assert ran == 4 * len(formats_of(g.dst, g.src)) and compared >= 1, (ran, compared)
    # 4:4:4 uint8, fill 0: the three planes are the three channels of pb_remap_track_u8's frames
    frames = random_frames(N, g.h, g.w, "444", np.uint8, seed=150)
    rgb = torch.from_numpy(np.ascontiguousarray(frames.reshape(N, 3, g.h, g.w).transpose(0, 2, 3, 1))).cuda()
    want = g.plan.remap_track(rgb, mats).permute(0, 3, 1, 2).contiguous().cpu().numpy().reshape(N, -1)
    assert_same(run(g.plan, mats, frames, "444", (0, 0, 0)), want, f"{name} remap_track")


@pytest.mark.parametrize("name", sorted(GOLDEN))
def test_the_fixture_s_four_frames_are_the_reference_s_own_output(name):
    case, g = GOLDEN[name], geometry(name)
    assert list(case.plan_rot) == list(g.plan_rot)
    mats = mats_of_track(case.frames)
    images = rc.case_frames(case)  # (4, h, w, 3) uint8
    frames = np.ascontiguousarray(images.transpose(0, 3, 1, 2)).reshape(4, -1)
    got = run(g.plan, mats, frames, "444", (0, 0, 0)).reshape(4, 3, g.Hd, g.Wd).transpose(0, 2, 3, 1)
    assert_same(got, g.plan.remap_track(torch.from_numpy(images).cuda(), mats).cpu().numpy(), f"{name} remap_track")
    if H.live_numpy_is_the_goldens_numpy():
        want = np.stack([GOLD[f"{name}/{f}/u8"] for f in range(4)])
    else:  # (the fixture's taps: a fragile pixel of this host's oracle may differ from it, never from the device)
        want = np.stack([np.stack(ref.stitch_planar(images[f][..., 0], images[f][..., 1], images[f][..., 2], *t, g.w, "444", (0, 0, 0)), axis=2)
                         for f, t in enumerate(g.taps(case.frames))])
    assert_same(got, want, f"{name} golden")
    # the same frames through the facade: typed arrays in and out, at 4:4:4 (3, h, w) frames too
    out = g.plan.stitch_track_planar(torch.from_numpy(frames.reshape(4, 3, g.h, g.w)).cuda(), mats[:, 0], "444", fill=(0, 0, 0))
    assert tuple(out.shape) == (4, 3, g.Hd, g.Wd) and np.array_equal(out.cpu().numpy().transpose(0, 2, 3, 1), want)


# ---- 2. plan states, layouts, one frame ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FORMATS)
def test_every_plan_state_pitched_swapped_and_offset_frames_and_one_frame(fmt):
    g = geometry("odd_half_width_40x82")
    sub = sub_of(fmt)
    track = track_degrees(N, 1)
    mats = mats_of_track(track)
    faithful = nat.Plan(g.dstp, g.plan_mats, g.srcp, bilinear=False)
    faithful.set_mode(nat.MODE_FAITHFUL)
    states = {"deferred": g.plan, "prepared": nat.Plan(g.dstp, g.plan_mats, g.srcp, bilinear=False), "faithful": faithful}
    for S, dt in SAMPLES:
        unit = 2 * S if fmt == "nv12" else S  # what pitches, offsets and pointers are multiples of
        frames = random_frames(N, g.h, g.w, sub, dt, seed=200 + S)
        want = g.expected(track, frames, sub, ref.default_fill(dt))
        for what, plan in states.items():
            assert_same(run(plan, mats, frames, fmt), want, f"{what} {fmt} S={S}")
        pitched = dict(pitch_pad=3 * unit, gap1=5 * unit, stride_pad=7 * unit) if fmt == "nv12" else dict(pitch_pad=6 * S, cpitch_pad=3 * S, gap1=5 * S, gap2=S, stride_pad=7 * S)
        assert_same(run(g.plan, mats, frames, fmt, None, pitched, pitched), want, f"pitched {fmt} S={S}")
        assert_same(run(g.plan, mats, frames, fmt, None, None, dict(stride_pad=unit)), want, f"padded stride {fmt} S={S}")
        assert_same(run(g.plan, mats, frames, fmt, None, None, None, unit), want, f"off a wide store {fmt} S={S}")
        if fmt != "nv12":
            swapped = dict(swap=True, gap2=3 * S)
            assert_same(run(g.plan, mats, frames, fmt, None, swapped, swapped), want, f"swapped planes {fmt} S={S}")
        # one frame; four: exactly a chunk
        assert_same(run(g.plan, mats[:1], frames[:1], fmt), want[:1], f"n = 1 {fmt} S={S}")
        assert_same(run(g.plan, mats[:F], frames[:F], fmt), want[:F], f"n = {F} {fmt} S={S}")
        # the facade: typed arrays in and out
        if fmt == "nv12":
            semi = torch.from_numpy(interleaved(frames, g.h, g.w).reshape(N, 3 * g.h // 2, g.w)).cuda()
            got = g.plan.stitch_track_nv12(semi, mats[:, 0])
            assert got.dtype == nat.torch_dtype(dt) and tuple(got.shape) == (N, 3 * g.Hd // 2, g.Wd)
            assert np.array_equal(planar_of(got.cpu().numpy().reshape(N, -1), g.Hd, g.Wd), want), S
        else:
            got = g.plan.stitch_track_planar(torch.from_numpy(frames).cuda(), mats[:, 0], sub)
            assert got.dtype == nat.torch_dtype(dt) and np.array_equal(got.cpu().numpy(), want), (fmt, S)
    with pytest.raises(ValueError, match="the table holds"):
        if fmt == "nv12":
            g.plan.stitch_track_nv12(semi, mats[: N - 1])
        else:
            g.plan.stitch_track_planar(torch.from_numpy(frames).cuda(), mats[: N - 1], sub)


# ---- 3. graph capture ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FORMATS)
def test_a_captured_launch_gives_the_plain_bytes(fmt):
    g = geometry("stereographic_36x36")
    sub, S = sub_of(fmt), 1
    mats = mats_of_track(track_degrees(N, 1))
    frames = random_frames(N, g.h, g.w, sub, np.uint8, seed=300)
    host = interleaved(frames, g.h, g.w) if fmt == "nv12" else frames
    src, table = torch.from_numpy(np.ascontiguousarray(host)).cuda(), torch.from_numpy(mats).cuda()
    nd = N * ref.frame_samples(g.Hd, g.Wd, sub)
    want = torch.zeros(nd, dtype=torch.uint8, device="cuda")
    assert track_call(g.plan, table, 1, src.data_ptr(), want.data_ptr(), N, fmt, S) == 0
    torch.cuda.synchronize()
    g_out = torch.zeros(nd, dtype=torch.uint8, device="cuda")
    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            assert track_call(g.plan, table, 1, src.data_ptr(), g_out.data_ptr(), N, fmt, S, stream=int(side.cuda_stream)) == 0
    torch.cuda.current_stream().wait_stream(side)
    g_out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(g_out, want) and bool((want != 0).any())


# ---- 4. the refusals -------------------------------------------------------------------------------------------------------------------------
def test_the_refusals_write_nothing():
    L = nat.load()
    g = geometry("T_double_195")
    table = torch.from_numpy(mats_of_track(track_degrees(2, 1))).cuda()
    frames = torch.from_numpy(random_frames(2, g.h, g.w, "444", np.uint8, seed=400)).cuda()
    buf = torch.full((2 * 3 * g.Hd * g.Wd,), SENTINEL, dtype=torch.uint8, device="cuda")
    for fmt in FORMATS:
        name = b"pb_track_stitch_nv12" if fmt == "nv12" else b"pb_track_stitch_planar"

        def call(plan=g.plan, tab_ptr=table.data_ptr(), k=1, S=1, n=2, dl=None):
            cls = nat.pb_nv12_layout if fmt == "nv12" else nat.pb_planar_layout
            d = None if dl is None else cls(*dl)
            args = [plan.handle, tab_ptr, k, frames.data_ptr(), buf.data_ptr(), n, None, None if d is None else nat.C.addressof(d)]
            return (L.pb_track_stitch_nv12 if fmt == "nv12" else L.pb_track_stitch_planar)(*args, *([] if fmt == "nv12" else [SUBS[fmt]]), S, None, nat.current_stream())

        # the table's checks are pb_remap_track_u8's
        assert call(tab_ptr=None) == INVALID and L.pb_last_error() == b"null rotation table"
        assert call(tab_ptr=table.data_ptr() + 4) == INVALID and b"8-byte aligned" in L.pb_last_error()
        assert call(k=0) == INVALID and b"n_rot_per_frame" in L.pb_last_error()
        assert call(k=nat.PB_MAX_ROTATIONS + 1) == INVALID and b"PB_MAX_ROTATIONS" in L.pb_last_error()
        assert call(S=3) == INVALID and call(n=-1) == INVALID
        assert call(n=0) == 0
        # frames that span 2^31 bytes; a single source
        assert call(dl=(1 << 30,) + (0,) * (2 if fmt == "nv12" else 4)) == UNSUPPORTED and name + b" takes frames whose planes span less than 2^31 bytes" in L.pb_last_error()
        dstp, srcp = projections(g.dst, pano(g.h, g.w))
        for single in (nat.Plan(dstp, [], srcp, defer=True), nat.Plan(dstp, [], srcp, bilinear=False)):
            assert call(plan=single) == UNSUPPORTED
            assert L.pb_last_error() == name + b" takes double-fisheye sources: use " + name.replace(b"pb_track_stitch", b"pb_remap_track") + b" for a single source"
    # the tracked calls of a single source keep refusing the double fisheye
    assert L.pb_remap_track_planar(g.plan.handle, table.data_ptr(), 1, frames.data_ptr(), buf.data_ptr(), 2, None, None, SUBS["444"], 1, None, nat.current_stream()) == UNSUPPORTED
    assert b"single sources" in L.pb_last_error()
    torch.cuda.synchronize()
    assert bool((buf == SENTINEL).all())


# ---- 5. the command ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["nv12", "p010", "yuv420p", "yuv422p10le", "gbrp"])
def test_the_command_s_five_frames_in_chunks_of_four_equal_the_plan_call(tmp_path, fmt):
    rad = pb.utils.to_radians
    h, w, Hd, Wd, rot = 40, 80, 34, 72, (3, 90, -7)
    dt, fam, fill = nat.VIDEO_FORMATS[fmt]
    nb = int(np.prod(fam.packed(h, w)[0])) * dt.itemsize
    frames = np.random.default_rng(500).integers(0, 256, (N, nb), dtype=np.uint8).view(dt)
    inp, out, track = tmp_path / "in.yuv", tmp_path / "out.yuv", tmp_path / "track.txt"
    frames.tofile(inp)
    degrees = DEGREES[:N] + [(9, 9, 9)]  # (a track may be longer than the input)
    track.write_text("# pitch yaw roll\n" + "".join(f"{a} {b} {c}\n" for a, b, c in degrees))
    args = [inp, out, "--width", w, "--height", h, "--pix-fmt", fmt, "--lens", "equidistant", "--fov", 195, "--out-width", Wd, "--out-height", Hd, "-r", *rot, "--chunk", 4,
            "--rotations", track]
    res = CliRunner().invoke(cli.main, ["stitch-track-yuv", *map(str, args)])
    assert res.exit_code == 0, (res.output, res.exception)
    cmap = pb.Rotation(*map(rad, rot)).rotate_coordinate_map(pb.PanoramaImage(np.zeros((Hd, Wd, 3), np.uint8)).get_coordinate_map())
    src = pb.DoubleCameraImage(np.zeros((h, w, 3), np.uint8), rad(195), pb.equidistant())
    plan = nat.Plan(cmap.dst_proj, list(cmap.rotations), src._proj(), defer=True)
    s = torch.from_numpy(frames.reshape((N,) + fam.packed(h, w)[0])).cuda()
    mats = mats_of(degrees[:N])
    want = (plan.stitch_track_nv12(s, mats) if fam.pairs else plan.stitch_track_planar(s, mats, fam.sub, fill=fill)).cpu().numpy().reshape(N, -1)
    got = np.fromfile(out, dt)
    assert got.size == want.size and np.array_equal(got.reshape(want.shape), want)
    assert not np.array_equal(want[0], want[1])
    # ... and frame 2 is what stitch-yuv's plan call writes for that frame's whole chain
    whole = pb.Rotation(*map(rad, degrees[2])).rotate_coordinate_map(cmap)
    tile = nat.Plan(whole.dst_proj, list(whole.rotations), src._proj(), bilinear=False)
    one = (tile.stitch_nv12(s[2:3]) if fam.pairs else tile.stitch_planar(s[2:3], fam.sub, fill=fill)).cpu().numpy().reshape(-1)
    assert np.array_equal(want[2], one)
