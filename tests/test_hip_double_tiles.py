"""pb_remap_u8 of a double-fisheye source - pb_hot_double_kernel (WMODE 0 / 1 / 2, its VEC form), pb_sep_double_kernel and the float64
pb_remap_kernel - against the CPU ORACLE's bytes: tests/double_cases.py's definition fed with the oracle's taps and factors (the fixture
tests/golden/double_tiles.npz for the edge shapes, a live run for the mid cases), on independent random bytes and on the constant frame
that shows a blend factor's last bit (tests/test_double_cases_host.py proves both claims on the CPU).  Every comparison is exact equality;
every destination sits between sentinel bytes that must survive; Plan.stitch_tile_mix proves that the lists reach every path.  The
video stitch kernels, which load the same factors through code of their own, get the constant frame too."""

import numpy as np
import pytest
import torch

from oracle import reference_path as orc
from photonbend_amd import _native as nat
from tests import double_cases as dc
from tests import helpers as H
from tests import stitch_video_ref as ref
from tests.test_hip_nv12 import GUARD, SENTINEL, guarded, guards_intact
from tests.test_hip_stitch_video import run as stitch_run
from tests.test_hip_track_nv12 import mats_of, projections
from tests.test_hip_track_stitch import run as track_run
from tests.test_track_stitch_ref_host import chain_taps

pytestmark = pytest.mark.gpu

MODES = {"auto": nat.MODE_AUTO, "fast": nat.MODE_FAST, "fast_direct": nat.MODE_FAST_DIRECT, "faithful": nat.MODE_FAITHFUL}
MIX = {}   # case name -> Plan.stitch_tile_mix(), filled by sections a and b, read by section c after them (file order)
INFO = {}  # case name -> Plan.info()
_WANT = {}


def plan_of(case):
    return H.pb_plan_private(case, bilinear=False)


def record(case, plan):
    MIX[case.name], INFO[case.name] = plan.stitch_tile_mix(), plan.info()
    print(f"{case.name}: fast_path {INFO[case.name]['fast_path']}, tile mix {MIX[case.name]}")


def edge_want(case, kind):
    """The oracle's bytes of an EDGES case (the fixture's taps: exact on any host), computed once."""
    if (case.name, kind) not in _WANT:
        _WANT[case.name, kind] = dc.stitch_rgb(dc.frames_of(case)[kind], *dc.fixture_taps(case), case.src[2])
    return _WANT[case.name, kind]


def aligned_source(frame, off=0):
    """-> (the device buffer, the address of the frame's copy in it: `off` bytes past a 256-byte boundary)."""
    flat = np.ascontiguousarray(frame).reshape(-1)
    buf = torch.zeros(flat.size + 512, dtype=torch.uint8, device="cuda")
    s_off = (-buf.data_ptr()) % 256 + off
    buf[s_off : s_off + flat.size] = torch.from_numpy(flat).cuda()
    return buf, buf.data_ptr() + s_off


def launch(plan, src_ptr, dst_ptr, n=1, ss=0, ds=0, stream=None):
    nat.check(nat.load().pb_remap_u8(plan.handle, src_ptr, dst_ptr, n, ss, ds, nat.current_stream() if stream is None else stream))


def run(plan, frame, s_off=0, d_off=0, launches=1):
    """`launches` packed single-frame pb_remap_u8 launches with a synchronisation after each, every one into a fresh guarded buffer ->
    the (H, W, 3) outputs.  Everything outside a payload keeps its sentinel."""
    Hd, Wd = plan.dst.height, plan.dst.width
    nd = Hd * Wd * 3
    keep, src = aligned_source(frame, s_off)
    outs = []
    for _ in range(launches):
        buf = guarded(nd + d_off)
        launch(plan, src, buf.data_ptr() + GUARD + d_off)
        torch.cuda.synchronize()
        host = buf.cpu().numpy()
        assert bool((host[: GUARD + d_off] == SENTINEL).all()) and bool((host[GUARD + d_off + nd :] == SENTINEL).all()), "the launch wrote outside the destination frame"
        outs.append(host[GUARD + d_off : GUARD + d_off + nd].reshape(Hd, Wd, 3))
    del keep
    return outs


def assert_bytes(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype == np.uint8, (what, got.shape, want.shape)
    bad = got != want
    assert not bad.any(), f"{what}: {int(bad.sum())} bytes in {int(bad.any(axis=2).sum())} pixels differ from the oracle's"


def assert_taps(case, plan, il, ir, fl, fr):
    """Plan.index_map(weights=True) - the taps and factors the device's chain gives - are the oracle's: the indices equal, the factors
    bit for bit (NaN with NaN counts as equal)."""
    Hd, Wd = case.dst[1], case.dst[2]
    idx, wts = plan.index_map(weights=True)
    idx, wts = idx.reshape(2, Hd, Wd).cpu().numpy(), wts.reshape(2, Hd, Wd).cpu().numpy()
    assert np.array_equal(idx[0], il) and np.array_equal(idx[1], ir), (case.name, int((idx[0] != il).sum()), int((idx[1] != ir).sum()))
    for name, got, want in (("fl", wts[0], fl), ("fr", wts[1], fr)):
        same = (H.bits(got) == H.bits(want)) | (np.isnan(got) & np.isnan(want))
        assert same.all(), f"{case.name}: {int((~same).sum())} factors {name} are not the oracle's bits"


# ---- a. the edge shapes against the fixture, both frames, the four modes -------------------------------------------------------------------
@pytest.mark.parametrize("case", dc.EDGES, ids=lambda c: c.name)
def test_edges_are_the_oracle_s_bytes_in_every_mode(case):
    plan = plan_of(case)
    record(case, plan)
    frames = dc.frames_of(case)
    for mode, m in MODES.items():
        plan.set_mode(m)
        if mode in ("auto", "faithful"):
            assert_taps(case, plan, *dc.fixture_taps(case))
        for kind, frame in frames.items():
            # FAST_DIRECT: the first launch runs the float64 kernel behind the separable tables' check, a later one pb_sep_double_kernel
            for k, got in enumerate(run(plan, frame, launches=2 if mode == "fast_direct" else 1)):
                assert_bytes(got, edge_want(case, kind), f"{case.name} {mode} {kind} frame, launch {k}")


# ---- b. the mid cases against the live oracle ---------------------------------------------------------------------------------------------
def mid_taps(case, plan):
    """-> (il, ir, fl, fr, exact).  Where the live NumPy is the goldens' NumPy: the oracle's, and the comparison is exact - the form that
    counts.  Elsewhere the suite's rule: the plan's own taps and factors, which must be the oracle's outside its fragile set and within
    tests/test_hip_parity.py's allowance."""
    il, ir, fl, fr = dc.oracle_taps(case)
    if H.live_numpy_is_the_goldens_numpy():
        return il, ir, fl, fr, True
    Hd, Wd = case.dst[1], case.dst[2]
    idx, wts = plan.index_map(weights=True)
    idx, wts = idx.reshape(2, Hd, Wd).cpu().numpy(), wts.reshape(2, Hd, Wd).cpu().numpy()
    with np.errstate(all="ignore"):
        fragile = orc.fragile_mask(orc.pretrunc(H.orc_proj(case.dst), H.orc_proj(case.src), H.orc_rots(case)))
        assert not ((idx[0] != il) & ~fragile).any() and not ((idx[1] != ir) & ~fragile).any(), case.name
        for got, want in ((wts[0], fl), (wts[1], fr)):
            assert ((got == want) | (np.isnan(got) & np.isnan(want)) | (np.abs(got - want) <= 1e-12 * np.abs(want))).all(), case.name
    print(f"{case.name}: this host's NumPy is not the goldens' NumPy - the EXACT oracle form did not run; compared with the plan's own taps and factors")
    return idx[0], idx[1], wts[0], wts[1], False


@pytest.mark.parametrize("case", dc.MID, ids=lambda c: c.name)
def test_mid_cases_are_the_oracle_s_bytes(case):
    plan = plan_of(case)
    record(case, plan)
    assert INFO[case.name]["fast_path"] and INFO[case.name]["tiles"] > 0, case.name
    *taps, exact = mid_taps(case, plan)
    print(f"{case.name}: the exact oracle form {'ran' if exact else 'DID NOT run'}")
    frames = dc.frames_of(case)
    want = {kind: dc.stitch_rgb(frame, *taps, case.src[2]) for kind, frame in frames.items()}
    for mode, m in MODES.items():
        plan.set_mode(m)
        if exact and mode in ("auto", "faithful"):
            assert_taps(case, plan, *taps)
        for kind in (("random", "constant") if mode == "auto" else ("random",)):
            for k, got in enumerate(run(plan, frames[kind], launches=2 if mode == "fast_direct" else 1)):
                assert_bytes(got, want[kind], f"{case.name} {mode} {kind} frame, launch {k}")


# ---- c. the lists reach every path --------------------------------------------------------------------------------------------------------
def wmode_of(case, mix):
    """The WMODE instantiation of pb_hot_double_kernel a plan launches: 1 with the separable path's row table (an unrotated panorama
    destination), else 2 with stored latitudes, else 0."""
    if case.dst[0] == "pano" and not case.rotations:
        return 1
    return 2 if mix["lat"] else 0


def test_the_cases_reach_every_path_of_the_kernels():
    """Runs after sections a and b and reads what they recorded; a case they did not run is classified here."""
    cases = dc.EDGES + dc.MID
    for case in cases:
        if case.name not in MIX:
            record(case, plan_of(case))
    keys = list(next(iter(MIX.values())))
    total = {k: sum(m[k] for m in MIX.values()) for k in keys}
    print("stitch_tile_mix per geometry (the RGB launch walks the same launch-order table):")
    for case in cases:
        i = INFO[case.name]
        print(f"  {case.name:24s} WMODE {wmode_of(case, MIX[case.name])} fast_path {i['fast_path']} lean {i['lean_tiles']} direct {i['direct_tiles']} {MIX[case.name]}")
    print(f"  {'total':24s} {total}")
    for path in ("solo", "unit", "row", "lat", "failed", "fix_tiles", "fix_pixels"):
        assert total[path] > 0, f"no case of the lists reaches the kernel's {path} path: {total}"
    assert all("fast_path" in INFO[c.name] for c in cases)
    assert sum(INFO[c.name]["lean_tiles"] for c in cases) > 0 and sum(INFO[c.name]["direct_tiles"] for c in cases) > 0
    # the three WMODE instantiations, each on a plan whose tile kernel is the route
    tiled = [c for c in cases if INFO[c.name]["fast_path"] and INFO[c.name]["tiles"] > 0]
    by_wmode = {w: [c.name for c in tiled if wmode_of(c, MIX[c.name]) == w] for w in (0, 1, 2)}
    print(f"  WMODE -> cases: {by_wmode}")
    assert set(dc.UNIT_ONLY) & set(by_wmode[0]) and all(MIX[n]["row"] == 0 and MIX[n]["lat"] == 0 for n in by_wmode[0])
    assert "stitch_195_aligned" in by_wmode[1] and MIX["stitch_195_aligned"]["row"] > 0
    assert "stitch_195_rot" in by_wmode[2] and MIX["stitch_195_rot"]["lat"] > 0
    assert MIX["edge_96x192_row_band"]["row"] > 0 and MIX["edge_96x192_lat_band"]["lat"] > 0


# ---- d. store paths: the destination 0 .. 3 bytes off a dword ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["edge_33x65_rot", "stitch_195_aligned"])
def test_a_destination_off_dword_alignment_gets_the_same_payload(name):
    case = dc.case_by_name(name)
    plan = plan_of(case)
    frame = dc.frames_of(case)["random"]
    want = edge_want(case, "random") if case in dc.EDGES else None
    first = None
    for d_off in (0, 1, 2, 3):
        (got,) = run(plan, frame, s_off=0, d_off=d_off)  # (the source stays 16-byte aligned: the route stays the tile kernel)
        first = got if first is None else first
        assert np.array_equal(got, first), (name, d_off)
        if want is not None:
            assert_bytes(got, want, f"{name} destination offset {d_off}")
    if want is None:
        *taps, exact = mid_taps(case, plan)
        assert_bytes(first, dc.stitch_rgb(frame, *taps, case.src[2]), name)


# ---- e. sources the windows cannot take -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["edge_96x192_row_band", "edge_96x192_lat_band"])
def test_a_source_off_16_byte_alignment_gets_the_oracle_s_bytes(name):
    """Unrotated: the separable route - the float64 kernel on the first launch, pb_sep_double_kernel once the tables' check has passed.
    Rotated: the float64 kernel."""
    case = dc.case_by_name(name)
    plan = plan_of(case)
    for s_off in (1, 7):
        for k, got in enumerate(run(plan, dc.frames_of(case)["random"], s_off=s_off, launches=3)):
            assert_bytes(got, edge_want(case, "random"), f"{name} source offset {s_off}, launch {k}")


# ---- f. batches -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["edge_96x192_row_band", "edge_96x192_lat_band"])
def test_five_frames_at_padded_strides_equal_five_single_launches_and_the_vec_form(name):
    case = dc.case_by_name(name)
    plan = plan_of(case)
    _, h, w, *_ = case.src
    Hd, Wd = case.dst[1], case.dst[2]
    n, n_src, n_dst = 5, h * w * 3, Hd * Wd * 3
    ss, ds = n_src + 48, n_dst + 5
    assert n_src % 16 == 0 and ss % 16 == 0 and ds % 4
    frames = [dc.random_rgb(h, w, seed=7100 + f) for f in range(n)]
    host = np.random.default_rng(7105).integers(0, 256, n * ss, dtype=np.uint8)  # (random bytes in the padding too)
    for f in range(n):
        host[f * ss : f * ss + n_src] = frames[f].reshape(-1)
    keep, src = aligned_source(host)
    buf = guarded(n * ds)
    launch(plan, src, buf.data_ptr() + GUARD, n, ss, ds)
    torch.cuda.synchronize()
    assert guards_intact(buf)
    got = buf[GUARD:-GUARD].cpu().numpy()
    singles = [run(plan, frames[f])[0] for f in range(n)]
    for f in range(n):
        assert np.array_equal(got[f * ds : f * ds + n_dst].reshape(Hd, Wd, 3), singles[f]), (name, f)
        assert bool((got[f * ds + n_dst : (f + 1) * ds] == SENTINEL).all()), (name, f)  # the padding between output frames is intact
    taps = dc.fixture_taps(case)
    for f in (0, 4):
        assert_bytes(singles[f], dc.stitch_rgb(frames[f], *taps, w), f"{name} frame {f}")
    assert not np.array_equal(singles[0], singles[4])
    # the same frames as separately allocated tensors: pb_remap_u8v, the kernel's VEC form
    bufs = [guarded(n_dst) for _ in range(n)]
    outs = [b[GUARD:-GUARD].view(Hd, Wd, 3) for b in bufs]
    plan.remap_each([torch.from_numpy(f).cuda() for f in frames], outs)
    torch.cuda.synchronize()
    for f in range(n):
        assert guards_intact(bufs[f]) and np.array_equal(outs[f].cpu().numpy(), singles[f]), (name, f)


# ---- g. graph capture and streams ---------------------------------------------------------------------------------------------------------
def test_a_captured_launch_and_launches_on_three_streams_give_the_plain_bytes():
    case = dc.case_by_name("stitch_195_rot")
    plan = plan_of(case)
    Hd, Wd = case.dst[1], case.dst[2]
    frame = dc.frames_of(case)["random"]
    keep, src = aligned_source(frame)
    (plain,) = run(plan, frame)
    *taps, exact = mid_taps(case, plan)
    assert_bytes(plain, dc.stitch_rgb(frame, *taps, case.src[2]), case.name)
    want = torch.from_numpy(plain.copy()).cuda()
    # never allocates or synchronises: the call captures into a graph, and a replay writes the frame again
    g_out = torch.zeros((Hd, Wd, 3), dtype=torch.uint8, device="cuda")
    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            launch(plan, src, g_out.data_ptr(), stream=int(side.cuda_stream))
    torch.cuda.current_stream().wait_stream(side)
    g_out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(g_out, want)
    streams = [torch.cuda.Stream() for _ in range(3)]
    outs = [torch.zeros((Hd, Wd, 3), dtype=torch.uint8, device="cuda") for _ in streams]
    torch.cuda.synchronize()
    for s, o in zip(streams, outs):
        launch(plan, src, o.data_ptr(), stream=int(s.cuda_stream))
    torch.cuda.synchronize()
    assert all(torch.equal(o, want) for o in outs)


# ---- h. the video stitch on the constant frame ---------------------------------------------------------------------------------------------
def constant_planes(h, w, dt):
    values = dc.PROBE if np.dtype(dt).itemsize == 1 else dc.PROBE16
    return np.repeat(np.array(values, dt), h * w)  # a packed 4:4:4 frame, constant per plane


@pytest.mark.parametrize("name", ["edge_96x192_row_band", "edge_96x192_lat_band", "stitch_195_rot", "edge_33x64_fov180_nan"])
def test_the_video_stitch_shows_the_factors_last_bit_on_a_constant_frame(name):
    """pb_stitch_planar at 4:4:4 loads the row weights, the stored latitudes and the stored factors through its own code.  (The fov-180
    edge: a row of NaN factors in the row table - the tile whose weight class the RGB launch once got wrong.)"""
    case = dc.case_by_name(name)
    plan = plan_of(case)
    _, h, w, *_ = case.src
    if case in dc.EDGES:
        taps = dc.fixture_taps(case)
    else:
        *taps, exact = mid_taps(case, plan)
    for dt in (np.uint8, np.uint16):
        frame = constant_planes(h, w, dt)
        got = stitch_run(plan, frame, "444", (0, 0, 0))
        want = ref.stitch_frame(frame, *taps, h, w, "444", (0, 0, 0))
        assert got.dtype == want.dtype and np.array_equal(got, want), (name, np.dtype(dt).name, int((got != want).sum()))


# ---- i. the tracked video stitch on the constant frame ------------------------------------------------------------------------------------
def test_the_tracked_video_stitch_shows_the_factors_last_bit_on_a_constant_frame():
    """One pb_track_stitch_planar call, two frames: the identity and (3, 90, -7), against the oracle of the two composed chains."""
    case = dc.case_by_name("stitch_195_aligned")
    _, h, w, *_ = case.src
    track = [[(0, 0, 0)], [(3, 90, -7)]]
    dstp, srcp = projections(case.dst, case.src)
    plan = nat.Plan(dstp, [], srcp, defer=True)
    mats = mats_of([r for fr in track for r in fr]).reshape(2, 1, 3, 3)
    frames = np.stack([constant_planes(h, w, np.uint8)] * 2)
    got = track_run(plan, mats, frames, "444", (0, 0, 0))
    for f, chain in enumerate(track):
        if H.live_numpy_is_the_goldens_numpy():
            taps = chain_taps(case.dst, case.src, chain)
        else:  # (the float64 chain's own taps, as tests/test_hip_track_stitch.py does on such a host)
            print("this host's NumPy is not the goldens' NumPy - the EXACT oracle form did not run")
            faithful = nat.Plan(dstp, list(mats[f]), srcp, defer=True)
            faithful.set_mode(nat.MODE_FAITHFUL)
            idx, wts = faithful.index_map(weights=True)
            idx, wts = idx.cpu().numpy(), wts.cpu().numpy()
            taps = (idx[0], idx[1], wts[0], wts[1])
        want = ref.stitch_frame(frames[f], *taps, h, w, "444", (0, 0, 0))
        assert np.array_equal(got[f], want), (f, int((got[f] != want).sum()))
    assert not np.array_equal(got[0], got[1])
