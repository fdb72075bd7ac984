"""The Catmull-Rom tile kernel (pb_catmull_rom_hot_kernel) held to the checks that made the bilinear tile kernel trustworthy,
and both interpolating tile kernels on random geometries with cube destinations and polynomial lenses (tests/interp_cases.py; the
conditions on those inputs: tests/test_interp_cases_host.py).

Every comparison with a definition - tests/catmull_rom_ref.py, oracle.reference_path.remap_bilinear, both from the float64 map
tests/cubemap_cases.ref_stages gives - is of EVERY pixel, on a frame of independent random texels (255 LSB per pixel of coordinate error):
  * no channel further than 1 LSB from the definition: Catmull-Rom's budget of DESIGN 3.8 (0.93 LSB from coordinates certified to 1/1024 px,
    plus float32 rounding), bilinear's existing single-source bound;
  * a pixel black in one result and sampled in the other only inside interp_cases.edge_band(B = 1/512 px): within twice the certified
    bound of a camera source's frame edge, the one place where the two may legitimately decide differently.  (A geometric rule: not the
    count of `rim_flips` tests/test_hip_catmull_rom._within_one allows the older tests.)
How the frames reach a kernel - pointers, strides, batches, budgets, a restored plan, a captured graph, several streams - never moves a byte."""

import functools

import numpy as np
import pytest
import torch

from oracle import reference_path as orc
from photonbend_amd import _native as nat
from tests import catmull_rom_ref as crr
from tests import cubemap_cases as cc
from tests import helpers as H
from tests import interp_cases as ic
from tests.cases import Case, cam, inscribed

pytestmark = pytest.mark.gpu
CR = "catmull-rom"
BIL = "bilinear"
BAND = 1.0 / 512.0
SENTINEL = 0xA5


def _plan(case, **kw):
    src, cmap = cc.pb_chain(case, image=np.zeros((case.src[1], case.src[2], 3), np.uint8))
    kw.setdefault("bilinear", True)
    return nat.Plan(cmap.dst_proj, cmap.rotations, src._proj("src"), **kw)


@functools.lru_cache(maxsize=None)
def _ref(name):
    """The definitions of a case on its noise frame, computed once and shared (read-only): frame, Catmull-Rom, bilinear, edge band."""
    case = ic.by_name(name)
    final = ic.final_map(case)
    frame = ic.noise_frame(case)
    sp = ic.src_proj(case)
    with np.errstate(all="ignore"):
        want = {CR: crr.remap(None, sp, frame, cmap=np.copy(final)), BIL: orc.remap_bilinear(None, sp, frame, cmap=np.copy(final))}
    band = ic.edge_band(case, final, BAND)
    for a in (frame, want[CR], want[BIL], band):
        a.setflags(write=False)
    return frame, want, band


def _check(got, want, band, double_src, name):
    """The comparison rule of this file; returns the share of pixels 1 LSB off."""
    assert got.shape == want.shape and got.dtype == want.dtype, (name, got.shape, got.dtype, want.shape, want.dtype)
    d = np.abs(got.astype(np.int64) - want.astype(np.int64))
    if double_src:
        d = np.minimum(d, 256 - d)  # the blend's cast wraps mod 256 like the reference's
    d = d.max(axis=2)
    flips = (got == 0).all(axis=2) != (want == 0).all(axis=2)
    off = (d > 1) & ~(flips & band)
    where = np.argwhere(off)[:4].tolist()
    assert not off.any(), (f"{name}: {int(off.sum())} pixels beyond 1 LSB of the definition (max {int(d[off].max())}; {int((off & flips).sum())} of them black in one "
                           f"result and sampled in the other, outside the edge band), first at {where}: got {[got[y, x].tolist() for y, x in where]}, "
                           f"want {[want[y, x].tolist() for y, x in where]}")
    return float((d == 1).mean())


def _remap(plan, frame, interp):
    return plan.remap(torch.from_numpy(np.array(frame)).cuda(), interpolation=interp).cpu().numpy()


def _waves(shape):
    """Waves per bilinear workgroup.  The library launches groups x (4 / waves) workgroups per frame (pb_bil_groups) over a table of
    4 x groups slots; the LDS pool says which: 40448 bytes is the four-wave pool, every other pool (20224, 23392, twice the budget) a
    two-wave one (pb_build_bilinear_launch)."""
    return 4 if shape["lds_bytes"] == 40448 else 2


# ---- a. sixteen random geometries on noise frames -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ic.SWEEP, ids=ic.label)
def test_noise_sweep_both_tile_kernels_against_their_definitions(case):
    frame, want, band = _ref(case.name)
    plan = _plan(case)
    info, mix = plan.info(), plan.bilinear_tile_mix()
    assert info["fast_path"], info
    if info["tiles"] > 8:
        assert mix["entries"] > 0 and info["bilinear_float64_tiles"] == 0, (info, mix)  # (the tile kernels, not the float64 routes)
    shares = {}
    for interp in (CR, BIL):
        shares[interp] = _check(_remap(plan, frame, interp), want[interp], band, False, f"{case.name} {interp}")
    print(f"{ic.label(case)}: {info['tiles']} tiles, 1 LSB off: catmull-rom {100 * shares[CR]:.3f} %, bilinear {100 * shares[BIL]:.3f} % of the pixels; "
          f"{int(band.sum())} pixels in the edge band")
    # the same plan's float64 route IS the Catmull-Rom definition
    plan.set_mode(nat.MODE_FAITHFUL)
    got = _remap(plan, frame, CR)
    d = np.abs(got.astype(np.int16) - want[CR].astype(np.int16))
    assert int(d.max(initial=0)) <= 1, f"{case.name}: the float64 route is {int(d.max())} LSB from the definition"
    if H.live_numpy_is_the_goldens_numpy():
        assert int((d != 0).sum()) == 0, f"{case.name}: {int((d != 0).sum())} samples of the float64 route differ from the definition"


# ---- b. what the kernel branches on is all there ----------------------------------------------------------------------------------------------
# (fixed cases for classes the sweep and the magnified cases may lack)
COVERAGE_EXTRA = [
    # a plan that keeps FOUR-wave bilinear workgroups (every sweep and magnified plan takes two): minified by 1.3, the windows of two slots do
    # not fit the two-wave pool for more than 2 % of the tiles, those of four slots fit the four-wave pool
    Case("cov_four_waves", cam(384, 384, "stereographic", 200, inscribed(384)), cam(512, 512, "equisolid", 220, inscribed(512)), [(5, 10, 15)]),
    # a 360-degree equisolid rim under a rotation: window, table and TD3 entries and hundreds of fix pixels in one plan
    Case("cov_rim", cam(512, 512, "equisolid", 360, inscribed(512)), cam(512, 512, "equidistant", 360, inscribed(512)), [(30, 45, 10)]),
]


def test_the_cases_cover_every_tile_class_and_both_workgroup_shapes():
    rows, total = [], dict.fromkeys(("window", "direct", "table", "black", "td3", "entries"), 0)
    for case in ic.SWEEP + ic.MAGNIFIED + COVERAGE_EXTRA:
        plan = _plan(case)
        info, mix, shape = plan.info(), plan.bilinear_tile_mix(), plan.bilinear_launch_shape()
        waves = _waves(shape) if shape["workgroups"] else 0
        assert mix["entries"] <= waves * shape["workgroups"], (case.name, mix, shape)  # (every entry has a wave)
        rows.append((case.name, info["tiles"], info["fix_pixels"], mix, waves))
        for k in total:
            total[k] += mix[k]
    print(f"{'case':26s} {'tiles':>6s} {'fix px':>7s} {'window':>7s} {'direct':>7s} {'table':>6s} {'black':>6s} {'td3':>6s} {'waves':>5s}")
    for name, tiles, fix, mix, waves in rows:
        print(f"{name:26s} {tiles:6d} {fix:7d} {mix['window']:7d} {mix['direct']:7d} {mix['table']:6d} {mix['black']:6d} {mix['td3']:6d} {waves:5d}")
    print(f"{'sum':26s} {'':6s} {'':7s} {total['window']:7d} {total['direct']:7d} {total['table']:6d} {total['black']:6d} {total['td3']:6d}")
    assert total["window"] + total["direct"] > 0 and total["table"] > 0 and total["black"] > 0 and total["td3"] > 0, total
    assert any(fix > 0 and mix["window"] + mix["direct"] > 0 for _, _, fix, mix, _ in rows), "no plan with fix pixels next to modelled tiles"
    assert {2, 4} <= {waves for *_, waves in rows}, "the plans do not show both a two-wave and a four-wave bilinear workgroup"


@pytest.mark.parametrize("case", COVERAGE_EXTRA, ids=lambda c: c.name)
def test_coverage_cases_against_their_definitions(case):
    """The fixed cases that bring a tile class or a workgroup shape: compared like the sweep (the Catmull-Rom kernel reads a two-wave and a
    four-wave plan's launch table alike, four slots per workgroup)."""
    final = ic.final_map(case)
    frame = ic.noise_frame(case)
    band = ic.edge_band(case, final, BAND)
    plan = _plan(case)
    with np.errstate(all="ignore"):
        _check(_remap(plan, frame, CR), crr.remap(None, ic.src_proj(case), frame, cmap=np.copy(final)), band, False, case.name + " catmull-rom")
        _check(_remap(plan, frame, BIL), orc.remap_bilinear(None, ic.src_proj(case), frame, cmap=np.copy(final)), band, False, case.name + " bilinear")


# ---- c. frames of a few pixels, sources magnified many times -----------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ic.TINY + ic.MAGNIFIED, ids=lambda c: c.name)
def test_tiny_and_magnified_cases_against_their_definitions(case):
    """Every tap clamps or wraps (a source under 4 px a side never takes the 12-byte row load; a 2 x 4 panorama wraps a tap twice), a tile
    holds more pixels than the source, partial tiles, 1 x 1 outputs."""
    frame, want, band = _ref(case.name)
    plan = _plan(case)
    double = case.src[0] == "double"
    share = _check(_remap(plan, frame, CR), want[CR], band, double, case.name + " catmull-rom")
    share_b = _check(_remap(plan, frame, BIL), want[BIL], band, double, case.name + " bilinear")
    print(f"{case.name}: 1 LSB off: catmull-rom {100 * share:.3f} %, bilinear {100 * share_b:.3f} % of the pixels")


# ---- d. how the frames reach the kernel never moves a byte -------------------------------------------------------------------------------------
LAYOUT_CASES = ["mag_pano_from_cam", "mag_pano_pole_and_seam", "sweep10", "sweep11", ic.ODD_DST.name]
N_BATCH = 5
LEAD = 64  # bytes of padding before the first and behind the last frame of a buffer: no frame ends an allocation


def _embed_sources(frames, offset, stride, rng):
    """One device buffer of random NON-ZERO bytes with frame k at offset + k * stride: a tap read outside a frame changes a pixel."""
    n = frames[0].size
    host = rng.integers(1, 256, size=offset + stride * (len(frames) - 1) + n + LEAD, dtype=np.uint8)
    for k, f in enumerate(frames):
        host[offset + k * stride:offset + k * stride + n] = f.reshape(-1)
    return torch.from_numpy(host).cuda()


def _outputs_of(buf, offset, stride, count, shape, name):
    """The frames of a sentinel-filled output buffer; every byte outside them must still be the sentinel (a store past a partial tile shows)."""
    host = buf.cpu().numpy()
    m = int(np.prod(shape))
    mask = np.ones(host.size, bool)
    outs = []
    for k in range(count):
        mask[offset + k * stride:offset + k * stride + m] = False
        outs.append(host[offset + k * stride:offset + k * stride + m].reshape(shape))
    assert (host[mask] == SENTINEL).all(), f"{name}: {int((host[mask] != SENTINEL).sum())} bytes outside the output frames were written"
    return outs


@pytest.mark.parametrize("interp", [CR, BIL])
@pytest.mark.parametrize("name", LAYOUT_CASES)
def test_pointers_strides_batches_and_direct_mode_give_the_same_bytes(name, interp):
    """A source pointer one byte off (LDS-DMA cannot stage it; the Catmull-Rom rows load 12 bytes from any address), a destination pointer one
    byte off (the 12-byte stores fall back to bytes), five frames at strides padded by 3 and by 48 bytes, PB_MODE_FAST_DIRECT: the bytes of
    aligned single launches.  Sources lie in random non-zero bytes, outputs in a sentinel that must survive."""
    case = ic.by_name(name)
    plan = _plan(case)
    rng = np.random.default_rng(11)
    _, sh, sw, *_ = case.src
    shape = (case.dst[1], case.dst[2], 3)
    n, m = sh * sw * 3, int(np.prod(shape))
    frames = [rng.integers(0, 256, size=(sh, sw, 3), dtype=np.uint8) for _ in range(N_BATCH)]
    want = [_remap(plan, f, interp) for f in frames]
    assert any(w.any() for w in want) and not np.array_equal(want[0], want[1])

    def run(src_off, src_stride, dst_off, dst_stride, count, tag):
        sbuf = _embed_sources(frames[:count], src_off, src_stride, rng)
        dbuf = torch.full((dst_off + dst_stride * (count - 1) + m + LEAD,), SENTINEL, dtype=torch.uint8, device="cuda")
        plan.launch(sbuf.data_ptr() + src_off, dbuf.data_ptr() + dst_off, count, None, interp, src_stride=src_stride if count > 1 else 0,
                    dst_stride=dst_stride if count > 1 else 0)
        torch.cuda.synchronize()
        outs = _outputs_of(dbuf, dst_off, dst_stride, count, shape, f"{name} {interp} {tag}")
        for k in range(count):
            bad = int((outs[k] != want[k]).any(axis=2).sum())
            assert bad == 0, f"{name} {interp} {tag}: frame {k} differs from the aligned single launch in {bad} pixels"

    assert torch.empty(1, dtype=torch.uint8, device="cuda").data_ptr() % 16 == 0  # (allocations are aligned: an offset of LEAD + 1 is odd)
    run(LEAD, n, LEAD, m, 1, "embedded, aligned")
    run(LEAD + 1, n, LEAD, m, 1, "source pointer + 1")
    run(LEAD, n, LEAD + 1, m, 1, "destination pointer + 1")
    for pad in (3, 48):
        run(LEAD, n + pad, LEAD, m + pad, N_BATCH, f"batch of {N_BATCH}, strides + {pad}")
    run(LEAD + 1, n + 3, LEAD + 1, m + 3, N_BATCH, f"batch of {N_BATCH}, both pointers + 1, strides + 3")
    plan.set_mode(nat.MODE_FAST_DIRECT)
    run(LEAD, n, LEAD, m, 1, "MODE_FAST_DIRECT")
    run(LEAD, n + 48, LEAD, m + 48, N_BATCH, "MODE_FAST_DIRECT, batch")


# ---- e. re-budgeted and restored plans --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sweep7", "sweep12"])
def test_rebudgeted_and_restored_plans_give_the_same_bytes(name):
    """pb_plan_set_window_budget re-deals the nearest mode's tiles and rebuilds the launch tables in place; a blob restores a plan without
    re-certifying.  Neither may change a byte of either interpolating mode, nor how the bilinear tables serve the tiles."""
    case = ic.by_name(name)
    frame, _, _ = _ref(name)
    dev = torch.from_numpy(np.array(frame)).cuda()
    plan = _plan(case)
    default = plan.info()["window_budget"]
    first = {i: plan.remap(dev, interpolation=i).clone() for i in (CR, BIL)}
    mix0 = plan.bilinear_tile_mix()
    assert mix0["window"] + mix0["direct"] > 0, mix0
    for budget in (4224, 12288, default):
        plan.set_window_budget(budget)
        assert plan.info()["window_budget"] == budget
        for i in (CR, BIL):
            got = plan.remap(dev, interpolation=i)
            assert torch.equal(got, first[i]), f"{name} {i}: a window budget of {budget} changes {int((got != first[i]).any(dim=2).sum())} pixels"
        assert plan.bilinear_tile_mix() == mix0, budget
    src, cmap = cc.pb_chain(case, image=np.zeros((case.src[1], case.src[2], 3), np.uint8))
    back = nat.Plan.deserialize(plan.serialize(), cmap.dst_proj, cmap.rotations, src._proj("src"))
    assert back.info()["fast_path"] and back.bilinear_tile_mix() == mix0, (back.bilinear_tile_mix(), mix0)
    for i in (CR, BIL):
        got = back.remap(dev, interpolation=i)
        assert torch.equal(got, first[i]), f"{name} {i}: the restored plan changes {int((got != first[i]).any(dim=2).sum())} pixels"


# ---- f. graph capture and streams ---------------------------------------------------------------------------------------------------------------
GRAPH_CASES = ["sweep2", "sweep14", "mag_pano_from_cam"]


@pytest.mark.parametrize("name", GRAPH_CASES)
def test_catmull_rom_remap_is_graph_capturable(name):
    """pb_remap_catmull_rom_u8 neither allocates nor synchronises (photonbend.h): a burst of single frames and a batch of two capture into
    one linear HIP graph on a side stream and replay with the same bytes, again on new pixels in the same buffers."""
    case = ic.by_name(name)
    plan = _plan(case)
    _, sh, sw, *_ = case.src
    rng = np.random.default_rng(5)
    noise = lambda: torch.from_numpy(rng.integers(0, 256, size=(4, sh, sw, 3), dtype=np.uint8)).cuda()  # noqa: E731
    frames = noise()
    outs = torch.zeros((4, case.dst[1], case.dst[2], 3), dtype=torch.uint8, device="cuda")
    want = plan.remap(frames, interpolation=CR).clone()
    assert all(torch.equal(plan.remap(frames[f], interpolation=CR), want[f]) for f in range(4))  # (eager single launches)
    lib = nat.load()
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            for f in range(2):
                nat.check(lib.pb_remap_catmull_rom_u8(plan.handle, frames[f].data_ptr(), outs[f].data_ptr(), 1, 0, 0, int(side.cuda_stream)))
            nat.check(lib.pb_remap_catmull_rom_u8(plan.handle, frames[2].data_ptr(), outs[2].data_ptr(), 2, 0, 0, int(side.cuda_stream)))
    torch.cuda.current_stream().wait_stream(side)
    outs.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(outs, want)
    frames.copy_(noise())
    want2 = plan.remap(frames, interpolation=CR).clone()
    assert not torch.equal(want2, want)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(outs, want2)


@pytest.mark.parametrize("name", ["sweep7", "mag_cube_from_pano"])
def test_one_plan_catmull_rom_on_several_streams_at_once(name):
    """Independent frames dealt round-robin to three HIP streams: launches of ONE plan overlap (the kernel's LDS parking and its fix-pixel
    pass are per wave and per frame) and every output equals the serial one."""
    case = ic.by_name(name)
    plan = _plan(case)
    lib = nat.load()
    _, sh, sw, *_ = case.src
    n = 9
    frames = torch.from_numpy(np.random.default_rng(9).integers(0, 256, size=(n, sh, sw, 3), dtype=np.uint8)).cuda()
    want = torch.stack([plan.remap(frames[f], interpolation=CR) for f in range(n)])
    got = torch.zeros_like(want)
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream() for _ in range(3)]
    sb, db = frames[0].numel(), want[0].numel()
    for rep in range(2):
        for f in range(n):
            nat.check(lib.pb_remap_catmull_rom_u8(plan.handle, frames.data_ptr() + f * sb, got.data_ptr() + f * db, 1, 0, 0, int(streams[f % 3].cuda_stream)))
    torch.cuda.synchronize()
    assert torch.equal(got, want)
