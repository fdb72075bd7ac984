"""pb_remap_ss_u8's fused tile kernel pb_ss_win_kernel per tile class, edge and frame layout, and pb_box_reduce by itself.

The reference is exact integers (tests/ss_cases.py): the oracle's index map of the n x destination, NumPy fancy indexing of a frame of
independent random bytes with it (black where the index is negative), then the n x n block mean of tests/ss_ref.py.  Every fused launch
is asserted to BE fused before it runs (the plan has a fast path and asks for no workspace with the very pointer and stride of the
call); source frames lie among random non-zero bytes, output frames among 0xA5 bytes that must all survive.

  a. the edge shapes of ss_cases.EDGES and the two FUSED_TWINS, n = 2 and 4, fused and forced generic, against the oracle
  b. the four mid plans of the pixel-format tests AS n x plans (every tile class, both launch-table layouts) against the oracle
  c. saturated frames: the packed 16-bit fields of the reduction at their largest
  d. pointer offsets, padded strides and batches never move a byte; unaligned sources fall to the generic route
  e. re-budgeted and restored plans
  f. graph capture and several streams
  g. pb_box_reduce against ss_ref.block_mean: both sample types, both factors, 1 .. 5 channels, rounding at every residue

Not covered: the second pass of pb_box_reduce_kernel's grid-stride loop, which needs more than 2^28 output pixels in one call."""

import functools

import numpy as np
import pytest
import torch

from photonbend_amd import _native as nat
from tests import cubemap_cases as cc
from tests import ss_cases as sc
from tests import ss_ref
from tests.ss_cases import ALL_EDGES, MID, NS, _mid_plan
from tests.test_hip_nv12 import _fix_pixels  # (the plan blob's reader: header, parameter block, sections)

pytestmark = pytest.mark.gpu

GUARD = 64  # bytes on either side of the source frames (random, non-zero) and of the output frames (sentinels)
SENTINEL = 0xA5
INVALID = -1
EDGE_NS = [(c, n) for c in ALL_EDGES for n in NS]
EDGE_IDS = [f"{c.name}-n{n}" for c, n in EDGE_NS]
MID_NS = [(c, n) for c in MID for n in NS]
MID_IDS = [f"{c.name}-n{n}" for c, n in MID_NS]

# pb_route serves a supersampled call fused where the plain call of the same frames takes pb_hot_win_kernel, and that kernel's LDS
# windows need the source pointer AND the source stride on 16-byte boundaries (pb_aligned16).  pb_check_frames fills a stride of 0 in
# with the packed frame size, 3 h w - so a packed frame whose size is no multiple of 16 goes generic even when it is the only one.
# Two edge sources are that small: their packed calls stay on the generic route (and must equal the oracle there); handed over with the
# stride rounded up to 16 the same shapes are served fused, and so are their twins of 48 and 96 bytes (ss_cases.FUSED_TWINS), packed.
PACKED_FRAME_BYTES_OFF_16 = {"ss_edge_tiny_src": 12, "ss_edge_last_px": 72}


# ---- plans: of their own (never the facade's shared cache entry), nearest tables only --------------------------------------------------
def _parts(case, n=1):
    """(destination projection, rotations, source projection) of a case at factor n: what nat.Plan and Plan.deserialize take."""
    src, cmap = cc.pb_chain(case, image=np.zeros((case.src[1], case.src[2], 3), np.uint8), supersample=n)
    return cmap.dst_proj, cmap.rotations, src._proj("src")


@functools.lru_cache(maxsize=None)
def _edge_plan(name, n):
    dst, rots, src = _parts(sc.edge_by_name(name), n)
    return nat.Plan(dst, rots, src, bilinear=False)


@functools.lru_cache(maxsize=None)
def _shared_mid_plan(name):
    """One plan per mid case for the tests that only launch it (section e changes budgets: it makes its own)."""
    return _mid_plan(sc.mid_by_name(name))


@functools.lru_cache(maxsize=None)
def _mid_frames(name, count=1):
    case = sc.mid_by_name(name)
    frames = [sc.random_frame(case.src[1], case.src[2], seed=8000 + 16 * [c.name for c in MID].index(name) + k) for k in range(count)]
    for f in frames:
        f.setflags(write=False)
    return frames


@functools.lru_cache(maxsize=None)
def _mid_want(name, n):
    """The oracle's output of a mid case's first frame: once per (case, n), shared and read-only."""
    w = sc.want(_mid_frames(name)[0], sc.mid_index(sc.mid_by_name(name))[0], n)
    w.setflags(write=False)
    return w


# ---- one launch through Plan.launch, between guards -------------------------------------------------------------------------------------
def _place_sources(frames, stride, off, seed):
    """The frames `stride` bytes apart, the first `off` bytes past a 16-byte boundary, in a device buffer of random non-zero bytes."""
    fb = frames[0].size
    host = np.random.default_rng(seed).integers(1, 256, GUARD + off + (len(frames) - 1) * stride + fb + GUARD, dtype=np.uint8)
    for f, fr in enumerate(frames):
        a = GUARD + off + f * stride
        host[a : a + fb] = fr.reshape(-1)
    dev = torch.from_numpy(host).cuda()
    assert dev.data_ptr() % 16 == 0
    return dev, dev.data_ptr() + GUARD + off


def _sentinels(n_frames, frame_bytes, stride, off):
    return torch.full((GUARD + off + (n_frames - 1) * stride + frame_bytes + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")


def _collect(buf, n_frames, frame_bytes, stride, off, shape, what):
    """The output frames of a sentinel buffer; every byte outside them - the guards, the offset, the padding between frames - must
    still be the sentinel."""
    host = buf.cpu().numpy()
    payload = np.zeros(host.size, bool)
    outs = []
    for f in range(n_frames):
        a = GUARD + off + f * stride
        outs.append(host[a : a + frame_bytes].reshape(shape).copy())
        payload[a : a + frame_bytes] = True
    stray = np.flatnonzero(~payload & (host != SENTINEL))
    assert stray.size == 0, f"{what}: {stray.size} bytes outside the output frames were written, first at {int(stray[0]) - GUARD - off} from the first frame's start"
    return outs


def ss_launch(plan, n, frames, route="fused", src_off=0, dst_off=0, src_stride=0, dst_stride=0, stream=None, seed=1, what=""):
    """One Plan.launch(..., supersample=n) of `frames` -> the list of (H / n, W / n, 3) outputs.  route: "fused" - asserted before the
    launch: a fast path, and no workspace for the pointer and stride actually passed; "unaligned" - asserted to need a workspace, which
    the call gets; "generic" - forced (PB_SS_GENERIC) with its workspace.  Strides in bytes, 0 = packed."""
    k = len(frames)
    sb = 3 * plan.src.height * plan.src.width
    oh, ow = plan.out_shape(n)
    db = 3 * oh * ow
    assert frames[0].shape == (plan.src.height, plan.src.width, 3) and (k == 1 or (src_stride or sb) >= sb)
    src, sp = _place_sources(frames, src_stride or sb, src_off, seed)
    buf = _sentinels(k, db, dst_stride or db, dst_off)
    dp = buf.data_ptr() + GUARD + dst_off
    assert sp % 16 == src_off % 16 and buf.data_ptr() % 16 == 0
    assert plan.info()["fast_path"], what
    need = plan.supersample_workspace_bytes(n, src_ptr=sp, src_stride=src_stride)
    ws = None
    if route == "fused":
        assert need == 0, f"{what}: not served by the fused kernel (a workspace of {need} bytes asked for)"
    elif route == "unaligned":
        assert need == 3 * plan.dst.height * plan.dst.width, what  # one n x frame: the generic route
        ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    else:
        assert route == "generic"
        ws = torch.empty(plan.supersample_workspace_bytes(n, generic=True), dtype=torch.uint8, device="cuda")
        assert ws.numel() == 3 * plan.dst.height * plan.dst.width
    plan.launch(sp, dp, k, stream, "nearest", src_stride=src_stride, dst_stride=dst_stride, supersample=n, generic=route == "generic", workspace=ws)
    torch.cuda.synchronize()
    del src
    return _collect(buf, k, db, dst_stride or db, dst_off, (oh, ow, 3), what)


def _pad16(nbytes):
    return (nbytes + 15) & ~15


# ---- a. the edges against the oracle ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,n", EDGE_NS, ids=EDGE_IDS)
def test_edges_fused_and_generic_equal_the_oracle(case, n):
    idx, fragile = sc.edge_index(case, n)
    img = sc.edge_frame(case)
    want = sc.want(img, idx, n)
    assert want.shape == (case.dst[1], case.dst[2], 3)
    plan = _edge_plan(case.name, n)
    assert (plan.dst.height, plan.dst.width) == idx.shape
    sb = img.size
    if case.name in PACKED_FRAME_BYTES_OFF_16:
        # (the reason above: the packed stride 3 h w is off a 16-byte boundary, so the plain route is not WIN and the supersampled one
        #  is SS_GENERIC; the same frame at a 16-byte stride is served fused)
        assert sb == PACKED_FRAME_BYTES_OFF_16[case.name] and sb % 16 != 0
        packed = ss_launch(plan, n, [img], route="unaligned", what=f"{case.name} n={n} packed")[0]
        sc.check(packed, want, fragile, n, f"{case.name} n={n} packed (generic route)")
        fused = ss_launch(plan, n, [img], src_stride=_pad16(sb), what=f"{case.name} n={n} at a 16-byte stride")[0]
    else:
        assert sb % 16 == 0
        fused = ss_launch(plan, n, [img], what=f"{case.name} n={n}")[0]
    sc.check(fused, want, fragile, n, f"{case.name} n={n} fused")
    generic = ss_launch(plan, n, [img], route="generic", what=f"{case.name} n={n} generic")[0]
    sc.check(generic, want, fragile, n, f"{case.name} n={n} forced generic")
    assert np.array_equal(fused, generic), f"{case.name} n={n}: fused and generic differ in {int((fused != generic).any(axis=2).sum())} pixels"


# ---- b. every tile class at mid size against the oracle ---------------------------------------------------------------------------------
def _failed_tiles(plan):
    """The plan's failed-tile list (tile index ty * tiles_x + tx) from its serialized form: the section before the fix pixels'."""
    import struct

    blob = plan.serialize()
    params_size = struct.unpack_from("<4I", blob, 0)[2]
    n_tiles, n_fail, n_fix = struct.unpack_from("<3I", blob, 32)
    sec = struct.unpack_from("<13Q", blob, 72)
    assert sec[0] == 256 * n_tiles and sec[2] == 4 * max(n_fail, 1)
    tiles = np.frombuffer(blob, np.int32, n_fail, 184 + params_size + sec[0] + sec[1])
    assert bool(((tiles >= 0) & (tiles < n_tiles)).all()) and len(np.unique(tiles)) == n_fail
    return tiles


def test_mid_plans_contain_every_tile_class_and_a_fix_pixel_inside_a_served_tile():
    """The coverage of the test below cannot go silently: over the four plans there are failed tiles, fix pixels, LEAN, DIRECT and BLACK
    tiles - and a fix pixel inside a tile that did NOT fail, the condition under which pb_ss_win_kernel's readlane loop patches a
    register before the reduction."""
    total = {"fix_tiles": 0, "fix_pixels": 0, "lean_tiles": 0, "direct_tiles": 0, "black_tiles": 0}
    patched = 0
    for case in MID:
        assert case.dst[1] % 4 == 0 and case.dst[2] % 4 == 0, case.name
        plan = _shared_mid_plan(case.name)
        info = plan.info()
        assert info["fast_path"], case.name
        for k in total:
            total[k] += info[k]
        px = _fix_pixels(plan)
        failed = _failed_tiles(plan)
        assert len(px) == info["fix_pixels"] and len(failed) == info["fix_tiles"], case.name
        tiles_x = (case.dst[2] + 31) // 32
        y, x = np.divmod(px, case.dst[2])
        patched += int((~np.isin((y // 32) * tiles_x + x // 32, failed)).sum())
    assert all(v >= 1 for v in total.values()), total
    assert patched >= 1
    # both layouts of pb_build_launch_table, by its own rule: super-tiles of 4 x 4 workgroups (2 x 2 tiles each) where the grid divides
    # into at least sixteen of them
    groups = [((c.dst[2] + 63) // 64, (c.dst[1] + 63) // 64) for c in MID]
    assert [gx % 4 == 0 and gy % 4 == 0 and (gx // 4) * (gy // 4) >= 16 for gx, gy in groups] == [True, True, False, False]


@pytest.mark.parametrize("case,n", MID_NS, ids=MID_IDS)
def test_mid_plans_as_n_x_plans_equal_the_oracle(case, n):
    fragile = sc.mid_index(case)[1]
    got = ss_launch(_shared_mid_plan(case.name), n, _mid_frames(case.name), what=f"{case.name} n={n}")[0]
    sc.check(got, _mid_want(case.name, n), fragile, n, f"{case.name} n={n}")


# ---- c. saturated frames ----------------------------------------------------------------------------------------------------------------
SATURATED = [(255, 255, 255), (255, 0, 255), (0, 255, 0)]  # ev's two 16-bit fields and od's one at 16 x 255, next to an empty neighbour


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("name", ["ss_edge_33_inscribed", "M_photo_stereographic"])
def test_saturated_frames_give_255_k_over_N_rounded(name, n):
    if name.startswith("M_"):
        case = sc.mid_by_name(name)
        plan, (idx, fragile) = _shared_mid_plan(name), sc.mid_index(case)
    else:
        case = sc.edge_by_name(name)
        plan, (idx, fragile) = _edge_plan(name, n), sc.edge_index(case, n)
    N = n * n
    valid = (idx >= 0).reshape(idx.shape[0] // n, n, idx.shape[1] // n, n).sum(axis=(1, 3))  # k: a block's sampled subsamples
    assert int((valid == N).sum()) >= 1 and int((valid == 0).sum()) >= 1 and int(((valid > 0) & (valid < N)).sum()) >= 1
    for rgb in SATURATED:
        img = np.empty((case.src[1], case.src[2], 3), np.uint8)
        img[:] = rgb
        want = sc.want(img, idx, n)
        # (the reference written out: 255 in fully valid blocks, the rounded 255 k / N in mixed ones, 0 in black ones)
        q, r = (255 * valid) // N, (255 * valid) % N
        level = (q + ((r > N // 2) | ((r == N // 2) & (q % 2 == 1)))).astype(np.uint8)
        assert np.array_equal(want, np.where(np.array(rgb) == 255, level[..., None], 0).astype(np.uint8))
        got = ss_launch(plan, n, [img], what=f"{name} n={n} {rgb}")[0]
        sc.check(got, want, fragile, n, f"{name} n={n} source {rgb}")


# ---- d. how the frames reach the kernel never moves a byte ------------------------------------------------------------------------------
LAYOUT_CASES = ["ss_edge_17x19", "ss_edge_33_inscribed", "M_pano_thoby"]


def _layout_plan_and_frames(name, n):
    if name.startswith("M_"):
        return _shared_mid_plan(name), _mid_frames(name, 5)
    case = sc.edge_by_name(name)
    return _edge_plan(name, n), [sc.edge_frame(case, k) for k in range(5)]


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("name", LAYOUT_CASES)
def test_offsets_strides_and_batches_give_the_bytes_of_the_aligned_single_launch(name, n):
    plan, frames = _layout_plan_and_frames(name, n)
    sb = frames[0].size
    oh, ow = plan.out_shape(n)
    db = 3 * oh * ow
    assert sb % 16 == 0
    tag = f"{name} n={n}"
    # embedded and aligned, one frame at a time: the launch that sections a / b hold to the oracle
    want = [ss_launch(plan, n, [f], what=f"{tag} frame {k}")[0] for k, f in enumerate(frames)]
    assert not np.array_equal(want[1], want[2])
    if name.startswith("M_"):
        sc.check(want[0], _mid_want(name, n), sc.mid_index(sc.mid_by_name(name))[1], n, tag)
    # destination pointer + 1: byte stores; + 4: dword stores at a base that is not 16-byte aligned
    for off in (1, 4):
        got = ss_launch(plan, n, frames[:1], dst_off=off, what=f"{tag} dst+{off}")[0]
        assert np.array_equal(got, want[0]), f"{tag}: destination pointer + {off} moved {int((got != want[0]).any(axis=2).sum())} pixels"
    # batches of five in one launch
    for so, do, ss, ds in ((0, 0, sb + 16, db + 3), (0, 0, sb + 48, db + 48), (0, 1, sb, db + 3)):
        got = ss_launch(plan, n, frames, dst_off=do, src_stride=ss, dst_stride=ds, what=f"{tag} batch ss={ss - sb} ds={ds - db} dst+{do}")
        for k in range(5):
            assert np.array_equal(got[k], want[k]), f"{tag}: batch (src stride +{ss - sb}, dst stride +{ds - db}, dst + {do}) frame {k} differs"
    # an unaligned source - pointer + 1, or a batch at stride + 3 - is the generic route's: the same bytes with a workspace ...
    got = ss_launch(plan, n, frames[:1], route="unaligned", src_off=1, what=f"{tag} src+1")[0]
    assert np.array_equal(got, want[0]), f"{tag}: source pointer + 1 (generic route) differs"
    got = ss_launch(plan, n, frames, route="unaligned", src_stride=sb + 3, dst_stride=db + 3, what=f"{tag} batch src stride +3")
    for k in range(5):
        assert np.array_equal(got[k], want[k]), f"{tag}: batch at source stride + 3 (generic route) frame {k} differs"
    # ... and PB_ERR_INVALID without one, before anything is launched
    lib = nat.load()
    for so, ss, k in ((1, 0, 1), (0, sb + 3, 5)):
        src, sp = _place_sources(frames[:k], ss or sb, so, seed=2)
        buf = _sentinels(k, db, db, 0)
        rc = lib.pb_remap_ss_u8(plan.handle, n, 0, sp, buf.data_ptr() + GUARD, k, ss, 0, None, 0, 0, nat.current_stream())
        assert rc == INVALID and b"workspace" in lib.pb_last_error(), (tag, so, ss, rc, lib.pb_last_error())
        torch.cuda.synchronize()
        assert bool((buf == SENTINEL).all()), (tag, so, ss)


# ---- e. re-budgeted and restored plans --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["M_photo_stereographic", "KM_cube384_pano_rot"])
def test_rebudgeted_and_restored_plans_give_the_same_bytes(name):
    """The kernel's generic-tile branch recomputes its window's row cap from the budget of the launch (Hd.win_budget); the classification
    under that budget chose which tiles are LEAN.  Both must move together, and a restored plan carries both."""
    n = 2
    case = sc.mid_by_name(name)
    plan = _mid_plan(case)  # (its own: the budget changes)
    frames = _mid_frames(name)
    default = plan.info()["window_budget"]
    want = ss_launch(plan, n, frames, what=f"{name} default budget")[0]
    sc.check(want, _mid_want(name, n), sc.mid_index(case)[1], n, name)
    classes = {(plan.info()["lean_tiles"], plan.info()["direct_tiles"])}
    for budget in (4224, 12288, default):
        plan.set_window_budget(budget)
        info = plan.info()
        assert info["window_budget"] == budget and info["fast_path"], (name, budget, info["window_budget"])
        classes.add((info["lean_tiles"], info["direct_tiles"]))
        got = ss_launch(plan, n, frames, what=f"{name} budget {budget}")[0]  # (asserts that no workspace is asked for)
        assert np.array_equal(got, want), f"{name}: budget {budget} moved {int((got != want).any(axis=2).sum())} pixels"
    assert len(classes) >= 2, f"{name}: no budget reclassified a tile {classes}"
    dst, rots, src = _parts(case)
    restored = nat.Plan.deserialize(plan.serialize(), dst, rots, src)
    assert restored.info()["window_budget"] == default
    got = ss_launch(restored, n, frames, what=f"{name} restored")[0]
    assert np.array_equal(got, want), f"{name}: the restored plan moved {int((got != want).any(axis=2).sum())} pixels"


# ---- f. graph capture and streams -------------------------------------------------------------------------------------------------------
def _ss_raw(plan, n, src_ptr, dst_ptr, n_frames, stream):
    """pb_remap_ss_u8 itself, packed frames, no workspace: fused or PB_ERR_INVALID."""
    return nat.load().pb_remap_ss_u8(plan.handle, n, 0, src_ptr, dst_ptr, n_frames, 0, 0, None, 0, 0, stream)


@pytest.mark.parametrize("n", NS)
def test_fused_supersample_is_graph_capturable(n):
    """The fused route neither allocates nor synchronises: a single-frame call and a two-frame call capture into one linear graph on a
    side stream and replay with the eager bytes, again on new pixels in the same buffers."""
    name = "M_pano_thoby"
    case = sc.mid_by_name(name)
    plan = _shared_mid_plan(name)
    _, sh, sw, *_ = case.src
    oh, ow = plan.out_shape(n)
    rng = np.random.default_rng(50 + n)
    noise = lambda: torch.from_numpy(rng.integers(0, 256, size=(3, sh, sw, 3), dtype=np.uint8)).cuda()  # noqa: E731
    frames = noise()
    assert plan.info()["fast_path"] and plan.supersample_workspace_bytes(n, src_ptr=frames.data_ptr(), src_stride=frames[0].numel()) == 0
    outs = torch.full((3, oh, ow, 3), SENTINEL, dtype=torch.uint8, device="cuda")
    want = plan.remap(frames, supersample=n).clone()
    assert all(torch.equal(plan.remap(frames[f], supersample=n), want[f]) for f in range(3))  # (eager single launches)
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            nat.check(_ss_raw(plan, n, frames[0].data_ptr(), outs[0].data_ptr(), 1, int(side.cuda_stream)))
            nat.check(_ss_raw(plan, n, frames[1].data_ptr(), outs[1].data_ptr(), 2, int(side.cuda_stream)))
    torch.cuda.current_stream().wait_stream(side)
    outs.fill_(SENTINEL)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(outs, want)
    frames.copy_(noise())
    want2 = plan.remap(frames, supersample=n).clone()
    assert not torch.equal(want2, want)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(outs, want2)


@pytest.mark.parametrize("n", NS)
def test_one_plan_fused_supersample_on_several_streams_at_once(n):
    """Nine independent frames dealt round-robin to three streams: launches of ONE plan overlap (windows and patched registers are per
    wave and per frame) and every output equals the serial one."""
    name = "M_pano_thoby"
    case = sc.mid_by_name(name)
    plan = _shared_mid_plan(name)
    _, sh, sw, *_ = case.src
    count = 9
    frames = torch.from_numpy(np.random.default_rng(90 + n).integers(0, 256, size=(count, sh, sw, 3), dtype=np.uint8)).cuda()
    sb = frames[0].numel()
    assert plan.info()["fast_path"] and sb % 16 == 0 and plan.supersample_workspace_bytes(n, src_ptr=frames.data_ptr(), src_stride=sb) == 0
    want = torch.stack([plan.remap(frames[f], supersample=n) for f in range(count)])
    assert not torch.equal(want[1], want[2])
    got = torch.zeros_like(want)
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream() for _ in range(3)]
    db = want[0].numel()
    for rep in range(2):
        for f in range(count):
            nat.check(_ss_raw(plan, n, frames.data_ptr() + f * sb, got.data_ptr() + f * db, 1, int(streams[f % 3].cuda_stream)))
    torch.cuda.synchronize()
    assert torch.equal(got, want)


# ---- g. pb_box_reduce by itself ---------------------------------------------------------------------------------------------------------
BOX_SHAPES = [(1, 1), (3, 5), (7, 64), (33, 257)]  # output (H, W): one pixel, odd sizes, one 256-thread block and a bit, several blocks
BOX_CHANNELS = (1, 2, 3, 4, 5)
BOX_FRAMES = 3


def _residue_input(frames, H, W, C, n, dt):
    """Samples whose block sums take every residue r in [0, N) under an even and an odd quotient, near zero and near the type's maximum:
    block b holds N - 1 samples v and one v + r, r = b mod N, v cycling through 6, 7, max - 16, max - 15; the odd sample's place in the
    block moves with b."""
    N = n * n
    top = int(np.iinfo(dt).max)
    b = np.arange(frames * H * W * C, dtype=np.int64).reshape(frames, H, W, C)
    r = b % N
    v = np.array([6, 7, top - 16, top - 15], dtype=np.int64)[(b // N) % 4]
    a = np.broadcast_to(v[:, :, None, :, None, :], (frames, H, n, W, n, C)).copy()
    pos = (b // (4 * N) + b) % N
    fi, yi, xi, ci = np.indices((frames, H, W, C))
    a[fi, yi, pos // n, xi, pos % n, ci] += r
    assert int(a.max()) <= top
    return a.reshape(frames, n * H, n * W, C).astype(dt), (v % 2, r)


def _box_call(x, n):
    """One raw pb_box_reduce of (F, n H, n W, C) samples, the source among random non-zero bytes, the output among sentinels."""
    F, Hn, Wn, C = x.shape
    H, W, S = Hn // n, Wn // n, x.dtype.itemsize
    src, sp = _place_sources([x.view(np.uint8)], x.nbytes, 0, seed=3)
    nbytes = F * H * W * C * S
    buf = _sentinels(1, nbytes, nbytes, 0)
    rc = nat.load().pb_box_reduce(sp, buf.data_ptr() + GUARD, H, W, C, S, n, F, nat.current_stream())
    assert rc == 0, nat.load().pb_last_error()
    torch.cuda.synchronize()
    out = _collect(buf, 1, nbytes, nbytes, 0, (nbytes,), f"pb_box_reduce {x.shape} {x.dtype} n={n}")[0]
    return out.view(x.dtype).reshape(F, H, W, C)


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("dt", [np.uint8, np.uint16], ids=["u8", "u16"])
def test_box_reduce_equals_the_block_mean(dt, n):
    N = n * n
    top = int(np.iinfo(dt).max)
    rng = np.random.default_rng(1000 + 10 * np.dtype(dt).itemsize + n)
    for H, W in BOX_SHAPES:
        for C in BOX_CHANNELS:
            what = f"{np.dtype(dt)} n={n} {H}x{W}x{C}"
            shape = (BOX_FRAMES, n * H, n * W, C)
            random = rng.integers(0, top + 1, shape, dtype=dt)
            full = np.full(shape, top, dt)  # 16 x 65535 per channel at n = 4: the largest sum there is
            residues, (parity, r) = _residue_input(BOX_FRAMES, H, W, C, n, dt)
            if BOX_FRAMES * H * W * C >= 4 * N:
                assert len(set(zip(parity.reshape(-1).tolist(), r.reshape(-1).tolist()))) == 2 * N, what  # every residue, q even and q odd
            for kind, x in (("random", random), ("maximum", full), ("residues", residues)):
                want = np.stack([ss_ref.block_mean(f, n) for f in x])
                got = _box_call(x, n)  # three frames in one call
                assert np.array_equal(got, want), f"{what} {kind}: {int((got != want).sum())} samples differ"
                if kind == "maximum":
                    assert bool((got == top).all()), what
            # nat.box_reduce: one frame, with and without a trailing axis
            one = random[1] if C > 1 else random[1, :, :, 0]
            got = nat.box_reduce(torch.from_numpy(np.ascontiguousarray(one)).cuda(), n).cpu().numpy()
            assert got.dtype == np.dtype(dt) and np.array_equal(got, ss_ref.block_mean(one, n)), what
