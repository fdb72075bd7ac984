"""pb_remap_nv12: NV12 and P010 video frames through the tile kernel pb_video_hot_kernel (its PAIRS form) - the bytes of the definition
(tests/nv12_ref.py) with the reference's index map, for both sample sizes, every tile class, edge, layout and launch shape.  Every
comparison is exact equality; images are independent random bytes per plane (a wrong index shows), destinations sit between sentinel
bytes that must survive, and so must the padding bytes inside pitched frames."""

import os
import struct

import numpy as np
import pytest
import torch

from oracle import reference_path as orc
from photonbend_amd import _hostpipe, batch
from photonbend_amd import _native as nat
from tests import cases as tc
from tests import cubemap_cases as cc
from tests import cubemap_ref as cr
from tests import helpers as H
from tests import nv12_ref
from tests import polynomial_cases as pc
from tests.cases import Case, cam, inscribed, pano
from tests.test_hip_pixel_formats import MID, _mid_plan  # (the four mid cases of the pixel-format tests, and their plans)

pytestmark = pytest.mark.gpu

SAMPLES = ((1, np.uint8), (2, np.uint16))
GUARD = 64  # sentinel bytes on either side of a destination
SENTINEL = 0xA5
INVALID, UNSUPPORTED = -1, -3
SMALL = H.load_small()
GOLD_CUBE = np.load(os.path.join(H.GOLD, "cubemap.npz"))
GOLD_POLY = np.load(os.path.join(H.GOLD, "polynomial.npz"))


def even(case):
    return not (case.src[1] | case.src[2] | case.dst[1] | case.dst[2]) & 1


def random_frame(h, w, dt, seed):
    """A packed (3h/2, w) frame of independent random bytes."""
    S = np.dtype(dt).itemsize
    return np.random.default_rng(seed).integers(0, 256, (3 * h // 2, w * S), dtype=np.uint8).view(dt)


def guarded(nbytes):
    """A device buffer of sentinel bytes with `nbytes` of payload between two guards."""
    return torch.full((nbytes + 2 * GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")


def guards_intact(buf):
    return bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[-GUARD:] == SENTINEL).all())


def nv12_call(plan, src_ptr, dst_ptr, S, n=1, sl=None, dl=None, fill=None, stream=None):
    sl = None if sl is None else nat.pb_nv12_layout(*sl)
    dl = None if dl is None else nat.pb_nv12_layout(*dl)
    f = None if fill is None else (nat.C.c_uint16 * 3)(*fill)
    return nat.load().pb_remap_nv12(plan.handle, src_ptr, dst_ptr, n, None if sl is None else nat.C.addressof(sl), None if dl is None else nat.C.addressof(dl), S,
                                    None if f is None else nat.C.addressof(f), nat.current_stream() if stream is None else stream)


def run_nv12(plan, frame, fill=None):
    """One packed pb_remap_nv12 launch of a (3h/2, w) frame -> (3H/2, W); the guards around the destination must survive."""
    Hd, Wd, S = plan.dst.height, plan.dst.width, frame.dtype.itemsize
    src = torch.from_numpy(frame.view(np.uint8)).cuda()
    buf = guarded(3 * Hd * Wd * S // 2)
    assert nv12_call(plan, src.data_ptr(), buf.data_ptr() + GUARD, S, fill=fill) == 0, nat.load().pb_last_error()
    torch.cuda.synchronize()
    assert guards_intact(buf), "pb_remap_nv12 wrote outside the destination frame"
    return buf[GUARD:-GUARD].cpu().numpy().view(frame.dtype).reshape(3 * Hd // 2, Wd)


def bad_planes(got, want, H_):
    """(luma pixels that differ (H, W), chroma pairs that differ (H/2, W/2)) of two packed frames."""
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    W_ = got.shape[1]
    return got[:H_] != want[:H_], (got[H_:] != want[H_:]).reshape(H_ // 2, W_ // 2, 2).any(axis=2)


def assert_equal(got, want, H_, fragile, exact, what):
    """The treatment of tests/test_hip_pixel_formats.py: nothing differs outside the fragile set (for chroma: the anchors'), and nothing
    at all where the index is the goldens' platform's."""
    by, buv = bad_planes(got, want, H_)
    if fragile is not None:
        assert int((by & ~fragile).sum()) == 0 and int((buv & ~fragile[0::2, 0::2]).sum()) == 0, \
            f"{what}: {int((by & ~fragile).sum())} luma pixels and {int((buv & ~fragile[0::2, 0::2]).sum())} pairs differ outside the fragile set"
    if exact:
        assert int(by.sum()) == 0 and int(buv.sum()) == 0, f"{what}: {int(by.sum())} luma pixels and {int(buv.sum())} pairs differ"


# ---- 1. the small case matrices against the reference's golden index maps -------------------------------------------------------------
def _small_plans():
    out = []
    for c in tc.small_cases():
        if c.src[0] != "double" and even(c):
            fragile = np.unpackbits(SMALL[f"{c.name}/fragile"])[: c.dst[1] * c.dst[2]].reshape(c.dst[1], c.dst[2]).astype(bool)
            out.append((c, lambda c=c: H.pb_plan_private(c, bilinear=False), SMALL[f"{c.name}/idx"], fragile))
    for mod, gold in ((cc, GOLD_CUBE), (pc, GOLD_POLY)):
        for c in mod.small_cases():
            if c.src[0] != "double" and even(c):
                def make(c=c, mod=mod):
                    src, cmap = mod.pb_chain(c, image=np.zeros((c.src[1], c.src[2], 3), np.uint8))
                    return nat.Plan(cmap.dst_proj, cmap.rotations, src._proj("src"), bilinear=False)
                out.append((c, make, gold[f"{c.name}/idx"], None))
    return out


SMALL_PLANS = _small_plans()
ODD = [c for c in tc.small_cases() if c.src[0] != "double" and not even(c)]


def test_the_small_cases_are_the_ones_the_feature_was_specified_on():
    names = {p[0].name for p in SMALL_PLANS}
    assert sum(1 for c in tc.small_cases() if c.name in names) == 49
    assert sorted(c.name for c in ODD) == ["A_photo_odd", "B_pano_odd"]
    assert any(c.name in names and c.src[0] != "double" and even(c) for c in cc.small_cases())
    assert any(c.name in names and c.src[0] != "double" and even(c) for c in pc.small_cases())


@pytest.mark.parametrize("case,make_plan,idx,fragile", SMALL_PLANS, ids=[p[0].name for p in SMALL_PLANS])
def test_small_cases_equal_the_definition_with_the_golden_index(case, make_plan, idx, fragile):
    plan = make_plan()
    _, h, w, *_ = case.src
    Hd = idx.shape[0]
    for k, (S, dt) in enumerate(SAMPLES):
        assert plan.nv12_supported(S), (case.name, S)
        frame = random_frame(h, w, dt, seed=100 + k)
        for fill in (None, (1, 2, 3)):
            want = nv12_ref.remap_frame(frame, idx, h, w, fill)
            got = run_nv12(plan, frame, fill)
            assert_equal(got, want, Hd, fragile, True, f"{case.name} S={S} fill={fill}")
        # through Plan.remap_nv12 with the typed array: same dtype back, into `out`
        buf = guarded(want.nbytes)
        out = buf[GUARD:-GUARD].view(nat.torch_dtype(dt)).reshape(want.shape)
        assert plan.remap_nv12(torch.from_numpy(frame).cuda(), out=out, fill=(1, 2, 3)) is out
        torch.cuda.synchronize()
        assert guards_intact(buf) and np.array_equal(out.cpu().numpy(), want), (case.name, S)


@pytest.mark.parametrize("case", ODD, ids=lambda c: c.name)
def test_an_odd_dimension_is_invalid_and_nothing_is_written(case):
    plan = H.pb_plan_private(case, bilinear=False)
    _, h, w, *_ = case.src
    for S, dt in SAMPLES:
        src = torch.zeros(4 * h * w, dtype=torch.uint8, device="cuda")
        buf = guarded(4 * case.dst[1] * case.dst[2])
        assert nv12_call(plan, src.data_ptr(), buf.data_ptr() + GUARD, S) == INVALID and b"even" in nat.load().pb_last_error()
        torch.cuda.synchronize()
        assert bool((buf == SENTINEL).all())
        with pytest.raises(nat.PbError, match="even"):
            plan.nv12_supported(S)


# ---- 2. every tile class at mid size, against the oracle --------------------------------------------------------------------------------
def _fix_pixels(plan):
    """The plan's fix list (destination pixel indices), read from its serialized form: header (184 bytes: the counts at 32, the thirteen
    section sizes at 72), the parameter block, then the sections - the tile table, the right eye's, the failed tiles, the fix pixels."""
    blob = plan.serialize()
    magic, version, params_size, entry_size = struct.unpack_from("<4I", blob, 0)
    assert (magic, version, entry_size) == (0x4C504250, 5, 256), "the plan blob's format changed: this reader must follow"
    n_tiles, n_fail, n_fix = struct.unpack_from("<3I", blob, 32)
    sec = struct.unpack_from("<13Q", blob, 72)
    assert sec[0] == 256 * n_tiles and sec[2] == 4 * max(n_fail, 1) and sec[3] == sec[5] == 4 * max(n_fix, 1) and 184 + params_size + sum(sec) == len(blob)
    off = 184 + params_size + sec[0] + sec[1] + sec[2]
    px = np.frombuffer(blob, np.int32, n_fix, off)
    assert bool(((px >= 0) & (px < plan.dst.height * plan.dst.width)).all()) and len(np.unique(px)) == n_fix
    return px


def test_mid_cases_contain_every_tile_class_and_a_fix_pixel_that_is_an_anchor():
    """The coverage of the test below cannot go silently: its plans hold failed tiles, fix pixels, LEAN, DIRECT and BLACK tiles - and a
    fix pixel on an even row and an even column, which re-copies its chroma pair."""
    total = {"fix_tiles": 0, "fix_pixels": 0, "lean_tiles": 0, "direct_tiles": 0, "black_tiles": 0}
    anchors = 0
    for case in MID:
        assert even(case), case.name
        plan = _mid_plan(case)
        info = plan.info()
        assert info["fast_path"], case.name
        for k in total:
            total[k] += info[k]
        px = _fix_pixels(plan)
        assert len(px) == info["fix_pixels"], case.name
        y, x = np.divmod(px, case.dst[2])
        anchors += int((((y | x) & 1) == 0).sum())
    assert all(v >= 1 for v in total.values()), total
    assert anchors >= 1


@pytest.mark.parametrize("case", MID, ids=lambda c: c.name)
def test_mid_cases_equal_the_definition_with_the_oracle_index(case):
    with np.errstate(all="ignore"):
        cmap = cc.ref_stages(case)[-1]
        idx = cc.ref_index(case, cmap)
        if case.src[0] == "cube":
            fragile = orc.fragile_mask(cr.pretrunc(cr.face_size(case.src[1], case.src[2]), np.copy(cmap)))
        else:
            fragile = orc.fragile_mask(orc.pretrunc(H.orc_proj(case.dst), H.orc_proj(case.src), H.orc_rots(case)))
    exact = H.live_numpy_is_the_goldens_numpy()  # (else the live oracle's last bits are this host's: the fragile set is the allowance)
    plan = _mid_plan(case)
    _, h, w, *_ = case.src
    for S, dt in SAMPLES:
        assert plan.nv12_supported(S)
        frame = random_frame(h, w, dt, seed=200 + S)
        for fill in (None, (1, 2, 3)):
            assert_equal(run_nv12(plan, frame, fill), nv12_ref.remap_frame(frame, idx, h, w, fill), idx.shape[0], fragile, exact, f"{case.name} S={S}")


# ---- 3. edges ---------------------------------------------------------------------------------------------------------------------------
EDGES = [
    Case("edge_2x2", cam(2, 2, "equidistant", 172), pano(16, 32)),  # one block
    Case("edge_2x34", cam(2, 34, "equidistant", 172), pano(16, 32)),
    Case("edge_34x2", cam(34, 2, "equidistant", 172), pano(16, 32)),
    Case("edge_34x36_src2x2", cam(34, 36, "equidistant", 180), pano(2, 2), [(10, 20, 30)]),
    Case("edge_36x34_src4x6", pano(36, 34), pano(4, 6), [(12, 34, 56)]),
    Case("edge_34x36_cam_src", cam(34, 36, "equisolid", 190), cam(48, 48, "equidistant", 360, inscribed(48)), [(30, 45, 10)]),
    Case("edge_66x66_inscribed", cam(66, 66, "equidistant", 360, inscribed(66)), pano(64, 128), [(30, 45, 10)]),  # partial tiles on both axes
    Case("edge_pano_identity", pano(32, 64), pano(32, 64)),
    Case("edge_pano_2x_last_pixel", pano(64, 128), pano(32, 64)),
]
# what the oracle's index says of a case, asserted below: the source's last luma pixel is sampled / its last chroma pair is / at least
# how many 2 x 2 blocks hold valid and black pixels together, by the anchor's kind
SAMPLES_LAST_PIXEL = ("edge_34x36_src2x2", "edge_36x34_src4x6", "edge_pano_2x_last_pixel")
SAMPLES_LAST_PAIR = SAMPLES_LAST_PIXEL + ("edge_pano_identity",)
# (blocks with a valid anchor among black pixels, blocks with a black anchor among valid ones): the oracle's counts on these geometries
# (34, 38 and 76 mixed blocks in all; the cases were specified with 24, 26 and 56, which the oracle does not give)
MIXED_BLOCKS = {"edge_34x36_src2x2": (16, 18), "edge_34x36_cam_src": (19, 19), "edge_66x66_inscribed": (32, 44)}


@pytest.mark.parametrize("case", EDGES, ids=lambda c: c.name)
def test_edges_partial_tiles_tiny_sources_mixed_blocks_and_the_last_pair(case):
    with np.errstate(all="ignore"):
        idx = orc.remap_index(H.orc_proj(case.dst), H.orc_proj(case.src), H.orc_rots(case))
        fragile = orc.fragile_mask(orc.pretrunc(H.orc_proj(case.dst), H.orc_proj(case.src), H.orc_rots(case)))
    _, h, w, *_ = case.src
    Hd, Wd = idx.shape
    a = idx[0::2, 0::2]
    r, c = np.divmod(np.where(a < 0, 0, a), w)
    if case.name in SAMPLES_LAST_PIXEL:
        assert int(idx.max()) == h * w - 1  # the source's very last luma pixel is sampled
    if case.name in SAMPLES_LAST_PAIR:
        assert bool(((a >= 0) & ((r >> 1) == h // 2 - 1) & ((c >> 1) == w // 2 - 1)).any())  # ... and its very last pair
    if case.name in MIXED_BLOCKS:
        blocks = (idx >= 0).reshape(Hd // 2, 2, Wd // 2, 2).transpose(0, 2, 1, 3).reshape(-1, 4)
        mixed = blocks.any(axis=1) & ~blocks.all(axis=1)
        # a valid anchor keeps its pair, a black one fills
        assert (int((mixed & blocks[:, 0]).sum()), int((mixed & ~blocks[:, 0]).sum())) == MIXED_BLOCKS[case.name]
    plan = H.pb_plan_private(case, bilinear=False)
    exact = H.live_numpy_is_the_goldens_numpy()
    for S, dt in SAMPLES:
        assert plan.nv12_supported(S)
        frame = random_frame(h, w, dt, seed=300 + S)
        for fill in (None, (1, 2, 3)):
            assert_equal(run_nv12(plan, frame, fill), nv12_ref.remap_frame(frame, idx, h, w, fill), Hd, fragile, exact, f"{case.name} S={S}")


# ---- 4. layouts -------------------------------------------------------------------------------------------------------------------------
LAYOUT_CASE = tc.case_by_name("D_photo_rot")


def layouts(h, w, S):
    """name -> (pitch, uv_offset) of the pitched layouts under test for an h x w frame."""
    p1, p2 = w * S + 2 * S, -(-w * S // 256) * 256
    return {"pitch_plus_a_pair": (p1, p1 * h), "pitch_256": (p2, p2 * h), "three_padding_rows": (p1, p1 * (h + 3))}


def span(pitch, uv, h):
    return uv + pitch * (h // 2)


def scatter(frame, h, pitch, uv, fill_byte=None, seed=0):
    """The packed frame laid out at (pitch, uv) in a byte buffer whose padding is random (a source) or `fill_byte` (a destination)."""
    rows = frame.view(np.uint8)
    n = span(pitch, uv, h)
    buf = np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8) if fill_byte is None else np.full(n, fill_byte, np.uint8)
    for y in range(h):
        buf[y * pitch : y * pitch + rows.shape[1]] = rows[y]
    for y in range(h // 2):
        buf[uv + y * pitch : uv + y * pitch + rows.shape[1]] = rows[h + y]
    return buf


def gather(buf, h, w, dt, pitch, uv):
    """(the packed frame found at (pitch, uv) in a byte buffer, the buffer's bytes outside that frame)."""
    rb = w * np.dtype(dt).itemsize
    pay = np.zeros(len(buf), bool)
    rows = []
    for y in range(h):
        rows.append(buf[y * pitch : y * pitch + rb]); pay[y * pitch : y * pitch + rb] = True
    for y in range(h // 2):
        rows.append(buf[uv + y * pitch : uv + y * pitch + rb]); pay[uv + y * pitch : uv + y * pitch + rb] = True
    return np.stack(rows).view(dt), buf[~pay]


@pytest.mark.parametrize("S,dt", SAMPLES)
def test_pitched_frames_padding_rows_and_a_base_one_pair_off_alignment(S, dt):
    case = LAYOUT_CASE
    plan = H.pb_plan_private(case, bilinear=False)
    _, h, w, *_ = case.src
    Hd, Wd = case.dst[1], case.dst[2]
    frame = random_frame(h, w, dt, seed=400 + S)
    want = run_nv12(plan, frame)
    assert np.array_equal(want, nv12_ref.remap_frame(frame, SMALL[f"{case.name}/idx"], h, w))
    A = 2 * S  # one pair
    for (name, (sp, su)), (dp, du) in zip(layouts(h, w, S).items(), layouts(Hd, Wd, S).values()):
        # the source's base one pair off a 256-byte boundary; the destination too
        src = torch.zeros(span(sp, su, h) + 256, dtype=torch.uint8, device="cuda")
        s_off = (-src.data_ptr()) % 256 + A
        src[s_off : s_off + span(sp, su, h)] = torch.from_numpy(scatter(frame, h, sp, su, seed=401)).cuda()
        buf = guarded(span(dp, du, Hd) + 256)
        d_off = GUARD + (-(buf.data_ptr() + GUARD)) % 256 + A
        assert (src.data_ptr() + s_off) % 256 == A and (buf.data_ptr() + d_off) % 256 == A
        assert nv12_call(plan, src.data_ptr() + s_off, buf.data_ptr() + d_off, S, sl=(sp, su, 0), dl=(dp, du, 0)) == 0, (name, nat.load().pb_last_error())
        torch.cuda.synchronize()
        host = buf.cpu().numpy()
        got, padding = gather(host[d_off : d_off + span(dp, du, Hd)], Hd, Wd, dt, dp, du)
        assert np.array_equal(got, want), name
        assert bool((padding == SENTINEL).all()) and bool((host[:d_off] == SENTINEL).all()) and bool((host[d_off + span(dp, du, Hd):] == SENTINEL).all()), name
    # each rule broken by one sample: PB_ERR_INVALID before any launch, the named rule in the message, the destination untouched
    sp, su = layouts(h, w, S)["pitch_plus_a_pair"]
    dp, du = layouts(Hd, Wd, S)["pitch_plus_a_pair"]
    src = torch.zeros(span(sp, su, h) + 256, dtype=torch.uint8, device="cuda")
    ok = dict(so=0, do=0, sl=(sp, su, span(sp, su, h)), dl=(dp, du, span(dp, du, Hd)))
    broken = [(dict(so=S), b"multiples of"), (dict(do=S), b"multiples of")]
    for side, (p, u, n, rows, cols) in (("sl", (sp, su, span(sp, su, h), h, w)), ("dl", (dp, du, span(dp, du, Hd), Hd, Wd))):
        broken += [({side: (p + S, u + S * rows, 0)}, b"multiples of"), ({side: (p, u + S, 0)}, b"multiples of"), ({side: (p, u, n + S)}, b"multiples of"),
                   ({side: (cols * S - A, 0, 0)}, b"pitch smaller than a row"), ({side: (p, p * rows - A, 0)}, b"uv_offset smaller than the luma plane"),
                   ({side: (p, u, n - A)}, b"frame_stride smaller than a frame")]
    for change, message in broken:
        kw = {**ok, **change}
        fresh = guarded(span(dp, du, Hd) + 64)
        rc = nv12_call(plan, src.data_ptr() + kw["so"], fresh.data_ptr() + GUARD + kw["do"], S, 2, kw["sl"], kw["dl"])
        assert rc == INVALID and message in nat.load().pb_last_error(), (change, rc, nat.load().pb_last_error())
        torch.cuda.synchronize()
        assert bool((fresh == SENTINEL).all()), change
    for bad_S in (0, 3, 4):
        fresh = guarded(64)
        assert nv12_call(plan, src.data_ptr(), fresh.data_ptr() + GUARD, bad_S) == INVALID and b"bytes_per_sample" in nat.load().pb_last_error()


# ---- 5. batches -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [tc.case_by_name("D_photo_rot"), tc.case_by_name("D_pano_pano_rot")], ids=lambda c: c.name)
def test_three_frames_at_padded_strides_equal_three_single_launches(case):
    plan = H.pb_plan_private(case, bilinear=False)
    _, h, w, *_ = case.src
    Hd, Wd = case.dst[1], case.dst[2]
    for S, dt in SAMPLES:
        sb, db = 3 * h * w * S // 2, 3 * Hd * Wd * S // 2
        for pad in (2 * S, 48):
            ss, ds = sb + pad, db + pad
            src_host = np.random.default_rng(500 + S + pad).integers(0, 256, 3 * ss, dtype=np.uint8)  # (random bytes in the padding too)
            src = torch.from_numpy(src_host).cuda()
            buf = guarded(3 * ds)
            assert nv12_call(plan, src.data_ptr(), buf.data_ptr() + GUARD, S, 3, (0, 0, ss), (0, 0, ds)) == 0, nat.load().pb_last_error()
            torch.cuda.synchronize()
            assert guards_intact(buf)
            got = buf[GUARD:-GUARD].cpu().numpy()
            for f in range(3):
                single = run_nv12(plan, src_host[f * ss : f * ss + sb].view(dt).reshape(3 * h // 2, w))
                assert np.array_equal(got[f * ds : f * ds + db].view(dt).reshape(single.shape), single), (case.name, S, pad, f)
                assert bool((got[f * ds + db : (f + 1) * ds] == SENTINEL).all()), (case.name, S, pad, f)  # the padding is intact
    # ... and through Plan.remap_nv12: (N, 3h/2, w) in, (N, 3H/2, W) out
    frames = np.stack([random_frame(h, w, np.uint8, seed=510 + f) for f in range(3)])
    got = plan.remap_nv12(torch.from_numpy(frames).cuda()).cpu().numpy()
    assert got.shape == (3, 3 * Hd // 2, Wd) and all(np.array_equal(got[f], run_nv12(plan, frames[f])) for f in range(3))


# ---- 6. consistency with pb_remap_px ----------------------------------------------------------------------------------------------------
def test_the_luma_plane_is_pb_remap_px_of_the_plane_byte_for_byte():
    case = tc.case_by_name("M_photo_stereographic")
    plan = _mid_plan(case)
    _, h, w, *_ = case.src
    Hd = case.dst[1]
    for S, dt in SAMPLES:
        frame = random_frame(h, w, dt, seed=600 + S)
        got = run_nv12(plan, frame, fill=(0, 7, 9))
        luma = plan.remap_px(torch.from_numpy(np.ascontiguousarray(frame[:h])).cuda()).cpu().numpy()
        assert np.array_equal(got[:Hd], luma), S


# ---- 7. plans the kernel does not serve -------------------------------------------------------------------------------------------------
def test_unsupported_plans_say_so_and_write_nothing():
    L = nat.load()
    single, double = tc.case_by_name("D_photo_rot"), tc.case_by_name("E_stitch_195_raw")
    faithful = H.pb_plan_private(single, bilinear=False)
    faithful.set_mode(nat.MODE_FAITHFUL)
    for what, case, plan in (("deferred", single, H.pb_plan_private(single, defer=True, bilinear=False)), ("faithful", single, faithful),
                             ("double-fisheye", double, H.pb_plan_private(double, bilinear=False))):
        assert even(case), what
        _, h, w, *_ = case.src
        Hd, Wd = case.dst[1], case.dst[2]
        for S, dt in SAMPLES:
            assert L.pb_remap_nv12_supported(plan.handle, S) == 0 and not plan.nv12_supported(S), (what, S)
            assert not plan.px_supported(S)  # (exactly the plans pb_remap_px refuses)
            frame = torch.from_numpy(random_frame(h, w, dt, seed=700 + S)).cuda()
            buf = guarded(3 * Hd * Wd * S // 2)
            assert nv12_call(plan, frame.data_ptr(), buf.data_ptr() + GUARD, S) == UNSUPPORTED, (what, S)
            assert b"pb_index_map_i32" in L.pb_last_error()
            nat.check(L.pb_stream_sync(nat.current_stream()))
            torch.cuda.synchronize()
            assert bool((buf == SENTINEL).all()), (what, S)
            with pytest.raises(nat.PbError):
                plan.remap_nv12(frame)


# ---- 8. graph capture and streams -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,dt", SAMPLES)
def test_a_captured_launch_and_launches_on_three_streams_give_the_plain_bytes(S, dt):
    case = tc.case_by_name("M_pano_thoby")
    plan = _mid_plan(case)
    _, h, w, *_ = case.src
    Hd, Wd = case.dst[1], case.dst[2]
    src = torch.from_numpy(random_frame(h, w, dt, seed=800 + S)).cuda()
    want = plan.remap_nv12(src).view(torch.uint8)  # (bytes: (3H/2, W * S))
    torch.cuda.synchronize()
    # never allocates or synchronises: the call captures into a graph, and a replay writes the frame again
    g_out = torch.zeros((3 * Hd // 2, Wd * S), dtype=torch.uint8, device="cuda")
    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            assert nv12_call(plan, src.data_ptr(), g_out.data_ptr(), S, stream=int(side.cuda_stream)) == 0
    torch.cuda.current_stream().wait_stream(side)
    g_out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(g_out, want)
    # one launch on each of three streams
    streams = [torch.cuda.Stream() for _ in range(3)]
    outs = [torch.zeros((3 * Hd // 2, Wd * S), dtype=torch.uint8, device="cuda") for _ in streams]
    torch.cuda.synchronize()
    for s, o in zip(streams, outs):
        assert nv12_call(plan, src.data_ptr(), o.data_ptr(), S, stream=int(s.cuda_stream)) == 0
    torch.cuda.synchronize()
    assert all(torch.equal(o, want) for o in outs)


# ---- 9. the host pipeline ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt,dt", [("nv12", np.uint8), ("p010", np.uint16)])
def test_remap_ndarray_and_remap_frames_take_video_frames(fmt, dt):
    case = tc.case_by_name("D_photo_rot")
    plan = H.pb_plan_private(case, bilinear=False)
    idx = SMALL[f"{case.name}/idx"]
    _, h, w, *_ = case.src
    frames = [random_frame(h, w, dt, seed=900 + k) for k in (0, 1, 0)]  # (the middle one differs)
    wants = [nv12_ref.remap_frame(f, idx, h, w) for f in frames]
    one = _hostpipe.remap_ndarray(plan, frames[0], pixel_format=fmt)
    assert one.dtype == np.dtype(dt) and np.array_equal(one, wants[0])
    outs = [np.array(o) for o in batch.remap_frames(plan, frames, pixel_format=fmt)]
    assert len(outs) == 3 and all(o.dtype == np.dtype(dt) and np.array_equal(o, want) for o, want in zip(outs, wants))
    assert not np.array_equal(outs[1], outs[0])
    with pytest.raises(ValueError):
        list(batch.remap_frames(plan, [frames[0], frames[0][:-2]], pixel_format=fmt))
    with pytest.raises(ValueError):
        _hostpipe.remap_ndarray(plan, frames[0][:h], pixel_format=fmt)
