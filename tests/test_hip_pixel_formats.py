"""pb_remap_px: grey, 16-bit and RGBA frames through the tile kernel pb_px_hot_kernel - the bytes of NumPy fancy
indexing with the reference's index map, for every pixel size, tile class, edge, alignment and launch shape.  Every comparison is exact
equality; images are independent random bytes (a wrong index shows), destinations sit between sentinel bytes that must survive."""

import os

import numpy as np
import pytest
import torch

import photonbend_amd as pb
from oracle import reference_path as orc
from oracle.synth import synth_image
from photonbend_amd import _hostpipe, batch
from photonbend_amd import _native as nat
from tests import cases as tc
from tests import cubemap_cases as cc
from tests import cubemap_ref as cr
from tests import helpers as H
from tests import polynomial_cases as pc
from tests.cases import Case, cam, inscribed, pano

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 4, 6, 8)
# (bytes per pixel, sample dtype, trailing shape): B = 2 both as uint16 (H, W) and as uint8 (H, W, 2)
FORMATS = [(1, np.uint8, ()), (2, np.uint16, ()), (2, np.uint8, (2,)), (4, np.uint8, (4,)), (6, np.uint16, (3,)), (8, np.uint16, (4,))]
GUARD = 64  # sentinel bytes on either side of a destination
SENTINEL = 0xA5
INVALID, UNSUPPORTED = -1, -3
SMALL = H.load_small()
GOLD_CUBE = np.load(os.path.join(H.GOLD, "cubemap.npz"))
GOLD_POLY = np.load(os.path.join(H.GOLD, "polynomial.npz"))


def random_bytes(h, w, B, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, B), dtype=np.uint8)


def fancy(img_bytes, idx):
    """NumPy fancy indexing of an (h, w, B) image with an int32 index map, black where the index is -1."""
    flat = img_bytes.reshape(-1, img_bytes.shape[-1])
    out = flat[np.where(idx < 0, 0, idx)]
    out[idx < 0] = 0
    return out


def guarded(nbytes):
    """A device buffer of sentinel bytes with `nbytes` of payload between two guards."""
    return torch.full((nbytes + 2 * GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")


def guards_intact(buf):
    return bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[-GUARD:] == SENTINEL).all())


def px_call(plan, src_ptr, dst_ptr, B, n=1, ss=0, ds=0, stream=None):
    return nat.load().pb_remap_px(plan.handle, src_ptr, dst_ptr, n, ss, ds, B, nat.current_stream() if stream is None else stream)


def run_px(plan, img_bytes, B):
    """One pb_remap_px launch of an (h, w, B) byte image -> (H, W, B) bytes; the guards around the destination must survive."""
    Hd, Wd = plan.dst.height, plan.dst.width
    src = torch.from_numpy(img_bytes).cuda()
    buf = guarded(Hd * Wd * B)
    assert px_call(plan, src.data_ptr(), buf.data_ptr() + GUARD, B) == 0, nat.load().pb_last_error()
    torch.cuda.synchronize()
    assert guards_intact(buf), "pb_remap_px wrote outside the destination frame"
    return buf[GUARD:-GUARD].cpu().numpy().reshape(Hd, Wd, B)


def n_diff(got, want):
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    return int((got != want).reshape(got.shape[0], got.shape[1], -1).any(axis=2).sum())


# ---- 1. the small case matrices against the reference's golden index maps -------------------------------------------------------------
def _small_plans():
    out = []
    for c in tc.small_cases():
        if c.src[0] != "double":
            fragile = np.unpackbits(SMALL[f"{c.name}/fragile"])[: c.dst[1] * c.dst[2]].reshape(c.dst[1], c.dst[2]).astype(bool)
            out.append((c, lambda c=c: H.pb_plan_private(c, bilinear=False), SMALL[f"{c.name}/idx"], fragile))
    for mod, gold in ((cc, GOLD_CUBE), (pc, GOLD_POLY)):
        for c in mod.small_cases():
            if c.src[0] != "double":
                def make(c=c, mod=mod):
                    src, cmap = mod.pb_chain(c, image=np.zeros((c.src[1], c.src[2], 3), np.uint8))
                    return nat.Plan(cmap.dst_proj, cmap.rotations, src._proj("src"), bilinear=False)
                out.append((c, make, gold[f"{c.name}/idx"], None))
    return out


SMALL_PLANS = _small_plans()


@pytest.mark.parametrize("case,make_plan,idx,fragile", SMALL_PLANS, ids=[p[0].name for p in SMALL_PLANS])
def test_small_cases_equal_fancy_indexing_with_the_golden_index(case, make_plan, idx, fragile):
    plan = make_plan()
    _, h, w, *_ = case.src
    Hd, Wd = idx.shape
    for k, (B, dt, tail) in enumerate(FORMATS):
        assert plan.px_supported(B), (case.name, B)
        img = random_bytes(h, w, B, seed=100 + k)
        want = fancy(img, idx)
        # through Plan.remap_px with the typed array: same shape tail and dtype back
        typed = np.ascontiguousarray(img).view(dt).reshape((h, w) + tail)
        buf = guarded(Hd * Wd * B)
        out = buf[GUARD:-GUARD].view(nat.torch_dtype(dt)).reshape((Hd, Wd) + tail)
        got = plan.remap_px(torch.from_numpy(typed).cuda(), out=out)
        torch.cuda.synchronize()
        assert got is out and guards_intact(buf), (case.name, B)
        got = buf[GUARD:-GUARD].cpu().numpy().reshape(Hd, Wd, B)
        bad = (got != want).any(axis=2)
        if fragile is not None:  # (the treatment of tests/test_hip_parity.py: nothing outside the fragile set, and no flip inside it either)
            assert int((bad & ~fragile).sum()) == 0, f"{case.name} B={B}: {int((bad & ~fragile).sum())} pixels differ outside the fragile set"
        assert int(bad.sum()) == 0, f"{case.name} B={B} {np.dtype(dt)}{tail}: {int(bad.sum())} pixels differ"


# ---- 2. every tile class at mid size, against the oracle --------------------------------------------------------------------------------
MID = [
    tc.case_by_name("M_photo_stereographic"),  # an inscribed fisheye destination: MASKED ring tiles, BLACK corners, DIRECT and LEAN inside
    tc.case_by_name("M_pano_thoby"),           # a fisheye source: fix pixels at its rim
    tc.case_by_name("M_ident_pano"),           # every coordinate on an integer
    Case("KM_cube384_pano_rot", pano(640, 1280), cc.cube(384), [(5, 60, -20)]),  # face seams: failed tiles; the truncation quirk: fix pixels
]


def _mid_plan(case):
    src, cmap = cc.pb_chain(case, image=np.zeros((case.src[1], case.src[2], 3), np.uint8))
    return nat.Plan(cmap.dst_proj, cmap.rotations, src._proj("src"), bilinear=False)


@pytest.mark.parametrize("case", MID, ids=lambda c: c.name)
def test_mid_cases_equal_fancy_indexing_with_the_oracle_index(case):
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
    for B in SIZES:
        assert plan.px_supported(B)
        img = random_bytes(h, w, B, seed=200 + B)
        bad = (run_px(plan, img, B) != fancy(img, idx)).any(axis=2)
        assert int((bad & ~fragile).sum()) == 0, f"{case.name} B={B}: {int((bad & ~fragile).sum())} pixels differ outside the fragile set"
        if exact:
            assert int(bad.sum()) == 0, f"{case.name} B={B}: {int(bad.sum())} pixels differ"


def test_mid_cases_contain_every_tile_class():
    """The coverage of the test above cannot go silently: its plans hold failed tiles, fix pixels, LEAN, DIRECT and BLACK tiles."""
    total = {"fix_tiles": 0, "fix_pixels": 0, "lean_tiles": 0, "direct_tiles": 0, "black_tiles": 0}
    for case in MID:
        info = _mid_plan(case).info()
        assert info["fast_path"], case.name
        for k in total:
            total[k] += info[k]
    assert all(v >= 1 for v in total.values()), total


# ---- 3. edges ---------------------------------------------------------------------------------------------------------------------------
EDGES = [
    Case("edge_1x1", cam(1, 1, "equidistant", 172), pano(16, 32)),
    Case("edge_1x3", cam(1, 3, "equidistant", 172), pano(16, 32)),
    Case("edge_33x35_src3x5", cam(33, 35, "equidistant", 180), pano(3, 5), [(10, 20, 30)]),
    Case("edge_35x33_src2x2", pano(35, 33), pano(2, 2), [(12, 34, 56)]),
    Case("edge_33x35_cam_src", cam(33, 35, "equisolid", 190), cam(48, 48, "equidistant", 360, inscribed(48)), [(30, 45, 10)]),
    # (the reference's panorama identity stops one row short of the source's end; the cases below it and the tiny sources above reach
    #  the source's very last pixel, whose load must not touch a byte past the frame)
    Case("edge_pano_identity", pano(32, 64), pano(32, 64)),
    Case("edge_pano_2x_last_pixel", pano(64, 128), pano(32, 64)),
    Case("edge_pano_pitch_last_pixel", pano(32, 64), pano(32, 64), [(10, 0, 0)]),
]
SAMPLES_LAST_PIXEL = ("edge_33x35_src3x5", "edge_35x33_src2x2", "edge_pano_2x_last_pixel", "edge_pano_pitch_last_pixel")


@pytest.mark.parametrize("case", EDGES, ids=lambda c: c.name)
def test_edges_partial_tiles_tiny_sources_and_the_last_pixel(case):
    with np.errstate(all="ignore"):
        idx = orc.remap_index(H.orc_proj(case.dst), H.orc_proj(case.src), H.orc_rots(case))
        fragile = orc.fragile_mask(orc.pretrunc(H.orc_proj(case.dst), H.orc_proj(case.src), H.orc_rots(case)))
    if case.name in SAMPLES_LAST_PIXEL:
        assert int(idx.max()) == case.src[1] * case.src[2] - 1  # the source's very last pixel is sampled
    plan = H.pb_plan_private(case, bilinear=False)
    _, h, w, *_ = case.src
    exact = H.live_numpy_is_the_goldens_numpy()
    for B in SIZES:
        assert plan.px_supported(B)
        img = random_bytes(h, w, B, seed=300 + B)
        bad = (run_px(plan, img, B) != fancy(img, idx)).any(axis=2)
        assert int((bad & ~fragile).sum()) == 0, (case.name, B, int(bad.sum()))
        if exact:
            assert int(bad.sum()) == 0, (case.name, B, int(bad.sum()))


# ---- 4. alignment -----------------------------------------------------------------------------------------------------------------------
ALIGN_CASE = tc.case_by_name("D_photo_rot")


@pytest.mark.parametrize("B", SIZES)
def test_pointers_offset_by_one_sample_and_offsets_below_the_rule(B):
    case = ALIGN_CASE
    plan = H.pb_plan_private(case, bilinear=False)
    _, h, w, *_ = case.src
    Hd, Wd = case.dst[1], case.dst[2]
    img = random_bytes(h, w, B, seed=400 + B)
    want = run_px(plan, img, B)
    assert n_diff(want, fancy(img, SMALL[f"{case.name}/idx"])) == 0
    a = nat.px_align(B)
    assert a == {1: 1, 2: 2, 4: 4, 6: 2, 8: 4}[B]
    # source and destination one sample off a 256-byte boundary: the bytes of the aligned call
    src = torch.zeros(h * w * B + 16, dtype=torch.uint8, device="cuda")
    src[a : a + h * w * B] = torch.from_numpy(img.reshape(-1)).cuda()
    buf = guarded(Hd * Wd * B + a)
    assert (src.data_ptr() + a) % (2 * a) == a and (buf.data_ptr() + GUARD + a) % (2 * a) == a
    assert px_call(plan, src.data_ptr() + a, buf.data_ptr() + GUARD + a, B) == 0, nat.load().pb_last_error()
    torch.cuda.synchronize()
    assert bool((buf[: GUARD + a] == SENTINEL).all()) and bool((buf[-GUARD:] == SENTINEL).all())
    got = buf[GUARD + a : GUARD + a + Hd * Wd * B].cpu().numpy().reshape(Hd, Wd, B)
    assert n_diff(got, want) == 0
    # below the rule: PB_ERR_INVALID before any launch, whichever argument is off; the destination stays untouched
    for off in range(1, a):
        for so, do, ss, ds in ((off, 0, 0, 0), (0, off, 0, 0), (0, 0, h * w * B + off, 0), (0, 0, 0, Hd * Wd * B + off)):
            fresh = guarded(Hd * Wd * B + 8)
            assert px_call(plan, src.data_ptr() + a + so, fresh.data_ptr() + GUARD + do, B, 1, ss, ds) == INVALID, (B, so, do, ss, ds)
            assert b"multiples of" in nat.load().pb_last_error()
            torch.cuda.synchronize()
            assert bool((fresh == SENTINEL).all())


# ---- 5. batches -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [tc.case_by_name("D_photo_rot"), tc.case_by_name("B_pano_odd")], ids=lambda c: c.name)
def test_three_frames_at_padded_strides_equal_three_single_launches(case):
    plan = H.pb_plan_private(case, bilinear=False)
    _, h, w, *_ = case.src
    Hd, Wd = case.dst[1], case.dst[2]
    for B in SIZES:
        sb, db = h * w * B, Hd * Wd * B
        for pad in (B, 48):
            ss, ds = sb + pad, db + pad
            rng = np.random.default_rng(500 + B + pad)
            src_host = rng.integers(0, 256, 3 * ss, dtype=np.uint8)  # (random bytes in the padding too)
            src = torch.from_numpy(src_host).cuda()
            buf = guarded(3 * ds)
            assert px_call(plan, src.data_ptr(), buf.data_ptr() + GUARD, B, 3, ss, ds) == 0, nat.load().pb_last_error()
            torch.cuda.synchronize()
            assert guards_intact(buf)
            got = buf[GUARD:-GUARD].cpu().numpy()
            for f in range(3):
                single = run_px(plan, src_host[f * ss : f * ss + sb].reshape(h, w, B), B)
                assert np.array_equal(got[f * ds : f * ds + db].reshape(Hd, Wd, B), single), (case.name, B, pad, f)
                assert bool((got[f * ds + db : (f + 1) * ds] == SENTINEL).all()), (case.name, B, pad, f)  # the padding is intact


# ---- 6. three-byte pixels are pb_remap_u8 -----------------------------------------------------------------------------------------------
def test_three_byte_pixels_are_pb_remap_u8_byte_for_byte():
    case = tc.case_by_name("M_photo_stereographic")  # (a mid case: its 16-byte-aligned call takes the windowed kernel)
    plan = _mid_plan(case)
    _, h, w, *_ = case.src
    Hd, Wd = case.dst[1], case.dst[2]
    img = random_bytes(h, w, 3, seed=600)
    L = nat.load()
    assert plan.px_supported(3)
    raw = torch.zeros(h * w * 3 + 16, dtype=torch.uint8, device="cuda")
    for off in (0, 3):  # 16-byte aligned: WIN; three bytes off: the direct-gather route
        raw[off : off + h * w * 3] = torch.from_numpy(img.reshape(-1)).cuda()
        a, b = guarded(Hd * Wd * 3), guarded(Hd * Wd * 3)
        assert L.pb_remap_u8(plan.handle, raw.data_ptr() + off, a.data_ptr() + GUARD, 1, 0, 0, nat.current_stream()) == 0
        assert px_call(plan, raw.data_ptr() + off, b.data_ptr() + GUARD, 3) == 0
        torch.cuda.synchronize()
        assert guards_intact(b) and torch.equal(a, b), off
    # ... on plans the tile kernel of the other sizes refuses, too: a deferred plan runs pb_remap_u8's float64 kernel
    lazy = H.pb_plan_private(tc.case_by_name("D_photo_rot"), defer=True, bilinear=False)
    small = torch.from_numpy(random_bytes(64, 128, 3, seed=601)).cuda()
    assert lazy.px_supported(3) and torch.equal(lazy.remap_px(small), lazy.remap(small))


# ---- 7. plans the kernel does not serve -------------------------------------------------------------------------------------------------
def _unsupported_plans():
    single, double = tc.case_by_name("D_photo_rot"), tc.case_by_name("E_stitch_195_raw")
    faithful = H.pb_plan_private(single, bilinear=False)
    faithful.set_mode(nat.MODE_FAITHFUL)
    return [("deferred", single, H.pb_plan_private(single, defer=True, bilinear=False)), ("faithful", single, faithful),
            ("double-fisheye", double, H.pb_plan_private(double, bilinear=False))]


def test_unsupported_plans_say_so_and_write_nothing():
    L = nat.load()
    for what, case, plan in _unsupported_plans():
        _, h, w, *_ = case.src
        Hd, Wd = case.dst[1], case.dst[2]
        for B in SIZES:
            assert L.pb_remap_px_supported(plan.handle, B) == 0 and not plan.px_supported(B), (what, B)
            src = torch.from_numpy(random_bytes(h, w, B, seed=700 + B)).cuda()
            buf = guarded(Hd * Wd * B)
            assert px_call(plan, src.data_ptr(), buf.data_ptr() + GUARD, B) == UNSUPPORTED, (what, B)
            msg = L.pb_last_error()
            assert b"pb_index_map_i32" in msg and b"pb_gather_px" in msg, msg
            nat.check(L.pb_stream_sync(nat.current_stream()))
            torch.cuda.synchronize()
            assert bool((buf == SENTINEL).all()), (what, B)
            with pytest.raises(nat.PbError):
                plan.remap_px(src)
        assert L.pb_remap_px_supported(plan.handle, 3) == 1  # (pb_remap_u8 takes every plan)
    assert L.pb_remap_px_supported(plan.handle, 5) == INVALID and L.pb_remap_px_supported(None, 4) == INVALID


# ---- 8. the facade ----------------------------------------------------------------------------------------------------------------------
GOLD_GENERIC = np.load(os.path.join(H.GOLD, "generic.npz"))
FACADE = [(n, c, layout) for n, c, layout in tc.generic_cases()
          if layout in ("RGBA", "L", "I;16", "RGB16") and c.src[0] != "double" and len(c.rotations) <= nat.PB_MAX_ROTATIONS
          and "custom" not in (c.src[3], c.dst[3])]


def _no_index_map(*args, **kwargs):
    raise AssertionError("Plan.index_map was called: the image did not take pb_remap_px")


def _generic_chain(case, img):
    cmap = H.pb_obj(case.dst).get_coordinate_map()
    for rot in case.rotations:
        cmap = pb.Rotation(*map(pb.utils.to_radians, rot)).rotate_coordinate_map(cmap)
    return H.pb_obj(case.src, img), cmap


@pytest.mark.parametrize("name,case,layout", FACADE, ids=[c[0] for c in FACADE])
def test_facade_takes_one_launch_for_grey_rgba_and_16_bit_images(name, case, layout, monkeypatch):
    """process_coordinate_map on a prepared plan (PB_PLAN_EAGER=1: from the first use on) never asks for an index map: ndarray in ->
    ndarray out and CUDA tensor in -> CUDA tensor out are the reference's bytes (tests/golden/generic.npz)."""
    assert len(FACADE) == 6
    monkeypatch.setenv("PB_PLAN_EAGER", "1")
    monkeypatch.setattr(nat.Plan, "index_map", _no_index_map)
    want = GOLD_GENERIC[name]
    _, h, w, *_ = case.src
    img = synth_image(h, w, layout, frame=3, circle_mask=case.mask)
    src, cmap = _generic_chain(case, img)
    got = src.process_coordinate_map(cmap)
    assert isinstance(got, np.ndarray) and got.dtype == want.dtype and n_diff(got, want) == 0, name
    src, cmap = _generic_chain(case, torch.from_numpy(img).cuda())
    got_t = src.process_coordinate_map(cmap)
    assert isinstance(got_t, torch.Tensor) and got_t.is_cuda and n_diff(got_t.cpu().numpy(), want) == 0, name


def test_remap_ndarray_and_remap_frames_take_rgba(monkeypatch):
    name, case, layout = next(c for c in FACADE if c[0] == "G_pano_RGBA")
    monkeypatch.setattr(nat.Plan, "index_map", _no_index_map)
    want = GOLD_GENERIC[name]
    _, h, w, *_ = case.src
    img = synth_image(h, w, layout, frame=3, circle_mask=case.mask)
    rots = [pb.Rotation(*map(pb.utils.to_radians, r)) for r in case.rotations]
    plan = batch.plan_for(H.pb_obj(case.dst), rots, H.pb_obj(case.src, img))
    if not plan.px_supported(4):  # (the facade's cache entry may still be deferred: this test is about the prepared one)
        plan = H.pb_plan_private(case, bilinear=False)
    one = _hostpipe.remap_ndarray(plan, img)
    assert one.dtype == want.dtype and n_diff(one, want) == 0
    outs = [np.array(o) for o in batch.remap_frames(plan, [img, img[::-1].copy(), img])]
    assert len(outs) == 3 and n_diff(outs[0], want) == 0 and n_diff(outs[2], want) == 0
    assert n_diff(outs[1], _hostpipe.remap_ndarray(plan, img[::-1].copy())) == 0 and n_diff(outs[1], want) != 0
    with pytest.raises(ValueError):
        list(batch.remap_frames(plan, [img, img[:, :, :3].copy()]))  # (all frames of a call share the first frame's format)


# ---- 9. graph capture and streams -------------------------------------------------------------------------------------------------------
def test_a_captured_launch_and_launches_on_three_streams_give_the_plain_bytes():
    case = tc.case_by_name("M_pano_thoby")
    plan = _mid_plan(case)
    _, h, w, *_ = case.src
    Hd, Wd = case.dst[1], case.dst[2]
    B = 4
    src = torch.from_numpy(random_bytes(h, w, B, seed=900)).cuda()
    want = plan.remap_px(src)
    torch.cuda.synchronize()
    # never allocates or synchronises: the call captures into a graph, and a replay writes the frame again
    g_out = torch.zeros((Hd, Wd, B), dtype=torch.uint8, device="cuda")
    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            assert px_call(plan, src.data_ptr(), g_out.data_ptr(), B, stream=int(side.cuda_stream)) == 0
    torch.cuda.current_stream().wait_stream(side)
    g_out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(g_out, want)
    # one launch on each of three streams
    streams = [torch.cuda.Stream() for _ in range(3)]
    outs = [torch.zeros((Hd, Wd, B), dtype=torch.uint8, device="cuda") for _ in streams]
    torch.cuda.synchronize()
    for s, o in zip(streams, outs):
        assert px_call(plan, src.data_ptr(), o.data_ptr(), B, stream=int(s.cuda_stream)) == 0
    torch.cuda.synchronize()
    assert all(torch.equal(o, want) for o in outs)
