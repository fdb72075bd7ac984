"""HIP kernels against the oracle and the committed goldens, through the C ABI.

Bar: the integer source-index map, the uint8 output and (since round 4) the materialised float64 maps are bit-exact against the
committed goldens: the device chain runs the reference platform's own transcendental functions (csrc/pb_math.hpp).  The *fragile set*
stored in the fixture - pixels whose pre-truncation coordinate sits within 2^-40 (relative) of an integer, where a last-bit difference
in a libm could flip the truncation - is kept as a diagnostic: flips inside it are counted and must be ZERO against the goldens; only
comparisons with a LIVE oracle on a host whose NumPy is not the goldens' NumPy (tests/helpers.py) may use it as an allowance."""

import numpy as np
import pytest
import torch

from oracle import reference_path as orc
from tests import helpers as H
from tests.cases import small_cases

pytestmark = pytest.mark.gpu
SMALL = H.load_small()


def fragile_of(case):
    m = np.unpackbits(SMALL[f"{case.name}/fragile"])
    H_, W_ = case.dst[1], case.dst[2]
    return m[: H_ * W_].reshape(H_, W_).astype(bool)


def assert_equal_outside_fragile(got, want, fragile, what):
    bad = got != want
    if bad.ndim == 3:
        bad = bad.any(axis=2)
    n_bad = int(bad.sum())
    if n_bad:
        outside = int((bad & ~fragile).sum())
        assert outside == 0, f"{what}: {outside} mismatching pixels outside the fragile set ({n_bad} total)"
    return n_bad


@pytest.mark.parametrize("case", small_cases(), ids=lambda c: c.name)
def test_index_map_matches_golden(case):
    plan = H.pb_plan(case)
    fragile = fragile_of(case)
    n = case.name
    if case.src[0] == "double":
        idx, w = plan.index_map(weights=True)
        idx, w = idx.cpu().numpy(), w.cpu().numpy()
        nb = assert_equal_outside_fragile(idx[0], SMALL[f"{n}/idx_l"], fragile, "left index")
        nb += assert_equal_outside_fragile(idx[1], SMALL[f"{n}/idx_r"], fragile, "right index")
        for k, key in enumerate(("w_l", "w_r")):
            want = SMALL[f"{n}/{key}"].view(np.float64)
            # the oracle's BITS (NaN with NaN counts as equal): tests/test_hip_double_tiles.py shows what a last bit moves
            ok = (H.bits(w[k]) == H.bits(want)) | (np.isnan(w[k]) & np.isnan(want))
            assert ok.all(), f"blend weight {key}: {int((~ok).sum())} factors are not the reference's bits"
    else:
        idx = plan.index_map().cpu().numpy()
        nb = assert_equal_outside_fragile(idx, SMALL[f"{n}/idx"], fragile, "index")
    assert nb == 0, f"{nb} fragile-set flips (allowed by the bar, reported so they are seen)"


@pytest.mark.parametrize("case", small_cases(), ids=lambda c: c.name)
def test_fused_remap_matches_golden_and_oracle(case):
    frame = H.case_frame(case)
    src, cmap = H.pb_chain(case, frame)
    out = src.process_coordinate_map(cmap)
    assert isinstance(out, np.ndarray) and out.dtype == np.uint8 and out.shape == (case.dst[1], case.dst[2], 3)
    want = SMALL[f"{case.name}/u8"]
    assert assert_equal_outside_fragile(out, want, fragile_of(case), "u8 vs golden") == 0
    live = orc.remap(H.orc_proj(case.dst), H.orc_proj(case.src), frame, H.orc_rots(case))
    assert assert_equal_outside_fragile(out, live, fragile_of(case), "u8 vs live oracle") == 0


def ulp_diff(a, b):
    ai = a.view(np.int64).astype(np.int64)
    bi = b.view(np.int64).astype(np.int64)
    ai = np.where(ai < 0, np.int64(-(2**63)) - ai, ai)
    bi = np.where(bi < 0, np.int64(-(2**63)) - bi, bi)
    return np.abs(ai - bi)


@pytest.mark.parametrize("case", [c for c in small_cases() if c.keep_map], ids=lambda c: c.name)
def test_materialised_maps_within_ulps(case, capsys):
    """north_star asks for 1 ULP per channel on floating-point results; since round 4 the maps are the reference's BITS.  The device chain
    runs the functions the reference's NumPy ran when the goldens were made, restated operation for operation: glibc 2.35's sin / cos
    (`_fma` build), its internal sincos behind np.exp(1j x) (plain build), its atan2 (csrc/pb_math_glibc.hpp) and NumPy's own AVX-512
    arcsin / arccos / arctan / tan (csrc/pb_math_np.hpp); everything else in the chain is IEEE-exact arithmetic in the reference's order.
    get_coordinate_map and every rotation stage: 0 ulp on every value of every case (round 3: up to 24 / 159 ulp after a rotation)."""
    import photonbend_amd as pb

    n = case.name
    dst = H.pb_obj(case.dst)
    cmap = dst.get_coordinate_map()
    stages = [np.array(np.asarray(cmap))]
    for rot in case.rotations:
        cmap = pb.Rotation(*map(pb.utils.to_radians, rot)).rotate_coordinate_map(cmap)
        stages.append(np.array(np.asarray(cmap)))
    for k, got in enumerate(stages):
        want = SMALL[f"{n}/map{k}"].view(np.float64).reshape(got.shape)
        assert np.array_equal(got[..., 2], want[..., 2]), f"invalid flags differ at stage {k}"
        for ch, name in ((0, "lat"), (1, "lon")):
            g, w = got[..., ch], want[..., ch]
            both_nan = np.isnan(g) & np.isnan(w)
            d = ulp_diff(np.where(both_nan, 0.0, g), np.where(both_nan, 0.0, w))
            lens = case.dst[3] if case.dst[0] != "pano" else "pano"
            with capsys.disabled():
                print(f"\n[maps {n}: dst lens {lens}, stage {k} ({'after %d rotation(s)' % k if k else 'get_coordinate_map'}), {name}] "
                      f"max {int(d.max())} ulp, {int((d > 0).sum())} of {d.size} values differ", end="")
            assert int(d.max()) == 0, f"stage {k} {name} ({lens}): {int((d > 0).sum())} values differ from the reference's bits, max {int(d.max())} ulp"
            assert np.array_equal(np.isnan(g), np.isnan(w))


@pytest.mark.parametrize("case", [c for c in small_cases() if c.keep_map], ids=lambda c: c.name)
def test_ndarray_map_path_and_side_effects(case):
    """Feeding the reference's own float64 map (golden bits) through the
    materialised-map kernel reproduces the golden image, and the in-place zeroing
    of invalid pixels is mirrored into the caller's array."""
    import photonbend_amd as pb

    n = case.name
    k = len(case.rotations)
    shape = (case.dst[1], case.dst[2], 3)
    ref_map = np.array(SMALL[f"{n}/map{k}"].view(np.float64).reshape(shape))
    frame = H.case_frame(case)
    src = H.pb_obj(case.src, frame)
    given = ref_map.copy()
    out = src.process_coordinate_map(given)
    assert assert_equal_outside_fragile(out, SMALL[f"{n}/u8"], fragile_of(case), "ndarray map path") == 0
    expect = ref_map.copy()
    if case.src[0] == "pano":
        expect[..., :2][expect[..., 2] != 0.0] = 0.0
    assert np.array_equal(H.bits(given), H.bits(expect))
    # rotate an ndarray map: the input's invalid pixels get zeroed, flags carried
    m0 = np.array(SMALL[f"{n}/map0"].view(np.float64).reshape(shape))
    inp = m0.copy()
    rot = pb.Rotation(0.3, -0.2, 0.1)
    got = rot.rotate_coordinate_map(inp)
    inv = m0[..., 2] != 0.0
    assert (inp[..., :2][inv] == 0).all() and np.array_equal(inp[..., 2], m0[..., 2])
    want = orc.rotate_map(orc.rotation_matrix(0.3, -0.2, 0.1), m0.copy())
    assert np.array_equal(got[..., 2], want[..., 2])
    if H.live_numpy_is_the_goldens_numpy():  # the live oracle is this machine's NumPy: bit for bit when that is the goldens' NumPy
        assert np.array_equal(H.bits(got[..., :2]), H.bits(want[..., :2]))
    else:
        assert np.allclose(got[..., :2], want[..., :2], rtol=0, atol=1e-13, equal_nan=True)


def test_synth_frames_match_host_formula():
    from oracle.synth import synth_frame
    from photonbend_amd import _native as nat

    for (h, w, f, s, m) in [(17, 33, 0, 0, 0), (40, 80, 5, 7, 2), (48, 48, 3, 0, 1), (31, 64, 2**31 + 5, 2**32 - 1, 0)]:
        dev = nat.synth_frame(h, w, f, s, m).cpu().numpy()
        assert np.array_equal(dev, synth_frame(h, w, f, s, m)), (h, w, f, s, m)


def test_batch_frames_and_tensor_io():
    """N frames in one launch == N single launches; CUDA tensors stay on device."""
    import photonbend_amd as pb
    from tests.cases import case_by_name

    case = case_by_name("D_photo_rot")
    plan = H.pb_plan(case)
    frames = np.stack([H.case_frame(case, f) for f in range(5)])
    dev = torch.from_numpy(frames).cuda()
    batched = plan.remap(dev)
    assert batched.is_cuda and tuple(batched.shape) == (5, 48, 48, 3)
    for f in range(5):
        single = plan.remap(dev[f])
        assert torch.equal(single, batched[f])
        want = orc.remap(H.orc_proj(case.dst), H.orc_proj(case.src), frames[f], H.orc_rots(case))
        assert np.array_equal(batched[f].cpu().numpy(), want)
    src = pb.PanoramaImage(dev[1])
    _, cmap = H.pb_chain(case)
    out = src.process_coordinate_map(cmap)
    assert isinstance(out, torch.Tensor) and out.is_cuda and torch.equal(out, batched[1])


def test_ragged_sizes_and_unaligned_tails():
    """Widths/heights that leave a tail in the 4-pixel store groups, 1xN and Nx1."""
    import photonbend_amd as pb

    for (h, w) in [(1, 1), (1, 7), (7, 1), (3, 5), (5, 3), (9, 13)]:
        dst = orc.Proj("camera", h, w, "equidistant", 3.0, None)
        srcp = orc.Proj("pano", 16, 32)
        frame = H.synth_frame(16, 32, 1, 0, 0)
        want = orc.remap(dst, srcp, frame)
        d = pb.CameraImage(np.zeros((h, w, 3), np.uint8), 3.0, pb.equidistant())
        got = pb.PanoramaImage(frame).process_coordinate_map(d.get_coordinate_map())
        assert np.array_equal(got, want), (h, w)


@pytest.mark.parametrize("case", [c for c in small_cases() if c.keep_map], ids=lambda c: c.name)
def test_map_projection_matches_reference(case):
    """f-3: map_projection on the reference's own float64 map -> the reference's colour map, bit for bit
    (pure IEEE work: subtract, multiply, round-half-even, wrap to uint8), plus the in-place side effect."""
    import photonbend_amd as pb

    g = np.load(H.GOLD + "/mapproj.npz")
    shape = (case.dst[1], case.dst[2], 3)
    m = np.array(SMALL[f"{case.name}/map{len(case.rotations)}"].view(np.float64).reshape(shape))
    given = m.copy()
    out = pb.map_projection(given)
    assert out.dtype == np.uint8 and np.array_equal(out, g[f"{case.name}/out"])
    expect = m.copy()
    expect[..., :2][expect[..., 2] != 0.0] = 0.0
    assert np.array_equal(H.bits(given), H.bits(expect))
