"""f-4: the opt-in bilinear mode against OUR written-down definition (oracle.remap_bilinear; the reference
has no bilinear behaviour - parity unpinned).  Tolerance: the hot kernel evaluates the source coordinate
from float32 tile models (~1e-5 px) and blends in float32, so a channel may land 1 LSB from the float64
definition when the blended value sits near x.5; pixels on a validity / image boundary may flip between
black and sampled."""

import os

import numpy as np
import pytest
import torch

from oracle import reference_path as orc
from oracle.synth import synth_frame
from photonbend_amd import _native as nat
from tests import helpers as H
from tests.cases import Case, cam, case_by_name, dbl, full_cases, inscribed, pano
from tests.interp_cases import TINY_BILINEAR

pytestmark = pytest.mark.gpu

CASES = [
    Case("bl_photo", cam(160, 160, "equidistant", 360, inscribed(160)), pano(128, 256)),
    Case("bl_photo_rot", cam(150, 170, "equisolid", 200, 70.0), pano(100, 200), [(30, 45, 10)]),
    Case("bl_pano", pano(96, 192), cam(140, 140, "equidistant", 360, inscribed(140))),
    Case("bl_alter", cam(128, 128, "stereographic", 200, inscribed(128)), cam(150, 150, "equidistant", 220, inscribed(150)), [(-20, 10, 100)]),
    Case("bl_pano_pano", pano(80, 160), pano(64, 128), [(12, 34, 56)]),
    Case("bl_double_dst", ("double", 64, 128, "equidistant", 195.0, None), pano(96, 192)),
    Case("bl_double_src", pano(96, 192), ("double", 120, 240, "equidistant", 195.0, None)),
    Case("bl_double_src_rot", cam(128, 128, "equidistant", 200, inscribed(128)), ("double", 120, 241, "equisolid", 200.0, None), [(3, 90, -7)]),
    # 0.5 K double-fisheye sources: dozens of window / direct / guarded tiles per eye, row-table, unit and latitude-table weights
    Case("bl_stitch_195", pano(512, 1024), ("double", 480, 960, "equidistant", 195.0, None)),
    Case("bl_stitch_180_rot", pano(384, 768), ("double", 480, 960, "equidistant", 180.0, None), [(3, 90, -7)]),
    Case("bl_fisheye_from_double", cam(400, 400, "equidistant", 360, inscribed(400)), ("double", 486, 972, "equisolid", 200.0, None), [(20, 30, 40)]),
]


def smooth_frame(h, w):
    """A smooth test pattern, periodic in x (a panorama's columns wrap): on noise, a sawtooth or a seam every pixel
    would sit on an interpolation edge, and the comparison would measure the pattern, not the sampler."""
    yy, xx = np.mgrid[0:h, 0:w]
    ph = 2.0 * np.pi * (xx + 0.5) / w
    r = 127.5 + 120.0 * np.cos(ph)
    g = 10.0 + 235.0 * yy / max(1, h - 1)
    b = 127.5 + 120.0 * np.sin(ph) * np.cos(np.pi * (yy + 0.5) / h)
    return np.rint(np.stack([r, g, b], axis=2)).astype(np.uint8)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
@pytest.mark.parametrize("mode", [nat.MODE_AUTO, nat.MODE_FAITHFUL], ids=["tiles", "faithful"])
def test_bilinear_matches_definition(case, mode):
    od, os_ = H.orc_proj(case.dst), H.orc_proj(case.src)
    rots = H.orc_rots(case)
    frame = smooth_frame(case.src[1], case.src[2])
    want = orc.remap_bilinear(od, os_, frame, rots)
    plan = H.pb_plan_private(case)  # (a plan of its own: the facade's cache entry is shared with other tests and must keep its mode)
    plan.set_mode(mode)
    got = plan.remap(torch.from_numpy(frame).cuda(), interpolation="bilinear").cpu().numpy()
    d = np.abs(got.astype(np.int16) - want.astype(np.int16)).max(axis=2)
    if case.src[0] == "double":
        d = np.minimum(d, 256 - d)  # the blend's cast wraps mod 256 like the reference's
    n = d.size
    # <= 1 LSB EVERYWHERE except on the rim of the black regions (one pixel either side of a black / sampled edge of
    # the definition's output), where a coordinate within float32 reach of a validity or image boundary may flip a
    # pixel between black and sampled; a double source additionally has the seam of its blend band, where a factor of
    # up to 1.0 multiplies a 1-LSB tap difference of EACH eye (2 LSB)
    black = (want == 0).all(axis=2)
    rim = np.zeros_like(black)
    for dy, dx in ((0, 1), (1, 0), (0, -1), (-1, 0), (1, 1), (1, -1), (-1, 1), (-1, -1)):
        rim |= black != np.roll(np.roll(black, dy, axis=0), dx, axis=1)
    limit = 1
    inside = d[~rim]
    assert int((inside > limit).sum()) == 0, f"{int((inside > limit).sum())} pixels off the black rims differ by more than {limit} LSB (max {int(inside.max())})"
    assert int(rim.sum()) <= n // 8 and int((d > 0).sum()) <= n // 8, f"{int((d > 0).sum())} of {n} pixels differ"


def test_bilinear_api_and_noise_frame():
    import photonbend_amd as pb

    case = case_by_name("D_photo_rot")
    frame = synth_frame(64, 128, frame=3)
    src, cmap = H.pb_chain(case, frame)
    out = src.process_coordinate_map(cmap, interpolation="bilinear")
    near = src.process_coordinate_map(cmap)
    assert out.shape == near.shape and out.dtype == np.uint8 and not np.array_equal(out, near)
    want = orc.remap_bilinear(H.orc_proj(case.dst), H.orc_proj(case.src), frame, H.orc_rots(case))
    d = np.abs(out.astype(np.int16) - want.astype(np.int16)).max(axis=2)
    assert int((d > 1).sum()) <= 16
    with pytest.raises(ValueError):
        src.process_coordinate_map(cmap, interpolation="bicubic")
    # round 5: a materialised map and images beyond uint8 RGB are served too (tests/test_hip_bilinear_map.py); what stays refused are
    # sample types the mode does not define
    dense = src.process_coordinate_map(np.array(np.asarray(cmap)), interpolation="bilinear")
    assert dense.shape == out.shape and int((np.abs(dense.astype(np.int16) - want.astype(np.int16)) > 1).sum()) == 0
    grey = pb.PanoramaImage(np.zeros((64, 128), np.uint8))
    assert grey.process_coordinate_map(cmap, interpolation="bilinear").shape == near.shape[:2]
    with pytest.raises(NotImplementedError):
        pb.PanoramaImage(np.zeros((64, 128, 3), np.float32)).process_coordinate_map(cmap, interpolation="bilinear")


def test_bilinear_folds_chains_beyond_one_fused_plan():
    """the reference applies every -r in turn (scripts/commands/make_photo.py:128-131).  Nine rotations leave the
    fused plan; the nearest mode then goes through the materialised-map kernels, the bilinear mode (no reference bits to keep) folds
    the chain into one matrix product and stays on the tile path: within 1 LSB of the definition applied rotation by rotation."""
    import photonbend_amd as pb

    frame = smooth_frame(128, 256)
    dst = pb.CameraImage(np.zeros((96, 96, 3), np.uint8), pb.utils.to_radians(180), pb.equidistant())
    cmap = dst.get_coordinate_map()
    rots = [(0.1 * k, -0.05 * k, 0.02) for k in range(9)]
    for r in rots:
        cmap = pb.Rotation(*r).rotate_coordinate_map(cmap)
    src = pb.PanoramaImage(frame)
    got = src.process_coordinate_map(cmap, interpolation="bilinear")
    want = orc.remap_bilinear(orc.Proj("camera", 96, 96, "equidistant", orc.to_radians(180), None), orc.Proj("pano", 128, 256), frame, rots)
    d = np.abs(got.astype(np.int16) - want.astype(np.int16)).max(axis=2)
    rim = _rim_of((want == 0).all(axis=2))
    assert int((d[~rim] > 1).sum()) == 0, f"{int((d[~rim] > 1).sum())} pixels beyond 1 LSB (max {int(d[~rim].max())})"
    assert src.process_coordinate_map(cmap).shape == (96, 96, 3)  # the nearest mode: every rotation in turn, as before


def _rim_of(black):
    """one pixel either side of a black / sampled edge of the definition's output (8-neighbourhood)"""
    rim = np.zeros_like(black)
    for dy, dx in ((0, 1), (1, 0), (0, -1), (-1, 0), (1, 1), (1, -1), (-1, 1), (-1, -1)):
        rim |= black != np.roll(np.roll(black, dy, axis=0), dx, axis=1)
    return rim


@pytest.mark.parametrize("case", full_cases(), ids=lambda c: c.name)
def test_bilinear_full_size_against_definition(case):
    """the bilinear mode at the sizes it is benchmarked at (c1, c2, c3, c5 at 180 and 195 degrees), on the
    synthetic NOISE frame (255 LSB per pixel of coordinate error), against oracle.remap_bilinear's values captured at full size
    (tests/golden/full_bilinear.npz, oracle/make_goldens.py --full-bilinear): 65 536 seeded samples, two whole 128 x 128 crops
    (centre; rim / seam), the number of black pixels and the sum of all bytes.  +-1 LSB EVERYWHERE, the double blend and the one-pixel
    rims of the black regions included, and no sample black in one output and not in the other (round 5: the allowances of rounds 3-4 -
    2 LSB on the blend, flips, rim pixels - were not in use any more; tests/test_hip_bilinear_map.py checks every pixel)."""
    pin = H.load_full()[case.name]
    gold = np.load(os.path.join(H.GOLD, "full_bilinear.npz"))
    plan = H.pb_plan_private(case)
    info = plan.info()
    assert info["fast_path"]
    _, h, w, *_ = case.src
    frame = nat.synth_frame(h, w, frame=0, seed=0, circle_mask=case.mask)
    out = plan.remap(frame, interpolation="bilinear")
    Hd, Wd = case.dst[1], case.dst[2]
    limit = 1  # (double sources too: measured on every pixel of c5 at 180 and 195 degrees - experiments/r6/quality_census.py - no pixel beyond 1)

    def diff(got, want):
        d = np.abs(got.astype(np.int16) - want.astype(np.int16))
        if case.src[0] == "double":
            d = np.minimum(d, 256 - d)  # the blend's cast wraps mod 256 like the reference's
        return d.max(axis=-1)

    pos = np.random.default_rng(pin["sample_seed"]).integers(0, Hd * Wd, size=65536)
    got = out.reshape(-1, 3)[torch.from_numpy(pos).cuda()].cpu().numpy()
    want = gold[f"{case.name}/samples"]
    d = diff(got, want)
    flips = ((got == 0).all(axis=1) != (want == 0).all(axis=1))  # black <-> sampled: a validity / image boundary within float32 reach
    off = int(((d > limit) & ~flips).sum())
    assert off == 0, f"{off} of 65536 sampled pixels beyond {limit} LSB (max {int(d[~flips].max())})"
    assert int(flips.sum()) == 0, f"{int(flips.sum())} sampled pixels flipped between black and sampled"
    assert int((d > 0).sum()) <= 65536 // 20, f"{int((d > 0).sum())} of 65536 samples differ at all"
    for tag, (r0, c0) in pin["bilinear"]["crops"].items():
        wantc = gold[f"{case.name}/crop_{tag}"]
        gotc = out[r0:r0 + 128, c0:c0 + 128].cpu().numpy()
        dc = diff(gotc, wantc)
        rim = _rim_of((wantc == 0).all(axis=2))
        assert int((dc[~rim] > limit).sum()) == 0, f"crop {tag}: {int((dc[~rim] > limit).sum())} pixels off the black rims beyond {limit} LSB (max {int(dc[~rim].max())})"
        assert int((dc[rim] > limit).sum()) == 0, f"crop {tag}: {int((dc[rim] > limit).sum())} of {int(rim.sum())} rim pixels differ"
    black = int((out == 0).all(dim=2).sum())
    assert abs(black - pin["bilinear"]["black_pixels"]) <= 64, (black, pin["bilinear"]["black_pixels"])
    total = int(out.to(torch.int64).sum())
    assert abs(total - pin["bilinear"]["byte_sum"]) <= 3 * Hd * Wd // 200, (total, pin["bilinear"]["byte_sum"])  # (mean error per byte below 1/200 LSB)
    assert info["bilinear_float64_tiles"] * 100 <= info["tiles"], f"{info['bilinear_float64_tiles']} of {info['tiles']} tiles still take the float64 pass"


@pytest.mark.parametrize("fov", [180, 195])
def test_bilinear_double_tiles_against_float64_at_full_size(fov):
    """c5's geometry (7776x3888 double fisheye -> 8192x4096): the tile-model kernel (round 3) against the per-pixel float64
    kernel of the same mode, on the masked synthetic frame: at most 1 LSB apart except on a sliver of rim / seam pixels."""
    from tests.cases import dbl

    case = Case("c5", pano(4096, 8192), dbl(3888, 7776, "equidistant", fov), mask=2)
    plan = H.pb_plan_private(case)  # (a plan of its own - the facade's shared cache entry must never be left in another mode)
    assert plan.info()["fast_path"]
    frame = nat.synth_frame(3888, 7776, frame=1, circle_mask=2)
    got = plan.remap(frame, interpolation="bilinear").to(torch.int16)
    plan.set_mode(nat.MODE_FAITHFUL)
    want = plan.remap(frame, interpolation="bilinear").to(torch.int16)
    d = (got - want).abs()
    d = torch.minimum(d, 256 - d).amax(dim=2)
    # beyond 2 LSB only where the float64 kernel's output has a black / sampled edge (one pixel either side): a coordinate within
    # float32 reach of an eye's rim or of the seam may flip a pixel between black and sampled
    black = (want == 0).all(dim=2)
    rim = torch.zeros_like(black)
    for dy, dx in ((0, 1), (1, 0), (0, -1), (-1, 0), (1, 1), (1, -1), (-1, 1), (-1, -1)):
        rim |= black != torch.roll(black, (dy, dx), (0, 1))
    # round 5: no pixel beyond 1 LSB, the rims included (rounds 3-4 allowed 2 LSB and more on the rims: no longer in use)
    assert int((d > 1).sum()) == 0, f"{int((d > 1).sum())} of {d.numel()} pixels differ by more than 1 LSB (max {int(d.max())}; {int(((d > 1) & rim).sum())} on a black rim)"
    assert int((d > 0).sum()) <= d.numel() // 100, int((d > 0).sum())


def _noise_cases():
    from tests.test_hip_random import random_case

    out = []
    for k in range(16):
        c = random_case(np.random.default_rng(20000 + 7 * k), k)
        up = lambda p: (p[0], p[1] * 3, p[2] * 3, p[3], p[4], None if p[5] is None else p[5] * 3)
        out.append(Case(f"noise{k}", up(c.dst), up(c.src), c.rotations, c.mask))
    return out


@pytest.mark.parametrize("case", _noise_cases(), ids=lambda c: f"{c.name}:{c.dst[0]}{c.dst[1]}x{c.dst[2]}<-{c.src[0]}{c.src[1]}x{c.src[2]}:r{len(c.rotations)}")
def test_bilinear_tiles_on_noise_frames(case):
    """The steepest content there is - independent random texels - shows every coordinate error as a value error (255 LSB per
    pixel of offset), on sixteen random geometries of 70-1000 px (small images: 32-px tiles span tens of degrees).  Round 3:
    certification measures each tile model against the faithful pre-truncation coordinate and the bilinear kernels leave tiles beyond
    1/1024 px (PB_TILE_COARSE) to exact coordinates.  Round 5: against the per-pixel DEFINITION kernel (pb_sample_map_bilinear_u8, equal
    to oracle.remap_bilinear to the bit) - single sources: no pixel beyond 1 LSB; double-fisheye sources: where BOTH eyes are sampled (the merge band,
    and the corners of the eyes' squares beyond it, where the factors are both 1.0) the definition adds two samples it has rounded to
    integers, each of ours may be the neighbouring integer, and the sum can land 2 LSB off - at the square of the one-eye rate (these
    sixteen geometries: at most 1 pixel in 50 000; experiments/r6/two_lsb_probe.py), never more.  The float64-mode
    kernel of the same plan (MODE_FAITHFUL) stays within 1 LSB of the definition everywhere."""
    plan = H.pb_plan_private(case)
    info = plan.info()
    assert info["bilinear_float64_tiles"] == 0  # (round 4: every tile the models cannot serve has its exact coordinates in the plan)
    frame = nat.synth_frame(case.src[1], case.src[2], frame=5)
    src, cmap = H.pb_chain(case, frame)
    want = nat.sample_map_bilinear(src._proj("src"), cmap.device_tensor(), frame, 3, np.uint8).reshape(case.dst[1], case.dst[2], 3).to(torch.int16)
    got = plan.remap(frame, interpolation="bilinear").to(torch.int16)
    plan.set_mode(nat.MODE_FAITHFUL)
    f64 = plan.remap(frame, interpolation="bilinear").to(torch.int16)

    def dist(a, b):
        d = (a - b).abs()
        return torch.minimum(d, 256 - d).amax(dim=2)

    d = dist(got, want)
    double = case.src[0] == "double"
    assert int((d > (2 if double else 1)).sum()) == 0, f"{int((d > 1).sum())} of {d.numel()} pixels beyond 1 LSB, max {int(d.max())}"
    assert int((d > 1).sum()) <= max(8, d.numel() // 50000), f"{int((d > 1).sum())} of {d.numel()} pixels beyond 1 LSB"
    assert int((dist(f64, want) > 1).sum()) == 0


@pytest.mark.parametrize("fov, tiles_expected", [(180.05, False), (180.6, False), (179.8, False), (181.0, True), (180.0, True), (195.0, True), (170.0, True)])
def test_a_stitch_with_a_merge_band_under_one_degree_runs_the_float64_kernels(fov, tiles_expected):
    """The reference keeps blending for half a degree past the merge band's end with the band's own slope (projection.py:416-418, :440-444):
    the factor there reaches -0.5 / (fov - 180), which multiplies whatever an eye's sample is off by (a 180.01-degree stitch: x 45; found
    by the round's fuzz: 42 LSB).  With a band of a degree or more the factor stays within [-0.5, 1] and two +-1 samples stay within 2 LSB;
    under a degree the plan builds no bilinear tile tables and the mode runs its per-pixel float64 kernels - within 1 LSB of the
    definition like everywhere.  (Exactly 180: the factor is infinite, the cast gives 0 whatever the sample.)"""
    case = Case(f"narrow_{fov}", pano(300, 600), dbl(440, 880, "equidistant", fov), [(20, -35, 10)])
    plan = H.pb_plan_private(case)
    info = plan.info()
    assert (info["bilinear_float64_tiles"] == 0) == tiles_expected and (tiles_expected or info["bilinear_float64_tiles"] == info["tiles"])
    assert (plan.bilinear_launch_shape()["workgroups"] > 0) == tiles_expected
    frame = nat.synth_frame(case.src[1], case.src[2], frame=3)
    src, cmap = H.pb_chain(case, frame)
    want = nat.sample_map_bilinear(src._proj("src"), cmap.device_tensor(), frame, 3, np.uint8).reshape(case.dst[1], case.dst[2], 3).to(torch.int16)
    got = plan.remap(frame, interpolation="bilinear").to(torch.int16)
    d = (got - want).abs()
    d = torch.minimum(d, 256 - d).amax(dim=2)
    assert int((d > (2 if tiles_expected else 1)).sum()) == 0, f"{int((d > 1).sum())} pixels beyond 1 LSB, max {int(d.max())}"
    plan.set_mode(nat.MODE_FAITHFUL)  # (the reference's sampler is untouched by any of this: tile kernels == float64 kernel)
    near64 = plan.remap(frame)
    plan.set_mode(nat.MODE_AUTO)
    assert torch.equal(plan.remap(frame), near64)


_TINY = TINY_BILINEAR  # (shared with tests/test_hip_catmull_rom_tiles.py, which adds sources and destinations for a 4 x 4 footprint)


@pytest.mark.parametrize("case", _TINY, ids=lambda c: c.name)
def test_bilinear_on_sources_and_destinations_of_a_few_pixels(case):
    """Frames of 1-12 pixels: every tap clamps or wraps, 8-byte loads end at the buffer's end, a tile holds more pixels than the source
    (half windows, unguarded table tiles and the LDS pool must all decline gracefully).  Against oracle.remap_bilinear: 1 LSB."""
    rng = np.random.default_rng(3)
    frame = rng.integers(0, 256, size=(case.src[1], case.src[2], 3), dtype=np.uint8)
    want = orc.remap_bilinear(H.orc_proj(case.dst), H.orc_proj(case.src), frame, H.orc_rots(case))
    plan = H.pb_plan_private(case)
    got = plan.remap(torch.from_numpy(frame).cuda(), interpolation="bilinear").cpu().numpy()
    d = np.abs(got.astype(np.int16) - want.astype(np.int16))
    if case.src[0] == "double":
        d = np.minimum(d, 256 - d)
    assert int(d.max()) <= 1, f"max difference {int(d.max())}"
