"""The polynomial (Kannala-Brandt) lens on the device: every route a built-in lens takes, against the REFERENCE's outputs for
the same lens handed over as two callables (tests/golden/polynomial.npz) and against the oracle with that pair at sizes the tile
kernels run at.  Nothing in the chain is approximate - the lens is + - * / in float64, everything else is already pinned to the bit -
so the nearest paths are compared without a tolerance; the interpolating tile kernels keep their modes' own 1-LSB bound."""

import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from click.testing import CliRunner
from PIL import Image

import photonbend_amd as pb
import photonbend_amd.batch  # noqa: F401  (pb.batch)
from oracle import reference_path as orc
from oracle.synth import synth_frame, synth_image
from photonbend_amd import _hostpipe
from photonbend_amd import _native as nat
from photonbend_amd.core import projection as proj_mod
from photonbend_amd.core.lens import lens_id
from photonbend_amd.core.projection import _plan_for
from photonbend_amd.scripts import cli
from tests import catmull_rom_ref as cr
from tests import helpers as H
from tests import polynomial_cases as pc
from tests import ss_ref
from tests.cases import Case, cam, inscribed, pano
from tests.test_hip_bilinear import smooth_frame
from tests.test_hip_catmull_rom import _within_one

pytestmark = pytest.mark.gpu
GOLD = np.load(os.path.join(H.GOLD, "polynomial.npz"))
SMALL = pc.small_cases()
MID = pc.mid_cases()
rad = pb.utils.to_radians


def _private_plan(case, **kw):
    src, cmap = pc.pb_chain(case, image=np.zeros((case.src[1], case.src[2], 3), np.uint8))
    return nat.Plan(cmap.dst_proj, cmap.rotations, src._proj("src"), **kw)


def _same_bits(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and bool(((H.bits(a) == H.bits(b)) | (np.isnan(a) & np.isnan(b))).all())


def _n_diff(a, b):
    return int((a != b).reshape(a.shape[0], a.shape[1], -1).any(axis=2).sum())


def _check_index(plan, case, gold_or_oracle):
    idx = plan.index_map(weights=True) if case.src[0] == "double" else plan.index_map()
    if case.src[0] == "double":
        i2, w2 = idx
        il, ir, wl, wr = gold_or_oracle
        i2, w2 = i2.cpu().numpy(), w2.cpu().numpy()
        assert np.array_equal(i2[0], il) and np.array_equal(i2[1], ir), case.name
        assert _same_bits(w2[0], wl) and _same_bits(w2[1], wr), case.name
    else:
        assert np.array_equal(idx.cpu().numpy(), gold_or_oracle), case.name


def _gold_index(case):
    n = case.name
    if case.src[0] == "double":
        return GOLD[f"{n}/idx_l"], GOLD[f"{n}/idx_r"], GOLD[f"{n}/w_l"].view(np.float64), GOLD[f"{n}/w_r"].view(np.float64)
    return GOLD[f"{n}/idx"]


# ---- the reference's bytes, index maps and float64 maps on every path ----------------------------------------------------------------
@pytest.mark.parametrize("case", SMALL, ids=lambda c: c.name)
def test_small_cases_equal_the_reference_on_every_path(case):
    n, want = case.name, GOLD[f"{case.name}/u8"]
    frame = pc.case_frame(case)
    dev = torch.from_numpy(frame).cuda()
    # the materialised float64 maps, stage by stage, to the bit
    cmap = pc.pb_obj(case.dst).get_coordinate_map()
    assert cmap.is_lazy
    stages = [np.array(np.asarray(cmap))]
    for rot in case.rotations:
        cmap = pb.Rotation(*map(rad, rot)).rotate_coordinate_map(cmap)
        stages.append(np.array(np.asarray(cmap)))
    for k, st in enumerate(stages):
        assert _same_bits(st, GOLD[f"{n}/map{k}"].view(np.float64)), f"{n}: float64 map stage {k} differs from the reference's"
    # a prepared plan: the tile kernels + exact tables
    plan = _private_plan(case)
    assert _n_diff(plan.remap(dev).cpu().numpy(), want) == 0, n
    _check_index(plan, case, _gold_index(case))
    # PB_MODE_FAITHFUL on the same plan: the float64 kernel
    plan.set_mode(nat.MODE_FAITHFUL)
    assert _n_diff(plan.remap(dev).cpu().numpy(), want) == 0, n
    _check_index(plan, case, _gold_index(case))
    # a deferred plan: no preparation, the float64 kernel
    deferred = _private_plan(case, defer=True)
    assert _n_diff(deferred.remap(dev).cpu().numpy(), want) == 0, n
    _check_index(deferred, case, _gold_index(case))
    # the facade, ndarray in -> ndarray out, twice (the first use of a geometry runs a deferred plan, the second prepares it)
    for _ in range(2):
        src, lazy = pc.pb_chain(case, image=frame)
        got = src.process_coordinate_map(lazy)
        assert isinstance(got, np.ndarray) and _n_diff(got, want) == 0, n
    # ... and through a materialised map (the map-stage kernels)
    src, lazy = pc.pb_chain(case, image=frame)
    assert _n_diff(src.process_coordinate_map(np.array(np.asarray(lazy))), want) == 0, n


@pytest.mark.parametrize("case", SMALL, ids=lambda c: c.name)
def test_untagged_callables_on_the_host_path_give_the_same_bytes(case):
    """The same lens as plain user callables runs through the host path (PB_LENS_CUSTOM): the old path is the new path's second oracle."""
    frame = pc.case_frame(case)
    src, cmap = pc.pb_chain(case, image=frame, make_lens=pc.untagged)
    if case.dst[0] != "pano" and case.dst[3] in pc.LENSES:
        first = pc.pb_obj(case.dst, make_lens=pc.untagged).get_coordinate_map()
        assert not first.is_lazy and first.dst_proj.lens == nat.LENS_CUSTOM
    if case.src[0] != "pano" and case.src[3] in pc.LENSES:
        assert src._proj("src").lens == nat.LENS_CUSTOM
    assert _n_diff(src.process_coordinate_map(cmap), GOLD[f"{case.name}/u8"]) == 0, case.name


def test_a_polynomial_lens_takes_the_lazy_map_and_the_fused_host_pipe(monkeypatch):
    case = pc.case_by_name("P_src_eqs9_rot")
    frame = pc.case_frame(case)
    calls = {"planes": 0, "pipe": 0}
    real_planes, real_pipe = proj_mod._GpuProjection._distance_planes, _hostpipe.remap_ndarray

    def planes(self, src, dev_map):
        calls["planes"] += 1
        return real_planes(self, src, dev_map)

    def pipe(plan, a, *args, **kw):
        calls["pipe"] += 1
        return real_pipe(plan, a, *args, **kw)

    monkeypatch.setattr(proj_mod._GpuProjection, "_distance_planes", planes)
    monkeypatch.setattr(_hostpipe, "remap_ndarray", pipe)
    src, cmap = pc.pb_chain(case, image=frame)
    assert cmap.is_lazy and pc.pb_obj(pc.case_by_name("P_dst_cal").dst).get_coordinate_map().is_lazy
    assert src._proj("src").lens >= nat.LENS_POLYNOMIAL_BASE
    got = src.process_coordinate_map(cmap)
    assert calls == {"planes": 0, "pipe": 1} and _n_diff(got, GOLD[f"{case.name}/u8"]) == 0
    for interp in ("bilinear", "catmull-rom"):
        src.process_coordinate_map(cmap, interpolation=interp)
    src2, cmap2 = pc.pb_chain(case, image=frame)
    src2.process_coordinate_map(pc.pb_obj(case.dst).get_coordinate_map(supersample=2))
    assert calls == {"planes": 0, "pipe": 4}
    # the user-callable form of the same lens still goes the old way
    src3, cmap3 = pc.pb_chain(case, image=frame, make_lens=pc.untagged)
    src3.process_coordinate_map(cmap3)
    assert calls["planes"] >= 1 and calls["pipe"] == 4


# ---- mid size: the tile kernels, the thresholds, the routes ---------------------------------------------------------------------------
def _builtin_twin(case):
    """the same geometry with the built-in equisolid lens in place of the polynomial one (for the printed tile counts)"""
    swap = lambda p: p if p[0] == "pano" or p[3] not in pc.LENSES else (p[0], p[1], p[2], "equisolid", p[4], p[5])  # noqa: E731
    return Case(case.name + "_equisolid", swap(case.dst), swap(case.src), case.rotations, mask=case.mask)


@pytest.mark.parametrize("case", MID, ids=lambda c: c.name)
def test_mid_cases_prepared_plan_float64_kernel_and_oracle_agree(case):
    frame = pc.case_frame(case)
    dev = torch.from_numpy(frame).cuda()
    od, os_, rots = pc.orc_proj(case.dst), pc.orc_proj(case.src), pc.orc_rots(case)
    with np.errstate(all="ignore"):
        want = orc.remap(od, os_, frame, rots)
        oidx = orc.remap_index(od, os_, rots)
    plan = _private_plan(case)
    info = plan.info()
    twin = _private_plan(_builtin_twin(case)).info()
    keys = ("tiles", "fix_tiles", "fix_pixels", "model_diff_pixels", "lean_tiles", "black_tiles", "direct_tiles")
    print(f"{case.name}: polynomial {({k: info[k] for k in keys})}")
    print(f"{case.name}: equisolid  {({k: twin[k] for k in keys})}")
    fast = plan.remap(dev).cpu().numpy()
    assert _n_diff(fast, want) == 0, f"{case.name}: {_n_diff(fast, want)} pixels of the prepared plan differ from the oracle"
    if case.src[0] == "double":
        # (a double-fisheye source has no `fast_path` / WIN route to assert: pb_plan_info reports the single-source fast path only, and a
        # rotated stitch runs pb_hot_double_kernel or the float64 kernel, whichever the plan's tables allow - the bytes and both eyes'
        # index maps and weights are what is held)
        _check_index(plan, case, oidx[:4])
    else:
        # the certified fast path, through the windowed tile kernel: a supersampled call needs no workspace exactly when the plain
        # call's route is WIN (pb_remap_ss_workspace asks pb_route)
        assert info["fast_path"] and info["tiles"] > 0 and plan.supersample_workspace_bytes(2) == 0, info
        _check_index(plan, case, oidx)
    plan.set_mode(nat.MODE_FAITHFUL)
    assert _n_diff(plan.remap(dev).cpu().numpy(), want) == 0, case.name
    plan.set_mode(nat.MODE_AUTO)
    if case.dst[0] != "pano" and case.src[0] == "pano":
        # the destination-validity thresholds (found by bisection, not covered by certification) against the per-pixel predicate on EVERY
        # pixel: a panorama source samples every valid direction, so the plan's black set is the invalid set
        with np.errstate(all="ignore"):
            m = orc.coordinate_map(od)
        invalid = m[:, :, 2] != 0.0
        black = plan.index_map().cpu().numpy() < 0
        assert np.array_equal(black, invalid), f"{case.name}: {int((black != invalid).sum())} pixels where the thresholds disagree with the predicate"
        assert invalid.any() and not invalid.all()
        lo, hi = info["thresholds"][:2]
        print(f"{case.name}: invalid <=> {lo} <= n4 < {hi}; {int(invalid.sum())} invalid pixels")


@pytest.mark.parametrize("name", ["PM_photo_cal", "PM_pano_eqs9"])
def test_interpolating_tile_kernels_keep_their_modes_bound(name):
    case = pc.case_by_name(name)
    od, os_, rots = pc.orc_proj(case.dst), pc.orc_proj(case.src), pc.orc_rots(case)
    plan = _private_plan(case, bilinear=True)
    assert plan.info()["fast_path"]
    # bilinear: a smooth frame (on noise every pixel sits on an interpolation edge), NO pixel beyond 1 LSB - the rims of the black regions
    # included: a polynomial source that looks past max_theta has a black / sampled boundary INSIDE its frame, where the tile model
    # continues the polynomial and the truth is black - and no pixel black in one result and sampled in the other except, at most two
    # of them, on such a rim (the bound the Catmull-Rom tile kernel is held to)
    frame = smooth_frame(case.src[1], case.src[2])
    with np.errstate(all="ignore"):
        want = orc.remap_bilinear(od, os_, frame, rots)
    got = plan.remap(torch.from_numpy(frame).cuda(), interpolation="bilinear").cpu().numpy()
    d = np.abs(got.astype(np.int16) - want.astype(np.int16)).max(axis=2)
    flips = (got == 0).all(axis=2) != (want == 0).all(axis=2)
    print(f"{name}: bilinear max difference {int(d.max())} LSB, {int((d > 1).sum())} pixels beyond 1 LSB, {int(flips.sum())} black <-> sampled flips, "
          f"{100 * float((d > 0).mean()):.3f} % of the pixels 1 LSB off")
    _within_one(got, want, False, name + " bilinear", rim_flips=2)
    # catmull-rom: tests/test_hip_catmull_rom.py's check
    frame = pc.case_frame(case)
    with np.errstate(all="ignore"):
        want = cr.remap(od, os_, frame, rots)
    got = plan.remap(torch.from_numpy(frame).cuda(), interpolation="catmull-rom").cpu().numpy()
    share = _within_one(got, want, False, name, rim_flips=2)
    print(f"{name}: catmull-rom {100 * share:.3f} % of the pixels 1 LSB off")


@pytest.mark.parametrize("case", SMALL, ids=lambda c: c.name)
def test_interpolating_map_kernels_are_their_definitions_to_the_bit(case):
    frame = pc.case_frame(case)
    od, os_, rots = pc.orc_proj(case.dst), pc.orc_proj(case.src), pc.orc_rots(case)
    for interp, ref in (("bilinear", orc.remap_bilinear), ("catmull-rom", cr.remap)):
        with np.errstate(all="ignore"):
            want = ref(od, os_, frame, rots)
        src, lazy = pc.pb_chain(case, image=frame)
        got = src.process_coordinate_map(np.array(np.asarray(lazy)), interpolation=interp)
        assert got.shape == want.shape and int((got != want).sum()) == 0, f"{case.name} {interp}: {int((got != want).sum())} samples differ"
        # the plan's float64 route of the mode
        plan = _private_plan(case, bilinear=True)
        plan.set_mode(nat.MODE_FAITHFUL)
        got = plan.remap(torch.from_numpy(frame).cuda(), interpolation=interp).cpu().numpy()
        if interp == "catmull-rom":  # (bilinear's per-pixel plan route keeps float32 taps: the mode's 1 LSB; catmull-rom's is its definition)
            assert int((got != want).sum()) == 0, f"{case.name} {interp} float64 route"
        else:
            d = np.abs(got.astype(np.int16) - want.astype(np.int16))
            if case.src[0] == "double":
                d = np.minimum(d, 256 - d)
            assert int(d.max(initial=0)) <= (2 if case.src[0] == "double" else 1), f"{case.name} bilinear float64 route"


@pytest.mark.parametrize("n", [2, 4])
@pytest.mark.parametrize("name", ["PM_photo_cal", "PM_pano_eqs9", "P_dst_eqs9_rot", "P_both_rot"])
def test_supersampled_nearest_takes_the_fused_kernel(name, n):
    case = pc.case_by_name(name)
    frame = pc.case_frame(case)
    od, os_, rots = pc.orc_proj(case.dst), pc.orc_proj(case.src), pc.orc_rots(case)
    kind, h, w, lens, fov, mag = case.dst
    od_n = orc.Proj("pano", n * h, n * w) if kind == "pano" else orc.Proj(kind, n * h, n * w, od.lens, od.fov, od.magnitude * n)
    with np.errstate(all="ignore"):
        want = ss_ref.block_mean(orc.remap(od_n, os_, frame, rots), n)
    cm = pc.pb_obj(case.dst).get_coordinate_map(supersample=n)
    for rot in case.rotations:
        cm = pb.Rotation(*map(rad, rot)).rotate_coordinate_map(cm)
    src = pc.pb_obj(case.src, frame)
    plan = nat.Plan(cm.dst_proj, cm.rotations, src._proj("src"))
    need = ctypes.c_size_t(1)
    nat.check(nat.load().pb_remap_ss_workspace(plan.handle, n, 0, 0, ctypes.byref(need)))
    if name.startswith("PM_"):  # (a plan of a few tiles has no launch table: its plain route is DIRECT, its supersampled one generic)
        assert need.value == 0, "a prepared single-source polynomial plan must take SS_FUSED"
    got = plan.remap(torch.from_numpy(frame).cuda(), supersample=n).cpu().numpy()
    assert got.shape == want.shape and _n_diff(got, want) == 0, f"{name} n={n}: {_n_diff(got, want)} pixels differ"
    assert _n_diff(plan.remap(torch.from_numpy(frame).cuda(), supersample=n, generic=True).cpu().numpy(), want) == 0
    assert _n_diff(src.process_coordinate_map(cm), want) == 0  # the facade


# ---- the lens id resolves to the right lens ----------------------------------------------------------------------------------------
def test_zero_equals_equidistant_and_eqs9_is_close_to_equisolid():
    frame = synth_image(32, 64, "RGB", frame=3)
    rot = [(10, 20, 30)]

    def run(lens, fov=190, mag=19.5):
        case = Case("x", cam(40, 40, lens, fov, mag), pano(32, 64), rot)
        src, cmap = pc.pb_chain(case, image=frame)
        plan = nat.Plan(cmap.dst_proj, cmap.rotations, src._proj("src"))
        out = plan.remap(torch.from_numpy(frame).cuda()).cpu().numpy()
        assert np.array_equal(out, src.process_coordinate_map(cmap))
        return out

    assert np.array_equal(run("ZERO"), run("equidistant"))
    a, b = run("EQS9"), run("equisolid")
    differ = int((a != b).any(axis=2).sum())
    nonblack = lambda x: int(x.any(axis=2).sum())  # noqa: E731
    print(f"EQS9 against the built-in equisolid lens: {differ} of {a.shape[0] * a.shape[1]} pixels differ")
    assert nonblack(a) > a.shape[0] * a.shape[1] // 2 and nonblack(b) > a.shape[0] * a.shape[1] // 2
    assert differ < a.shape[0] * a.shape[1] - differ
    # ... and as a source
    f2 = synth_frame(48, 48, frame=0, seed=0, circle_mask=1)
    outs = {}
    for lens in ("ZERO", "equidistant"):
        src, cmap = pc.pb_chain(Case("y", pano(32, 64), cam(48, 48, lens, 200, inscribed(48)), rot, mask=1), image=f2)
        outs[lens] = src.process_coordinate_map(cmap)
    assert np.array_equal(outs["ZERO"], outs["equidistant"]) and outs["ZERO"].any()


def test_coefficients_are_part_of_the_request():
    frame = synth_frame(64, 128, frame=0, seed=0)
    k, deg = pc.LENSES["CAL"]
    mt = orc.to_radians(deg)

    def chain(k1):
        L = pb.polynomial(k1, *k[1:], max_theta=mt)
        dst = pb.CameraImage(np.zeros((96, 96, 3), np.uint8), rad(200), L, magnitude=47.5)
        return L, dst.get_coordinate_map()

    La, ma = chain(k[0])
    Lb, mb = chain(k[0] - 0.02)
    Lc, mc = chain(k[0])  # the same set, registered a second time
    assert lens_id(La) == lens_id(Lc) != lens_id(Lb)
    src = pb.PanoramaImage(frame)._proj("src")
    pa, pb_, pc_ = (_plan_for(m.dst_proj, m.rotations, src) for m in (ma, mb, mc))
    assert pa is pc_ and pa is not pb_
    dev = torch.from_numpy(frame).cuda()
    oa, ob = pa.remap(dev).cpu().numpy(), pb_.remap(dev).cpu().numpy()
    assert _n_diff(oa, ob) > 0
    for L, out in ((La, oa), (Lb, ob)):
        want = orc.remap(orc.Proj("camera", 96, 96, (L.forward_function, L.reverse_function), rad(200), 47.5), orc.Proj("pano", 64, 128), frame)
        assert _n_diff(out, want) == 0
    lib = nat.load()
    assert lib.pb_plan_matches(pa.handle, ctypes.byref(ma.dst_proj), None, 0, ctypes.byref(src)) == 1
    other = nat.pb_proj.from_buffer_copy(mb.dst_proj)
    other.f_distance, other.magnitude = ma.dst_proj.f_distance, ma.dst_proj.magnitude  # now ONLY the coefficients differ
    assert lib.pb_plan_matches(pa.handle, ctypes.byref(other), None, 0, ctypes.byref(src)) == 0


# ---- batches, blobs, broadcast ----------------------------------------------------------------------------------------------------
_CHILD = r"""
import sys
import numpy as np, torch
import photonbend_amd as pb
from photonbend_amd import _native as nat
from tests import polynomial_cases as pc

blob = open(sys.argv[1], "rb").read()
case = pc.case_by_name(sys.argv[2])
kk, mt = (nat.C.c_double * 4)(), nat.C.c_double()
assert nat.load().pb_lens_polynomial_info(16, kk, nat.C.byref(mt)) == -1, "the child's registry must start empty"
# some other lens first: the child's ids are not the parent's
pb.core.lens.lens_id(pb.polynomial(0.01, max_theta=1.0))
frame = pc.case_frame(case)
src, cmap = pc.pb_chain(case, image=frame)
plan = nat.Plan.deserialize(blob, cmap.dst_proj, cmap.rotations, src._proj("src"))
assert plan.info()["fast_path"] == (case.src[0] != "double")
out = plan.remap(torch.from_numpy(frame).cuda()).cpu().numpy()
np.save(sys.argv[3], out)
# the blob of one lens is not the plan of another
k, deg = pc.LENSES["CAL"]
mine = src._proj("src")
other = nat.make_proj(mine.kind, mine.height, mine.width, nat.lens_polynomial(k, pb.utils.to_radians(deg)), mine.fov, mine.magnitude, mine.f_distance)
try:
    nat.Plan.deserialize(blob, cmap.dst_proj, cmap.rotations, other)
except nat.PbError as exc:
    assert "another geometry" in str(exc)
else:
    raise SystemExit("a blob matched another lens's request")
print("child ok")
"""


def test_remap_frames_and_a_blob_in_a_fresh_process(tmp_path):
    case = pc.case_by_name("PM_pano_eqs9")
    od, os_, rots = pc.orc_proj(case.dst), pc.orc_proj(case.src), pc.orc_rots(case)
    frames = [pc.case_frame(case, frame=f) for f in range(3)]
    src, cmap = pc.pb_chain(case, image=frames[0])
    plan = pb.batch.plan_for(pc.pb_obj(case.dst), [pb.Rotation(*map(rad, r)) for r in case.rotations], src)
    outs = list(pb.batch.remap_frames(plan, frames))
    with np.errstate(all="ignore"):
        wants = [orc.remap(od, os_, f, rots) for f in frames]
    assert len(outs) == 3 and all(_n_diff(o, w) == 0 for o, w in zip(outs, wants))
    # separately allocated device frames in one launch
    each = plan.remap_each([torch.from_numpy(f).cuda() for f in frames])
    assert all(_n_diff(o.cpu().numpy(), w) == 0 for o, w in zip(each, wants))
    # serialize here, deserialize in a child whose registry is empty: ids are process-local, a blob must carry the coefficients
    fresh = nat.Plan(cmap.dst_proj, cmap.rotations, src._proj("src"))
    blob = fresh.serialize()
    back = nat.Plan.deserialize(blob, cmap.dst_proj, cmap.rotations, src._proj("src"))
    assert _n_diff(back.remap(torch.from_numpy(frames[0]).cuda()).cpu().numpy(), wants[0]) == 0
    blob_path, out_path, script = tmp_path / "plan.pbplan", tmp_path / "out.npy", tmp_path / "child.py"
    blob_path.write_bytes(blob)
    script.write_text(_CHILD)
    root = os.path.dirname(os.path.dirname(H.GOLD))
    env = dict(os.environ, PYTHONPATH=root + os.pathsep + os.environ.get("PYTHONPATH", ""))
    res = subprocess.run([sys.executable, str(script), str(blob_path), case.name, str(out_path)], capture_output=True, text=True, cwd=root, env=env, timeout=600)
    assert res.returncode == 0 and "child ok" in res.stdout, res.stdout + res.stderr
    assert _n_diff(np.load(out_path), wants[0]) == 0


def _bcast_worker(q):
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    torch.cuda.set_device(0)
    lib = nat.load()
    uid = ctypes.create_string_buffer(128)
    nat.check(lib.pb_comm_unique_id(uid))
    comm = ctypes.c_void_p()
    nat.check(lib.pb_comm_init(1, 0, uid, ctypes.byref(comm)))
    case = pc.case_by_name("P_both_rot")
    src, cmap = pc.pb_chain(case, image=np.zeros((case.src[1], case.src[2], 3), np.uint8))
    d, s = cmap.dst_proj, src._proj("src")
    d2, s2 = nat.pb_proj.from_buffer_copy(d), nat.pb_proj.from_buffer_copy(s)
    rot = (ctypes.c_double * (9 * nat.PB_MAX_ROTATIONS))()
    mats = np.asarray(cmap.rotations, dtype=np.float64).ravel()
    for k, v in enumerate(mats):
        rot[k] = v
    n_rot = ctypes.c_int(len(cmap.rotations))
    nat.check(lib.pb_bcast_params(comm, ctypes.byref(d2), rot, ctypes.byref(n_rot), ctypes.byref(s2), 0, None))
    same = (d2.key() == d.key() and s2.key() == s.key() and nat.lens_polynomial_info(d2.lens) == nat.lens_polynomial_info(d.lens)
            and nat.lens_polynomial_info(s2.lens) == nat.lens_polynomial_info(s.lens) and n_rot.value == len(cmap.rotations))
    frame = pc.case_frame(case)
    plan = nat.Plan(d2, [np.frombuffer(rot, dtype=np.float64)[9 * k : 9 * k + 9].reshape(3, 3).copy() for k in range(n_rot.value)], s2)
    out = plan.remap(torch.from_numpy(frame).cuda()).cpu().numpy()
    # an id the root never registered does not travel (another rank's registry may hold a different lens under it): every rank gets
    # PB_ERR_INVALID, and the projections it passed are left alone
    bogus = nat.pb_proj.from_buffer_copy(d)
    bogus.lens = nat.LENS_POLYNOMIAL_BASE + 100000
    s3 = nat.pb_proj.from_buffer_copy(s)
    refused = lib.pb_bcast_params(comm, ctypes.byref(bogus), rot, ctypes.byref(n_rot), ctypes.byref(s3), 0, None) == -1 and b"never registered" in lib.pb_last_error()
    nat.check(lib.pb_comm_destroy(comm))
    q.put((same and refused and bogus.lens == nat.LENS_POLYNOMIAL_BASE + 100000, out))


def test_broadcast_carries_the_coefficients():
    import torch.multiprocessing as mp

    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_bcast_worker, args=(q,))
    p.start()
    same, out = q.get(timeout=300)
    p.join(timeout=120)
    assert p.exitcode == 0 and same
    assert _n_diff(out, GOLD["P_both_rot/u8"]) == 0


# ---- the CLI and a C host ------------------------------------------------------------------------------------------------------------
def test_cli_equals_api(tmp_path):
    k, deg = pc.LENSES["CAL"]
    img = synth_image(72, 72, "RGB", frame=5, circle_mask=1)
    inp, out = tmp_path / "in.png", tmp_path / "out.png"
    Image.fromarray(img).save(inp)
    args = ["make-pano", str(inp), "--type", "inscribed", "--lens", "polynomial", "--lens-coefficients", *[repr(v) for v in k], "--lens-max-theta", repr(deg),
            "--fov", "200", "-s", "48", "-r", "15", "-40", "5", str(out)]
    res = CliRunner().invoke(cli.main, args)
    assert res.exit_code == 0, (res.output, res.exception)
    got = np.asarray(Image.open(out))
    L = pb.polynomial(*k, max_theta=rad(deg))
    src = pb.CameraImage(img, rad(200), L, magnitude=72 / 2 - 0.5)
    cmap = pb.Rotation(rad(15), rad(-40), rad(5)).rotate_coordinate_map(pb.PanoramaImage(np.zeros((48, 96, 3), np.uint8)).get_coordinate_map())
    want = src.process_coordinate_map(cmap)
    assert np.array_equal(got, want) and got.any()
    with np.errstate(all="ignore"):
        ref = orc.remap(orc.Proj("pano", 48, 96), orc.Proj("camera", 72, 72, (L.forward_function, L.reverse_function), rad(200), 35.5), img, [(rad(15), rad(-40), rad(5))])
    assert np.array_equal(got, ref)
    # alter-photo: a polynomial lens on both ends
    out2 = tmp_path / "out2.png"
    k2, deg2 = pc.LENSES["EQS9"]
    res = CliRunner().invoke(cli.main, ["alter-photo", str(inp), "--itype", "inscribed", "--ilens", "polynomial", "--ilens-coefficients", *[repr(v) for v in k],
                                        "--ilens-max-theta", repr(deg), "--ifov", "200", "--otype", "inscribed", "--olens", "polynomial", "--olens-coefficients",
                                        *[repr(v) for v in k2], "--olens-max-theta", repr(deg2), "--ofov", "190", str(out2)])
    assert res.exit_code == 0, (res.output, res.exception)
    L2 = pb.polynomial(*k2, max_theta=rad(deg2))
    with np.errstate(all="ignore"):
        ref2 = orc.remap(orc.Proj("camera", 72, 72, (L2.forward_function, L2.reverse_function), rad(190), 35.5),
                         orc.Proj("camera", 72, 72, (L.forward_function, L.reverse_function), rad(200), 35.5), img)
    assert np.array_equal(np.asarray(Image.open(out2)), ref2)


def test_c_abi_with_a_registered_id():
    """What a C host does: register, fill a pb_proj with the id and its own f_distance, and call the existing entry points."""
    lib = nat.load()
    k, deg = pc.LENSES["CAL"]
    mt = orc.to_radians(deg)
    lens = ctypes.c_int()
    assert lib.pb_lens_polynomial((ctypes.c_double * 4)(*k), mt, ctypes.byref(lens)) == 0
    L = pb.polynomial(*k, max_theta=mt)
    fov, mag, h = rad(200), 63.5, 128
    dst = nat.make_proj(nat.KIND_CAMERA, h, h, lens.value, fov, mag, mag / L.forward_function(fov / 2))
    src = nat.make_proj(nat.KIND_PANO, 96, 192)
    od, os_ = orc.Proj("camera", h, h, (L.forward_function, L.reverse_function), fov, mag), orc.Proj("pano", 96, 192)
    # pb_coordmap_f64
    m = torch.empty((h, h, 3), dtype=torch.float64, device="cuda")
    assert lib.pb_coordmap_f64(ctypes.byref(dst), m.data_ptr(), None) == 0
    torch.cuda.synchronize()
    with np.errstate(all="ignore"):
        assert _same_bits(m.cpu().numpy(), orc.coordinate_map(od))
    # pb_plan_create + pb_remap_u8 + pb_index_map_i32
    plan = ctypes.c_void_p()
    assert lib.pb_plan_create(ctypes.byref(dst), None, 0, ctypes.byref(src), ctypes.byref(plan)) == 0
    frame = synth_frame(96, 192, frame=1, seed=0)
    s, o = torch.from_numpy(frame).cuda(), torch.zeros((h, h, 3), dtype=torch.uint8, device="cuda")
    idx = torch.empty((h, h), dtype=torch.int32, device="cuda")
    assert lib.pb_remap_u8(plan, s.data_ptr(), o.data_ptr(), 1, 0, 0, None) == 0
    assert lib.pb_index_map_i32(plan, idx.data_ptr(), None, None) == 0
    torch.cuda.synchronize()
    with np.errstate(all="ignore"):
        assert np.array_equal(o.cpu().numpy(), orc.remap(od, os_, frame)) and np.array_equal(idx.cpu().numpy(), orc.remap_index(od, os_))
    fast = ctypes.c_int()
    assert lib.pb_plan_info(plan, ctypes.byref(fast), None, None) == 0 and fast.value == 1
    lib.pb_plan_destroy(plan)
    # as a source of the map-stage calls
    cam_src = nat.make_proj(nat.KIND_CAMERA, h, h, lens.value, fov, mag, dst.f_distance)
    with np.errstate(all="ignore"):
        pm = orc.coordinate_map(orc.Proj("pano", 64, 128))
    dm = torch.from_numpy(pm.copy()).cuda()
    f2 = synth_frame(h, h, frame=2, seed=0, circle_mask=1)
    s2, o2 = torch.from_numpy(f2).cuda(), torch.zeros((64, 128, 3), dtype=torch.uint8, device="cuda")
    assert lib.pb_sample_map_u8(ctypes.byref(cam_src), dm.data_ptr(), 64, 128, s2.data_ptr(), o2.data_ptr(), None) == 0
    torch.cuda.synchronize()
    with np.errstate(all="ignore"):
        assert np.array_equal(o2.cpu().numpy(), orc.sample(od, f2, pm.copy()))
    # an id nobody registered is refused by every gate
    bogus = nat.make_proj(nat.KIND_CAMERA, h, h, 16 + 100000, fov, mag, dst.f_distance)
    assert lib.pb_coordmap_f64(ctypes.byref(bogus), m.data_ptr(), None) == -1
    assert lib.pb_plan_create(ctypes.byref(bogus), None, 0, ctypes.byref(src), ctypes.byref(plan)) == -1
