"""The equi-angular cube map without a GPU: its NumPy definition (tests/eac_ref.py) against the cube's, the properties the
definition was checked for, the host build of the two warp functions against NumPy's bits in both math flavours, the facade, the fixture."""

import itertools
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import photonbend_amd as pb
from photonbend_amd import _native as nat
from photonbend_amd.core import projection as pj
from tests import cubemap_cases as cc
from tests import cubemap_ref as cr
from tests import eac_cases as ec
from tests import eac_ref as er
from tests import helpers as H
from tests.cases import Case, pano

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (1, 2, 3, 24, 25, 28, 32)
rad = pb.utils.to_radians


def _same_bits(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and bool(((H.bits(a) == H.bits(b)) | (np.isnan(a) & np.isnan(b))).all())


# ---- 1. the definition differs from the cube's by the warp alone ------------------------------------------------------------------------
def test_with_the_identity_for_both_functions_the_definition_is_the_cube_s(monkeypatch):
    monkeypatch.setattr(er, "warp", lambda c, half: np.asarray(c))
    monkeypatch.setattr(er, "unwarp", lambda c, half: np.asarray(c))
    swap = {c.name: e for c, e in zip(cc.small_cases(), ec.small_cases())}
    seen = 0
    for case in cc.small_cases():
        twin = swap[case.name]
        assert [p[0] for p in (twin.dst, twin.src)] == [{"cube": "eac"}.get(p[0], p[0]) for p in (case.dst, case.src)]
        with np.errstate(all="ignore"):
            want, got = cc.ref_stages(case), ec.ref_stages(twin)
            assert len(want) == len(got) and all(_same_bits(a, b) for a, b in zip(want, got)), case.name
            final = want[-1]
            wi, gi = cc.ref_index(case, final), ec.ref_index(twin, final)
            for a, b in zip(wi if isinstance(wi, tuple) else (wi,), gi if isinstance(gi, tuple) else (gi,)):
                assert np.array_equal(a, b), case.name
            if case.src[0] != "cube":
                continue
            n = case.src[1] // 2
            for layout in ("RGB", "I;16"):
                image = cc.case_frame(case, layout=layout)
                assert np.array_equal(cr.sample(image, np.copy(final)), er.sample(image, np.copy(final))), case.name
                assert np.array_equal(cr.remap_bilinear(image, np.copy(final)), er.remap_bilinear(image, np.copy(final))), case.name
                assert np.array_equal(cr.remap_catmull_rom(image, np.copy(final)), er.remap_catmull_rom(image, np.copy(final))), case.name
            for a, b in zip(cr.pretrunc(n, np.copy(final)), er.pretrunc(n, np.copy(final))):
                assert _same_bits(a, b), case.name
            seen += 1
    assert seen == 7  # every small case with a cube source


def test_the_substituted_position_function_and_the_restated_taps_agree():
    """Bilinear from an equi-angular source is oracle._bilinear_camera on the selected face at the unwarped position: calling it with the
    position function substituted (eac_ref.remap_bilinear) and restating its tap arithmetic from eac_ref.pretrunc give the same samples."""
    n = 24
    image = cc.case_frame(Case("t", pano(8, 16), er.eac(n)))
    cmap = er.stages(Case("t", pano(40, 80), er.eac(n), [(10, 20, 30)]))[-1]
    with np.errstate(all="ignore"):
        got = er.remap_bilinear(image, np.copy(cmap))
        face, fy, fx = er.pretrunc(n, np.copy(cmap))
    live = np.isfinite(fy) & np.isfinite(fx) & (fy >= 0) & (fy < n) & (fx >= 0) & (fx < n)
    sy, sx = np.where(live, fy, 0.5) - 0.5, np.where(live, fx, 0.5) - 0.5
    r0, c0 = np.floor(sy).astype(np.int64), np.floor(sx).astype(np.int64)
    ty, tx = (sy - r0)[..., None], (sx - c0)[..., None]
    r1, c1 = np.clip(r0 + 1, 0, n - 1), np.clip(c0 + 1, 0, n - 1)
    r0, c0 = np.clip(r0, 0, n - 1), np.clip(c0, 0, n - 1)
    img = image.astype(np.float64)
    oy, ox = (face // 3) * n, (face % 3) * n
    top = img[r0 + oy, c0 + ox] + tx * (img[r0 + oy, c1 + ox] - img[r0 + oy, c0 + ox])
    bot = img[r1 + oy, c0 + ox] + tx * (img[r1 + oy, c1 + ox] - img[r1 + oy, c0 + ox])
    want = np.clip(np.rint(top + ty * (bot - top)), 0, 255).astype(np.uint8)
    want[~live] = 0
    assert np.array_equal(got, want) and 0 < int((~live).sum()) < live.size // 8


def test_catmull_rom_with_the_position_substituted_and_from_the_restated_sampler_agree():
    """The same for Catmull-Rom: tests/catmull_rom_ref._camera with the position function substituted (eac_ref.remap_catmull_rom) against
    the 4 x 4 sum restated here from eac_ref.pretrunc - Keys' weights in the definition's order, taps clamped to the selected face."""
    n = 24
    image = cc.case_frame(Case("t", pano(8, 16), er.eac(n)))
    cmap = er.stages(Case("t", pano(40, 80), er.eac(n), [(10, 20, 30)]))[-1]
    with np.errstate(all="ignore"):
        got = er.remap_catmull_rom(image, np.copy(cmap))
        face, fy, fx = er.pretrunc(n, np.copy(cmap))
    live = np.isfinite(fy) & np.isfinite(fx) & (fy >= 0) & (fy < n) & (fx >= 0) & (fx < n)
    sy, sx = np.where(live, fy, 0.5) - 0.5, np.where(live, fx, 0.5) - 0.5
    ry, rx = np.floor(sy), np.floor(sx)

    def weights(t):
        return (((-0.5 * t + 1.0) * t - 0.5) * t, (1.5 * t - 2.5) * t * t + 1.0, ((-1.5 * t + 2.0) * t + 0.5) * t, (0.5 * t - 0.5) * t * t)

    wy, wx = weights((sy - ry)[..., None]), weights((sx - rx)[..., None])
    i0, j0 = ry.astype(np.int64), rx.astype(np.int64)
    oy, ox = (face // 3) * n, (face % 3) * n
    rows = [np.clip(i0 + k, 0, n - 1) + oy for k in (-1, 0, 1, 2)]
    cols = [np.clip(j0 + k, 0, n - 1) + ox for k in (-1, 0, 1, 2)]
    img = image.astype(np.float64)
    v = None
    for k in range(4):
        r = wx[0] * img[rows[k], cols[0]]
        for c in range(1, 4):
            r = r + wx[c] * img[rows[k], cols[c]]
        v = wy[0] * r if k == 0 else v + wy[k] * r
    want = np.clip(np.rint(v), 0, 255).astype(np.uint8)
    want[~live] = 0
    assert np.array_equal(got, want) and 0 < int((~live).sum()) < live.size // 8


# ---- 2. the properties the definition was checked for -------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_every_entry_is_valid_and_every_pixel_selects_its_own_face(n):
    with np.errstate(all="ignore"):
        m = er.coordinate_map(n)
        assert np.isfinite(m).all() and not m[:, :, 2].any()
        own = np.repeat(np.repeat(np.arange(6).reshape(2, 3), n, axis=0), n, axis=1)
        assert np.array_equal(er.select_face(np.copy(m)), own)
        # a rotated 32 x 64 panorama sampled from an equi-angular source of this face size has no black pixel
        case = Case("p", pano(32, 64), er.eac(n), [(10, 20, 30)])
        assert int((ec.ref_index(case, ec.ref_stages(case)[-1]) < 0).sum()) == 0


def test_no_black_pixel_between_cubes_and_the_identity_moves_what_the_cube_s_moves():
    rot = [(12, 34, 56)]
    with np.errstate(all="ignore"):
        for case in (Case("a", er.eac(28), er.eac(28), rot), Case("b", cr.cube(24), er.eac(32), rot), Case("c", er.eac(24), cr.cube(32), rot)):
            assert int((ec.ref_index(case, ec.ref_stages(case)[-1]) < 0).sum()) == 0, case.name
        # the reference's convention puts pixel centres on integers before truncation: the last bit decides each texel of an identity
        # remap, for the cube and for this one - documented, not repaired
        moved = {}
        for kind in (er.eac, cr.cube):
            case = Case("i", kind(24), kind(24))
            idx = ec.ref_index(case, ec.ref_stages(case)[-1])
            assert int((idx < 0).sum()) == 0
            moved[kind] = float((idx != np.arange(idx.size).reshape(idx.shape)).mean())
    print(f"identity remap, N = 24: {100 * moved[er.eac]:.1f} % of the texels move (cube: {100 * moved[cr.cube]:.1f} %)")
    assert 0.3 < moved[er.eac] < 0.5 and 0.3 < moved[cr.cube] < 0.5


# ---- 3. the host build of csrc/pb_eac.hpp against NumPy's bits, both math flavours -----------------------------------------------------------
HOST_SIZES = (1, 2, 3, 25, 28, 2048)
_CHILD = """
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from tests import eac_ref as er
groups = {}
for line in open(sys.argv[2]):
    which, n, arg, _ = line.split()
    groups.setdefault((which, int(n)), []).append(int(arg, 16))
for (which, n), args in groups.items():  # (insertion order: the program's)
    c = np.array(args, np.uint64).view(np.float64)
    r = (er.warp if which == "w" else er.unwarp)(c, n / 2)
    for arg, res in zip(args, r.view(np.uint64)):
        print(which, n, "%016x" % arg, "%016x" % int(res))
"""


def _numpy_lines(path, env):
    """The host program's lines recomputed by NumPy in a child process (its CPU dispatch is fixed when it starts): per function and face
    size ONE contiguous float64 array through tests/eac_ref.py."""
    res = subprocess.run([sys.executable, "-c", _CHILD, REPO, path], capture_output=True, text=True, env=env)
    assert res.returncode == 0, res.stderr
    return res.stdout.splitlines()


def _simd_kernels_in_use(env) -> bool:
    """Whether a child NumPy under `env` evaluates np.tan / np.arctan with its AVX-512 kernels (the goldens' SVML bits) or with libm."""
    probe = ("import numpy as np, sys; sys.path.insert(0, sys.argv[1]); from tests import helpers as H; "
             "print(int(H.live_numpy_is_the_goldens_numpy()))")
    res = subprocess.run([sys.executable, "-c", probe, REPO], capture_output=True, text=True, env=env)
    assert res.returncode == 0, res.stderr
    return res.stdout.strip() == "1"


def test_the_host_build_of_the_warp_functions_returns_numpy_s_bits(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    src = os.path.join(REPO, "tests", "c_host", "eac_warp_host.cpp")
    ran = []
    for flavour, defines in (("svml", ()), ("libm", ("-DPB_MATH_LIBM",))):
        exe = str(tmp_path / f"eac_warp_{flavour}")
        subprocess.run([gxx, *H.CHECK_MATH_FLAGS, *defines, "-o", exe, src], check=True)
        out = subprocess.run([exe, *map(str, HOST_SIZES)], capture_output=True, text=True, check=True).stdout
        lines = out.splitlines()
        assert len(lines) == sum(HOST_SIZES) + 4096 * len(HOST_SIZES)
        listing = tmp_path / f"{flavour}.txt"
        listing.write_text(out)
        env = dict(os.environ)
        if flavour == "libm":
            env["NPY_DISABLE_CPU_FEATURES"] = "AVX512F AVX512CD AVX512_SKX AVX512_CLX AVX512_CNL AVX512_ICL AVX512_SPR AVX512_KNL AVX512_KNM"
        if _simd_kernels_in_use(env) != (flavour == "svml"):
            continue  # this host's NumPy cannot produce this flavour
        want = _numpy_lines(str(listing), env)
        wrong = [(a, b) for a, b in zip(lines, want) if a != b]
        assert len(want) == len(lines) and not wrong, f"{flavour}: {len(wrong)} of {len(lines)} results differ from NumPy's; the first: {wrong[:2]}"
        ran.append(flavour)
    print(f"flavours checked against this host's NumPy: {ran}")
    assert ran, "neither math flavour could be produced by this host's NumPy"
    if H.live_numpy_is_the_goldens_numpy():
        assert "svml" in ran
    # the same program under the host sanitizers, run on its own
    exe = str(tmp_path / "eac_warp_san")
    subprocess.run([gxx, *H.CHECK_MATH_SANITIZER_FLAGS, "-o", exe, src], check=True)
    res = subprocess.run([exe, "1", "3", "28"], capture_output=True, text=True)
    assert res.returncode == 0 and not res.stderr, res.stderr


# ---- 4. the facade -------------------------------------------------------------------------------------------------------------------------
def test_mapping_keyword_and_projection_kinds():
    img = np.zeros((48, 72, 3), np.uint8)
    plain, named, eac = pb.CubemapImage(img), pb.CubemapImage(img, mapping="gnomonic"), pb.CubemapImage(img, "equiangular")
    assert plain.mapping == named.mapping == "gnomonic" and eac.mapping == "equiangular" and plain.face_size == eac.face_size == 24
    assert plain._proj("dst").key() == named._proj("src").key() == (5, 0, 48, 72, 0.0, 0.0, 0.0)  # the default: today's object
    assert (nat.KIND_CUBE, nat.KIND_EAC) == (5, 8) and nat.KIND_EAC in nat.LENSLESS_KINDS  # (6 and 7 stay refused kinds)
    assert eac._proj("dst").key() == eac._proj("src").key() == (8, 0, 48, 72, 0.0, 0.0, 0.0)
    for bad in ("equi-angular", "EAC", "", None, 6):
        with pytest.raises(ValueError, match="'gnomonic' or 'equiangular'"):
            pb.CubemapImage(img, mapping=bad)
    with pytest.raises(ValueError):
        pb.CubemapImage(np.zeros((10, 14, 3), np.uint8), mapping="equiangular")  # the cube's shape rule
    m4 = eac.get_coordinate_map(supersample=4)
    assert m4.is_lazy and m4.shape == (192, 288, 3) and m4.supersample == 4 and m4.dst_proj.kind == nat.KIND_EAC
    # plan-cache keys and the parameter block of a multi-GPU run tell the two mappings apart
    from photonbend_amd import parallel

    other = pb.PanoramaImage(np.zeros((32, 64, 3), np.uint8))._proj()
    p5, p6 = plain._proj(), eac._proj()
    assert len({pj._plan_key(p5, [], other, 0), pj._plan_key(p6, [], other, 0), pj._plan_key(other, [], p5, 0), pj._plan_key(other, [], p6, 0)}) == 4
    d, rots, s = parallel.unpack_params(parallel.pack_params(p6, [np.eye(3)], p5))
    assert d.key() == p6.key() and s.key() == p5.key() and len(rots) == 1


def test_the_library_takes_the_kind_and_applies_the_cube_s_shape_rule():
    import ctypes

    lib = nat.load()
    h = ctypes.c_void_p()
    pano_p, cube_p, eac_p = nat.make_proj(nat.KIND_PANO, 4, 8), nat.make_proj(nat.KIND_CUBE, 8, 12), nat.make_proj(nat.KIND_EAC, 8, 12, 4242, 1.5, 2.5, 3.5)
    for dst, src in ((eac_p, pano_p), (pano_p, eac_p), (eac_p, eac_p), (cube_p, eac_p)):
        assert lib.pb_plan_create_ex(ctypes.byref(dst), None, 0, ctypes.byref(src), nat.PLAN_DEFER, 0, ctypes.byref(h)) == 0
        assert lib.pb_plan_matches(h, ctypes.byref(dst), None, 0, ctypes.byref(src)) == 1
        # a plan of one mapping does not match a request of the other, same shape
        flip = lambda p: nat.make_proj({5: 8, 8: 5}.get(p.kind, p.kind), p.height, p.width)  # noqa: E731
        assert lib.pb_plan_matches(h, ctypes.byref(flip(dst)), None, 0, ctypes.byref(flip(src))) == 0
        lib.pb_plan_destroy(h)
    for hgt, wid in ((8, 13), (9, 12), (8, 8), (2, 4)):
        bad = nat.make_proj(nat.KIND_EAC, hgt, wid)
        for dst, src in ((bad, pano_p), (pano_p, bad)):
            assert lib.pb_plan_create_ex(ctypes.byref(dst), None, 0, ctypes.byref(src), nat.PLAN_DEFER, 0, ctypes.byref(h)) == -1
            assert b"(2N, 3N)" in lib.pb_last_error()
    assert lib.pb_index_from_map_i32(ctypes.byref(eac_p), ctypes.c_void_p(16), 4, 4, ctypes.c_void_p(16), None, ctypes.c_void_p(16), None, None) == -1
    assert b"cube source has no lens" in lib.pb_last_error()
    assert lib.pb_abi_version() == 5  # additive


def _route_row(r):
    return None if r is None else (r.name, r.fallback, len(r.rotations), r.eager, r.device_out, r.supersample, _route_row(r.inner))


def test_route_gives_the_cube_s_row_for_every_call_shape_of_the_grid():
    """Every (layout, image residency, map, interpolation, supersample) tests/test_facade_routes_host.py enumerates for a cube source,
    asked of ``_route`` directly: the equi-angular cube's answer - route or argument error - is the cube's."""
    from tests import test_facade_routes_host as grid

    def ask(mapping, layout, residency, map_kind, interpolation, n):
        cmap, ss = grid._map(map_kind, n)
        try:
            k = nat.check_interpolation(interpolation, pj._map_supersample(cmap, ss))
            call = pj.CubemapImage(grid._image(layout, residency), mapping=mapping)._call(cmap, interpolation, k)
            return call._replace(src=None), _route_row(pj._route(call)), call.src.kind
        except Exception as exc:
            return type(exc).__name__, str(exc), None

    seen = set()
    with grid.stand_ins():
        axes = [grid.AXES[a] for a in ("layout", "image", "map", "interpolation", "supersample")]
        for cell in itertools.product(*axes):
            a, b = ask("gnomonic", *cell), ask("equiangular", *cell)
            assert repr(a[:2]) == repr(b[:2]), (cell, a, b)
            assert (a[2], b[2]) in ((5, 8), (None, None)), cell
            seen.add(a[1][0] if a[2] else a[0])
    assert {"HOST_RGB8", "HOST_PX", "DEV_RGB8", "DEV_PX", "PLAN_GATHER", "MAP_RGB8", "MAP_GATHER", "MAP_INTERP", "SS_FUSED", "SS_GENERIC"} <= seen, seen


def test_cli_has_the_mapping_options_and_the_third_command(tmp_path):
    from click.testing import CliRunner
    from PIL import Image

    from oracle.synth import synth_frame
    from photonbend_amd.scripts import cli

    assert {"pano-to-cubemap", "cubemap-to-pano", "cubemap-to-cubemap"} <= set(cli.main.commands)
    opts = lambda name: {o for p in cli.main.commands[name].params for o in p.opts}  # noqa: E731
    assert "--mapping" in opts("pano-to-cubemap") and "--mapping" in opts("cubemap-to-pano")
    assert {"--input-mapping", "--output-mapping", "--face-size", "-r", "--interpolation", "--supersample"} <= opts("cubemap-to-cubemap")
    for name in ("pano-to-cubemap", "cubemap-to-pano", "cubemap-to-cubemap"):
        for p in cli.main.commands[name].params:
            if "mapping" in (p.name or ""):
                assert p.default == "gnomonic" and list(p.type.choices) == ["gnomonic", "equiangular"]
    cube, odd = tmp_path / "cube.png", tmp_path / "odd.png"
    Image.fromarray(synth_frame(16, 24)).save(cube)
    Image.fromarray(synth_frame(16, 26)).save(odd)
    run = lambda *a: CliRunner().invoke(cli.main, list(a))  # noqa: E731
    assert run("cubemap-to-cubemap", str(cube), "--output-mapping", "conformal", str(tmp_path / "o.png")).exit_code == 2
    assert run("cubemap-to-pano", str(cube), "--mapping", "eac", str(tmp_path / "o.png")).exit_code == 2
    bad = run("cubemap-to-cubemap", str(odd), "--input-mapping", "equiangular", str(tmp_path / "o.png"))
    assert bad.exit_code == 2 and "(2N, 3N)" in bad.output
    assert run("cubemap-to-cubemap", str(cube), "--face-size", "0", str(tmp_path / "o.png")).exit_code == 2
    assert run("cubemap-to-cubemap", str(cube), str(tmp_path / "o.bmp")).exit_code == 1


# ---- 5. the fixture --------------------------------------------------------------------------------------------------------------------------
def test_the_definition_reproduces_the_fixture_on_the_goldens_platform():
    if not H.live_numpy_is_the_goldens_numpy():
        pytest.skip("this host's NumPy is not the goldens': the fixture holds that platform's bits")
    from tests import make_eac_goldens

    gold = np.load(os.path.join(H.GOLD, "eac.npz"))
    got = make_eac_goldens.arrays()
    assert sorted(got) == sorted(gold.files)
    for key in gold.files:
        assert got[key].dtype == gold[key].dtype and np.array_equal(got[key], gold[key]), key
    assert os.path.getsize(os.path.join(H.GOLD, "eac.npz")) < 1 << 20
