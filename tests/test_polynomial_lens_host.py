"""The polynomial (Kannala-Brandt) lens on the host: the factory's definition and validation, its tags and roles, the oracle with the
(forward, reverse) pair against the REFERENCE's outputs (tests/golden/polynomial.npz, tests/make_polynomial_goldens.py), the registry of
the C ABI through ctypes, the multi-GPU parameter block and the CLI's usage errors.  No GPU."""

import math
import os

import numpy as np
import pytest

import photonbend_amd as pb
from oracle import reference_path as orc
from photonbend_amd import _native as nat
from photonbend_amd import parallel
from photonbend_amd.core.lens import lens_id
from tests import helpers as H
from tests import polynomial_cases as pc

GOLD = np.load(os.path.join(H.GOLD, "polynomial.npz"))
CASES = pc.small_cases()
ALL_LENSES = dict(pc.LENSES, ORTH9=pc.ORTH9)


def make(name):
    k, deg = ALL_LENSES[name]
    return pb.polynomial(*k, max_theta=orc.to_radians(deg))


# ---- the definition, written out a second time in plain Python floats: one operation per line --------------------------------------
def p_plain(k, t):
    t2 = t * t
    a = t2 * k[3]
    a = k[2] + a
    a = t2 * a
    a = k[1] + a
    a = t2 * a
    a = k[0] + a
    a = t2 * a
    a = 1.0 + a
    return t * a


def dp_plain(d, t):
    t2 = t * t
    a = t2 * d[3]
    a = d[2] + a
    a = t2 * a
    a = d[1] + a
    a = t2 * a
    a = d[0] + a
    a = t2 * a
    return 1.0 + a


def forward_plain(k, max_theta, theta):
    return p_plain(k, theta) if theta <= max_theta else math.inf


def reverse_plain(k, max_theta, r):
    d = (3.0 * k[0], 5.0 * k[1], 7.0 * k[2], 9.0 * k[3])
    r_max = p_plain(k, max_theta)
    if not r <= r_max:
        return math.inf
    t = r
    for _ in range(10):
        num = p_plain(k, t) - r
        den = dp_plain(d, t)
        step = num / den
        t = t - step
    return t


def same_bits(a, b):
    return H.bits(np.asarray(a, np.float64)).tolist() == H.bits(np.asarray(b, np.float64)).tolist()


@pytest.mark.parametrize("name", sorted(ALL_LENSES))
def test_bits_of_the_definition(name):
    k, deg = ALL_LENSES[name]
    mt = orc.to_radians(deg)
    L = make(name)
    rng = np.random.default_rng(11)
    theta = np.concatenate([np.linspace(0.0, mt, 257), rng.uniform(0.0, 1.2 * mt, 300), [mt, np.nextafter(mt, 4.0), 0.0, 1e-300, 3.2]])
    r_max = p_plain(k, mt)
    r = np.concatenate([np.linspace(0.0, r_max, 257), rng.uniform(0.0, 1.3 * r_max, 300), [r_max, np.nextafter(r_max, 9.0), 0.0, 1e-300, np.nan, np.inf]])
    fwd, rev = L.forward_function(theta.copy()), L.reverse_function(r.copy())
    assert fwd.dtype == np.float64 and rev.dtype == np.float64
    assert same_bits(fwd, [forward_plain(k, mt, float(t)) for t in theta])
    assert same_bits(rev, [reverse_plain(k, mt, float(x)) for x in r])
    # scalar == array, bit for bit; Python floats in, Python floats out
    for t in theta[::7]:
        s = L.forward_function(float(t))
        assert isinstance(s, float) and same_bits(s, forward_plain(k, mt, float(t)))
    for x in r[::7]:
        s = L.reverse_function(float(x))
        assert isinstance(s, float) and same_bits(s, reverse_plain(k, mt, float(x)))
    # beyond the domain: +inf (NaN included - the comparison is false)
    assert L.forward_function(float(np.nextafter(mt, 4.0))) == math.inf and L.reverse_function(float("nan")) == math.inf
    assert np.isposinf(fwd[theta > mt]).all() and np.isposinf(rev[~(r <= r_max)]).all() and np.isfinite(rev[r <= r_max]).all()
    # the caller's arrays are not written
    keep = theta.copy()
    L.forward_function(theta)
    assert same_bits(theta, keep)


def test_zero_is_the_identity_both_ways():
    Z = pb.polynomial()
    x = np.concatenate([np.linspace(0.0, math.pi, 1001), [1e-300, 1.234, math.pi]])
    assert same_bits(Z.forward_function(x.copy()), x) and same_bits(Z.reverse_function(x.copy()), x)
    assert Z.forward_function(1.234) == 1.234 and Z.reverse_function(1.234) == 1.234
    assert Z.forward_function(3.2) == math.inf and Z.reverse_function(3.2) == math.inf


# |reverse(forward(theta)) - theta| on 2 M angles and how far Newton steps 8, 9, 10 still move the iterate (in ulp): properties of the
# definition, measured when it was fixed (equisolid series to 110 degrees, stereographic to 100, an OpenCV-like set to 105: <= 6.7e-16 and
# 0-4 ulp; the orthographic series to 85 degrees, where dp falls to 0.087: 4.7e-15 and 17-22 ulp)
ROUND_TRIP = {"EQS9": (6.7e-16, 4.0), "STE9": (6.7e-16, 4.0), "CAL": (6.7e-16, 4.0), "ORTH9": (4.7e-15, 22.0)}


@pytest.mark.parametrize("name", sorted(ROUND_TRIP))
def test_round_trip_and_convergence_bounds(name):
    k, deg = ALL_LENSES[name]
    bound, ulps = ROUND_TRIP[name]
    L = make(name)
    theta = np.linspace(0.0, orc.to_radians(deg), 2_000_001)
    r = L.forward_function(theta)
    err = float(np.abs(L.reverse_function(r) - theta).max())
    print(f"{name}: max |reverse(forward(theta)) - theta| = {err:.3e} (bound {bound:.1e})")
    assert err <= bound
    d = (3.0 * k[0], 5.0 * k[1], 7.0 * k[2], 9.0 * k[3])
    t, moves = r.copy(), []
    for _ in range(10):
        tn = t - (p_plain(k, t) - r) / dp_plain(d, t)
        moves.append(float(np.max(np.abs(tn - t) / np.spacing(np.maximum(np.abs(tn), 1e-300)))))
        t = tn
    print(f"{name}: steps 8, 9, 10 move the iterate by at most {moves[7]:.1f}, {moves[8]:.1f}, {moves[9]:.1f} ulp; step 6 by {moves[5]:.3g}")
    assert max(moves[7:]) <= ulps
    assert same_bits(t, L.reverse_function(r))


def test_six_steps_are_not_enough_on_the_orthographic_series():
    """why the count is ten: after six steps the orthographic series is still 2.5e-10 off at the rim"""
    k, deg = pc.ORTH9
    d = (3.0 * k[0], 5.0 * k[1], 7.0 * k[2], 9.0 * k[3])
    theta = np.linspace(0.0, orc.to_radians(deg), 200_001)
    r = p_plain(k, theta)
    t = r.copy()
    for _ in range(6):
        t = t - (p_plain(k, t) - r) / dp_plain(d, t)
    assert float(np.abs(t - theta).max()) > 1e-11


def test_factory_validation():
    with pytest.raises(ValueError, match="finite"):
        pb.polynomial(k1=float("nan"))
    with pytest.raises(ValueError, match="finite"):
        pb.polynomial(k3=float("inf"), max_theta=1.0)
    for bad in (0.0, -1.0, 3.2, float("nan")):
        with pytest.raises(ValueError, match="max_theta"):
            pb.polynomial(0.01, max_theta=bad)
    with pytest.raises(ValueError, match="real numbers"):
        pb.polynomial("a")
    # not monotonic on the domain: the message says what to do about it
    with pytest.raises(ValueError, match="not increasing.*max_theta") as exc:
        pb.polynomial(*pc.ORTH9[0])  # default max_theta = pi: the series of sin(theta) turns over at 90 degrees
    assert "max_theta" in str(exc.value) and "pi" in str(exc.value)
    with pytest.raises(ValueError, match="not increasing"):
        pb.polynomial(*pc.ORTH9[0], max_theta=orc.to_radians(95))  # sin's series: dp = 0 at 90 degrees
    with pytest.raises(ValueError, match="not increasing"):
        pb.polynomial(k1=-0.5, max_theta=1.0)  # dp = 1 - 1.5 t^2 = 0 at 0.816
    # a root of dp strictly inside the domain that no coarse sampling of the ends would see: dp = (1 - u / 0.49)^2-like dip
    with pytest.raises(ValueError, match="not increasing"):
        pb.polynomial(k1=-2.0 / (3 * 0.49), k2=1.0 / (5 * 0.49 * 0.49), max_theta=1.5)  # dp = (1 - t^2 / 0.49)^2: a double root at t = 0.7
    # monotonic, but ten steps from t = r do not invert it to 2^-40: dp comes within 1e-9 of zero at the rim
    with pytest.raises(ValueError, match="Newton|not increasing"):
        pb.polynomial(*pc.ORTH9[0], max_theta=orc.to_radians(89.9999))
    # the lenses of the test suite pass
    for name in ALL_LENSES:
        make(name)


def test_tags_and_roles():
    L = make("CAL")
    k, deg = pc.LENSES["CAL"]
    want = tuple(k) + (orc.to_radians(deg),)
    for fn in (L.forward_function, L.reverse_function):
        assert fn.pb_lens_name == "polynomial" and fn.pb_lens_polynomial == want
    lid = lens_id(L)
    assert lid is not None and lid >= nat.LENS_POLYNOMIAL_BASE and nat.lens_polynomial_info(lid) == want
    assert lens_id(make("CAL")) == lid and lens_id(make("EQS9")) != lid  # the same coefficients: the same id
    cam = pb.CameraImage(np.zeros((40, 40, 3), np.uint8), pb.utils.to_radians(190), L, magnitude=19.5)
    assert cam.f_distance == 19.5 / L.forward_function(pb.utils.to_radians(190) / 2) and isinstance(cam.f_distance, float)
    assert cam._proj("dst").lens == lid and cam._proj("src").lens == lid
    # device only in the role whose callable is tagged
    user = lambda x: L.reverse_function(x)  # noqa: E731
    mixed = pb.CameraImage(np.zeros((40, 40, 3), np.uint8), 3.0, pb.Lens(L.forward_function, user))
    assert mixed._proj("src").lens == lid and mixed._proj("dst").lens == nat.LENS_CUSTOM
    assert lens_id(pb.Lens(L.forward_function, user)) is None
    both = pb.Lens(L.forward_function, make("EQS9").reverse_function)  # two polynomial lenses: each role its own
    m2 = pb.CameraImage(np.zeros((40, 40, 3), np.uint8), 3.0, both)
    assert m2._proj("src").lens == lid and m2._proj("dst").lens == lens_id(make("EQS9")) and lens_id(both) is None
    # a lazy recipe, like a built-in lens's (no GPU touched)
    cmap = cam.get_coordinate_map()
    assert cmap.is_lazy and cmap.shape == (40, 40, 3)
    d = pb.DoubleCameraImage(np.zeros((32, 64, 3), np.uint8), pb.utils.to_radians(195), make("EQS9"))
    assert d._proj("dst").lens == lens_id(make("EQS9")) and d.get_coordinate_map().is_lazy
    assert "polynomial" in pb.core.lens.__all__ and pb.polynomial is pb.core.lens.polynomial


def test_half_fov_beyond_max_theta_is_refused():
    L = make("CAL")  # max_theta = 105 degrees
    cam = pb.CameraImage(np.zeros((40, 40, 3), np.uint8), pb.utils.to_radians(220), L)
    assert cam.f_distance == 0.0  # magnitude / inf: why it must be refused
    for role in ("dst", "src"):
        with pytest.raises(ValueError, match="max_theta") as exc:
            cam._proj(role)
        assert repr(pb.utils.to_radians(220) / 2) in str(exc.value) and repr(orc.to_radians(105.0)) in str(exc.value)
    with pytest.raises(ValueError, match="max_theta"):
        cam.get_coordinate_map()
    dbl = pb.DoubleCameraImage(np.zeros((32, 64, 3), np.uint8), pb.utils.to_radians(220), L)
    with pytest.raises(ValueError, match="max_theta"):
        dbl._proj("src")
    pb.CameraImage(np.zeros((40, 40, 3), np.uint8), pb.utils.to_radians(210), L)._proj("dst")  # fov / 2 == max_theta: fine


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_oracle_with_the_pair_equals_the_reference(case):
    n = case.name
    for k, st in enumerate(pc.orc_stages(case)):
        want = GOLD[f"{n}/map{k}"].view(np.float64)
        assert st.shape == want.shape and bool(((H.bits(st) == H.bits(want)) | (np.isnan(st) & np.isnan(want))).all()), (n, k)
    od, os_, rots = pc.orc_proj(case.dst), pc.orc_proj(case.src), pc.orc_rots(case)
    idx = orc.remap_index(od, os_, rots)
    if case.src[0] == "double":
        assert np.array_equal(idx[0], GOLD[f"{n}/idx_l"]) and np.array_equal(idx[1], GOLD[f"{n}/idx_r"])
        assert np.array_equal(H.bits(idx[2]), GOLD[f"{n}/w_l"]) and np.array_equal(H.bits(idx[3]), GOLD[f"{n}/w_r"])
    else:
        assert np.array_equal(idx, GOLD[f"{n}/idx"])
    assert np.array_equal(orc.remap(od, os_, pc.case_frame(case), rots), GOLD[f"{n}/u8"])


def test_goldens_cover_the_cases_they_should():
    assert len(CASES) >= 12 and os.path.getsize(os.path.join(H.GOLD, "polynomial.npz")) < 1 << 20
    # the corners of P_dst_beyond_rmax lie beyond r_max: latitude +inf, invalid
    m = GOLD["P_dst_beyond_rmax/map0"].view(np.float64)
    assert np.isposinf(m[0, 0, 0]) and m[0, 0, 2] == 1.0 and np.isfinite(m[20, 20, 0])
    # P_src_past_max_theta: directions past the lens's domain are black although the frame has data there
    idx = GOLD["P_src_past_max_theta/idx"]
    assert (idx[-1] == -1).all() and (idx[0] >= 0).any()
    # ZERO is geometrically the built-in equidistant lens: the same bytes
    z = pc.case_by_name("P_zero")
    eq = orc.Proj("camera", 48, 48, "equidistant", orc.to_radians(360), z.dst[5])
    assert np.array_equal(orc.remap(eq, pc.orc_proj(z.src), pc.case_frame(z), pc.orc_rots(z)), GOLD["P_zero/u8"])


# ---- the C ABI's registry through ctypes (the library loads without a GPU) -----------------------------------------------------------
def test_registry_through_ctypes():
    import ctypes as C

    lib = nat.load()
    assert hasattr(lib, "pb_lens_polynomial") and hasattr(lib, "pb_lens_polynomial_info") and lib.pb_abi_version() == 5

    def register(k, mt):
        out = C.c_int(-1)
        rc = lib.pb_lens_polynomial((C.c_double * 4)(*k), mt, C.byref(out))
        return rc, out.value

    k, deg = pc.LENSES["STE9"]
    rc, a = register(k, orc.to_radians(deg))
    assert rc == 0 and a >= nat.LENS_POLYNOMIAL_BASE
    assert register(k, orc.to_radians(deg)) == (0, a)  # the same coefficients: the same id
    rc, b = register(k, orc.to_radians(deg - 1))
    assert rc == 0 and b != a  # max_theta is part of the lens
    rc, c = register((k[0] + 1e-9,) + tuple(k[1:]), orc.to_radians(deg))
    assert rc == 0 and c not in (a, b)
    kk, mt = (C.c_double * 4)(), C.c_double()
    assert lib.pb_lens_polynomial_info(a, kk, C.byref(mt)) == 0 and tuple(kk) == tuple(k) and mt.value == orc.to_radians(deg)
    assert lib.pb_lens_polynomial_info(a, None, None) == 0
    # refused like the Python factory refuses them
    for bad_k, bad_mt in (((float("nan"), 0, 0, 0), 1.0), ((0, 0, 0, 0), 0.0), ((0, 0, 0, 0), 3.2), (pc.ORTH9[0], math.pi), (pc.LENSES["EQS9"][0], math.pi),
                          ((-0.5, 0, 0, 0), 1.0), ((-2.0 / (3 * 0.49), 1.0 / (5 * 0.49 * 0.49), 0, 0), 1.5)):
        rc, _ = register(bad_k, bad_mt)
        assert rc == -1, (bad_k, bad_mt)
        assert b"polynomial lens" in lib.pb_last_error()
    assert lib.pb_lens_polynomial(None, 1.0, None) == -1
    for not_an_id in (0, 6, 7, 15, 16 + 100000, -1):
        assert lib.pb_lens_polynomial_info(not_an_id, kk, C.byref(mt)) == -1
    # an id nobody registered is no lens: the request gate refuses it
    bogus = nat.make_proj(nat.KIND_CAMERA, 8, 8, 16 + 100000, 3.0, 4.0, 1.0)
    pano = nat.make_proj(nat.KIND_PANO, 8, 16)
    h = C.c_void_p()
    assert lib.pb_plan_create_ex(C.byref(bogus), None, 0, C.byref(pano), nat.PLAN_DEFER, 0, C.byref(h)) == -1
    assert b"registered" in lib.pb_last_error()
    # a deferred plan (no device work) takes a registered id in either role, and matches by coefficients
    for role in ("dst", "src"):
        L = make("CAL")
        cam = pb.CameraImage(np.zeros((8, 8, 3), np.uint8), 3.0, L)._proj(role)
        d, s = (cam, pano) if role == "dst" else (pano, cam)
        plan = nat.Plan(d, [], s, defer=True)
        assert lib.pb_plan_matches(plan.handle, C.byref(d), None, 0, C.byref(s)) == 1
        other = pb.CameraImage(np.zeros((8, 8, 3), np.uint8), 3.0, pb.polynomial(-0.0357 + 1e-6, 0.0031, -0.00042, 0.00002, max_theta=orc.to_radians(105)))._proj(role)
        other.f_distance = cam.f_distance  # only the coefficients differ
        d2, s2 = (other, pano) if role == "dst" else (pano, other)
        assert lib.pb_plan_matches(plan.handle, C.byref(d2), None, 0, C.byref(s2)) == 0


def test_python_and_c_validators_agree_on_random_sets_near_the_boundary():
    """polynomial() and pb_lens_polynomial validate independently (the factory needs no library); a set one accepts and the other refuses
    would surface as a PbError out of _proj.  3 000 random sets, most of them built to sit near a boundary: dp with a root just inside or
    just outside the domain, a double root, dp barely positive at the rim (where the Newton self-check decides), plain random ones."""
    rng = np.random.default_rng(20240607)
    verdicts = {True: 0, False: 0}
    for i in range(3000):
        mt = float(rng.uniform(0.3, math.pi))
        kind = i % 5
        if kind == 0:  # dp = (1 - a u)(1 - b u): roots at 1 / a and 1 / b, around the end of the domain
            a = 1.0 / (mt * mt * float(rng.uniform(0.9, 1.1)))
            b = float(rng.uniform(-0.2, 0.2))
            d = (-(a + b), a * b, 0.0, 0.0)
        elif kind == 1:  # a double root inside the domain, lifted or lowered by a hair
            u0 = float(rng.uniform(0.05, 1.0)) * mt * mt
            eps = float(rng.choice([-1e-9, 0.0, 1e-9, 1e-6, 1e-3]))
            d = (-2.0 / u0, 1.0 / (u0 * u0) + eps / (u0 * u0), 0.0, 0.0)
        elif kind == 2:  # a truncated cosine-like series scaled so that its first zero lies near max_theta
            s_ = (math.pi / 2 / mt) ** 2 * float(rng.uniform(0.8, 1.2))
            d = (-s_ / 2, s_ * s_ / 24, -s_ ** 3 / 720, s_ ** 4 / 40320)
        elif kind == 3:  # calibration-sized coefficients
            d = tuple(float(v) for v in rng.normal(0.0, [0.3, 0.1, 0.03, 0.01]))
        else:  # large ones
            d = tuple(float(v) for v in rng.normal(0.0, 2.0, 4) / np.array([mt ** 2, mt ** 4, mt ** 6, mt ** 8]))
        k = (d[0] / 3.0, d[1] / 5.0, d[2] / 7.0, d[3] / 9.0)
        try:
            pb.polynomial(*k, max_theta=mt)
            py = True
        except ValueError:
            py = False
        try:
            nat.lens_polynomial(k, mt)
            c = True
        except nat.PbError:
            c = False
        assert py == c, (k, mt, py, c)
        verdicts[py] += 1
    print(f"accepted {verdicts[True]}, refused {verdicts[False]} of 3000 - the same by both validators")
    assert verdicts[True] > 300 and verdicts[False] > 300


def test_registry_is_thread_safe_and_bounded_ids_are_stable():
    import threading

    ids = [[] for _ in range(8)]

    def work(slot):
        for i in range(40):
            ids[slot].append(nat.lens_polynomial((1e-4 * i, 0.0, 0.0, 0.0), 1.0))

    ts = [threading.Thread(target=work, args=(s,)) for s in range(8)]
    [t.start() for t in ts]
    [t.join() for t in ts]
    assert all(row == ids[0] for row in ids) and len(set(ids[0])) == 40
    for i, lid in enumerate(ids[0]):
        assert nat.lens_polynomial_info(lid) == (1e-4 * i, 0.0, 0.0, 0.0, 1.0)


def test_proj_key_names_coefficients_not_ids():
    L = make("EQS9")
    p = pb.CameraImage(np.zeros((8, 8, 3), np.uint8), 3.0, L)._proj("src")
    key = p.key()
    assert p.lens not in key and ("polynomial",) + L.forward_function.pb_lens_polynomial in key


def test_parallel_block_round_trips_coefficients():
    cal, eqs = make("CAL"), make("EQS9")
    dst = pb.CameraImage(np.zeros((40, 40, 3), np.uint8), 3.0, cal, magnitude=19.5)._proj("dst")
    src = pb.DoubleCameraImage(np.zeros((32, 64, 3), np.uint8), pb.utils.to_radians(195), eqs)._proj("src")
    rots = [np.arange(9.0).reshape(3, 3), np.eye(3)]
    block = parallel.pack_params(dst, rots, src)
    assert block.shape == (parallel.BLOCK_LEN,) and block.dtype == np.float64
    # the block carries coefficients and a marker, never the process-local id
    assert block[3] == nat.LENS_POLYNOMIAL_BASE and block[10] == nat.LENS_POLYNOMIAL_BASE
    assert tuple(block[-10:-5]) == cal.forward_function.pb_lens_polynomial and tuple(block[-5:]) == eqs.forward_function.pb_lens_polynomial
    d2, r2, s2 = parallel.unpack_params(block)
    assert d2.key() == dst.key() and s2.key() == src.key() and d2.lens == dst.lens and s2.lens == src.lens
    assert all(np.array_equal(a, b) for a, b in zip(r2, rots))
    # built-in lenses: zeros behind the rotations, ids as before
    pano = nat.make_proj(nat.KIND_PANO, 8, 16)
    eq = pb.CameraImage(np.zeros((8, 8, 3), np.uint8), 3.0, pb.equisolid())._proj("src")
    b2 = parallel.pack_params(pano, [], eq)
    assert not b2[-10:].any() and b2[10] == nat.LENS_IDS["equisolid"]
    d3, _, s3 = parallel.unpack_params(b2)
    assert d3.key() == pano.key() and s3.key() == eq.key()
    # a marker without coefficients is a corrupt block, not a lens
    b3 = block.copy()
    b3[-10:] = 0.0
    with pytest.raises(nat.PbError, match="without coefficients"):
        parallel.unpack_params(b3)


# ---- CLI ------------------------------------------------------------------------------------------------------------------------------
def test_cli_usage_errors(tmp_path):
    from click.testing import CliRunner
    from PIL import Image

    from photonbend_amd.scripts.cli import main

    inp, out = str(tmp_path / "in.png"), str(tmp_path / "out.png")
    Image.fromarray(np.zeros((32, 32, 3), np.uint8)).save(inp)
    base = ["make-pano", inp, "--type", "inscribed", "--fov", "180"]

    def run(*args):
        res = CliRunner().invoke(main, list(args))
        return res.exit_code, res.output

    code, text = run(*base, "--lens", "polynomial", out)
    assert code == 2 and "--lens-coefficients" in text
    code, text = run(*base, "--lens", "equidistant", "--lens-coefficients", "0", "0", "0", "0", out)
    assert code == 2 and "polynomial" in text
    code, text = run(*base, "--lens", "equidistant", "--lens-max-theta", "100", out)
    assert code == 2 and "polynomial" in text
    code, text = run(*base, "--lens", "polynomial", "--lens-coefficients", "-0.5", "0", "0", "0", out)
    assert code == 2 and "max_theta" in text  # the factory's refusal, as a usage error
    code, text = run(*base, "--lens", "polynomial", "--lens-coefficients", "1", "2", "3", out)
    assert code == 2
    code, text = run("make-photo", inp, "--type", "inscribed", "--fov", "180", "--lens", "polynomial", out)
    assert code == 2 and "--lens-coefficients" in text
    alter = ["alter-photo", inp, "--itype", "inscribed", "--ifov", "180", "--otype", "inscribed", "--ofov", "180"]
    code, text = run(*alter, "--ilens", "polynomial", "--olens", "equidistant", out)
    assert code == 2 and "--ilens-coefficients" in text
    code, text = run(*alter, "--ilens", "equidistant", "--olens", "polynomial", out)
    assert code == 2 and "--olens-coefficients" in text
    code, text = run(*alter, "--ilens", "equidistant", "--olens", "equidistant", "--olens-coefficients", "0", "0", "0", "0", out)
    assert code == 2 and "--olens" in text
    code, text = run(*alter, "--ilens", "equidistant", "--ilens-max-theta", "90", "--olens", "equidistant", out)
    assert code == 2 and "--ilens" in text
    assert not os.path.exists(out)
    for cmd in ("make-photo", "make-pano", "alter-photo"):
        code, text = run(cmd, "--help")
        assert code == 0 and "polynomial" in text and "coefficients" in text and "max-theta" in text
