"""Lens models - the drop-in for photonbend.core.lens (lens.py:48-64, :341-412).

A ``Lens`` is a pair of callables (forward: incidence angle -> distance in
focal-length units, reverse: the inverse).  The built-in factories return
callables that (a) work on the host for scalars/arrays exactly like the
reference's (they are needed there: f_distance = magnitude / forward(fov / 2) is
a host-side scalar, projection.py:141-144) and (b) carry a ``pb_lens`` id, which
is what the HIP kernels dispatch on.  A Lens built from user callables has no
id: its functions are evaluated by the host on planes the device supplies (the
exact radius mesh of a destination, the latitude plane of a source) and the
device does everything else - index map, gather, blend (PB_LENS_CUSTOM,
pb_index_from_map_i32's distance planes; projection.py of this package).

``polynomial(k1..k4, max_theta)`` - a calibrated Kannala-Brandt lens - has no factory in the reference, which takes it as a
Lens of two callables; here its callables carry their coefficients and the library evaluates the same definition on the
device (PB_LENS_POLYNOMIAL).
"""

from __future__ import annotations

import warnings
from dataclasses import dataclass
from typing import Callable

import numpy as np

from ..utils import to_radians
from .. import _native
from .._native import LENS_IDS


@dataclass
class Lens:
    forward_function: Callable
    reverse_function: Callable


def lens_id(lens_or_fn) -> int | None:
    """pb_lens id of a built-in lens (or one of its functions), else None.  The functions of a ``polynomial()`` lens carry their
    coefficients (``pb_lens_polynomial``); their id is the one the library's registry gives those (pb_lens_polynomial: the same
    coefficients give the same id, in this process)."""
    if isinstance(lens_or_fn, Lens):
        a = lens_id(lens_or_fn.forward_function)
        b = lens_id(lens_or_fn.reverse_function)
        return a if (a is not None and a == b) else None
    poly = getattr(lens_or_fn, "pb_lens_polynomial", None)
    if poly is not None:
        return _native.lens_polynomial(poly[:4], poly[4])
    return getattr(lens_or_fn, "pb_lens_id", None)


def _tag(name):
    def deco(fn):
        fn.pb_lens_id = LENS_IDS[name]
        fn.pb_lens_name = name
        return fn

    return deco


# -- equidistant (lens.py:148-187) ----------------------------------------------
@_tag("equidistant")
def _equidistant(theta):
    return theta


@_tag("equidistant")
def _equidistant_inverse(r):
    return r


# -- equisolid (lens.py:191-243) -------------------------------------------------
@_tag("equisolid")
def _equisolid(theta):
    return 2 * np.sin(theta / 2.0)


@_tag("equisolid")
def _equisolid_inverse(r):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        theta = 2.0 * np.arcsin(r / 2.0)
    if isinstance(theta, float):
        return 0.0 if np.isnan(theta) else theta
    theta[np.isnan(theta)] = 0.0  # outside the image circle -> 0.0, lens.py:219
    return theta


# -- stereographic (lens.py:105-145) ---------------------------------------------
@_tag("stereographic")
def _stereographic(theta):
    return 2.0 * np.tan(theta / 2.0)


@_tag("stereographic")
def _stereographic_inverse(r):
    return 2.0 * np.arctan(r / 2.0)


# -- orthographic (lens.py:247-285) -----------------------------------------------
@_tag("orthographic")
def _orthographic(theta):
    return np.sin(theta)


@_tag("orthographic")
def _orthographic_inverse(r):
    return np.arcsin(r)


# -- rectilinear (lens.py:68-103) --------------------------------------------------
@_tag("rectilinear")
def _rectilinear(theta):
    limit = to_radians(89)
    if isinstance(theta, float):
        if theta < 0:
            raise ValueError("The angle theta cannot be negative")
        if theta > limit:
            raise ValueError("The Rectilinear lens can't handle FoV larger than 179 degrees")
        return np.tan(theta)
    out = np.tan(theta)
    out[np.logical_or(theta < 0, theta > limit)] = np.nan
    return out


@_tag("rectilinear")
def _rectilinear_inverse(r):
    return np.arctan(r)


# -- thoby (lens.py:290-335) --------------------------------------------------------
@_tag("thoby")
def _thoby(theta):
    return 1.47 * np.sin(0.713 * theta)


@_tag("thoby")
def _thoby_inverse(r):
    return np.arcsin(r / 1.47) / 0.713


def rectilinear() -> Lens:
    r"""$f(\theta) = \tan\theta$ (lens.py:341-348)."""
    return Lens(_rectilinear, _rectilinear_inverse)


def equisolid() -> Lens:
    r"""$f(\theta) = 2\sin(\theta/2)$ (lens.py:351-358)."""
    return Lens(_equisolid, _equisolid_inverse)


def equidistant() -> Lens:
    r"""$f(\theta) = \theta$ (lens.py:361-370)."""
    return Lens(_equidistant, _equidistant_inverse)


def orthographic() -> Lens:
    r"""$f(\theta) = \sin\theta$ (lens.py:373-380)."""
    return Lens(_orthographic, _orthographic_inverse)


def stereographic() -> Lens:
    r"""$f(\theta) = 2\tan(\theta/2)$ (lens.py:383-390)."""
    return Lens(_stereographic, _stereographic_inverse)


def thoby() -> Lens:
    r"""$f(\theta) = 1.47\sin(0.713\,\theta)$ (lens.py:393-401)."""
    return Lens(_thoby, _thoby_inverse)


# -- polynomial (Kannala-Brandt): no counterpart in the reference, which accepts it as a Lens of two callables --------------------
_POLY_NEWTON_STEPS = 10  # a constant of the definition (csrc/pb_params.hpp: PB_POLY_NEWTON_STEPS)


def _real_roots(c, lo, hi):
    """Real roots in [lo, hi] of c[0] + c[1] x + ... + c[n] x^n: between consecutive roots of the derivative the polynomial is
    monotonic, so every sign change brackets exactly one root (bisection)."""
    c = list(c)
    while len(c) > 1 and c[-1] == 0.0:
        c.pop()
    if len(c) <= 1:
        return []
    if len(c) == 2:
        r = -c[0] / c[1]
        return [r] if lo <= r <= hi else []

    def f(x):
        v = c[-1]
        for a in c[-2::-1]:
            v = v * x + a
        return v

    pts = sorted([lo] + _real_roots([i * c[i] for i in range(1, len(c))], lo, hi) + [hi])
    roots = []
    for a, b in zip(pts, pts[1:]):
        fa, fb = f(a), f(b)
        if fa == 0.0:
            roots.append(a)
        if not ((fa < 0.0 < fb) or (fb < 0.0 < fa)):
            continue
        for _ in range(200):
            m = 0.5 * (a + b)
            if not a < m < b:
                break
            if (f(m) < 0.0) == (fa < 0.0):
                a = m
            else:
                b = m
        roots.append(0.5 * (a + b))
    if f(hi) == 0.0:
        roots.append(hi)
    return roots


def polynomial(k1: float = 0.0, k2: float = 0.0, k3: float = 0.0, k4: float = 0.0, max_theta: float | None = None) -> Lens:
    r"""The Kannala-Brandt lens a fisheye calibration yields (the ``k1..k4`` of OpenCV's ``fisheye`` module):
    $r(\theta) = \theta + k_1\theta^3 + k_2\theta^5 + k_3\theta^7 + k_4\theta^9$, r in focal-length units.

    THE DEFINITION (float64; every operation rounded on its own, in exactly this nesting - NumPy does so by construction, the device
    under -ffp-contract=off - so host and device, scalar and array agree to the bit).  With ``d = (3.0*k1, 5.0*k2, 7.0*k3, 9.0*k4)``
    computed once and ``t2 = t*t``::

        p(t)  = t * (1.0 + t2*(k1 + t2*(k2 + t2*(k3 + t2*k4))))
        dp(t) =      1.0 + t2*(d1 + t2*(d2 + t2*(d3 + t2*d4)))

    ``max_theta`` (radians, default pi) ends the lens's domain; ``r_max = p(max_theta)``.

    * ``forward_function(theta)`` = ``p(theta)`` where ``theta <= max_theta``, else ``+inf``.
    * ``reverse_function(r)``: where ``r <= r_max``: ``t = r``, then TEN times ``t = t - (p(t) - r) / dp(t)``; elsewhere (NaN included: the
      comparison is false) ``+inf``.  The count is a constant, not data dependent.

    ``+inf`` makes the reference's own rules do the right thing: a destination pixel beyond the image circle has latitude inf > fov / 2
    (invalid), a source direction beyond ``max_theta`` lands at an infinite distance and fails the bounds test (black).  Both callables
    take a Python float (and return one) or an ndarray.  All-zero coefficients give the identity, bit for bit, both ways.

    Raises ``ValueError`` unless: the coefficients are finite; ``0 < max_theta <= pi``; ``dp > 0`` on ``[0, max_theta]`` (decided at the
    real stationary points of the quartic in ``t2`` and at both ends, not on samples - a non-monotonic model folds the image); and ten
    steps do invert ``p``: ``|reverse(forward(theta)) - theta| <= 2**-40`` on a grid of 4097 angles over the domain (a loose bound that
    detects non-convergence; it is no precision claim).

    The callables carry their coefficients: the library evaluates the same definition on the device (PB_LENS_POLYNOMIAL), so the lens runs
    on every route a built-in lens does, in either role."""
    try:
        k = tuple(float(v) for v in (k1, k2, k3, k4))
        mt = float(np.pi if max_theta is None else max_theta)
    except (TypeError, ValueError) as exc:
        raise ValueError(f"polynomial lens: coefficients and max_theta must be real numbers ({exc})") from None
    if not all(np.isfinite(v) for v in k):
        raise ValueError(f"polynomial lens: the coefficients must be finite, got {k}")
    if not (0.0 < mt <= float(np.pi)):
        raise ValueError(f"polynomial lens: max_theta must lie in (0, pi] radians, got {mt!r}")
    d = (3.0 * k[0], 5.0 * k[1], 7.0 * k[2], 9.0 * k[3])

    def p(t):
        t2 = t * t
        return t * (1.0 + t2 * (k[0] + t2 * (k[1] + t2 * (k[2] + t2 * k[3]))))

    def dp(t):
        t2 = t * t
        return 1.0 + t2 * (d[0] + t2 * (d[1] + t2 * (d[2] + t2 * d[3])))

    r_max = p(mt)

    def forward(theta):
        if isinstance(theta, (float, int)):
            theta = float(theta)
            return p(theta) if theta <= mt else float("inf")
        theta = np.asarray(theta, dtype=np.float64)
        with np.errstate(invalid="ignore", over="ignore"):
            ok = theta <= mt
            return np.where(ok, p(np.where(ok, theta, 0.0)), np.inf)

    def reverse(r):
        if isinstance(r, (float, int)):
            r = float(r)
            if not r <= r_max:
                return float("inf")
            t = r
            for _ in range(_POLY_NEWTON_STEPS):
                t = t - (p(t) - r) / dp(t)
            return t
        r = np.asarray(r, dtype=np.float64)
        with np.errstate(invalid="ignore"):
            ok = r <= r_max
        rr = np.where(ok, r, 0.0)
        t = rr
        for _ in range(_POLY_NEWTON_STEPS):
            t = t - (p(t) - rr) / dp(t)
        return np.where(ok, t, np.inf)

    # dp > 0 on [0, max_theta]: q(u) = 1 + d1 u + d2 u^2 + d3 u^3 + d4 u^4 on u = t^2 in [0, max_theta^2], at its stationary points and ends
    big_u = mt * mt
    q = (1.0, d[0], d[1], d[2], d[3])
    at = [0.0] + _real_roots([q[1], 2.0 * q[2], 3.0 * q[3], 4.0 * q[4]], 0.0, big_u) + [big_u]
    if not all(q[0] + u * (q[1] + u * (q[2] + u * (q[3] + u * q[4]))) > 0.0 for u in at):
        raise ValueError(
            f"polynomial lens: r(theta) is not increasing on [0, max_theta = {mt!r} rad] (a non-monotonic model folds the image).  A "
            "calibration holds on the lens's own field only - most real coefficient sets turn over before the default max_theta = pi: "
            "pass max_theta, the largest incidence angle the lens images"
        )
    if not (np.isfinite(r_max) and r_max > 0.0):
        raise ValueError(f"polynomial lens: r(max_theta) = {r_max!r} is not a positive finite number")
    grid = np.arange(4097, dtype=np.float64) * (mt / 4096.0)
    grid[-1] = mt
    with np.errstate(all="ignore"):
        err = np.abs(reverse(forward(grid)) - grid)
    if not bool(np.all(err <= 2.0**-40)):
        raise ValueError("polynomial lens: ten Newton steps from t = r do not invert r(theta) on [0, max_theta]; pass a smaller max_theta")

    for fn in (forward, reverse):
        fn.pb_lens_name = "polynomial"
        fn.pb_lens_polynomial = k + (mt,)
    forward.__name__, reverse.__name__ = "_polynomial", "_polynomial_inverse"
    return Lens(forward, reverse)


__all__ = ["Lens", "equisolid", "equidistant", "rectilinear", "stereographic", "orthographic", "thoby", "polynomial"]
