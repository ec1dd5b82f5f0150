"""Absorbing layers, host side: fenicsxfus_amd.sponge's profiles, and the sub-step and stepper of tests/sponge_ref.py
(the reference of the device tests): second order of the splitting, the exact-scaling identity, sigma = 0."""
import numpy as np
import pytest

import relaxation_ref as rr
import source_ref as sr
import sponge_ref as spr
from fenicsxfus_amd import sponge as sp

C0 = 1500.0


def test_layer_sigma_values_3d():
    lo, hi, L = [0.0, 0.0, 0.0], [0.1, 0.08, 0.06], 0.02
    smax = sp.sigma_max(L, C0, 1e-3, 2)
    assert smax == pytest.approx(3 * C0 * np.log(1e3) / (2 * L), rel=1e-15)
    X = np.array([[0.05, 0.04, 0.03],      # interior
                  [0.10, 0.04, 0.03],      # on the face x+
                  [0.09, 0.04, 0.03],      # half-way into the x+ layer
                  [0.08, 0.04, 0.03],      # where the x+ layer begins
                  [0.00, 0.04, 0.03],      # on x-: left out below
                  [0.10, 0.08, 0.03],      # the edge x+ y+
                  [0.10, 0.08, 0.06],      # the corner x+ y+ z+
                  [0.09, 0.07, 0.03]])     # half-way into both x+ and y+
    th = {f: L for f in sp.FACES if f != "x-"}
    s = sp.layer_sigma(X, lo, hi, th, C0)
    assert np.allclose(s, smax * np.array([0, 1, 0.25, 0, 0, 2, 3, 0.5]), rtol=1e-12, atol=1e-9 * smax)
    assert s[0] == 0.0 and s[3] < 1e-9 * smax and s[4] == 0.0
    # a scalar thickness: every face, x- included
    assert sp.layer_sigma(X, lo, hi, L, C0)[4] == pytest.approx(smax, rel=1e-12)
    # order and reflection enter as the formula says
    s1 = sp.layer_sigma(X[2:3], lo, hi, th, C0, reflection=1e-2, order=1)
    assert s1[0] == pytest.approx(2 * C0 * np.log(1e2) / (2 * L) * 0.5, rel=1e-12)
    # different thicknesses per face
    s2 = sp.layer_sigma(X[[2, 5]], lo, hi, {"x+": 0.02, "y+": 0.01}, C0)
    assert s2[0] == pytest.approx(0.25 * smax, rel=1e-12)
    assert s2[1] == pytest.approx(smax + sp.sigma_max(0.01, C0), rel=1e-12)


def test_layer_sigma_symmetry_2d():
    lo, hi = [-0.03, 0.0], [0.03, 0.05]
    rng = np.random.default_rng(0)
    X = np.column_stack([rng.uniform(lo[0], hi[0], 200), rng.uniform(lo[1], hi[1], 200), np.zeros(200)])
    s = sp.layer_sigma(X, lo, hi, 0.01, C0)
    Xm = X.copy()
    Xm[:, 0] = -X[:, 0]
    assert np.allclose(s, sp.layer_sigma(Xm, lo, hi, 0.01, C0), rtol=1e-12)
    Xm = X.copy()
    Xm[:, 1] = hi[1] - X[:, 1]
    assert np.allclose(s, sp.layer_sigma(Xm, lo, hi, 0.01, C0), rtol=1e-12)
    inner = (np.abs(X[:, 0]) < 0.02) & (X[:, 1] > 0.01) & (X[:, 1] < 0.04)
    assert inner.any() and not s[inner].any() and (s[~inner] > 0).all() and (s >= 0).all()
    # the sum of the per-face profiles
    parts = sum(sp.layer_sigma(X, lo, hi, {f: 0.01}, C0) for f in ("x-", "x+", "y-", "y+"))
    assert np.allclose(s, parts, rtol=1e-14)
    with pytest.raises(ValueError):
        sp.layer_sigma(X, lo, hi, {"z+": 0.01}, C0)


def test_design_reflection_inverts_sigma_max():
    for R in (0.5, 0.1, 1e-3, 1e-6):
        for order in (1, 2, 3):
            for L in (0.006, 0.02):
                assert sp.design_reflection(sp.sigma_max(L, C0, R, order), L, C0, order) == pytest.approx(R, rel=1e-12)
    X = np.array([[0.1, 0.0]])
    smax = sp.layer_sigma(X, [0, 0], [0.1, 0.1], {"x+": 0.02}, C0, reflection=0.1)[0]
    assert sp.design_reflection(smax, 0.02, C0, 2) == pytest.approx(0.1, rel=1e-12)
    assert sp.min_thickness(C0, 0.5e6) == pytest.approx(0.006) and sp.min_thickness(C0, 1e6, 3.0) == pytest.approx(0.0045)


def small_case(orc):
    cs = sr.Case(orc, (2, 2, 2), 2, 0.1)
    x = cs.X[:, 0] / cs.hi[0]
    sigma = np.where(x > 0.4, (0.6 / cs.dt) * (x - 0.4) ** 2 * (1.0 + 0.5 * cs.X[:, 1] / cs.hi[1]), 0.0)
    return cs, sigma


def test_stepper_is_second_order_in_dt(orc):
    """Non-constant sigma (up to 0.3 / dt), R = 2 relaxation, a live start state and the default source over 16 dt: the
    error against 1024 steps falls by 4 per halving of dt (RK4's own error is far below the splitting's)."""
    cs, sigma = small_case(orc)
    rng = np.random.default_rng(3)
    nd = cs.pr.ndofs
    omega = 2 * np.pi * cs.f0 * np.array([0.5, 2.0])
    A = rng.uniform(0.0, 0.3 * 2 * np.pi * cs.f0, (2, nd))
    u0, v0 = rng.standard_normal(nd), 2 * np.pi * cs.f0 * rng.standard_normal(nd)
    T = 16 * cs.dt

    def run(n):
        return spr.stepper(cs, "linear", 0, sigma, A, omega, 6e4, 0.0, T / n, n, u=u0, v=v0)
    fine = run(1024)
    errs = [max(sr.rel(a, b) for a, b in zip(run(n), fine)) for n in (16, 32, 64)]
    rates = np.log2(np.array(errs[:-1]) / np.array(errs[1:]))
    print("sponge stepper: errors", errs, "rates", rates)
    assert errs[0] > 1e-6 and np.all(rates > 1.8) and np.all(rates < 2.2)


@pytest.mark.parametrize("kind", ["linear", "lossy"])
@pytest.mark.parametrize("R", [0, 2])
def test_exact_scaling_identity(orc, kind, R):
    """Constant sigma, no source: the run with the sponge is e^{-sigma N dt} times the run without it."""
    cs, _ = small_case(orc)
    rng = np.random.default_rng(4)
    nd, N = cs.pr.ndofs, 10
    omega = 2 * np.pi * cs.f0 * np.array([0.5, 2.0])[:R]
    A = rng.uniform(0.0, 0.3 * 2 * np.pi * cs.f0, (R, nd))
    u0, v0 = rng.standard_normal(nd), 2 * np.pi * cs.f0 * rng.standard_normal(nd)
    z0 = rng.standard_normal((R, nd))
    s0 = 0.05 / cs.dt
    args = (A, omega, 0.0, 0.0, cs.dt, N)
    plain = spr.stepper(cs, kind, 0, None, *args, u=u0, v=v0, z=z0)
    damped = spr.stepper(cs, kind, 0, np.full(nd, s0), *args, u=u0, v=v0, z=z0)
    f = np.exp(-s0 * N * cs.dt)
    assert 0.5 < f < 0.7
    for a, b in zip(damped[:2 + (R > 0)], plain):
        assert np.abs(b).max() > 0 and sr.rel(a, f * b) < 1e-12


def test_zero_sigma_keeps_every_bit(orc):
    rng = np.random.default_rng(2)
    u, v, z = rng.standard_normal(50), rng.standard_normal(50), rng.standard_normal((2, 50))
    for dtype in (np.float64, np.float32):
        a, b, c = spr.substep(u.astype(dtype), v.astype(dtype), z.astype(dtype), np.zeros(50), 3e-8, dtype=dtype)
        assert a.dtype == b.dtype == c.dtype == dtype
        assert np.array_equal(a, u.astype(dtype)) and np.array_equal(b, v.astype(dtype)) and np.array_equal(c, z.astype(dtype))
    # and the stepper without a sponge is relaxation_ref's, bit for bit; with sigma = 0 too
    cs, _ = small_case(orc)
    omega = 2 * np.pi * cs.f0 * np.array([0.5, 2.0])
    A = np.full((2, cs.pr.ndofs), 0.1 * 2 * np.pi * cs.f0)
    ref = rr.stepper(cs, "linear", 0, A, omega, 6e4, 0.0, cs.dt, 5)
    for sigma in (None, np.zeros(cs.pr.ndofs)):
        got = spr.stepper(cs, "linear", 0, sigma, A, omega, 6e4, 0.0, cs.dt, 5)
        assert all(np.array_equal(x, y) for x, y in zip(got, ref))
