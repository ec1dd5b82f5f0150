"""Relaxation absorption, host side: the sub-step of tests/relaxation_ref.py (the reference of the device tests) against
the exact flow of its local system, its energy, and fenicsxfus_amd.absorption's dispersion relation and power-law fit."""
import numpy as np
import scipy.linalg

import relaxation_ref as rr
from fenicsxfus_amd import absorption as ab


def local_matrix(A, omega):
    """d/dt (v, z_1..z_R) = L (v, z): v' = -sum A_nu (v - w_nu z_nu), z_nu' = v - w_nu z_nu."""
    R = len(A)
    L = np.zeros((R + 1, R + 1))
    L[0, 0] = -np.sum(A)
    for k in range(R):
        L[0, 1 + k] = A[k] * omega[k]
        L[1 + k, 0] = 1.0
        L[1 + k, 1 + k] = -omega[k]
    return L


def test_substep_converges_at_second_order():
    A, omega = np.array([3.0e5, 8.0e4, 2.0e5]), 2 * np.pi * np.array([0.3e6, 1.0e6, 3.0e6])
    x0 = np.array([1.0, 2.0e-7, -1.0e-7, 0.5e-7])
    T = 4.0e-7
    exact = scipy.linalg.expm(T * local_matrix(A, omega)) @ x0
    errs = []
    for n in (8, 16, 32, 64):
        v, z = np.array([x0[0]]), x0[1:, None].copy()
        for _ in range(n):
            v, z = rr.substep(v, z, A[:, None], omega, T / n)
        errs.append(np.abs(np.concatenate([v, z[:, 0]]) - exact).max())
    rates = np.log2(np.array(errs[:-1]) / np.array(errs[1:]))
    print("relaxation sub-step: errors", errs, "rates", rates)
    assert errs[-1] < 1e-4 * np.abs(exact).max()
    assert np.all(rates > 1.9) and np.all(rates < 2.1)


def test_energy_never_grows():
    """1000 random sub-steps on 64 DOFs, h w_nu up to 50 (far past any explicit limit): E per DOF is non-increasing,
    up to the rounding of the update itself (a few ulps of E)."""
    rng = np.random.default_rng(5)
    omega = 2 * np.pi * np.array([0.25e6, 1.0e6, 4.0e6])
    A = rng.uniform(0.0, 4e5, (3, 64))
    A[:, :8] = 0.0
    v, z = rng.standard_normal(64), 1e-7 * rng.standard_normal((3, 64))
    hs = np.concatenate([[50.0 / omega[0], 50.0 / omega[2]], 10.0 ** rng.uniform(-10, -5, 998)])
    worst = -np.inf
    for h in hs:
        E0 = rr.energy(v, z, A, omega)
        v, z = rr.substep(v, z, A, omega, h)
        E1 = rr.energy(v, z, A, omega)
        worst = max(worst, float(((E1 - E0) / np.maximum(E0, np.finfo(np.float64).tiny)).max()))
    print(f"relaxation energy: largest relative growth in one sub-step {worst:.3e}")
    assert worst <= 16 * np.finfo(np.float64).eps


def test_alpha_limits():
    fr, a, c = np.array([0.3e6, 2.0e6]), np.array([4.0e3, 9.0e4]), 1500.0
    wn = 2 * np.pi * fr
    # high frequency: alpha -> sum a_nu / (2 c), speed -> c
    f = 1e10
    assert abs(ab.relaxation_alpha(f, fr, a, c) / (a.sum() / (2 * c)) - 1) < 1e-4
    assert abs(ab.relaxation_speed(f, fr, a, c) / c - 1) < 1e-6
    # low frequency: alpha -> w^2 sum (a_nu / w_nu^2) / (2 c_low (1 + sum a_nu / w_nu)), speed -> c_low
    f = 10.0
    w = 2 * np.pi * f
    q = 1.0 + (a / wn).sum()
    c_low = c / np.sqrt(q)
    assert abs(ab.relaxation_speed(f, fr, a, c) / c_low - 1) < 1e-8
    assert abs(ab.relaxation_alpha(f, fr, a, c) / (w * w * (a / wn**2).sum() / (2 * c_low * q)) - 1) < 1e-6
    # weak absorption: the closed form in between
    f = np.array([0.5e6, 1e6, 2e6])
    w = 2 * np.pi * f[:, None]
    approx = (a * w * w / (wn**2 + w * w)).sum(axis=1) / (2 * c)
    assert np.all(np.abs(ab.relaxation_alpha(f, fr, a, c) / approx - 1) < 0.02)


def test_fit_power_law():
    f2, a2, e2 = ab.fit_power_law(5, 1.1, 0.25e6, 4e6, 1500)
    f3, a3, e3 = ab.fit_power_law(5, 1.1, 0.25e6, 4e6, 1500, nrelax=3)
    print(f"fit_power_law: max relative error {e2:.4f} (two processes), {e3:.4f} (three)")
    assert len(f2) == len(a2) == 2 and len(f3) == len(a3) == 3
    assert f2[0] == 0.25e6 and f2[-1] == 4e6 and np.all(a2 >= 0) and np.all(a3 >= 0)
    assert e2 < 0.1
    assert e3 < e2
    f = np.geomspace(0.25e6, 4e6, 64)
    assert np.abs(ab.relaxation_alpha(f, f2, a2, 1500) / (5 * (f / 1e6) ** 1.1) - 1).max() == e2


def test_zero_strength_leaves_v_alone():
    rng = np.random.default_rng(2)
    v, z = rng.standard_normal(50), rng.standard_normal((2, 50))
    for dtype in (np.float64, np.float32):
        vp, zp = rr.substep(v.astype(dtype), z.astype(dtype), np.zeros((2, 50)), [1e6, 2e7], 3e-8, dtype=dtype)
        assert vp.dtype == dtype and np.array_equal(vp, v.astype(dtype))
        assert not np.array_equal(zp, z.astype(dtype))      # the memory variables still follow v
