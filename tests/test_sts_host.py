"""Super-time-stepping of the bioheat model, host side (no device): the RKL2 recurrence of tests/sts_ref.py against what
the scheme promises (stability interval, second order, heat balance), the coefficient header csrc/sts_coef.hpp through a
plain C++ driver under AddressSanitizer + UBSan (a stand-alone program), its numpy mirror
``thermal.rkl2_coefficients``, and the ABI -- before anything on the device is compared with them (test_gpu_sts.py)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import sts_ref
from fenicsxfus_amd import _abi
from fenicsxfus_amd.thermal import rkl2_coefficients
from thermal_ref import Bioheat, case, rel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fenicsx-fus_amd", "csrc")
DRIVER = os.path.join(ROOT, "tests", "cpp", "sts_coef_driver.cpp")
STAGES = (2, 3, 4, 8, 9, 16, 32)
NEW = ["fus_thermal_steps_sts", "fus_thermal_stable_dt"]


# ---- the scalar polynomial ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", STAGES)
def test_stability_interval(s):
    """max |R| <= 1 on 20001 points of [-beta_s, 0]; at 1.02 beta_s an even s has left the unit disc."""
    z = np.linspace(-sts_ref.beta(s), 0.0, 20001)
    worst = float(np.abs(sts_ref.polynomial(s, z)).max())
    print(f"s = {s}: max |R| on [-beta_s, 0] = {worst:.15f}")
    assert worst <= 1.0 + 1e-12
    if s % 2 == 0:
        assert abs(sts_ref.polynomial(s, -1.02 * sts_ref.beta(s))) > 1.0


@pytest.mark.parametrize("s", STAGES)
def test_polynomial_matches_the_exponential_to_second_order(s):
    for z in (1e-3, -1e-3):
        assert abs(sts_ref.polynomial(s, z) - (1.0 + z + 0.5 * z * z)) <= abs(z) ** 3
    # and not to third order's constant 1/6 by accident of a wrong recurrence: the z^3 term is bounded but not zero
    r = [(sts_ref.polynomial(s, z) - (1.0 + z + 0.5 * z * z)) / z ** 3 for z in (-1e-2, -2e-2)]
    assert abs(r[0] - r[1]) <= 0.05 * abs(r[0]) + 1e-9


# ---- on the meshes ------------------------------------------------------------------------------------------------------
def test_second_order_on_case_b(orc):
    """s = 6 from a zero start with the heat on, total time four steps of stable_dt(6), against RK4 at an eighth of that
    step: with n = 4, 8, 16 steps the error falls by a factor in [3.5, 4.6] per halving (measured: 4.32 and 4.14)."""
    cs = case(orc, "B")
    dt = sts_ref.stable_dt(cs.rho20, 6)
    zero = np.zeros(cs.pr.ndofs)
    fine = cs.ref.run(zero, dt / 8.0, 32, cs.h)
    err = [rel(sts_ref.run(cs.ref, zero, 4.0 * dt / n, n, 6, cs.h), fine) for n in (4, 8, 16)]
    print(f"case B, s = 6: errors {err[0]:.3e} {err[1]:.3e} {err[2]:.3e}, ratios {err[0] / err[1]:.2f} {err[1] / err[2]:.2f}")
    assert np.abs(fine).max() > 0
    for a, b in zip(err[:-1], err[1:]):
        assert 3.5 <= a / b <= 4.6


@pytest.mark.parametrize("s", [2, 8])
def test_heat_balance(orc, s):
    """W = 0, theta_0 = 0, constant h: 1^T K = 0 and the scheme is consistent (mu_j + nu_j + (1 - mu_j - nu_j) = 1 and
    R'(0) = 1), so m_C . theta_9 = 9 dt sum(h)."""
    cs = case(orc, "C")
    ref = Bioheat(cs.pr, cs.k, cs.rho_c, 0.0)
    n, dt = 9, sts_ref.stable_dt(cs.rho20, s)
    th = sts_ref.run(ref, np.zeros(cs.pr.ndofs), dt, n, s, cs.h)
    total = n * dt * cs.h.sum()
    assert total > 0 and abs(ref.m_c @ th - total) <= 1e-12 * total


def test_trapezoid_dose_fixed_points():
    """A constant 43 degrees for a minute is one minute; 44 and 42 at the two ends of a minute average 2 and 1/4."""
    at = lambda T: np.array([T - 37.0])   # noqa: E731
    assert sts_ref.dose_trapezoid([at(43.0), at(43.0)], 60.0, 37.0)[0] == 1.0
    assert sts_ref.dose_trapezoid([at(44.0), at(42.0)], 60.0, 37.0)[0] == 0.5 * (2.0 + 0.25)
    assert sts_ref.dose_trapezoid([at(43.0), at(43.0), at(44.0)], 60.0, 37.0)[0] == 1.0 + 1.5


# ---- the coefficients ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", range(2, 33))
def test_python_coefficients_equal_the_reference(s):
    got, ref = rkl2_coefficients(s), sts_ref.coefficients(s)
    for g, r in zip(got, ref):
        assert g.dtype == np.float64 and g.shape == (s + 1,) and np.array_equal(g, r)
    mu, nu, mut, gat = got
    assert mu[2:].min() > 0 and nu[2:].max() < 0 and mut[1:].min() > 0 and gat[2:].max() < 0
    for bad in (1, 0, -1, 33):
        with pytest.raises(ValueError, match="stages"):
            rkl2_coefficients(bad)


def test_coefficient_header_under_sanitizers(tmp_path):
    """csrc/sts_coef.hpp as a stand-alone program under AddressSanitizer + UBSan (never loaded into python): the
    coefficients for s = 2..32 equal numpy's to the last bit, the run is clean, s = 1 and s = 33 are refused."""
    exe = str(tmp_path / "sts_coef_driver")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-O1", "-g", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", CSRC, DRIVER, "-o", exe])
    out = subprocess.run([exe, "2", "32"], capture_output=True, text=True)
    assert out.returncode == 0 and out.stderr == "", out.stderr
    rows = [ln.split() for ln in out.stdout.splitlines()]
    assert len(rows) == sum(range(2, 33))
    seen = set()
    for w in rows:
        s, j = int(w[0]), int(w[1])
        ref = sts_ref.coefficients(s)
        for k in range(4):
            assert float.fromhex(w[2 + k]) == ref[k][j], (s, j, k)
        assert float.fromhex(w[6]) == sts_ref.beta(s)
        seen.add((s, j))
    assert seen == {(s, j) for s in range(2, 33) for j in range(1, s + 1)}
    for bad in ("1", "33"):
        out = subprocess.run([exe, bad, bad], capture_output=True, text=True)
        assert out.returncode == 2 and out.stdout == "" and out.stderr == ""


# ---- the ABI ------------------------------------------------------------------------------------------------------------
def test_abi_declares_and_exports_the_sts_symbols():
    hdr = open(os.path.join(ROOT, "include", "fusmi.h")).read()
    declared = set(re.findall(r"\b(fus_[a-z0-9_]+)\s*\(", hdr))
    L = _abi.lib()
    for s in NEW:
        assert s in declared and s in _abi.SYMBOLS and hasattr(L, s), s
    # null handles are refused before any device call
    assert L.fus_thermal_steps_sts(None, C.c_double(1.0), C.c_int64(1), C.c_double(1.0), C.c_int(8)) == -1
    assert b"null" in L.fus_last_error()
    out = C.c_double(-5.0)
    assert L.fus_thermal_stable_dt(None, C.c_int(20), C.c_int(8), C.byref(out)) == -1
    assert b"null" in L.fus_last_error() and out.value == -5.0
