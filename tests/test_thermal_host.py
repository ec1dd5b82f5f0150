"""Bioheat model, host side: the numpy reference (thermal_ref.py) against closed forms, the power iteration against
a dense eigenvalue, the dose rule's fixed points, and the ABI -- before anything on the device is compared with them
(test_gpu_thermal.py)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from fenicsxfus_amd import _abi
from fenicsxfus_amd.thermal import cem43
from thermal_ref import BONE, TISSUE, Bioheat, box_hi, case, dose, rel
from util import Problem

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["fus_thermal_create", "fus_thermal_destroy", "fus_thermal_init", "fus_thermal_set", "fus_thermal_get",
       "fus_thermal_set_heat", "fus_thermal_set_heat_from_monitor", "fus_thermal_lambda_max", "fus_thermal_steps"]


def test_abi_declares_and_exports_the_thermal_symbols():
    hdr = open(os.path.join(ROOT, "include", "fusmi.h")).read()
    declared = set(re.findall(r"\b(fus_[a-z0-9_]+)\s*\(", hdr))
    L = _abi.lib()
    for s in NEW:
        assert s in declared and s in _abi.SYMBOLS and hasattr(L, s), s
    assert L.fus_version() == 1
    # null arguments are refused before any device call
    out = C.c_void_p()
    assert L.fus_thermal_create(None, None, None, None, None, C.c_double(37.0), C.byref(out)) == -1
    assert b"null" in L.fus_last_error() and not out
    for call in (lambda: L.fus_thermal_init(None), lambda: L.fus_thermal_steps(None, C.c_double(1.0), C.c_int64(1), C.c_double(1.0)),
                 lambda: L.fus_thermal_lambda_max(None, 20, None), lambda: L.fus_thermal_set_heat(None, None, None, 0),
                 lambda: L.fus_thermal_set_heat_from_monitor(None, None, None), lambda: L.fus_thermal_get(None, 0, None, 0),
                 lambda: L.fus_thermal_set(None, 0, None, 0)):
        assert call() == -1
    assert L.fus_thermal_destroy(None) == 0


def test_heat_balance(orc):
    """W = 0, theta_0 = 0, constant h: 1^T K = 0 and RK4 integrates a constant exactly, so m_C . theta_n = n dt sum(h)."""
    cs = case(orc, "C")
    ref = Bioheat(cs.pr, cs.k, cs.rho_c, 0.0)
    n, dt = 7, cs.dt
    th = ref.run(np.zeros(cs.pr.ndofs), dt, n, cs.h)
    total = n * dt * cs.h.sum()
    assert total > 0 and abs(ref.m_c @ th - total) <= 1e-12 * total


def test_perfusion_decay(orc):
    """Uniform theta_0 = 5, uniform coefficients, no heat, any k: K theta = 0, so ten steps give 5 R(-W dt / rho C)^10
    with RK4's stability polynomial R."""
    pr = Problem(orc, (3, 2, 2), 3, hi=box_hi((3, 2, 2)), perturb=0.1)
    ref = Bioheat(pr, TISSUE["k"], TISSUE["rho_c"], TISSUE["w"])
    dt = 2.0 / ref.power_iteration(20)
    z = -TISSUE["w"] * dt / TISSUE["rho_c"]
    R = 1 + z + z**2 / 2 + z**3 / 6 + z**4 / 24
    th = ref.run(np.full(pr.ndofs, 5.0), dt, 10)
    assert R < 1 and np.abs(th - 5.0 * R**10).max() <= 1e-12 * 5.0


def test_diffusion_mode(orc):
    """(8, 2, 2) box, P = 4, uniform tissue, theta_0 = 5 cos(pi x / L): 20 steps of dt = 2 / rho_20 reproduce the decay
    exp(-(k / rho C (pi / L)^2 + W / rho C) t) of that insulated-box eigenmode within 1e-7 (measured: 5.3e-9 at a
    decay factor of 0.934), and the energy theta^T m_C theta has decreased."""
    n = (8, 2, 2)
    hi = box_hi(n)
    pr = Problem(orc, n, 4, hi=hi)
    ref = Bioheat(pr, TISSUE["k"], TISSUE["rho_c"], TISSUE["w"])
    dt = 2.0 / ref.power_iteration(20)
    x = pr.V.tabulate_dof_coordinates()[:, 0]
    th0 = 5.0 * np.cos(np.pi * x / hi[0])
    th = ref.run(th0, dt, 20)
    decay = np.exp(-(TISSUE["k"] / TISSUE["rho_c"] * (np.pi / hi[0]) ** 2 + TISSUE["w"] / TISSUE["rho_c"]) * 20 * dt)
    err = rel(th, th0 * decay)
    print(f"diffusion mode: decay {decay:.4f}, rel err {err:.2e}")
    assert err <= 1e-7
    assert th @ (ref.m_c * th) < th0 @ (ref.m_c * th0)


@pytest.mark.parametrize("label", ["A", "B", "C"])
def test_power_iteration_against_dense(orc, label):
    """The 20-iteration quotient lies in [0.95, 1 + 1e-12] lambda_max of the dense symmetric pencil (measured: 0.977,
    0.973, 0.969), so dt = 2 / rho_20 is inside RK4's limit 2.785 / lambda_max."""
    cs = case(orc, label)
    lam = cs.ref.dense_lambda_max()
    frac = cs.rho20 / lam
    print(f"case {label}: rho_20 / lambda_max = {frac:.4f}")
    assert 0.95 <= frac <= 1 + 1e-12
    assert cs.dt * lam <= 2.785


def test_cem43_fixed_points():
    for T, minutes in ((43.0, 1.0), (44.0, 2.0), (42.0, 0.25), (37.0, 4.0 ** -6)):
        assert cem43([T], 60.0) == minutes
        assert cem43([T - 37.0], 60.0, t_base=37.0) == minutes
        assert dose([np.array([T - 37.0])], 60.0, 37.0)[0] == minutes
    # two steps add; arrays keep their shape
    assert np.array_equal(cem43(np.array([[43.0, 44.0], [43.0, 42.0]]), 60.0), [2.0, 2.25])


def test_materials_are_the_stated_ones(orc):
    """Bone where the cell centroid lies in (0.4, 0.6) of the box along x: two of B's six layers and the middle one of
    D's three; boxes of four or two layers (A, C, E, F) have no centroid there and are tissue throughout."""
    cs = case(orc, "B")
    assert set(np.unique(cs.k)) == {BONE["k"], TISSUE["k"]} and set(np.unique(cs.w)) == {0.0, TISSUE["w"]}
    assert (cs.k == BONE["k"]).sum() == 2 * 5 and np.array_equal(cs.rho_c[cs.k == BONE["k"]], np.full(10, BONE["rho_c"]))
    assert set(np.unique(case(orc, "A").k)) == {TISSUE["k"]}
    assert cs.q.max() > 4e7 and cs.h.min() >= 0


def test_cpp_example_compiles(tmp_path):
    """examples/cpp_bioheat_run.cpp against include/fusmi.hpp (compile and link only; it runs in the GPU tests)."""
    libdir = os.path.join(ROOT, "fenicsx-fus_amd", "fenicsxfus_amd")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "cpp_bioheat_run.cpp"), "-L", libdir, "-lfusmi",
                           f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib", "-o", str(tmp_path / "cpp_bioheat_run")])
