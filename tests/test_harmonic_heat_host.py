"""Per-harmonic heat load, host side (fusmi.h "per-harmonic heat load"): the ABI carries the entry point, the absorption
helpers match their formulas, and the definition a_k = (2 / n^2)(C_k^2 + S_k^2) is the mean square of harmonic k on a
synthetic signal -- before anything on the device is compared with harmonic_heat_ref.py (test_gpu_harmonic_heat.py)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from fenicsxfus_amd import _abi, monitor
from harmonic_heat_ref import accumulate, harmonic_heat, mean_squares, synthetic_signal
from util import Problem

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "fus_thermal_set_heat_from_harmonics"


def test_abi_declares_and_exports_the_symbol():
    hdr = open(os.path.join(ROOT, "include", "fusmi.h")).read()
    declared = set(re.findall(r"\b(fus_[a-z0-9_]+)\s*\(", hdr))
    L = _abi.lib()
    assert NAME in declared and NAME in _abi.SYMBOLS and hasattr(L, NAME)
    # null handles are refused before any device call
    a = np.zeros(4)
    for nharm in (1, 0, 9):
        assert L.fus_thermal_set_heat_from_harmonics(None, None, C.c_int(nharm), None) == -1
        assert L.fus_thermal_set_heat_from_harmonics(None, None, C.c_int(nharm), _abi.ptr(a)) == -1
        assert b"fus_thermal_set_heat_from_harmonics: null" in L.fus_last_error()


def test_power_law_and_thermoviscous_absorption():
    alpha = np.array([0.5, 20.0, 3.0])
    rows = monitor.power_law(alpha, 1.1, 4)
    assert rows.shape == (4, 3) and rows.dtype == np.float64
    for k in range(1, 5):
        assert np.array_equal(rows[k - 1], alpha * float(k) ** 1.1)
    assert np.array_equal(rows[0], alpha)
    y = np.array([1.0, 2.0, 1.3])                                   # per cell
    rows = monitor.power_law(alpha, y, 3)
    assert rows.shape == (3, 3)
    for k in range(1, 4):
        assert np.array_equal(rows[k - 1], alpha * float(k) ** y)
    assert np.array_equal(monitor.power_law(alpha, 2, 3)[2], 9.0 * alpha)
    assert monitor.power_law(0.7, 2.0, 2).shape == (2, 1)           # a scalar alpha: one column
    delta, c, f = np.array([4.3e-6, 1.2e-4]), np.array([1500.0, 2800.0]), 0.5e6
    tv = monitor.thermoviscous_absorption(delta, c, f)
    assert np.array_equal(tv, delta * (2.0 * np.pi * f) ** 2 / (2.0 * c ** 3))
    # the inverse of compute_diffusivity_of_sound (which takes dB/m: Np = dB / 20 ln 10), and the y = 2 law
    from fenicsxfus_amd.utils import compute_diffusivity_of_sound
    back = np.array([compute_diffusivity_of_sound(2 * np.pi * f, ci, ai * 20.0 / np.log(10.0)) for ci, ai in zip(c, tv)])
    assert np.abs(back - delta).max() <= 8 * 2.0 ** -53 * delta.max()
    assert np.abs(monitor.thermoviscous_absorption(delta, c, 3 * f) - monitor.power_law(tv, 2, 3)[2]).max() <= 1e-15 * tv.max() * 9


def test_parseval_on_a_synthetic_signal():
    """x_j = mu + sum_{k <= 3} (A_k cos + B_k sin)(2 pi k f t_j) over two whole periods, 9 samples per period (> 2 * 3):
    the monitor's accumulation rule gives sum_k a_k = rms^2 - mu^2 to 1e-13 relative, and a_k = (A_k^2 + B_k^2) / 2."""
    freq, nharm = 0.5e6, 3
    t, x, mu, A, B = synthetic_signal(np.random.default_rng(7), 13, nharm, freq, periods=2, spp=9)
    n, S, Q, Ck, Sk = accumulate(x, t, freq, nharm)
    assert n == 18
    ak = mean_squares(n, Ck, Sk)
    rms2, mean = Q / n, S / n
    want = rms2 - mean ** 2
    assert want.min() > 0
    assert np.all(np.abs(sum(ak) - want) <= 1e-13 * rms2)            # relative to each DOF's own mean square
    assert np.abs(mean - mu).max() <= 1e-13 * np.abs(x).max()
    for k in range(nharm):
        assert np.abs(ak[k] - 0.5 * (A[k] ** 2 + B[k] ** 2)).max() <= 1e-13 * rms2.max()


def test_equal_absorption_gives_the_rms_load_of_the_zero_mean_signal(orc):
    """With all alpha_k equal the reference load is M(2 alpha / (rho c)) 1 .* rms^2 of the signal minus its mean, the
    rms path's load, to the same bound (heterogeneous alpha, rho, c per cell)."""
    pr = Problem(orc, (3, 2, 2), 2, hi=[0.009, 0.006, 0.006], perturb=0.1)
    nc = pr.mesh.num_cells
    rng = np.random.default_rng(9)
    freq, nharm = 0.5e6, 3
    t, x, mu, A, B = synthetic_signal(rng, pr.ndofs, nharm, freq, periods=2, spp=9)
    n, S, Q, Ck, Sk = accumulate(x - mu, t, freq, nharm)
    alpha = rng.uniform(0.5, 20.0, nc)
    rho, c = rng.uniform(1000.0, 1850.0, nc), rng.uniform(1500.0, 2800.0, nc)
    cos_maps, sin_maps = [2.0 / n * ck for ck in Ck], [2.0 / n * sk for sk in Sk]
    h = harmonic_heat(pr, np.tile(alpha, (nharm, 1)), rho, c, cos_maps, sin_maps)
    rms_load = pr.M(np.ones(pr.ndofs), 2.0 * alpha / (rho * c)) * (Q / n)
    assert rms_load.max() > 0 and np.abs(h - rms_load).max() <= 1e-13 * rms_load.max()
    # and a law that grows with frequency heats more, by harmonics 2 and 3 alone
    more = harmonic_heat(pr, monitor.power_law(alpha, 1.1, nharm), rho, c, cos_maps, sin_maps)
    only1 = harmonic_heat(pr, alpha[None, :], rho, c, cos_maps[:1], sin_maps[:1])
    assert np.all(more > h) and np.all(h > only1)


def test_cpp_example_compiles(tmp_path):
    """examples/cpp_bioheat_harmonics.cpp against include/fusmi.hpp (compile and link only; it runs in the GPU tests)."""
    libdir = os.path.join(ROOT, "fenicsx-fus_amd", "fenicsxfus_amd")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "cpp_bioheat_harmonics.cpp"), "-L", libdir, "-lfusmi",
                           f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib", "-o", str(tmp_path / "cpp_bioheat_harmonics")])
