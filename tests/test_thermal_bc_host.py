"""Boundary conditions of the bioheat model, host side (no device): the numpy reference of tests/thermal_bc_ref.py against
closed forms on affine meshes, its power iteration against a dense eigenvalue, the step rule with and without the surface
term, the entry-list header csrc/thermal_bc.hpp through a plain C++ driver under AddressSanitizer + UBSan (a stand-alone
program), and the ABI -- before anything on the device is compared with them (test_gpu_thermal_bc.py)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from fenicsxfus_amd import _abi
from thermal_bc_ref import CONV_X, FIXED, THETA_EXT, BioheatBC, Boundary, cooled_face, face_dofs, face_tags, standard
from thermal_ref import TISSUE, box_hi, case
from util import Problem, live_state

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fenicsx-fus_amd", "csrc")
DRIVER = os.path.join(ROOT, "tests", "cpp", "thermal_bc_driver.cpp")
NEW = ["fus_thermal_set_boundary", "fus_thermal_boundary_info"]
EPS = 2.0 ** -53
AFFINE = [((4, 3, 3), 2), ((4, 3, 3), 3), ((6, 5), 4), ((2, 2, 2), 8)]


# ---- closed forms -------------------------------------------------------------------------------------------------------
def _affine(orc, n, P):
    hi = box_hi(n)
    pr = Problem(orc, n, P, hi=hi, perturb=0.0)
    x = pr.V.tabulate_dof_coordinates()[:, 0].astype(np.float64)
    tags = face_tags(pr.mesh, {FIXED: (0, 0), CONV_X: (0, 1)})
    return pr, hi[0], x, tags


@pytest.mark.parametrize("n,P", AFFINE)
def test_parabola_is_stationary(orc, n, P):
    """Both x faces fixed at 0, uniform q = 1e6, k = 0.5, no perfusion: theta = q x (L - x) / (2 k) is the steady state,
    and it lies in the discrete space, so f = 0 at the free DOFs up to rounding.  Bound: the change of one step of
    dt = 2 / rho_20, max |f| dt, is at most 64 * 2^-53 of max |theta| (the sums behind one entry of K theta have at most
    (P + 1) * 2^tdim * tdim <= 64 * 3 terms whose rounding errors partly cancel; measured: 5e-17 to 2e-16)."""
    pr, L, x, tags = _affine(orc, n, P)
    k, q = 0.5, 1e6
    mask = face_dofs(pr, tags, FIXED) | face_dofs(pr, tags, CONV_X)
    ref = BioheatBC(pr, k, TISSUE["rho_c"], None, fixed=mask, fixed_rise=0.0)
    theta = ref.impose(q * x * (L - x) / (2.0 * k))
    f = ref.f(theta, ref.load(np.full(pr.ndofs, q)))
    dt = 2.0 / ref.power_iteration(20)
    drift = float(np.abs(f).max() * dt / np.abs(theta).max())
    print(f"parabola {n} P={P}: max|f| dt / max|theta| = {drift:.2e}")
    assert mask.any() and not mask.all() and np.array_equal(f[mask], np.zeros(int(mask.sum())))
    assert drift <= 64 * EPS
    # and the check can fail: without the fixed faces the same state is heated everywhere
    free = BioheatBC(pr, k, TISSUE["rho_c"], None)
    assert np.abs(free.f(theta, free.load(np.full(pr.ndofs, q)))).max() * dt / np.abs(theta).max() > 1e-6


@pytest.mark.parametrize("n,P", AFFINE)
def test_linear_profile_is_stationary(orc, n, P):
    """x = lo fixed at 3 K, x = hi convective with h_c = 500 and theta_ext = -17, no heat, no perfusion:
    theta = 3 + s x with s = -h_c (3 - theta_ext) / (k + h_c L) meets -k theta' = h_c (theta - theta_ext) at x = L, so
    f = 0 at the free DOFs; the same bound as for the parabola, 64 * 2^-53 per step."""
    pr, L, x, tags = _affine(orc, n, P)
    k, h_c = 0.5, 500.0
    m_h = pr.facet_diag(tags, CONV_X, np.full(pr.mesh.num_cells, h_c))
    ref = BioheatBC(pr, k, TISSUE["rho_c"], None, fixed=face_dofs(pr, tags, FIXED), fixed_rise=3.0, m_h=m_h,
                    theta_ext=THETA_EXT)
    s = -h_c * (3.0 - THETA_EXT) / (k + h_c * L)
    theta = ref.impose(3.0 + s * x)
    f = ref.f(theta)
    dt = 2.0 / ref.power_iteration(20)
    drift = float(np.abs(f).max() * dt / np.abs(theta).max())
    print(f"linear profile {n} P={P}: slope {s:.1f} K/m, max|f| dt / max|theta| = {drift:.2e}")
    assert drift <= 64 * EPS
    # r enters unscaled by sigma, and the check can fail: another coolant temperature leaves the profile
    assert np.array_equal(ref.f(theta, np.ones(pr.ndofs), 0.0), f)
    other = BioheatBC(pr, k, TISSUE["rho_c"], None, fixed=face_dofs(pr, tags, FIXED), fixed_rise=3.0, m_h=m_h,
                      theta_ext=THETA_EXT + 1.0)
    assert np.abs(other.f(theta)).max() * dt / np.abs(theta).max() > 1e-6


# ---- the operator behind the step ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("label", ["A", "B"])
def test_power_iteration_against_dense(orc, label):
    """Standard boundary: the quotient is a Rayleigh quotient of the reduced operator, so it never exceeds the dense
    lambda_max, and dt = 2 / rho_20 lies inside RK4's limit 2.785 / lambda_max."""
    bd, ref, rho20 = standard(orc, label)
    lam = ref.dense_lambda_max()
    print(f"case {label}: rho_20 / lambda_max = {rho20 / lam:.4f} with the standard boundary")
    assert rho20 <= (1 + 1e-12) * lam
    assert 2.0 / rho20 * lam <= 2.785
    assert ref.start_vector()[bd.mask].max() == 0.0 and bd.mask.any() and (ref.m_h > 0).any()
    assert not (bd.mask & (ref.m_h > 0)).any()                     # fixed wins on the shared edge


@pytest.mark.parametrize("label", ["A", "B", "F"])
def test_convective_faces_raise_lambda(orc, label):
    """Adding the non-negative diagonal m_H cannot lower an eigenvalue of the symmetric pencil; with forced water
    cooling (h_c = 5000) the quotient grows by far more than the power iteration's slack."""
    cs = case(orc, label)
    _, ref, rho20 = cooled_face(orc, label)
    print(f"case {label}: rho_20 {cs.rho20:.4e} insulating, {rho20:.4e} with h_c = 5000; "
          f"dt_ins max(m_H / m_C) = {cs.dt * (ref.m_h / ref.m_c).max():.2f}")
    assert rho20 >= cs.rho20
    refs = standard(orc, label)[1]
    assert BioheatBC(cs.pr, cs.k, cs.rho_c, cs.w, m_h=refs.m_h).power_iteration(20) >= cs.rho20


def test_the_step_rule_must_know_the_boundary(orc):
    """Case A, h_c = 5000 on the face x = hi, coolant at -17 K, live start, no heat: 20 RK4 steps at the insulating
    operator's 2 / rho_20 blow up beyond 1e10, at the boundary operator's 2 / rho_20 they stay below max |theta_0| + 17."""
    cs = case(orc, "A")
    _, ref, rho20 = cooled_face(orc, "A")
    th0 = live_state(cs.prt, 3, 5.0)[0].astype(np.float64)
    bad = ref.run(th0, cs.dt, 20)
    good = ref.run(th0, 2.0 / rho20, 20)
    print(f"max |theta| after 20 steps: {np.abs(bad).max():.2e} at dt {cs.dt:.3e}, {np.abs(good).max():.3f} at {2.0 / rho20:.3e}")
    assert np.abs(bad).max() > 1e10
    assert np.abs(good).max() < np.abs(th0).max() + 17.0


# ---- the ABI ------------------------------------------------------------------------------------------------------------
def test_abi_declares_and_exports_the_boundary_symbols():
    hdr = open(os.path.join(ROOT, "include", "fusmi.h")).read()
    declared = set(re.findall(r"\b(fus_[a-z0-9_]+)\s*\(", hdr))
    L = _abi.lib()
    for s in NEW:
        assert s in declared and s in _abi.SYMBOLS and hasattr(L, s), s
    # null handles are refused before any device call
    assert L.fus_thermal_set_boundary(None, None, None, None, None) == -1
    assert b"null" in L.fus_last_error()
    nf, nc = C.c_int64(-5), C.c_int64(-5)
    assert L.fus_thermal_boundary_info(None, C.byref(nf), C.byref(nc)) == -1
    assert b"null" in L.fus_last_error() and nf.value == -5 and nc.value == -5


def test_cpp_example_compiles(tmp_path):
    """examples/cpp_bioheat_bc.cpp against include/fusmi.hpp (compile and link only; it runs in the GPU tests)."""
    libdir = os.path.join(ROOT, "fenicsx-fus_amd", "fenicsxfus_amd")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "cpp_bioheat_bc.cpp"), "-L", libdir, "-lfusmi",
                           f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib", "-o", str(tmp_path / "cpp_bioheat_bc")])


# ---- the entry lists ----------------------------------------------------------------------------------------------------
def _lists(perm, fixed, rise, diag, ext, t):
    """numpy mirror of thermal_bc_lists: (fix_idx, fix_val, conv_idx, hw, r)."""
    n = len(perm)
    fx = np.zeros(n, bool) if fixed is None else fixed != 0
    cv = np.zeros(n, bool) if diag is None else (diag > 0) & ~fx
    fo, co = np.argsort(perm[fx]), np.argsort(perm[cv])
    fval = (np.zeros(n, t) if rise is None else rise)[fx][fo]
    hw = (np.zeros(n, t) if diag is None else diag)[cv][co]
    r = np.zeros(len(hw), t) if ext is None else (hw.astype(np.float64) * ext[cv][co].astype(np.float64)).astype(t)
    return perm[fx][fo], fval, perm[cv][co], hw, r


def _drive(exe, path, perm, fixed, rise, diag, ext, t):
    with open(path, "wb") as f:
        np.array([len(perm), 8 * np.dtype(t).itemsize] + [int(a is not None) for a in (fixed, rise, diag, ext)],
                 dtype=np.int64).tofile(f)
        perm.astype(np.int32).tofile(f)
        if fixed is not None:
            fixed.astype(np.uint8).tofile(f)
        for a in (rise, diag, ext):
            if a is not None:
                np.ascontiguousarray(a, dtype=t).tofile(f)
    out = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert out.returncode == 0 and out.stderr == "", out.stdout + out.stderr
    rows = [ln.split() for ln in out.stdout.splitlines()]
    err = int(rows[0][1])
    if err:
        assert rows[1][:2] == ["untouched", "1"], rows[1]
        return err, " ".join(rows[1][3:])
    nf, nc = int(rows[1][1]), int(rows[1][3])
    F, Cc = rows[2:2 + nf], rows[2 + nf:]
    assert len(Cc) == nc and all(w[0] == "F" for w in F) and all(w[0] == "C" for w in Cc)
    hexes = lambda ws, j: np.array([float.fromhex(w[j]) for w in ws]).astype(t)   # noqa: E731
    ints = lambda ws: np.array([int(w[1]) for w in ws], dtype=np.int64)           # noqa: E731
    return 0, (ints(F), hexes(F, 2), ints(Cc), hexes(Cc, 2), hexes(Cc, 3))


@pytest.mark.parametrize("t", [np.float64, np.float32])
def test_entry_lists_under_sanitizers(tmp_path, t):
    """csrc/thermal_bc.hpp as a stand-alone program under AddressSanitizer + UBSan (never loaded into python): the lists
    equal numpy's -- ascending unique internal indices, fixed over convective, zero entries dropped, r = hw * theta_ext
    formed in double and rounded once -- for every combination of absent arrays, and every argument error is reported
    with the output lists untouched."""
    exe = str(tmp_path / "thermal_bc_driver")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-O1", "-g", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", CSRC, DRIVER, "-o", exe])
    rng = np.random.default_rng(7)
    n = 203
    perm = rng.permutation(n + 13)[:n].astype(np.int32)            # injective into a padded internal range
    fixed = (rng.random(n) < 0.2).astype(np.uint8) * rng.integers(1, 255, n).astype(np.uint8)
    rise = rng.standard_normal(n).astype(t)
    diag = np.where(rng.random(n) < 0.4, rng.uniform(0.1, 3.0, n), 0.0).astype(t)
    diag[:3] = -0.0                                                 # minus zero is zero: dropped, not refused
    ext = rng.uniform(-20.0, 5.0, n).astype(t)
    assert ((fixed != 0) & (diag > 0)).any() and ((fixed == 0) & (diag > 0)).any()
    path = tmp_path / "in.bin"
    for use in range(16):
        f_, r_, d_, e_ = (a if use >> i & 1 else None for i, a in enumerate((fixed, rise, diag, ext)))
        err, got = _drive(exe, path, perm, f_, r_, d_, e_, t)
        if e_ is not None and d_ is None:
            assert err == 4 and "conv_rise given without conv_diag" in got
            continue
        assert err == 0, (use, got)
        ref = _lists(perm, f_, r_, d_, e_, t)
        for g, r in zip(got, ref):
            assert g.shape == r.shape and np.array_equal(g, r), use
        for idx in (got[0], got[2]):
            assert (np.diff(idx) > 0).all()
        assert not set(got[0]) & set(got[2])
    # the argument errors; values that are never read may be anything
    free = np.flatnonzero((fixed == 0) & (diag > 0))[0]
    held = np.flatnonzero(fixed != 0)[0]
    idle = np.flatnonzero((fixed == 0) & (diag == 0))[5]

    def broken(a, i, v):
        b = a.copy()
        b[i] = v
        return b

    for v in (-1.0, np.nan, np.inf):
        for i in (free, held):
            assert _drive(exe, path, perm, fixed, rise, broken(diag, i, v), ext, t)[0] == 1
    for v in (np.nan, -np.inf):
        assert _drive(exe, path, perm, fixed, broken(rise, held, v), diag, ext, t)[0] == 2
        assert _drive(exe, path, perm, fixed, rise, diag, broken(ext, free, v), t)[0] == 3
        assert _drive(exe, path, perm, fixed, broken(rise, free, v), diag, broken(ext, idle, v), t)[0] == 0
    assert _drive(exe, path, perm, None, None, None, ext, t)[0] == 4
    # nothing set at all: empty lists
    err, got = _drive(exe, path, perm, None, None, None, None, t)
    assert err == 0 and all(len(g) == 0 for g in got)


def test_boundary_helper_matches_its_description(orc):
    """The standard boundary of case B: a fixed face, two convective faces that add on their common corner, bone cells
    with their own h_c, and the fixed face winning the corner it shares with y = lo."""
    cs = case(orc, "B")
    bd, ref, _ = standard(orc, "B")
    X = cs.prt.V.tabulate_dof_coordinates()[:, :2]
    lo_x, hi_x, lo_y = X[:, 0] < 1e-12, X[:, 0] > cs.hi[0] - 1e-12, X[:, 1] < 1e-12
    assert np.array_equal(bd.mask, lo_x)
    assert np.array_equal(ref.m_h > 0, (hi_x | lo_y) & ~lo_x)
    assert np.abs(ref.fixed_rise[lo_x] - (2.0 + np.sin(40.0 * X[lo_x, 1]))).max() <= 1e-14   # through 37 + rise - 37
    corner = hi_x & lo_y
    one = Boundary(cs, {CONV_X: (0, 1)}, convective={CONV_X: (500.0, THETA_EXT)}).m_h
    assert corner.sum() == 1 and ref.m_h[corner][0] > one[corner][0] > 0
    assert np.allclose(ref.r[ref.m_h > 0] / ref.m_h[ref.m_h > 0], THETA_EXT)
