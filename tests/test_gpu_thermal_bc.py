"""Fixed-temperature and convective boundaries of the bioheat model on the device (fusmi.h "bioheat",
fus_thermal_set_boundary; fenicsxfus_amd.thermal) against the numpy reference of thermal_bc_ref.py, which
test_thermal_bc_host.py pins to closed forms first.

(1) the RK4 stepper; (2) RKL2; (3) closed forms; (4) lambda_max and stable_dt; (5) cooling and duty cycle; (6) nothing
changes when nothing is set, and the launch counts; (7) life cycle and arguments; (8) the C++ example."""
import os
import subprocess

import numpy as np
import pytest

import fenicsxfus_amd as fa
import sts_ref
import test_gpu_thermal as plain          # its wave-model helper (imported as a module: no test is collected twice)
from thermal_bc_ref import CONV_X, FIXED, THETA_EXT, Boundary, cooled_face, standard
from thermal_ref import TISSUE, case, rel
from util import live_state

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL64, TOL32 = 1e-10, 1e-5          # BASELINE section 3: 20 RK4 steps in fp64 / fp32


def tol(cs):
    return TOL64 if cs.dtype == np.float64 else TOL32


def start(cs, seed=3, amp=5.0):
    """A rise that is live at every DOF, in the case's scalar type (returned in double too)."""
    u = live_state(cs.prt, seed, amp)[0].astype(cs.dtype)
    return u, u.astype(np.float64)


def fresh(cs, bd=None, th0=None):
    ctx = fa.Context(0, deterministic=True)
    th = cs.model(fa, ctx)
    if bd is not None:
        bd.apply(th)
    if th0 is not None:
        th.set_state(rise=th0)
    return ctx, th


def held(cs, bd):
    """The values the library holds at the fixed DOFs, in the case's scalar type."""
    return bd.rise[bd.mask].astype(cs.dtype)


def pull(th):
    return th.rise().x.array.copy(), th.dose().x.array.copy()


# ---- (1) stepper ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("label", ["A", "B", "E", "F"])
def test_stepper_against_the_reference(orc, label):
    """Standard boundary, live start, heat on, 20 steps of dt = 2 / rho_20 of the boundary operator: fp64 within 1e-10 of
    the reference in the max norm, fp32 within 1e-5 of the double reference on the float-rounded inputs.  The fixed DOFs
    hold their values exactly after every call; twenty calls of one step and one call of twenty steps give the same bits
    in theta and D, and so do two fresh objects."""
    cs = case(orc, label)
    bd, ref, rho20 = standard(orc, label)
    dt = 2.0 / rho20
    th0, th0d = start(cs)
    want = ref.run(ref.impose(th0d), dt, 20, cs.h)
    insulating = cs.ref.run(th0d, dt, 20, cs.h)
    ctx, th = fresh(cs, bd, th0)
    assert np.array_equal(th.rise().x.array[bd.mask], held(cs, bd))
    for _ in range(20):
        th.steps(dt, 1)
        assert np.array_equal(th.rise().x.array[bd.mask], held(cs, bd))
    got, D = pull(th)
    th.close(), ctx.close()
    err = rel(got, want)
    print(f"case {label}: rel err after 20 steps {err:.3e} (dt = {dt:.4e} s; boundary against insulating: "
          f"{rel(want, insulating):.3e})")
    assert got.dtype == cs.dtype and D.dtype == np.float64
    assert err <= tol(cs)
    assert rel(want, insulating) > 1e-3                          # the boundary is visible
    for _ in range(2):
        ctx, th = fresh(cs, bd, th0)
        th.steps(dt, 20)
        again, D2 = pull(th)
        th.close(), ctx.close()
        assert np.array_equal(got, again) and np.array_equal(D, D2) and D.min() > 0


# ---- (2) RKL2 ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stages", [2, 8])
@pytest.mark.parametrize("label", ["A", "F"])
def test_rkl2_against_the_reference(orc, label, stages):
    """5 steps at 0.72 beta_s / rho_20 of the boundary operator against sts_ref.run on BioheatBC, same tolerances
    (s = 2 is the aliasing corner of the stage rotation); the fixed DOFs hold their values exactly."""
    cs = case(orc, label)
    bd, ref, rho20 = standard(orc, label)
    dt = sts_ref.stable_dt(rho20, stages)
    th0, th0d = start(cs)
    want = sts_ref.run(ref, ref.impose(th0d), dt, 5, stages, cs.h)
    ctx, th = fresh(cs, bd, th0)
    th.steps(dt, 5, stages=stages)
    got, D = pull(th)
    th.close(), ctx.close()
    err = rel(got, want)
    print(f"case {label}, s = {stages}: rel err after 5 steps {err:.3e} (dt = {dt:.4e} s)")
    assert err <= tol(cs)
    assert np.array_equal(got[bd.mask], held(cs, bd)) and D.min() > 0
    assert rel(want, sts_ref.run(cs.ref, th0d, dt, 5, stages, cs.h)) > 1e-3


# ---- (3) closed forms -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["parabola", "linear"])
def test_closed_forms_stay_put(orc, form):
    """Case C (affine), k = 0.5, no perfusion.  Parabola: both x faces fixed at 0, uniform q = 1e6,
    theta = q x (L - x) / (2 k).  Linear profile: x = lo fixed at 3 K, x = hi convective with h_c = 500 and
    theta_ext = -17, theta = 3 + s x, s = -h_c (3 - theta_ext) / (k + h_c L).  Both are steady states in the discrete
    space: max |theta_n - theta_0| <= 1e-10 max |theta_0| over 20 RK4 steps and over 5 RKL2 steps of 8 stages."""
    cs = case(orc, "C")
    pr, L, k = cs.prt, cs.hi[0], 0.5
    x = pr.V.tabulate_dof_coordinates()[:, 0].astype(np.float64)
    faces = {FIXED: (0, 0), CONV_X: (0, 1)}
    if form == "parabola":
        bd = Boundary(cs, faces, fixed={FIXED: 0.0, CONV_X: 0.0})
        q, th0 = np.full(pr.ndofs, 1e6), 1e6 * x * (L - x) / (2.0 * k)
    else:
        bd = Boundary(cs, faces, fixed={FIXED: 3.0}, convective={CONV_X: (500.0, THETA_EXT)})
        q, th0 = None, 3.0 + (-500.0 * (3.0 - THETA_EXT) / (k + 500.0 * L)) * x
    ctx = fa.Context(0, deterministic=True)
    th = fa.BioheatSpectralExplicit(pr.mesh, cs.P, k, TISSUE["rho_c"], None, V=pr.V, ctx=ctx)
    bd.apply(th)
    th.set_heat(q)
    for stages, n in ((0, 20), (8, 5)):
        th.set_state(rise=th0)
        start_ = th.rise().x.array.copy()
        th.steps(th.stable_dt(stages), n, stages=stages)
        drift = float(np.abs(th.rise().x.array - start_).max() / np.abs(start_).max())
        print(f"{form}, stages = {stages}: drift over {n} steps {drift:.2e}")
        assert drift <= 1e-10
    # the check can fail: with the boundary cleared the same start moves
    th.clear_boundary()
    th.set_state(rise=th0)
    th.steps(th.stable_dt(), 20)
    assert np.abs(th.rise().x.array - th0).max() > 1e-6 * np.abs(th0).max()
    th.close(), ctx.close()


# ---- (4) lambda_max and stable_dt -------------------------------------------------------------------------------------
@pytest.mark.parametrize("label", ["A", "B", "F"])
def test_lambda_max(orc, label):
    """Against BioheatBC.power_iteration at the tolerance test_gpu_thermal.py::test_lambda_max uses for the label; with
    h_c = 5000 on a face, 20 steps at stable_dt() from a live start without heat stay below max |theta_0| + 17."""
    cs = case(orc, label)
    bd, ref, rho20 = standard(orc, label)
    ctx, th = fresh(cs, bd)
    lam, dt, lam3 = th.lambda_max(20), th.stable_dt(), th.lambda_max(3)
    dt8 = th.stable_dt(8)
    th.close(), ctx.close()
    print(f"case {label}: lambda_max(20) {lam:.6e} against {rho20:.6e} (insulating: {cs.rho20:.6e})")
    assert abs(lam - rho20) <= tol(cs) * rho20
    assert abs(dt - 2.0 / rho20) <= tol(cs) * dt and abs(dt8 - sts_ref.stable_dt(rho20, 8)) <= tol(cs) * dt8
    assert abs(lam3 - ref.power_iteration(3)) <= tol(cs) * lam3
    cold, cref, crho = cooled_face(orc, label)
    th0, th0d = start(cs)
    ctx, th = fresh(cs, cold, th0)
    th.set_heat(None)
    dtc = th.stable_dt()
    th.steps(dtc, 20)
    got = th.rise().x.array.astype(np.float64)
    th.close(), ctx.close()
    print(f"case {label}: h_c = 5000: stable_dt {dtc:.4e} (insulating {cs.dt:.4e}), max |theta| {np.abs(got).max():.3f}")
    assert abs(dtc - 2.0 / crho) <= tol(cs) * dtc and dtc < cs.dt
    assert np.abs(got).max() < np.abs(th0d).max() + 17.0
    assert rel(got, cref.run(th0d, dtc, 20)) <= tol(cs)


# ---- (5) cooling and duty ---------------------------------------------------------------------------------------------
def test_cooling_and_duty(orc):
    """heat_scale = 0 with the coolant on follows the reference, whose r is not scaled by sigma; a duty cycle of two
    segments does too."""
    cs = case(orc, "A")
    bd, ref, rho20 = standard(orc, "A")
    dt = 2.0 / rho20
    th0, th0d = start(cs)
    ctx, th = fresh(cs, bd, th0)
    th.steps(dt, 10, heat_scale=0.0)
    got = th.rise().x.array.copy()
    want = ref.run(ref.impose(th0d), dt, 10, cs.h, 0.0)
    assert rel(got, want) <= TOL64
    # a coolant switched off with the beam would show: the reference without r, and the one without the boundary
    no_r = bd.ref(cs)
    no_r.r[:] = 0.0
    assert rel(no_r.run(ref.impose(th0d), dt, 10), want) > 1e-3
    th.set_state(rise=th0)
    want = ref.impose(th0d)
    for sigma in (1.0, 0.5):
        th.steps(dt, 5, heat_scale=sigma)
        want = ref.run(want, dt, 5, cs.h, sigma)
    got = th.rise().x.array.copy()
    th.close(), ctx.close()
    assert rel(got, want) <= TOL64
    assert rel(ref.run(ref.impose(th0d), dt, 10, cs.h, 1.0), want) > 1e-3   # the segments' heat scales are visible


# ---- (6) nothing changes when nothing is set --------------------------------------------------------------------------
def _counted(cs, th0, dt, prepare, rk4_steps, sts_steps=0, stages=0):
    ctx, th = fresh(cs)
    prepare(th)
    th.set_state(rise=th0)
    ctx.profile_enable(True)
    th.steps(dt, rk4_steps)
    if sts_steps:
        th.steps(dt, sts_steps, stages=stages)
    counts = {name: ctx.profile_get(name)[1] for name in ("thermal", "thermal_sts", "thermal_bc")}
    out = pull(th)
    th.close(), ctx.close()
    return out, counts


def test_nothing_changes_when_nothing_is_set(orc):
    """Case A, 20 steps: an object that never had a boundary, one that set the standard boundary and cleared it, and one
    that was given all-zero arrays hold identical bits in theta and D, with no "thermal_bc" launch and the same number of
    "thermal" launches.  Fixed DOFs alone add no "thermal_bc" launch; convective DOFs add 4 per RK4 step and s per
    RKL2 step."""
    cs = case(orc, "A")
    bd, ref, rho20 = standard(orc, "A")
    th0 = start(cs)[0]
    nd = cs.prt.ndofs

    def cleared(th):
        bd.apply(th)
        assert th.boundary_info() != (0, 0)
        th.clear_boundary()

    def zeros(th):
        th.set_boundary_arrays(np.zeros(nd, np.uint8), np.ones(nd), np.zeros(nd), np.ones(nd))

    runs = [_counted(cs, th0, cs.dt, prep, 20) for prep in (lambda th: None, cleared, zeros)]
    for (rise, D), counts in runs:
        assert np.array_equal(rise, runs[0][0][0]) and np.array_equal(D, runs[0][0][1])
        assert counts["thermal_bc"] == 0 and counts["thermal"] == 80
    assert rel(runs[0][0][0], cs.ref.run(th0.astype(np.float64), cs.dt, 20, cs.h)) <= TOL64
    dt = 2.0 / rho20
    fixed_only = Boundary(cs, {FIXED: (0, 0)}, fixed={FIXED: 1.0})
    _, counts = _counted(cs, th0, dt, fixed_only.apply, 3, 2, 5)
    assert counts["thermal_bc"] == 0 and counts["thermal"] == 12 and counts["thermal_sts"] == 10
    _, counts = _counted(cs, th0, dt, bd.apply, 3, 2, 5)
    assert counts["thermal_bc"] == 3 * 4 + 2 * 5 and counts["thermal"] == 12 and counts["thermal_sts"] == 10


# ---- (7) life cycle and arguments -------------------------------------------------------------------------------------
def test_life_cycle_and_arguments(orc):
    cs = case(orc, "A")
    bd, ref, rho20 = standard(orc, "A")
    dt, nd = 2.0 / rho20, cs.prt.ndofs
    th0, th0d = start(cs)
    ctx, th = fresh(cs)
    assert th.boundary_info() == (0, 0)
    bd.apply(th)                                                  # before init
    assert th.boundary_info() == (int(bd.mask.sum()), int((ref.m_h > 0).sum()))
    th.init()
    assert np.array_equal(th.rise().x.array, np.where(bd.mask, bd.rise, 0.0))
    th.set_state(rise=th0)                                        # the fixed values are imposed again
    assert np.array_equal(th.rise().x.array, np.where(bd.mask, bd.rise, th0))
    # every argument error leaves the boundary in force: the object then steps like a twin that never saw the calls
    mask, ext = bd.mask.astype(np.uint8), np.full(nd, THETA_EXT)
    free = int(np.flatnonzero(~bd.mask & (bd.m_h > 0))[0])
    at_fixed = int(np.flatnonzero(bd.mask & (bd.m_h == 0))[0])
    edge = int(np.flatnonzero(bd.mask & (bd.m_h > 0))[0])        # fixed and on the convective face y = lo: fixed

    def broken(a, i, v):
        b = np.array(a, dtype=np.float64)
        b[i] = v
        return b

    for args, what in (((mask, bd.rise, broken(bd.m_h, free, -1.0), ext), "conv_diag must be"),
                       ((mask, bd.rise, broken(bd.m_h, at_fixed, np.nan), ext), "conv_diag must be"),
                       ((mask, bd.rise, broken(bd.m_h, free, np.inf), ext), "conv_diag must be"),
                       ((mask, broken(bd.rise, at_fixed, np.nan), bd.m_h, ext), "fixed_rise must be finite"),
                       ((mask, bd.rise, bd.m_h, broken(ext, free, np.inf)), "conv_rise must be finite"),
                       ((mask, bd.rise, bd.m_h, broken(ext, edge, np.nan)), "conv_rise must be finite"),
                       ((mask, bd.rise, None, ext), "conv_rise given without conv_diag")):
        with pytest.raises(fa.FusError, match=f"error -1: .*{what}"):
            th.set_boundary_arrays(*args)
    with pytest.raises(fa.FusError, match="no facet carries the tag 9"):
        th.set_boundary(bd.tags, fixed={9: 37.0})
    with pytest.raises(fa.FusError, match="conv_diag: expected"):
        th.set_boundary_arrays(conv_diag=np.zeros(nd + 1))
    assert th.boundary_info() == (int(bd.mask.sum()), int((ref.m_h > 0).sum()))
    assert np.array_equal(th.rise().x.array, np.where(bd.mask, bd.rise, th0))
    th.steps(dt, 3)
    ctx2, twin = fresh(cs, bd, th0)
    twin.steps(dt, 3)
    assert all(np.array_equal(a, b) for a, b in zip(pull(th), pull(twin)))
    # values that are never read may be anything
    twin.set_boundary_arrays(mask, broken(bd.rise, free, np.nan), bd.m_h, broken(ext, at_fixed, np.nan))
    assert twin.boundary_info() == th.boundary_info()
    twin.close(), ctx2.close()
    # set_boundary after the state exists overwrites theta at the fixed DOFs at once, and only there
    ctx2, late = fresh(cs, None, th0)
    bd.apply(late)
    assert np.array_equal(late.rise().x.array, np.where(bd.mask, bd.rise, th0))
    late.steps(dt, 3)
    assert all(np.array_equal(a, b) for a, b in zip(pull(th), pull(late)))
    # the heat load vector is what it was
    assert rel(late.heat().x.array, cs.h) <= 1e-12
    # replacing the boundary: the cooled face alone; nothing of the standard one is left
    cold, cref, crho = cooled_face(orc, "A")
    cold.apply(late)
    assert late.boundary_info() == (0, int((cref.m_h > 0).sum()))
    late.set_state(rise=th0, dose=np.zeros(nd))
    late.steps(2.0 / crho, 5)
    assert rel(late.rise().x.array, cref.run(th0d, 2.0 / crho, 5, cs.h)) <= TOL64
    late.clear_boundary()
    assert late.boundary_info() == (0, 0)
    late.close(), late.close(), ctx2.close()
    # an object sharing the op with a wave model takes its heat from the monitor with a boundary set
    mdl, wdt, bone, c, rho = plain._wave_model(cs, ctx)
    shared = fa.BioheatSpectralExplicit(cs.prt.mesh, cs.P, cs.k, cs.rho_c, cs.w, model=mdl)
    bd.apply(shared)
    shared.init()
    shared.set_heat_from(mdl, np.where(bone, 20.0, 0.5))
    h = shared.heat().x.array.astype(np.float64)
    shared.steps(dt, 5)
    want = ref.run(ref.impose(np.zeros(nd)), dt, 5, h)
    assert h.max() > 0 and rel(shared.rise().x.array, want) <= TOL64
    assert np.array_equal(shared.rise().x.array[bd.mask], held(cs, bd))
    shared.close(), mdl.close()
    th.close(), th.close(), ctx.close()


# ---- (8) the C++ example ----------------------------------------------------------------------------------------------
def test_cpp_example(orc, tmp_path):
    """examples/cpp_bioheat_bc.cpp, built as test_gpu_thermal.py builds its example, on case C: x = lo held at 1.5 K,
    x = hi water-cooled (h_c = 500, coolant at -17 K), 12 steps at stable_dt().  It prints the values the Python path
    gives for the same boundary."""
    cs = case(orc, "C")
    libdir = os.path.join(ROOT, "fenicsx-fus_amd", "fenicsxfus_amd")
    exe = tmp_path / "cpp_bioheat_bc"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "cpp_bioheat_bc.cpp"), "-L", libdir, "-lfusmi",
                           f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)])
    pr, m, nsteps = cs.pr, cs.pr.mesh, 12
    bd = Boundary(cs, {FIXED: (0, 0), CONV_X: (0, 1)}, fixed={FIXED: 1.5}, convective={CONV_X: (500.0, THETA_EXT)})
    fx, cv = bd.tags.find(FIXED), bd.tags.find(CONV_X)
    with open(tmp_path / "in.bin", "wb") as f:
        np.array([pr.tdim, pr.P, m.num_cells, pr.ndofs, m.geometry.x.shape[0], nsteps, len(fx), len(cv)],
                 dtype=np.int64).tofile(f)
        np.array([1.5, 500.0, THETA_EXT], dtype=np.float64).tofile(f)
        pr.dm.astype(np.int32).tofile(f)
        np.asarray(pr.nodes, dtype=np.float64).tofile(f)
        np.ascontiguousarray(m.geometry.x, dtype=np.float64).tofile(f)
        np.ascontiguousarray(m.geometry.dofmap, dtype=np.int32).tofile(f)
        for a in (cs.k, cs.rho_c, cs.w, cs.q):
            np.ascontiguousarray(a, dtype=np.float64).tofile(f)
        for sel in (fx, cv):
            bd.tags.cells[sel].astype(np.int32).tofile(f)
            bd.tags.local_facets[sel].astype(np.int32).tofile(f)
    out = subprocess.run([str(exe), str(tmp_path / "in.bin")], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    w = out.stdout.split()
    val = lambda key, j=1: float(w[w.index(key) + j])   # noqa: E731
    ctx, th = fresh(cs, bd)
    th.init()
    nf, nc = th.boundary_info()
    dt = th.stable_dt()
    th.steps(dt, nsteps)
    rise, D = pull(th)
    th.close(), ctx.close()
    ref = bd.ref(cs)
    assert (val("nfixed"), val("nconvective")) == (nf, nc) == (bd.mask.sum(), (ref.m_h > 0).sum())
    assert val("held_min") == val("held_max") == 1.5
    close = lambda a, b: abs(a - b) <= 1e-12 * abs(b)   # noqa: E731
    assert close(val("stable_dt"), dt) and val("stable_dt") < val("insulating_stable_dt")
    assert close(val("peak_rise"), rise.max()) and close(val("min_rise"), rise.min()) and close(val("peak_cem43"), D.max())
    assert close(val("coolest_convective"), rise[ref.m_h > 0].min()) and val("coolest_convective") < 0
    assert (val("after_clear"), val("after_clear", 2)) == (0, 0)
    assert rel(rise, ref.run(ref.impose(np.zeros(pr.ndofs)), dt, nsteps, cs.h)) <= TOL64
