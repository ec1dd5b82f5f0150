"""The bioheat model on the device (fusmi.h "bioheat"; fenicsxfus_amd.thermal) against the numpy reference of
thermal_ref.py, which test_thermal_host.py pins to closed forms first.

(1) the RK4 stepper against the reference, cases A-F; (2) the dose kernel against the GPU's own states; (3) the heat
balance; (4) cooling and duty cycle; (5) lambda_max; (6) the heat load from the field monitor; (7) life cycle and
arguments; (8) the C++ example."""
import os
import subprocess

import numpy as np
import pytest

import fenicsxfus_amd as fa
from thermal_ref import CASES, Bioheat, case, dose, materials, rel
from util import live_state

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -53
TOL64, TOL32 = 1e-10, 1e-5          # BASELINE section 3: 20 RK4 steps in fp64 / fp32
F0, P0, S0 = 0.5e6, 6e4, 1500.0


def start(cs, seed=3, amp=5.0):
    """A rise that is live at every DOF, in the case's scalar type (returned in double too)."""
    u = live_state(cs.prt, seed, amp)[0].astype(cs.dtype)
    return u, u.astype(np.float64)


def fresh(cs, **kw):
    ctx = fa.Context(0, deterministic=True)
    return ctx, cs.model(fa, ctx, **kw)


# ---- (1) stepper ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("label", list(CASES))
def test_stepper_against_the_reference(orc, label):
    """20 steps of dt = 2 / rho_20 from a live rise, heat on: fp64 within 1e-10 of the reference in the max norm, fp32
    within 1e-5 of the double reference on the float-rounded inputs.  Twenty calls of one step and one call of twenty
    steps give the same bits in theta and D."""
    cs = case(orc, label)
    th0, th0d = start(cs)
    ref = cs.ref.run(th0d, cs.dt, 20, cs.h)
    ctx, th = fresh(cs)
    th.set_state(rise=th0)
    for _ in range(20):
        th.steps(cs.dt, 1)
    got, D = th.rise().x.array.copy(), th.dose().x.array.copy()
    th.close(), ctx.close()
    err = rel(got, ref)
    print(f"case {label}: rel err after 20 steps {err:.3e} (dt = {cs.dt:.4e} s, max rise {np.abs(ref).max():.3f} K)")
    assert got.dtype == cs.dtype and D.dtype == np.float64
    assert err <= (TOL64 if cs.dtype == np.float64 else TOL32)
    assert rel(ref, th0d) > 1e-3                                  # the run moved the state
    ctx, th = fresh(cs)
    th.set_state(rise=th0)
    th.steps(cs.dt, 20)
    again, D2 = th.rise().x.array.copy(), th.dose().x.array.copy()
    th.close(), ctx.close()
    assert np.array_equal(got, again) and np.array_equal(D, D2) and D.min() > 0


# ---- (2) dose ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("label", ["A", "F"])
def test_dose_against_the_gpus_own_states(orc, label):
    """t_base = 37, rise spanning [2, 10] K, 12 steps one call each with theta pulled after each: D equals the numpy
    rule on those states per DOF within 16 n 2^-53 relative (the monitor test's summation bound, with room for an ulp
    of exp2 on either side); set_state(dose=D) then dose() returns D bit for bit."""
    cs = case(orc, label)
    u = start(cs, seed=5)[1]
    th0 = (2.0 + 8.0 * (u - u.min()) / (u.max() - u.min())).astype(cs.dtype)
    ctx, th = fresh(cs)
    th.set_state(rise=th0)
    states, n = [], 12
    for _ in range(n):
        th.steps(cs.dt, 1)
        states.append(th.rise().x.array.astype(np.float64))
    D = th.dose().x.array.copy()
    assert any((37.0 + x >= 43.0).any() and (37.0 + x < 43.0).any() for x in states)
    ref = dose(states, cs.dt, 37.0)
    worst = float((np.abs(D - ref) / (16 * n * EPS * ref)).max())
    print(f"case {label}: dose error / bound {worst:.3f}, D in [{ref.min():.3e}, {ref.max():.3e}] min")
    assert ref.min() > 0 and worst <= 1.0
    th.set_state(dose=2.0 * D)
    assert np.array_equal(th.dose().x.array, 2.0 * D)
    assert np.array_equal(th.rise().x.array.astype(np.float64), states[-1])       # the rise is untouched
    th.close(), ctx.close()


# ---- (3) heat balance -------------------------------------------------------------------------------------------------
def test_heat_balance_on_the_device(orc):
    """Case C without perfusion, theta_0 = 0, constant h: m_C . theta_n = n dt sum(h) to 1e-10."""
    cs = case(orc, "C")
    ctx = fa.Context(0, deterministic=True)
    th = fa.BioheatSpectralExplicit(cs.prt.mesh, cs.P, cs.k, cs.rho_c, None, V=cs.prt.V, ctx=ctx)
    th.init()
    th.set_heat(cs.q)
    n = 9
    th.steps(cs.dt, n)
    got, h = th.rise().x.array.copy(), th.heat().x.array.copy()
    th.close(), ctx.close()
    total = n * cs.dt * cs.h.sum()
    assert total > 0 and rel(h, cs.h) <= 1e-12
    assert abs(cs.ref.m_c @ got - total) <= 1e-10 * total


# ---- (4) cooling and duty ---------------------------------------------------------------------------------------------
def test_cooling_and_duty(orc):
    cs = case(orc, "A")
    th0, th0d = start(cs)
    ctx, th = fresh(cs)
    th.set_state(rise=th0)
    ref = th0d
    for sigma in (1.0, 0.0, 0.5):
        th.steps(cs.dt, 5, heat_scale=sigma)
        ref = cs.ref.run(ref, cs.dt, 5, cs.h, sigma)
    got = th.rise().x.array.copy()
    th.close(), ctx.close()
    full = cs.ref.run(th0d, cs.dt, 15, cs.h, 1.0)
    assert rel(got, ref) <= TOL64
    assert rel(full, ref) > 1e-3                                 # the segments' heat scales are visible


# ---- (5) lambda_max ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("label", ["A", "B", "F"])
def test_lambda_max(orc, label):
    cs = case(orc, label)
    ctx, th = fresh(cs)
    lam, dt = th.lambda_max(20), th.stable_dt()
    lam3 = th.lambda_max(3)
    th.close(), ctx.close()
    tol = TOL64 if cs.dtype == np.float64 else TOL32
    print(f"case {label}: lambda_max(20) {lam:.6e} against {cs.rho20:.6e}")
    assert abs(lam - cs.rho20) <= tol * cs.rho20
    assert abs(dt - 2.0 / cs.rho20) <= tol * dt
    assert abs(lam3 - cs.ref.power_iteration(3)) <= tol * lam3 and lam3 < lam


# ---- (6) heat from the monitor ----------------------------------------------------------------------------------------
def _wave_model(cs, ctx):
    pr = cs.prt
    bone = materials(pr.mesh, cs.hi)[0] == 0.32
    c = np.where(bone, 2800.0, 1500.0).astype(cs.dtype)
    rho = np.where(bone, 1850.0, 1000.0).astype(cs.dtype)
    dt = 0.5 * 0.003 / (2800.0 * cs.P ** 2)
    mdl = fa.LinearSpectralExplicit(pr.mesh, fa.tag_box_boundary(pr.mesh), cs.P, c, rho, F0, P0, S0, 4, dt, V=pr.V, ctx=ctx)
    u0, v0 = live_state(pr, 11, P0, F0)
    mdl.init()
    mdl.set_state(u0, v0)
    mdl.monitor(which="u", every=1)
    mdl.rk4_steps(0.0, dt, 18)
    return mdl, dt, bone, c.astype(np.float64), rho.astype(np.float64)


def _wave_maps(mdl):
    mdl.u_sol()
    out = {"u": mdl.u_n.x.array.copy(), "v": mdl.v_n.x.array.copy()}
    for q in ("max", "min", "mean", "rms"):
        out[q] = mdl.monitor_get(q).x.array.copy()
    return out


@pytest.mark.parametrize("label", ["A", "F", "B"])       # B: the one small case with bone cells (per-cell alpha, rho c)
def test_heat_from_the_monitor(orc, label):
    """A Linear model watches u over 18 steps; a thermal object on the same operator data takes its heat load from the
    monitor: h = M(2 alpha / (rho c)) 1 .* rms^2 (1e-12 of the maximum in fp64, 1e-5 in fp32), five thermal steps follow
    the reference driven by that vector (fp64), the wave model's state and maps keep their bits, and three further
    wave steps give the bits of a model that never had a thermal object beside it."""
    cs = case(orc, label)
    ctx = fa.Context(0, deterministic=True)
    mdl, wdt, bone, c, rho = _wave_model(cs, ctx)
    before = _wave_maps(mdl)
    t = cs.dtype
    th = fa.BioheatSpectralExplicit(cs.prt.mesh, cs.P, cs.k.astype(t), cs.rho_c.astype(t), cs.w.astype(t), model=mdl)
    alpha = np.where(bone, 20.0, 0.5)
    th.init()
    th.set_heat_from(mdl, alpha.astype(t))
    h = th.heat().x.array.copy()
    rms = before["rms"].astype(np.float64)
    href = cs.pr.M(np.ones(cs.pr.ndofs), 2.0 * alpha / (rho * c)) * rms ** 2
    err = float(np.abs(h - href).max() / href.max())
    print(f"case {label}: heat from the monitor, error / max {err:.3e}; max h {href.max():.3e} W")
    assert href.max() > 0 and err <= (1e-12 if cs.dtype == np.float64 else 1e-5)
    th.steps(cs.dt, 5)
    got = th.rise().x.array.copy()
    if cs.dtype == np.float64:
        ref = cs.ref.run(np.zeros(cs.pr.ndofs), cs.dt, 5, h.astype(np.float64))
        assert np.abs(ref).max() > 0 and rel(got, ref) <= TOL64
    th.lambda_max(2)
    after = _wave_maps(mdl)
    for key in before:
        assert np.array_equal(before[key], after[key]), key
    mdl.rk4_steps(18 * wdt, wdt, 3)
    with_thermal = _wave_maps(mdl)
    th.close()
    th.close()                                                    # twice is harmless
    mdl.close(), ctx.close()
    ctx = fa.Context(0, deterministic=True)
    mdl = _wave_model(cs, ctx)[0]
    mdl.rk4_steps(18 * wdt, wdt, 3)
    alone = _wave_maps(mdl)
    mdl.close(), ctx.close()
    for key in alone:
        assert np.array_equal(alone[key], with_thermal[key]), key


# ---- (7) life cycle and arguments -------------------------------------------------------------------------------------
def test_life_cycle_and_arguments(orc):
    cs = case(orc, "A")
    pr, nc = cs.prt, cs.prt.mesh.num_cells
    ctx = fa.Context(0, deterministic=True)
    mk = lambda k, rc, w, **kw: fa.BioheatSpectralExplicit(pr.mesh, cs.P, k, rc, w, V=pr.V, ctx=ctx, **kw)   # noqa: E731
    bad = cs.k.copy()
    bad[nc // 2] = -1.0
    nan = cs.k.copy()
    nan[0] = np.nan
    zero = cs.rho_c.copy()
    zero[1] = 0.0
    for args, what in (((bad, cs.rho_c, cs.w), "conductivity"), ((nan, cs.rho_c, cs.w), "conductivity"),
                       ((cs.k, zero, cs.w), "rho_c"), ((cs.k, cs.rho_c, -cs.w - 1.0), "perfusion"),
                       ((cs.k, cs.rho_c, np.full(nc, np.inf)), "perfusion")):
        with pytest.raises(fa.FusError, match=f"error -1: .*{what}"):
            mk(*args)
    th = mk(cs.k, cs.rho_c, cs.w)
    with pytest.raises(fa.FusError, match="error -4: .*fus_thermal_init"):
        th.steps(cs.dt, 1)
    th.init()
    th0 = start(cs)[0]
    th.set_state(rise=th0)
    th.set_heat(cs.q)
    for dt in (0.0, -1.0, np.nan):
        with pytest.raises(fa.FusError, match="error -1: .*dt"):
            th.steps(dt, 1)
    with pytest.raises(fa.FusError, match="error -1: .*iters"):
        th.lambda_max(0)
    assert np.array_equal(th.rise().x.array, th0)                                    # the state is as it was
    assert rel(th.heat().x.array, cs.h) <= 1e-12
    # the monitor's states
    mdl, wdt, bone, _, _ = _wave_model(cs, ctx)          # its own operator data: not the thermal object's
    alpha = np.where(bone, 20.0, 0.5)
    with pytest.raises(fa.FusError, match="error -1: .*another fus_op"):
        th.set_heat_from(mdl, alpha)
    th2 = fa.BioheatSpectralExplicit(pr.mesh, cs.P, cs.k, cs.rho_c, cs.w, model=mdl)
    with pytest.raises(fa.FusError, match="error -1: .*absorption"):
        th2.set_heat_from(mdl, -alpha)
    mdl.monitor(which="v", every=1)
    mdl.rk4_steps(0.0, wdt, 1)
    with pytest.raises(fa.FusError, match="error -4: .*FUS_V"):
        th2.set_heat_from(mdl, alpha)
    mdl.monitor(which="u", every=1)
    with pytest.raises(fa.FusError, match="error -4: .*no sample"):
        th2.set_heat_from(mdl, alpha)
    mdl.monitor_off()
    with pytest.raises(fa.FusError, match="error -4: .*monitor is off"):
        th2.set_heat_from(mdl, alpha)
    assert np.array_equal(th2.heat().x.array, np.zeros(pr.ndofs))                  # the heat load is as it was
    # a second thermal object on the SAME operator data (one fus_op, one set of scratch), stepped in turns with the
    # first and with set_heat and lambda_max calls between the first one's steps: the same bits in rise and dose, and
    # the bits of an object that ran alone on operator data of its own
    same = fa.BioheatSpectralExplicit(pr.mesh, cs.P, cs.k, cs.rho_c, cs.w, data=th.data)
    assert same.data is th.data and same.data.h.value == th.data.h.value
    same.set_state(rise=th0)
    for _ in range(3):
        th.steps(cs.dt, 1)
        same.set_heat(cs.q)
        same.steps(cs.dt, 1)
        same.lambda_max(2)
    th2.set_state(rise=th0)
    th2.set_heat(cs.q)
    th2.steps(cs.dt, 3)
    for other in (same, th2):
        assert np.array_equal(th.rise().x.array, other.rise().x.array)
        assert np.array_equal(th.dose().x.array, other.dose().x.array)
    assert rel(th.rise().x.array, cs.ref.run(th0.astype(np.float64), cs.dt, 3, cs.h)) <= TOL64
    same.close(), same.close()
    assert th.data.h                                               # closing a sharer leaves the operator data alone
    th.steps(cs.dt, 1)
    th2.close(), th2.close(), mdl.close()
    th.close(), th.close()
    # operator data created for two fields is accepted; several ranks are refused
    data2 = fa.SpectralOperatorData(pr.V, ctx, fields=2)
    th3 = fa.BioheatSpectralExplicit(pr.mesh, cs.P, cs.k, cs.rho_c, cs.w, data=data2)
    th3.set_state(rise=th0)
    th3.set_heat(cs.q)
    th3.steps(cs.dt, 3)
    assert rel(th3.rise().x.array, cs.ref.run(th0.astype(np.float64), cs.dt, 3, cs.h)) <= TOL64
    th3.close(), data2.close()
    slab = fa.BoxMesh([0.0] * 3, cs.hi, cs.n, rank=0, size=2)
    Vs = fa.FunctionSpace(slab, cs.P)
    assert Vs.neighbours
    with pytest.raises(fa.FusError, match="error -4: .*several ranks"):
        fa.BioheatSpectralExplicit(slab, cs.P, 0.5, 3.6e6, V=Vs, ctx=ctx)
    ctx.close()


# ---- (8) the C++ example ----------------------------------------------------------------------------------------------
def test_cpp_example(orc, tmp_path):
    """examples/cpp_bioheat_run.cpp, built as test_cpp_host.py builds its example: without perfusion the energy it
    prints equals the heat put in (sonication, then cooling) to 1e-10, and that is n dt sum(h) of the reference."""
    cs = case(orc, "C")
    libdir = os.path.join(ROOT, "fenicsx-fus_amd", "fenicsxfus_amd")
    exe = tmp_path / "cpp_bioheat_run"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "cpp_bioheat_run.cpp"), "-L", libdir, "-lfusmi",
                           f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)])
    pr, m = cs.pr, cs.pr.mesh
    nheat, ncool = 6, 4
    with open(tmp_path / "in.bin", "wb") as f:
        np.array([pr.tdim, pr.P, m.num_cells, pr.ndofs, m.geometry.x.shape[0], nheat, ncool], dtype=np.int64).tofile(f)
        np.array([cs.dt], dtype=np.float64).tofile(f)
        pr.dm.astype(np.int32).tofile(f)
        np.asarray(pr.nodes, dtype=np.float64).tofile(f)
        np.ascontiguousarray(m.geometry.x, dtype=np.float64).tofile(f)
        np.ascontiguousarray(m.geometry.dofmap, dtype=np.int32).tofile(f)
        for a in (cs.k, cs.rho_c, np.zeros(m.num_cells), cs.q):
            np.ascontiguousarray(a, dtype=np.float64).tofile(f)
    out = subprocess.run([str(exe), str(tmp_path / "in.bin")], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    w = out.stdout.split()
    val = lambda key: float(w[w.index(key) + 1])   # noqa: E731
    total = nheat * cs.dt * cs.h.sum()
    assert abs(val("energy") - val("heat_in")) <= 1e-10 * total and abs(val("heat_in") - total) <= 1e-10 * total
    assert val("peak_rise") > 0 and val("peak_cem43") > 0
    assert abs(val("stable_dt") - 2.0 / Bioheat(pr, cs.k, cs.rho_c, 0.0).power_iteration(20)) <= 1e-10 * cs.dt
