"""Super-time-stepping of the bioheat model on the device (fusmi.h "bioheat", fus_thermal_steps_sts) against the numpy
reference of sts_ref.py, which test_sts_host.py pins to the scheme's promises first.

(1) the RKL2 stepper against the reference, cases A-F; (2) the trapezoid dose against the GPU's own states; (3) stages = 0
is the RK4 path; (4) mixed RK4 / RKL2 segments; (5) the heat balance; (6) stable_dt(stages); (7) arguments and sharing;
(8) the C++ example."""
import os
import subprocess

import numpy as np
import pytest

import fenicsxfus_amd as fa
import sts_ref
from test_gpu_thermal import _wave_maps, _wave_model, fresh, start
from thermal_ref import CASES, Bioheat, case, rel

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -53
TOL64, TOL32 = 1e-10, 1e-5          # the RK4 path's bounds: the recurrence's rounding stays far inside them up to s = 32


def tol(cs):
    return TOL64 if cs.dtype == np.float64 else TOL32


# ---- (1) stepper ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("label,s", [(lb, s) for lb in CASES for s in (2, 3, 8, 9)] + [("A", 32)])
def test_stepper_against_the_reference(orc, label, s):
    """Five steps of dt = 0.72 beta_s / rho_20 from a live rise, heat on: fp64 within 1e-10 of the reference in the max
    norm, fp32 within 1e-5 of the double reference on the float-rounded inputs.  s = 2 has no middle stage, 3 is the
    first stage index on the b_j formula, 8 and 9 end the buffer rotation on either side.  Five calls of one step and
    one call of five steps give the same bits in theta and D."""
    cs = case(orc, label)
    dt = sts_ref.stable_dt(cs.rho20, s)
    th0, th0d = start(cs)
    ref = sts_ref.run(cs.ref, th0d, dt, 5, s, cs.h)
    ctx, th = fresh(cs)
    th.set_state(rise=th0)
    for _ in range(5):
        th.steps(dt, 1, stages=s)
    got, D = th.rise().x.array.copy(), th.dose().x.array.copy()
    th.close(), ctx.close()
    err = rel(got, ref)
    print(f"case {label}, s = {s}: rel err after 5 steps {err:.3e} (dt = {dt:.4e} s, max rise {np.abs(ref).max():.3f} K)")
    assert got.dtype == cs.dtype and D.dtype == np.float64
    assert err <= tol(cs)
    assert rel(ref, th0d) > 1e-3                                  # the run moved the state
    ctx, th = fresh(cs)
    th.set_state(rise=th0)
    th.steps(dt, 5, stages=s)
    again, D2 = th.rise().x.array.copy(), th.dose().x.array.copy()
    th.close(), ctx.close()
    assert np.array_equal(got, again) and np.array_equal(D, D2) and D.min() > 0


# ---- (2) dose ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("label", ["A", "F"])
def test_dose_against_the_gpus_own_states(orc, label):
    """t_base = 37, rise spanning [2, 10] K, six steps of s = 8, one call each with theta pulled after each: D equals
    the trapezoid rule on those states (the start state included) per DOF within 16 (2 n) 2^-53 relative -- the RK4
    dose test's bound, doubled because every step adds two exp2 terms."""
    cs = case(orc, label)
    s, n = 8, 6
    dt = sts_ref.stable_dt(cs.rho20, s)
    u = start(cs, seed=5)[1]
    th0 = (2.0 + 8.0 * (u - u.min()) / (u.max() - u.min())).astype(cs.dtype)
    ctx, th = fresh(cs)
    th.set_state(rise=th0)
    states = [th0.astype(np.float64)]
    for _ in range(n):
        th.steps(dt, 1, stages=s)
        states.append(th.rise().x.array.astype(np.float64))
    D = th.dose().x.array.copy()
    th.close(), ctx.close()
    assert any((37.0 + x >= 43.0).any() and (37.0 + x < 43.0).any() for x in states)
    ref = sts_ref.dose_trapezoid(states, dt, 37.0)
    worst = float((np.abs(D - ref) / (16 * 2 * n * EPS * ref)).max())
    print(f"case {label}: dose error / bound {worst:.3f}, D in [{ref.min():.3e}, {ref.max():.3e}] min")
    assert ref.min() > 0 and worst <= 1.0


# ---- (3) stages = 0 ---------------------------------------------------------------------------------------------------
def test_stages_zero_is_the_rk4_path(orc):
    cs = case(orc, "A")
    th0 = start(cs)[0]
    out = []
    for kw in ({"stages": 0}, {}):
        ctx, th = fresh(cs)
        th.set_state(rise=th0)
        th.steps(cs.dt, 5, **kw)
        out.append((th.rise().x.array.copy(), th.dose().x.array.copy()))
        th.close(), ctx.close()
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])
    assert rel(out[0][0], cs.ref.run(th0.astype(np.float64), cs.dt, 5, cs.h)) <= TOL64


# ---- (4) mixed segments -----------------------------------------------------------------------------------------------
def test_mixed_segments(orc):
    """3 RK4 steps, 3 RKL2 steps of s = 8, 2 RKL2 steps of s = 4 with the heat off, 2 RK4 steps: the reference doing the
    same, and visibly not the all-heated run."""
    cs = case(orc, "A")
    th0, th0d = start(cs)
    d8, d4 = sts_ref.stable_dt(cs.rho20, 8), sts_ref.stable_dt(cs.rho20, 4)
    ctx, th = fresh(cs)
    th.set_state(rise=th0)
    th.steps(cs.dt, 3)
    th.steps(d8, 3, stages=8)
    th.steps(d4, 2, heat_scale=0.0, stages=4)
    th.steps(cs.dt, 2)
    got = th.rise().x.array.copy()
    th.close(), ctx.close()

    def reference(sigma):
        r = cs.ref.run(th0d, cs.dt, 3, cs.h)
        r = sts_ref.run(cs.ref, r, d8, 3, 8, cs.h)
        r = sts_ref.run(cs.ref, r, d4, 2, 4, cs.h, sigma)
        return cs.ref.run(r, cs.dt, 2, cs.h)

    ref = reference(0.0)
    assert rel(got, ref) <= TOL64
    assert rel(reference(1.0), ref) > 1e-3


# ---- (5) heat balance -------------------------------------------------------------------------------------------------
def test_heat_balance_on_the_device(orc):
    """Case C without perfusion, theta_0 = 0, constant h, s = 8: m_C . theta_9 = 9 dt sum(h) to 1e-10."""
    cs = case(orc, "C")
    ctx = fa.Context(0, deterministic=True)
    th = fa.BioheatSpectralExplicit(cs.prt.mesh, cs.P, cs.k, cs.rho_c, None, V=cs.prt.V, ctx=ctx)
    th.init()
    th.set_heat(cs.q)
    n, dt = 9, sts_ref.stable_dt(cs.rho20, 8)
    th.steps(dt, n, stages=8)
    got = th.rise().x.array.copy()
    th.close(), ctx.close()
    total = n * dt * cs.h.sum()
    assert total > 0 and abs(cs.ref.m_c @ got - total) <= 1e-10 * total


# ---- (6) stable_dt ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("label", ["A", "B", "F"])
def test_stable_dt(orc, label):
    cs = case(orc, label)
    ctx, th = fresh(cs)
    dts = {s: th.stable_dt(stages=s) for s in (0, 2, 8)}
    plain = th.stable_dt()
    th.close(), ctx.close()
    for s in (2, 8):
        want = 0.72 * (s * s + s - 2) / (2.0 * cs.rho20)
        assert abs(dts[s] - want) <= tol(cs) * want
    assert dts[0] == plain and abs(plain - 2.0 / cs.rho20) <= tol(cs) * plain


# ---- (7) arguments and sharing ----------------------------------------------------------------------------------------
def test_arguments(orc):
    cs = case(orc, "A")
    ctx = fa.Context(0, deterministic=True)
    th = fa.BioheatSpectralExplicit(cs.prt.mesh, cs.P, cs.k, cs.rho_c, cs.w, V=cs.prt.V, ctx=ctx)
    dt = sts_ref.stable_dt(cs.rho20, 8)
    with pytest.raises(fa.FusError, match="error -4: .*fus_thermal_init"):
        th.steps(dt, 1, stages=8)
    th0 = start(cs)[0]
    th.set_state(rise=th0)
    th.set_heat(cs.q)
    for s in (1, -1, 33):
        with pytest.raises(fa.FusError, match="error -1: .*stages"):
            th.steps(dt, 1, stages=s)
        with pytest.raises(fa.FusError, match="error -1: .*stages"):
            th.stable_dt(stages=s)
    for bad in (0.0, -1.0, np.nan):
        with pytest.raises(fa.FusError, match="error -1: .*dt"):
            th.steps(bad, 1, stages=8)
    with pytest.raises(fa.FusError, match="error -1: .*nsteps"):
        th.steps(dt, -1, stages=8)
    assert np.array_equal(th.rise().x.array, th0)                                    # the state is as it was
    assert not th.dose().x.array.any()
    th.close(), ctx.close()


def test_two_objects_on_one_operator(orc):
    """Two thermal objects on the SAME operator data, stepped in turns (one super-stepping with s = 8, the other with
    RK4; set_heat and lambda_max calls between): each has the bits of an object that ran alone."""
    cs = case(orc, "A")
    th0 = start(cs)[0]
    d8 = sts_ref.stable_dt(cs.rho20, 8)
    ctx, a = fresh(cs)
    b = fa.BioheatSpectralExplicit(cs.prt.mesh, cs.P, cs.k, cs.rho_c, cs.w, data=a.data)
    a.set_state(rise=th0), b.set_state(rise=th0)
    for _ in range(3):
        a.steps(d8, 1, stages=8)
        b.set_heat(cs.q)
        b.steps(cs.dt, 1)
        b.lambda_max(2)
        a.lambda_max(2)
    b.steps(d8, 2, stages=8)
    shared = [(o.rise().x.array.copy(), o.dose().x.array.copy()) for o in (a, b)]
    b.close(), a.close(), ctx.close()
    alone = []
    for segs in (((d8, 3, 8),), ((cs.dt, 3, 0), (d8, 2, 8))):
        ctx, o = fresh(cs)
        o.set_state(rise=th0)
        for dt, n, s in segs:
            o.steps(dt, n, stages=s)
        alone.append((o.rise().x.array.copy(), o.dose().x.array.copy()))
        o.close(), ctx.close()
    for (r, d), (r1, d1) in zip(shared, alone):
        assert np.array_equal(r, r1) and np.array_equal(d, d1)
    assert rel(shared[0][0], sts_ref.run(cs.ref, th0.astype(np.float64), d8, 3, 8, cs.h)) <= TOL64


def test_wave_model_beside_a_super_stepped_run(orc):
    """A Linear model and a thermal object on its operator data: after a super-stepped thermal run the model's state and
    maps keep their bits, and five further wave steps give the bits of a model that never had a thermal object beside
    it."""
    cs = case(orc, "A")
    ctx = fa.Context(0, deterministic=True)
    mdl, wdt, bone, _, _ = _wave_model(cs, ctx)
    before = _wave_maps(mdl)
    th = fa.BioheatSpectralExplicit(cs.prt.mesh, cs.P, cs.k, cs.rho_c, cs.w, model=mdl)
    th.init()
    th.set_heat_from(mdl, np.where(bone, 20.0, 0.5))
    h = th.heat().x.array.copy()
    d8 = sts_ref.stable_dt(cs.rho20, 8)
    th.steps(d8, 4, stages=8)
    got = th.rise().x.array.copy()
    ref = sts_ref.run(cs.ref, np.zeros(cs.pr.ndofs), d8, 4, 8, h)
    assert np.abs(ref).max() > 0 and rel(got, ref) <= TOL64
    after = _wave_maps(mdl)
    for key in before:
        assert np.array_equal(before[key], after[key]), key
    mdl.rk4_steps(18 * wdt, wdt, 5)
    with_thermal = _wave_maps(mdl)
    th.close(), mdl.close(), ctx.close()
    ctx = fa.Context(0, deterministic=True)
    mdl = _wave_model(cs, ctx)[0]
    mdl.rk4_steps(18 * wdt, wdt, 5)
    alone = _wave_maps(mdl)
    mdl.close(), ctx.close()
    for key in alone:
        assert np.array_equal(alone[key], with_thermal[key]), key


# ---- (8) the C++ example ----------------------------------------------------------------------------------------------
def test_cpp_example(orc, tmp_path):
    """examples/cpp_bioheat_sts.cpp, built as test_gpu_thermal.py builds its example: without perfusion the energy it
    prints equals the heat put in (sonication, then cooling, both super-stepped with s = 8) to 1e-10, that is
    n dt sum(h) of the reference, and its stable_dt is the reference's."""
    cs = case(orc, "C")
    libdir = os.path.join(ROOT, "fenicsx-fus_amd", "fenicsxfus_amd")
    exe = tmp_path / "cpp_bioheat_sts"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "cpp_bioheat_sts.cpp"), "-L", libdir, "-lfusmi",
                           f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)])
    pr, m = cs.pr, cs.pr.mesh
    nheat, ncool, stages = 6, 4, 8
    with open(tmp_path / "in.bin", "wb") as f:
        np.array([pr.tdim, pr.P, m.num_cells, pr.ndofs, m.geometry.x.shape[0], nheat, ncool, stages], dtype=np.int64).tofile(f)
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
    dt = sts_ref.stable_dt(Bioheat(pr, cs.k, cs.rho_c, 0.0).power_iteration(20), stages)
    total = nheat * dt * cs.h.sum()
    assert abs(val("stable_dt") - dt) <= 1e-10 * dt
    assert abs(val("energy") - val("heat_in")) <= 1e-10 * total and abs(val("heat_in") - total) <= 1e-10 * total
    assert val("peak_rise") > 0 and val("peak_cem43") > 0
