"""Perfusion response and Arrhenius damage of the bioheat model on the device (fusmi.h "bioheat", perfusion response and
damage; fenicsxfus_amd.thermal) against the numpy reference of response_ref.py, which test_response_host.py pins to closed
forms first.  The cases are thermal_ref's A (trilinear P = 3), B (quadrilaterals) and F (fp32) with the tissue perfusion
raised to 4e5 W/m^3/K, so that the response shows within 20 steps.

(1) the RK4 stepper and (2) RKL2 at 2 and 8 stages against the reference; (3) the perfusion plane and the damage against
the GPU's own states; (4) a step function in the dose; (5) the step rule; (6) nothing changes while both are off, and the
launch budget while they are on; (7) several ranks; (8) arguments and life cycle; (9) the C++ example."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import fenicsxfus_amd as fa
import sts_ref
from fenicsxfus_amd import _abi
from response_ref import HENRIQUES, KNOTS, BioheatResponse, Response, damage, hot_materials
from thermal_multirank_util import (SHAPES, Global, Group, assert_interfaces_identical, quadrant_parts, slab_parts,
                                    worst_rel)
from thermal_ref import CASES, rel

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -53
TOL64, TOL32 = 1e-10, 1e-5          # the tolerances of test_gpu_thermal.py for 20 steps in fp64 / fp32
T_BASE = 37.0
DMG = (HENRIQUES["A"], HENRIQUES["Ea"])
# duty cycle of the heat load by stage count.  20 steps of the 8-stage scheme span minutes; at full power every DOF would
# be coagulated long before the end and the run would not show the three regimes of S any more
HEAT_SCALE = {0: 1.0, 2: 1.0, 8: 0.05}


@functools.lru_cache(maxsize=None)
def hot(orc, label) -> Global:
    """Case ``label`` of thermal_ref.CASES with the raised perfusion, and its step rule with phi_max of KNOTS."""
    g = Global(orc, **CASES[label], mats=hot_materials)
    g.rho_resp = BioheatResponse(g.pr, g.k, g.rho_c, g.w, response=Response(*KNOTS)).power_iteration(20)
    return g


def step_size(g, stages):
    return 2.0 / g.rho_resp if stages == 0 else sts_ref.stable_dt(g.rho_resp, stages)


class Run:
    """The reference run a test compares with: 20 steps from the live start, the dose range taken from the final dose of
    the same run without shutdown (its 30th and 70th percentiles)."""

    def __init__(self, g, stages, nsteps=20, step_at=None):
        self.g, self.stages, self.nsteps = g, stages, nsteps
        self.dt, self.sigma = step_size(g, stages), HEAT_SCALE[stages]
        self.th0, th0d = g.start()
        args = (g.pr, g.k, g.rho_c, g.w)
        run = lambda ref: ref.advance(th0d, self.dt, nsteps, g.h, self.sigma, stages=stages)   # noqa: E731
        open_doses = run(BioheatResponse(*args, response=Response(*KNOTS)))[1]
        if step_at is None:
            self.lo, self.hi = (float(v) for v in np.percentile(open_doses[-1], [30, 70]))
        else:
            self.lo = self.hi = step_at(open_doses)
        self.response = Response(*KNOTS, self.lo, self.hi)
        self.ref = BioheatResponse(*args, t_base=T_BASE, response=self.response, damage=DMG)
        self.states, self.doses = run(self.ref)
        self.omega = self.ref.omega.copy()
        self.passive = run(BioheatResponse(*args))[0][-1]

    def model(self, ctx, response=True, dmg=True):
        g, t = self.g, self.g.dtype
        th = fa.BioheatSpectralExplicit(g.prt.mesh, g.P, g.k.astype(t), g.rho_c.astype(t), g.w.astype(t), t_base=T_BASE,
                                        V=g.prt.V, ctx=ctx)
        th.set_heat(g.q.astype(t))
        if response:
            th.set_response(*KNOTS, dose_range=(self.lo, self.hi))
        if dmg:
            th.set_damage(*DMG)
        return th

    def steps(self, th, n):
        th.steps(self.dt, n, heat_scale=self.sigma, stages=self.stages)


@functools.lru_cache(maxsize=None)
def reference(orc, label, stages) -> Run:
    return Run(hot(orc, label), stages)


def pull(th):
    return th.rise().x.array.copy(), th.dose().x.array.copy(), th.damage().x.array.copy(), th.perfusion().x.array.copy()


# ---- (1), (2) the steppers --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stages", [0, 2, 8])
@pytest.mark.parametrize("label", ["A", "B", "F"])
def test_stepper_against_the_reference(orc, label, stages):
    """20 steps from a live rise, heat on, knots (37, 1), (41, 4), (45, 4) and the shutdown between the 30th and 70th
    percentile of the reference's own final dose: RK4 at 2 / rho_20 and RKL2 at stable_dt(stages), both of the phi_max
    operator.  fp64 within 1e-10 of the reference in the max norm, fp32 within 1e-5.  On the reference alone: the
    response moves the state by more than 1e-3, and DOFs with S = 1, 0 < S < 1 and S = 0 all exist at the end.  Twenty
    calls of one step and one call of twenty give the same bits in theta, D, Omega and the perfusion plane."""
    r = reference(orc, label, stages)
    g, want = r.g, r.states[-1]
    S = r.response.S(r.doses[-1])
    moved = rel(want, r.passive)
    print(f"case {label} stages {stages}: dt {r.dt:.4e} s, max rise {np.abs(want).max():.2f} K, response moves the state by "
          f"{moved:.3e}; S = 1 / between / 0 at {(S == 1).sum()} / {((S > 0) & (S < 1)).sum()} / {(S == 0).sum()} DOFs")
    assert moved > 1e-3
    assert (S == 1).any() and ((S > 0) & (S < 1)).any() and (S == 0).any()
    ctx = fa.Context(0, deterministic=True)
    th = r.model(ctx)
    assert abs(th.stable_dt(stages) - r.dt) <= (TOL64 if g.dtype == np.float64 else TOL32) * r.dt
    th.set_state(rise=r.th0)
    for _ in range(r.nsteps):
        r.steps(th, 1)
    one_by_one = pull(th)
    th.close()
    th = r.model(ctx)
    th.set_state(rise=r.th0)
    r.steps(th, r.nsteps)
    at_once = pull(th)
    th.close(), ctx.close()
    err = rel(at_once[0], want)
    print(f"case {label} stages {stages}: rel err after {r.nsteps} steps {err:.3e}")
    assert at_once[0].dtype == g.dtype and at_once[2].dtype == np.float64
    assert err <= (TOL64 if g.dtype == np.float64 else TOL32)
    for a, b in zip(one_by_one, at_once):
        assert np.array_equal(a, b)
    if g.dtype == np.float64:                                     # the dose and the damage follow the same states
        assert np.abs(at_once[1] / r.doses[-1] - 1.0).max() <= 1e-6 and np.abs(at_once[2] / r.omega - 1.0).max() <= 1e-6


# ---- (3) against the GPU's own states ---------------------------------------------------------------------------------
@pytest.mark.parametrize("label", ["A", "F"])
def test_perfusion_and_damage_against_the_gpus_own_states(orc, label):
    """12 single steps with theta and D pulled after each.  perfusion() equals T(m_W phi(theta, D)) of the pulled state
    within one ulp of T, m_W being the plane the object shows before a response is set.  damage() equals the numpy rule
    on the pulled states per DOF within the rule's own rounding: every term r = exp(x) carries the rounding of its
    argument x = lnA - Ea / (R T_K), at most (lnA + Ea / (R T_K)) 2^-53 relative to r, and an ulp of exp on either side
    (4 * 2^-53); the n trapezoid sums add n + 2 roundings.  All terms are positive, so the bound holds relative to Omega:
    (max_x + 4 + n + 2) 2^-53 with max_x = lnA + Ea / (R * 310.15 K), the coldest DOF."""
    r = reference(orc, label, 0)
    g, n = r.g, 12
    ctx = fa.Context(0, deterministic=True)
    th = r.model(ctx, response=False)
    m_w = th.perfusion().x.array.astype(np.float64)
    assert m_w.max() > 0 and np.abs(m_w - r.ref.m_w0).max() <= (1e-12 if g.dtype == np.float64 else 1e-5) * m_w.max()
    th.set_response(*KNOTS, dose_range=(r.lo, r.hi))
    th.set_state(rise=r.th0)
    states, worst_ulp = [r.th0.astype(np.float64)], 0.0
    for i in range(n + 1):
        if i:
            th.steps(r.dt, 1)
            states.append(th.rise().x.array.astype(np.float64))
        D = th.dose().x.array.copy()
        want = (m_w * r.response.phi(T_BASE + states[-1], D)).astype(g.dtype)
        got = th.perfusion().x.array
        err, ulp = np.abs(got.astype(np.float64) - want.astype(np.float64)), np.spacing(np.abs(want)).astype(np.float64)
        assert np.isfinite(got).all() and (err <= ulp).all(), i     # (a shut DOF: 0 against 0)
        worst_ulp = max(worst_ulp, float((err[want != 0] / ulp[want != 0]).max()))
    S = r.response.S(D)
    assert (S == 1).any() and ((S > 0) & (S < 1)).any() and (S == 0).any()
    assert got.dtype == g.dtype and worst_ulp <= 1.0
    om = th.damage().x.array.copy()
    th.close(), ctx.close()
    want = damage(states, r.dt, T_BASE, *DMG)
    max_x = np.log(DMG[0]) + DMG[1] / (8.314462618 * (T_BASE + min(s.min() for s in states) + 273.15))
    bound = (max_x + 4 + n + 2) * EPS
    ratio = float((np.abs(om - want) / (bound * want)).max())
    print(f"case {label}: perfusion within {worst_ulp:.1f} ulp; damage error / bound {ratio:.4f} (bound {bound:.2e} relative), "
          f"Omega in [{want.min():.3e}, {want.max():.3e}], peak {T_BASE + states[-1].max():.1f} C")
    assert (T_BASE + states[-1]).max() > 50.0 and want.min() > np.finfo(np.float64).tiny and om.min() > 0
    assert ratio <= 1.0


# ---- (4) a step function ----------------------------------------------------------------------------------------------
def _step_threshold(doses):
    """A dose near the median of the final doses that no dose of any step start comes closer to than 1e-6 relative."""
    every = np.concatenate(doses)
    for q in (50, 45, 55, 40, 60, 35, 65):
        thr = float(np.percentile(doses[-1], q)) * (1.0 + 1e-3)
        if np.abs(every / thr - 1.0).min() > 1e-6:
            return thr
    raise AssertionError("no threshold clear of the reference's doses")


def test_step_function_in_the_dose(orc):
    """dose_lo == dose_hi: the perfusion of a DOF stops from one step to the next.  No reference dose lies within 1e-6
    relative of the threshold at any step start, so both sides take the same branch everywhere; parity as in (1)."""
    r = Run(hot(orc, "A"), 0, step_at=_step_threshold)
    every = np.concatenate(r.doses)
    assert r.lo == r.hi > 0 and np.abs(every / r.hi - 1.0).min() > 1e-6
    S = r.response.S(r.doses[-1])
    assert set(np.unique(S)) == {0.0, 1.0} and rel(r.states[-1], r.passive) > 1e-3
    assert not np.array_equal(r.response.S(r.doses[5]), S)                   # DOFs cross the threshold during the run
    ctx = fa.Context(0, deterministic=True)
    th = r.model(ctx)
    th.set_state(rise=r.th0)
    r.steps(th, r.nsteps)
    got, D = th.rise().x.array.copy(), th.dose().x.array.copy()
    w = th.perfusion().x.array.copy()
    th.close(), ctx.close()
    err = rel(got, r.states[-1])
    print(f"step at {r.hi:.4e} min: {int((S == 0).sum())} of {len(S)} DOFs shut, rel err {err:.3e}")
    assert err <= TOL64 and np.array_equal(r.response.S(D), S)
    assert np.array_equal(w == 0, (S == 0) | (r.ref.m_w0 == 0))


# ---- (5) the step rule ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("label", ["A", "B", "F"])
def test_step_rule_takes_the_largest_factor(orc, label):
    g = hot(orc, label)
    tol = TOL64 if g.dtype == np.float64 else TOL32
    r = reference(orc, label, 0)
    passive = BioheatResponse(g.pr, g.k, g.rho_c, g.w).power_iteration(20)
    ctx = fa.Context(0, deterministic=True)
    th = r.model(ctx, response=False, dmg=False)
    lam0 = th.lambda_max(20)
    th.set_response(*KNOTS, dose_range=(r.lo, r.hi))
    lam, dt, dt8 = th.lambda_max(20), th.stable_dt(), th.stable_dt(8)
    th.set_response((37.0, 45.0), (1.0, 0.25))
    lam_down = th.lambda_max(20)
    th.set_response(dose_range=(r.lo, r.hi))                       # a shutdown alone: phi <= 1
    lam_shut = th.lambda_max(20)
    th.clear_response()
    lam_clear = th.lambda_max(20)
    th.close(), ctx.close()
    print(f"case {label}: lambda_max {lam0:.6e} passive, {lam:.6e} with phi_max = 4 against {g.rho_resp:.6e}")
    assert abs(lam0 - passive) <= tol * passive and lam_clear == lam0 == lam_shut
    assert abs(lam - g.rho_resp) <= tol * g.rho_resp and lam > lam0
    assert abs(dt - 2.0 / g.rho_resp) <= tol * dt and abs(dt8 - sts_ref.stable_dt(g.rho_resp, 8)) <= tol * dt8
    assert lam_down <= lam0


# ---- (6) nothing changes when off; the launch budget when on ----------------------------------------------------------
NAMES = ("thermal", "thermal_sts", "thermal_bc", "thermal_fix", "thermal_response")


def _boundary(g, th):
    """A fixed face at x = lo and a convective one at x = hi, so that every profile name of a step counts."""
    x = g.prt.V.tabulate_dof_coordinates()[:, 0]
    fixed = (x < 1e-12).astype(np.uint8)
    diag = np.where(x > g.hi[0] - 1e-12, 1e-4, 0.0).astype(g.dtype)
    th.set_boundary_arrays(fixed, np.full(len(x), 1.5, g.dtype), diag, np.full(len(x), -5.0, g.dtype))


def test_nothing_changes_when_off(orc):
    """3 RK4 steps and 3 RKL2 steps of 3 stages under a boundary with fixed and convective DOFs: an object that had a
    response and a damage law set and cleared enqueues the launches of one that never had them ("thermal_response": 0)
    and ends with the same bits in theta and D.  With them on, "thermal_response" counts nsteps + 1 for the steps call
    after a set_state and nsteps for the next one, whichever of the two is on; the other names count what they did."""
    r = reference(orc, "A", 0)
    g = r.g

    def counted(prepare):
        ctx = fa.Context(0, deterministic=True)
        th = r.model(ctx, response=False, dmg=False)
        _boundary(g, th)
        prepare(th)
        dt, dts = th.stable_dt(), th.stable_dt(3)
        th.init()
        th.set_state(rise=r.th0)
        ctx.profile_enable(True)
        th.steps(dt, 3)
        first = {nm: ctx.profile_get(nm)[1] for nm in NAMES}
        th.steps(dts, 3, stages=3)
        th.steps(dt, 2)
        counts = {nm: ctx.profile_get(nm)[1] for nm in NAMES}
        out = th.rise().x.array.copy(), th.dose().x.array.copy()
        th.close(), ctx.close()
        return out, first, counts

    def set_and_clear(th):
        th.set_response(*KNOTS, dose_range=(r.lo, r.hi))
        th.set_damage(*DMG)
        th.set_state(rise=r.th0)
        th.steps(th.stable_dt(), 2)
        th.clear_response()
        th.set_damage(0.0)

    never, first0, counts0 = counted(lambda th: None)
    cleared, first1, counts1 = counted(set_and_clear)
    assert first0 == first1 and counts0 == counts1 and counts0["thermal_response"] == 0
    assert counts0["thermal"] == 20 and counts0["thermal_sts"] == 9 and counts0["thermal_bc"] == 29 and counts0["thermal_fix"] > 0
    for a, b in zip(never, cleared):
        assert np.array_equal(a, b)
    for prepare in (lambda th: th.set_response(*KNOTS, dose_range=(r.lo, r.hi)), lambda th: th.set_damage(*DMG),
                    lambda th: (th.set_response(*KNOTS), th.set_damage(*DMG))):
        out, first, counts = counted(prepare)
        assert first["thermal_response"] == 3 + 1 and counts["thermal_response"] == 3 + 1 + 3 + 2
        assert {nm: counts[nm] for nm in NAMES[:3]} == {nm: counts0[nm] for nm in NAMES[:3]}
        assert counts["thermal_fix"] == counts0["thermal_fix"]


# ---- (7) several ranks ------------------------------------------------------------------------------------------------
def _group_case(orc, which):
    if which == "slabs":
        g = Global(orc, **SHAPES["S3"], mats=hot_materials)
        return g, slab_parts(g, 2), 20
    g = Global(orc, (4, 4, 3), 3, 0.1, np.float64, hi=[0.016, 0.016, 0.012], mats=hot_materials)
    return g, quadrant_parts(g), 10


@pytest.mark.parametrize("which", ["slabs", "quadrants"])
def test_several_ranks(orc, which):
    """Two slabs (20 RK4 steps, then 4 RKL2 steps of 4 stages) and the 2 x 2 quadrant partition (10 RK4 steps) in an
    in-process group against the one-rank reference at 1e-10; rise, dose, damage and the perfusion plane carry the same
    bits on every DOF two ranks hold.  The step rule of the group is the reference's with phi_max.  Members that differ
    in their laws are refused with FUS_ERR_STATE before anything is enqueued."""
    g, parts, nsteps = _group_case(orc, which)
    g.rho_resp = BioheatResponse(g.pr, g.k, g.rho_c, g.w, response=Response(*KNOTS)).power_iteration(20)
    r = Run(g, 0, nsteps)
    dts = sts_ref.stable_dt(g.rho_resp, 4)
    want, want_D, want_om = r.states[-1], r.doses[-1], r.omega
    nsts = 4 if which == "slabs" else 0
    for _ in range(nsts):                                          # the reference goes on from where it stands
        want = r.ref.sts_step(want, dts, 4, g.h, 0.05)
    want_D2, want_om2 = r.ref.D, r.ref.omega
    grp = Group(g, parts)
    for b in grp.bios:
        b.set_response(*KNOTS, dose_range=(r.lo, r.hi))
        b.set_damage(*DMG)
    grp.finish()
    x0 = np.zeros(g.pr.ndofs)                                      # the group's documented start vector
    for p in parts:
        x0[p.gids] += 1.0 + 0.5 * np.sin(37.0 * np.arange(len(p.gids)) + 1.0)
    want_lam = BioheatResponse(g.pr, g.k, g.rho_c, g.w, response=r.response).power_iteration(20, x0=x0)
    lam = fa.group_thermal_lambda_max(grp.bios)
    assert abs(lam - want_lam) <= TOL64 * lam and lam > g.ref.power_iteration(20, x0=x0) * (1 + 1e-3)
    assert abs(fa.group_thermal_stable_dt(grp.bios) - 2.0 / want_lam) <= TOL64 * r.dt
    grp.set_rise(r.th0)
    grp.steps(r.dt, nsteps)
    got = [grp.pull(what) for what in ("rise", "dose", "damage", "perfusion")]
    err = worst_rel(g, parts, got[0], r.states[-1])
    print(f"{which}: rel err after {nsteps} RK4 steps {err:.3e}")
    assert err <= TOL64 and rel(r.states[-1], r.passive) > 1e-3
    for a, ref, p in zip(got[1], [want_D] * len(parts), parts):
        assert np.abs(a / ref[p.gids] - 1.0).max() <= 1e-6
    for a, p in zip(got[2], parts):
        assert np.abs(a / want_om[p.gids] - 1.0).max() <= 1e-6
    w_ref = r.ref.m_weff(r.states[-1], want_D)
    assert worst_rel(g, parts, got[3], w_ref) <= 1e-6
    S = r.response.S(want_D)
    assert (S == 1).any() and ((S > 0) & (S < 1)).any() and (S == 0).any()
    assert_interfaces_identical(parts, *got)
    if nsts:
        grp.steps(dts, nsts, heat_scale=0.05, stages=4)
        got2 = [grp.pull(what) for what in ("rise", "dose", "damage", "perfusion")]
        err2 = worst_rel(g, parts, got2[0], want)
        print(f"{which}: rel err after {nsts} RKL2 steps more {err2:.3e}")
        assert err2 <= TOL64
        for a, p in zip(got2[2], parts):
            assert np.abs(a / want_om2[p.gids] - 1.0).max() <= 1e-6
        assert_interfaces_identical(parts, *got2)
        got = got2
    # members that differ: refused, and the states are as they were
    grp.bios[1].set_response(*KNOTS, dose_range=(r.lo, 2.0 * r.hi))
    for call in (lambda: grp.steps(r.dt, 1), lambda: fa.group_thermal_lambda_max(grp.bios),
                 lambda: fa.group_thermal_stable_dt(grp.bios)):
        with pytest.raises(fa.FusError, match="error -4: .*differ in their perfusion response or damage"):
            call()
    grp.bios[1].set_response(*KNOTS, dose_range=(r.lo, r.hi))
    grp.bios[0].set_damage(DMG[0], 1.01 * DMG[1])
    with pytest.raises(fa.FusError, match="error -4: .*differ in their perfusion response or damage"):
        grp.steps(r.dt, 1)
    for what, before in zip(("rise", "dose", "damage", "perfusion"), got):
        for a, b in zip(grp.pull(what), before):
            assert np.array_equal(a, b), what
    grp.close()


# ---- (8) arguments and life cycle -------------------------------------------------------------------------------------
def test_arguments_and_life_cycle(orc):
    r = reference(orc, "A", 0)
    g = r.g
    nd = g.pr.ndofs
    ctx = fa.Context(0, deterministic=True)
    th = r.model(ctx, response=False, dmg=False)
    m_w = th.perfusion().x.array.copy()
    # legal before init; the damage is off until it is set
    th.set_response(*KNOTS, dose_range=(r.lo, r.hi))
    for call in (th.damage, lambda: th.set_state(damage=np.zeros(nd))):
        with pytest.raises(fa.FusError, match="error -4: .*damage is off"):
            call()
    th.set_state(rise=r.th0)
    w0 = th.perfusion().x.array.copy()
    assert not np.array_equal(w0, m_w)
    # every argument error leaves the response as it was
    bad = [dict(temps=np.arange(9.0), factors=np.ones(9)), dict(temps=(37.0, 37.0), factors=(1.0, 2.0)),
           dict(temps=(41.0, 37.0), factors=(1.0, 2.0)), dict(temps=(37.0, np.nan), factors=(1.0, 2.0)),
           dict(temps=(37.0, np.inf), factors=(1.0, 2.0)), dict(temps=(37.0, 41.0), factors=(1.0, -2.0)),
           dict(temps=(37.0, 41.0), factors=(np.nan, 2.0)), dict(dose_range=(2.0, 1.0)), dict(dose_range=(-1.0, 1.0)),
           dict(dose_range=(0.0, np.inf)), dict(dose_range=(np.nan, 1.0))]
    for kw in bad:
        with pytest.raises(fa.FusError, match="error -1: fus_thermal_set_response"):
            th.set_response(**kw)
        assert np.array_equal(th.perfusion().x.array, w0), kw
    with pytest.raises(fa.FusError, match="temperatures but"):
        th.set_response(temps=(37.0, 41.0), factors=(1.0,))
    for A, Ea in ((-1.0, DMG[1]), (np.nan, DMG[1]), (np.inf, DMG[1]), (DMG[0], 0.0), (DMG[0], -1.0), (DMG[0], np.nan)):
        with pytest.raises(fa.FusError, match="error -1: fus_thermal_set_damage"):
            th.set_damage(A, Ea)
    with pytest.raises(fa.FusError, match="error -4: .*damage is off"):
        th.damage()
    buf = np.zeros(nd)
    assert _abi.lib().fus_thermal_set(th.h, C.c_int(_abi.FUS_TH_PERFUSION), _abi.ptr(buf), C.c_int(_abi.FUS_HOST)) == -1
    assert _abi.lib().fus_thermal_get(th.h, C.c_int(5), _abi.ptr(buf), C.c_int(_abi.FUS_HOST)) == -1
    # the damage: zero when switched on, kept by new constants, settable, zeroed by init, gone when switched off
    th.set_damage(*DMG)
    assert np.array_equal(th.damage().x.array, np.zeros(nd))
    th.steps(r.dt, 2)
    om = th.damage().x.array.copy()
    assert om.min() > 0 and np.abs(om / damage(r.states[:3], r.dt, T_BASE, *DMG) - 1.0).max() <= 1e-6
    th.set_damage(2.0 * DMG[0], DMG[1])
    assert np.array_equal(th.damage().x.array, om)
    th.set_state(damage=3.0 * om)
    assert np.array_equal(th.damage().x.array, 3.0 * om)
    state = th.rise().x.array.copy(), th.dose().x.array.copy()
    th.set_damage(0.0)
    with pytest.raises(fa.FusError, match="error -4: .*damage is off"):
        th.damage()
    assert np.array_equal(th.rise().x.array, state[0]) and np.array_equal(th.dose().x.array, state[1])
    th.set_damage(*DMG)
    assert np.array_equal(th.damage().x.array, np.zeros(nd))
    th.set_state(damage=om)
    th.init()
    assert np.array_equal(th.damage().x.array, np.zeros(nd)) and np.array_equal(th.dose().x.array, np.zeros(nd))
    # a dose above dose_hi shuts the perfusion at the next step
    D0 = np.where(np.arange(nd) % 2 == 0, 2.0 * r.hi, 0.0)
    th.set_state(rise=r.th0, dose=D0)
    w = th.perfusion().x.array
    assert np.array_equal(w[::2], np.zeros((nd + 1) // 2)) and (w[1::2] > 0).any()
    th.steps(r.dt, 3)
    want = BioheatResponse(g.pr, g.k, g.rho_c, g.w, response=r.response).advance(r.th0.astype(np.float64), r.dt, 3, g.h, D0=D0)
    assert rel(th.rise().x.array, want[0][-1]) <= TOL64
    assert rel(want[0][-1], r.states[3]) > 1e-3                    # the shut half is visible
    th.close()
    # without perfusion the call is accepted and changes nothing
    out = []
    for respond in (False, True):
        t0 = fa.BioheatSpectralExplicit(g.prt.mesh, g.P, g.k, g.rho_c, None, V=g.prt.V, ctx=ctx)
        t0.set_heat(g.q)
        if respond:
            t0.set_response(*KNOTS, dose_range=(r.lo, r.hi))
            assert np.array_equal(t0.perfusion().x.array, np.zeros(nd))
        t0.set_state(rise=r.th0)
        t0.steps(r.dt, 3)
        out.append((t0.rise().x.array.copy(), t0.dose().x.array.copy()))
        assert np.array_equal(t0.perfusion().x.array, np.zeros(nd))
        t0.close()
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])
    ctx.close()


# ---- (9) the C++ example ----------------------------------------------------------------------------------------------
def test_cpp_example(orc, tmp_path):
    """examples/cpp_bioheat_response.cpp, built as test_cpp_host.py builds its example, on case A: the step rules and the
    maxima it prints are those of the Python path on the same inputs (the same library calls: 1e-13), and the response
    shows in them."""
    r = reference(orc, "A", 0)
    g = r.g
    libdir = os.path.join(ROOT, "fenicsx-fus_amd", "fenicsxfus_amd")
    exe = tmp_path / "cpp_bioheat_response"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "cpp_bioheat_response.cpp"), "-L", libdir, "-lfusmi",
                           f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)])
    pr, m, nsteps = g.pr, g.pr.mesh, 8
    with open(tmp_path / "in.bin", "wb") as f:
        np.array([pr.tdim, pr.P, m.num_cells, pr.ndofs, m.geometry.x.shape[0], nsteps, len(KNOTS[0])], dtype=np.int64).tofile(f)
        np.array([r.lo, r.hi, *DMG, *KNOTS[0], *KNOTS[1]], dtype=np.float64).tofile(f)
        pr.dm.astype(np.int32).tofile(f)
        np.asarray(pr.nodes, dtype=np.float64).tofile(f)
        np.ascontiguousarray(m.geometry.x, dtype=np.float64).tofile(f)
        np.ascontiguousarray(m.geometry.dofmap, dtype=np.int32).tofile(f)
        for a in (g.k, g.rho_c, g.w, g.q, r.th0):
            np.ascontiguousarray(a, dtype=np.float64).tofile(f)
    out = subprocess.run([str(exe), str(tmp_path / "in.bin")], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    w = out.stdout.split()
    val = lambda key: float(w[w.index(key) + 1])   # noqa: E731
    ctx = fa.Context(0, deterministic=True)
    th = r.model(ctx, response=False)
    th.set_state(rise=r.th0)
    dt0 = th.stable_dt()
    th.steps(dt0, nsteps)
    passive_peak = th.rise().x.array.max()
    th.set_response(*KNOTS, dose_range=(r.lo, r.hi))
    th.init()
    th.set_state(rise=r.th0)
    dt = th.stable_dt()
    th.steps(dt, nsteps)
    rise, D, om, weff = pull(th)
    th.clear_response()
    m_w = th.perfusion().x.array
    th.close(), ctx.close()
    phi = weff[m_w > 0] / m_w[m_w > 0]
    for key, ref in (("passive_dt", dt0), ("passive_peak_rise", passive_peak), ("stable_dt", dt), ("peak_rise", rise.max()),
                     ("peak_cem43", D.max()), ("peak_damage", om.max()), ("phi_min", phi.min()), ("phi_max", phi.max())):
        assert abs(val(key) - ref) <= 1e-13 * abs(ref) + 1e-300, key
    assert abs(dt - r.dt) <= TOL64 * dt and dt < dt0 and val("phi_min") == 0.0 and 1.0 < val("phi_max") <= 4.0
    assert rel(rise, r.states[nsteps]) <= TOL64 and abs(val("peak_rise") - val("passive_peak_rise")) > 1e-3
