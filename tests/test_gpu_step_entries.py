"""Every stepping entry of the wave models takes the same steps: one step function (wave.hip wave_step) is behind
rk4_steps, rk, group_rk4_steps and the external stage halves, and this file pins what writing it once could break.

(1) the state after 5 steps is bit for bit the same through (a) one rk4_steps call, (b) five calls of one step,
    (c) rk(0, 5 dt), (d) group_rk4_steps on a group of one, (e) the stage halves driven from Python;
(2) the end-of-step bookkeeping -- the swap of the orders 1-3, the receiver record, the monitor sample -- happens once
    per step at the same time in every form;
(3) k_boundary_partial runs only when the pseudo boundary slots are stale: once at RK4 (the first stage after the state
    was set; stage_end leaves the next stage's terms, also across the calls of form (b)), at every stage at RK2.

The cases: perturbed hexahedra, (4, 2, 2) cells in four blocks, so shared boundary DOFs exist; deterministic = 1, the
setting under which a run repeats its bits; live starts.  dt is the largest power of two not above the case's stable
step, so every time of the run is exact in float as in double and the float clock of rk() lands on the same times."""
import math

import numpy as np
import pytest

import fenicsxfus_amd as fa
from live_cases import Case

pytestmark = pytest.mark.gpu
NSTEPS = 5
FORMS = ("steps", "single", "rk", "group", "external")
TYPES = {"f64": np.float64, "f32": np.float32}
CASES = [(kind, P, tname, order) for kind in ("linear", "westervelt") for P in (2, 4) for tname in TYPES
         for order in (4, 2)]
IDS = [f"{k}-p{P}-{t}-rk{o}" for k, P, t, o in CASES]
_cases, _runs = {}, {}


def the_case(orc, kind, P, tname, order):
    key = (kind, P, tname, order)
    if key not in _cases:
        # cfl 0.1 below order 4, as the rk1-3 cases of live_cases.py
        cs = Case(orc, kind, (4, 2, 2), P, nsteps=NSTEPS, order=order, dtype=TYPES[tname], cfl=0.5 if order == 4 else 0.1)
        cs.dt2 = 2.0 ** math.floor(math.log2(cs.dt))
        assert cs.dt / 2 < cs.dt2 <= cs.dt and float(np.float32(NSTEPS * cs.dt2)) == NSTEPS * cs.dt2
        lo, hi = np.zeros(3), np.array(cs.hi)
        cs.points = lo + (hi - lo) * np.array([[0.5, 0.5, 0.5], [0.07, 0.4, 0.6], [0.93, 0.81, 0.22]])
        _cases[key] = cs
    return _cases[key]


def run(cs, form, profile=False):
    """5 steps of dt2 from the case's live start through one entry form, with 3 receivers recorded and the monitor
    sampling after every step."""
    dt = cs.dt2
    ctx = fa.Context(0, block_elems=4, deterministic=True)
    if form == "external":
        ctx.init_external(0, 1)
    elif form == "group":
        fa.Context.init_local_group([ctx])
    mdl = cs.model(ctx)
    try:
        info = mdl.data.info()
        assert info["nblocks"] >= 2 and info["shared_dofs"] > 0
        assert len(mdl.set_receivers(cs.points)) == 3
        u0, v0 = cs.start()
        mdl.set_state(u=u0, v=v0)
        mdl.record(1, 2 * NSTEPS, "u")
        mdl.monitor("u", nharm=1, skip=0, every=1)
        if profile:
            ctx.profile_enable(True)
        nsteps = NSTEPS
        if form == "steps":
            mdl.rk4_steps(0.0, dt, NSTEPS)
        elif form == "single":
            for s in range(NSTEPS):
                mdl.rk4_steps(s * dt, dt, 1)
        elif form == "rk":
            mdl.dt = dt
            mdl.rk(0.0, NSTEPS * dt)
            nsteps = mdl.nsteps
        elif form == "group":
            fa.group_rk4_steps([mdl], 0.0, dt, NSTEPS)
        else:
            mdl.external_rk_steps(0.0, dt, NSTEPS, lambda: None, rk_order=cs.order)
        u = mdl.u_sol().x.array.copy()
        out = dict(u=u, v=mdl.v_n.x.array.copy(), nsteps=nsteps, records=mdl.records(), mon=mdl.monitor_info(),
                   mon_max=mdl.monitor_get("max").x.array.copy(), mon_cos=mdl.monitor_get("cos", 1).x.array.copy())
        if profile:
            out["boundary"] = ctx.profile_get("boundary")[1]
    finally:
        mdl.close(), ctx.close()
    return out


def runs(orc, kind, P, tname, order):
    key = (kind, P, tname, order)
    if key not in _runs:
        cs = the_case(orc, *key)
        _runs[key] = {form: run(cs, form) for form in FORMS}
    return _runs[key]


@pytest.mark.parametrize("kind,P,tname,order", CASES, ids=IDS)
def test_all_entry_points_take_the_same_steps(orc, kind, P, tname, order):
    """u and v after the 5 steps: the same bits from every entry form, and rk() counts 5 steps."""
    R = runs(orc, kind, P, tname, order)
    ref = R["steps"]
    assert np.isfinite(ref["u"]).all() and np.abs(ref["u"]).max() > 0 and np.abs(ref["v"]).max() > 0
    assert R["rk"]["nsteps"] == NSTEPS
    for form in FORMS[1:]:
        assert np.array_equal(R[form]["u"], ref["u"]), form
        assert np.array_equal(R[form]["v"], ref["v"]), form


@pytest.mark.parametrize("kind,P,tname,order", CASES, ids=IDS)
def test_end_of_step_bookkeeping(orc, kind, P, tname, order):
    """5 records at the times dt, ..., 5 dt with the same values, and 5 monitor samples over the same window with the
    same maps (the harmonic's phase factors come from the sample times), from every entry form."""
    R = runs(orc, kind, P, tname, order)
    dt = the_case(orc, kind, P, tname, order).dt2
    times = np.array([(s + 1) * dt for s in range(NSTEPS)])
    t_ref, rec_ref = R["steps"]["records"]
    assert np.abs(rec_ref).min() > 0
    for form in FORMS:
        t, rec = R[form]["records"]
        assert rec.shape == (NSTEPS, 3) and np.array_equal(t, times), form
        assert np.array_equal(rec, rec_ref), form
        assert R[form]["mon"] == (NSTEPS, dt, NSTEPS * dt), form
        for name in ("mon_max", "mon_cos"):
            assert np.array_equal(R[form][name], R["steps"][name]), (form, name)


@pytest.mark.parametrize("form", ("steps", "single"))
@pytest.mark.parametrize("kind,P,order", [(k, P, o) for k, P, t, o in CASES if t == "f64"])
def test_boundary_kernel_only_when_slots_are_stale(orc, kind, P, order, form):
    """The "boundary" profile scope counts the launches of k_boundary_partial.  RK4: stage_end leaves the next stage's
    boundary terms in the pseudo partial slots and predicts the next step's first stage time as t + dt, which the steps
    of both forms hit exactly: one launch, at the first stage after set_state.  RK2 has no such hand-over: one launch
    per stage, 2 x 5."""
    got = run(the_case(orc, kind, P, "f64", order), form, profile=True)["boundary"]
    assert got == (1 if order == 4 else 2 * NSTEPS)
