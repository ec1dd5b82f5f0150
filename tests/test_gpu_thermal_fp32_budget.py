"""The fp32 bioheat kernels held to the float reference's own rounding error (fp32_budget.py): k_thermal_stage,
k_thermal_sts_stage, k_thermal_robin, k_thermal_fix, k_thermal_if_stage, k_thermal_if_sts_stage and k_thermal_heat in
float, on the cases of thermal_fp32_cases.py -- every degree 2-10 on perturbed and box hexahedra, quadrilaterals,
second-order cells; RK4 and RKL2 of 2, 8 and 32 stages; a fixed and a convective face; two and three x-slabs in an
in-process group with and without a boundary that the interface cuts.

Every comparison is fb.check(label, (rise, heat load), r32, r64, regions): the GPU's error against the double reference on
the promoted float inputs may be at most CAP times the float reference's own, in every element layer, on every face (and
interface plane) and over the whole vector.  The fixed bound 1e-5 of the older fp32 thermal tests is asserted beside it.
The CPU guards (test_thermal_fp32_guards.py) show on the same cases that the references are live, that the yardstick is
sane and that the criterion sees a small mistake even at CAP's ceiling.  Every test prints, per stepper, its largest ratio
err(g, R) / yard(R) ("fp32-budget [thermal ...]") and the largest of either field ("fp32-field ...": pytest -s);
DESIGN.md section 2 holds the table measured on the MI355X."""
import numpy as np
import pytest

import fenicsxfus_amd as fa
import fp32_budget as fb
import test_gpu_thermal_multirank as multirank     # its boundary helper (imported as a module: no test is collected twice)
import thermal_fp32_cases as tc
from thermal_multirank_util import Group, assert_interfaces_identical, slab_parts, worst_rel
from thermal_ref import rel

pytestmark = pytest.mark.gpu


def family(cs, stepper):
    """The kernel family of a run, for the labels and the table of DESIGN.md."""
    where = "slabs" if cs.slabs else "one-rank"
    return f"{where}{'-bc' if cs.bd is not None else ''}-{'rk4' if stepper == tc.RK4 else 'rkl2'}"


def check(label, g, h, r32, r64, h32, h64, regions):
    """The budget on both fields in one call (its line names the larger ratio), then the largest ratio of either field:
    the heat load is the same vector for every stepper of a case and would otherwise hide the rise's."""
    _, _, table = fb.check(label, (g, h), (r32, h32), (r64, h64), regions)
    for f, what in (("u", "rise"), ("v", "heat")):
        k = max(table[f], key=lambda m: table[f][m][0] / table[f][m][1])
        e, y = table[f][k]
        print(f"fp32-field {label} {what}: ratio {e / y:.3f} at {k} (err {e:.3e}, yard {y:.3e})")


def advance(step, cs, stepper, one_call):
    for s, n in stepper:
        for _ in range(1 if one_call else n):
            step(cs.dt(s), n if one_call else 1, stages=s)


def run(cs, th, stepper, one_call=True):
    th.set_state(rise=cs.th0, dose=np.zeros(cs.prt.ndofs))
    advance(th.steps, cs, stepper, one_call)
    return th.rise().x.array.copy(), th.dose().x.array.copy()


def held(cs):
    return cs.bd.rise[cs.bd.mask].astype(np.float32)


@pytest.mark.parametrize("name", tc.PLAIN + tc.BOUNDARY)
def test_one_rank(orc, name):
    """deterministic=True: the budget on the rise and the heat load for every stepper of the case; one steps(dt, n)
    call and n calls of one step give the same bits in rise and dose; the fixed DOFs hold their float values."""
    cs = tc.case(orc, name)
    ctx = fa.Context(0, deterministic=True)
    th = cs.model(ctx)
    assert th.data.dtype == np.float32 and th.data.geometry_mode() == cs.expected_mode()
    th.init()
    h = th.heat().x.array.copy()
    assert h.dtype == np.float32
    for st in cs.steppers:
        r32, r64 = cs.refs(st)
        g, D = run(cs, th, st)
        assert g.dtype == np.float32 and D.dtype == np.float64 and D.min() > 0
        check(f"[thermal {family(cs, st)}] {name} {tc.stepper_name(st)} deterministic", g, h, r32, r64, cs.h32, cs.h64,
              cs.regions)
        assert rel(g, r64) <= tc.TOL32
        g1, D1 = run(cs, th, st, one_call=False)
        assert np.array_equal(g, g1) and np.array_equal(D, D1)
        if cs.bd is not None:
            assert np.array_equal(g[cs.bd.mask], held(cs))
    th.close(), ctx.close()


@pytest.mark.parametrize("name", ["hex-p4", "hex-p7", "hex-p9"])
def test_one_rank_default_context(orc, name):
    """The default context, where the operator's LDS atomics run free: the same budget."""
    cs = tc.case(orc, name)
    ctx = fa.Context(0)
    th = cs.model(ctx)
    assert th.data.dtype == np.float32 and th.data.geometry_mode() == cs.expected_mode()
    th.init()
    h = th.heat().x.array.copy()
    for st in cs.steppers:
        r32, r64 = cs.refs(st)
        g, _ = run(cs, th, st)
        check(f"[thermal {family(cs, st)}] {name} {tc.stepper_name(st)} default", g, h, r32, r64, cs.h32, cs.h64, cs.regions)
        assert rel(g, r64) <= tc.TOL32
    th.close(), ctx.close()


def run_group(cs, grp, stepper, one_call=True):
    grp.set_rise(cs.th0)
    for b in grp.bios:
        b.set_state(dose=np.zeros(b.data.ndofs))
    advance(grp.steps, cs, stepper, one_call)
    return grp.pull("rise"), grp.pull("dose")


@pytest.mark.parametrize("name", tc.SLABS)
def test_slabs(orc, name):
    """x-slabs in an in-process group (deterministic contexts): every rank's slice against the global references, the
    interface planes among the regions; rise, dose and heat load carry the same bits on every interface plane."""
    cs = tc.case(orc, name)
    parts = slab_parts(cs, cs.slabs)
    grp = Group(cs, parts)
    if cs.bd is not None:
        multirank._apply_boundary(grp, cs.bd)
    grp.finish()
    for b in grp.bios:
        b.init()
    h = grp.pull("heat")
    mine = []
    for p in parts:
        lo, k = p.gids[0], len(p.gids)
        assert np.array_equal(p.gids, lo + np.arange(k))
        own = {nm: idx[(idx >= lo) & (idx < lo + k)] - lo for nm, idx in cs.regions.items()}
        mine.append({nm: idx for nm, idx in own.items() if len(idx)})
        assert any(nm.startswith("cut") for nm in mine[-1])
    for st in cs.steppers:
        r32, r64 = cs.refs(st)
        got, D = run_group(cs, grp, st)
        for r, p in enumerate(parts):
            assert got[r].dtype == np.float32 and D[r].min() > 0
            check(f"[thermal {family(cs, st)}] {name} {tc.stepper_name(st)} rank {r}", got[r], h[r], r32[p.gids],
                  r64[p.gids], cs.h32[p.gids], cs.h64[p.gids], mine[r])
            if cs.bd is not None:
                m = cs.bd.mask[p.gids]
                assert m.any() and np.array_equal(got[r][m], cs.bd.rise[p.gids][m].astype(np.float32))
        assert worst_rel(cs, parts, got, r64) <= tc.TOL32
        assert_interfaces_identical(parts, got, D, h)
        again, D1 = run_group(cs, grp, st, one_call=False)
        for a, b in zip(got + D, again + D1):
            assert np.array_equal(a, b)
    grp.close()
