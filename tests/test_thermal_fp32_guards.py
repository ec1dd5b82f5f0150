"""CPU guards of the fp32 bioheat budget tests (test_gpu_thermal_fp32_budget.py; references only, no GPU).

For every case and stepper of thermal_fp32_cases.py: (a) the double reference's rise is live in every region, and the
run moved the start; (b) the yardstick is sane, yard(R) <= 128 x 2^-23 in every region, for the rise and for the heat
load -- a larger one would make the GPU assertion vacuous; (c) the float reference's own error in the max norm stays
below half of the fixed bound 1e-5 that the GPU tests assert beside the budget; (d) the float reference run with one small
change of the problem (thermal_fp32_cases.CONTROLS) lands above CAP_CEILING x yard(R) in at least one region, so the GPU
comparison sees such a mistake even when CAP sits at its ceiling.

The heat load is compared region by region like the rise but is not asked to be live against its own maximum: it is a
Gaussian of 2 mm around the centre of the box, h = m .* q is a product per DOF, and an error there stays at its DOF."""
import numpy as np
import pytest

import fp32_budget as fb
import thermal_fp32_cases as tc
from thermal_ref import rel
from util import assert_live

ULP = fb.EPS32


@pytest.mark.parametrize("name", list(tc.CASES))
def test_case_is_live_and_its_yardstick_sane(orc, name):
    cs = tc.case(orc, name)
    assert cs.h32.dtype == np.float32 and cs.bio32.m_c.dtype == np.float32 and cs.bio64.m_c.dtype == np.float64
    yard = fb.yardstick(cs.h32, cs.h64, cs.regions)
    print(f"fp32-yard [thermal-heat] {name}: {max(yard.values()) / ULP:.1f} ulp")
    assert max(yard.values()) <= fb.YARD_SANE, f"{name}/heat: yardstick above 128 ulp"
    for st in cs.steppers:
        sn = tc.stepper_name(st)
        r32, r64 = cs.refs(st)
        assert_live(r64, cs.regions)
        assert rel(r64, cs.th0.astype(np.float64)) > 1e-3                      # the run moved the state
        yard = fb.yardstick(r32, r64, cs.regions)
        worst = max(yard, key=yard.get)
        own = rel(r32, r64)
        print(f"fp32-yard [thermal] {name} {sn}: {yard[worst] / ULP:.1f} ulp at {worst}; max norm {own:.2e}")
        big = {k: y / ULP for k, y in yard.items() if y > fb.YARD_SANE}
        assert not big, f"{name} {sn}: yardstick above 128 ulp in {big}"
        assert own <= 0.5 * tc.TOL32
        if cs.bd is not None:       # the float reference holds the fixed values as the library does: bit for bit
            assert np.array_equal(r32[cs.bd.mask], cs.bd.rise[cs.bd.mask].astype(np.float32)) and cs.bd.mask.any()
            assert (cs.bio32.m_h > 0).any() and np.abs(cs.bd.rise[cs.bd.mask]).min() > 0.9


@pytest.mark.parametrize("name,stepper", tc.case_steppers(), ids=lambda v: v if isinstance(v, str) else tc.stepper_name(v))
def test_budget_at_its_ceiling_sees_the_controls(orc, name, stepper):
    cs = tc.case(orc, name)
    sn = tc.stepper_name(stepper)
    r32, r64 = cs.refs(stepper)
    for change in cs.controls():
        eps = None if change == "drop" else tc.EPS[change][sn]
        assert eps is None or eps <= tc.eps_limit(stepper)
        # the changed float reference in the role of the GPU result
        worst, where, table = fb.budget(cs.changed(stepper, change, eps), r32, r64, cs.regions)
        line = fb.report(f"[thermal-control] {name} {sn} {change} eps = {eps}", worst, where, table)
        print(line)
        assert worst > fb.CAP_CEILING, line


def test_float_restatement_rounds_where_the_library_does(orc):
    """The stage scalars of the float reference: dt is rounded to float before it meets a and b, the RKL2 scalars are
    formed in double and rounded once, 1 / m_C is a stored float vector.  Each is told from the other order by bits."""
    cs = tc.case(orc, "hex-p2-box")
    bio, th0, h = cs.bio32, cs.th0, cs.h32
    dt, f32 = cs.dt(0), np.float32
    k0 = (bio.b(th0) - bio.m_w * th0 + f32(1.0) * h) * (f32(1) / bio.m_c)
    assert np.array_equal(bio.f(th0, h), k0) and k0.dtype == np.float32
    assert not np.array_equal(k0, (bio.b(th0) - bio.m_w * th0 + h) / bio.m_c)     # the division rounds differently
    one = bio.step(th0, dt, h)
    assert one.dtype == np.float32
    acc, stage = th0.copy(), th0
    for a, b in zip((0.5, 0.5, 1.0, 0.0), (1.0 / 6.0, 1.0 / 3.0, 1.0 / 3.0, 1.0 / 6.0)):
        ki = bio.f(stage, h)
        acc = acc + f32(dt) * f32(b) * ki
        stage = th0 + f32(dt) * f32(a) * ki
    assert np.array_equal(one, acc)
    import sts_ref
    dts = cs.dt(3)
    mu, nu, mut, gat = sts_ref.coefficients(3)
    y0, f0 = th0, bio.f(th0, h)
    y1 = y0 + f32(mut[1] * dts) * f0
    y2 = f32(mu[2]) * y1 + f32(nu[2]) * y0 + f32(1.0 - mu[2] - nu[2]) * y0 + f32(mut[2] * dts) * bio.f(y1, h) + f32(gat[2] * dts) * f0
    y3 = f32(mu[3]) * y2 + f32(nu[3]) * y1 + f32(1.0 - mu[3] - nu[3]) * y0 + f32(mut[3] * dts) * bio.f(y2, h) + f32(gat[3] * dts) * f0
    got = sts_ref.step(bio, th0, dts, 3, h)
    assert got.dtype == np.float32 and np.array_equal(got, y3)
