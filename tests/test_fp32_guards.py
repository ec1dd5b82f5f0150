"""CPU guards of the fp32 budget tests (test_gpu_fp32_budget.py; oracle only, no GPU).

The oracle's fixed step count: for double it reproduces the tf-driven loop bit for bit, and the float instantiation
takes the steps it is asked for (its tf-driven loop, with t in float, does not).

For every model-run case of the GPU tests: (a) the double reference is live in every region; (b) the yardstick is
sane, yard(R) <= 128 x 2^-23 in every region and field -- a larger one would make the GPU assertion vacuous; (c) a
1e-4 relative change of the far face's absorbing weight and of the last element layer's coefficient moves the
reference by at least 2 x 8 x yard(R) in at least one (region, field), so the GPU comparison still sees a 1e-4
mistake with headroom when CAP sits at its ceiling of 8."""
import copy

import numpy as np
import pytest

import fp32_budget as fb
from live_cases import FP32_LONG, FP32_RUNS, FP32_SLABS, FP32_SLABS_RK3, FP32_WALK, case, fp32_case
from util import assert_live, slab_interface_regions


@pytest.mark.parametrize("name", ["linear-p4", "lossy-p4", "westervelt-p4", "linear-rk2", "linear-quad-p4",
                                  "westervelt-p8"])
def test_fixed_step_count_reproduces_the_tf_loop_in_double(orc, name):
    """With dt a power of two and tf = t0 + nsteps dt the tf-driven loop takes nsteps FULL steps (every t and tf - t
    is exact); with the usual tf = nsteps dt (1 - 1e-9) its last step is shorter than dt, and the two differ."""
    cs = copy.copy(case(orc, name))
    cs.dt = 2.0 ** np.floor(np.log2(cs.dt))
    u0, v0 = cs.start()
    for t0 in (0.0, 3 * cs.dt):
        a = cs.oracle(u0, v0, t0=t0, margin=0.0)         # asserts that it took cs.nsteps steps
        b = cs.oracle(u0, v0, t0=t0, fixed=True)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        short = cs.oracle(u0, v0, t0=t0)
        assert not np.array_equal(short[1], b[1]) and np.abs(short[1] - b[1]).max() < 1e-6 * np.abs(b[1]).max()
    z = cs.oracle(u0, v0, nsteps=0, fixed=True)
    assert np.array_equal(z[0], u0) and np.array_equal(z[1], v0)


@pytest.mark.parametrize("name", ["linear-p3", "lossy-p6", "westervelt-p8"])
def test_fixed_step_count_in_float_composes(orc, name):
    """Float: k then n - k steps (the second leg started at t0 = k dt) are the n steps of one call, bit for bit --
    the loop time is advanced by dt in double, not in float."""
    cs = fp32_case(orc, name)
    (u0, v0), _, _ = cs.fp32_refs()
    whole = cs.oracle(u0, v0, dtype=np.float32, fixed=True)
    k = cs.nsteps // 2
    half = cs.oracle(u0, v0, dtype=np.float32, fixed=True, nsteps=k)
    t0 = 0.0
    for _ in range(k):
        t0 += cs.dt
    rest = cs.oracle(*half, dtype=np.float32, fixed=True, nsteps=cs.nsteps - k, t0=t0)
    assert np.array_equal(whole[0], rest[0]) and np.array_equal(whole[1], rest[1])
    assert not np.array_equal(whole[0], half[0])


def _regions(cs, name):
    slabs = name in FP32_SLABS or name in FP32_SLABS_RK3
    return {**cs.regions, **slab_interface_regions(cs.pr, 2)} if slabs else cs.regions


@pytest.mark.parametrize("name", list(FP32_RUNS) + list(FP32_LONG) + list(FP32_SLABS) + list(FP32_SLABS_RK3)
                         + list(FP32_WALK))
def test_case_is_live_and_its_yardstick_sane(orc, name):
    cs = fp32_case(orc, name)
    (u0, v0), r32, r64 = cs.fp32_refs()
    regions = _regions(cs, name)
    assert_live(r64, regions)
    if name in FP32_LONG:     # bounded over the long run (measured: 1.70 |u0|, 0.83 |v0|)
        assert np.abs(r64[0]).max() <= 2.5 * np.abs(u0).max() and np.abs(r64[1]).max() <= np.abs(v0).max()
    for f, r in (("u", 0), ("v", 1)):
        yard = fb.yardstick(r32[r], r64[r], regions)
        big = {k: y for k, y in yard.items() if y > fb.YARD_SANE}
        assert not big, f"{name}/{f}: yardstick above 128 ulp in {big}"


@pytest.mark.parametrize("name", list(FP32_RUNS) + list(FP32_LONG) + list(FP32_SLABS_RK3) + list(FP32_WALK))
@pytest.mark.parametrize("change", ["absb_far", "coef_last"])
def test_budget_at_its_ceiling_sees_a_1e4_mistake(orc, name, change):
    cs = fp32_case(orc, name)
    _, r32, r64 = cs.fp32_refs()
    _, _, d64 = cs.fp32_refs(change=change, eps=1e-4)
    # the changed reference in the role of the GPU result
    worst, where, table = fb.budget(d64, r32, r64, cs.regions)
    assert worst >= 2 * fb.CAP_CEILING, fb.report(f"{name} {change}", worst, where, table)


def test_cap_follows_the_rule():
    assert fb.CAP in (2, 4, 8) and fb.CAP <= fb.CAP_CEILING
