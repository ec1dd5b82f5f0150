"""CPU guards of the live-start RK tests (oracle only, no GPU): the problems of test_gpu_live_state.py and the live
variants of the multi-rank tests stay comparisons that can fail.  For each problem: the reference is live (>= 1e-2
of its max) in every element layer, on every boundary face and on every interface plane; the oracle state stays
within 10x the start's max over the run; and a 1e-6 relative change of the far face's absorbing weight, of the last
layer's stiffness coefficient and (multi-rank) of the mass on either side of each cut moves the oracle state by at
least 100x the fp64 RK tolerance -- so the GPU comparison at that tolerance would see such a mistake.  (The fp32
cases here are guarded through their fp64 reference: their GPU comparison at a fixed fp32 tolerance is the weaker one
by construction.  The fp32 comparisons that see a 1e-4 mistake are those of test_gpu_fp32_budget.py, guarded by
test_fp32_guards.py.)"""
import numpy as np
import pytest

import test_multirank as mr
from live_cases import CASES, MR_CASES, TOL_RK, case, mr_case, mr_partitions
from util import assert_live, layer_and_face_regions, slab_interface_regions


def relmax(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


@pytest.mark.parametrize("name", list(CASES))
def test_single_rank_case_is_live_bounded_and_sensitive(orc, name):
    cs = case(orc, name)
    u0, v0 = cs.start()
    half = cs.oracle(u0, v0, nsteps=cs.nsteps // 2)
    u, v = cs.oracle(u0, v0)
    assert_live((u, v), cs.regions)
    for a, b in ((half[0], u0), (u, u0), (half[1], v0), (v, v0)):
        assert np.abs(a).max() < 10 * np.abs(b).max()
    for change in ("absb_far", "coef_last"):
        du = cs.oracle(u0, v0, change=change, eps=1e-6)
        assert max(relmax(du[0], u), relmax(du[1], v)) > 100 * TOL_RK, change
    # the negative control's change (1e-4 on a few far-corner cells) is far beyond the tolerance
    assert relmax(cs.oracle(u0, v0, scale_far_corner=1 + 1e-4)[0], u) > 100 * TOL_RK


@pytest.mark.parametrize("size", [2, 3])
def test_slab_problem_is_live_bounded_and_sensitive(orc, size):
    """test_multirank's slab problem from its live start (the in-process, external-transport, distinct-process and
    gloo variants)."""
    pr, m, u, v = mr.single_rank_reference(orc, "live")
    u0, v0 = mr.start_state(pr, "live")
    regions = {**layer_and_face_regions(pr), **slab_interface_regions(pr, size)}
    assert_live((u, v), regions)
    assert np.abs(u).max() < 10 * np.abs(u0).max() and np.abs(v).max() < 10 * np.abs(v0).max()
    layer = np.zeros(pr.ndofs, int)
    for i in range(pr.mesh.n[0]):
        layer[regions[f"layer{i}"]] = i
    for r in range(1, size):
        cut = (pr.mesh.n[0] * r) // size                # element layers [0, cut) left of the cut
        plane = np.zeros(pr.ndofs, bool)
        plane[regions[f"cut{r - 1}|{r}"]] = True
        for side in (layer < cut, layer >= cut):
            mask = side & ~plane
            _, _, du, dv = mr.single_rank_reference(orc, "live", mass_scale=(mask, 1 + 1e-6))
            assert max(relmax(du, u), relmax(dv, v)) > 100 * TOL_RK


def _plane_diff(a, b, idx):
    """The difference of the states a and b on the DOFs idx, relative to b's max: the smaller of u's and v's."""
    return min(np.abs(x[idx] - y[idx]).max() / np.abs(y).max() for x, y in zip(a, b))


@pytest.mark.parametrize("name", list(MR_CASES))
def test_multirank_case_is_live_bounded_and_sensitive(orc, name):
    """The cases of test_gpu_multirank_matrix.py, against the reference that file uses (the oracle's fixed step
    count): live in every layer, on every face and on every interface of every partition the case is run on; bounded;
    sensitive to the far face's absorbing weight, the last layer's coefficient and the mass on either side of each
    cut; and, for the orders 1-3, apart from the neighbouring orders' states on every interface -- a stage update
    of another order's table on the interface DOFs alone is then far above the tolerance."""
    cs = mr_case(orc, name)
    u0, v0 = cs.start()
    half = cs.oracle(u0, v0, nsteps=cs.nsteps // 2, fixed=True)
    u, v = cs.oracle(u0, v0, fixed=True)
    partitions = mr_partitions(cs, name)
    for label, planes, _ in partitions:
        assert all(len(idx) > 0 for idx in planes.values()), label
        assert_live((u, v), {**cs.regions, **planes})
    for a, b in ((half[0], u0), (u, u0), (half[1], v0), (v, v0)):
        assert np.abs(a).max() < 10 * np.abs(b).max()
    for change in ("absb_far", "coef_last"):
        du = cs.oracle(u0, v0, change=change, eps=1e-6, fixed=True)
        assert max(relmax(du[0], u), relmax(du[1], v)) > 100 * TOL_RK, change
    for label, _, sides in partitions:
        for k, mask in enumerate(sides):
            assert mask.any()
            du = cs.oracle(u0, v0, change=("mass", mask), eps=1e-6, fixed=True)
            assert max(relmax(du[0], u), relmax(du[1], v)) > 100 * TOL_RK, (label, k)
    if cs.order < 4:
        for other in (cs.order - 1, cs.order + 1):
            if 1 <= other <= 3:
                w = cs.oracle(u0, v0, order=other, fixed=True)
                for label, planes, _ in partitions:
                    for plane, idx in planes.items():
                        assert _plane_diff(w, (u, v), idx) > 100 * TOL_RK, (other, label, plane)
