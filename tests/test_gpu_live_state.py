"""The fused RK stage path against the oracle from LIVE starts: u, v of O(1) on every DOF (live_state), the
time-dependent source on.  From the rest state the compared state is zero to rounding over most of the mesh after a
few steps, so a comparison at a relative tolerance never checks the stage epilogues of the far blocks, their boundary
lists or the pseudo-partial slots of their shared boundary DOFs.  Every test first asserts that the reference is live
in every element layer along x and on every boundary face (assert_live); the CPU guards (test_live_guards.py) show on
the same cases that the comparisons see a 1e-6 change of the far face's absorbing weight or of the last layer's
coefficient, and the negative controls here show that the library's state reaches the far corner."""
import ctypes as C

import numpy as np
import pytest

import fenicsxfus_amd as fa
from fenicsxfus_amd import _abi
from live_cases import TOL_F32_VS_F32, TOL_F32_VS_F64, TOL_RK, case
from util import assert_live

pytestmark = pytest.mark.gpu


def relmax(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def run_gpu(cs, ctx, u0, v0, **kw):
    model = cs.model(ctx, **kw)
    model.init()
    model.set_state(u0, v0)
    un, vn, _ = model.rk(0.0, cs.tf)
    assert model.nsteps == cs.nsteps
    out = un.x.array.copy(), vn.x.array.copy()
    model.close()
    return out


def check(got, ref, tol):
    assert relmax(got[0], ref[0]) < tol and relmax(got[1], ref[1]) < tol, (relmax(got[0], ref[0]),
                                                                            relmax(got[1], ref[1]))


def live_reference(orc, name):
    cs = case(orc, name)
    u0, v0 = cs.start()
    ref = cs.oracle(u0, v0)
    assert_live(ref, cs.regions)
    return cs, u0, v0, ref


GEOMETRY = {  # path -> (case suffix, context keywords, options, expected geometry mode)
    "stream": ("p4", dict(geometry="stream"), {}, "stream"),
    "trilinear": ("p4", dict(), {}, "trilinear"),
    "affine": ("p4-box", dict(), {"diag_metric": 0}, "affine"),
    "diag": ("p4-box", dict(), {"diag_metric": 1}, "affine"),
}


@pytest.mark.parametrize("path", list(GEOMETRY))
@pytest.mark.parametrize("kind", ["linear", "lossy", "westervelt"])
def test_models_every_geometry_path_lean_and_blocks(orc, kind, path):
    """P=4 on a 6 x 5 x 4 box, each geometry path, the lean stage kinds 4-7 and the accumulator form (0/1/3), with
    the default blocks and ragged 16-element blocks."""
    suffix, ckw, opts, mode = GEOMETRY[path]
    cs, u0, v0, ref = live_reference(orc, f"{kind}-{suffix}")
    for lean in (1, 0):
        for be in (None, 16):
            cx = fa.Context(0, block_elems=be, **ckw)
            cx.set_option("lean_rk4", lean)
            for k, val in opts.items():
                cx.set_option(k, val)
            model = cs.model(cx)
            assert model.data.geometry_mode() == mode
            if path in ("affine", "diag"):
                assert model.data.uses_diag_metric() == (path == "diag")
            model.close()
            check(run_gpu(cs, cx, u0, v0), ref, TOL_RK)
            cx.close()


@pytest.mark.parametrize("order", [1, 2, 3])
def test_lower_rk_orders(orc, order):
    cs, u0, v0, ref = live_reference(orc, f"linear-rk{order}")
    cx = fa.Context(0)
    check(run_gpu(cs, cx, u0, v0), ref, TOL_RK)
    cx.close()


@pytest.mark.parametrize("kind", ["linear", "lossy"])
def test_deterministic_stage_kernels_and_planes(orc, kind):
    """deterministic=1 (the stage kernels without atomics), the shared-DOF stage kernel reading planes (1), the CSR
    (0) and a plane limit of 4 (the CSR where more blocks share a DOF): each against the oracle."""
    cs, u0, v0, ref = live_reference(orc, f"{kind}-p4")
    for be in (None, 4):
        for planes in (1, 0, 4):
            cx = fa.Context(0, deterministic=1, block_elems=be)
            cx.set_option("planes", planes)
            check(run_gpu(cs, cx, u0, v0), ref, TOL_RK)
            cx.close()


@pytest.mark.parametrize("walk", [1, 2])
def test_walking_workgroups(orc, walk):
    cs, u0, v0, ref = live_reference(orc, "linear-walk")
    for geometry in (None, "stream"):
        cx = fa.Context(0, block_elems=4, geometry=geometry)
        cx.set_option("walk", walk)
        check(run_gpu(cs, cx, u0, v0), ref, TOL_RK)
        cx.close()


def test_graph_replay(orc):
    cs = case(orc, "linear-p4")
    u0, v0 = cs.start()
    ref = cs.oracle(u0, v0, exact=True)
    assert_live(ref, cs.regions)
    cx = fa.Context(0)
    cx.set_option("graph", 1)
    model = cs.model(cx)
    model.init()
    model.set_state(u0, v0)
    model.rk4_steps(0.0, cs.dt, cs.nsteps)
    check((model.u_sol().x.array.copy(), model.v_n.x.array.copy()), ref, TOL_RK)
    model.close()
    cx.close()


@pytest.mark.parametrize("name", ["linear-p2", "linear-p3", "linear-p5", "linear-p8", "westervelt-p8", "linear-p9",
                                  "westervelt-p9", "linear-p10", "westervelt-p10"])
def test_degrees(orc, name):
    """Perturbed first-order hexahedra: the trilinear kernels (degrees 8-10: elem_compute_hi on distorted cells)."""
    cs, u0, v0, ref = live_reference(orc, name)
    cx = fa.Context(0)
    model = cs.model(cx)
    assert cs.perturb > 0 and model.data.geometry_mode() == "trilinear"
    model.close()
    check(run_gpu(cs, cx, u0, v0), ref, TOL_RK)
    cx.close()


@pytest.mark.parametrize("P", [6, 7])
@pytest.mark.parametrize("mfma", [None, 0])
def test_degrees_6_7_mfma(orc, P, mfma):
    cs, u0, v0, ref = live_reference(orc, f"linear-p{P}")
    cx = fa.Context(0)
    if mfma is not None:
        cx.set_option("mfma", mfma)
    check(run_gpu(cs, cx, u0, v0), ref, TOL_RK)
    cx.close()


@pytest.mark.parametrize("P", [4, 6])
@pytest.mark.parametrize("pack32", [1, 0])
def test_fp32(orc, P, pack32):
    cs, u0, v0, ref = live_reference(orc, f"linear-p{P}-fp32")
    ref32 = cs.oracle(u0, v0, dtype=np.float32)
    cx = fa.Context(0)
    cx.set_option("pack32", pack32)
    got = run_gpu(cs, cx, u0, v0)
    assert got[0].dtype == np.float32
    check(got, ref32, TOL_F32_VS_F32)
    check(got, ref, TOL_F32_VS_F64)
    cx.close()


@pytest.mark.parametrize("name", ["linear-quad-p4", "westervelt-quad-p4", "linear-quad-p9", "westervelt-quad-p9"])
def test_quadrilaterals(orc, name):
    cs, u0, v0, ref = live_reference(orc, name)
    cx = fa.Context(0)
    check(run_gpu(cs, cx, u0, v0), ref, TOL_RK)
    cx.close()


def test_second_order_geometry(orc):
    cs, u0, v0, ref = live_reference(orc, "linear-q2")
    cx = fa.Context(0)
    check(run_gpu(cs, cx, u0, v0), ref, TOL_RK)
    cx.close()


@pytest.mark.parametrize("kind", ["linear", "westervelt"])
def test_set_state_mid_run(orc, kind):
    """k steps, a new live state through fus_model_set, then on: the oracle restarted from the new state.  The
    pseudo-partial slots that the last stage left for the next step are stale after the set (bnd_valid)."""
    cs = case(orc, f"{kind}-p4")
    u0, v0 = cs.start()
    k = 4
    u1, v1 = cs.start(seed=cs.seed + 1)
    ref = cs.oracle(u1, v1, t0=k * cs.dt, exact=True)
    assert_live(ref, cs.regions)
    for lean in (1, 0):
        cx = fa.Context(0)
        cx.set_option("lean_rk4", lean)
        model = cs.model(cx)
        model.init()
        model.set_state(u0, v0)
        model.rk4_steps(0.0, cs.dt, k)
        model.set_state(u1, v1)
        model.rk4_steps(k * cs.dt, cs.dt, cs.nsteps)
        check((model.u_sol().x.array.copy(), model.v_n.x.array.copy()), ref, TOL_RK)
        # only u set: v keeps the state the run left
        model.set_state(u1)
        v_left = model.v_n.x.array.copy()
        model.rk4_steps(0.0, cs.dt, 3)
        ref2 = cs.oracle(u1, v_left, nsteps=3, exact=True)
        check((model.u_sol().x.array.copy(), model.v_n.x.array.copy()), ref2, TOL_RK)
        model.close()
        cx.close()


def test_rk_order_switch_between_steps(orc):
    """fus_model_set_rk_order between steps: 4 -> 2 -> 4, against the oracle run in the same three legs."""
    cs = case(orc, "linear-rk2")
    u, v = cs.start()
    legs = ((4, 6), (2, 6), (4, 6))
    t = 0.0
    ru, rv = u.copy(), v.copy()
    for order, ns in legs:
        ru, rv = cs.oracle(ru, rv, t0=t, nsteps=ns, order=order, exact=True)
        t += ns * cs.dt
    assert_live((ru, rv), cs.regions)
    cx = fa.Context(0)
    model = cs.model(cx, order=4)
    model.init()
    model.set_state(u, v)
    t = 0.0
    for order, ns in legs:
        _abi.check(_abi.lib().fus_model_set_rk_order(model.h, C.c_int(order)))
        model.rk4_steps(t, cs.dt, ns)
        t += ns * cs.dt
    check((model.u_sol().x.array.copy(), model.v_n.x.array.copy()), (ru, rv), TOL_RK)
    model.close()
    cx.close()


def test_two_models_on_one_op(orc, monkeypatch):
    """Two Linear models created on ONE fus_op (different materials, different live starts), stepped in turn: each
    must match its own oracle run.  The pseudo-partial slots of the shared boundary DOFs live in the op and belong to
    one model at a time (bnd_owner)."""
    cs = case(orc, "linear-p4")
    cx = fa.Context(0, block_elems=16)
    data = fa.SpectralOperatorData(cs.pr.V, cx)
    monkeypatch.setattr(fa.models, "SpectralOperatorData", lambda V, ctx, fields=1: data)
    a = cs.model(cx)
    b = cs.model(cx, scale_far_corner=1.5)        # another material in the far corner
    assert a.data is b.data
    starts = [cs.start(seed=11), cs.start(seed=12)]
    refs = [cs.oracle(*starts[0], exact=True), cs.oracle(*starts[1], scale_far_corner=1.5, exact=True)]
    for r in refs:
        assert_live(r, cs.regions)
    for mdl, (u0, v0) in zip((a, b), starts):
        mdl.init()
        mdl.set_state(u0, v0)
    for s in range(cs.nsteps):                      # in turn, step by step
        for mdl in (a, b):
            mdl.rk4_steps(s * cs.dt, cs.dt, 1)
    for mdl, r in zip((a, b), refs):
        check((mdl.u_sol().x.array.copy(), mdl.v_n.x.array.copy()), r, TOL_RK)
    assert relmax(refs[0][0], refs[1][0]) > 1e-3
    for mdl in (a, b):
        _abi.lib().fus_model_destroy(mdl.h)
        mdl.h = C.c_void_p()
    data.close()
    cx.close()


@pytest.mark.parametrize("kind", ["linear", "lossy", "westervelt", "linear-p6-box", "lossy-p7", "westervelt-p9-box",
                                  "lossy-rk2"])
def test_negative_control_far_corner(orc, kind):
    """The GPU model with its family's coefficient (c0 / delta / beta) of the far-corner cells scaled by 1 + 1e-4
    must FAIL the comparison with the unchanged oracle by more than 100x the tolerance: the live start, set_state and
    the comparison reach those DOFs.  A family alone: its p=4 case; the named cases: one per path of
    test_gpu_live_matrix.py (a box, two operator inputs at the degrees 7 and 9, a lower RK order)."""
    cs, u0, v0, ref = live_reference(orc, kind if "-" in kind else f"{kind}-p4")
    cx = fa.Context(0)
    got = run_gpu(cs, cx, u0, v0, scale_far_corner=1 + 1e-4)
    assert relmax(got[0], ref[0]) > 100 * TOL_RK
    check(got, cs.oracle(u0, v0, scale_far_corner=1 + 1e-4), TOL_RK)
    cx.close()
