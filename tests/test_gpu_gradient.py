"""The gradient / pair-product kernel and the intensity maps on the device (fusmi.h "gradient", "intensity") against the
numpy reference of gradient_ref.py.

(1) gradient and gradient_pairs against the reference, NODAL and WEIGHTED, on the smallest shapes at which the kernel can
go wrong; (2) analytic checks on the device result; (3) two halves joined on the host; (4) fus_model_intensity on the
monitor's maps, and what must not move; (5) arguments and call sequence; (6) the C++ example.

The error measure is fp32_budget.py's, per component and for the whole vector, rms / rms and max / max:
``err(gpu, ref_hi) <= CAP * max(err(ref_T, ref_hi), ulp_T)`` with ref_hi the reference in float64 (fp32 cases) or long
double (fp64 cases), ulp_T = 2^-23 or 2^-52, and CAP = fp32_budget.CAP_CEILING = 8, the project's stated condition."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import fenicsxfus_amd as fa
import gradient_ref
from fenicsxfus_amd import _abi, intensity, monitor
from fp32_budget import CAP_CEILING
from util import Problem, live_state

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAP = CAP_CEILING
H = 0.003                                    # cell size, m
F0, P0, S0 = 0.5e6, 6e4, 1500.0


def _bend(x):
    return x + np.c_[20.0 * x[:, 1] ** 2 - 12.0 * x[:, 2] ** 2, 15.0 * x[:, 2] ** 2, 0 * x[:, 0]]


def _bend2(x):
    return x + np.c_[20.0 * x[:, 1] ** 2, 12.0 * x[:, 0] ** 2]


def _hi(n):
    return [H * k for k in n]


# label -> (problem keywords, context keywords, fields)
CASES = {
    "a": (dict(n=(4, 3, 3), P=3, perturb=0.15), dict(block_elems=8), 1),                  # trilinear, several blocks
    "b8": (dict(n=(4, 3, 3), P=4), dict(block_elems=8), 1),                               # box: affine / diagonal metric
    "b64": (dict(n=(4, 3, 3), P=4), dict(block_elems=64), 1),                             # one block
    "c": (dict(n=(3, 2, 2), P=2, order=2, warp=_bend), dict(block_elems=8), 1),           # second-order cells, streamed
    "d7": (dict(n=(2, 2, 2), P=7, perturb=0.15), dict(block_elems=8), 1),                 # N = 8: a plane is one wave
    "d8": (dict(n=(2, 2, 1), P=8), dict(block_elems=8), 1),                               # more than 64 columns
    "e4": (dict(n=(5, 4), P=4, perturb=0.15), dict(block_elems=8), 1),                    # quadrilaterals, 357 DOFs
    "e4w": (dict(n=(6, 5), P=4, perturb=0.15), dict(block_elems=8), 1),                   # 525 DOFs: the vector tail is live
    "e2": (dict(n=(5, 4), P=2, perturb=0.15), dict(block_elems=8), 1),
    "eq2": (dict(quad2=True, n=(3, 2), P=3, warp=_bend2), dict(block_elems=4), 1),        # second-order quadrilaterals
    "f": (dict(n=(4, 3, 3), P=3, perturb=0.15, node_order=[2, 0, 3, 1]), dict(block_elems=8), 1),
    "ga": (dict(n=(4, 3, 3), P=3, perturb=0.15, dtype=np.float32), dict(block_elems=8), 1),
    "gb": (dict(n=(4, 3, 3), P=4, dtype=np.float32), dict(block_elems=8), 1),
    "ge": (dict(n=(5, 4), P=4, perturb=0.15, dtype=np.float32), dict(block_elems=8), 1),
    "gew": (dict(n=(6, 5), P=4, perturb=0.15, dtype=np.float32), dict(block_elems=8), 1),
    "h2": (dict(n=(4, 3, 3), P=3, perturb=0.15), dict(block_elems=8), 2),                 # LDS image sized for two fields
    "stream": (dict(n=(4, 3, 3), P=3, perturb=0.15), dict(block_elems=8, geometry="stream"), 1),
    "det": (dict(n=(4, 3, 3), P=3, perturb=0.15), dict(block_elems=8, deterministic=True), 1),
    # blocks of 19^3 = 6859 local DOFs: three fp64 accumulator images do not fit LDS together, one launch per component
    "cp6": (dict(n=(3, 3, 3), P=6, perturb=0.15), dict(block_elems=27), 1),
    "cp6f": (dict(n=(3, 3, 3), P=6, perturb=0.15, dtype=np.float32), dict(block_elems=27), 1),
    "cp9": (dict(n=(2, 2, 2), P=9), dict(block_elems=8), 1),
}
COMPONENT_PASSES = ("cp6", "cp6f", "cp9")


@functools.lru_cache(maxsize=None)
def _problem(orc, label):
    kw = dict(CASES[label][0])
    if kw.pop("quad2", False):
        return gradient_ref.Quad2Problem(orc, hi=_hi(kw["n"]), **kw)
    return Problem(orc, hi=_hi(kw["n"]), **kw)


@functools.lru_cache(maxsize=None)
def _refs(orc, label):
    """(reference in T, reference in the higher precision, one ulp of T) of a case: computed once, left unchanged."""
    pr = _problem(orc, label)
    hi = np.float64 if pr.dtype == np.float32 else np.longdouble
    return gradient_ref.of_problem(pr, pr.dtype, orc), gradient_ref.of_problem(pr, hi, orc), \
        (2.0 ** -23 if pr.dtype == np.float32 else 2.0 ** -52)


def _data(orc, label):
    pr = _problem(orc, label)
    ctx = fa.Context(0, **CASES[label][1])
    return pr, ctx, fa.SpectralOperatorData(pr.V, ctx, fields=CASES[label][2])


def _two_materials(pr, rows, lo=1.0, hi=2.5):
    """Per-cell coefficients that differ between two materials (a slab in x) and from row to row, in the problem's type."""
    cx = pr.mesh.cell_centroids()[:, 0]
    slab = cx > 0.5 * (cx.min() + cx.max())
    return np.array([np.where(slab, hi + 0.3 * k, lo / (1 + k)) for k in range(rows)]).astype(pr.dtype)


def _check(label, g, ref_T, ref_hi, ulp):
    worst, where, table = gradient_ref.budget(g, ref_T, ref_hi, ulp)
    e, y = table[where]
    line = f"gradient-budget {label}: ratio {worst:.3f} at {where} (err {e:.3e}, yard {y:.3e})"
    print(line)
    assert worst <= CAP, f"{line} exceeds CAP = {CAP}"
    return worst


# ---- (1) against the reference ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("label", list(CASES))
def test_gradient_and_pairs_against_the_reference(orc, label):
    """gradient (unit and two-material coefficients) and gradient_pairs (K = 1 and K = 3), NODAL and WEIGHTED -- the latter
    on a non-zero ``out``: it accumulates -- on live inputs (every DOF carries an O(1) value)."""
    pr, ctx, data = _data(orc, label)
    plan = data.gradient_plan()
    print(f"gradient-plan {label}: {plan}, {data.info()['max_local_dofs']} local DOFs in the largest block")
    if label in COMPONENT_PASSES:
        assert plan["launches"] == pr.tdim and plan["components"] == 1 and data.info()["max_local_dofs"] == 6859
    else:
        assert plan["launches"] == 1 and plan["components"] == pr.tdim
    assert plan["lds_bytes"] <= 160 * 1024
    rT, rH, ulp = _refs(orc, label)
    t = pr.dtype
    x = live_state(pr, 5, 1.0)[0]
    a = np.array([live_state(pr, 20 + k, 1.0)[0] for k in range(3)])
    b = np.array([live_state(pr, 30 + k, 1.0)[0] for k in range(3)])
    c1, c3 = _two_materials(pr, 1), _two_materials(pr, 3)
    base = (0.5 * np.abs(rT.gradient(x, nodal=False)).max() * np.sin(1.0 + np.arange(pr.tdim * pr.ndofs))).astype(t)
    base = base.reshape(pr.tdim, pr.ndofs)
    worst = 0.0
    # gradient
    for tag, coef in (("unit", None), ("two materials", c1[0])):
        g = data.gradient(x, coef)
        assert g.dtype == t and g.shape == (pr.tdim, pr.ndofs)
        worst = max(worst, _check(f"{label} gradient nodal, {tag}", g, rT.gradient(x, coef), rH.gradient(x, coef), ulp))
        out = base.copy()
        assert data.gradient(x, coef, nodal=False, out=out) is out
        worst = max(worst, _check(f"{label} gradient weighted, {tag}", out, base + rT.gradient(x, coef, nodal=False),
                                  base.astype(rH.dtype) + rH.gradient(x, coef, nodal=False), ulp))
    # pairs
    for K, coef in ((1, c1), (3, c3)):
        g = data.gradient_pairs(a[:K], b[:K], coef)
        worst = max(worst, _check(f"{label} pairs nodal, K = {K}", g, rT.gradient_pairs(a[:K], b[:K], coef),
                                  rH.gradient_pairs(a[:K], b[:K], coef), ulp))
        out = base.copy()
        data.gradient_pairs(a[:K], b[:K], coef, nodal=False, out=out)
        worst = max(worst, _check(f"{label} pairs weighted, K = {K}", out,
                                  base + rT.gradient_pairs(a[:K], b[:K], coef, nodal=False),
                                  base.astype(rH.dtype) + rH.gradient_pairs(a[:K], b[:K], coef, nodal=False), ulp))
    # the same call gives the same bits
    assert np.array_equal(data.gradient_pairs(a, b, c3), data.gradient_pairs(a, b, c3))
    print(f"gradient-budget {label}: largest ratio {worst:.3f}; {data.info()['nblocks']} blocks, mode {data.geometry_mode()}")
    data.close(), ctx.close()


def test_cases_reach_their_paths(orc):
    """The shapes above are what they are meant to be: several blocks with shared DOFs or one block, the geometry modes."""
    seen = {}
    for label in ("a", "b8", "b64", "c", "e4", "stream"):
        pr, ctx, data = _data(orc, label)
        info = data.info()
        seen[label] = (info["nblocks"], info["shared_dofs"], data.geometry_mode(), data.uses_diag_metric())
        data.close(), ctx.close()
    print(seen)
    assert seen["a"][0] > 1 and seen["a"][1] > 0 and seen["a"][2] == "trilinear"
    assert seen["b8"][0] > 1 and seen["b8"][2] == "affine" and seen["b8"][3]
    assert seen["b64"][0] == 1 and seen["b64"][1] == 0
    assert seen["c"][2] == "stream" and seen["e4"][2] == "stream" and seen["stream"][2] == "stream"
    assert _problem(orc, "e4").ndofs == 357 and _problem(orc, "e4w").ndofs == 525


# ---- (2) analytic checks on the device result ------------------------------------------------------------------------------
def test_polynomial_exactness_on_the_device(orc):
    """Case b (affine, P = 4): u = x^2 y - 3 z^3 + x y z is differentiated exactly -- the device result is as close to the
    analytic gradient as the float64 reference is, within CAP."""
    pr, ctx, data = _data(orc, "b8")
    X = pr.V.tabulate_dof_coordinates().astype(np.longdouble) / H      # in cell sizes: O(1) values
    x, y, z = X[:, 0], X[:, 1], X[:, 2]
    u = (x * x * y - 3 * z ** 3 + x * y * z).astype(np.float64)
    exact = np.array([2 * x * y + y * z, x * x + x * z, -9 * z * z + x * y]) / H
    g = data.gradient(u)
    eg = gradient_ref.errors(g, exact)
    er = gradient_ref.errors(_refs(orc, "b8")[0].gradient(u), exact)
    print("polynomial on the device:", {k: (eg[k], er[k]) for k in eg})
    for k in eg:
        assert eg[k] <= CAP * max(er[k], 2.0 ** -52), (k, eg[k], er[k])
    data.close(), ctx.close()


def test_plane_wave_intensity_on_the_device(orc):
    """(6, 2, 2) P = 6 box one wavelength long, a = A cos(kappa x), b = A sin(kappa x), coef = 1 / (2 rho w): the error of the
    device result against A^2 / (2 rho c) along x is at most twice that of the float64 reference against the same value."""
    A, rho, c = P0, 1000.0, S0
    lam = c / F0
    pr = Problem(orc, (6, 2, 2), 6, hi=[lam, lam / 3, lam / 3])
    ctx = fa.Context(0, block_elems=8)
    data = fa.SpectralOperatorData(pr.V, ctx)
    x = pr.V.tabulate_dof_coordinates()[:, 0]
    kap = 2 * np.pi / lam
    a, b = A * np.cos(kap * x), A * np.sin(kap * x)
    coef = intensity.intensity_coef(np.full(pr.mesh.num_cells, rho), F0, 1)
    want = np.zeros((3, pr.ndofs))
    want[0] = A * A / (2 * rho * c)
    err = lambda I: float(np.abs(I - want).max() / want[0, 0])   # noqa: E731
    eg = err(data.gradient_pairs(a, b, coef))
    er = err(gradient_ref.of_problem(pr, np.float64, orc).gradient_pairs(a, b, coef))
    print(f"plane wave: I0 {want[0, 0]:.6e} W/m^2, device error {eg:.3e}, float64 reference error {er:.3e}")
    assert 0 < er < 1e-4 and eg <= 2 * er
    data.close(), ctx.close()


# ---- (3) two halves ---------------------------------------------------------------------------------------------------------
def test_two_halves_sum_to_the_whole(orc):
    """Case a cut in two x-slabs, two operators in one process: the WEIGHTED sums and mass(1, 1) of each, added on the host
    over the interface, then divided, are the one-rank NODAL result within the budget."""
    kw = dict(CASES["a"][0])
    pr = _problem(orc, "a")
    rT, rH, ulp = _refs(orc, "a")
    x = live_state(pr, 5, 1.0)[0]
    a = np.array([live_state(pr, 20 + k, 1.0)[0] for k in range(3)])
    b = np.array([live_state(pr, 30 + k, 1.0)[0] for k in range(3)])
    c3 = _two_materials(pr, 3)
    num_g, num_p, den = np.zeros((3, pr.ndofs)), np.zeros((3, pr.ndofs)), np.zeros(pr.ndofs)
    cell0 = 0
    ctxs = [fa.Context(0, block_elems=8) for _ in range(2)]
    fa.Context.init_local_group(ctxs)                      # ranks 0 and 1 in one process; nothing is exchanged here
    for r, ctx in enumerate(ctxs):
        part = Problem(orc, hi=_hi(kw["n"]), rank=r, size=2, **kw)
        assert part.V.neighbours and part.V.neighbours[0][0] == 1 - r
        data = fa.SpectralOperatorData(part.V, ctx)
        ids = part.V.global_offset + np.arange(part.ndofs)
        cells = slice(cell0, cell0 + part.mesh.num_cells)          # slabs hold the global cells in order
        cell0 += part.mesh.num_cells
        assert np.allclose(part.V.tabulate_dof_coordinates(), pr.V.tabulate_dof_coordinates()[ids], rtol=0, atol=1e-15)
        num_g[:, ids] += data.gradient(x[ids], c3[0][cells], nodal=False)
        num_p[:, ids] += data.gradient_pairs(a[:, ids], b[:, ids], c3[:, cells], nodal=False)
        den[ids] += data.mass(np.ones(part.ndofs), np.ones(part.mesh.num_cells), np.zeros(part.ndofs))
        data.close()
    for ctx in ctxs:
        ctx.close()
    assert cell0 == pr.mesh.num_cells
    _check("two halves, gradient", num_g / den, rT.gradient(x, c3[0]), rH.gradient(x, c3[0]), ulp)
    _check("two halves, pairs K = 3", num_p / den, rT.gradient_pairs(a, b, c3), rH.gradient_pairs(a, b, c3), ulp)


# ---- (4) fus_model_intensity ------------------------------------------------------------------------------------------------
NHARM = 3


def _bone(pr):
    cx = pr.mesh.cell_centroids()[:, 0] / (H * pr.mesh.n[0])
    return (cx > 0.4) & (cx < 0.6)


def _wave_model(pr, ctx, westervelt=False, nharm=NHARM, which="u", steps=18):
    """The wave run of test_gpu_harmonic_heat.py: bone and tissue cells, live start, 18 steps, the monitor keeping nharm
    harmonics."""
    bone = _bone(pr)
    c = np.where(bone, 2800.0, 1500.0).astype(pr.dtype)
    rho = np.where(bone, 1850.0, 1000.0).astype(pr.dtype)
    dt = 0.5 * H / (2800.0 * pr.P ** 2)
    tags = fa.tag_box_boundary(pr.mesh)
    if westervelt:
        w0 = 2 * np.pi * F0
        delta = np.where(bone, fa.compute_diffusivity_of_sound(w0, 2800.0, 400.0 / 20.0 * np.log(10.0)),
                         fa.compute_diffusivity_of_sound(w0, 1500.0, 0.2)).astype(pr.dtype)
        beta = np.where(bone, 6.0, 3.5).astype(pr.dtype)
        mdl = fa.WesterveltSpectralExplicit(pr.mesh, tags, pr.P, c, rho, delta, beta, F0, P0, S0, 4, dt, V=pr.V, ctx=ctx)
    else:
        mdl = fa.LinearSpectralExplicit(pr.mesh, tags, pr.P, c, rho, F0, P0, S0, 4, dt, V=pr.V, ctx=ctx)
    u0, v0 = live_state(pr, 11, P0, F0)
    mdl.init()
    mdl.set_state(u0, v0)
    if nharm is not None:
        mdl.monitor(which=which, nharm=nharm, every=1)
    if steps:
        mdl.rk4_steps(0.0, dt, steps)
    return mdl, bone, c.astype(np.float64), rho.astype(np.float64)


def _wave_maps(mdl, nharm=NHARM):
    mdl._pull()
    out = {"u": mdl.u_n.x.array.copy(), "v": mdl.v_n.x.array.copy()}
    for q in ("max", "min", "mean", "rms"):
        out[q] = mdl.monitor_get(q).x.array.copy()
    for k in range(1, nharm + 1):
        out[f"cos{k}"] = mdl.monitor_get("cos", k).x.array.copy()
        out[f"sin{k}"] = mdl.monitor_get("sin", k).x.array.copy()
    return out


@pytest.mark.parametrize("label", ["a", "e4w", "ga"])
def test_model_intensity(orc, label):
    """Cases a (fp64), e (a Westervelt model on quadrilaterals, 525 DOFs) and g (fp32): intensity() over the three harmonics held and
    intensity(2), and radiation_force(rows), against the reference pair form on the PULLED maps; the wave state and every
    monitor map keep their bits; a second call returns the first call's bits; sampling goes on afterwards."""
    pr = _problem(orc, label)
    rT, rH, ulp = _refs(orc, label)
    t = pr.dtype
    ctx = fa.Context(0, block_elems=8, deterministic=True)
    mdl, bone, c, rho = _wave_model(pr, ctx, westervelt=label == "e4w")
    before = _wave_maps(mdl)
    I3 = mdl.intensity()
    I2 = mdl.intensity(2)
    rows = monitor.power_law(np.where(bone, 20.0, 0.5), 1.1, NHARM).astype(t)
    Fr = mdl.radiation_force(rows)
    F1 = mdl.radiation_force(rows[0])
    again = mdl.intensity()
    assert I3.dtype == t and I3.shape == (pr.ndofs, pr.tdim) and Fr.shape == I3.shape
    assert np.array_equal(I3, again)
    after = _wave_maps(mdl)
    for key in before:
        assert np.array_equal(before[key], after[key]), key
    cos = np.array([before[f"cos{k}"] for k in range(1, NHARM + 1)])
    sin = np.array([before[f"sin{k}"] for k in range(1, NHARM + 1)])
    ic = intensity.intensity_coef(rho, F0, NHARM).astype(t)
    fc = intensity.force_coef(rows.astype(np.float64), rho, c, F0).astype(t)
    for tag, got, K, coef in (("intensity, all three harmonics", I3, 3, ic), ("intensity(2)", I2, 2, ic[:2]),
                              ("radiation force, three rows", Fr, 3, fc), ("radiation force, fundamental", F1, 1, fc[:1])):
        _check(f"{label} {tag}", got.T, rT.gradient_pairs(cos[:K], sin[:K], coef), rH.gradient_pairs(cos[:K], sin[:K], coef), ulp)
    assert np.abs(I3 - I2).max() > 1e-6 * np.abs(I3).max()           # the third harmonic is live: leaving it out shows
    n0 = mdl.monitor_info()[0]
    mdl.rk4_steps(18 * mdl.dt, mdl.dt, 2)
    assert mdl.monitor_info()[0] == n0 + 2 and not np.array_equal(mdl.intensity(), I3)
    mdl.close(), ctx.close()


# ---- (5) arguments and call sequence ---------------------------------------------------------------------------------------
def _raises(code, name):
    return pytest.raises(fa.FusError, match=rf"error {code}: {name}")


def test_arguments(orc):
    pr, ctx, data = _data(orc, "a")
    L, H_ = _abi.lib(), C.c_int(_abi.FUS_HOST)
    nd, nc = pr.ndofs, pr.mesh.num_cells
    x, c, out = np.ones(nd), np.ones(nc), np.zeros((3, nd))
    p = _abi.ptr
    calls = {
        "fus_op_gradient": [lambda: L.fus_op_gradient(None, p(x), p(c), p(out), C.c_int(1), H_),
                            lambda: L.fus_op_gradient(data.h, None, p(c), p(out), C.c_int(1), H_),
                            lambda: L.fus_op_gradient(data.h, p(x), p(c), None, C.c_int(1), H_),
                            lambda: L.fus_op_gradient(data.h, p(x), p(c), p(out), C.c_int(2), H_),
                            lambda: L.fus_op_gradient(data.h, p(x), p(c), p(out), C.c_int(-1), H_),
                            lambda: L.fus_op_gradient(data.h, p(x), p(c), p(out), C.c_int(1), C.c_int(5))],
        "fus_op_gradient_pairs": [lambda: L.fus_op_gradient_pairs(None, C.c_int(1), p(x), p(x), p(c), p(out), C.c_int(1), H_),
                                  lambda: L.fus_op_gradient_pairs(data.h, C.c_int(1), None, p(x), p(c), p(out), C.c_int(1), H_),
                                  lambda: L.fus_op_gradient_pairs(data.h, C.c_int(1), p(x), None, p(c), p(out), C.c_int(1), H_),
                                  lambda: L.fus_op_gradient_pairs(data.h, C.c_int(1), p(x), p(x), None, p(out), C.c_int(1), H_),
                                  lambda: L.fus_op_gradient_pairs(data.h, C.c_int(1), p(x), p(x), p(c), None, C.c_int(1), H_),
                                  lambda: L.fus_op_gradient_pairs(data.h, C.c_int(0), p(x), p(x), p(c), p(out), C.c_int(1), H_),
                                  lambda: L.fus_op_gradient_pairs(data.h, C.c_int(9), p(x), p(x), p(c), p(out), C.c_int(1), H_),
                                  lambda: L.fus_op_gradient_pairs(data.h, C.c_int(1), p(x), p(x), p(c), p(out), C.c_int(3), H_)],
    }
    for name, fns in calls.items():
        for fn in fns:
            with _raises(-1, name):
                _abi.check(fn())
    assert not out.any()
    assert np.array_equal(data.gradient(x, None), data.gradient(x, c))          # NULL coefficients are ones
    data.close(), ctx.close()


def test_call_sequence(orc):
    pr = _problem(orc, "a")
    ctx = fa.Context(0, block_elems=8)
    L, H_ = _abi.lib(), C.c_int(_abi.FUS_HOST)
    out = np.zeros((3, pr.ndofs))
    name = "fus_model_intensity"
    mdl, bone, c, rho = _wave_model(pr, ctx, nharm=None, steps=2)
    with _raises(-4, name):                                           # monitor off
        mdl.intensity()
    with _raises(-4, name):
        mdl.intensity(1)
    mdl.monitor(which="v", nharm=2, every=1)
    mdl.rk4_steps(0.0, mdl.dt, 2)
    with _raises(-4, name):                                           # it watches v
        mdl.intensity()
    mdl.monitor(which="u", nharm=2, every=1)
    with _raises(-4, name):                                           # no sample yet
        mdl.intensity()
    mdl.rk4_steps(0.0, mdl.dt, 2)
    with _raises(-4, name):                                           # fewer harmonics held than asked for
        mdl.intensity(3)
    for nh in (0, 9):
        with _raises(-1, name):
            mdl.intensity(nh)
    with _raises(-1, name):
        _abi.check(L.fus_model_intensity(None, C.c_int(1), None, _abi.ptr(out), H_))
    with _raises(-1, name):
        _abi.check(L.fus_model_intensity(mdl.h, C.c_int(1), None, None, H_))
    bad = np.ones((2, pr.mesh.num_cells))
    bad[1, 3] = np.inf
    with _raises(-1, name):
        _abi.check(L.fus_model_intensity(mdl.h, C.c_int(2), _abi.ptr(bad), _abi.ptr(out), H_))
    assert not out.any()
    ok = mdl.intensity()                                              # and the model still answers
    assert np.isfinite(ok).all() and ok.any()
    mdl.close(), ctx.close()


def test_a_model_on_an_operator_with_neighbours_is_refused(orc):
    kw = dict(CASES["a"][0])
    ctxs = [fa.Context(0, block_elems=8) for _ in range(2)]
    fa.Context.init_local_group(ctxs)
    models = []
    for r, cx in enumerate(ctxs):
        part = Problem(orc, hi=_hi(kw["n"]), rank=r, size=2, **kw)
        nc = part.mesh.num_cells
        models.append(fa.LinearSpectralExplicit(part.mesh, fa.tag_box_boundary(part.mesh), part.P, np.full(nc, 1500.0),
                                                np.full(nc, 1000.0), F0, P0, S0, 4, 1e-8, V=part.V, ctx=cx))
    fa.group_finish_setup(models)
    for m in models:
        m.init()
        m.monitor(which="u", nharm=1, every=1)
    with _raises(-4, "fus_model_intensity"):
        models[0].intensity()
    x = np.ones(models[0].data.ndofs)                                  # the building block still works there
    assert np.isfinite(models[0].data.gradient(x, nodal=False)).all()
    for m in models:
        m.close()
    for cx in ctxs:
        cx.close()


# ---- (6) the C++ example ----------------------------------------------------------------------------------------------------
def test_cpp_intensity_example(tmp_path):
    """examples/cpp_intensity.cpp compiles against fusmi.hpp, runs, and prints the plane-wave value check (2) checks."""
    exe = str(tmp_path / "cpp_intensity")
    libdir = os.path.join(ROOT, "fenicsx-fus_amd", "fenicsxfus_amd")
    subprocess.run(["g++", "-std=c++17", "-O1", os.path.join(ROOT, "examples", "cpp_intensity.cpp"), "-I",
                    os.path.join(ROOT, "include"), "-L", libdir, "-lfusmi", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib",
                    "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    vals = dict(line.split("=") for line in r.stdout.split() if "=" in line)
    I0 = P0 * P0 / (2 * 1000.0 * S0)
    assert abs(float(vals["I0"]) - I0) <= 1e-12 * I0
    assert float(vals["err_x"]) <= 1e-4 and float(vals["transverse"]) <= 1e-4 and float(vals["velocity_err"]) <= 1e-4
