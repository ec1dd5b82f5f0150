"""Which block kernel an operator runs (csrc/block_variant.hpp), on the device: for every degree at which the choice
changes (4: no special variant; 5, 6, 7: packed fp32, matrix-core, diagonal metric; 8: two waves per element), both
scalar types, three meshes and the options that steer the choice, the operator reports what
tests/block_variant_ref.py -- the former flag expressions and launch cascade -- predicts from its facts, and the kernel
that then runs gives the oracle's stiffness and mass actions.  3 x 2 x 2 cells: an odd number, so the packed kernel's
last pair is a lone element.  fp64: the bounds of test_gpu_parity.py; fp32: fp32_budget.check as
test_gpu_fp32_budget.py::test_operator_actions applies it."""
import functools

import numpy as np
import pytest

import block_variant_ref as ref
import fenicsxfus_amd as fa
import fp32_budget as fb
from util import Problem, assert_live, layer_and_face_regions

pytestmark = pytest.mark.gpu

TOL_OP, TOL_MASS = 1e-12, 1e-14   # test_gpu_parity.py
# every coordinate is a multiple of 1/4 and the shear keeps it one: exact in float, so the affinity test sees exact parallelepipeds
HI3 = [0.75, 0.5, 0.5]
MESHES = {"box": (ref.AFFINE, True), "sheared": (ref.AFFINE, False), "perturbed": (ref.TRILINEAR, False)}
# label -> (context keywords, options); what the reference is told: (deterministic, mfma, pack32, diag_metric, stream)
OPTION_SETS = {
    "default": ({}, {}),
    "mfma=1": ({}, dict(mfma=1)),
    "pack32=1": ({}, dict(pack32=1)),
    "pack32=0": ({}, dict(pack32=0)),
    "diag_metric=0": ({}, dict(diag_metric=0)),
    "deterministic=1": (dict(deterministic=1), {}),
    "geometry=stream": (dict(geometry="stream"), {}),
}


def relmax(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def _recompute_geometry(orc, pr):
    pr.G, pr.detJ = orc.geometry(pr.tdim, pr.mesh.geometry.x, pr.mesh.geometry.dofmap, pr.nodes, pr.wts, dtype=pr.dtype)


@functools.lru_cache(maxsize=None)
def _case(orc, n, P, dtype, mesh):
    """The problem, its inputs and the oracle's actions, computed once per (shape, degree, type, mesh)."""
    dtype = np.dtype(dtype)
    hi = HI3 if len(n) == 3 else [1.0, 0.75]
    pr = Problem(orc, n, P, hi=hi, perturb=0.2 if mesh == "perturbed" else 0.0, dtype=dtype)
    if mesh == "sheared":   # affine, edges not orthogonal
        x = pr.mesh.geometry.x.copy()
        x[:, 0] += 0.5 * x[:, 1] + 0.25 * x[:, 2]
        pr.mesh.geometry.x = np.ascontiguousarray(x, dtype=dtype)
        _recompute_geometry(orc, pr)
    rng = np.random.default_rng(P)
    x = rng.standard_normal(pr.ndofs).astype(dtype)
    coef = rng.uniform(0.5, 2.0, pr.mesh.num_cells).astype(dtype)
    y0 = rng.standard_normal(pr.ndofs)
    if dtype == np.float64:
        return pr, x, coef, {op: (y0, None, None, None) for op in ("stiffness", "mass")}
    pr64 = fb.promoted(orc, pr)
    regions = layer_and_face_regions(pr64)
    t, N, out = pr.tdim, pr.N, {}
    for op in ("stiffness", "mass"):
        refs = {}
        for dt_, p in ((np.float64, pr64), (np.float32, pr)):
            if op == "stiffness":
                act = lambda y: orc.stiffness(t, N, p.dm, p.G, p.D, coef.astype(dt_), x.astype(dt_), y, dtype=dt_)  # noqa
            else:
                act = lambda y: orc.mass(t, N, p.dm, p.detJ, coef.astype(dt_), x.astype(dt_), y, dtype=dt_)  # noqa
            if dt_ == np.float64:     # the start vector: a quarter of the action's rms, in float
                scale = 0.25 * np.sqrt(np.mean(act(np.zeros(p.ndofs)) ** 2))
                y_start = (scale * y0).astype(np.float32)
            refs[dt_] = act(y_start.astype(dt_))
        assert_live(refs[np.float64], regions)
        out[op] = (y_start, refs[np.float32], refs[np.float64], regions)
    return pr, x, coef, out


def _check_actions(label, d, pr, x, coef, refs):
    for op in ("stiffness", "mass"):
        y_start, r32, r64, regions = refs[op]
        if pr.dtype == np.float64:
            want = y_start + (pr.K(x, coef) if op == "stiffness" else pr.M(x, coef))
            assert relmax(getattr(d, op)(x, coef, y_start.copy()), want) < (TOL_OP if op == "stiffness" else TOL_MASS), (label, op)
        else:
            g = getattr(d, op)(x, coef, y_start.copy())
            assert g.dtype == np.float32
            fb.check(f"[variant-{op}] {label}", g, r32, r64, regions)


def _reported(d):
    return dict(geometry_mode=("stream", "affine", "trilinear").index(d.geometry_mode()), uses_mfma=int(d.uses_mfma()),
                uses_pack32=int(d.uses_pack32()), uses_diag_metric=int(d.uses_diag_metric()), uses_mfma4=int(d.uses_mfma4()))


@pytest.mark.parametrize("mesh", list(MESHES))
@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("P", [4, 5, 6, 7, 8])
def test_reported_variant_and_actions(orc, P, dtype, mesh):
    pr, x, coef, refs = _case(orc, (3, 2, 2), P, dtype, mesh)
    nbytes = np.dtype(dtype).itemsize
    seen = set()
    for label, (ckw, opts) in OPTION_SETS.items():
        mode, ortho = MESHES[mesh] if ckw.get("geometry") != "stream" else (ref.STREAM, False)
        want = ref.introspection(P, nbytes, 3, mode, ortho, bool(ckw.get("deterministic", 0)), opts.get("mfma", -1),
                                 opts.get("pack32", -1), opts.get("diag_metric", 1))
        cx = fa.Context(0, **ckw)
        for k, v in opts.items():
            cx.set_option(k, v)
        d = fa.SpectralOperatorData(pr.V, cx)
        assert d.dtype == np.dtype(dtype)
        assert _reported(d) == want, (label, _reported(d), want)
        _check_actions(f"p{P} {dtype} {mesh} {label}", d, pr, x, coef, refs)
        seen.add(tuple(sorted(want.items())))
        d.close()
        cx.close()
    assert len(seen) >= 2   # the option sets do reach different kernels (at the least: a per-cell and the streamed one)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("P", [4, 8])
def test_quadrilaterals_take_the_streamed_kernel(orc, P, dtype):
    pr, x, coef, refs = _case(orc, (4, 3), P, dtype, "perturbed")
    want = ref.introspection(P, np.dtype(dtype).itemsize, 2, ref.STREAM, False, False)
    assert not any(want[k] for k in want)
    cx = fa.Context(0)
    d = fa.SpectralOperatorData(pr.V, cx)
    assert _reported(d) == want
    _check_actions(f"quad p{P} {dtype}", d, pr, x, coef, refs)
    d.close()
    cx.close()
