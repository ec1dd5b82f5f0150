"""The fp32 kernels held to the float oracle's own rounding error (fp32_budget.py): operator actions and model runs
of every family and degree, the options, a longer run and two x-slabs, all from live starts; the GPU is driven with
set_state + rk4_steps (exact steps) and both oracles run the same fixed number of steps.  The CPU guards
(test_fp32_guards.py) show on the same cases that the references are live, that the yardstick is sane and that the
criterion sees a 1e-4 mistake even at CAP's ceiling.  Every test prints its largest ratio err(g, R) / yard(R) and
where it occurred (pytest -s); DESIGN.md section 2 holds the table measured on the MI355X, from which CAP follows.

Nothing is left out silently.  REJECTED lists what the library refuses by design; YIELDS lists option combinations
that are no errors but in which one option gives way to another -- those are asserted through uses_*()."""
import numpy as np
import pytest

import fenicsxfus_amd as fa
import fp32_budget as fb
from live_cases import FP32_RUNS, KINDS, fp32_case
from util import Problem, assert_live, layer_and_face_regions, slab_interface_regions

pytestmark = pytest.mark.gpu

# combination -> the error text the library gives (test_gpu_high_degree.py::test_unsupported_combinations_are_errors)
REJECTED = {"degree 11 (any dtype)": "unsupported polynomial degree (2..10)"}
# no errors: the first option gives way, so these are no cases of their own
YIELDS = {
    "pack32=1 with deterministic=1": "packed kernels accumulate with LDS atomics: uses_pack32() is False",
    "pack32=1 with mfma=1": "the matrix-core variants have no packed form: uses_pack32() is False",
    "mfma=1 with deterministic=1": "the matrix-core variants accumulate with LDS atomics: uses_mfma() is False",
    "diag_metric=1 with pack32=1 or mfma=1": "the diagonal-metric form is a scalar kernel: uses_diag_metric() is False",
    "diag_metric=1 at degrees 8-10": "no diagonal-metric form of elem_compute_hi: uses_diag_metric() is False",
    "walk=1 with geometry=stream or on quadrilaterals": "the streamed-geometry kernel keeps one workgroup per block",
}


def test_rejected_combination_gives_its_error(orc):
    c = fa.Context(0)
    p11 = Problem(orc, (1, 1, 1), 11, dtype=np.float32)
    with pytest.raises(fa.FusError, match=r"unsupported polynomial degree \(2\.\.10\)"):
        fa.SpectralOperatorData(p11.V, c)
    c.close()


def context(ckw=None, opts=None):
    cx = fa.Context(0, **(ckw or {}))
    for k, v in (opts or {}).items():
        cx.set_option(k, v)
    return cx


# ---- 1. operator actions ------------------------------------------------------------------------------------------------
def _bend(x):
    return x + np.c_[20.0 * x[:, 1] ** 2 - 12.0 * x[:, 2] ** 2, 15.0 * x[:, 2] ** 2, 0 * x[:, 0]]


L3 = [0.012, 0.012, 0.012]
OPS = {}   # name -> (Problem keywords, context keywords, options, expected (mode, pack32, diag, mfma))
for _P in range(2, 11):
    _n = (3, 3, 3) if _P <= 7 else (2, 2, 2)          # 27 cells: the packed kernels' last pair is a lone element
    _pk_auto = _P == 5                                  # auto: degree 5, and degree 6 on affine cells
    OPS[f"trilinear-p{_P}"] = (dict(n=_n, P=_P, hi=L3, perturb=0.2), {}, {}, ("trilinear", _pk_auto, False, False))
    OPS[f"trilinear-det-p{_P}"] = (dict(n=_n, P=_P, hi=L3, perturb=0.2), dict(deterministic=1), {},
                                   ("trilinear", False, False, False))
    OPS[f"stream-p{_P}"] = (dict(n=_n, P=_P, hi=L3, perturb=0.2), dict(geometry="stream"), {},
                            ("stream", False, False, False))
    for _dm in (1, 0):
        OPS[f"box-diag{_dm}-p{_P}"] = (dict(n=_n, P=_P, hi=L3), {}, dict(diag_metric=_dm, pack32=0, mfma=0),
                                       ("affine", False, bool(_dm) and _P <= 7, False))
    OPS[f"box-det-p{_P}"] = (dict(n=_n, P=_P, hi=L3), dict(deterministic=1), {}, ("affine", False, _P <= 7, False))
for _P in (5, 6, 7):
    for _pk in (1, 0):
        OPS[f"trilinear-pack{_pk}-p{_P}"] = (dict(n=(3, 3, 3), P=_P, hi=L3, perturb=0.2), {}, dict(pack32=_pk),
                                             ("trilinear", bool(_pk), False, False))
        OPS[f"box-pack{_pk}-p{_P}"] = (dict(n=(3, 3, 3), P=_P, hi=L3), {}, dict(pack32=_pk, diag_metric=0),
                                       ("affine", bool(_pk), False, False))
for _P in (6, 7):
    OPS[f"trilinear-mfma-p{_P}"] = (dict(n=(3, 3, 3), P=_P, hi=L3, perturb=0.2), {}, dict(mfma=1),
                                    ("trilinear", False, False, True))
    OPS[f"box-mfma-p{_P}"] = (dict(n=(3, 3, 3), P=_P, hi=L3), {}, dict(mfma=1), ("affine", False, False, True))
for _P in (4, 9):
    OPS[f"q2-p{_P}"] = (dict(n=(3, 2, 2), P=_P, hi=[0.012, 0.008, 0.008], order=2, warp=_bend), {}, {},
                        ("stream", False, False, False))
    OPS[f"q2-det-p{_P}"] = (dict(n=(3, 2, 2), P=_P, hi=[0.012, 0.008, 0.008], order=2, warp=_bend),
                            dict(deterministic=1), {}, ("stream", False, False, False))
    _nq = (9, 7) if _P == 4 else (4, 3)
    OPS[f"quad-p{_P}"] = (dict(n=_nq, P=_P, hi=[0.012, 0.012 * _nq[1] / _nq[0]], perturb=0.2), {}, {},
                          ("stream", False, False, False))
    OPS[f"quad-det-p{_P}"] = (dict(n=_nq, P=_P, hi=[0.012, 0.012 * _nq[1] / _nq[0]], perturb=0.2),
                              dict(deterministic=1), {}, ("stream", False, False, False))


@pytest.mark.parametrize("name", list(OPS))
def test_operator_actions(orc, name):
    """y += K(c) x and y += M(c) x, random x and per-cell coefficients in [0.5, 2], from a non-zero y."""
    pkw, ckw, opts, (mode, pk, diag, mfma) = OPS[name]
    pkw = dict(pkw)
    pr32 = Problem(orc, pkw.pop("n"), pkw.pop("P"), dtype=np.float32, **pkw)
    pr64 = fb.promoted(orc, pr32)
    regions = layer_and_face_regions(pr64)
    rng = np.random.default_rng(pr32.P)
    x = rng.standard_normal(pr32.ndofs).astype(np.float32)
    coef = rng.uniform(0.5, 2.0, pr32.mesh.num_cells).astype(np.float32)
    y0 = rng.standard_normal(pr32.ndofs)
    cx = context(ckw, opts)
    d = fa.SpectralOperatorData(pr32.V, cx)
    assert d.dtype == np.float32
    assert (d.geometry_mode(), d.uses_pack32(), d.uses_diag_metric(), d.uses_mfma()) == (mode, pk, diag, mfma)
    t, N = pr32.tdim, pr32.N
    for op in ("stiffness", "mass"):
        refs = {}
        for dt_, pr in ((np.float64, pr64), (np.float32, pr32)):
            if op == "stiffness":
                act = lambda y: orc.stiffness(t, N, pr.dm, pr.G, pr.D, coef.astype(dt_), x.astype(dt_), y, dtype=dt_)  # noqa
            else:
                act = lambda y: orc.mass(t, N, pr.dm, pr.detJ, coef.astype(dt_), x.astype(dt_), y, dtype=dt_)  # noqa
            if dt_ == np.float64:     # the start vector: a quarter of the action's rms, in float
                scale = 0.25 * np.sqrt(np.mean(act(np.zeros(pr.ndofs)) ** 2))
                y_start = (scale * y0).astype(np.float32)
            refs[dt_] = act(y_start.astype(dt_))
        assert_live(refs[np.float64], regions)
        g = getattr(d, op)(x, coef, y_start.copy())
        assert g.dtype == np.float32
        fb.check(f"[op-{op}] {name}", g, refs[np.float32], refs[np.float64], regions)
    d.close()
    cx.close()


# ---- model runs ---------------------------------------------------------------------------------------------------------
def run_gpu(cs, cx, start, nsteps=None, expect=None, **kw):
    model = cs.model(cx, **kw)
    assert model.data.dtype == np.float32
    if expect is not None:
        mode, diag = expect
        assert model.data.geometry_mode() == mode
        assert diag is None or model.data.uses_diag_metric() == diag
    model.init()
    model.set_state(*start)
    model.rk4_steps(0.0, cs.dt, cs.nsteps if nsteps is None else nsteps)
    out = model.u_sol().x.array.copy(), model.v_n.x.array.copy()
    assert out[0].dtype == np.float32
    model.close()
    return out


def expected_mode(cs, stream=False):
    """(geometry mode, diagonal metric) of a case under the default options."""
    if stream or cs.tdim == 2 or cs.mesh_order == 2:
        return "stream", False
    if cs.perturb > 0:
        return "trilinear", False
    return "affine", cs.P <= 7


def references(orc, name):
    cs = fp32_case(orc, name)
    start, r32, r64 = cs.fp32_refs()
    assert_live(r64, cs.regions)
    return cs, start, r32, r64


@pytest.mark.parametrize("name", list(FP32_RUNS))
def test_model_runs(orc, name):
    """2. Linear, Lossy and Westervelt at every degree: perturbed (trilinear) and box (diagonal metric up to degree
    7) hexahedra, quadrilaterals, second-order geometry."""
    cs, start, r32, r64 = references(orc, name)
    cx = context()
    g = run_gpu(cs, cx, start, expect=expected_mode(cs))
    fb.check(f"[run-{cs.kind}] {name}", g, r32, r64, cs.regions)
    cx.close()


@pytest.mark.parametrize("P", [4, 6, 9])
@pytest.mark.parametrize("kind", KINDS)
def test_model_runs_streamed_geometry(orc, kind, P):
    cs, start, r32, r64 = references(orc, f"{kind}-p{P}")
    cx = context(dict(geometry="stream"))
    g = run_gpu(cs, cx, start, expect=expected_mode(cs, stream=True))
    fb.check(f"[run-{kind}] {kind}-p{P} stream", g, r32, r64, cs.regions)
    cx.close()


# 3. options: label -> (context keywords, options); each setting passes the budget by itself
OPTIONS = {
    "default": ({}, {}),
    "lean_rk4=0": ({}, dict(lean_rk4=0)),
    "deterministic=1": (dict(deterministic=1), {}),
    "planes=0": ({}, dict(planes=0)),
    "deterministic=1,planes=0": (dict(deterministic=1), dict(planes=0)),
    "deterministic=1,lean_rk4=0": (dict(deterministic=1), dict(lean_rk4=0)),
    "block_elems=4": (dict(block_elems=4), {}),
    "block_elems=16": (dict(block_elems=16), {}),
    "block_elems=16,lean_rk4=0": (dict(block_elems=16), dict(lean_rk4=0)),
    "pack32=1": ({}, dict(pack32=1)),
    "pack32=0": ({}, dict(pack32=0)),
    "graph=1": ({}, dict(graph=1)),
}


@pytest.mark.parametrize("P", [4, 6])
@pytest.mark.parametrize("kind", ["linear", "westervelt"])
def test_options(orc, kind, P):
    cs, start, r32, r64 = references(orc, f"{kind}-p{P}")
    err = {}
    for label, (ckw, opts) in OPTIONS.items():
        if label.startswith("pack32") and P != 6:
            continue                                   # packed kernels: degrees 5-7 (every degree: test_operator_actions)
        cx = context(ckw, opts)
        if label.startswith("pack32"):
            model = cs.model(cx)
            assert model.data.uses_pack32() == (label == "pack32=1")
            model.close()
        g = run_gpu(cs, cx, start, expect=expected_mode(cs))
        _, _, table = fb.check(f"[options-{kind}] {kind}-p{P} {label}", g, r32, r64, cs.regions)
        err[label] = {f: table[f]["all"][0] for f in ("u", "v")}
        cx.close()
    # what the accumulator-free form costs in accuracy: reported, not gated
    for f in ("u", "v"):
        print(f"fp32-lean {kind}-p{P} {f}: err(lean_rk4=1) / err(lean_rk4=0) = "
              f"{err['default'][f] / err['lean_rk4=0'][f]:.3f} ({err['default'][f]:.3e} / {err['lean_rk4=0'][f]:.3e})")


@pytest.mark.parametrize("P", [4, 6])
@pytest.mark.parametrize("kind", ["linear", "westervelt"])
def test_walking_workgroups(orc, kind, P):
    """walk=1 on 320 two-element blocks (more than the device has CUs, so workgroups do walk), lean and not."""
    cs, start, r32, r64 = references(orc, f"{kind}-walk-p{P}")
    for lean in (1, 0):
        cx = context(dict(block_elems=2), dict(walk=1, lean_rk4=lean))
        model = cs.model(cx)
        assert model.data.info()["nblocks"] >= 320
        model.close()
        g = run_gpu(cs, cx, start, expect=expected_mode(cs))
        fb.check(f"[options-{kind}] {kind}-walk-p{P} walk=1,lean_rk4={lean}", g, r32, r64, cs.regions)
        cx.close()


@pytest.mark.parametrize("lean", [1, 0])
def test_longer_run(orc, lean):
    """4. configs[4]'s arithmetic (Linear, p = 6) over 50 steps (why not 200: live_cases.FP32_LONG): the lean form
    rounds u more often per step than the accumulator form; the same criterion against the 50-step yardstick."""
    cs, start, r32, r64 = references(orc, "linear-p6-long")
    assert cs.nsteps == 50
    cx = context(None, dict(lean_rk4=lean))
    g = run_gpu(cs, cx, start, expect=expected_mode(cs))
    fb.check(f"[long-linear] linear-p6-long lean_rk4={lean}", g, r32, r64, cs.regions)
    cx.close()


@pytest.mark.parametrize("P", [6, 4])
@pytest.mark.parametrize("kind", ["lossy", "westervelt"])
def test_two_slabs_in_process(orc, kind, P):
    """5. Two x-slabs through the library's pack / ordered-sum / stage kernels (in-process transport): each rank's
    part within the budget, the interface plane bit-identical on both sharers."""
    size = 2
    cs, (u0, v0), r32, r64 = references(orc, f"{kind}-slabs-p{P}")
    regions = {**cs.regions, **slab_interface_regions(cs.pr, size)}
    assert_live(r64, regions)
    ctxs = [fa.Context(0) for _ in range(size)]
    fa.Context.init_local_group(ctxs)
    models = [cs.model(ctxs[r], rank=r, size=size) for r in range(size)]
    offs = [m.data.V.global_offset for m in models]
    for m in models:
        assert m.data.geometry_mode() == "trilinear" and m.data.dtype == np.float32
    fa.group_finish_setup(models)
    for m, off in zip(models, offs):
        m.init()
        m.set_state(u0[off:off + m.data.ndofs], v0[off:off + m.data.ndofs])
    fa.group_rk4_steps(models, 0.0, cs.dt, cs.nsteps)
    got = [(m.u_sol().x.array.copy(), m.v_n.x.array.copy()) for m in models]
    for r, (m, off) in enumerate(zip(models, offs)):
        k = m.data.ndofs
        mine = {}
        for name, idx in regions.items():
            sel = idx[(idx >= off) & (idx < off + k)] - off
            if len(sel):
                mine[name] = sel
        assert any(name.startswith("cut") for name in mine)
        part = lambda a: tuple(b[off:off + k] for b in a)  # noqa: E731
        fb.check(f"[slabs-{kind}] {kind}-slabs-p{P} rank {r}", got[r], part(r32), part(r64), mine)
    plane = len(got[0][0]) - (offs[1] - offs[0])
    assert plane > 0
    for f in (0, 1):
        assert np.array_equal(got[0][f][-plane:], got[1][f][:plane])
    for m in models:
        m.close()
    for cx in ctxs:
        cx.close()


@pytest.mark.parametrize("kind", KINDS)
def test_negative_control_far_corner(orc, kind):
    """6. The GPU model with its family's coefficient (c0 / delta / beta) of the far-corner cells scaled by 1 + 1e-2
    must FAIL the budget against the unchanged oracles by at least 2 x CAP, and pass against the oracles with the
    same change.  (1e-2: Westervelt's beta at 1 + 1e-3 moves the reference by only 6.7 x the yardstick.)"""
    cs, start, r32, r64 = references(orc, f"{kind}-p4")
    cx = context()
    g = run_gpu(cs, cx, start, scale_far_corner=1 + 1e-2)
    worst, where, table = fb.budget(g, r32, r64, cs.regions)
    print(fb.report(f"[control-{kind}] unchanged oracle", worst, where, table))
    assert worst >= 2 * fb.CAP, fb.report(kind, worst, where, table)
    _, c32, c64 = cs.fp32_refs(scale_far_corner=1 + 1e-2)
    fb.check(f"[control-{kind}] {kind}-p4 far corner x (1 + 1e-2)", g, c32, c64, cs.regions)
    cx.close()
