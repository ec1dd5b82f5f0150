"""Relaxation absorption on the device (fus_model_set_relaxation): the sub-step kernel, the Strang-split steps of every
model, the stepping entries, off-is-off, two slabs in one process, argument errors and the absorption it imposes.

Reference: tests/relaxation_ref.py (pinned in test_relaxation_host.py).  Shapes: those of test_gpu_source.py -- the
4 x 3 x 3 box at p = 3 with perturbed vertices and 4-element blocks, 6 x 5 quadrilaterals at p = 4 -- and a 2 x 2 x 2 box
at p = 2.  The strengths differ per cell and vanish in the cells whose centroid lies in the first 0.3 of the box along x."""
import functools
import math

import numpy as np
import pytest

import fenicsxfus_amd as fa
import relaxation_ref as rr
import source_ref as sr
from test_gpu_model_memory import _hip_runtime, _used_bytes
from test_gpu_source import P0, S0, TOL, make_ctx, make_model, slab_models

pytestmark = pytest.mark.gpu
NAMES = ("3d", "2d", "small")


@functools.lru_cache(maxsize=None)
def case(orc, name, dtype=np.float64):
    if name == "small":
        return sr.Case(orc, (2, 2, 2), 2, 0.1, dtype=dtype)
    return sr.case3d(orc, dtype) if name == "3d" else sr.case2d(orc, dtype)


def cell_strengths(cs, R, mesh=None, dtype=np.float64):
    """(freqs_hz [R], a [R, ncells]): relaxation frequencies around the source frequency, strengths up to 0.3 w0 that
    depend on the cell's centroid alone (so every slab of a mesh sees the same) and are zero for x < 0.3 Lx."""
    mesh = cs.pr.mesh if mesh is None else mesh
    X = np.asarray(mesh.cell_centroids(), np.float64)
    x = X[:, 0] / cs.hi[0]
    y = X[:, 1] / cs.hi[1]
    freqs = cs.f0 * np.array([0.5, 2.0, 1.0, 4.0])[:R]
    w0 = 2 * np.pi * cs.f0
    a = np.stack([w0 * 0.3 / (k + 1) * (0.25 + np.sin(3.0 * x + k) ** 2) * (0.5 + y) for k in range(R)])
    a[:, x < 0.3] = 0.0
    return freqs, a.astype(dtype).astype(np.float64)


def ctx_for(name, opts=None):
    return make_ctx("3d" if name == "small" else name, opts)


def model_for(cs, name, kind="linear", ctx=None, order=4, forms="cpp", p0=P0):
    return make_model(cs, kind, ctx, order, forms, p0)


# ---- 1. the kernel alone ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hfac", [1, 100])
@pytest.mark.parametrize("tname", ["f64", "f32"])
@pytest.mark.parametrize("R", [1, 2, 3, 4])
@pytest.mark.parametrize("name", NAMES)
def test_substep_kernel(orc, name, R, tname, hfac):
    """fus_model_relaxation_apply on random v, z against the sub-step evaluated in long double on the same inputs
    (the device's own A_nu and the coefficients rounded to T).  Bounds from the count of roundings:
    |dv+| <= (4 R + 8) eps (|v| + sum A g |z|),  |dz+| <= 6 eps (|p z| + e (|v| + |v+|)) + e (the bound on v+)."""
    T = np.float64 if tname == "f64" else np.float32
    cs = case(orc, name, T)
    freqs, a = cell_strengths(cs, R, dtype=T)
    omega = 2 * np.pi * freqs
    h = hfac * 0.5 * cs.dt
    nd = cs.pr.ndofs
    rng = np.random.default_rng(11 + R)
    v0 = rng.standard_normal(nd).astype(T)
    z0 = (rng.standard_normal((R, nd)) / omega[:, None]).astype(T)
    ctx = ctx_for(name)
    mdl = model_for(cs, name, ctx=ctx)
    mdl.init()
    mdl.set_relaxation(freqs, a)
    A = np.stack([mdl.relaxation_strength(k) for k in range(R)])
    mdl.set_state(v=v0)
    for k in range(R):
        mdl.set_relaxation_state(k, z0[k])
    mdl.relaxation_apply(h)
    mdl.u_sol()
    v1 = mdl.v_n.x.array.copy()
    z1 = np.stack([mdl.relaxation_state(k) for k in range(R)])
    assert not mdl.u_n.x.array.any()
    mdl.close(), ctx.close()
    # the strengths: the lumped quotient of the oracle's mass actions, to a few roundings of T
    A_ref = rr.lumped_strengths(cs.pr, a, cs.c, cs.rho)
    assert A.dtype == T and np.abs(A - A_ref).max() <= 64 * np.finfo(T).eps * np.abs(A_ref).max()
    zero = ~A.any(axis=0)
    assert zero.any() and (~zero).any() and (A >= 0).all()
    LD = np.longdouble
    vr_, zr_ = rr.substep(v0, z0, A, omega, h, dtype=LD, coef_dtype=T)
    p, e, g = (c.astype(LD) for c in rr.coefficients(omega, h, T))
    eps = LD(np.finfo(T).eps)
    av, az, AL = np.abs(v0.astype(LD)), np.abs(z0.astype(LD)), A.astype(LD)
    bv = (4 * R + 8) * eps * (av + (AL * g[:, None] * az).sum(axis=0))
    dv = np.abs(v1.astype(LD) - vr_)
    print(f"relax kernel {name} R={R} {tname} h x{hfac}: max dv / bound {float((dv / bv).max()):.3f}")
    assert np.all(dv <= bv)
    for k in range(R):
        bz = 6 * eps * (np.abs(p[k]) * az[k] + e[k] * (av + np.abs(vr_))) + e[k] * bv
        assert np.all(np.abs(z1[k].astype(LD) - zr_[k]) <= bz), k
    assert np.array_equal(v1[zero], v0[zero])
    E0, E1 = rr.energy(v0, z0, A, omega).sum(), rr.energy(v1, z1, A, omega).sum()
    assert E1 <= E0


# ---- 2. every model against the stepper ------------------------------------------------------------------------------
# (the two-field models on the 3-D case only, as in test_gpu_source.py)
MODELS = [("3d", "linear", 0, 4), ("2d", "linear", 0, 4), ("3d", "linear", 0, 2), ("2d", "linear", 0, 2), ("3d", "lossy", 0, 4),
          ("3d", "lossy", 1, 4), ("3d", "westervelt", 0, 4)]
MODEL_IDS = [f"{n}-{k}-forms{f}-rk{o}" for n, k, f, o in MODELS]


def model_p0(kind):
    return 6e6 if kind == "westervelt" else P0


def run_gpu(cs, name, kind, forms, order, relax, opts=None, nsteps=sr.NSTEPS):
    ctx = ctx_for(name, opts)
    mdl = model_for(cs, name, kind, ctx, order, "python" if forms else "cpp", model_p0(kind))
    mdl.init()
    if relax is not None:
        mdl.set_relaxation(*relax)
    mdl.rk4_steps(0.0, cs.dt, nsteps)
    mdl.u_sol()
    out = (mdl.u_n.x.array.copy(), mdl.v_n.x.array.copy(),
           None if relax is None else np.stack([mdl.relaxation_state(k) for k in range(len(relax[0]))]))
    mdl.close(), ctx.close()
    return out


@functools.lru_cache(maxsize=None)
def reference(orc, name, kind, forms, order, dtype=np.float64, relax=True):
    cs = case(orc, name, dtype)
    freqs, a = cell_strengths(cs, 2, dtype=dtype)
    A = rr.lumped_strengths(cs.pr, a, cs.c, cs.rho)
    om = 2 * np.pi * freqs
    return rr.stepper(cs, kind, forms, A if relax else None, om if relax else om[:0], model_p0(kind), 0.0, cs.dt, sr.NSTEPS, order)


@pytest.mark.parametrize("name,kind,forms,order", MODELS, ids=MODEL_IDS)
def test_models_vs_stepper(orc, name, kind, forms, order):
    """20 steps from rest with the default source, R = 2: u, v and each z_nu at 1e-10 relative."""
    cs = case(orc, name)
    u, v, z = run_gpu(cs, name, kind, forms, order, cell_strengths(cs, 2))
    ur, vr_, zr_ = reference(orc, name, kind, forms, order)
    errs = [sr.rel(u, ur), sr.rel(v, vr_)] + [sr.rel(z[k], zr_[k]) for k in range(2)]
    print(f"relax {name} {kind} forms={forms} rk{order}: rel err u, v, z0, z1 = " + ", ".join(f"{e:.3e}" for e in errs))
    assert all(np.abs(x).max() > 0 for x in (ur, vr_, zr_[0], zr_[1]))
    assert all(e < TOL for e in errs), errs
    # and the absorption acts within these steps: without it the comparison above could not pass
    assert sr.rel(vr_, reference(orc, name, kind, forms, order, relax=False)[1]) > 100 * TOL


@pytest.mark.parametrize("name,kind,forms,order", MODELS, ids=MODEL_IDS)
def test_fp32_vs_double_stepper(orc, name, kind, forms, order):
    """The float run against the double stepper on the float-rounded inputs, held to the yardstick of
    test_gpu_source.py::test_fp32_vs_double_stepper: err <= 4 yard per field, yard = the error of the same float model
    WITHOUT relaxation against its double stepper (what the float kernels lose by themselves); 2 for the run-to-run
    order of the LDS sums x 2 for the strengths and coefficients, rounded to float once more, and the two extra
    roundings of v per sub-step.  z_nu is an integral of v: it is held to v's yardstick."""
    cs = case(orc, name, np.float32)
    g0 = run_gpu(cs, name, kind, forms, order, None)
    r0 = reference(orc, name, kind, forms, order, np.float32, relax=False)
    yard = max(sr.rel(g0[0], r0[0]), fb_floor()), max(sr.rel(g0[1], r0[1]), fb_floor())
    u, v, z = run_gpu(cs, name, kind, forms, order, cell_strengths(cs, 2, dtype=np.float32))
    assert u.dtype == np.float32 and z.dtype == np.float32
    ur, vr_, zr_ = reference(orc, name, kind, forms, order, np.float32)
    errs = [sr.rel(u, ur), sr.rel(v, vr_)] + [sr.rel(z[k], zr_[k]) for k in range(2)]
    print(f"relax fp32 {name} {kind} forms={forms} rk{order}: err u, v, z0, z1 = " + ", ".join(f"{e:.3e}" for e in errs)
          + f"   yard u {yard[0]:.3e} v {yard[1]:.3e}")
    assert errs[0] <= 4 * yard[0] and all(e <= 4 * yard[1] for e in errs[1:])


def fb_floor():
    import fp32_budget as fb

    return fb.EPS32      # one float ulp: the floor of every yardstick (fp32_budget.py)


# ---- 3. entry points ------------------------------------------------------------------------------------------------------
NENT = 6


def entry_run(cs, form, opts=None):
    """NENT steps of dt2 (a power of two: the clock of rk() lands on the same times) with R = 2 through one entry form,
    a receiver record of v after every step and the monitor sampling v after the last step only."""
    dt = 2.0 ** math.floor(math.log2(cs.dt))
    ctx = make_ctx("3d", dict(deterministic=1, **(opts or {})))
    if form == "external":
        ctx.init_external(0, 1)
    mdl = make_model(cs, "linear", ctx)
    mdl.init()
    mdl.set_relaxation(*cell_strengths(cs, 2))
    lo, hi = np.zeros(3), np.array(cs.hi)
    assert len(mdl.set_receivers(lo + (hi - lo) * np.array([[0.5, 0.5, 0.5], [0.07, 0.4, 0.6], [0.93, 0.81, 0.22]]))) == 3
    mdl.record(1, 2 * NENT, "v")
    mdl.monitor("v", skip=NENT - 1)
    if form == "rk":
        mdl.dt = dt
        mdl.rk(0.0, NENT * dt)
        assert mdl.nsteps == NENT
    elif form == "steps":
        mdl.rk4_steps(0.0, dt, NENT)
    elif form == "two_calls":
        mdl.rk4_steps(0.0, dt, 2)
        mdl.rk4_steps(2 * dt, dt, NENT - 2)
    elif form == "single":
        for s in range(NENT):
            mdl.rk4_steps(s * dt, dt, 1)
    else:
        mdl.external_rk_steps(0.0, dt, NENT, lambda: None, rk_order=4)
    mdl.u_sol()
    out = dict(u=mdl.u_n.x.array.copy(), v=mdl.v_n.x.array.copy(), z=[mdl.relaxation_state(k) for k in range(2)],
               records=mdl.records(), sample=mdl.sample("v"), mon=mdl.monitor_info(), mon_max=mdl.monitor_get("max").x.array.copy())
    mdl.close(), ctx.close()
    return out


def same_state(a, b):
    return (np.array_equal(a["u"], b["u"]) and np.array_equal(a["v"], b["v"])
            and all(np.array_equal(x, y) for x, y in zip(a["z"], b["z"])))


def test_entry_points_give_the_same_bits(orc):
    cs = case(orc, "3d")
    ref = entry_run(cs, "steps")
    assert np.abs(ref["v"]).max() > 0 and np.abs(ref["z"][1]).max() > 0
    for form in ("rk", "two_calls", "single", "external"):
        got = entry_run(cs, form)
        assert same_state(got, ref), form
        assert np.array_equal(got["records"][1], ref["records"][1]) and np.array_equal(got["mon_max"], ref["mon_max"]), form
    # records and monitor samples see the state after the trailing half-step
    t, rec = ref["records"]
    assert rec.shape == (NENT, 3) and np.abs(rec[-1]).min() > 0
    assert np.array_equal(rec[-1], ref["sample"])
    assert ref["mon"][0] == 1 and np.array_equal(ref["mon_max"], ref["v"])


def test_graph_replay_matches_stepwise(orc):
    cs = case(orc, "3d")
    a, b = entry_run(cs, "steps", dict(graph=1)), entry_run(cs, "single", dict(graph=0))
    assert same_state(a, b) and np.array_equal(a["records"][1], b["records"][1])


# ---- 4. off is off ----------------------------------------------------------------------------------------------------------
def test_off_is_off(orc):
    cs = case(orc, "3d")
    freqs, a = cell_strengths(cs, 2)
    runs = []
    for mode in ("never", "cleared", "zero"):
        ctx = make_ctx("3d", dict(deterministic=1))
        ctx.profile_enable(True)
        mdl = make_model(cs, "linear", ctx)
        mdl.init()
        if mode == "cleared":
            mdl.set_relaxation(freqs, a)
            mdl.clear_relaxation()
            with pytest.raises(fa.FusError, match="error -4"):
                mdl.relaxation_state(0)
        elif mode == "zero":
            mdl.set_relaxation(freqs, np.zeros_like(a))
        mdl.rk4_steps(0.0, cs.dt, 5)
        mdl.u_sol()
        runs.append((mdl.u_n.x.array.copy(), mdl.v_n.x.array.copy()))
        assert ctx.profile_get("relax")[1] == (10 if mode == "zero" else 0)
        mdl.close(), ctx.close()
    assert np.abs(runs[0][0]).max() > 0
    for r in runs[1:]:
        assert np.array_equal(r[0], runs[0][0]) and np.array_equal(r[1], runs[0][1])


def test_clear_frees_the_planes():
    """24^3 cells at p = 4 (912 673 DOFs), R = 4 in fp64: the z and A planes take S = 2 x 4 x n_internal x 8 bytes, at
    least 58 MB.  Used device memory rises by more than S / 2 with set_relaxation and returns to within S / 2 of the
    start with clear_relaxation.  Used memory is device-wide and the device may be shared: up to three tries."""
    L, P, n = 0.024, 4, 24
    mesh = fa.BoxMesh([0, 0, 0], [L, L, L], (n, n, n))
    V = fa.FunctionSpace(mesh, P)
    nc = mesh.num_cells
    ctx = fa.Context(0)
    mdl = fa.LinearSpectralExplicit(mesh, fa.tag_box_boundary(mesh), P, np.full(nc, 1500.0), np.full(nc, 1000.0), 0.5e6, P0,
                                    S0, 4, 1e-8, V=V, ctx=ctx)
    hip = _hip_runtime()
    S = 2 * 4 * V.num_dofs * 8
    ok = False
    for _ in range(3):
        ctx.synchronize()
        before = _used_bytes(hip)
        mdl.set_relaxation([0.25e6, 0.5e6, 1e6, 2e6], [1e3, 2e3, 3e3, 4e3])
        ctx.synchronize()
        with_planes = _used_bytes(hip)
        mdl.clear_relaxation()
        ctx.synchronize()
        after = _used_bytes(hip)
        print(f"relax planes: S = {S} bytes, set +{(with_planes - before) / S:.3f} S, after clear +{(after - before) / S:.3f} S")
        if with_planes - before > S // 2 and after - before < S // 2:
            ok = True
            break
    mdl.close(), ctx.close()
    assert ok


# ---- 5. two slabs in one process -----------------------------------------------------------------------------------------
def test_two_slabs_in_process(orc):
    cs = case(orc, "3d")
    freqs, a = cell_strengths(cs, 2)
    single = run_gpu(cs, "3d", "linear", 0, 4, (freqs, a))
    ctxs = [fa.Context(0, block_elems=4) for _ in range(2)]
    fa.Context.init_local_group(ctxs)
    models = slab_models(cs, ctxs, 0)
    ms = [m for m, _ in models]
    with pytest.raises(fa.FusError, match="error -4"):      # the setup is not finished
        ms[0].set_relaxation(freqs, a[:, :ms[0].mesh.num_cells])
    fa.group_finish_setup(ms)
    for m in ms:
        m.init()
        m.set_relaxation(*cell_strengths(cs, 2, mesh=m.mesh))
    with pytest.raises(fa.FusError, match="error -4"):      # the strengths are not summed over the sharers yet
        fa.group_rk4_steps(ms, 0.0, cs.dt, 1)
    with pytest.raises(fa.FusError, match="error -4"):
        ms[0].relaxation_apply(0.5 * cs.dt)
    fa.group_relaxation_finish(ms)
    fa.group_rk4_steps(ms, 0.0, cs.dt, sr.NSTEPS)
    got = []
    for m, off in models:
        n = m.data.ndofs
        m.u_sol()
        fields = [m.u_n.x.array.copy(), m.v_n.x.array.copy()] + [m.relaxation_state(k) for k in range(2)]
        got.append((off, fields))
        for f, ref, nm in zip(fields, (single[0], single[1], single[2][0], single[2][1]), ("u", "v", "z0", "z1")):
            err = np.abs(f - ref[off:off + n]).max() / np.abs(ref).max()
            print(f"relax slabs rank off {off}: {nm} rel err vs single {err:.3e}")
            assert err < TOL
    off1 = got[1][0]
    plane = len(got[0][1][0]) - off1
    assert plane > 0
    for f0, f1 in zip(got[0][1][1:], got[1][1][1:]):        # v and every z_nu on the interface: the same bits
        assert np.abs(f0[off1:]).max() > 0 and np.array_equal(f0[off1:], f1[:plane])
    for m in ms:
        m.close()
    for c in ctxs:
        c.close()


# ---- 6. argument errors ---------------------------------------------------------------------------------------------------
def test_argument_errors(orc):
    cs = case(orc, "small")
    nc = cs.pr.mesh.num_cells
    ctx = ctx_for("small")
    mdl = model_for(cs, "small", ctx=ctx)
    mdl.init()
    good = np.full((2, nc), 1e4)
    for freqs, a in (([1e5] * 5, np.full((5, nc), 1e4)), ([1e5, 0.0], good), ([1e5, -1e5], good), ([1e5, np.nan], good),
                     ([1e5, np.inf], good)):
        with pytest.raises(fa.FusError, match="error -1"):
            mdl.set_relaxation(freqs, a)
    for bad in (-1e-9, np.nan, np.inf):
        a = good.copy()
        a[1, 3] = bad
        with pytest.raises(fa.FusError, match="error -1"):
            mdl.set_relaxation([1e5, 1e6], a)
    with pytest.raises(fa.FusError):
        mdl.set_relaxation([1e5, 1e6], good[:, :-1])
    with pytest.raises(fa.FusError, match="error -4"):      # still off after the failed calls
        mdl.relaxation_state(0)
    mdl.set_relaxation([1e5, 1e6], good)
    for nu in (-1, 2):
        with pytest.raises(fa.FusError, match="error -1"):
            mdl.relaxation_state(nu)
    with pytest.raises(fa.FusError, match="error -1"):
        mdl.relaxation_apply(-1.0)
    assert not mdl.relaxation_state(1).any()
    mdl.close(), ctx.close()


# ---- 7. physics: the absorption the model imposes -----------------------------------------------------------------------
# The deviation of relaxation_ref's stepper on the CPU from the exact alpha (rr.Bar.cpu_alpha, the identical run):
CPU_DEV = {0.5e6: 8.24e-3, 1.0e6: 1.17e-3}


@functools.lru_cache(maxsize=None)
def bar_alpha(orc, ncells, f0):
    bar = rr.Bar(orc, ncells, f0)
    ctx = fa.Context(0)
    mdl = fa.LinearSpectralExplicit(bar.pr.mesh, bar.tags, bar.P, bar.c, bar.rho, f0, rr.BAR_P0, S0, 4, bar.dt, V=bar.pr.V, ctx=ctx)
    mdl.init()
    mdl.set_relaxation(bar.freqs, bar.strength)
    mdl.monitor("u", nharm=1, skip=bar.skip)
    mdl.rk4_steps(0.0, bar.dt, bar.nsteps)
    assert mdl.monitor_info()[0] == 2 * bar.spp
    alpha = bar.alpha_from(mdl.monitor_get("cos", 1).x.array, mdl.monitor_get("sin", 1).x.array)
    mdl.close(), ctx.close()
    return alpha, bar.alpha_exact, bar.nsteps


@pytest.mark.parametrize("ncells,f0", [(32, 0.5e6), (64, 1.0e6)])
def test_imposed_absorption(orc, ncells, f0):
    """A plane wave down a bar of 24 mm (rr.Bar: p = 4, c = 1500, source on x = 0, absorbing on x = L, natural side walls;
    R = 2 with alpha(0.5 MHz) L = 0.95): minus the slope of ln |first harmonic| over 2 to 6 wavelengths, from the
    monitor over the last two whole periods, against relaxation_alpha(f0).  The tolerance is twice the deviation of
    relaxation_ref's stepper on the identical case, measured on the CPU: 8.24e-3 at 0.5 MHz (39.993 against the exact
    39.666 Np/m, 2816 steps), 1.17e-3 at 1 MHz (78.761 against 78.669 Np/m, 4864 steps)."""
    alpha, exact, nsteps = bar_alpha(orc, ncells, f0)
    dev = alpha / exact - 1.0
    print(f"relax absorption f0 = {f0:g}: alpha {alpha:.4f} Np/m, exact {exact:.4f}, deviation {dev:.3e} ({nsteps} steps)")
    assert abs(dev) <= 2 * CPU_DEV[f0]


def test_absorption_ratio_is_not_f_squared(orc):
    """alpha(1 MHz) / alpha(0.5 MHz) from the two runs against the exact ratio 1.983 (f^2 would give 4), within the sum
    of the two margins above."""
    a1, e1, _ = bar_alpha(orc, 64, 1.0e6)
    a0, e0, _ = bar_alpha(orc, 32, 0.5e6)
    print(f"relax absorption ratio: {a1 / a0:.4f}, exact {e1 / e0:.4f}")
    assert abs((a1 / a0) / (e1 / e0) - 1.0) <= 2 * (CPU_DEV[0.5e6] + CPU_DEV[1.0e6])
