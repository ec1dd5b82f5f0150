"""Phased / apodised source on the device (fus_model_set_source): per-DOF amplitude and delay, tone burst.

Reference: the numpy RK stepper of tests/source_ref.py (pinned against the oracle in test_source_host.py).  Shapes: a
4 x 3 x 3 box at p = 3 with perturbed vertices and 4-element blocks (nine blocks: the boundary entries fall into the
block-interior range and into the shared range; 596 boundary entries, 100 of them on the source face -- neither a
multiple of 64) and 6 x 5 quadrilaterals at p = 4 (88 boundary entries; by default one block, so every boundary entry
is block-interior and the shared-entry path is idle, and with 8-element blocks both ranges again).  A source period
is 9 steps of the CFL dt; amp in [0, 1.5] with exact zeros towards the rim of the face, tau in [0, 3 / f]; 20 RK steps
from rest starting at t0 = 0 (onset), 3.5 / f (ramp end) and, for a burst of D = 10 / f, D - 1 / f (burst end).
fp64 bound: 1e-10 relative, the project's bound for 20 steps."""
import functools

import numpy as np
import pytest

import fenicsxfus_amd as fa
from fenicsxfus_amd import monitor as fmon, source as fsrc
import source_ref as sr
from util import Problem

pytestmark = pytest.mark.gpu

S0 = sr.S0
P0 = 6e4
TOL = 1e-10
CLASSES = {"linear": fa.LinearSpectralExplicit, "lossy": fa.LossySpectralExplicit,
           "westervelt": fa.WesterveltSpectralExplicit}


@functools.lru_cache(maxsize=None)
def case(orc, name, dtype=np.float64):
    return sr.case3d(orc, dtype) if name == "3d" else sr.case2d(orc, dtype)


def make_ctx(name, opts=None, blocks=None):
    opts = dict(opts or {})
    be = blocks if blocks is not None else (4 if name == "3d" else None)
    ctx = fa.Context(0, block_elems=be, deterministic=bool(opts.pop("deterministic", 0)) or None)
    for k, v in opts.items():
        ctx.set_option(k, v)
    return ctx


def make_model(cs, kind, ctx, rk_order=4, forms="cpp", p0=P0):
    pr = cs.pr_dev
    args = [pr.mesh, cs.tags, cs.P, cs.c, cs.rho]
    kw = dict(V=pr.V, ctx=ctx)
    if kind != "linear":
        args.append(cs.delta)
        kw["forms"] = forms
    if kind == "westervelt":
        args.append(cs.beta)
    return CLASSES[kind](*args, cs.f0, p0, S0, rk_order, cs.dt, **kw)


def run_model(cs, kind, ctx, t0, nsteps, amp=None, tau=None, D=0.0, rk_order=4, forms="cpp", p0=P0, source=True):
    mdl = make_model(cs, kind, ctx, rk_order, forms, p0)
    mdl.init()
    if source:
        mdl.set_source(amp, tau, D)
    mdl.rk4_steps(t0, cs.dt, nsteps)
    mdl.u_sol()
    u, v = mdl.u_n.x.array.copy(), mdl.v_n.x.array.copy()
    mdl.close()
    return u, v


@functools.lru_cache(maxsize=None)
def reference(orc, name, kind, forms, which, order=4, dtype=np.float64):
    """The stepper's (u, v) after 20 steps for the aperture of the case; float cases: on the float-rounded inputs."""
    cs = case(orc, name, dtype)
    t0, D = cs.t0s()[which]
    amp, tau = (a.astype(dtype).astype(np.float64) for a in cs.aperture())
    vec, scale = cs.vectors(kind, forms)
    return sr.rk_stepper(cs.pr, vec, scale, cs.f0, P0, t0, cs.dt, sr.NSTEPS, amp, tau, D, order)


def check(u, v, ref, tol=TOL, label=""):
    eu, ev = sr.rel(u, ref[0]), sr.rel(v, ref[1])
    print(f"source {label}: rel err u {eu:.3e} v {ev:.3e}")
    assert np.abs(ref[0]).max() > 0 and np.abs(ref[1]).max() > 0
    assert eu < tol and ev < tol, (label, eu, ev)


# ---- 1. Linear fp64 against the stepper -----------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["onset", "ramp_end", "burst_end"])
@pytest.mark.parametrize("name", ["3d", "2d"])
def test_linear_vs_stepper(orc, name, which):
    cs = case(orc, name)
    t0, D = cs.t0s()[which]
    amp, tau = cs.aperture()
    ctx = make_ctx(name)
    u, v = run_model(cs, "linear", ctx, t0, sr.NSTEPS, amp, tau, D)
    ctx.close()
    check(u, v, reference(orc, name, "linear", 0, which), label=f"linear {name} {which}")


VARIANTS = {"lean_rk4=0": (dict(lean_rk4=0), 4), "rk_order=2": ({}, 2), "rk_order=3": ({}, 3), "planes=0": (dict(planes=0), 4),
            "deterministic=1": (dict(deterministic=1), 4)}


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("name", ["3d", "2d"])
def test_linear_vs_stepper_options(orc, name, variant):
    """The onset run again with each option that changes which kernels read the weights, and when."""
    opts, order = VARIANTS[variant]
    cs = case(orc, name)
    amp, tau = cs.aperture()
    ctx = make_ctx(name, opts)
    u, v = run_model(cs, "linear", ctx, 0.0, sr.NSTEPS, amp, tau, 0.0, rk_order=order)
    ctx.close()
    check(u, v, reference(orc, name, "linear", 0, "onset", order), label=f"linear {name} {variant}")


@pytest.mark.parametrize("which", ["onset", "burst_end"])
def test_linear_2d_several_blocks(orc, which):
    """The quadrilateral case with 8-element blocks: its boundary entries in both ranges, as in 3-D."""
    cs = case(orc, "2d")
    t0, D = cs.t0s()[which]
    amp, tau = cs.aperture()
    ctx = make_ctx("2d", blocks=8)
    mdl = make_model(cs, "linear", ctx)
    info = mdl.data.info()
    mdl.close()
    assert info["nblocks"] > 1 and info["shared_dofs"] > 0
    u, v = run_model(cs, "linear", ctx, t0, sr.NSTEPS, amp, tau, D)
    ctx.close()
    check(u, v, reference(orc, "2d", "linear", 0, which), label=f"linear 2d blocks {which}")


@pytest.mark.parametrize("name", ["3d", "2d"])
def test_graph_replay_matches_stepwise(orc, name):
    """Option "graph": 20 steps in one call (steps 2.. replayed from the captured graph, the per-stage source launches
    carrying each step's times) against 20 one-step calls without it -- bit for bit under deterministic = 1, the
    criterion of the monitor tests for graph-replayed runs -- and against the stepper."""
    cs = case(orc, name)
    amp, tau = cs.aperture()
    out = {}
    for graph in (0, 1):
        ctx = make_ctx(name, dict(deterministic=1, graph=graph))
        mdl = make_model(cs, "linear", ctx)
        mdl.init()
        mdl.set_source(amp, tau)
        if graph:
            mdl.rk4_steps(0.0, cs.dt, sr.NSTEPS)
        else:
            t = 0.0
            for _ in range(sr.NSTEPS):
                mdl.rk4_steps(t, cs.dt, 1)
                t += cs.dt
        mdl.u_sol()
        out[graph] = (mdl.u_n.x.array.copy(), mdl.v_n.x.array.copy())
        mdl.close()
        ctx.close()
    check(*out[1], reference(orc, name, "linear", 0, "onset"), label=f"linear {name} graph")
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])


# ---- 2. Lossy fp64 against the stepper: the bsrc2 / dg path -------------------------------------------------------------
@pytest.mark.parametrize("which", ["onset", "ramp_end", "burst_end"])
@pytest.mark.parametrize("forms", [0, 1])
def test_lossy_vs_stepper(orc, forms, which):
    cs = case(orc, "3d")
    t0, D = cs.t0s()[which]
    amp, tau = cs.aperture()
    ctx = make_ctx("3d")
    u, v = run_model(cs, "lossy", ctx, t0, sr.NSTEPS, amp, tau, D, forms="python" if forms else "cpp")
    ctx.close()
    check(u, v, reference(orc, "3d", "lossy", forms, which), label=f"lossy forms={forms} {which}")


# ---- 3. amplitude only: folded into the weights, the kernel never runs ---------------------------------------------------
@pytest.mark.parametrize("name", ["3d", "2d"])
def test_amplitude_only_is_folded(orc, name):
    cs = case(orc, name)
    pr = cs.pr
    amp, _ = cs.aperture()
    vec, _ = cs.vectors("linear")
    u, v = np.zeros(pr.ndofs), np.zeros(pr.ndofs)
    orc.linear_rk4(cs.tdim, pr.N, pr.dm, pr.G, pr.D, vec["lin"], vec["m"], vec["src"] * amp, vec["absb"], cs.f0, P0, S0,
                   0.0, 0.0, cs.dt, u, v, steps=sr.NSTEPS)
    ctx = make_ctx(name)
    ctx.profile_enable(True)
    mdl = make_model(cs, "linear", ctx)
    mdl.init()
    mdl.set_source(amplitude=amp)
    mdl.rk4_steps(0.0, cs.dt, sr.NSTEPS)
    mdl.u_sol()
    check(mdl.u_n.x.array, mdl.v_n.x.array, (u, v), label=f"amplitude only {name}")
    assert ctx.profile_get("source")[1] == 0 and ctx.profile_get("stiffness")[1] == 4 * sr.NSTEPS
    # with delays the kernel runs once per NEW stage time (never more than once per stage after the first): classical
    # RK4 has the stage times t, t + dt/2 (twice) and t + dt (= the next step's first), so 2 per step and 1 to start
    mdl.init()
    mdl.set_source(amp, np.zeros(pr.ndofs))
    ctx.profile_enable(True)
    mdl.rk4_steps(0.0, cs.dt, sr.NSTEPS)
    n = ctx.profile_get("source")[1]
    assert n == 2 * sr.NSTEPS + 1, n
    mdl.u_sol()
    check(mdl.u_n.x.array, mdl.v_n.x.array, (u, v), label=f"amplitude through the kernel {name}")
    mdl.close()
    ctx.close()


# ---- 4. the uniform source through the kernel ------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["linear", "lossy", "westervelt"])
def test_uniform_source_through_kernel(orc, kind):
    """delay = zeros: the per-entry path with the default waveform, against the default (scalar) path."""
    cs = case(orc, "3d")
    p0 = 6e6 if kind == "westervelt" else P0
    res = []
    for source in (False, True):
        ctx = make_ctx("3d")
        res.append(run_model(cs, kind, ctx, 0.0, sr.NSTEPS, None, np.zeros(cs.pr.ndofs), 0.0, p0=p0, source=source))
        ctx.close()
    check(*res[1], res[0], label=f"uniform through the kernel {kind}")


# ---- 5. causality and time shift ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["linear", "lossy", "westervelt"])
def test_causality_and_time_shift(orc, kind):
    cs = case(orc, "3d")
    p0 = 6e6 if kind == "westervelt" else P0
    k, n, nd = 5, sr.NSTEPS, cs.pr.ndofs
    ctx = make_ctx("3d")
    # nothing moves before the delay has passed: exactly 0.0
    u, v = run_model(cs, kind, ctx, 0.0, k, None, np.full(nd, (k + 0.5) * cs.dt), p0=p0)
    assert not u.any() and not v.any()
    # a common delay of k steps shifts the run by k steps
    u, v = run_model(cs, kind, ctx, 0.0, n + k, None, np.full(nd, k * cs.dt), p0=p0)
    ref = run_model(cs, kind, ctx, 0.0, n, source=False, p0=p0)
    ctx.close()
    check(u, v, ref, label=f"time shift {kind}")


# ---- 6. argument errors, clear_source ------------------------------------------------------------------------------------
def test_argument_errors_and_clear(orc):
    cs = case(orc, "3d")
    nd = cs.pr.ndofs
    amp, tau = cs.aperture()
    on, off = cs.face[3], np.setdiff1d(np.arange(nd), cs.face)[0]
    ctx = make_ctx("3d")
    fresh = run_model(cs, "linear", ctx, 0.0, sr.NSTEPS, source=False)
    mdl = make_model(cs, "linear", ctx)
    mdl.init()
    for bad in (-1e-9, np.nan, np.inf):
        for arg in ("amplitude", "delay"):
            x = (amp if arg == "amplitude" else tau).copy()
            x[on] = bad
            with pytest.raises(fa.FusError, match="error -1"):
                mdl.set_source(**{arg: x})
            x[on], x[off] = 0.5 * abs(tau[on]), bad       # off the source boundary: ignored
            mdl.set_source(**{arg: x})
    Lr = 4.0 / cs.f0
    for D in (0.5 * Lr, np.nextafter(2 * Lr, 0), -1.0, np.inf, np.nan):
        with pytest.raises(fa.FusError, match="error -1"):
            mdl.set_source(amp, tau, D)
    mdl.set_source(amp, tau, 2 * Lr)
    with pytest.raises(fa.FusError):
        mdl.set_source(amp[:-1], tau)
    # after clear_source: the default source, bit for bit what a fresh model computes
    mdl.rk4_steps(0.0, cs.dt, 3)
    mdl.clear_source()
    mdl.init()
    mdl.rk4_steps(0.0, cs.dt, sr.NSTEPS)
    mdl.u_sol()
    assert np.array_equal(mdl.u_n.x.array, fresh[0]) and np.array_equal(mdl.v_n.x.array, fresh[1])
    assert np.abs(fresh[0]).max() > 0
    mdl.close()
    ctx.close()


def test_set_source_before_setup_is_finished(orc):
    """In-process group: the models exist but fus_group_finish_setup has not run -> FUS_ERR_STATE."""
    cs = case(orc, "3d")
    ctxs = [fa.Context(0, block_elems=4) for _ in range(2)]
    fa.Context.init_local_group(ctxs)
    models = slab_models(cs, ctxs, 0)
    with pytest.raises(fa.FusError, match="error -4"):
        models[0][0].set_source(delay=np.zeros(models[0][0].data.ndofs))
    fa.group_finish_setup([m for m, _ in models])
    models[0][0].set_source(delay=np.zeros(models[0][0].data.ndofs))
    for m, _ in models:
        m.close()
    for c in ctxs:
        c.close()


# ---- 7. two slabs in one process, the interface crossing the source face ---------------------------------------------------
def slab_models(cs, ctxs, source_axis):
    out = []
    for r, ctx in enumerate(ctxs):
        mesh = fa.BoxMesh([0.0] * 3, cs.hi, cs.n, rank=r, size=len(ctxs), perturb=0.1)
        V = fa.FunctionSpace(mesh, cs.P)
        cx = mesh.cell_centroids()[:, 0]
        sel = (cx > 0.4 * cs.hi[0]) & (cx < 0.6 * cs.hi[0])
        c, rho = np.where(sel, 2800.0, 1500.0), np.where(sel, 1850.0, 1000.0)
        mdl = fa.LinearSpectralExplicit(mesh, fa.tag_box_boundary(mesh, source_axis=source_axis), cs.P, c, rho, cs.f0, P0,
                                        S0, 4, cs.dt, V=V, ctx=ctx)
        out.append((mdl, V.global_offset))
    return out


@pytest.mark.parametrize("overlap", [0, 1])
def test_two_slabs_in_process(orc, overlap):
    cs = sr.Case(orc, (4, 3, 3), 3, 0.1, source_axis=1)
    amp, tau = cs.aperture()
    t0, D = cs.t0s()["onset"]
    vec, scale = cs.vectors("linear")
    ref = sr.rk_stepper(cs.pr, vec, scale, cs.f0, P0, t0, cs.dt, sr.NSTEPS, amp, tau, D)
    ctx1 = make_ctx("3d")
    single = run_model(cs, "linear", ctx1, t0, sr.NSTEPS, amp, tau, D)
    ctx1.close()
    check(*single, ref, label="single model, source on the y face")
    ctxs = [fa.Context(0, block_elems=4) for _ in range(2)]
    for c in ctxs:
        c.set_option("overlap_blocks", overlap)
    fa.Context.init_local_group(ctxs)
    models = slab_models(cs, ctxs, 1)
    fa.group_finish_setup([m for m, _ in models])
    for m, off in models:
        n = m.data.ndofs
        m.init()
        m.set_source(amp[off:off + n], tau[off:off + n], D)
    fa.group_rk4_steps([m for m, _ in models], t0, cs.dt, sr.NSTEPS)
    got = []
    for m, off in models:
        n = m.data.ndofs
        m.u_sol()
        u, v = m.u_n.x.array.copy(), m.v_n.x.array.copy()
        got.append((off, u, v))
        for a, b, nm in ((u, single[0], "u"), (v, single[1], "v")):
            err = np.abs(a - b[off:off + n]).max() / np.abs(b).max()
            print(f"source slabs overlap={overlap} rank off {off}: {nm} rel err vs single {err:.3e}")
            assert err < TOL
    off1 = got[1][0]
    plane = len(got[0][1]) - off1
    assert plane > 0 and np.abs(got[0][1][off1:]).max() > 0
    assert np.array_equal(got[0][1][off1:], got[1][1][:plane]) and np.array_equal(got[0][2][off1:], got[1][2][:plane])
    for m, _ in models:
        m.close()
    for c in ctxs:
        c.close()


# ---- 8. fp32 ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fp32_yard(orc, name):
    """Relative error of the DEFAULT fp32 path over the same mesh and steps against orc.linear_rk4 in double (on the
    float-rounded coordinates): what the float kernels lose by themselves."""
    cs = case(orc, name, np.float32)
    pr = cs.pr
    vec, _ = cs.vectors("linear")
    u, v = np.zeros(pr.ndofs), np.zeros(pr.ndofs)
    orc.linear_rk4(cs.tdim, pr.N, pr.dm, pr.G, pr.D, vec["lin"], vec["m"], vec["src"], vec["absb"], cs.f0, P0, S0, 0.0, 0.0,
                   cs.dt, u, v, steps=sr.NSTEPS)
    ctx = make_ctx(name)
    g = run_model(cs, "linear", ctx, 0.0, sr.NSTEPS, source=False)
    ctx.close()
    assert g[0].dtype == np.float32
    return sr.rel(g[0], u), sr.rel(g[1], v)


@pytest.mark.parametrize("which", ["onset", "ramp_end", "burst_end"])
@pytest.mark.parametrize("name", ["3d", "2d"])
def test_fp32_vs_double_stepper(orc, name, which):
    """err <= 4 yard per field: 2 for the run-to-run order of the LDS sums x 2 for the second
    rounding of the weights (facet weight x waveform, rounded to float once more)."""
    cs = case(orc, name, np.float32)
    t0, D = cs.t0s()[which]
    amp, tau = (a.astype(np.float32) for a in cs.aperture())
    ctx = make_ctx(name)
    u, v = run_model(cs, "linear", ctx, t0, sr.NSTEPS, amp, tau, D)
    ctx.close()
    assert u.dtype == np.float32
    ref = reference(orc, name, "linear", 0, which, 4, np.float32)
    yard = fp32_yard(orc, name)
    err = sr.rel(u, ref[0]), sr.rel(v, ref[1])
    print(f"source fp32 {name} {which}: err u {err[0]:.3e} v {err[1]:.3e}   yard u {yard[0]:.3e} v {yard[1]:.3e}")
    assert err[0] <= 4 * yard[0] and err[1] <= 4 * yard[1]


# ---- 9. focusing ----------------------------------------------------------------------------------------------------------------
LAMBDAS, FOCAL = 8, 4          # box of 8 x 8 wavelengths, focus on the axis 4 wavelengths deep


@functools.lru_cache(maxsize=None)
def focus_setup(orc):
    P, c0, rho0 = 4, 1500.0, 1000.0
    n = (2 * LAMBDAS, 2 * LAMBDAS)              # two elements per wavelength
    h = 0.0015
    lam = 2 * h
    f0 = c0 / lam
    pr = Problem(orc, n, P, hi=[LAMBDAS * lam] * 2)
    tags = fa.tag_box_boundary(pr.mesh)
    X = pr.V.tabulate_dof_coordinates()[:, :2]
    focus = np.array([FOCAL * lam, 0.5 * LAMBDAS * lam])
    tau = fsrc.focus_delays(X, focus, c0)       # over all DOFs; only the source side x = 0 counts
    face = np.flatnonzero(pr.facet_diag(tags, 1, np.ones(pr.mesh.num_cells)))
    tau = tau - tau[face].min()
    tau[tau < 0] = 0.0
    t_end = LAMBDAS / f0 + 4.0 / f0 + tau[face].max()          # transit + ramp + max delay
    dt, nsteps, skip, spp = fmon.whole_period_window(f0, 0.5 * h / (c0 * P**2), t_end, 2)
    ifoc = int(np.argmin(np.linalg.norm(X - focus, axis=1)))
    m, src, absb, lin = pr.linear_model_vectors(c0, rho0, tags)
    return dict(pr=pr, tags=tags, tau=tau, f0=f0, dt=dt, nsteps=nsteps, skip=skip, ifoc=ifoc, P=P, c0=c0, rho0=rho0,
                vec=dict(m=m, src=src, absb=absb, lin=lin))


def focus_reference(orc):
    """(G_ref, final u with the delays) from the stepper: RMS over the last two whole periods at the focus DOF."""
    S = focus_setup(orc)
    pr, out = S["pr"], {}
    for key, tau in (("focused", S["tau"]), ("plain", 0.0)):
        q = np.zeros(1)

        def on_step(s, u, v, q=q):
            if s > S["skip"]:
                q[0] += u[S["ifoc"]] ** 2
        u, _ = sr.rk_stepper(pr, S["vec"], 1.0, S["f0"], P0, 0.0, S["dt"], S["nsteps"], 1.0, tau, on_step=on_step)
        out[key] = (np.sqrt(q[0] / (S["nsteps"] - S["skip"])), u)
    return out["focused"][0] / out["plain"][0], out["focused"][1]


def test_focusing_gain(orc):
    """A flat aperture (the whole side x = 0 of an 8 x 8 wavelength box, two p = 4 elements per wavelength) focused
    with source.focus_delays on the axis 4 wavelengths deep; the monitor's RMS map over the last two whole periods of
    a run of transit time + ramp + max delay.  G = RMS at the DOF nearest the focus with the delays / without them.
    Condition on the inputs, checked with the stepper on the CPU: G_ref >= 2 -- G_ref = 3.77 for this geometry (875 steps).
    Asserted: G_gpu >= 1.5, and the final u against the stepper within 4 x the error of the default path against
    orc.linear_rk4 over the same steps on the same mesh, measured here."""
    S = focus_setup(orc)
    pr = S["pr"]
    G_ref, u_ref = focus_reference(orc)
    print(f"source focusing: G_ref {G_ref:.4f}, {S['nsteps']} steps, window after step {S['skip']}")
    assert G_ref >= 2.0
    nc = pr.mesh.num_cells
    rms, u_fin = {}, {}
    for key in ("focused", "plain"):
        ctx = fa.Context(0)
        mdl = fa.LinearSpectralExplicit(pr.mesh, S["tags"], S["P"], np.full(nc, S["c0"]), np.full(nc, S["rho0"]), S["f0"],
                                        P0, S0, 4, S["dt"], V=pr.V, ctx=ctx)
        mdl.init()
        if key == "focused":
            mdl.set_source(delay=S["tau"])
        mdl.monitor(which="u", skip=S["skip"])
        mdl.rk4_steps(0.0, S["dt"], S["nsteps"])
        assert mdl.monitor_info()[0] == S["nsteps"] - S["skip"]
        rms[key] = mdl.monitor_get("rms").x.array[S["ifoc"]]
        mdl.u_sol()
        u_fin[key] = mdl.u_n.x.array.copy()
        mdl.close()
        ctx.close()
    G = rms["focused"] / rms["plain"]
    u_def, v_def = np.zeros(pr.ndofs), np.zeros(pr.ndofs)
    V = S["vec"]
    orc.linear_rk4(2, pr.N, pr.dm, pr.G, pr.D, V["lin"], V["m"], V["src"], V["absb"], S["f0"], P0, S0, 0.0, 0.0, S["dt"],
                   u_def, v_def, steps=S["nsteps"])
    yard, err = sr.rel(u_fin["plain"], u_def), sr.rel(u_fin["focused"], u_ref)
    print(f"source focusing: G_gpu {G:.4f}; final u err {err:.3e}, default path vs oracle {yard:.3e}")
    assert G >= 1.5
    assert err <= 4 * yard
