"""The on-device field monitor (fusmi.h "field monitor"; model.monitor / monitor_get): per-DOF running max / min, mean,
RMS and the cosine / sine coefficients of the harmonics of the source frequency, accumulated by one HIP kernel after
selected steps from the state resident in HBM.

(1) the kernel against numpy accumulation of the GPU's own states, at the summation's rounding bound;
(2) the three models against the oracle stepped one step at a time, at the tolerance the states are held to;
(3) the harmonics of the reference's Westervelt validation case against the Fubini series, reference threshold;
(4) slab ranks (in-process transport, external stage API) against the single model;
(5) life cycle and argument checks."""
import ctypes as C

import numpy as np
import pytest
from scipy.special import jv

import fenicsxfus_amd as fa
from fenicsxfus_amd import _abi, monitor
from live_cases import case
from util import Problem, live_state

pytestmark = pytest.mark.gpu
F0, P0, S0 = 0.5e6, 6e4, 1500.0
EPS = 2.0 ** -53


def maps(mdl, nharm):
    """Every quantity of the monitor as {name: array} ("cos1", "sin1", ...)."""
    out = {q: mdl.monitor_get(q).x.array.copy() for q in ("max", "min", "mean", "rms")}
    for k in range(1, nharm + 1):
        out[f"cos{k}"] = mdl.monitor_get("cos", k).x.array.copy()
        out[f"sin{k}"] = mdl.monitor_get("sin", k).x.array.copy()
    return out


def accumulate(states, times, freq, nharm):
    """The definitions of fusmi.h in numpy, sequentially in double over the samples (states promoted)."""
    x0 = np.asarray(states[0])
    mx, mn = x0.copy(), x0.copy()
    S, Q = np.zeros(len(x0)), np.zeros(len(x0))
    Ck, Sk = [np.zeros(len(x0)) for _ in range(nharm)], [np.zeros(len(x0)) for _ in range(nharm)]
    for x, t in zip(states, times):
        mx, mn = np.maximum(mx, x), np.minimum(mn, x)
        xd = np.asarray(x, dtype=np.float64)
        S += xd
        Q += xd * xd
        for k in range(1, nharm + 1):
            Ck[k - 1] += xd * np.cos(2.0 * np.pi * k * freq * t)
            Sk[k - 1] += xd * np.sin(2.0 * np.pi * k * freq * t)
    n = len(states)
    out = {"max": mx, "min": mn, "mean": S / n, "rms": np.sqrt(Q / n)}
    for k in range(1, nharm + 1):
        out[f"cos{k}"], out[f"sin{k}"] = 2.0 / n * Ck[k - 1], 2.0 / n * Sk[k - 1]
    return out


def within(out, ref, bound):
    """|value - ref| <= bound for the value the library computed in double.  A double model returns that value.  A
    float model returns it rounded to float (out is T[ndofs]); rounding is monotone, so the bound holds for the double
    value exactly when the float lies between the rounded ends of [ref - bound, ref + bound]."""
    if out.dtype == np.float64:
        return bool(np.all(np.abs(out - ref) <= bound))
    return bool(np.all(((ref - bound).astype(np.float32) <= out) & (out <= (ref + bound).astype(np.float32))))


# ---- (1) the kernel against the GPU's own states --------------------------------------------------------------------
KERNEL_CASES = {f"{'f64' if dt_ == np.float64 else 'f32'}-p{P}": dict(n=(4, 3, 3), P=P, dtype=dt_, which="u")
                for dt_ in (np.float64, np.float32) for P in (2, 4, 7)}
KERNEL_CASES["f64-quad-p4"] = dict(n=(5, 4), P=4, dtype=np.float64, which="u")
KERNEL_CASES["f64-p4-v"] = dict(n=(4, 3, 3), P=4, dtype=np.float64, which="v")


def _linear(pr, ctx, P, dt):
    nc, dt_ = pr.mesh.num_cells, pr.dtype
    return fa.LinearSpectralExplicit(pr.mesh, fa.tag_box_boundary(pr.mesh), P, np.full(nc, 1500.0, dt_),
                                     np.full(nc, 1000.0, dt_), F0, P0, S0, 4, dt, V=pr.V, ctx=ctx)


@pytest.mark.parametrize("name", list(KERNEL_CASES))
def test_kernel_against_the_gpus_own_states(orc, name):
    """monitor(nharm=3, skip=2, every=2) over 12 steps taken one rk4_steps call each: samples after steps 4, 6, 8, 10,
    12.  MAX / MIN bit-equal to numpy over the pulled states; MEAN, COS_k, SIN_k within 16 n 2^-53 max|x| per DOF (the
    sequential-summation bound of n double additions, with room for FMA contraction and an ulp of libm in the phase
    factors); RMS within the same bound relative to its own value; x = the sampled vector (u, or v for which="v").
    Then the same 12 steps in ONE rk4_steps call on a fresh model (steps 2.. replayed from the captured graph): every
    quantity bit-identical.  deterministic=1: the states themselves are reproducible bit for bit."""
    kw = KERNEL_CASES[name]
    n, P, which, nharm = kw["n"], kw["P"], kw["which"], 3
    h = 0.003
    pr = Problem(orc, n, P, hi=[h * k for k in n], perturb=0.1, dtype=kw["dtype"])
    dt = 0.5 * h / (1500.0 * P**2)
    u0, v0 = live_state(pr, 11, P0, F0)

    def fresh():
        ctx = fa.Context(0, deterministic=True)
        ctx.set_option("graph", 1)
        mdl = _linear(pr, ctx, P, dt)
        mdl.init()
        mdl.set_state(u0, v0)
        mdl.monitor(which=which, nharm=nharm, skip=2, every=2)
        return ctx, mdl

    ctx, mdl = fresh()
    t, states, times = 0.0, [], []
    for s in range(1, 13):
        mdl.rk4_steps(t, dt, 1)
        t += dt
        mdl.u_sol()                                       # pulls u and v
        x = (mdl.u_n if which == "u" else mdl.v_n).x.array.copy()
        if s in (4, 6, 8, 10, 12):
            states.append(x), times.append(t)
    got = maps(mdl, nharm)
    info = mdl.monitor_info()
    mdl.close(), ctx.close()
    nsamp = len(states)
    assert info == (5, times[0], times[-1])
    ref = accumulate(states, times, F0, nharm)
    top = max(np.abs(x).max() for x in states)
    assert top > 0
    bound = 16 * nsamp * EPS * float(top)
    assert got["max"].dtype == pr.dtype
    assert np.array_equal(got["max"], ref["max"]) and np.array_equal(got["min"], ref["min"])
    worst = {}
    for q in ref:
        if q in ("max", "min"):
            continue
        b = 16 * nsamp * EPS * ref[q] if q == "rms" else bound
        worst[q] = float((np.abs(got[q] - ref[q]) / b).max())
    print(f"{name}: error / bound per quantity {worst}")
    for q in worst:
        b = 16 * nsamp * EPS * ref[q] if q == "rms" else bound
        assert within(got[q], ref[q], b), (q, worst[q])
    assert all(np.abs(ref[q]).max() > 0 for q in ref)                            # no quantity compared at zero
    # one call, graph replay
    ctx, mdl = fresh()
    mdl.rk4_steps(0.0, dt, 12)
    again = maps(mdl, nharm)
    assert mdl.monitor_info() == info
    mdl.close(), ctx.close()
    for q in got:
        assert np.array_equal(got[q], again[q]), q


# ---- (2) against the oracle -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["linear", "lossy", "westervelt"])
def test_against_the_oracle(orc, kind):
    """Heterogeneous perturbed (6, 5, 4) box at degree 4 (the box of test_python_forms_vs_oracle), live start, 20 steps,
    every=1, nharm=2; the oracle advanced one step at a time and accumulated in numpy.  Every quantity is an extremum
    or a weighted mean (weights <= 2) of states the library holds to 1e-10 max|u| after 20 steps: 2e-10 max|u|."""
    cs = case(orc, f"{kind}-p4")
    nsteps, nharm = 20, 2
    u0, v0 = cs.start()
    ctx = fa.Context(0)
    mdl = cs.model(ctx)
    mdl.init()
    mdl.set_state(u0, v0)
    mdl.monitor(nharm=nharm, every=1)
    mdl.rk4_steps(0.0, cs.dt, nsteps)
    got = maps(mdl, nharm)
    n_, t0_, t1_ = mdl.monitor_info()
    mdl.close(), ctx.close()
    u, v, t, states, times = u0.copy(), v0.copy(), 0.0, [], []
    for _ in range(nsteps):
        u, v = cs.oracle(u, v, t0=t, nsteps=1, fixed=True)
        t += cs.dt
        states.append(u.copy()), times.append(t)
    assert (n_, t0_, t1_) == (nsteps, times[0], times[-1])
    ref = accumulate(states, times, F0, nharm)
    top = max(np.abs(x).max() for x in states)
    err = {q: float(np.abs(got[q] - ref[q]).max() / top) for q in ref}
    print(f"{kind}: max error / max|u| per quantity {err}")
    for q in ref:
        assert np.abs(ref[q]).max() > 0, q                                           # the reference maps are live
        assert err[q] < 2e-10, (q, err[q])


# ---- (3) harmonics against the Fubini series --------------------------------------------------------------------------
@pytest.mark.parametrize("degree,epw", [(3, 16), (4, 8), (5, 4), (6, 2)])
def test_harmonics_against_fubini(orc, degree, epw):
    """The reference's Westervelt validation case (test_westerveltspectral_1d.py:12-127, the parameters of
    test_westerveltspectral_L2) read as the harmonic statement it is: u = p0 sum_k B_k sin(k w0 (t - X / c0)) with
    B_k = 2 / (k sigma) J_k(k sigma), so COS_k = -p0 B_k sin(k w0 X / c0), SIN_k = p0 B_k cos(k w0 X / c0).  Window:
    the last two periods of L / c0 + 8 / f0, dt the largest step <= the CFL one that divides the period.  For
    k = 1..4 the combined GLL-weighted L2 error of (COS_k, SIN_k), relative to the exact fundamental, is below the
    reference's threshold 1e-1.  (The CPU oracle through the same procedure: <= 1.9e-3, 3.0e-3, 2.1e-2, 2.6e-2.)"""
    from test_gpu_reference_python_tests import interval_as_box
    f0, c0, rho0, beta0, L, nharm = 10.0, 1.0, 1.0, 0.01, 1.0, 4
    w0, u0 = 2 * np.pi * f0, 1.0
    p0 = rho0 * c0 * u0
    pr, tags, h = interval_as_box(orc, degree, epw, f0, c0, L)
    nc = pr.mesh.num_cells
    dt, nsteps, skip, spp = monitor.whole_period_window(f0, 0.9 * h / (c0 * degree**2), L / c0 + 8 / f0, 2, nharm=nharm)
    ctx = fa.Context(0)
    mdl = fa.WesterveltSpectralExplicit(pr.mesh, tags, degree, np.full(nc, c0), np.full(nc, rho0), np.zeros(nc),
                                        np.full(nc, beta0), f0, p0, c0, 4, dt, V=pr.V, ctx=ctx, forms="python")
    mdl.init()
    mdl.monitor(nharm=nharm, skip=skip, every=1)
    mdl.rk4_steps(0.0, dt, nsteps)
    assert mdl.monitor_info()[0] == 2 * spp
    got = maps(mdl, nharm)
    mdl.close(), ctx.close()
    X = pr.V.tabulate_dof_coordinates()[:, 0]
    sigma = (X + 0.0000001) / (c0**2 / w0 / beta0 / u0)
    w = pr.M(np.ones(pr.ndofs))                                                   # GLL-collocated L2 norm
    norm = lambda a, b: np.sqrt(w @ (a**2 + b**2))  # noqa: E731
    exact = {}
    for k in range(1, nharm + 1):
        B = p0 * 2 / (k * sigma) * jv(k, k * sigma)
        exact[k] = (-B * np.sin(k * w0 * X / c0), B * np.cos(k * w0 * X / c0))
    h1 = norm(*exact[1])
    err = {k: float(norm(got[f"cos{k}"] - exact[k][0], got[f"sin{k}"] - exact[k][1]) / h1) for k in exact}
    ratio = float(norm(got["cos2"], got["sin2"]) / norm(got["cos1"], got["sin1"]))
    print(f"degree {degree} epw {epw}: error relative to the fundamental {err}, |h2| / |h1| = {ratio:.3f}")
    for k in err:
        assert err[k] < 1e-1, (k, err[k])
    assert ratio > 0.1                                                            # the second harmonic is really there
    amp2 = monitor.amplitude(got["cos2"], got["sin2"])
    assert np.abs(amp2 - np.hypot(got["cos2"], got["sin2"])).max() == 0


# ---- (4) transports ---------------------------------------------------------------------------------------------------
def _slab_setup(orc, make_ctx):
    import test_multirank as tm
    pr = Problem(orc, tm.N_GLOBAL, tm.P, hi=tm.HI, perturb=0.1)
    dt = tm.dt_value()
    u0, v0 = live_state(pr, tm.SEED, tm.P0, tm.F0)
    c, rho = tm.material(pr.mesh)
    ctx = fa.Context(0)
    one = fa.LinearSpectralExplicit(pr.mesh, fa.tag_box_boundary(pr.mesh), tm.P, c, rho, tm.F0, tm.P0, tm.S0, 4, dt,
                                    V=pr.V, ctx=ctx)
    one.init()
    one.set_state(u0, v0)
    one.monitor(nharm=2, every=1)
    one.rk4_steps(0.0, dt, tm.NSTEPS)
    ref = maps(one, 2)
    top = np.abs(ref["max"]).max()
    info = one.monitor_info()
    one.close(), ctx.close()
    return tm, dt, (u0, v0), ref, float(top), info, [make_ctx(r) for r in range(2)]


def _slab_models(tm, dt, ctxs):
    models, offs = [], []
    for r, cx in enumerate(ctxs):
        mesh = fa.BoxMesh([0, 0, 0], tm.HI, tm.N_GLOBAL, rank=r, size=len(ctxs), perturb=0.1)
        V = fa.FunctionSpace(mesh, tm.P)
        c, rho = tm.material(mesh)
        models.append(fa.LinearSpectralExplicit(mesh, fa.tag_box_boundary(mesh), tm.P, c, rho, tm.F0, tm.P0, tm.S0, 4, dt,
                                                V=V, ctx=cx))
        offs.append(V.global_offset)
    return models, offs


def _check_slabs(models, offs, ref, top, info):
    got = [maps(mdl, 2) for mdl in models]
    for r, mdl in enumerate(models):
        assert mdl.monitor_info() == info
        k = mdl.data.ndofs
        for q in ref:
            assert np.abs(ref[q]).max() > 0
            assert np.abs(got[r][q] - ref[q][offs[r]:offs[r] + k]).max() < 1e-10 * top, (r, q)
    plane = models[0].data.ndofs - (offs[1] - offs[0])                           # the shared interface plane
    assert plane > 0
    for q in ref:
        assert np.array_equal(got[0][q][-plane:], got[1][q][:plane]), q


def test_slabs_in_process(orc):
    """Two x-slabs advanced by group_rk4_steps: each rank's maps are the single model's on its DOFs (1e-10 max|u|, the
    tolerance test_multirank.py holds the states to), and bit-identical on the plane both hold."""
    tm, dt, (u0, v0), ref, top, info, ctxs = _slab_setup(orc, lambda r: fa.Context(0))
    fa.Context.init_local_group(ctxs)
    models, offs = _slab_models(tm, dt, ctxs)
    fa.group_finish_setup(models)
    for mdl, off in zip(models, offs):
        mdl.init()
        mdl.set_state(u0[off:off + mdl.data.ndofs], v0[off:off + mdl.data.ndofs])
        mdl.monitor(nharm=2, every=1)
    fa.group_rk4_steps(models, 0.0, dt, tm.NSTEPS)
    _check_slabs(models, offs, ref, top, info)
    for mdl in models:
        mdl.close()
    for cx in ctxs:
        cx.close()


def test_slabs_external_stage_api(orc):
    """The same through the external-transport stage halves, the exchange done here by device copies."""
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]

    def make_ctx(r):
        cx = fa.Context(0)
        cx.init_external(r, 2)
        return cx

    tm, dt, (u0, v0), ref, top, info, ctxs = _slab_setup(orc, make_ctx)
    models, offs = _slab_models(tm, dt, ctxs)
    layouts = [mdl.data.halo_layout() for mdl in models]
    bufs = [mdl.data.halo_buffers() for mdl in models]

    def exchange():
        for r in range(2):
            for q, cnt, off in zip(*layouts[r]):
                k = list(layouts[q][0]).index(r)
                assert layouts[q][1][k] == cnt
                assert hip.hipMemcpy(bufs[q][1] + 8 * int(layouts[q][2][k]), bufs[r][0] + 8 * int(off), 8 * int(cnt), 3) == 0

    for k in range(models[0].setup_count()):
        for mdl in models:
            mdl.setup_pack(k)
        exchange()
        for mdl in models:
            mdl.setup_unpack(k)
    for mdl, off in zip(models, offs):
        mdl.setup_finish()
        mdl.init()
        mdl.set_state(u0[off:off + mdl.data.ndofs], v0[off:off + mdl.data.ndofs])
        mdl.monitor(nharm=2, every=1)
    t = 0.0
    for _ in range(tm.NSTEPS):
        for i in range(4):
            for mdl in models:
                mdl.stage_begin(i, t, dt)
            exchange()
            for mdl in models:
                mdl.stage_end(i, t, dt)
        t += dt
    _check_slabs(models, offs, ref, top, info)
    for mdl in models:
        mdl.close()
    for cx in ctxs:
        cx.close()


# ---- (5) life cycle -----------------------------------------------------------------------------------------------------
@pytest.fixture()
def small(orc):
    h, n, P = 0.003, (4, 3, 3), 4
    pr = Problem(orc, n, P, hi=[h * k for k in n], perturb=0.1)
    dt = 0.5 * h / (1500.0 * P**2)
    ctx = fa.Context(0, deterministic=True)
    mdl = _linear(pr, ctx, P, dt)
    mdl.init()
    mdl.set_state(*live_state(pr, 11, P0, F0))
    yield pr, mdl, dt
    mdl.close(), ctx.close()


def _raises(code):
    return pytest.raises(fa.FusError, match=rf"libfusmi error {code}:")


def test_restart_count_and_off(small):
    pr, mdl, dt = small
    with _raises(-4):                                    # never switched on
        mdl.monitor_get("max")
    mdl.monitor(nharm=1, skip=1, every=1)
    with _raises(-4):                                    # on, no sample yet
        mdl.monitor_get("max")
    mdl.rk4_steps(0.0, dt, 1)
    assert mdl.monitor_info()[0] == 0                    # step 1 is skipped
    with _raises(-4):
        mdl.monitor_get("max")
    mdl.rk4_steps(dt, dt, 3)
    first = maps(mdl, 1)
    assert mdl.monitor_info()[0] == 3
    assert np.array_equal(maps(mdl, 1)["rms"], first["rms"])          # a get does not alter the accumulators
    # a second call restarts from zero: one sample of the current state
    mdl.monitor(nharm=0, every=1, count=2)
    mdl.rk4_steps(4 * dt, dt, 1)
    u = mdl.u_sol().x.array
    n, t0, t1 = mdl.monitor_info()
    assert n == 1 and t0 == t1 == 4 * dt + dt
    for q in ("max", "min", "mean"):
        assert np.array_equal(mdl.monitor_get(q).x.array, u), q
    assert np.all(np.abs(mdl.monitor_get("rms").x.array - np.abs(u)) <= 4 * EPS * np.abs(u))
    with _raises(-1):                                    # nharm = 0 now: no harmonic to ask for
        mdl.monitor_get("cos", 1)
    # count caps n
    mdl.rk4_steps(5 * dt, dt, 4)
    assert mdl.monitor_info()[0] == 2
    mdl.monitor_off()
    with _raises(-4):
        mdl.monitor_get("max")
    with _raises(-4):
        mdl.monitor_info()
    mdl.rk4_steps(9 * dt, dt, 1)                         # stepping goes on without it


def test_argument_errors(small):
    pr, mdl, dt = small
    lib, h = _abi.lib(), mdl.h
    call = lambda which, nharm, every, skip=0, count=0: lib.fus_model_monitor(  # noqa: E731
        h, C.c_int(which), C.c_int(nharm), C.c_double(0.0), C.c_int64(skip), C.c_int(every), C.c_int64(count))
    assert call(0, 9, 1) == -1
    assert call(0, -1, 1) == -1
    assert call(0, 1, -1) == -1
    assert call(2, 1, 1) == -1
    assert call(0, 1, 1, skip=-1) == -1 and call(0, 1, 1, count=-1) == -1
    with _raises(-1):
        mdl.monitor(nharm=9)
    with _raises(-1):
        mdl.monitor(every=-1)
    mdl.monitor(nharm=2, every=1)
    mdl.rk4_steps(0.0, dt, 2)
    out = np.zeros(pr.ndofs)
    get = lambda q, k: lib.fus_model_monitor_get(h, C.c_int(q), C.c_int(k), _abi.ptr(out), C.c_int(_abi.FUS_HOST))  # noqa: E731
    assert get(6, 0) == -1 and get(-1, 0) == -1          # bad quantity
    assert get(_abi.FUS_MON_COS, 0) == -1 and get(_abi.FUS_MON_SIN, 3) == -1      # k outside 1..nharm
    assert get(_abi.FUS_MON_COS, 2) == 0 and get(_abi.FUS_MON_MAX, 99) == 0       # k ignored for the others
    with pytest.raises(fa.FusError, match="unknown monitor quantity"):
        mdl.monitor_get("peak")
    for bad in ("U", "p", ""):
        with pytest.raises(fa.FusError, match="unknown monitor field"):
            mdl.monitor(which=bad)
    assert mdl.monitor_info()[0] == 2                    # the rejected calls did not restart the window


def test_monitor_leaves_the_run_alone_and_works_beside_the_receivers(orc):
    """12 steps with the monitor (and the receivers' recording) on leave (u, v) and the records bit-identical to the
    same run with the monitor off; both see every step, at the same times."""
    h, n, P = 0.003, (4, 3, 3), 4
    pr = Problem(orc, n, P, hi=[h * k for k in n], perturb=0.1)
    dt = 0.5 * h / (1500.0 * P**2)
    u0, v0 = live_state(pr, 11, P0, F0)
    pts = np.random.default_rng(4).uniform([0, 0, 0], [h * k for k in n], size=(9, 3))
    res = {}
    for on in (False, True):
        ctx = fa.Context(0, deterministic=True)
        mdl = _linear(pr, ctx, P, dt)
        mdl.init()
        mdl.set_state(u0, v0)
        assert len(mdl.set_receivers(pts)) == 9
        mdl.record(1, 16)
        if on:
            mdl.monitor(nharm=4, every=1)
        mdl.rk4_steps(0.0, dt, 12)
        u = mdl.u_sol().x.array.copy()
        times, rec = mdl.records()
        res[on] = (u, mdl.v_n.x.array.copy(), times, rec)
        if on:
            assert mdl.monitor_info() == (12, times[0], times[-1])
            mx = mdl.monitor_get("max").x.array
            assert np.all(mx >= u) and np.all(mdl.monitor_get("min").x.array <= u)
        mdl.close(), ctx.close()
    for a, b in zip(res[False], res[True]):
        assert np.array_equal(a, b)
    assert len(res[True][2]) == 12
