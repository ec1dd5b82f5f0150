"""The device-side receivers (fus_model_set_receivers / _sample / _record / _get_records, k_sample) at every degree, in
both types, on distorted cells, while recording under every stepping path, and on several ranks.

(1) sampling matrix: P = 2..10 on perturbed hexahedra and quadrilaterals plus the Gmsh fixture, fp64 and fp32, a
    random and a smooth field, against the long-double interpolant at points whose (cell, X) is known by
    construction, per point class, at the budget of receiver_ref.py (CPU guards: test_receivers_host.py);
(2) receiver counts 1, 2, 3, 5 and 258: every point's sample is bit for bit its row of the 258-point result;
(3) recording on one rank: the three models, RK4 lean / with accumulators, orders 2 and 3, quadrilaterals, fp32,
    graph replay and rk(t0, tf) with a remainder step: every record is bit for bit the sample of a twin model stepped
    that far, at the loop's times, the last one at the oracle's state; capacity stop, restart, no receiver at all;
(4) several ranks (in-process group, external stage API): who holds which point, each rank's sample against the
    single model's, sharers of an interface point against each other, and recording on every rank -- also on those
    that hold no receiver -- against a twin group, with the monitor running beside it.

Runs that are compared bit for bit use deterministic = 1 (the elements of a block accumulate in a fixed order), the
setting under which the project asserts that a run repeats its bits."""
import ctypes as C

import numpy as np
import pytest

import fenicsxfus_amd as fa
import receiver_ref as rr
import test_multirank as tm
from fenicsxfus_amd.evaluate import locate
from live_cases import TOL_F32_VS_F64, TOL_RK, Case
from util import Problem, live_state

pytestmark = pytest.mark.gpu
TYPES = {"f64": np.float64, "f32": np.float32}
IDS = [f"{g}-p{P}" for g, P in rr.MATRIX]


# ---- (1) sampling matrix -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tname", list(TYPES))
@pytest.mark.parametrize("geom,P", rr.MATRIX, ids=IDS)
def test_sampling_matrix(geom, P, tname):
    """set_state(u = random, v = smooth); sample("u") and sample("v") per point class: (a) against the truth, the
    long-double interpolant at the constructed (cell, X), (b) the kernel alone, against the long-double interpolant
    at the located pair; both at cap x the error of the sequential restatement in the model's type.  The points
    outside are dropped, the same call gives the same bits."""
    T = TYPES[tname]
    cs = rr.sample_case(geom, P, T)
    p = cs.points
    ctx = fa.Context(0)
    mdl = cs.model(ctx)
    try:
        on = mdl.set_receivers(p.pts)
        assert np.array_equal(on, p.inside)
        mdl.set_state(u=cs.u, v=cs.v)
        us, vs = mdl.sample("u"), mdl.sample("v")
        again = mdl.sample("u"), mdl.sample("v")
    finally:
        mdl.close(), ctx.close()
    assert us.dtype == T and us.shape == (p.n_inside,)
    assert np.array_equal(us, again[0]) and np.array_equal(vs, again[1])
    rr.check(f"{cs.label} truth", (us, vs), cs.pair(cs.yard), cs.pair(cs.ref), p.regions, T)
    rr.check(f"{cs.label} kernel", (us, vs), cs.pair(cs.yard), cs.pair(cs.kref), p.regions, T)


# ---- (2) receiver counts ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom,P", rr.COUNT_CASES)
def test_receiver_counts(geom, P):
    """(n + 3) / 4 blocks of four waves: with 1, 2, 3 and 5 receivers the tail waves of the last block leave early.  No
    receiver depends on its neighbours in the block: each sample is its row of the 258-point result, bit for bit."""
    cs = rr.sample_case(geom, P)
    pts = cs.points.pts[:rr.N_COUNTS]
    ctx = fa.Context(0)
    mdl = cs.model(ctx)
    try:
        mdl.set_state(u=cs.u, v=cs.v)
        assert len(mdl.set_receivers(pts)) == rr.N_COUNTS
        full = {f: mdl.sample(f) for f in ("u", "v")}
        got = {}
        for n, idx in rr.SUBSETS.items():
            assert len(mdl.set_receivers(pts[idx])) == n
            got[n] = {f: mdl.sample(f) for f in ("u", "v")}
    finally:
        mdl.close(), ctx.close()
    assert np.abs(full["u"]).min() > 0
    for n, idx in rr.SUBSETS.items():
        for f in ("u", "v"):
            assert got[n][f].shape == (n,) and np.array_equal(got[n][f], full[f][idx]), (n, f)


# ---- (3) recording on one rank -----------------------------------------------------------------------------------------
# kind, RK order, options, mesh, type, recorded field; every kind and every stepping form at least twice
REC_CASES = {
    "linear-rk4": dict(kind="linear"),
    "linear-rk4-acc": dict(kind="linear", opts=dict(lean_rk4=0), which="v"),
    "linear-rk2": dict(kind="linear", order=2),
    "lossy-rk4-acc": dict(kind="lossy", opts=dict(lean_rk4=0)),
    "lossy-rk3": dict(kind="lossy", order=3, which="v"),
    "lossy-rk2": dict(kind="lossy", order=2),
    "westervelt-rk4": dict(kind="westervelt", which="v"),
    "westervelt-rk3": dict(kind="westervelt", order=3),
    "linear-quad": dict(kind="linear", n=(5, 4)),
    "linear-fp32": dict(kind="linear", dtype=np.float32),
    "linear-quad-graph": dict(kind="linear", n=(5, 4), opts=dict(graph=1), which="v"),
}
_rec = {}


def rec_case(orc, name, **over):
    """(Case on the (4, 3, 3) box of test_recording_during_rk4_matches_oracle, perturb = 0.1, or on a (5, 4) rectangle;
    options; recorded field; constructed receivers).  The lower orders run at CFL 0.1 like live_cases' own."""
    kw = {**REC_CASES.get(name, {}), **over}
    key = (name, tuple(sorted((k, str(v)) for k, v in over.items())))
    if key not in _rec:
        order = kw.get("order", 4)
        cs = Case(orc, kw["kind"], n=kw.get("n", (4, 3, 3)), P=4, L=0.016, order=order, cfl=0.5 if order == 4 else 0.1,
                  dtype=kw.get("dtype", np.float64))
        _rec[key] = (cs, kw.get("opts", {}), kw.get("which", "u"), rr.Points(cs.prt.mesh, cs.prt.V.nodes1d, max_cells=4))
    return _rec[key]


def rec_model(cs, opts):
    ctx = fa.Context(0, deterministic=True)
    for k, v in opts.items():
        ctx.set_option(k, v)
    mdl = cs.model(ctx)
    u0, v0 = (a.astype(cs.dtype) for a in cs.start())
    mdl.init()
    mdl.set_state(u0, v0)
    return ctx, mdl, (u0, v0)


def times_after(t, dt, n):
    """[t + dt, t + dt + dt, ...]: the loop's own additions."""
    out = []
    for _ in range(n):
        t = t + dt
        out.append(t)
    return out


def oracle_at(cs, start, p, nsteps, which, **kw):
    """The oracle's state after ``nsteps`` steps interpolated at the constructed receivers (long double), and its
    largest value.  fp32 cases: the double oracle on the float-rounded problem."""
    u, v = cs.oracle(*start, pr=cs.pr64r, nsteps=nsteps, **kw)
    a = u if which == "u" else v
    return np.asarray(rr.interp(cs.prt.V, a, p.cell, p.X, np.longdouble), dtype=np.float64), float(np.abs(a).max())


def tol_state(cs):
    """The project's tolerance of a state against the double oracle: 1e-10 in fp64, live_cases' fp32 one in fp32."""
    return TOL_RK if cs.dtype == np.float64 else TOL_F32_VS_F64


@pytest.mark.parametrize("name", list(REC_CASES))
def test_recording_on_one_rank(orc, name):
    cs, opts, which, p = rec_case(orc, name)
    other = "v" if which == "u" else "u"
    dt, every, nsteps = cs.dt, 2, 6
    t = [0.0] + times_after(0.0, dt, 18)
    ctx, mdl, start = rec_model(cs, opts)
    ctx2, twin, _ = rec_model(cs, opts)
    try:
        on = mdl.set_receivers(p.pts)
        assert np.array_equal(on, p.inside) and np.array_equal(twin.set_receivers(p.pts), on)
        mdl.record(every=every, capacity=4, which=which)
        mdl.rk4_steps(0.0, dt, nsteps)
        times, rec = mdl.records()
        first = (times.copy(), rec.copy())
        # (a) the twin, stepped `every` steps at a time from the loop's own times
        tw = []
        for k in range(nsteps // every):
            twin.rk4_steps(t[k * every], dt, every)
            tw.append(twin.sample(which))
        # (d) capacity: six more steps add the fourth record and no fifth; a new record() starts again
        mdl.rk4_steps(t[6], dt, 6)
        times4, rec4 = mdl.records()
        mdl.record(every=1, capacity=4, which=other)
        mdl.rk4_steps(t[12], dt, 2)
        times2, rec2 = mdl.records()
        now = mdl.sample(other)
    finally:
        mdl.close(), ctx.close(), twin.close(), ctx2.close()
    n = p.n_inside
    assert rec.shape == (3, n) and rec.dtype == cs.dtype
    for k in range(3):
        assert np.array_equal(first[1][k], tw[k]), f"record {k} is not the twin's sample"                 # (a)
    assert np.allclose(first[0], [t[2], t[4], t[6]], rtol=1e-12, atol=0.0)                                 # (b)
    ref, top = oracle_at(cs, start, p, nsteps, which, exact=True)                                          # (c)
    err = np.abs(rec[2] - ref).max() / top
    print(f"recording {name}: last record against the oracle {err:.3e} of max|{which}|")
    assert top > 0 and err < tol_state(cs)
    assert rec4.shape == (4, n) and np.array_equal(rec4[:3], first[1])                                     # (d)
    assert np.allclose(times4, [t[2], t[4], t[6], t[8]], rtol=1e-12, atol=0.0)
    assert rec2.shape == (2, n) and np.allclose(times2, [t[13], t[14]], rtol=1e-12, atol=0.0)
    assert np.array_equal(rec2[1], now) and not np.array_equal(rec2[0], rec2[1])


@pytest.mark.parametrize("tname", list(TYPES))
def test_recording_through_rk_with_a_remainder_step(orc, tname):
    """rk(0, 4.4 dt): fus_model_rk4's own loop, four full steps and one of 0.4 dt, recorded after every step.  The
    times are the loop's t -- in fp32 accumulated in float, as the library documents -- and each record is the sample
    of a twin that takes the same steps one by one."""
    T = TYPES[tname]
    cs, opts, which, p = rec_case(orc, "linear-rk4", dtype=T)
    tf = 0.0 + 4 * cs.dt * (1 + 0.1)
    t, dt, tend = T(0.0), T(cs.dt), T(tf)
    steps = []
    while t < tend:
        dt = min(dt, tend - t)
        steps.append((float(t), float(dt)))
        t = t + dt
        assert isinstance(t, T)
    loop_times = [a + b if T == np.float64 else float(np.float32(a) + np.float32(b)) for a, b in steps]
    assert len(steps) == 5 and steps[-1][1] < 0.5 * cs.dt
    ctx, mdl, start = rec_model(cs, opts)
    ctx2, twin, _ = rec_model(cs, opts)
    try:
        on = mdl.set_receivers(p.pts)
        twin.set_receivers(p.pts)
        mdl.record(every=1, capacity=8, which=which)
        mdl.rk(0.0, tf)
        assert mdl.nsteps == 5
        times, rec = mdl.records()
        tw = []
        for a, b in steps:
            twin.rk4_steps(a, b, 1)
            tw.append(twin.sample(which))
    finally:
        mdl.close(), ctx.close(), twin.close(), ctx2.close()
    assert rec.shape == (5, len(on)) and len(on) == p.n_inside
    assert np.allclose(times, loop_times, rtol=1e-12, atol=0.0)
    if T == np.float32:
        assert np.array_equal(times, loop_times)                       # the float-accumulated time, exactly
    for k in range(5):
        assert np.array_equal(rec[k], tw[k]), f"record {k} is not the twin's sample"
    ref, top = oracle_at(cs, start, p, 4, which, exact=True, margin=0.1)
    err = np.abs(rec[4] - ref).max() / top
    print(f"recording rk() {tname}: last record against the oracle {err:.3e} of max|{which}|")
    assert top > 0 and err < tol_state(cs)


def test_recording_without_any_receiver(orc):
    """Every point lies outside: the steps run, every record is counted with its time and holds nothing."""
    cs, opts, which, p = rec_case(orc, "linear-rk4")
    ctx, mdl, _ = rec_model(cs, opts)
    try:
        on = mdl.set_receivers(p.pts[p.n_inside:])
        assert len(on) == 0
        assert mdl.sample("u").shape == (0,)
        mdl.record(every=2, capacity=4, which="u")
        mdl.rk4_steps(0.0, cs.dt, 6)
        times, rec = mdl.records()
        u_after = mdl.u_sol().x.array.copy()
        assert mdl.sample("v").shape == (0,)
    finally:
        mdl.close(), ctx.close()
    t = times_after(0.0, cs.dt, 6)
    assert rec.shape == (3, 0) and np.allclose(times, [t[1], t[3], t[5]], rtol=1e-12, atol=0.0)
    assert np.isfinite(u_after).all() and np.abs(u_after).max() > 0


def test_a_smaller_capacity_after_a_larger_one_is_the_limit(orc):
    """record(1, 8), eight steps, then record(1, 4) and eight more: the second recording takes four records, those of
    its first four steps, bit-equal to a model that recorded with capacity 4 from the start; and
    fus_model_get_records, called as a C caller does with ``out`` sized for what it asked for, writes 4 npts values."""
    from fenicsxfus_amd import _abi

    cs, opts, which, p = rec_case(orc, "linear-rk4")
    dt = cs.dt
    t = [0.0] + times_after(0.0, dt, 16)
    ctx, mdl, _ = rec_model(cs, opts)
    ctx2, twin, _ = rec_model(cs, opts)
    try:
        mdl.set_receivers(p.pts), twin.set_receivers(p.pts)
        n = p.n_inside
        mdl.record(every=1, capacity=8, which=which)
        mdl.rk4_steps(0.0, dt, 8)
        assert mdl.records()[1].shape == (8, n)
        mdl.record(every=1, capacity=4, which=which)
        mdl.rk4_steps(t[8], dt, 8)
        out = np.full(8 * n, np.nan)                       # twice what the caller asked for, to see an overrun
        times = np.full(8, np.nan)
        nrec = C.c_int64(-1)
        _abi.check(_abi.lib().fus_model_get_records(mdl.h, out.ctypes.data_as(C.c_void_p),
                                                    times.ctypes.data_as(C.POINTER(C.c_double)), C.byref(nrec)))
        twin.rk4_steps(0.0, dt, 8)
        twin.record(every=1, capacity=4, which=which)
        twin.rk4_steps(t[8], dt, 8)
        ttimes, trec = twin.records()
    finally:
        mdl.close(), ctx.close(), twin.close(), ctx2.close()
    assert n > 0 and cs.dtype == np.float64
    assert nrec.value == 4
    assert np.isfinite(out[:4 * n]).all() and np.isnan(out[4 * n:]).all() and np.isnan(times[4:]).all()
    assert np.allclose(times[:4], t[9:13], rtol=1e-12, atol=0.0)
    assert trec.shape == (4, n) and np.array_equal(ttimes, times[:4])
    assert np.array_equal(out[:4 * n].reshape(4, n), trec)
    assert not np.array_equal(trec[0], trec[3])


# ---- (4) several ranks ---------------------------------------------------------------------------------------------------
MR_CASES = {            # transport, slabs, degree, dimension, monitor beside the recording
    "group-2": ("local", 2, 4, 3, True),
    "group-3": ("local", 3, 4, 3, False),
    "external-3": ("external", 3, 4, 3, False),
    "group-2-p7": ("local", 2, 7, 3, False),
    "group-2-quad": ("local", 2, 4, 2, False),
}
IF_X = [(0.5, 0.5), (0.25, 0.75), (0.0, 0.5), (1.0, 1.0), (0.75, 0.0)]   # on each cut: inside a face, on an edge, a vertex
_mr = {}


def mr_problem(orc, P, tdim):
    """The problem of test_multirank.py (its box, materials, live start) at degree P, or its x-y rectangle."""
    if (P, tdim) not in _mr:
        n, hi = tm.N_GLOBAL[:tdim], tm.HI[:tdim]
        pr = Problem(orc, n, P, hi=hi, perturb=0.1)
        dt = 0.5 * (hi[0] / n[0]) / (2800.0 * P**2)
        _mr[P, tdim] = (pr, dt, live_state(pr, tm.SEED, tm.P0, tm.F0))
    return _mr[P, tdim]


def mr_receivers(pr, size):
    """(a) 50 points: a line along x through all slabs and, placed exactly on every interface, len(IF_X) points each
    (the forward map of the cell left of the cut at X0 = 1); (b) a short line inside the last slab only.  Returns
    (a, b, {cut index: rows of a on that cut})."""
    n, hi, t = pr.mesh.n, pr.mesh.hi, pr.tdim
    cuts = [(n[0] * r) // size for r in range(1, size)]
    mid = tuple(k // 2 for k in n[1:])
    cells, X = [], []
    for c in cuts:
        for yz in IF_X:
            cells.append(np.ravel_multi_index((c - 1,) + mid, n))
            X.append((1.0,) + yz[:t - 1])
    on_cut = rr.forward(pr.mesh, np.array(cells), np.array(X))
    nline = 50 - len(on_cut)
    line = np.stack([np.linspace(0.0, hi[0], nline)] + [np.full(nline, 0.5 * hi[d]) for d in range(1, t)], axis=1)
    a = np.vstack([line, on_cut])
    h = hi[0] / n[0]
    xb = np.linspace((cuts[-1] + 0.3) * h, hi[0] - 0.2 * h, 7)
    b = np.stack([xb] + [np.full(7, 0.45 * hi[d]) for d in range(1, t)], axis=1)
    rows = {j: nline + j * len(IF_X) + np.arange(len(IF_X)) for j in range(len(cuts))}
    return a, b, rows


class Group:
    """``size`` slab models on one GPU from the live start: an in-process group (group_rk4_steps) or the external stage
    API with the exchange of test_external_transport_gpu (device copies between the ranks' buffers)."""

    def __init__(self, transport, size, pr, dt, start):
        self.transport, self.size, self.dt, self.t = transport, size, dt, 0.0
        P, t = pr.P, pr.tdim
        self.ctxs, self.models, self.offs = [], [], []
        for r in range(size):
            cx = fa.Context(0, deterministic=True)
            if transport == "external":
                cx.init_external(r, size)
            self.ctxs.append(cx)
        if transport == "local":
            fa.Context.init_local_group(self.ctxs)
        for r, cx in enumerate(self.ctxs):
            mesh = fa.BoxMesh([0.0] * t, tm.HI[:t], tm.N_GLOBAL[:t], rank=r, size=size, perturb=0.1)
            V = fa.FunctionSpace(mesh, P)
            c, rho = tm.material(mesh)
            self.models.append(fa.LinearSpectralExplicit(mesh, fa.tag_box_boundary(mesh), P, c, rho, tm.F0, tm.P0, tm.S0,
                                                         4, dt, V=V, ctx=cx))
            self.offs.append(V.global_offset)
        if transport == "local":
            fa.group_finish_setup(self.models)
        else:
            self._external_setup()
        for mdl, off in zip(self.models, self.offs):
            k = mdl.data.ndofs
            mdl.init()
            mdl.set_state(start[0][off:off + k], start[1][off:off + k])

    def _external_setup(self):
        hip = C.CDLL("libamdhip64.so")
        hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        layouts = [mdl.data.halo_layout() for mdl in self.models]
        bufs = [mdl.data.halo_buffers() for mdl in self.models]

        def exchange():
            """rank r's send range for neighbour q -> q's receive range for neighbour r (8-byte values)."""
            for r in range(self.size):
                for q, cnt, off in zip(*layouts[r]):
                    k = list(layouts[q][0]).index(r)
                    assert layouts[q][1][k] == cnt
                    rc = hip.hipMemcpy(bufs[q][1] + 8 * int(layouts[q][2][k]), bufs[r][0] + 8 * int(off), 8 * int(cnt), 3)
                    assert rc == 0

        self.exchange = exchange
        for k in range(self.models[0].setup_count()):
            for mdl in self.models:
                mdl.setup_pack(k)
            exchange()
            for mdl in self.models:
                mdl.setup_unpack(k)
        for mdl in self.models:
            mdl.setup_finish()

    def steps(self, n):
        if self.transport == "local":
            fa.group_rk4_steps(self.models, self.t, self.dt, n)
            for _ in range(n):
                self.t += self.dt
            return
        for _ in range(n):
            for i in range(4):
                for mdl in self.models:
                    mdl.stage_begin(i, self.t, self.dt)
                self.exchange()
                for mdl in self.models:
                    mdl.stage_end(i, self.t, self.dt)
            self.t += self.dt
        for cx in self.ctxs:
            cx.synchronize()

    def close(self):
        for mdl in self.models:
            mdl.close()
        for cx in self.ctxs:
            cx.close()


def monitor_maps(mdl):
    out = {q: mdl.monitor_get(q).x.array.copy() for q in ("max", "min", "mean", "rms")}
    for k in (1, 2):
        out[f"cos{k}"], out[f"sin{k}"] = mdl.monitor_get("cos", k).x.array.copy(), mdl.monitor_get("sin", k).x.array.copy()
    return out


def record_phase(grp, pts, nsteps=6, every=2):
    """set_receivers + record on every rank, nsteps steps: [(on, times, records)] per rank."""
    ons = [mdl.set_receivers(pts) for mdl in grp.models]
    for mdl in grp.models:
        mdl.record(every=every, capacity=8, which="u")
    grp.steps(nsteps)
    return [(on,) + mdl.records() for on, mdl in zip(ons, grp.models)]


def twin_phase(grp, pts, nsteps=6, every=2):
    """The same steps `every` at a time without recording: [[sample per rank] per record]."""
    for mdl in grp.models:
        mdl.set_receivers(pts)
    out = []
    for _ in range(nsteps // every):
        grp.steps(every)
        out.append([mdl.sample("u") for mdl in grp.models])
    return out


@pytest.mark.parametrize("name", list(MR_CASES))
def test_receivers_on_several_ranks(orc, name):
    transport, size, P, tdim, with_monitor = MR_CASES[name]
    pr, dt, start = mr_problem(orc, P, tdim)
    top = float(np.abs(start[0]).max())
    a, b, rows = mr_receivers(pr, size)
    last = size - 1

    # the single model's samples at the live start
    ctx = fa.Context(0)
    c, rho = tm.material(pr.mesh)
    one = fa.LinearSpectralExplicit(pr.mesh, fa.tag_box_boundary(pr.mesh), P, c, rho, tm.F0, tm.P0, tm.S0, 4, dt, V=pr.V,
                                    ctx=ctx)
    try:
        one.init()
        one.set_state(*start)
        single = {}
        for key, pts in (("a", a), ("b", b)):
            assert len(one.set_receivers(pts)) == len(pts)
            single[key] = one.sample("u")
    finally:
        one.close(), ctx.close()
    assert np.abs(single["a"]).max() > 0.1 * top and np.abs(single["b"]).max() > 0.1 * top

    grp = Group(transport, size, pr, dt, start)
    try:
        # who holds what, and each rank's sample against the single model's
        held = {}
        for key, pts in (("a", a), ("b", b)):
            ons = [mdl.set_receivers(pts) for mdl in grp.models]
            held[key] = (ons, [mdl.sample("u") for mdl in grp.models])
        for mdl in grp.models:
            if with_monitor:
                mdl.monitor(nharm=2, every=1)
        recs = {"b": record_phase(grp, b), "a": record_phase(grp, a)}
        maps = [monitor_maps(mdl) for mdl in grp.models] if with_monitor else None
        meshes = [(mdl.mesh, mdl.V) for mdl in grp.models]
    finally:
        grp.close()
    twin = Group(transport, size, pr, dt, start)
    try:
        if with_monitor:
            for mdl in twin.models:
                mdl.monitor(nharm=2, every=1)
        tw = {"b": twin_phase(twin, b), "a": twin_phase(twin, a)}
        maps_tw = [monitor_maps(mdl) for mdl in twin.models] if with_monitor else None
    finally:
        twin.close()
    plain = None
    if with_monitor:          # the same recording without the monitor
        g3 = Group(transport, size, pr, dt, start)
        try:
            plain = {"b": record_phase(g3, b), "a": record_phase(g3, a)}
        finally:
            g3.close()

    for key, pts in (("a", a), ("b", b)):
        ons, smp = held[key]
        assert np.array_equal(np.unique(np.concatenate(ons)), np.arange(len(pts))), "a point inside is held by no rank"
        for r in range(size):
            assert smp[r].shape == (len(ons[r]),)
            if len(ons[r]):
                assert np.abs(smp[r] - single[key][ons[r]]).max() < 1e-10 * top, (key, r)
    assert all(len(held["b"][0][r]) == 0 for r in range(last)) and len(held["b"][0][last]) == len(b)
    assert all(len(on) > 0 for on in held["a"][0])

    # an interface point is held by both sharers; each one's sample against the other's long-double interpolant, at
    # the budget of the own restatement (X0 is 1 on one side and 0 on the other: the bits need not match)
    ons, smp = held["a"]
    for j, idx in rows.items():
        side = {}
        for r in (j, j + 1):
            assert np.isin(idx, ons[r]).all(), f"cut {j}: rank {r} does not hold its interface points"
            mesh, V = meshes[r]
            cell, X = locate(mesh, a[idx])
            off, k = grp.offs[r], V.num_dofs
            u = start[0][off:off + k]
            side[r] = (smp[r][np.searchsorted(ons[r], idx)], rr.interp(V, u, cell, X, np.float64),
                       np.asarray(rr.interp(V, u, cell, X, np.longdouble), dtype=np.float64))
        for r, q in ((j, j + 1), (j + 1, j)):
            rr.check(f"{name} cut {j}: rank {r} against rank {q}", side[r][0], side[r][1], side[q][2],
                     {"interface": np.arange(len(idx))}, np.float64)

    # recording: every rank -- also one that holds no receiver -- has nsteps // 2 records at the loop's times, each the
    # sample of the twin group stepped that far
    t = [0.0] + times_after(0.0, dt, 12)
    for key, t0 in (("b", 0), ("a", 6)):
        for r in range(size):
            on, times, rec = recs[key][r]
            assert rec.shape == (3, len(on)), (key, r, rec.shape)
            assert np.allclose(times, [t[t0 + 2], t[t0 + 4], t[t0 + 6]], rtol=1e-12, atol=0.0), (key, r)
            for k in range(3):
                assert np.array_equal(rec[k], tw[key][k][r]), f"{key}: rank {r}, record {k} is not the twin's sample"
            if plain is not None:     # the monitor beside the recording changes no record ...
                assert np.array_equal(rec, plain[key][r][2]) and np.array_equal(times, plain[key][r][1])
        assert np.abs(recs[key][last][2]).max() > 0
    if with_monitor:                  # ... and the recording no map
        for r in range(size):
            for q in maps[r]:
                assert np.array_equal(maps[r][q], maps_tw[r][q]), (r, q)
            assert np.abs(maps[r]["rms"]).max() > 0
