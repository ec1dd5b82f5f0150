"""Source weights at any DOF on the device (fus_model_set_source_weights).

Reference: the numpy RK stepper of tests/volume_source_ref.py (pinned against tests/source_ref.py's in
test_source_signal_host.py), whose source weights are the facet weights plus the caller's.  Shapes: those of
test_gpu_source.py -- the 4 x 3 x 3 box at p = 3 with perturbed vertices and 4-element blocks (nine blocks) and 6 x 5
quadrilaterals at p = 4 in one block and in 8-element blocks; 20 RK steps from rest.  The weights (``weights``) are
non-zero at a cell-interior DOF off the boundary (block-interior), at interior mesh vertices (in 3-D a vertex's eight
cells cannot lie in one 4-element block, in 2-D one of the interior vertices lies on a block's border: rank-local shared
DOFs), at a DOF of the absorbing boundary, at a DOF of the source face (where they add to the facet weight), over all
DOFs of two neighbouring cells (a smooth blob: dense entries), and negative at some of them.
fp64 bound: 1e-10 relative, the project's bound for 20 steps."""
import functools
import os
import subprocess

import numpy as np
import pytest

import fenicsxfus_amd as fa
from fenicsxfus_amd import source as fsrc
import source_ref as sr
import volume_source_ref as vr
import test_gpu_source as tgs
from test_gpu_source import P0, S0, TOL, case, check, make_ctx, make_model

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def weights(cs, variant=0):
    """The weight vector described above, scaled to the facet weights of the case; ``variant`` 1: another set."""
    pr = cs.pr
    dm = np.asarray(pr.dm)
    nd, t = pr.ndofs, cs.tdim
    mult = np.bincount(dm.ravel(), minlength=nd)
    vec, _ = cs.vectors("lossy", 0)                 # absb of the C++ lossy forms: non-zero on every boundary DOF
    bnd = vec["absb"] != 0
    lin, _ = cs.vectors("linear")
    scale = lin["src"].max()
    rng = np.random.default_rng(17 + variant)
    w = np.zeros(nd)
    bubble = np.flatnonzero((mult == 1) & ~bnd)                          # cell-interior DOFs
    vertex = np.flatnonzero((mult == 2**t) & ~bnd)                       # interior mesh vertices
    absorbing = np.flatnonzero((lin["absb"] != 0) & (lin["src"] == 0) & (mult == 1))
    assert len(bubble) and len(vertex) and len(absorbing)
    w[bubble[len(bubble) // 3 + variant]] = 0.8 * scale
    w[vertex] = scale * rng.uniform(0.3, 1.0, len(vertex)) * np.where(np.arange(len(vertex)) % 3 == 1, -1.0, 1.0)
    w[absorbing[len(absorbing) // 2 + variant]] = -0.6 * scale
    w[cs.face[3 + variant]] += 0.5 * scale
    cells = (dm.shape[0] // 2, dm.shape[0] // 2 + 1)                     # x-neighbours in the box's cell order
    assert len(np.intersect1d(dm[cells[0]], dm[cells[1]])) > 0
    blob = np.union1d(dm[cells[0]], dm[cells[1]])
    xc = cs.X[blob].mean(axis=0)
    r2 = ((cs.X[blob] - xc) ** 2).sum(axis=1)
    w[blob] += 0.4 * scale * np.exp(-r2 / (0.5 * r2.max()))
    return w


@functools.lru_cache(maxsize=None)
def reference(orc, name, kind, forms, source, order=4, variant=0, dtype=np.float64):
    """The stepper's (u, v) after 20 steps: ``source`` "default" (the model's own waveform from t = 0), "aperture" (the
    per-DOF amplitude and delay of the case, from t = 0) or "none" (the same without the caller's weights)."""
    cs = case(orc, name, dtype)
    vec, scale = vr.westervelt_vectors(cs, forms) if kind == "westervelt" else cs.vectors(kind, forms)
    p0 = 6e6 if kind == "westervelt" else P0
    amp, tau = (a.astype(dtype).astype(np.float64) for a in cs.aperture()) if source == "aperture" else (1.0, 0.0)
    w = 0.0 if source == "none" else weights(cs, variant).astype(dtype).astype(np.float64)
    g, dg = vr.analytic(cs.f0, p0, scale, amp, tau)
    return vr.rk_stepper(cs.pr, vec, vec["src"] + w, g, dg, 0.0, cs.dt, sr.NSTEPS, order)


def run(cs, kind, ctx, w, source="default", rk_order=4, forms="cpp", nsteps=sr.NSTEPS):
    p0 = 6e6 if kind == "westervelt" else P0
    mdl = make_model(cs, kind, ctx, rk_order, forms, p0)
    mdl.init()
    mdl.set_source_weights(w)
    if source == "aperture":
        mdl.set_source(*cs.aperture())
    mdl.rk4_steps(0.0, cs.dt, nsteps)
    mdl.u_sol()
    out = mdl.u_n.x.array.copy(), mdl.v_n.x.array.copy()
    mdl.close()
    return out


# ---- 1. every model against the stepper, default waveform and per-DOF amplitude / delay ----------------------------------
@pytest.mark.parametrize("source", ["default", "aperture"])
@pytest.mark.parametrize("kind,forms", [("linear", 0), ("lossy", 0), ("lossy", 1), ("westervelt", 0)])
def test_models_vs_stepper(orc, kind, forms, source):
    cs = case(orc, "3d")
    ctx = make_ctx("3d")
    u, v = run(cs, kind, ctx, weights(cs), source, forms="python" if forms else "cpp")
    ctx.close()
    ref = reference(orc, "3d", kind, forms, source)
    check(u, v, ref, label=f"volume {kind} forms={forms} {source}")
    # the weights are not spectators of the comparison
    plain = reference(orc, "3d", kind, forms, "none") if source == "default" else None
    assert plain is None or sr.rel(plain[0], ref[0]) > 1e-3


@pytest.mark.parametrize("blocks", [None, 8])
@pytest.mark.parametrize("source", ["default", "aperture"])
def test_linear_2d(orc, source, blocks):
    """Quadrilaterals: one block (every entry block-interior) and 8-element blocks (both ranges)."""
    cs = case(orc, "2d")
    ctx = make_ctx("2d", blocks=blocks)
    if blocks:
        mdl = make_model(cs, "linear", ctx)
        info = mdl.data.info()
        mdl.close()
        assert info["nblocks"] > 1 and info["shared_dofs"] > 0
    u, v = run(cs, "linear", ctx, weights(cs), source)
    ctx.close()
    check(u, v, reference(orc, "2d", "linear", 0, source), label=f"volume linear 2d blocks={blocks} {source}")


# ---- 2. RK orders 1-3 (k_boundary_partial runs every stage) and the options that change who reads the weights ---------
@pytest.mark.parametrize("order", [1, 2, 3])
def test_rk_orders(orc, order):
    cs = case(orc, "3d")
    ctx = make_ctx("3d")
    u, v = run(cs, "linear", ctx, weights(cs), "aperture", rk_order=order)
    ctx.close()
    check(u, v, reference(orc, "3d", "linear", 0, "aperture", order), label=f"volume linear rk_order={order}")


@pytest.mark.parametrize("opts", [dict(planes=0), dict(deterministic=1), dict(lean_rk4=0)], ids=lambda o: next(iter(o)))
@pytest.mark.parametrize("name", ["3d", "2d"])
def test_options(orc, name, opts):
    cs = case(orc, name)
    ctx = make_ctx(name, opts, blocks=8 if name == "2d" else None)
    u, v = run(cs, "linear", ctx, weights(cs), "aperture")
    ctx.close()
    check(u, v, reference(orc, name, "linear", 0, "aperture"), label=f"volume linear {name} {opts}")


@pytest.mark.parametrize("source", ["default", "aperture"])
def test_graph_replay_matches_stepwise(orc, source):
    """Option "graph": 20 steps in one call against 20 one-step calls without it, bit for bit under deterministic = 1
    (the criterion of test_gpu_source.py), and against the stepper."""
    cs = case(orc, "3d")
    out = {}
    for graph in (0, 1):
        ctx = make_ctx("3d", dict(deterministic=1, graph=graph))
        mdl = make_model(cs, "linear", ctx)
        mdl.init()
        mdl.set_source_weights(weights(cs))
        if source == "aperture":
            mdl.set_source(*cs.aperture())
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
    check(*out[1], reference(orc, "3d", "linear", 0, source), label=f"volume linear graph {source}")
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])


# ---- 3. replacement, removal, errors ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["linear", "lossy"])
def test_replace_and_remove(orc, kind):
    """NULL restores the bits of a fresh model; W1 then W2 gives the bits of a fresh model with W2; the state, and a
    step taken in between, do not matter (deterministic = 1: the runs are compared bit for bit)."""
    cs = case(orc, "3d")
    w1, w2 = weights(cs, 0), weights(cs, 1)
    assert not np.array_equal(w1, w2)
    ctx = make_ctx("3d", dict(deterministic=1))
    fresh = tgs.run_model(cs, kind, ctx, 0.0, sr.NSTEPS, source=False)
    fresh_w2 = run(cs, kind, ctx, w2)
    assert not np.array_equal(fresh[0], fresh_w2[0])
    mdl = make_model(cs, kind, ctx)
    mdl.init()
    mdl.set_source_weights(w1)
    mdl.set_source(*cs.aperture())                      # ... and the per-entry arrays of the old list go with it
    mdl.rk4_steps(0.0, cs.dt, 3)
    mdl.set_source_weights(w2)
    mdl.init()
    mdl.rk4_steps(0.0, cs.dt, sr.NSTEPS)
    mdl.u_sol()
    assert np.array_equal(mdl.u_n.x.array, fresh_w2[0]) and np.array_equal(mdl.v_n.x.array, fresh_w2[1])
    mdl.set_source_weights(None)
    mdl.init()
    mdl.rk4_steps(0.0, cs.dt, sr.NSTEPS)
    mdl.u_sol()
    assert np.array_equal(mdl.u_n.x.array, fresh[0]) and np.array_equal(mdl.v_n.x.array, fresh[1])
    assert np.abs(fresh[0]).max() > 0
    mdl.close()
    ctx.close()


def test_state_receivers_and_monitor_are_kept(orc):
    """The call between steps keeps u and v, the receivers and the monitor's window."""
    cs = case(orc, "3d")
    ctx = make_ctx("3d")
    mdl = make_model(cs, "linear", ctx)
    mdl.init()
    on = mdl.set_receivers(cs.X[cs.face[:5]] + 1e-4)
    mdl.monitor(which="u")
    mdl.rk4_steps(0.0, cs.dt, 5)
    mdl.u_sol()
    u5, v5, s5 = mdl.u_n.x.array.copy(), mdl.v_n.x.array.copy(), mdl.sample()
    mdl.set_source_weights(weights(cs))
    mdl.u_sol()
    assert np.array_equal(mdl.u_n.x.array, u5) and np.array_equal(mdl.v_n.x.array, v5) and np.abs(u5).max() > 0
    assert len(on) == 5 and np.array_equal(mdl.sample(), s5)
    mdl.rk4_steps(5 * cs.dt, cs.dt, 2)
    assert mdl.monitor_info()[0] == 7
    mdl.close()
    ctx.close()


def test_errors(orc):
    cs = case(orc, "3d")
    nd = cs.pr.ndofs
    w = weights(cs)
    ctx = make_ctx("3d", dict(deterministic=1))
    good = run(cs, "linear", ctx, w)
    mdl = make_model(cs, "linear", ctx)
    mdl.init()
    mdl.set_source_weights(w)
    for bad in (np.nan, np.inf, -np.inf):
        x = w.copy()
        x[nd // 2] = bad
        with pytest.raises(fa.FusError, match="error -1"):
            mdl.set_source_weights(x)
    with pytest.raises(fa.FusError):
        mdl.set_source_weights(w[:-1])
    mdl.rk4_steps(0.0, cs.dt, sr.NSTEPS)                 # the model is as it was: the run with w
    mdl.u_sol()
    assert np.array_equal(mdl.u_n.x.array, good[0]) and np.array_equal(mdl.v_n.x.array, good[1])
    mdl.close()
    ctx.close()
    # before the setup is finished (in-process group, fus_group_finish_setup has not run) -> FUS_ERR_STATE
    ctxs = [fa.Context(0, block_elems=4) for _ in range(2)]
    fa.Context.init_local_group(ctxs)
    models = tgs.slab_models(cs, ctxs, 0)
    with pytest.raises(fa.FusError, match="error -4"):
        models[0][0].set_source_weights(np.zeros(models[0][0].data.ndofs))
    fa.group_finish_setup([m for m, _ in models])
    models[0][0].set_source_weights(np.zeros(models[0][0].data.ndofs))
    for m, _ in models:
        m.close()
    for c in ctxs:
        c.close()


# ---- 4. fp32 ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["3d", "2d"])
def test_fp32_vs_double_stepper(orc, name):
    """Held as test_gpu_source.py holds its fp32 case: err <= 4 yard per field, yard the error of the default fp32 path
    against orc.linear_rk4 in double over the same mesh and steps."""
    cs = case(orc, name, np.float32)
    ctx = make_ctx(name)
    u, v = run(cs, "linear", ctx, weights(cs).astype(np.float32), "aperture")
    ctx.close()
    assert u.dtype == np.float32
    ref = reference(orc, name, "linear", 0, "aperture", 4, 0, np.float32)
    yard = tgs.fp32_yard(orc, name)
    err = sr.rel(u, ref[0]), sr.rel(v, ref[1])
    print(f"volume fp32 {name}: err u {err[0]:.3e} v {err[1]:.3e}   yard u {yard[0]:.3e} v {yard[1]:.3e}")
    assert err[0] <= 4 * yard[0] and err[1] <= 4 * yard[1]


# ---- 5. two x-slabs in one process: a point source in a rank-0 cell that touches the interface -------------------------
@pytest.mark.parametrize("overlap", [0, 1])
def test_two_slabs_in_process(orc, overlap):
    """The interface DOFs carry weight on rank 0 only (the rank whose cell was located); both sharers end with the same
    bits on the plane, and the result is the global stepper's."""
    cs = case(orc, "3d")
    lin, _ = cs.vectors("linear")
    q = 40.0 * lin["src"].max()
    ctxs = [fa.Context(0, block_elems=4) for _ in range(2)]
    for c in ctxs:
        c.set_option("overlap_blocks", overlap)
    fa.Context.init_local_group(ctxs)
    models = tgs.slab_models(cs, ctxs, 0)
    fa.group_finish_setup([m for m, _ in models])
    off1 = models[1][1]
    plane = models[0][0].data.ndofs - off1
    assert plane > 0
    # the centre of the rank-0 cell nearest the interface plane, moved towards the plane (still inside the cell)
    Xp = cs.X[off1:off1 + plane].mean(axis=0)
    cen = cs.pr.mesh.cell_centroids()[:, :3]
    left = np.flatnonzero(cen[:, 0] < Xp[0])
    c0 = left[np.argmin(np.linalg.norm(cen[left] - Xp, axis=1))]
    pt = cen[c0] + np.array([0.25 * (Xp[0] - cen[c0, 0]), 0.0, 0.0])
    w_glob = fsrc.point_weights(cs.pr.V, pt[None, :], q)
    assert np.abs(w_glob[off1:off1 + plane]).max() > 0 and not w_glob[off1 + plane:].any()
    shares = [fsrc.point_weights(m.V, pt[None, :], q) for m, _ in models]
    assert not shares[1].any() and np.abs(shares[0] - w_glob[:len(shares[0])]).max() <= 1e-9 * q
    vec, scale = cs.vectors("linear")
    g, dg = vr.analytic(cs.f0, P0, scale)
    ref = vr.rk_stepper(cs.pr, vec, vec["src"] + w_glob, g, dg, 0.0, cs.dt, sr.NSTEPS)
    plain = reference(orc, "3d", "linear", 0, "none")
    assert sr.rel(plain[0], ref[0]) > 1e-3
    for (m, _), w in zip(models, shares):
        m.init()
        m.set_source_weights(w)
    fa.group_rk4_steps([m for m, _ in models], 0.0, cs.dt, sr.NSTEPS)
    got = []
    for m, off in models:
        n = m.data.ndofs
        m.u_sol()
        u, v = m.u_n.x.array.copy(), m.v_n.x.array.copy()
        got.append((u, v))
        for a, b, nm in ((u, ref[0], "u"), (v, ref[1], "v")):
            err = np.abs(a - b[off:off + n]).max() / np.abs(b).max()
            print(f"volume slabs overlap={overlap} rank off {off}: {nm} rel err vs the global stepper {err:.3e}")
            assert err < TOL
    assert np.abs(got[0][0][off1:]).max() > 0
    assert np.array_equal(got[0][0][off1:], got[1][0][:plane]) and np.array_equal(got[0][1][off1:], got[1][1][:plane])
    for m, _ in models:
        m.close()
    for c in ctxs:
        c.close()


# ---- 6. the C++ example -------------------------------------------------------------------------------------------------------
def test_cpp_example(orc, tmp_path):
    """examples/cpp_source_signal.cpp, built as test_cpp_host.py builds its example: a point source in a small box
    driven by a sampled Gaussian pulse, against the stepper with the same weights and samples."""
    from fenicsxfus_amd.evaluate import locate

    cs = case(orc, "3d")
    pr, m = cs.pr, cs.pr.mesh
    libdir = os.path.join(ROOT, "fenicsx-fus_amd", "fenicsxfus_amd")
    exe = tmp_path / "cpp_source_signal"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "cpp_source_signal.cpp"), "-L", libdir, "-lfusmi",
                           f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)])
    pt = np.array([0.55, 0.45, 0.6]) * np.array(cs.hi)
    cell, X = locate(m, pt[None, :])
    assert cell[0] >= 0
    nsamp, ds, t_first = 37, 0.7 * cs.dt, -2.0 * cs.dt
    centre, width, q = 8.0 * cs.dt, 2.5 * cs.dt, 3.0e4
    with open(tmp_path / "in.bin", "wb") as f:
        np.array([3, pr.P, m.num_cells, pr.ndofs, m.geometry.x.shape[0], len(cs.tags.cells), sr.NSTEPS, nsamp, cell[0]],
                 dtype=np.int64).tofile(f)
        np.array([cs.dt, ds, t_first, centre, width, q, *X[0]], dtype=np.float64).tofile(f)
        pr.dm.astype(np.int32).tofile(f)
        np.asarray(pr.nodes, dtype=np.float64).tofile(f)
        np.ascontiguousarray(m.geometry.x, dtype=np.float64).tofile(f)
        np.ascontiguousarray(m.geometry.dofmap, dtype=np.int32).tofile(f)
        for a in (cs.tags.cells, cs.tags.local_facets, cs.tags.values):
            np.ascontiguousarray(a, dtype=np.int32).tofile(f)
        for a in (cs.c, cs.rho):
            np.ascontiguousarray(a, dtype=np.float64).tofile(f)
    out = subprocess.run([str(exe), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    raw = np.fromfile(tmp_path / "out.bin", dtype=np.float64)
    u, v = raw[:pr.ndofs], raw[pr.ndofs:]
    pulse = np.exp(-0.5 * ((t_first + ds * np.arange(nsamp) - centre) / width) ** 2)
    vec, _ = cs.vectors("linear")
    w = vec["src"] + fsrc.point_weights(pr.V, pt[None, :], q)
    g, dg = vr.sampled(pulse, ds, t_first, np.where(w != 0, 0, -1))
    ref = vr.rk_stepper(pr, vec, w, g, dg, 0.0, cs.dt, sr.NSTEPS)
    check(u, v, ref, label="cpp_source_signal")
    assert abs(float(out.stdout.split()[-1]) - np.abs(u).max()) <= 1e-15 * np.abs(u).max()
