"""Sampled drive signals on the device (fus_model_set_source_signals, k_source_entries_signal).

Reference: the numpy RK stepper of tests/volume_source_ref.py with the interpolant ``source.signal_value`` (held against
the C++ header in test_source_signal_host.py).  Shapes: those of test_gpu_source.py -- the 4 x 3 x 3 box at p = 3 with
perturbed vertices and 4-element blocks (nine blocks; 100 entries on the source face, not a multiple of 64) and 6 x 5
quadrilaterals at p = 4; 20 RK steps.  fp64 bound: 1e-10 relative."""
import functools

import numpy as np
import pytest

import fenicsxfus_amd as fa
from fenicsxfus_amd import source as fsrc
import source_ref as sr
import volume_source_ref as vr
import test_gpu_source as tgs
from test_gpu_source import P0, S0, TOL, case, check, make_ctx, make_model
from test_gpu_volume_source import weights

pytestmark = pytest.mark.gpu

NCHAN = 7
USED = np.array([-1, 0, 1, 3, 4, 6])          # channels 2 and 5 are never used, -1 is silent


def p0_of(kind):
    return 6e6 if kind == "westervelt" else P0


def general(cs, kind, which):
    """Inputs of the general case: 7 channels of smooth random signals (a few sinusoids up to the source frequency, of
    the default waveform's size), two of them unused and about a sixth of the DOFs silent; ds = 0.37 dt; ``which``
    "positive": t_first = 3.2 dt and the run starts at 0, "negative": t_first = -2.7 dt and the run starts at -6 dt; 30
    samples, so the 20 steps start before the first sample and end after the last; amplitude and delay per DOF."""
    rng = np.random.default_rng(23)
    nsamp, ds = 30, 0.37 * cs.dt
    t_first, t0 = (3.2 * cs.dt, 0.0) if which == "positive" else (-2.7 * cs.dt, -6.0 * cs.dt)
    assert t0 < t_first - ds and t_first + nsamp * ds < t0 + sr.NSTEPS * cs.dt
    tj = t_first + ds * np.arange(nsamp)
    C = p0_of(kind) * 2 * np.pi * cs.f0 / S0
    sig = np.zeros((NCHAN, nsamp))
    for c in range(NCHAN):
        for _ in range(4):
            sig[c] += rng.uniform(0.2, 1.0) * np.sin(2 * np.pi * rng.uniform(0.1, 1.0) * cs.f0 * tj + rng.uniform(0, 6.28))
    channel = USED[rng.integers(0, len(USED), cs.pr.ndofs)].astype(np.int32)
    amp, tau = cs.aperture()
    return dict(sig=C * sig, ds=ds, t_first=t_first, t0=t0, channel=channel, amp=amp, tau=tau)


def stepper(cs, kind, forms, G, w=0.0, dtype=np.float64, nsteps=sr.NSTEPS):
    vec, _ = vr.westervelt_vectors(cs, forms) if kind == "westervelt" else cs.vectors(kind, forms)
    amp, tau = (np.asarray(a).astype(dtype).astype(np.float64) for a in (G["amp"], G["tau"]))
    g, dg = vr.sampled(G["sig"], G["ds"], G["t_first"], G["channel"], amp, tau)
    return vr.rk_stepper(cs.pr, vec, vec["src"] + np.asarray(w, dtype).astype(np.float64), g, dg, G["t0"], cs.dt, nsteps)


def set_signals(mdl, G, dtype=np.float64):
    mdl.set_source_signals(G["sig"], G["ds"], G["t_first"], G["channel"], np.asarray(G["amp"], dtype),
                           np.asarray(G["tau"], dtype))


def run(cs, kind, ctx, G, w=None, forms="cpp", dtype=np.float64):
    mdl = make_model(cs, kind, ctx, 4, forms, p0_of(kind))
    mdl.init()
    if w is not None:
        mdl.set_source_weights(np.asarray(w, dtype))
    set_signals(mdl, G, dtype)
    mdl.rk4_steps(G["t0"], cs.dt, sr.NSTEPS)
    mdl.u_sol()
    out = mdl.u_n.x.array.copy(), mdl.v_n.x.array.copy()
    mdl.close()
    return out


# ---- 1. tie to the analytic per-entry path --------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["3d", "2d"])
def test_sampled_analytic_waveform_equals_set_source(orc, name):
    """One channel per source-face DOF holding that DOF's delayed analytic waveform, sampled at ds = dt / 2 from
    t_first = t0: every RK4 stage time is a sample point, where the interpolant returns the sample, so the run equals
    the set_source run to rounding."""
    cs = case(orc, name)
    t0, _ = cs.t0s()["ramp_end"]
    amp, tau = cs.aperture()
    ds = 0.5 * cs.dt
    tj = t0 + ds * np.arange(2 * sr.NSTEPS + 3)
    sig = np.stack([fsrc.waveform(tj, cs.f0, P0, S0, amp[d], tau[d]) for d in cs.face])
    channel = np.full(cs.pr.ndofs, -1, dtype=np.int32)
    channel[cs.face] = np.arange(len(cs.face))
    ctx = make_ctx(name)
    ref = tgs.run_model(cs, "linear", ctx, t0, sr.NSTEPS, amp, tau, 0.0)
    G = dict(sig=sig, ds=ds, t_first=t0, t0=t0, channel=channel, amp=np.ones(cs.pr.ndofs), tau=np.zeros(cs.pr.ndofs))
    u, v = run(cs, "linear", ctx, G)
    ctx.close()
    check(u, v, ref, label=f"signals = sampled analytic waveform {name}")


# ---- 2. the general case against the stepper ------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["positive", "negative"])
@pytest.mark.parametrize("kind,forms", [("linear", 0), ("lossy", 0), ("lossy", 1), ("westervelt", 0)])
def test_general_vs_stepper(orc, kind, forms, which):
    """All three models (the dg term of Lossy / Westervelt plays the derivative), both forms, on the source face and at
    the volume weights of test_gpu_volume_source.py."""
    cs = case(orc, "3d")
    G, w = general(cs, kind, which), weights(cs)
    ctx = make_ctx("3d")
    u, v = run(cs, kind, ctx, G, w, forms="python" if forms else "cpp")
    ctx.close()
    check(u, v, stepper(cs, kind, forms, G, w), label=f"signals {kind} forms={forms} t_first {which}")


@pytest.mark.parametrize("blocks", [None, 8])
def test_general_2d_without_weights(orc, blocks):
    """Quadrilaterals, the tag-1 boundary alone is the emitter: one block and 8-element blocks."""
    cs = case(orc, "2d")
    G = general(cs, "linear", "positive")
    ctx = make_ctx("2d", blocks=blocks)
    u, v = run(cs, "linear", ctx, G)
    ctx.close()
    check(u, v, stepper(cs, "linear", 0, G), label=f"signals linear 2d blocks={blocks}")


# ---- 3. edge sizes -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("edge", ["nsamp=2", "nchan=1, channel=None"])
def test_edge_sizes(orc, edge):
    """The smallest table, and one channel with channel=None (channel 0 everywhere), on the 100 source-face entries of
    the 3-D case (not a multiple of the wavefront)."""
    cs = case(orc, "3d")
    assert len(cs.face) == 100
    G = general(cs, "linear", "positive")
    if edge == "nsamp=2":
        G["sig"], G["ds"] = G["sig"][:, 7:9].copy(), 4.1 * cs.dt
    else:
        G["sig"], G["channel"] = G["sig"][4:5].copy(), None
    ctx = make_ctx("3d")
    mdl = make_model(cs, "linear", ctx)
    mdl.init()
    mdl.set_source_signals(G["sig"] if edge == "nsamp=2" else G["sig"][0], G["ds"], G["t_first"], G["channel"], G["amp"],
                           G["tau"])
    mdl.rk4_steps(G["t0"], cs.dt, sr.NSTEPS)
    mdl.u_sol()
    u, v = mdl.u_n.x.array.copy(), mdl.v_n.x.array.copy()
    mdl.close()
    ctx.close()
    if G["channel"] is None:
        G["channel"] = np.zeros(cs.pr.ndofs, dtype=np.int32)
    check(u, v, stepper(cs, "linear", 0, G), label=f"signals {edge}")


# ---- 4. launch count, mode switching, errors ------------------------------------------------------------------------------
def test_launch_count(orc):
    """One launch per NEW stage time, as the analytic path: 2 per RK4 step and 1 to start, all under "source_signal"."""
    cs = case(orc, "3d")
    G = general(cs, "linear", "positive")
    ctx = make_ctx("3d")
    mdl = make_model(cs, "linear", ctx)
    mdl.init()
    set_signals(mdl, G)
    ctx.profile_enable(True)
    mdl.rk4_steps(G["t0"], cs.dt, sr.NSTEPS)
    assert ctx.profile_get("source_signal")[1] == 2 * sr.NSTEPS + 1
    assert ctx.profile_get("source")[1] == 0 and ctx.profile_get("stiffness")[1] == 4 * sr.NSTEPS
    mdl.u_sol()
    check(mdl.u_n.x.array, mdl.v_n.x.array, stepper(cs, "linear", 0, G), label="signals with profiling on")
    mdl.close()
    ctx.close()


@pytest.mark.parametrize("kind", ["linear", "lossy"])
def test_mode_switching(orc, kind):
    """Signals -> analytic -> cleared -> signals: each run has the bits of a fresh model in that mode (deterministic = 1)."""
    cs = case(orc, "3d")
    G = general(cs, kind, "positive")
    amp, tau = cs.aperture()
    ctx = make_ctx("3d", dict(deterministic=1))
    fresh = {"signals": run(cs, kind, ctx, G), "analytic": tgs.run_model(cs, kind, ctx, 0.0, sr.NSTEPS, amp, tau),
             "amplitude": tgs.run_model(cs, kind, ctx, 0.0, sr.NSTEPS, amp), "cleared": tgs.run_model(cs, kind, ctx, 0.0, sr.NSTEPS, source=False)}
    assert not np.array_equal(fresh["signals"][0], fresh["analytic"][0]) and np.abs(fresh["signals"][0]).max() > 0
    mdl = make_model(cs, kind, ctx)
    setters = {"signals": lambda: set_signals(mdl, G), "analytic": lambda: mdl.set_source(amp, tau),
               "amplitude": lambda: mdl.set_source(amplitude=amp), "cleared": mdl.clear_source}
    for mode in ("signals", "analytic", "signals", "amplitude", "signals", "cleared", "signals"):
        setters[mode]()
        mdl.init()
        mdl.rk4_steps(0.0, cs.dt, sr.NSTEPS)
        mdl.u_sol()
        assert np.array_equal(mdl.u_n.x.array, fresh[mode][0]) and np.array_equal(mdl.v_n.x.array, fresh[mode][1]), mode
    mdl.close()
    ctx.close()


def test_argument_errors(orc):
    cs = case(orc, "3d")
    nd = cs.pr.ndofs
    G = general(cs, "linear", "positive")
    on, off = cs.face[3], np.setdiff1d(np.arange(nd), cs.face)[0]
    ctx = make_ctx("3d", dict(deterministic=1))
    good = run(cs, "linear", ctx, G)
    mdl = make_model(cs, "linear", ctx)
    mdl.init()
    set_signals(mdl, G)
    sig, ds, tf, ch, amp, tau = G["sig"], G["ds"], G["t_first"], G["channel"], G["amp"], G["tau"]

    def bad(**kw):
        a = dict(signals=sig, ds=ds, t_first=tf, channel=ch, amplitude=amp, delay=tau)
        a.update(kw)
        with pytest.raises(fa.FusError, match="error -1"):
            mdl.set_source_signals(**a)
    for c in (NCHAN, NCHAN + 5, -2):
        x = ch.copy()
        x[on] = c
        bad(channel=x)
        x[on], x[off] = 0, c                      # at a DOF without a source weight: ignored
        mdl.set_source_signals(sig, ds, tf, x, amp, tau)
        set_signals(mdl, G)
    bad(signals=sig[:, :1])
    for d in (0.0, -ds, np.inf, np.nan):
        bad(ds=d)
    for t in (np.inf, np.nan):
        bad(t_first=t)
    for v in (np.nan, np.inf):
        x = sig.copy()
        x[5, 3] = v                                # (in a channel no DOF uses: refused all the same)
        bad(signals=x)
    for v in (-1e-9, np.nan, np.inf):
        for arg, a in (("amplitude", amp), ("delay", tau)):
            x = a.copy()
            x[on] = v
            bad(**{arg: x})
    with pytest.raises(fa.FusError):
        mdl.set_source_signals(sig, ds, tf, None, amp, tau)           # channel=None needs one channel
    with pytest.raises(fa.FusError):
        mdl.set_source_signals(sig, ds, tf, ch[:-1], amp, tau)
    mdl.rk4_steps(G["t0"], cs.dt, sr.NSTEPS)                          # the model is as it was
    mdl.u_sol()
    assert np.array_equal(mdl.u_n.x.array, good[0]) and np.array_equal(mdl.v_n.x.array, good[1])
    mdl.close()
    ctx.close()
    # before the setup is finished -> FUS_ERR_STATE
    ctxs = [fa.Context(0, block_elems=4) for _ in range(2)]
    fa.Context.init_local_group(ctxs)
    models = tgs.slab_models(cs, ctxs, 0)
    with pytest.raises(fa.FusError, match="error -4"):
        models[0][0].set_source_signals(np.ones(4), 1.0)
    for m, _ in models:
        m.close()
    for c in ctxs:
        c.close()


# ---- 5. variants: graph replay, fp32, two slabs ------------------------------------------------------------------------------
def test_graph_replay_matches_stepwise(orc):
    """Option "graph": 20 steps in one call (the stage time is a kernel argument that the per-step re-capture updates)
    against 20 one-step calls without it, bit for bit under deterministic = 1, and against the stepper."""
    cs = case(orc, "3d")
    G, w = general(cs, "linear", "positive"), weights(cs)
    out = {}
    for graph in (0, 1):
        ctx = make_ctx("3d", dict(deterministic=1, graph=graph))
        mdl = make_model(cs, "linear", ctx)
        mdl.init()
        mdl.set_source_weights(w)
        set_signals(mdl, G)
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
    check(*out[1], stepper(cs, "linear", 0, G, w), label="signals graph")
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])


@pytest.mark.parametrize("name", ["3d", "2d"])
def test_fp32_vs_double_stepper(orc, name):
    """Held as test_gpu_source.py holds its fp32 case: err <= 4 yard per field, yard the error of the default fp32 path
    against orc.linear_rk4 in double over the same mesh and steps (2 for the run-to-run order of the LDS sums x 2 for
    the second rounding of weight x signal)."""
    cs = case(orc, name, np.float32)
    G, w = general(cs, "linear", "positive"), weights(cs)
    ctx = make_ctx(name)
    u, v = run(cs, "linear", ctx, G, w, dtype=np.float32)
    ctx.close()
    assert u.dtype == np.float32
    ref = stepper(cs, "linear", 0, G, w, np.float32)
    yard = tgs.fp32_yard(orc, name)
    err = sr.rel(u, ref[0]), sr.rel(v, ref[1])
    print(f"signals fp32 {name}: err u {err[0]:.3e} v {err[1]:.3e}   yard u {yard[0]:.3e} v {yard[1]:.3e}")
    assert err[0] <= 4 * yard[0] and err[1] <= 4 * yard[1]


@pytest.mark.parametrize("overlap", [0, 1])
def test_two_slabs_in_process(orc, overlap):
    """Two x-slabs, the source on the y face so that the interface crosses it: every sharer passes the same channel,
    amplitude and delay for an interface DOF; both end with the same bits on the plane and with the global stepper's
    result."""
    cs = sr.Case(orc, (4, 3, 3), 3, 0.1, source_axis=1)
    G = general(cs, "linear", "positive")
    ref = stepper(cs, "linear", 0, G)
    ctxs = [fa.Context(0, block_elems=4) for _ in range(2)]
    for c in ctxs:
        c.set_option("overlap_blocks", overlap)
    fa.Context.init_local_group(ctxs)
    models = tgs.slab_models(cs, ctxs, 1)
    fa.group_finish_setup([m for m, _ in models])
    for m, off in models:
        n = m.data.ndofs
        m.init()
        m.set_source_signals(G["sig"], G["ds"], G["t_first"], G["channel"][off:off + n], G["amp"][off:off + n],
                             G["tau"][off:off + n])
    fa.group_rk4_steps([m for m, _ in models], G["t0"], cs.dt, sr.NSTEPS)
    got = []
    for m, off in models:
        n = m.data.ndofs
        m.u_sol()
        u, v = m.u_n.x.array.copy(), m.v_n.x.array.copy()
        got.append((off, u, v))
        for a, b, nm in ((u, ref[0], "u"), (v, ref[1], "v")):
            err = np.abs(a - b[off:off + n]).max() / np.abs(b).max()
            print(f"signals slabs overlap={overlap} rank off {off}: {nm} rel err vs the global stepper {err:.3e}")
            assert err < TOL
    off1 = got[1][0]
    plane = len(got[0][1]) - off1
    assert plane > 0 and np.abs(got[0][1][off1:]).max() > 0
    assert np.array_equal(got[0][1][off1:], got[1][1][:plane]) and np.array_equal(got[0][2][off1:], got[1][2][:plane])
    for m, _ in models:
        m.close()
    for c in ctxs:
        c.close()


# ---- 6. time reversal end to end --------------------------------------------------------------------------------------------
def test_time_reversal(orc):
    """The set-up of test_source_signal_host.py::test_time_reversal_guard on the device.  Run A: a point source at
    (4.2, 3.1) wavelengths (set_source_weights of point_weights; the face's own source silenced by amplitude 0) emits
    the 8-period burst, receivers at the 65 DOFs of the face x = 0 record u after each of the 992 steps.  Run B: the
    recording through source.time_reversed drives the face (one channel per DOF: the mirror layout of the table), the
    monitor keeps the max and min maps.  Asserted: along the mesh column nearest the source the maximum of the peak-|u|
    map lies within half a wavelength of the source's y and the peak at the DOF nearest the source is at least 3 x the
    column's median; the final u of run B against the stepper (driven by the same recording) within 4 x the error of
    the default path against orc.linear_rk4 over the same steps on that mesh, measured here."""
    S = vr.tr_setup(orc)
    pr = S["pr"]
    nc = pr.mesh.num_cells

    def model(ctx):
        return fa.LinearSpectralExplicit(pr.mesh, S["tags"], S["P"], np.full(nc, S["c0"]), np.full(nc, S["rho0"]), S["f0"],
                                         vr.TR_P0, S0, 4, S["dt"], V=pr.V, ctx=ctx)
    ctx = fa.Context(0)
    mdl = model(ctx)
    mdl.init()
    mdl.set_source_weights(S["w"])
    mdl.set_source(amplitude=S["amp_a"], duration=S["duration"])
    on = mdl.set_receivers(S["X"][S["face"]])
    assert len(on) == len(S["face"]) == 65
    mdl.record(1, vr.TR_STEPS)
    mdl.rk4_steps(0.0, S["dt"], vr.TR_STEPS)
    times, rec = mdl.records()
    assert rec.shape == (vr.TR_STEPS, 65) and np.abs(rec).max() > 0
    sig, ds, t_first = fsrc.time_reversed(rec, times)
    # run B on the same model: the weights go, the face plays the recording
    mdl.set_source_weights(None)
    mdl.init()
    mdl.set_source_signals(sig, ds, t_first, vr.tr_channels(S))
    mdl.record(0, 0)
    mdl.monitor(which="u")
    mdl.rk4_steps(0.0, S["dt"], vr.TR_STEPS)
    assert mdl.monitor_info()[0] == vr.TR_STEPS
    peak = np.maximum(mdl.monitor_get("max").x.array, -mdl.monitor_get("min").x.array)
    mdl.u_sol()
    u_b = mdl.u_n.x.array.copy()
    # the default path over the same steps: the yardstick
    mdl.monitor_off()
    mdl.clear_source()
    mdl.init()
    mdl.rk4_steps(0.0, S["dt"], vr.TR_STEPS)
    mdl.u_sol()
    u_plain = mdl.u_n.x.array.copy()
    mdl.close()
    ctx.close()
    dist, ratio = vr.tr_conditions(S, peak)
    print(f"time reversal (gpu): |y_max - y_src| = {dist:.3f} wavelengths, peak / column median = {ratio:.2f}")
    assert dist <= 0.5
    assert ratio >= 3.0
    _, u_ref = vr.tr_playback(orc, sig, ds, t_first)
    V = S["vec"]
    u_def, v_def = np.zeros(pr.ndofs), np.zeros(pr.ndofs)
    orc.linear_rk4(2, pr.N, pr.dm, pr.G, pr.D, V["lin"], V["m"], V["src"], V["absb"], S["f0"], vr.TR_P0, S0, 0.0, 0.0, S["dt"],
                   u_def, v_def, steps=vr.TR_STEPS)
    yard, err = sr.rel(u_plain, u_def), sr.rel(u_b, u_ref)
    print(f"time reversal (gpu): final u err {err:.3e}, default path vs oracle {yard:.3e}")
    assert err <= 4 * yard
