"""Reference of the tests of sources anywhere in the mesh and of sampled drive signals (test_source_signal_host.py,
test_gpu_volume_source.py, test_gpu_source_signal.py).

``rk_stepper`` is tests/source_ref.py's numpy Runge-Kutta loop with a general source term: the right-hand side gains
``w * g(t)`` (and, where the model has a dg term, ``w2 * dg(t)``) with ``w`` a weight per DOF and ``g`` / ``dg`` callables
``t -> [ndofs]`` (or a scalar).  Same formulas, same order of operations:
    Linear      f1 = (K(lin) u + w g(t) - absb v) / m
    Lossy       f1 = (K(lin) u + K(att) v + w g(t) + w2 dg(t) - absb v) / m
    Westervelt  f1 = (the Lossy numerator - mn1 v^2) / (m + mn1 u)
``w = vec["src"] + volume weights`` and ``w2 = vec["src2"]``: the dg term keeps the facet part only (fusmi.h).
test_source_signal_host.py pins it against source_ref.rk_stepper with the facet weights and the analytic waveform."""
import functools

import numpy as np

import fenicsxfus_amd as fa
from fenicsxfus_amd import source as fsrc
from util import Problem
from source_ref import RK, S0, Case, NSTEPS, rel   # noqa: F401  (the cases are source_ref's)


def rk_stepper(pr, vec, w, g, dg, t0, dt, nsteps, order=4, u=None, v=None, on_step=None):
    """``nsteps`` explicit RK steps of size dt from (u, v) (default: rest) at t0; returns (u, v).  float64 throughout.
    ``w`` [ndofs]: the source weights (facet + volume); ``g(t)``, ``dg(t)``: the source function and its derivative per
    DOF; ``on_step(s, u, v)`` is called after step s = 1..nsteps."""
    a_r, b_r, c_r = RK[order]
    nd = pr.ndofs
    u0 = np.zeros(nd) if u is None else np.array(u, dtype=np.float64)
    v0 = np.zeros(nd) if v is None else np.array(v, dtype=np.float64)
    w = np.asarray(w, dtype=np.float64)
    absb, m = (np.asarray(vec[k], dtype=np.float64) for k in ("absb", "m"))
    src2, mn1 = vec.get("src2"), vec.get("mn1")
    t = t0
    for step in range(nsteps):
        ua, va = u0.copy(), v0.copy()
        ku, kv = np.zeros(nd), np.zeros(nd)
        for i in range(order):
            un, vn = u0 + dt * a_r[i] * ku, v0 + dt * a_r[i] * kv
            tn = t + c_r[i] * dt
            b = pr.K(un, vec["lin"]) + w * g(tn) - absb * vn
            if src2 is not None:
                b = b + pr.K(vn, vec["att"]) + src2 * dg(tn)
            ku, kv = vn, (b / m if mn1 is None else (b - mn1 * vn * vn) / (m + mn1 * un))
            ua, va = ua + dt * b_r[i] * ku, va + dt * b_r[i] * kv
        u0, v0 = ua, va
        t += dt
        if on_step is not None:
            on_step(step + 1, u0, v0)
    return u0, v0


def analytic(f0, p0, scale, amp=1.0, tau=0.0, duration=0.0):
    """(g, dg) of the library's analytic waveform (source.waveform) as callables of the stage time."""
    return (lambda t: fsrc.waveform(t, f0, p0, S0, amp, tau, duration, scale),
            lambda t: fsrc.waveform(t, f0, p0, S0, amp, tau, duration, scale, derivative=True))


def sampled(signals, ds, t_first, channel, amp=1.0, tau=0.0):
    """(g, dg) of sampled drive signals: DOF d plays ``amp[d] * S_channel[d](t - tau[d])``, silent where channel < 0."""
    sig = np.atleast_2d(np.asarray(signals, dtype=np.float64))
    ch = np.asarray(channel)
    live = ch >= 0
    a = np.broadcast_to(np.asarray(amp, dtype=np.float64), ch.shape)
    ta = np.broadcast_to(np.asarray(tau, dtype=np.float64), ch.shape)

    def make(derivative):
        def f(t):
            out = np.zeros(len(ch))
            if live.any() and np.all(ta[live] == ta[live][0]):      # one local time: every channel in one call
                out[live] = a[live] * fsrc.signal_value(sig, ds, t_first, t - ta[live][0], derivative=derivative)[ch[live]]
                return out
            for c in np.unique(ch[live]):
                sel = ch == c
                out[sel] = a[sel] * fsrc.signal_value(sig[c], ds, t_first, t - ta[sel], derivative=derivative)
            return out
        return f
    return make(False), make(True)


def westervelt_vectors(cs, forms):
    """cs.vectors("lossy", forms) with the diagonal of the nonlinear mass term added (Westervelt.hpp:185, 249-254)."""
    vec, scale = cs.vectors("lossy", forms)
    vec = dict(vec)
    vec["mn1"] = cs.pr.M(np.ones(cs.pr.ndofs), -2.0 * cs.beta / (cs.rho**2 * cs.c**4))
    return vec, scale


# ---- time reversal: a point source inside the medium, recorded on the face x = 0 and played back ---------------------
# 16 x 16 quadrilaterals at p = 4 over a box of 8 x 8 wavelengths (two cells per wavelength), 64 steps per period (the
# CFL dt of the focusing test), homogeneous water.  Run A: a point source at (4.2, 3.1) wavelengths -- not a node --
# emits the library's 8-period burst while the face x = 0 (tag 1, its own source silenced) records u after every one
# of the 992 steps.  Run B: the recording, reversed in time, drives the face for 992 steps.
TR_LAMBDAS, TR_STEPS, TR_SPP, TR_P0 = 8, 992, 64, 6e4
TR_POINT = (4.2, 3.1)          # in wavelengths


@functools.lru_cache(maxsize=None)
def tr_setup(orc):
    P, c0, rho0, h = 4, 1500.0, 1000.0, 0.0015
    lam = 2 * h
    f0 = c0 / lam
    pr = Problem(orc, (2 * TR_LAMBDAS,) * 2, P, hi=[TR_LAMBDAS * lam] * 2)
    tags = fa.tag_box_boundary(pr.mesh)
    X = pr.V.tabulate_dof_coordinates()[:, :2]
    m, src, absb, lin = pr.linear_model_vectors(c0, rho0, tags)
    face = np.flatnonzero(src)
    face = face[np.argsort(X[face, 1])]
    x0 = np.array(TR_POINT) * lam
    w = fsrc.point_weights(pr.V, x0[None, :])
    xs = np.unique(X[:, 0])
    xcol = xs[np.argmin(np.abs(xs - x0[0]))]
    col = np.flatnonzero(X[:, 0] == xcol)
    col = col[np.argsort(X[col, 1])]
    amp_a = np.ones(pr.ndofs)
    amp_a[face] = 0.0                                  # run A: the face listens, only the point source emits
    return dict(pr=pr, tags=tags, X=X, f0=f0, dt=1.0 / (TR_SPP * f0), lam=lam, c0=c0, rho0=rho0, P=P, face=face, w=w,
                x0=x0, col=col, inear=int(np.argmin(np.linalg.norm(X - x0, axis=1))), amp_a=amp_a,
                duration=8.0 / f0, vec=dict(m=m, src=src, absb=absb, lin=lin))


def tr_forward(orc):
    """Run A on the numpy stepper: (times [992], records [992, 65] of u on the face)."""
    S = tr_setup(orc)
    rec = np.zeros((TR_STEPS, len(S["face"])))

    def on_step(s, u, v):
        rec[s - 1] = u[S["face"]]
    g, dg = analytic(S["f0"], TR_P0, 1.0, S["amp_a"], 0.0, S["duration"])
    rk_stepper(S["pr"], S["vec"], S["vec"]["src"] + S["w"], g, dg, 0.0, S["dt"], TR_STEPS, on_step=on_step)
    return S["dt"] * np.arange(1, TR_STEPS + 1), rec


def tr_channels(S):
    ch = np.full(S["pr"].ndofs, -1, dtype=np.int32)
    ch[S["face"]] = np.arange(len(S["face"]), dtype=np.int32)
    return ch


def tr_playback(orc, signals, ds, t_first):
    """Run B on the numpy stepper: (peak |u| over the steps per DOF, final u)."""
    S = tr_setup(orc)
    peak = np.zeros(S["pr"].ndofs)

    def on_step(s, u, v):
        np.maximum(peak, np.abs(u), out=peak)
    g, dg = sampled(signals, ds, t_first, tr_channels(S))
    u, _ = rk_stepper(S["pr"], S["vec"], S["vec"]["src"], g, dg, 0.0, S["dt"], TR_STEPS, on_step=on_step)
    return peak, u


def tr_conditions(S, peak):
    """(distance in wavelengths between the source's y and the maximum of the peak map along the mesh column nearest
    the source, peak at the DOF nearest the source over the column's median)."""
    col = S["col"]
    ymax = S["X"][col[np.argmax(peak[col])], 1]
    return abs(ymax - S["x0"][1]) / S["lam"], peak[S["inear"]] / np.median(peak[col])
