"""Delays and waveform of the phased / apodised source (``model.set_source``, ``fus_model_set_source``).  Pure numpy.

A flat aperture focuses or steers by firing its elements at different times: element at ``x`` with delay ``tau(x)``
radiates ``a(x) g(t - tau(x))``.  The helpers return delays that are >= 0 with minimum 0, as the library asks.

Further down: sources anywhere in the mesh (``point_weights`` for ``model.set_source_weights``) and sampled drive signals
(``model.set_source_signals``): the interpolant restated (``signal_value``), playback of a recording (``time_reversed``)
and phase conjugation from the monitor's maps (``conjugate_delays``).
"""
from __future__ import annotations

import numpy as np


def focus_delays(x, focus, c: float):
    """Delays that make the wavefronts of all points ``x`` [n, d] arrive at ``focus`` [d] together in a medium of
    sound speed ``c``: ``(max r - r) / c`` with ``r = |x - focus|`` (the farthest point fires first)."""
    x = np.atleast_2d(np.asarray(x, dtype=np.float64))
    f = np.asarray(focus, dtype=np.float64)
    r = np.linalg.norm(x[:, :f.shape[0]] - f, axis=1)
    return (r.max() - r) / c


def steer_delays(x, direction, c: float):
    """Delays of a plane wave leaving the points ``x`` [n, d] in ``direction`` [d] (normalised here):
    ``x . n / c``, shifted so that the smallest is 0."""
    x = np.atleast_2d(np.asarray(x, dtype=np.float64))
    n = np.asarray(direction, dtype=np.float64)
    n = n / np.linalg.norm(n)
    tau = x[:, :n.shape[0]] @ n / c
    return tau - tau.min()


def waveform(t, f: float, p0: float, s0: float, amp=1.0, tau=0.0, duration: float = 0.0, scale: float = 1.0,
             derivative: bool = False):
    """The source value ``g`` (or its time derivative ``dg``) at time(s) ``t`` of an entry with amplitude ``amp`` and
    delay ``tau`` (broadcast against ``t``); mirrors csrc/source_wave.hpp.  With s = t - tau, Lr = 4 / f, w0 = 2 pi f,
    C = scale p0 w0 / s0:  g = amp C W(s) cos(w0 s), the window W rising as (1 - cos(pi f s / 4)) / 2 over (0, Lr),
    1 afterwards and, for a burst (``duration`` D >= 2 Lr), falling the same way over (D - Lr, D); 0 outside (0, D)."""
    if duration != 0.0 and not (duration >= 8.0 / f and np.isfinite(duration)):
        raise ValueError("duration is 0 (continuous) or at least two ramp lengths, 8 / f")
    s = np.asarray(t, dtype=np.float64) - np.asarray(tau, dtype=np.float64)
    w0 = 2.0 * np.pi * f
    C = scale * p0 * w0 / s0
    Lr, q = 4.0 / f, 0.25 * np.pi * f
    W, dW = np.ones_like(s), np.zeros_like(s)
    up = s < Lr
    W = np.where(up, 0.5 * (1.0 - np.cos(q * s)), W)
    dW = np.where(up, 0.5 * q * np.sin(q * s), dW)
    off = ~(s > 0.0)
    if duration > 0.0:
        down = (s > duration - Lr) & ~up
        W = np.where(down, 0.5 * (1.0 - np.cos(q * (duration - s))), W)
        dW = np.where(down, -0.5 * q * np.sin(q * (duration - s)), dW)
        off = off | (s >= duration)
    W, dW = np.where(off, 0.0, W), np.where(off, 0.0, dW)
    a = np.asarray(amp, dtype=np.float64)
    if derivative:
        return a * C * (dW * np.cos(w0 * s) - W * w0 * np.sin(w0 * s))
    return a * C * W * np.cos(w0 * s)


# ---- sources anywhere in the mesh and sampled drive signals (model.set_source_weights / set_source_signals) ----------
def _lagrange(nodes, t):
    """Values of the Lagrange basis on ``nodes`` [N] at the points ``t`` [m] -> [m, N] (product form, as the library's
    receivers evaluate it)."""
    nodes = np.asarray(nodes, dtype=np.float64)
    t = np.asarray(t, dtype=np.float64)
    out = np.ones((len(t), len(nodes)))
    for i in range(len(nodes)):
        for j in range(len(nodes)):
            if j != i:
                out[:, i] *= (t - nodes[j]) / (nodes[i] - nodes[j])
    return out


def point_weights(V, points, strengths=1.0):
    """Source weights ``w`` [ndofs] of point sources of the given ``strengths`` at ``points`` [n, tdim|3] for
    ``model.set_source_weights``: ``w_d = sum_k q_k phi_d(x_k)`` with ``phi_d`` the Lagrange basis of ``V`` on the cell
    that :func:`fenicsxfus_amd.evaluate.locate` finds for ``x_k`` -- the transpose of point evaluation, so that
    ``w . f = sum_k q_k f_h(x_k)``.  Points outside the local mesh are dropped, as the receivers drop them."""
    from .evaluate import locate

    pts = np.atleast_2d(np.asarray(points, dtype=np.float64))
    q = np.broadcast_to(np.asarray(strengths, dtype=np.float64), (len(pts),))
    cell, X = locate(V.mesh, pts)
    dm = np.asarray(V.tensor_dofmap)
    w = np.zeros(int(dm.max()) + 1)
    for k in np.flatnonzero(cell >= 0):
        b = [_lagrange(V.nodes1d, X[k:k + 1, d])[0] for d in range(X.shape[1])]
        phi = np.einsum("i,j->ij", b[0], b[1]) if len(b) == 2 else np.einsum("i,j,k->ijk", b[0], b[1], b[2])
        np.add.at(w, dm[cell[k]], q[k] * phi.ravel())
    return w


def signal_value(signals, ds: float, t_first: float, t, derivative: bool = False):
    """The cubic (Catmull-Rom) interpolant ``S_c(t)`` of the samples ``signals`` [nchan, nsamp] (or [nsamp]) taken at
    ``t_first + j * ds``, or its time derivative; mirrors csrc/source_signal.hpp.  ``t`` [m] (or a scalar) -> [nchan, m]
    (or [m], or a scalar).  Segment j = floor((t - t_first) / ds) uses the samples j-1 .. j+2, samples outside the
    table counting as 0; exactly 0 before ``t_first - ds`` and from ``t_first + nsamp * ds`` on."""
    s = np.asarray(signals, dtype=np.float64)
    s2 = np.atleast_2d(s)
    nsamp = s2.shape[1]
    tt = np.atleast_1d(np.asarray(t, dtype=np.float64))
    x = (tt - t_first) / ds
    live = (x >= -1.0) & (x < float(nsamp))
    fl = np.floor(np.where(live, x, 0.0))
    u, j = np.where(live, x, 0.0) - fl, fl.astype(np.int64)
    u2, u3 = u * u, u * u * u
    if derivative:
        w = [0.5 * (-1.0 + 4.0 * u - 3.0 * u2), 0.5 * (-10.0 * u + 9.0 * u2), 0.5 * (1.0 + 8.0 * u - 9.0 * u2),
             0.5 * (-2.0 * u + 3.0 * u2)]
    else:
        w = [0.5 * (-u + 2.0 * u2 - u3), 0.5 * (2.0 - 5.0 * u2 + 3.0 * u3), 0.5 * (u + 4.0 * u2 - 3.0 * u3),
             0.5 * (-u2 + u3)]
    pad = np.zeros((s2.shape[0], nsamp + 4))           # sample r sits at column r + 2
    pad[:, 2:nsamp + 2] = s2
    out = np.zeros((s2.shape[0], len(tt)))
    for q in range(4):
        out = out + w[q][None, :] * pad[:, np.clip(j - 1 + q + 2, 0, nsamp + 3)]
    if derivative:
        out = out / ds
    out = np.where(live[None, :], out, 0.0)
    if s.ndim == 1:
        out = out[0]
    return out[..., 0] if np.ndim(t) == 0 else out


def time_reversed(records, times):
    """Playback signals of a time-reversal mirror from a recording: ``records`` [nrec, nchan] and ``times`` [nrec]
    (uniformly spaced) as ``model.records()`` returns them -> ``(signals [nchan, nrec], ds, t_first)`` with
    ``signals[c][j] = records[nrec - 1 - j][c]`` and ``t_first = 0``: played from t = 0, channel c emits what it recorded
    last first, the sample recorded at ``times[-1] - s`` at time ``s``."""
    r = np.asarray(records, dtype=np.float64)
    tm = np.asarray(times, dtype=np.float64)
    if r.ndim != 2 or tm.shape != (r.shape[0],) or len(tm) < 2:
        raise ValueError("records [nrec, nchan] and times [nrec] with nrec >= 2 are expected")
    d = np.diff(tm)
    ds = float((tm[-1] - tm[0]) / (len(tm) - 1))
    if not (ds > 0 and np.all(np.abs(d - ds) <= 1e-6 * ds)):
        raise ValueError("the record times must ascend uniformly")
    return np.ascontiguousarray(r[::-1].T), ds, 0.0


def conjugate_delays(cos, sin, f: float):
    """Phase conjugation, the continuous-wave counterpart of time reversal: from the monitor's ``COS`` / ``SIN`` maps
    of harmonic 1 of a continuous-wave run from the target -- the field at a point is ``A cos(2 pi f t - phi)`` with
    ``A cos(phi) = cos`` and ``A sin(phi) = sin`` -- the delays ``tau = ((-phi) mod 2 pi) / (2 pi f)`` in ``[0, 1 / f)``
    with which ``cos(2 pi f (t - tau))`` has the conjugate phase ``+phi``.  Points where both maps are 0 get delay 0."""
    c, s = np.asarray(cos, dtype=np.float64), np.asarray(sin, dtype=np.float64)
    phi = np.arctan2(s, c)
    tau = np.mod(-phi, 2.0 * np.pi) / (2.0 * np.pi * f)
    return np.where(tau >= 1.0 / f, 0.0, tau)
