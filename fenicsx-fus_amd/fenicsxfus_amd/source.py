"""Delays and waveform of the phased / apodised source (``model.set_source``, ``fus_model_set_source``).  Pure numpy.

A flat aperture focuses or steers by firing its elements at different times: element at ``x`` with delay ``tau(x)``
radiates ``a(x) g(t - tau(x))``.  The helpers return delays that are >= 0 with minimum 0, as the library asks.
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
