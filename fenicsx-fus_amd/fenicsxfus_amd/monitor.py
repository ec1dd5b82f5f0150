"""Host-side helpers for the field monitor (``model.monitor`` / ``monitor_get``, fusmi.h): amplitude and phase of a
harmonic from its cosine / sine maps, the signal the maps stand for, and the step size / window that makes the
harmonic sums exact -- a whole number of steps per source period and a window of whole periods.  numpy only."""
from __future__ import annotations

import math

import numpy as np


def _arr(a):
    return np.asarray(getattr(getattr(a, "x", None), "array", a), dtype=np.float64)


def amplitude(cos, sin):
    """|harmonic| per DOF: sqrt(COS_k^2 + SIN_k^2)."""
    return np.hypot(_arr(cos), _arr(sin))


def phase(cos, sin):
    """phi per DOF with COS_k cos(wt) + SIN_k sin(wt) = amplitude * cos(wt - phi), in (-pi, pi]."""
    return np.arctan2(_arr(sin), _arr(cos))


def reconstruct(mean, cos_list, sin_list, freq, t):
    """MEAN + sum_k COS_k cos(2 pi k f t) + SIN_k sin(2 pi k f t) at the time(s) ``t``: shape t.shape + mean.shape."""
    mean = _arr(mean)
    t = np.asarray(t, dtype=np.float64)
    tt = t.reshape(t.shape + (1,) * mean.ndim)
    out = np.broadcast_to(mean, t.shape + mean.shape).copy()
    for k, (c, s) in enumerate(zip(cos_list, sin_list), start=1):
        out += _arr(c) * np.cos(2 * np.pi * k * freq * tt) + _arr(s) * np.sin(2 * np.pi * k * freq * tt)
    return out


def whole_period_window(freq, dt_max, t_end, nperiods, every=1, nharm=0):
    """(dt, nsteps, skip, steps_per_period) for a run to about ``t_end`` whose last ``nperiods`` source periods are
    monitored: dt = T / ceil(T / dt_max) with T = 1 / freq, so a period is a whole number of steps;
    nsteps = ceil(t_end / dt); skip = nsteps - nperiods * steps_per_period, to be passed to ``model.monitor``.
    Both quotients are rounded up with a relative slack of 1e-14, so that a ``dt_max`` that divides the period (or
    the run) exactly but for its last bit, such as T / 8 computed in floating point, gives 8 steps and not 9: dt may
    exceed ``dt_max`` by that much, 1e-14 relative, far below any stability margin.
    Raises when the samples per period, steps_per_period / every, do not exceed 2 * nharm (aliasing), when the window
    does not fit into the run, or when ``every`` does not divide steps_per_period.  The last is a deliberate
    restriction, stricter than needed (uniform sampling over the window only asks that ``every`` divide
    nperiods * steps_per_period): it makes every period of the window carry the same sample phases, so that any
    whole number of periods of it is a valid window too."""
    if not (freq > 0 and dt_max > 0 and nperiods >= 1 and every >= 1 and nharm >= 0):
        raise ValueError("freq, dt_max > 0, nperiods >= 1, every >= 1, nharm >= 0")
    T = 1.0 / freq
    spp = int(math.ceil(T / dt_max * (1 - 1e-14)))
    if spp / every <= 2 * nharm:
        raise ValueError(f"{spp / every:g} samples per period do not resolve harmonic {nharm}: more than {2 * nharm} needed")
    if spp % every:
        raise ValueError(f"every = {every} does not divide the {spp} steps of a period: the samples would not be uniform "
                         "over whole periods")
    dt = T / spp
    nsteps = int(math.ceil(t_end / dt * (1 - 1e-14)))
    skip = nsteps - nperiods * spp
    if skip < 0:
        raise ValueError(f"{nperiods} periods ({nperiods * spp} steps) do not fit into the {nsteps} steps to t_end")
    return dt, nsteps, skip, spp
