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


def power_law(alpha, y, nharm):
    """Absorption of the harmonics ``1..nharm`` under the power law ``alpha(f) ~ f^y``: an array of shape
    ``(nharm, ncells)`` whose row ``k - 1`` is ``alpha * k**y``.  ``alpha``: amplitude absorption in Np/m at the source
    frequency, one value per cell (or a scalar: one column); ``y``: a scalar or one value per cell (about 1 to 1.3 in
    soft tissue, 2 in water and thermoviscous media).  What ``BioheatSpectralExplicit.set_heat_from`` takes as a 2-D
    ``absorption``."""
    if int(nharm) < 1:
        raise ValueError("nharm >= 1")
    alpha, y = np.atleast_1d(_arr(alpha)), _arr(y)
    k = np.arange(1, int(nharm) + 1, dtype=np.float64)[:, None]
    return alpha[None, :] * k ** np.broadcast_to(y, alpha.shape)[None, :]


def thermoviscous_absorption(delta, c, f):
    """``delta (2 pi f)^2 / (2 c^3)``: the amplitude absorption in Np/m at the frequency ``f`` that the Lossy and
    Westervelt models themselves impose through the diffusivity of sound ``delta`` (the inverse of
    ``compute_diffusivity_of_sound``, which takes the attenuation in dB/m = Np/m * 20 / ln 10).  It grows like f^2, so ``power_law(thermoviscous_absorption(delta, c, f0), 2, K)``
    makes the heat load equal what the wave loses."""
    delta, c = _arr(delta), _arr(c)
    return delta * (2.0 * np.pi * f) ** 2 / (2.0 * c ** 3)
