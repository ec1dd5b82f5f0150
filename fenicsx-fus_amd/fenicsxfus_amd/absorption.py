"""Relaxation absorption of the wave models (``model.set_relaxation``; fusmi.h, "relaxation absorption"): the dispersion
relation of a medium with R relaxation processes and the fit of a power law alpha = alpha0 (f / MHz)^y by such processes.

A plane wave e^{i(w t - k x)} in a medium with the relaxation frequencies w_nu = 2 pi f_nu and the strengths a_nu (1/s) has

    k = (w / c) sqrt(1 + sum_nu a_nu / (w_nu + i w)),    alpha = -Im k ~ (1 / 2c) sum_nu a_nu w^2 / (w_nu^2 + w^2)

with c the HIGH-frequency sound speed (the model's ``c0``); the low-frequency one is c / sqrt(1 + sum_nu a_nu / w_nu).
Host-side numpy; only :func:`fit_power_law` needs scipy."""
from __future__ import annotations

import numpy as np


def _wavenumber(f, freqs_hz, strength, c):
    w = 2.0 * np.pi * np.asarray(f, dtype=np.float64)[..., None]
    wn = 2.0 * np.pi * np.atleast_1d(np.asarray(freqs_hz, dtype=np.float64))
    a = np.atleast_1d(np.asarray(strength, dtype=np.float64))
    if wn.shape != a.shape or wn.ndim != 1:
        raise ValueError(f"one strength per relaxation frequency: shapes {a.shape} and {wn.shape}")
    return (w[..., 0] / c) * np.sqrt(1.0 + (a / (wn + 1j * w)).sum(axis=-1))


def relaxation_alpha(f, freqs_hz, strength, c):
    """The exact absorption -Im k in Np/m at the frequencies ``f`` (Hz) for the relaxation frequencies ``freqs_hz`` (Hz),
    strengths ``strength`` (1/s, one per process) and high-frequency sound speed ``c``."""
    return -_wavenumber(f, freqs_hz, strength, c).imag


def relaxation_speed(f, freqs_hz, strength, c):
    """The phase speed w / Re k at the frequencies ``f``: c / sqrt(1 + sum a_nu / w_nu) as f -> 0, c as f -> infinity."""
    return 2.0 * np.pi * np.asarray(f, dtype=np.float64) / _wavenumber(f, freqs_hz, strength, c).real


def fit_power_law(alpha0, y, f_lo, f_hi, c, nrelax=2, freqs_hz=None, npoints=64, reweight=20):
    """Strengths a_nu >= 0 such that the relaxation absorption follows alpha0 (f / 1 MHz)^y Np/m over [f_lo, f_hi] Hz.

    Non-negative least squares of the RELATIVE error of the weak-absorption form (1 / 2c) sum_nu a_nu w^2 / (w_nu^2 + w^2),
    which is linear in the strengths, on ``npoints`` log-spaced frequencies, reweighted ``reweight`` times towards the
    smallest maximum error (0: plain least squares).  ``freqs_hz``: the relaxation frequencies (default: ``nrelax``
    log-spaced from f_lo to f_hi).  Returns ``(freqs_hz, strengths, max_rel_error)`` with the last
    the largest relative deviation of the EXACT :func:`relaxation_alpha` from the law on the same frequencies."""
    from scipy.optimize import nnls

    if freqs_hz is None:
        freqs_hz = np.geomspace(f_lo, f_hi, nrelax) if nrelax > 1 else np.array([np.sqrt(f_lo * f_hi)])
    freqs_hz = np.atleast_1d(np.asarray(freqs_hz, dtype=np.float64))
    f = np.geomspace(f_lo, f_hi, npoints)
    target = alpha0 * (f / 1e6) ** y
    w, wn = 2.0 * np.pi * f[:, None], 2.0 * np.pi * freqs_hz[None, :]
    basis = w * w / (wn * wn + w * w) / (2.0 * c) / target[:, None]
    # Plain least squares leaves its largest error at the ends of the band (0.103 for 5 f^1.1 over 0.25-4 MHz with two
    # processes).  Lawson's reweighting -- each frequency's weight multiplied by its current error -- moves the fit
    # towards the smallest MAXIMUM relative error (0.091 there); the error that steers it is the exact alpha's, the
    # weak-absorption form being corrected by the ratio of the two at the current strengths.
    weight, ratio = np.full(npoints, 1.0 / npoints), np.ones(npoints)
    best = None
    for _ in range(reweight + 1):
        sw = np.sqrt(weight)
        a, _ = nnls(basis * (ratio * sw)[:, None], sw)
        rel = relaxation_alpha(f, freqs_hz, a, c) / target
        err = np.abs(rel - 1.0)
        if best is None or err.max() < best[1]:
            best = (a, float(err.max()))
        lin = basis @ a
        ratio = np.where(lin > 0, rel / np.where(lin > 0, lin, 1.0), 1.0)
        weight = weight * np.maximum(err, 1e-300)
        weight /= weight.sum()
    return freqs_hz, best[0], best[1]
