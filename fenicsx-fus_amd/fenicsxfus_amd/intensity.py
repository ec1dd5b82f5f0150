"""Host helpers around the intensity and radiation-force maps (fusmi.h "intensity"); no device needed.

With ``p_k(t) = C_k cos(w_k t) + S_k sin(w_k t)`` per harmonic (the monitor's ``cos`` / ``sin`` maps, ``w_k = 2 pi k f0``)
and the first-order momentum equation ``rho dw/dt = -grad p``:

* time-averaged intensity          ``I = sum_k (C_k grad S_k - S_k grad C_k) / (2 rho w_k)``          W/m^2
* radiation force density          ``F = sum_k 2 alpha_k I_k / c``                                    N/m^3
* particle velocity of harmonic k  ``w_k(t) = (C_k' sin(w_k t) - S_k' cos(w_k t)) / (rho w_k)``, ``X' = grad X``

The model methods ``intensity()`` and ``radiation_force()`` pass the coefficient rows built here to the device."""
from __future__ import annotations

import numpy as np


def _cells(v, name):
    v = np.asarray(v, dtype=np.float64)
    if v.ndim != 1 or len(v) == 0:
        raise ValueError(f"{name} must be a 1-D array, one value per cell, got shape {v.shape}")
    return v


def intensity_coef(rho, f0: float, K: int) -> np.ndarray:
    """Rows ``1 / (2 rho w_k)``, k = 1..K, shape (K, ncells), in m^3 s / kg: the pair form with them is I in W/m^2."""
    rho = _cells(rho, "rho")
    if not (K >= 1 and f0 > 0 and np.all(rho > 0)):
        raise ValueError("intensity_coef: K >= 1, f0 > 0 and rho > 0 in every cell")
    w = 2.0 * np.pi * f0 * np.arange(1, K + 1, dtype=np.float64)
    return 1.0 / (2.0 * rho[None, :] * w[:, None])


def force_coef(alpha_rows, rho, c, f0: float) -> np.ndarray:
    """Rows ``alpha_k / (rho c w_k)`` = ``(2 alpha_k / c) x intensity_coef``, shape (K, ncells): the pair form with them is
    the radiation force density in N/m^3.  ``alpha_rows``: (K, ncells) in Np/m, or 1-D for the fundamental only."""
    a = np.atleast_2d(np.asarray(alpha_rows, dtype=np.float64))
    rho, c = _cells(rho, "rho"), _cells(c, "c")
    if a.ndim != 2 or a.shape[1] != len(rho) or c.shape != rho.shape:
        raise ValueError(f"force_coef: absorption rows {a.shape} do not match {len(rho)} cells")
    if not (np.all(np.isfinite(a)) and np.all(a >= 0) and np.all(c > 0)):
        raise ValueError("force_coef: absorption must be >= 0 and finite, c > 0 in every cell")
    return 2.0 * a / c[None, :] * intensity_coef(rho, f0, a.shape[0])


def velocity_amplitude(grad_cos, grad_sin, rho, omega: float) -> np.ndarray:
    """``|w_k|`` per DOF in m/s, the peak particle speed of one harmonic: ``sqrt(|grad C|^2 + |grad S|^2) / (rho w)`` from
    the nodal gradients (tdim, ndofs) of its maps; ``rho`` a scalar or one value per DOF."""
    gc, gs = np.asarray(grad_cos, dtype=np.float64), np.asarray(grad_sin, dtype=np.float64)
    if gc.ndim != 2 or gc.shape != gs.shape:
        raise ValueError(f"velocity_amplitude: gradients must both be (tdim, ndofs), got {gc.shape} and {gs.shape}")
    rho = np.asarray(rho, dtype=np.float64)
    if rho.ndim and rho.shape != (gc.shape[1],):
        raise ValueError(f"velocity_amplitude: rho must be a scalar or {gc.shape[1]} values, one per DOF")
    if not omega > 0:
        raise ValueError("velocity_amplitude: omega > 0")
    return np.sqrt((gc * gc + gs * gs).sum(axis=0)) / (rho * omega)


def power_through(V, I, dofs, normal, weights) -> float:
    """``sum_i weights[i] I(dofs[i]) . normal`` in W: the power through a flat patch of face DOFs with unit ``normal``
    and quadrature ``weights`` (m^2 per DOF, e.g. a facet_diag of ones on that face).  ``I``: (ndofs, tdim) as
    ``model.intensity()`` returns it."""
    I = np.asarray(getattr(getattr(I, "x", I), "array", I), dtype=np.float64)
    dofs = np.asarray(dofs, dtype=np.int64)
    n, w = np.asarray(normal, dtype=np.float64), np.asarray(weights, dtype=np.float64)
    nd = V.dofmap.index_map.size_local + V.dofmap.index_map.num_ghosts
    if I.ndim != 2 or I.shape[0] != nd or n.shape != (I.shape[1],):
        raise ValueError(f"power_through: I must be ({nd}, tdim) and normal (tdim,), got {I.shape} and {n.shape}")
    if dofs.ndim != 1 or w.shape != dofs.shape or (len(dofs) and (dofs.min() < 0 or dofs.max() >= nd)):
        raise ValueError("power_through: dofs and weights must be 1-D of one length, dofs inside the space")
    return float(w @ (I[dofs] @ n))
