"""Damping profiles for the absorbing layers of the wave models (``model.set_sponge``; fusmi.h, "absorbing layers").

Inside a layer the models solve ``(d/dt + sigma)^2 u = RHS``: a plane wave decays as ``exp(-sigma s / c)`` along its
path whatever its direction.  For the profile ``sigma(d) = sigma_max (d / L)^n`` over the thickness ``L`` (``d`` the depth
into the layer) the amplitude that returns from whatever lies behind the layer, after the way in and the way out, is

    R = exp(-2 sigma_max L / ((n + 1) c)),        sigma_max = (n + 1) c ln(1 / R) / (2 L)

at normal incidence, and smaller at any other angle (the path is longer).  What the layer itself reflects comes from the
gradient of sigma: keep it at two wavelengths or more (:func:`min_thickness`)."""
from __future__ import annotations

import numpy as np

FACES = ("x-", "x+", "y-", "y+", "z-", "z+")


def sigma_max(thickness: float, c: float, reflection: float = 1e-3, order: int = 2) -> float:
    """The peak damping rate (1/s) of a layer designed for the round-trip amplitude reflection ``reflection``."""
    if not (0.0 < reflection < 1.0) or thickness <= 0.0 or order < 0:
        raise ValueError("sigma_max: needs 0 < reflection < 1, thickness > 0 and order >= 0")
    return (order + 1) * c * np.log(1.0 / reflection) / (2.0 * thickness)


def design_reflection(sigma_max: float, thickness: float, c: float, order: int = 2) -> float:
    """The round-trip amplitude reflection of a layer with the peak rate ``sigma_max``: the inverse of :func:`sigma_max`."""
    return float(np.exp(-2.0 * sigma_max * thickness / ((order + 1) * c)))


def min_thickness(c: float, f0: float, wavelengths: float = 2.0) -> float:
    """A layer thickness of ``wavelengths`` wavelengths at the frequency ``f0`` in a medium with sound speed ``c``."""
    return wavelengths * c / f0


def layer_sigma(X, lo, hi, thickness, c: float, reflection: float = 1e-3, order: int = 2):
    """The damping rate per DOF for layers on the faces of the box [lo, hi], from the DOF coordinates ``X`` [ndofs, >= tdim]
    (``V.tabulate_dof_coordinates()``; 2-D and 3-D by the length of ``lo``).

    ``thickness`` is one thickness for every face, or a mapping over the faces "x-", "x+", "y-", "y+" (, "z-", "z+"); a
    face left out gets no layer -- normally the source face.  Each face contributes ``sigma_max (d / L)^order`` with ``d``
    the depth behind the plane a distance ``L`` inside the face, and the result is the sum over the faces: in edges and
    corners the tapers multiply.  ``c`` is the sound speed in the layer, ``reflection`` the design round-trip amplitude
    reflection of each layer (see the module text)."""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    tdim = len(lo)
    X = np.asarray(X, np.float64)
    if tdim not in (2, 3) or len(hi) != tdim or X.ndim != 2 or X.shape[1] < tdim:
        raise ValueError("layer_sigma: lo and hi have 2 or 3 entries and X at least as many columns")
    faces = FACES[:2 * tdim]
    if isinstance(thickness, dict):
        unknown = set(thickness) - set(faces)
        if unknown:
            raise ValueError(f"layer_sigma: unknown faces {sorted(unknown)}; the faces are {faces}")
        per_face = {f: float(L) for f, L in thickness.items() if L}
    else:
        per_face = {f: float(thickness) for f in faces}
    sigma = np.zeros(X.shape[0])
    for face, L in per_face.items():
        ax = "xyz".index(face[0])
        depth = (lo[ax] + L) - X[:, ax] if face[1] == "-" else X[:, ax] - (hi[ax] - L)
        d = np.clip(depth / L, 0.0, 1.0)
        sigma += sigma_max(L, c, reflection, order) * np.where(d > 0.0, d**order, 0.0)
    return sigma
