"""Transducers outside the mesh: the Rayleigh integral of a radiating surface (fusmi.h "transducers").

A bowl or an array sits in a homogeneous coupling medium in front of the meshed region.  Its surface is sampled by
equal-area points (:func:`bowl`, :func:`disc`) that carry a complex volume velocity ``q = v_n dA`` in m^3/s
(:func:`volume_velocity`); with the time convention ``p(x, t) = Re[P(x) exp(-i w t)]`` -- ``P = COS_1 + i SIN_1`` in the
monitor's terms --

    P(x)      = -(i w rho / 2 pi) sum_s q_s exp(i k r_s) exp(-alpha r_s) / r_s,      r_s = |x - x_s|,  k = w / c
    grad P(x) = -(i w rho / 2 pi) sum_s q_s (i k - alpha - 1/r_s) exp(i k r_s) exp(-alpha r_s) / r_s (x - x_s) / r_s

:func:`field` evaluates both on the device (``fus_rayleigh``; there is no host path behind it), :func:`drive` turns the
field on the source face of a box into the per-DOF amplitude and delay of ``model.set_source``, and
``model.set_transducer`` does the two for the DOFs of the tag-1 facets.  The same integral over all DOFs is the free-field
reference of a homogeneous run: compare it with ``monitor_get("cos", 1) + 1j * monitor_get("sin", 1)``.

The geometry helpers and :func:`drive` are numpy only.  3-D only."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _abi
from ._abi import check, lib, ptr

_GOLDEN = math.pi * (3.0 - math.sqrt(5.0))


def _frame(axis):
    """Two unit vectors that complete the unit vector ``axis`` to a right-handed frame."""
    k = int(np.argmin(np.abs(axis)))
    e1 = np.cross(axis, np.eye(3)[k])
    e1 /= np.linalg.norm(e1)
    return e1, np.cross(axis, e1)


def _check_n(n, d, di):
    if not (int(n) >= 1 and d > 0 and 0 <= di < d):
        raise ValueError("n >= 1, diameter > 0 and 0 <= inner_diameter < diameter")
    return int(n)


def bowl(apex, focus, diameter: float, n: int, inner_diameter: float = 0.0):
    """``n`` equal-area Fibonacci points on a spherical cap: radius of curvature ``R = |focus - apex|``, aperture radius
    ``a = diameter / 2`` (at most R), depth ``h = R - sqrt(R^2 - a^2)``.  Point i sits at the height
    ``z_i = h_in + (h - h_in) (i + 1/2) / n`` above the apex along the axis (``h_in`` the depth of the cap that
    ``inner_diameter`` removes) at the azimuth ``i pi (3 - sqrt 5)``.  Returns ``(points [n, 3], areas [n], normals
    [n, 3])`` with ``dA = 2 pi R (h - h_in) / n`` and the normals towards the focus, the radiating side."""
    apex, focus = np.asarray(apex, dtype=np.float64), np.asarray(focus, dtype=np.float64)
    n = _check_n(n, diameter, inner_diameter)
    R = float(np.linalg.norm(focus - apex))
    a, ai = 0.5 * diameter, 0.5 * inner_diameter
    if not (R > 0 and a <= R):
        raise ValueError("the focus must differ from the apex and the aperture radius must not exceed |focus - apex|")
    axis = (focus - apex) / R
    e1, e2 = _frame(axis)
    h, hi = R - math.sqrt(R * R - a * a), R - math.sqrt(R * R - ai * ai)
    i = np.arange(n, dtype=np.float64)
    z = hi + (h - hi) * (i + 0.5) / n
    s = np.sqrt(z * (2.0 * R - z))
    phi = i * _GOLDEN
    pts = apex + z[:, None] * axis + s[:, None] * (np.cos(phi)[:, None] * e1 + np.sin(phi)[:, None] * e2)
    return pts, np.full(n, 2.0 * math.pi * R * (h - hi) / n), (focus - pts) / R


def disc(center, normal, diameter: float, n: int, inner_diameter: float = 0.0):
    """``n`` equal-area Fibonacci points on a flat disc (an annulus with ``inner_diameter``): radius
    ``sqrt(a_in^2 + (a^2 - a_in^2) (i + 1/2) / n)``, azimuth ``i pi (3 - sqrt 5)``, ``dA = pi (a^2 - a_in^2) / n``.
    Returns ``(points [n, 3], areas [n], normals [n, 3])``, the normals along ``normal``, the radiating side."""
    center, nv = np.asarray(center, dtype=np.float64), np.asarray(normal, dtype=np.float64)
    n = _check_n(n, diameter, inner_diameter)
    nv = nv / np.linalg.norm(nv)
    e1, e2 = _frame(nv)
    a, ai = 0.5 * diameter, 0.5 * inner_diameter
    i = np.arange(n, dtype=np.float64)
    r = np.sqrt(ai * ai + (a * a - ai * ai) * (i + 0.5) / n)
    phi = i * _GOLDEN
    pts = center + r[:, None] * (np.cos(phi)[:, None] * e1 + np.sin(phi)[:, None] * e2)
    return pts, np.full(n, math.pi * (a * a - ai * ai) / n), np.tile(nv, (n, 1))


def points_needed(area: float, f: float, c: float, per_wavelength: float = 2.0) -> int:
    """The smallest ``n`` for which ``sqrt(area / n) <= lambda / per_wavelength``, ``lambda = c / f``."""
    if not (area > 0 and f > 0 and c > 0 and per_wavelength > 0):
        raise ValueError("area, f, c and per_wavelength must be positive")
    return max(1, int(math.ceil(area * (per_wavelength * f / c) ** 2 * (1 - 1e-14))))


def volume_velocity(areas, v0=1.0, phase=0.0):
    """Complex ``q = v0 exp(i phase) dA`` in m^3/s; ``v0`` (m/s) and ``phase`` (rad) scalars or one value per point:
    apodisation and array steering.  Under exp(-i w t) a point that fires ``tau`` later has ``phase = w tau``."""
    areas = np.asarray(areas, dtype=np.float64)
    return (np.asarray(v0, dtype=np.float64) * areas) * np.exp(1j * np.asarray(phase, dtype=np.float64))


# ---- the field, on the device ------------------------------------------------------------------------------------------
_PREC = {"f64": _abi.FUS_RAY_F64, "mixed": _abi.FUS_RAY_MIXED}


_hip = None


def _hiplib():
    global _hip
    if _hip is None:
        _hip = C.CDLL("libamdhip64.so")
    return _hip


class DeviceArray:
    """A float64 array in device memory: what :func:`field` returns when its inputs are device arrays, and a way to make
    such inputs from numpy (any object with ``__cuda_array_interface__`` serves as well, a torch tensor for one).
    ``numpy()`` copies it back; ``free()`` (or the collector) releases the memory."""

    def __init__(self, shape):
        self.shape = tuple(int(k) for k in shape)
        self.nbytes = 8 * int(np.prod(self.shape))
        self.ptr = C.c_void_p()
        if _hiplib().hipMalloc(C.byref(self.ptr), C.c_size_t(max(self.nbytes, 16))) != 0:
            raise _abi.FusError(f"cannot allocate {self.nbytes} bytes of device memory")

    @classmethod
    def from_numpy(cls, a):
        """float64 as it is; complex128 [n] as float64 [n, 2] (re, im)."""
        a = np.asarray(a)
        a = np.ascontiguousarray(a, dtype=np.complex128).view(np.float64).reshape(a.shape + (2,)) if np.iscomplexobj(a) \
            else np.ascontiguousarray(a, dtype=np.float64)
        d = cls(a.shape)
        if a.nbytes and _hiplib().hipMemcpy(d.ptr, ptr(a), C.c_size_t(a.nbytes), C.c_int(1)) != 0:
            raise _abi.FusError("hipMemcpy to the device failed")
        return d

    def numpy(self):
        out = np.empty(self.shape)
        if self.nbytes and _hiplib().hipMemcpy(ptr(out), self.ptr, C.c_size_t(self.nbytes), C.c_int(2)) != 0:
            raise _abi.FusError("hipMemcpy from the device failed")
        return out

    @property
    def __cuda_array_interface__(self):
        return {"shape": self.shape, "typestr": "<f8", "data": (self.ptr.value, False), "version": 3}

    def free(self):
        if self.ptr:
            _hiplib().hipFree(self.ptr)
            self.ptr = C.c_void_p()

    def __del__(self):
        try:
            self.free()
        except Exception:   # interpreter shutdown
            pass


def _is_device(a):
    return hasattr(a, "__cuda_array_interface__")


def _device_view(a, name, last):
    """(pointer, rows) of a contiguous device array float64 [rows, last] (or, last == 2, complex128 [rows])."""
    i = a.__cuda_array_interface__
    shape, ts = tuple(i["shape"]), i["typestr"]
    if i.get("strides") is not None:
        raise _abi.FusError(f"field: the device array {name} must be contiguous")
    if ts == "<c16" and last == 2 and len(shape) == 1:
        shape = shape + (2,)
    elif ts != "<f8":
        raise _abi.FusError(f"field: the device array {name} must be float64, got {ts}")
    if len(shape) != 2 or shape[1] != last:
        raise _abi.FusError(f"field: {name} must be [n, {last}], got {shape}")
    return C.c_void_p(i["data"][0]), shape[0]


def plan(ctx, nsrc: int, ntgt: int, gradient: bool = False, rmin: bool = False):
    """What :func:`field` launches for these sizes: ``(source chunks, targets per workgroup, kernel launches, workspace
    bytes)`` (``fus_rayleigh_plan``; the context option "rayleigh_chunks" forces the chunk count)."""
    what = _abi.FUS_RAY_P | (_abi.FUS_RAY_GRAD if gradient else 0) | (_abi.FUS_RAY_RMIN if rmin else 0)
    out = (C.c_int64 * 4)()
    check(lib().fus_rayleigh_plan(ctx.h, C.c_int64(nsrc), C.c_int64(ntgt), C.c_int(what), out))
    return tuple(out)


def field(ctx, points, q, targets, f: float, c: float, rho: float, alpha: float = 0.0, gradient: bool = False,
          rmin: bool = False, precision: str = "f64"):
    """The complex pressure ``P [ntgt]`` of the surface ``points [nsrc, 3]`` with volume velocities ``q [nsrc]`` (complex)
    at ``targets [ntgt, 3]``, in a medium of sound speed ``c``, density ``rho`` and absorption ``alpha`` (Np/m).  With
    ``gradient`` also ``gradP [ntgt, 3]`` (complex), with ``rmin`` also the distance to the nearest surface point; the
    result is ``P`` or the tuple ``(P, gradP, rmin)`` without what was not asked for.  ``precision``: "f64", or "mixed" --
    distances and phase reduction in double, the transcendental functions and products in float, sums in double.
    numpy arrays in, numpy arrays out.  Or all three inputs device arrays (:class:`DeviceArray`, or anything with
    ``__cuda_array_interface__``: float64 [n, 3], ``q`` float64 [n, 2] or complex128 [n]), written before the call is made:
    then nothing crosses the bus and the result is the :class:`DeviceArray` double[planes, ntgt] of fusmi.h -- P_re, P_im;
    with ``gradient`` Px_re, Px_im, Py_re, Py_im, Pz_re, Pz_im; with ``rmin`` the nearest distance."""
    if precision not in _PREC:
        raise _abi.FusError(f"unknown precision {precision!r}: \"f64\" or \"mixed\"")
    what = _abi.FUS_RAY_P | (_abi.FUS_RAY_GRAD if gradient else 0) | (_abi.FUS_RAY_RMIN if rmin else 0)
    planes = 2 + (6 if gradient else 0) + (1 if rmin else 0)
    dev = [_is_device(a) for a in (points, q, targets)]
    if any(dev):
        if not all(dev):
            raise _abi.FusError("field: points, q and targets must all be host arrays or all device arrays")
        (psx, nsrc), (pq, nq), (ptx, ntgt) = (_device_view(points, "points", 3), _device_view(q, "q", 2),
                                               _device_view(targets, "targets", 3))
        if nq != nsrc:
            raise _abi.FusError(f"field: {nsrc} points but {nq} volume velocities")
        out = DeviceArray((planes, ntgt))
        ctx.synchronize()
        check(lib().fus_rayleigh(ctx.h, C.c_int64(nsrc), psx, pq, C.c_int64(ntgt), ptx, C.c_double(f), C.c_double(c),
                                 C.c_double(rho), C.c_double(alpha), C.c_int(what), C.c_int(_PREC[precision]), out.ptr,
                                 C.c_int(_abi.FUS_DEVICE)))
        return out
    sx = np.ascontiguousarray(points, dtype=np.float64)
    qq = np.ascontiguousarray(q, dtype=np.complex128).reshape(-1).view(np.float64).reshape(-1, 2)
    tx = np.ascontiguousarray(targets, dtype=np.float64)
    nsrc, ntgt = sx.shape[0], tx.shape[0]
    if sx.ndim != 2 or sx.shape[1] != 3 or qq.shape != (nsrc, 2) or tx.ndim != 2 or tx.shape[1] != 3:
        raise _abi.FusError(f"field: points [nsrc, 3], q [nsrc] and targets [ntgt, 3] are expected, got {sx.shape}, "
                            f"{np.shape(q)} and {tx.shape}")
    out = np.zeros((planes, max(ntgt, 1)))
    check(lib().fus_rayleigh(ctx.h, C.c_int64(nsrc), ptr(sx), ptr(qq), C.c_int64(ntgt), ptr(tx), C.c_double(f), C.c_double(c),
                             C.c_double(rho), C.c_double(alpha), C.c_int(what), C.c_int(_PREC[precision]), ptr(out),
                             C.c_int(_abi.FUS_HOST)))
    cplx, stack = (lambda re, im: re + 1j * im), (lambda v: np.stack(v, axis=1))  # noqa: E731
    res = [cplx(out[0], out[1])]
    if gradient:
        res.append(stack([cplx(out[2 + 2 * d], out[3 + 2 * d]) for d in range(3)]))
    if rmin:
        res.append(out[planes - 1])
    return res[0] if len(res) == 1 else tuple(res)


# ---- the boundary drive ------------------------------------------------------------------------------------------------
def drive(P, gradP, normal, f: float, C: float, c: float | None = None, mode: str = "neumann", arrival=None):
    """Amplitude and delay of ``model.set_source`` from the field on the source boundary.  The tag-1 term of the models is
    facet weight x ``g_d(t)``, in steady state ``g_d = a_d C cos(w (t - tau_d))``, the outward normal derivative of p.
    ``mode="neumann"`` (source facets without an absorbing term: Linear; Lossy / Westervelt with ``forms="python"``):
    ``G = grad P . n``.  ``mode="transparent"`` (with one: Lossy / Westervelt with ``forms="cpp"``):
    ``G = grad P . n - (i w / c) P``.  Then ``a = |G| / C`` and ``tau = arg(G) / w`` wrapped into [0, 1/f), so that
    ``a C cos(w (t - tau)) = Re[G exp(-i w t)]``.  ``normal``: the outward unit normal, [3] or one per point.
    With ``arrival`` (seconds per point, e.g. ``rmin / c``) the delay is moved by whole periods to the one nearest to
    it, ``tau + round((arrival - tau) f) / f``: ramp and burst then start when the first wavelet arrives.
    Returns ``(amplitude, delay)``."""
    if mode not in ("neumann", "transparent"):
        raise ValueError(f"unknown mode {mode!r}: \"neumann\" or \"transparent\"")
    if not (f > 0 and C > 0):
        raise ValueError("f and C must be positive")
    P, gradP = np.asarray(P, dtype=np.complex128), np.asarray(gradP, dtype=np.complex128)
    nv = np.asarray(normal, dtype=np.float64)
    if gradP.ndim != 2 or gradP.shape != P.shape + (3,) or nv.shape not in ((3,), gradP.shape):
        raise ValueError(f"P [n], gradP [n, 3] and normal [3] or [n, 3] are expected, got {P.shape}, {gradP.shape}, {nv.shape}")
    w = 2.0 * math.pi * f
    G = (gradP * nv).sum(axis=1)
    if mode == "transparent":
        if c is None or not c > 0:
            raise ValueError("the transparent mode needs the sound speed c > 0")
        G = G - (1j * w / c) * P
    amp = np.abs(G) / C
    tau = np.mod(np.angle(G), 2.0 * math.pi) / w
    tau = np.where(tau >= 1.0 / f, 0.0, tau)
    if arrival is not None:
        ta = np.asarray(arrival, dtype=np.float64)
        tau = tau + np.round((ta - tau) * f) / f
    return amp, tau


# ---- the DOFs of the source boundary -----------------------------------------------------------------------------------
_HEX_FACETS = [(2, 0), (1, 0), (0, 0), (0, 1), (1, 1), (2, 1)]   # DOLFINx local facet -> (axis, side)


def facet_dofs(V, cells, local_facets):
    """The DOFs (ascending, unique) on the hexahedron facets given as (cell, local facet) pairs, from the tensor dofmap
    of ``V``."""
    dm = np.asarray(V.tensor_dofmap)
    N = int(V.P) + 1
    if dm.shape[1] != N ** 3:
        raise ValueError("transducers are 3-D only: the space is not one of hexahedra")
    nodes = np.asarray(V.nodes1d, dtype=np.float64)
    loc = np.indices((N,) * 3).reshape(3, -1)
    cells, lf = np.asarray(cells, dtype=np.int64), np.asarray(local_facets, dtype=np.int64)
    parts = []
    for k, (ax, side) in enumerate(_HEX_FACETS):
        sel = cells[lf == k]
        if len(sel):
            on = np.flatnonzero(np.abs(nodes[loc[ax]] - side) < 1e-12)
            parts.append(dm[sel][:, on].ravel())
    return np.unique(np.concatenate(parts)) if parts else np.zeros(0, dtype=np.int64)


def outward_normal(x, centroid, tol: float = 1e-9):
    """The unit normal of the plane through the points ``x [n, 3]``, on the side away from ``centroid``.  ValueError when
    the points do not lie in a plane (to ``tol`` of their extent) -- a curved source boundary needs the caller's normals."""
    x = np.asarray(x, dtype=np.float64)
    if x.ndim != 2 or x.shape[1] != 3 or len(x) < 3:
        raise ValueError("at least three points [n, 3] are needed to fit the source plane")
    m = x.mean(axis=0)
    _, s, vt = np.linalg.svd(x - m, full_matrices=False)
    if not s[1] > tol * s[0]:
        raise ValueError("the source boundary's DOFs lie on a line: no plane to fit")
    if s[2] > tol * s[0]:
        raise ValueError("the source boundary is not planar: pass the outward normals of its DOFs (normal=...)")
    nv = vt[2]
    return -nv if np.dot(nv, m - np.asarray(centroid, dtype=np.float64)) < 0 else nv
