"""Pennes bioheat model and CEM43 thermal dose on the mesh of the wave models (fusmi.h "bioheat").

``BioheatSpectralExplicit`` advances the temperature rise ``theta = T - t_base`` of

    rho C dtheta/dt = div(k grad theta) - W theta + Q

with classical RK4 on the GPU, or with the super-time-stepping scheme RKL2 (``steps(..., stages=s)``: s operator
applications per step, a step about ``(s^2 + s - 2) / 5.6`` times the RK4 step), and accumulates the thermal dose in
cumulative equivalent minutes at 43 degrees C.  The
heat load comes from a nodal field (:meth:`set_heat`) or, without leaving the device, from the field monitor of a wave
model that shares the operator data (:meth:`set_heat_from`): ``Q = 2 alpha p_rms^2 / (rho c)``, or harmonic by harmonic
with an absorption that grows with frequency.  Every face is
insulating until :meth:`BioheatSpectralExplicit.set_boundary` holds it at a temperature (a cut face in tissue) or lets it
exchange heat with a coolant (water-cooled skin).  The perfusion may follow the temperature and the dose
(:meth:`BioheatSpectralExplicit.set_response`; :func:`perfusion_factor`), and the Arrhenius damage integral is accumulated
beside the dose (:meth:`BioheatSpectralExplicit.set_damage`; :func:`arrhenius_rate`).  The reference package has no thermal model; this module replaces
nothing there."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _abi
from ._abi import Context, check, lib, ptr
from .mesh import Function, FunctionSpace
from .operators import SpectralOperatorData, _array


def cem43(temps, dt: float, t_base: float = 0.0):
    """The dose rule in numpy: ``temps`` holds the end-of-step values of a sequence of steps of size ``dt`` seconds,
    first axis = step -- temperatures in degrees C, or rises over ``t_base``.  Returns the cumulative equivalent
    minutes at 43 degrees C, ``sum (dt / 60) 2^(-c (43 - T))`` with c = 1 for T >= 43 and 2 below (Sapareto and
    Dewey), evaluated in double in the order the kernel uses."""
    temps = np.asarray(temps, dtype=np.float64)
    D = np.zeros(temps.shape[1:], dtype=np.float64)
    for x in temps:
        T = t_base + x
        c = np.where(T >= 43.0, 1.0, 2.0)
        D = D + (dt / 60.0) * np.exp2(-(c * (43.0 - T)))
    return D


GAS_CONSTANT = 8.314462618          # J/mol/K


def perfusion_factor(T, D, temps=None, factors=None, dose_range=None):
    """The perfusion response in numpy (fusmi.h "perfusion response and damage"): ``phi = P(T) * S(D)`` for temperatures
    ``T`` in degrees C and doses ``D`` in CEM43 minutes, in double, in the order the kernel uses.  ``P`` is piecewise
    linear through the knots ``(temps[j], factors[j])`` and constant outside them (1 without knots); ``S`` falls linearly
    from 1 at ``dose_range[0]`` to 0 at ``dose_range[1]`` (1 without a range; equal ends: a step, 1 at the end itself)."""
    T, D = np.asarray(T, dtype=np.float64), np.asarray(D, dtype=np.float64)
    P = np.ones_like(T)
    if temps is not None and len(temps):
        t, f = np.asarray(temps, dtype=np.float64), np.asarray(factors, dtype=np.float64)
        j = np.clip(np.searchsorted(t, T, side="right") - 1, 0, max(len(t) - 2, 0))
        if len(t) > 1:
            P = f[j] + (f[j + 1] - f[j]) * ((T - t[j]) / (t[j + 1] - t[j]))
        P = np.where(T <= t[0], f[0], np.where(T >= t[-1], f[-1], P))
    S = np.ones_like(D)
    if dose_range is not None and dose_range[1] > 0:
        lo, hi = float(dose_range[0]), float(dose_range[1])
        with np.errstate(divide="ignore", invalid="ignore"):
            S = np.where(D <= lo, 1.0, np.where(D >= hi, 0.0, (hi - D) / (hi - lo)))
    return P * S


def arrhenius_rate(T, A: float, Ea: float):
    """The damage rate in numpy: ``exp(log(A) - Ea / (R (T + 273.15)))`` in 1/s for temperatures ``T`` in degrees C, ``A``
    in 1/s, ``Ea`` in J/mol, R = 8.314462618, in double, in the order the kernel uses.  One step from ``T_old`` to
    ``T_new`` adds ``(dt / 2) * (rate(T_old) + rate(T_new))`` to the damage integral."""
    T = np.asarray(T, dtype=np.float64)
    return np.exp(np.log(float(A)) - float(Ea) / (GAS_CONSTANT * (T + 273.15)))


STS_MIN_STAGES, STS_MAX_STAGES = 2, 32


def rkl2_coefficients(s: int):
    """``(mu, nu, mut, gat)`` of the s-stage Runge-Kutta-Legendre scheme of second order (Meyer, Balsara and Aslam, J.
    Comput. Phys. 257, 2014), float64 arrays of length s + 1 indexed by the stage j = 1..s (entry 0, and mu, nu, gat
    of stage 1, are 0); mirrors csrc/sts_coef.hpp bit for bit.  One step of y' = f(y):

        Y_0 = y,  F_0 = f(Y_0),  Y_1 = Y_0 + mut_1 dt F_0
        Y_j = mu_j Y_{j-1} + nu_j Y_{j-2} + (1 - mu_j - nu_j) Y_0 + mut_j dt f(Y_{j-1}) + gat_j dt F_0,   y <- Y_s

    stable on the negative real axis for ``dt lambda <= (s^2 + s - 2) / 2``."""
    s = int(s)
    if not STS_MIN_STAGES <= s <= STS_MAX_STAGES:
        raise ValueError(f"stages must lie in {STS_MIN_STAGES}..{STS_MAX_STAGES}, got {s}")

    def b(j):
        x = float(j)
        return 1.0 / 3.0 if j < 3 else (x * x + x - 2.0) / (2.0 * x * (x + 1.0))

    x = float(s)
    w1 = 4.0 / (x * x + x - 2.0)
    mu, nu, mut, gat = (np.zeros(s + 1) for _ in range(4))
    mut[1] = b(1) * w1
    for j in range(2, s + 1):
        y = float(j)
        mu[j] = (2.0 * y - 1.0) / y * b(j) / b(j - 1)
        nu[j] = -((y - 1.0) / y) * b(j) / b(j - 2)
        mut[j] = float(mu[j]) * w1
        gat[j] = -((1.0 - b(j - 1)) * float(mut[j]))
    return mu, nu, mut, gat


class BioheatSpectralExplicit:
    """``BioheatSpectralExplicit(mesh, k, conductivity, rho_c, perfusion=None, t_base=37.0)``: ``k`` the polynomial
    degree; ``conductivity`` (W/m/K, >= 0), ``rho_c`` (J/m^3/K, > 0) and ``perfusion`` (w_b rho_b C_b, W/m^3/K, >= 0;
    None = 0) one value per cell; ``t_base`` the arterial and initial temperature in degrees C.  ``model=`` shares the
    operator data of a wave model (required for :meth:`set_heat_from`), ``data=`` an existing
    :class:`SpectralOperatorData` (as the operator classes take it); the object then does not own the data and
    :meth:`close` leaves it alone.  On a mesh part with neighbours (``V.neighbours``) the context needs a transport:
    under an RCCL communicator the calls of this class are collective; the members of an in-process group are finished
    and advanced together by :func:`group_thermal_finish`, :func:`group_thermal_steps`, :func:`group_thermal_lambda_max`
    and :func:`group_thermal_stable_dt`."""

    def __init__(self, mesh, k, conductivity, rho_c, perfusion=None, t_base: float = 37.0, V=None,
                 ctx: Context | None = None, model=None, data: SpectralOperatorData | None = None):
        self.mesh, self.t_base = mesh, float(t_base)
        if model is not None and data is not None and data is not model.data:
            raise _abi.FusError("BioheatSpectralExplicit: data must be the operator data of model")
        if model is not None:
            data = model.data
        if data is not None:
            self.data, self._own_data = data, False
            self.V = data.V
            if V is not None and V is not data.V:
                raise _abi.FusError("BioheatSpectralExplicit: V must be the function space of the shared operator data")
            if ctx is not None and ctx is not data.ctx:
                raise _abi.FusError("BioheatSpectralExplicit: ctx must be the context of the shared operator data")
        else:
            self.V = V or FunctionSpace(mesh, k)
            self.data, self._own_data = SpectralOperatorData(self.V, ctx), True
        self.ctx = self.data.ctx
        self.dtype = self.data.dtype
        ka, ca = self._cells(conductivity, "conductivity"), self._cells(rho_c, "rho_c")
        wa = None if perfusion is None else self._cells(perfusion, "perfusion")
        self.h = C.c_void_p()
        try:
            check(lib().fus_thermal_create(self.ctx.h, self.data.h, ptr(ka), ptr(ca), ptr(wa), C.c_double(self.t_base),
                                           C.byref(self.h)))
        except _abi.FusError:
            if self._own_data:
                self.data.close()
            raise

    def _cells(self, a, name):
        """One value per cell (a scalar is broadcast), in the operator's scalar type."""
        a = np.asarray(_array(a), dtype=self.dtype)
        if a.ndim and a.shape != (self.data.ncells,):
            raise _abi.FusError(f"{name}: expected {self.data.ncells} values, one per cell, got shape {a.shape}")
        return np.ascontiguousarray(np.broadcast_to(a, (self.data.ncells,)))

    def _dofs(self, a, name, dtype=None):
        a = np.ascontiguousarray(_array(a), dtype=dtype or self.dtype)
        if a.shape != (self.data.ndofs,):
            raise _abi.FusError(f"{name}: expected {self.data.ndofs} values, one per DOF, got shape {a.shape}")
        return a

    def init(self):
        """Rise and dose to zero."""
        check(lib().fus_thermal_init(self.h))

    def set_state(self, rise=None, dose=None, damage=None):
        """Set the temperature rise (K over ``t_base``), the dose (minutes, float64) and / or the damage integral
        (float64; :meth:`set_damage` must be on), one value per DOF."""
        if damage is not None:
            a = self._dofs(damage, "damage", np.float64)
            check(lib().fus_thermal_set(self.h, C.c_int(_abi.FUS_TH_DAMAGE), ptr(a), C.c_int(_abi.FUS_HOST)))
        if rise is not None:
            a = self._dofs(rise, "rise")
            check(lib().fus_thermal_set(self.h, C.c_int(_abi.FUS_TH_RISE), ptr(a), C.c_int(_abi.FUS_HOST)))
        if dose is not None:
            a = self._dofs(dose, "dose", np.float64)
            check(lib().fus_thermal_set(self.h, C.c_int(_abi.FUS_TH_DOSE), ptr(a), C.c_int(_abi.FUS_HOST)))

    def set_heat(self, q, coef=None):
        """Heat load ``h = (M(coef) 1) .* q``: ``q`` a nodal field (W/m^3 with ``coef`` None = 1), ``coef`` a per-cell
        factor.  ``q`` None: no heat."""
        if q is None:
            check(lib().fus_thermal_set_heat(self.h, None, None, C.c_int(_abi.FUS_HOST)))
            return
        qa = self._dofs(q, "q")
        ca = None if coef is None else self._cells(coef, "coef")
        check(lib().fus_thermal_set_heat(self.h, ptr(qa), ptr(ca), C.c_int(_abi.FUS_HOST)))

    def set_heat_from(self, model, absorption):
        """Acoustic heating ``Q = 2 alpha p_rms^2 / (rho c)`` from the field monitor of ``model`` (watching u, at least
        one sample), on the device: ``absorption`` = alpha, amplitude absorption in Np/m at the source frequency, one
        value per cell (or a scalar).  ``model`` must be the one this object was created with (``model=``).

        A 2-D ``absorption`` of shape ``(K, ncells)`` takes the per-harmonic load instead (fusmi.h "per-harmonic heat
        load"): row ``k - 1`` is alpha at ``k`` times the source frequency (:func:`fenicsxfus_amd.monitor.power_law`),
        and ``Q = sum_k 2 alpha_k <p_k^2> / (rho c)`` over the harmonics ``1..K`` of the monitor (``nharm >= K``),
        ``<p_k^2>`` the mean square of harmonic ``k`` over the monitor's window -- whole periods, see
        :func:`fenicsxfus_amd.monitor.whole_period_window`.  The mean and the harmonics above ``K`` carry no heat."""
        if np.ndim(_array(absorption)) == 2:
            a = np.ascontiguousarray(_array(absorption), dtype=self.dtype)
            if a.shape[1] == 1:                                   # one value for all cells, as a scalar alpha gives
                a = np.ascontiguousarray(np.broadcast_to(a, (a.shape[0], self.data.ncells)))
            if a.shape[1] != self.data.ncells:
                raise _abi.FusError(f"absorption: expected {self.data.ncells} values per harmonic, one per cell, got shape "
                                    f"{a.shape}")
            check(lib().fus_thermal_set_heat_from_harmonics(self.h, model.h, C.c_int(a.shape[0]), ptr(a)))
            return
        a = self._cells(absorption, "absorption")
        check(lib().fus_thermal_set_heat_from_monitor(self.h, model.h, ptr(a)))

    def set_boundary(self, tags, fixed=None, convective=None):
        """Boundary conditions on tagged facets; every other face stays insulating, and any boundary set before is
        replaced.  ``tags``: a :class:`FacetTags` / DOLFINx-style mesh-tags object, as the wave models take it.
        ``fixed``: ``{tag: temperature}`` in degrees C, a scalar or one value per DOF (read on the face) -- the DOFs of
        those facets are held there.  ``convective``: ``{tag: (h_c, coolant temperature)}``, ``h_c`` >= 0 in W/m^2/K, a
        scalar or one value per cell (the facet takes its cell's), the temperature in degrees C, a scalar or one value
        per DOF: ``-k dT/dn = h_c (T - T_coolant)``.  A DOF on both kinds of face is fixed; where two convective faces
        meet their terms add, the coolant temperature being the average weighted by them."""
        nd, dt = self.data.ndofs, self.dtype
        cells, lf = np.asarray(tags.cells), np.asarray(tags.local_facets)
        values = np.asarray(tags.values)

        def diag(tag, coef):
            sel = np.flatnonzero(values == tag)
            if not len(sel):
                raise _abi.FusError(f"set_boundary: no facet carries the tag {tag}")
            return self.data.facet_diag(cells[sel], lf[sel], self._cells(coef, "h_c")).astype(np.float64)

        def rises(temp, name):
            a = np.asarray(_array(temp), dtype=np.float64)
            if a.ndim and a.shape != (nd,):
                raise _abi.FusError(f"{name}: expected a scalar or {nd} values, one per DOF, got shape {a.shape}")
            return np.broadcast_to(a - self.t_base, (nd,))

        mask = rise = m_h = r = None
        if fixed:
            mask, rise = np.zeros(nd, np.uint8), np.zeros(nd, np.float64)
            for tag, temp in fixed.items():
                on = diag(tag, 1.0) > 0.0
                mask[on] = 1
                rise[on] = rises(temp, "fixed temperature")[on]
        if convective:
            parts = [(diag(tag, h_c), rises(temp, "coolant temperature")) for tag, (h_c, temp) in convective.items()]
            m_h = np.sum([m for m, _ in parts], axis=0)
            faces = np.sum([m > 0.0 for m, _ in parts], axis=0)
            # several faces at a DOF: the average of their coolants' rises weighted by their terms; one face: its
            # coolant's rise as given (m theta / m need not return theta)
            r = np.divide(np.sum([m * ext for m, ext in parts], axis=0), m_h, out=np.zeros(nd), where=faces > 1)
            for m, ext in parts:
                on = (faces == 1) & (m > 0.0)
                r[on] = ext[on]
        self.set_boundary_arrays(mask, None if rise is None else rise.astype(dt),
                                 None if m_h is None else m_h.astype(dt), None if r is None else r.astype(dt))

    def set_boundary_arrays(self, fixed=None, fixed_rise=None, conv_diag=None, conv_rise=None):
        """The boundary per DOF (fus_thermal_set_boundary): ``fixed`` a mask (nonzero = held at ``fixed_rise``, K over
        ``t_base``; None = 0), ``conv_diag`` = m_H >= 0, the facet diagonal of h_c (``data.facet_diag`` with the
        coefficient h_c, summed over the convective faces), ``conv_rise`` the coolant's rise over ``t_base`` (None = 0).
        Replaces any boundary set before; all None clears it."""
        fa = None if fixed is None else self._dofs(np.asarray(_array(fixed)) != 0, "fixed", np.uint8)
        fr = None if fixed_rise is None else self._dofs(fixed_rise, "fixed_rise")
        cd = None if conv_diag is None else self._dofs(conv_diag, "conv_diag")
        cr = None if conv_rise is None else self._dofs(conv_rise, "conv_rise")
        check(lib().fus_thermal_set_boundary(self.h, ptr(fa), ptr(fr), ptr(cd), ptr(cr)))

    def clear_boundary(self):
        """Back to insulating faces everywhere: steps then run exactly as on an object that never had a boundary."""
        check(lib().fus_thermal_set_boundary(self.h, None, None, None, None))

    def boundary_info(self):
        """``(number of fixed DOFs, number of convective DOFs)`` in force."""
        nf, nc = C.c_int64(), C.c_int64()
        check(lib().fus_thermal_boundary_info(self.h, C.byref(nf), C.byref(nc)))
        return nf.value, nc.value

    def set_response(self, temps=None, factors=None, dose_range=None):
        """Let the perfusion follow the temperature and the dose (:func:`perfusion_factor`): each step runs with
        ``m_W * phi`` of the state it starts from.  ``temps`` / ``factors``: up to 8 knots, temperatures in degrees C
        strictly ascending, factors >= 0; ``dose_range`` = ``(dose_lo, dose_hi)`` in CEM43 minutes, the shutdown of
        coagulated tissue.  Replaces any response set before; all None clears it.  Call it before :meth:`stable_dt`: the
        step rule then takes the largest factor."""
        t = np.zeros(0) if temps is None else np.ascontiguousarray(temps, dtype=np.float64).ravel()
        f = np.zeros(0) if factors is None else np.ascontiguousarray(factors, dtype=np.float64).ravel()
        if len(t) != len(f):
            raise _abi.FusError(f"set_response: {len(t)} temperatures but {len(f)} factors")
        lo, hi = (0.0, 0.0) if dose_range is None else (float(dose_range[0]), float(dose_range[1]))
        check(lib().fus_thermal_set_response(self.h, C.c_int(len(t)), ptr(t) if len(t) else None,
                                             ptr(f) if len(f) else None, C.c_double(lo), C.c_double(hi)))

    def clear_response(self):
        """Back to the passive perfusion: steps then run exactly as on an object that never had a response."""
        check(lib().fus_thermal_set_response(self.h, C.c_int(0), None, None, C.c_double(0.0), C.c_double(0.0)))

    def set_damage(self, A: float, Ea: float = 0.0):
        """Accumulate the Arrhenius damage integral (:func:`arrhenius_rate`; trapezoid rule per step) from now on: ``A``
        in 1/s, ``Ea`` in J/mol.  ``A`` = 0 switches it off and frees its memory."""
        check(lib().fus_thermal_set_damage(self.h, C.c_double(A), C.c_double(Ea)))

    def lambda_max(self, iters: int = 20) -> float:
        """Rayleigh quotient after ``iters`` power iterations: a lower bound of the largest eigenvalue of
        ``m_C^-1 (K(k) + diag(phi_max m_W + m_H))`` (1/s) with the rows and columns of the fixed DOFs removed -- m_H the
        convective faces' diagonal, zero without :meth:`set_boundary`; phi_max the largest factor of
        :meth:`set_response`, 1 without one."""
        out = C.c_double()
        check(lib().fus_thermal_lambda_max(self.h, C.c_int(iters), C.byref(out)))
        return out.value

    def stable_dt(self, stages: int = 0) -> float:
        """Of the operator :meth:`lambda_max` names, the boundary in force included (a water-cooled face shortens the
        step).  ``stages`` = 0: ``2 / lambda_max(20)``, inside the RK4 limit 2.785 / lambda_max while the quotient has reached
        0.72 of it.  ``stages`` = s in 2..32: ``0.72 (s^2 + s - 2) / (2 lambda_max(20))``, inside the RKL2 limit
        (s^2 + s - 2) / (2 lambda_max) with the same margin, under the same condition."""
        out = C.c_double()
        check(lib().fus_thermal_stable_dt(self.h, C.c_int(20), C.c_int(stages), C.byref(out)))
        return out.value

    def steps(self, dt: float, n: int, heat_scale: float = 1.0, stages: int = 0):
        """``n`` steps of ``dt`` seconds with the heat load scaled by ``heat_scale`` (duty cycle; 0 = cooling).
        ``stages`` = 0: classical RK4, the dose by the rectangle rule on the end-of-step temperature.  ``stages`` = s in
        2..32: the super-time-stepping scheme RKL2 (:func:`rkl2_coefficients`) with s operator applications per step,
        the dose by the trapezoid rule on the temperatures at both ends of the step; take ``dt`` from
        ``stable_dt(stages=s)``.  Segments of either kind may follow each other."""
        if stages == 0:
            check(lib().fus_thermal_steps(self.h, C.c_double(dt), C.c_int64(n), C.c_double(heat_scale)))
        else:
            check(lib().fus_thermal_steps_sts(self.h, C.c_double(dt), C.c_int64(n), C.c_double(heat_scale),
                                              C.c_int(stages)))

    def _get(self, which, dtype) -> Function:
        f = Function(self.V, dtype)
        check(lib().fus_thermal_get(self.h, C.c_int(which), ptr(f.x.array), C.c_int(_abi.FUS_HOST)))
        return f

    def rise(self) -> Function:
        """Temperature rise over ``t_base`` (K)."""
        return self._get(_abi.FUS_TH_RISE, self.dtype)

    def temperature(self) -> Function:
        """``t_base + rise`` in degrees C."""
        f = self.rise()
        f.x.array[:] = f.x.array + f.x.array.dtype.type(self.t_base)
        return f

    def dose(self) -> Function:
        """CEM43 in minutes (float64)."""
        return self._get(_abi.FUS_TH_DOSE, np.float64)

    def heat(self) -> Function:
        """The heat load vector ``h`` (W per DOF)."""
        return self._get(_abi.FUS_TH_HEAT, self.dtype)

    def damage(self) -> Function:
        """The Arrhenius damage integral Omega (float64); :meth:`set_damage` must be on."""
        return self._get(_abi.FUS_TH_DAMAGE, np.float64)

    def perfusion(self) -> Function:
        """The perfusion plane the next step will use, ``m_W * phi`` (W/K per DOF): ``m_W`` itself without a response."""
        return self._get(_abi.FUS_TH_PERFUSION, self.dtype)

    def close(self):
        """Frees the thermal object, and the operator data if this object created it."""
        if self.h:
            lib().fus_thermal_destroy(self.h)
            self.h = C.c_void_p()
        if self._own_data:
            self.data.close()


def _handles(bios):
    return (C.c_void_p * len(bios))(*[b.h for b in bios]), C.c_int(len(bios))


def group_thermal_finish(bios):
    """In-process transport: the sharers' parts of m_C, m_W, the heat weight and the boundary flags of every member are
    added (ordered sums, the same bits on all sharers).  Call it after the members are created and again after any
    ``set_heat`` / ``set_heat_from`` / ``set_boundary``; a call with nothing pending does nothing."""
    check(lib().fus_group_thermal_finish(*_handles(bios)))


def group_thermal_steps(bios, dt: float, nsteps: int, heat_scale: float = 1.0, stages: int = 0):
    """In-process transport: ``nsteps`` steps of all members in lock-step, RK4 (``stages`` = 0) or RKL2 (2..32)."""
    arr, n = _handles(bios)
    check(lib().fus_group_thermal_steps(arr, n, C.c_double(dt), C.c_int64(nsteps), C.c_double(heat_scale), C.c_int(stages)))


def group_thermal_lambda_max(bios, iters: int = 20) -> float:
    """:meth:`BioheatSpectralExplicit.lambda_max` of the operator the members hold together."""
    arr, n = _handles(bios)
    out = C.c_double()
    check(lib().fus_group_thermal_lambda_max(arr, n, C.c_int(iters), C.byref(out)))
    return out.value


def group_thermal_stable_dt(bios, stages: int = 0, iters: int = 20) -> float:
    """:meth:`BioheatSpectralExplicit.stable_dt` of the operator the members hold together."""
    arr, n = _handles(bios)
    out = C.c_double()
    check(lib().fus_group_thermal_stable_dt(arr, n, C.c_int(iters), C.c_int(stages), C.byref(out)))
    return out.value
