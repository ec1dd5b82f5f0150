"""Host-side mirror of the reference model classes for the offloaded path.

``LinearSpectralExplicit`` keeps the constructor and ``init()`` / ``rk(t0, tf)`` signatures of
python/src/fenicsxfus/_linear.py:258-513 (and is the Python face of the C++ ``LinearSpectral3D``,
cpp/fenicsx-sf/common/Linear.hpp:52-347).  The whole RK4 loop runs on the GPU through
``fus_model_rk4`` with the reference's Runge-Kutta tables (``rk_order`` 1-4, _linear.py:286-311).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _abi
from ._abi import Context, check, lib, ptr
from .mesh import Function, FunctionSpace
from .operators import SpectralOperatorData, _array


class _SpectralExplicit:
    """Shared host side of the offloaded explicit models (constructor plumbing, init, rk)."""

    _kind = _abi.FUS_LINEAR

    def _create(self, mesh, meshtags, k, c0, rho0, delta0, freq0, p0, s0, rk_order, dt, V, ctx, beta0=None,
                forms="cpp"):
        if rk_order not in (1, 2, 3, 4):
            raise _abi.FusError("rk_order must be 1, 2, 3 or 4 (_linear.py:286-311)")
        if forms not in ("cpp", "python"):
            raise _abi.FusError("forms must be 'cpp' or 'python'")
        self.mesh, self.dt = mesh, dt
        self.freq, self.p0, self.s0 = float(freq0), float(p0), float(s0)
        self.V = V or FunctionSpace(mesh, k)
        self.data = SpectralOperatorData(self.V, ctx, fields=2 if delta0 is not None else 1)
        self.ctx = self.data.ctx
        dt_ = self.data.dtype
        c0a = np.ascontiguousarray(_array(c0), dtype=dt_)
        rhoa = np.ascontiguousarray(_array(rho0), dtype=dt_)
        dla = None if delta0 is None else np.ascontiguousarray(_array(delta0), dtype=dt_)
        bta = None if beta0 is None else np.ascontiguousarray(_array(beta0), dtype=dt_)
        cells = np.ascontiguousarray(meshtags.cells, dtype=np.int32)
        lf = np.ascontiguousarray(meshtags.local_facets, dtype=np.int32)
        tags = np.ascontiguousarray(meshtags.values, dtype=np.int32)
        self.h = C.c_void_p()
        self.ctx.set_option("forms", 1 if forms == "python" else 0)
        try:
            check(lib().fus_model_create(self.ctx.h, C.c_int(self._kind), self.data.h, ptr(c0a), ptr(rhoa),
                                         ptr(dla), ptr(bta), C.c_int64(len(cells)), ptr(cells), ptr(lf), ptr(tags),
                                         C.c_double(self.freq), C.c_double(self.p0), C.c_double(self.s0),
                                         C.byref(self.h)))
        finally:
            self.ctx.set_option("forms", 0)
        check(lib().fus_model_set_rk_order(self.h, C.c_int(rk_order)))
        self._c0, self._rho0 = c0a, rhoa          # radiation_force() forms alpha_k / (rho c w_k) from them
        self._source_facets = (cells[tags == 1], lf[tags == 1])   # set_transducer() takes their DOFs
        self._forms = forms
        self._mon_nharm, self._mon_freq = 0, self.freq
        self.u_n = Function(self.V, dt_)
        self.v_n = Function(self.V, dt_)
        self._nrecv = 0

    # ---- external transport (the caller exchanges the interface values; fusmi.h) ----
    def setup_count(self) -> int:
        return int(lib().fus_model_setup_count(self.h))

    def setup_pack(self, k: int):
        check(lib().fus_model_setup_pack(self.h, C.c_int(k)))

    def setup_unpack(self, k: int):
        check(lib().fus_model_setup_unpack(self.h, C.c_int(k)))

    def setup_finish(self):
        check(lib().fus_model_setup_finish(self.h))

    def stage_begin(self, i: int, t: float, dt: float):
        check(lib().fus_model_stage_begin(self.h, C.c_int(i), C.c_double(t), C.c_double(dt)))

    def stage_end(self, i: int, t: float, dt: float):
        check(lib().fus_model_stage_end(self.h, C.c_int(i), C.c_double(t), C.c_double(dt)))

    def init(self):
        """u_n = v_n = 0 (_linear.py:363-369, Linear.hpp:161-164)."""
        self.u_n.x.array[:] = 0.0
        self.v_n.x.array[:] = 0.0
        check(lib().fus_model_init(self.h))

    def set_state(self, u=None, v=None):
        for which, a in ((_abi.FUS_U, u), (_abi.FUS_V, v)):
            if a is not None:
                a = np.ascontiguousarray(_array(a), dtype=self.data.dtype)
                check(lib().fus_model_set(self.h, C.c_int(which), ptr(a), C.c_int(_abi.FUS_HOST)))

    def _pull(self):
        check(lib().fus_model_get(self.h, C.c_int(_abi.FUS_U), ptr(self.u_n.x.array), C.c_int(_abi.FUS_HOST)))
        check(lib().fus_model_get(self.h, C.c_int(_abi.FUS_V), ptr(self.v_n.x.array), C.c_int(_abi.FUS_HOST)))

    def rk(self, t0: float, tf: float):
        """Runge-Kutta solve from t0 to tf; returns (u_n, v_n, t) like _linear.py:430-513."""
        n = C.c_int64()
        check(lib().fus_model_rk4(self.h, C.c_double(t0), C.c_double(tf), C.c_double(self.dt), C.byref(n)))
        self.nsteps = n.value
        self._pull()
        return self.u_n, self.v_n, tf

    # C++-style aliases (Linear.hpp:228, 316, 318)
    def rk4(self, t0, tf, dt):
        self.dt = dt
        return self.rk(t0, tf)

    def rk4_steps(self, t0: float, dt: float, nsteps: int, sync: bool = True):
        """Exactly nsteps steps, asynchronous unless ``sync`` (benchmark entry)."""
        check(lib().fus_model_rk4_steps(self.h, C.c_double(t0), C.c_double(dt), C.c_int64(nsteps)))
        if sync:
            self.ctx.synchronize()

    def external_setup(self, exchange):
        """External transport, setup phase: sums the lumped mass (and Westervelt's mass diagonal) over
        the sharers through ``exchange()``, a callable that moves every neighbour's range of the send
        buffer into the matching range of the neighbour's receive buffer (see fusmi.h)."""
        for k in range(self.setup_count()):
            self.setup_pack(k)
            exchange()
            self.setup_unpack(k)
        self.setup_finish()

    def external_rk_steps(self, t0: float, dt: float, nsteps: int, exchange, rk_order: int = 4):
        """External transport: nsteps steps with the two halves of every stage around ``exchange()``."""
        t = t0
        for _ in range(nsteps):
            for i in range(rk_order):
                self.stage_begin(i, t, dt)
                exchange()
                self.stage_end(i, t, dt)
            t += dt

    # ---- receivers: point samples of the resident solution (utils.py:10-47 compute_eval_params + Function.eval) ----
    def set_receivers(self, points):
        """Locate ``points`` [n, tdim|3] in the local mesh (host, once) and hand (cell, reference coordinates) to the
        library; returns the indices of the points found on this rank (the reference's ``points_on_proc``)."""
        from .evaluate import locate

        cell, X = locate(self.mesh, points)
        on = np.flatnonzero(cell >= 0)
        cells = np.ascontiguousarray(cell[on], dtype=np.int32)
        Xr = np.ascontiguousarray(X[on], dtype=np.float64)
        check(lib().fus_model_set_receivers(self.h, C.c_int64(len(on)), ptr(cells), ptr(Xr)))
        self._nrecv = len(on)
        return on

    def sample(self, which: str = "u"):
        """u_h (or v_h) at the receivers, evaluated on the device from the resident vector."""
        out = np.zeros(self._nrecv, dtype=self.data.dtype)
        w = _abi.FUS_U if which == "u" else _abi.FUS_V
        check(lib().fus_model_sample(self.h, C.c_int(w), ptr(out), C.c_int(_abi.FUS_HOST)))
        return out

    def record(self, every: int, capacity: int, which: str = "u"):
        """Sample the receivers after every ``every``-th step into a device buffer of ``capacity`` records: the steps of
        rk() / rk4_steps(), of group_rk4_steps() (every slab model records its own receivers) and of the external stage
        loop (stage_end of a step's last stage).  A rank that holds no receiver still counts the records and times."""
        w = _abi.FUS_U if which == "u" else _abi.FUS_V
        check(lib().fus_model_record(self.h, C.c_int(w), C.c_int(every), C.c_int64(capacity)))

    def records(self):
        """(times [nrec], samples [nrec, npts]) recorded so far."""
        n = C.c_int64()
        check(lib().fus_model_get_records(self.h, None, None, C.byref(n)))
        out = np.zeros((n.value, self._nrecv), dtype=self.data.dtype)
        times = np.zeros(n.value)
        check(lib().fus_model_get_records(self.h, ptr(out), ptr(times), C.byref(n)))
        return times, out

    # ---- field monitor: whole-field maps accumulated on the device over a window of steps (fusmi.h) ----
    _MON = {"max": _abi.FUS_MON_MAX, "min": _abi.FUS_MON_MIN, "mean": _abi.FUS_MON_MEAN, "rms": _abi.FUS_MON_RMS,
            "cos": _abi.FUS_MON_COS, "sin": _abi.FUS_MON_SIN}

    def monitor(self, which: str = "u", nharm: int = 0, freq: float | None = None, skip: int = 0, every: int = 1,
                count: int = 0):
        """After every ``every``-th step past the first ``skip`` steps (at most ``count`` times; 0 = no cap) fold
        u (or v) into per-DOF running max / min, sum, sum of squares and the cosine / sine sums of the harmonics
        1..``nharm`` of ``freq`` (default: the source frequency).  Restarts the window; ``every=0`` is monitor_off()."""
        if which not in ("u", "v"):
            raise _abi.FusError(f"unknown monitor field {which!r}: \"u\" or \"v\"")
        w = _abi.FUS_U if which == "u" else _abi.FUS_V
        check(lib().fus_model_monitor(self.h, C.c_int(w), C.c_int(nharm), C.c_double(0.0 if freq is None else freq),
                                      C.c_int64(skip), C.c_int(every), C.c_int64(count)))
        self._mon_nharm, self._mon_freq = (nharm, float(freq or self.freq)) if every else (0, self.freq)

    def monitor_off(self):
        """Stop sampling and free the accumulators."""
        check(lib().fus_model_monitor(self.h, C.c_int(_abi.FUS_U), C.c_int(0), C.c_double(0.0), C.c_int64(0), C.c_int(0),
                                      C.c_int64(0)))
        self._mon_nharm = 0

    def monitor_info(self):
        """(number of samples, time of the first sample, time of the last sample)."""
        n, t0, t1 = C.c_int64(), C.c_double(), C.c_double()
        check(lib().fus_model_monitor_info(self.h, C.byref(n), C.byref(t0), C.byref(t1)))
        return n.value, t0.value, t1.value

    def monitor_get(self, name: str, k: int | None = None) -> Function:
        """The map ``name`` in "max", "min", "mean", "rms", "cos", "sin" (the last two: harmonic ``k`` >= 1) as a
        Function on the model's space (what output.write_vtu takes)."""
        if name not in self._MON:
            raise _abi.FusError(f"unknown monitor quantity {name!r}: one of {sorted(self._MON)}")
        f = Function(self.V, self.data.dtype)
        check(lib().fus_model_monitor_get(self.h, C.c_int(self._MON[name]), C.c_int(0 if k is None else k),
                                          ptr(f.x.array), C.c_int(_abi.FUS_HOST)))
        return f

    # ---- intensity and radiation force from the monitor's harmonic maps, on the device (fusmi.h "intensity") ----
    def _intensity(self, nharm, coef):
        out = np.zeros((self.data.tdim, self.data.ndofs), dtype=self.data.dtype)
        check(lib().fus_model_intensity(self.h, C.c_int(nharm), ptr(coef), ptr(out), C.c_int(_abi.FUS_HOST)))
        return np.ascontiguousarray(out.T)

    def intensity(self, nharm: int | None = None) -> np.ndarray:
        """The time-averaged intensity vector ``I = sum_k (COS_k grad SIN_k - SIN_k grad COS_k) / (2 rho w_k)`` in W/m^2
        over the harmonics 1..``nharm`` (default: all the monitor holds), recovered at the DOFs: an array (ndofs, tdim),
        the shape output.write_vtu writes as a vector field.  The monitor must watch "u" and hold a sample; neither the
        wave state nor the monitor changes."""
        return self._intensity(self._mon_nharm if nharm is None else int(nharm), None)

    def radiation_force(self, absorption) -> np.ndarray:
        """The acoustic radiation force density ``F = sum_k 2 alpha_k I_k / c`` in N/m^3, (ndofs, tdim).  ``absorption``:
        rows (K, ncells) in Np/m, one per harmonic (:func:`fenicsxfus_amd.monitor.power_law`), or 1-D for the fundamental
        only."""
        from .intensity import force_coef

        a = np.atleast_2d(np.asarray(_array(absorption), dtype=np.float64))
        if a.ndim != 2 or not 1 <= a.shape[0] <= 8 or a.shape[1] != self.data.ncells:
            raise _abi.FusError(f"radiation_force: absorption must be (K, {self.data.ncells}) with K in 1..8 or one row, "
                                f"got shape {a.shape}")
        coef = force_coef(a, self._rho0.astype(np.float64), self._c0.astype(np.float64), self._mon_freq)
        return self._intensity(a.shape[0], np.ascontiguousarray(coef, dtype=self.data.dtype))

    # ---- phased / apodised source: per-DOF amplitude and delay, optional tone burst (fusmi.h) ----
    def set_source(self, amplitude=None, delay=None, duration: float = 0.0):
        """Give every DOF of the source boundary (tag 1) its own amplitude factor (>= 0, default 1) and time delay
        (>= 0, default 0): the source there is ``amplitude * g(t - delay)``, 0 until ``t = delay``.  ``duration`` > 0
        makes it a tone burst that ramps down over its last four periods (at least eight periods long).  Arrays or
        Functions over the model's space; values off the source boundary are ignored (see
        :mod:`fenicsxfus_amd.source` for focusing and steering delays).  All defaults: :meth:`clear_source`."""
        a, d = (None if x is None else np.ascontiguousarray(_array(x), dtype=self.data.dtype) for x in (amplitude, delay))
        for x in (a, d):
            if x is not None and x.shape != (self.data.ndofs,):
                raise _abi.FusError(f"set_source: expected {self.data.ndofs} values, one per DOF, got shape {x.shape}")
        check(lib().fus_model_set_source(self.h, ptr(a), ptr(d), C.c_double(duration), C.c_int(_abi.FUS_HOST)))

    def clear_source(self):
        """Back to the default source: the same g(t) at every DOF of the source boundary."""
        check(lib().fus_model_set_source(self.h, None, None, C.c_double(0.0), C.c_int(_abi.FUS_HOST)))

    # ---- a transducer outside the mesh: the Rayleigh integral as the boundary drive (fusmi.h "transducers") ----
    def source_scale(self) -> float:
        """``scale`` of ``C = scale p0 w0 / s0``: 2 for Lossy / Westervelt with ``forms="cpp"`` (source doubled), else 1."""
        return 2.0 if self._kind != _abi.FUS_LINEAR and self._forms == "cpp" else 1.0

    def set_transducer(self, points, q, c: float, rho: float, alpha: float = 0.0, duration: float = 0.0, normal=None,
                       precision: str = "f64"):
        """Drive the source boundary (tag 1) with the field of a transducer outside the mesh: surface ``points [n, 3]``
        with complex volume velocities ``q [n]`` (:mod:`fenicsxfus_amd.transducer`) in a coupling medium of sound speed
        ``c``, density ``rho`` and absorption ``alpha`` (Np/m).  The Rayleigh integral with gradient and nearest
        distance is evaluated on the device at the DOFs of the tag-1 facets and becomes the per-DOF amplitude and
        delay of :meth:`set_source` (:func:`fenicsxfus_amd.transducer.drive`): the normal derivative where the source
        facets carry no absorbing term (Linear; ``forms="python"``), the transparent combination where they do
        (Lossy / Westervelt with ``forms="cpp"``), with ``C`` from the model's frequency, ``p0``, ``s0`` and source
        scale; the delays are moved by whole periods to the arrival of the first wavelet.  ``normal``: the outward unit
        normal(s) of the source boundary, [3] or one per source DOF in ascending DOF order; ``None`` fits a plane
        through those DOFs (ValueError when they are not planar) and takes the side away from the mesh centroid.
        Returns ``(P, amplitude, delay)`` on those DOFs (``self.transducer_dofs``); :meth:`clear_source` undoes it."""
        from . import transducer as td

        dofs = td.facet_dofs(self.V, *self._source_facets)
        if len(dofs) == 0:
            raise _abi.FusError("set_transducer: the model has no tag-1 (source) facets")
        x = np.ascontiguousarray(np.asarray(self.V.tabulate_dof_coordinates(), dtype=np.float64)[dofs])
        if normal is None:
            nv = td.outward_normal(x, np.asarray(self.mesh.geometry.x, dtype=np.float64).mean(axis=0))
        else:
            nv = np.asarray(normal, dtype=np.float64)
            if nv.shape not in ((3,), (len(dofs), 3)):
                raise _abi.FusError(f"set_transducer: normal must be [3] or [{len(dofs)}, 3], got shape {nv.shape}")
        P, gP, rmin = td.field(self.ctx, points, q, x, self.freq, c, rho, alpha, gradient=True, rmin=True,
                               precision=precision)
        scale = self.source_scale()
        Cs = scale * self.p0 * 2.0 * np.pi * self.freq / self.s0
        amp, tau = td.drive(P, gP, nv, self.freq, Cs, c=c, mode="transparent" if scale == 2.0 else "neumann",
                            arrival=rmin / c)
        if tau.min() < 0.0:   # whole periods: the phases stay
            tau = tau + np.ceil(-tau.min() * self.freq) / self.freq
        a, d = np.zeros(self.data.ndofs), np.zeros(self.data.ndofs)
        a[dofs], d[dofs] = amp, tau
        self.set_source(a, d, duration)
        self.transducer_dofs = dofs
        return P, amp, tau

    # ---- sources anywhere in the mesh, sampled drive signals (fusmi.h) ----
    def set_source_weights(self, w):
        """Give every DOF a source weight of its own (array or Function over the model's space, either sign): DOF d
        gains the right-hand-side term ``w[d] * g_d(t)`` with the model's source function, on top of the facet weight
        where d lies on the source boundary (:func:`fenicsxfus_amd.source.point_weights` for point sources).  Replaces
        earlier weights and puts the source function back to the default -- call :meth:`set_source` /
        :meth:`set_source_signals` afterwards; ``None`` removes the weights."""
        a = None if w is None else np.ascontiguousarray(_array(w), dtype=self.data.dtype)
        if a is not None and a.shape != (self.data.ndofs,):
            raise _abi.FusError(f"set_source_weights: expected {self.data.ndofs} values, one per DOF, got shape {a.shape}")
        check(lib().fus_model_set_source_weights(self.h, ptr(a), C.c_int(_abi.FUS_HOST)))

    def set_source_signals(self, signals, ds: float, t_first: float = 0.0, channel=None, amplitude=None, delay=None):
        """Drive the source with sampled signals: ``signals`` [nchan, nsamp] (or [nsamp]) holds samples at the times
        ``t_first + j * ds``, ``channel`` [ndofs] names the row each DOF plays (-1: silent; ``None`` with one channel:
        that channel everywhere), interpolated with the C1 cubic of :func:`fenicsxfus_amd.source.signal_value`; DOF d
        with a source weight emits ``amplitude[d] * S(t - delay[d])``.  The signal stands in for the whole default
        waveform (``source.waveform(..., scale=)`` produces such samples).  :meth:`clear_source` leaves this mode."""
        s = np.ascontiguousarray(np.atleast_2d(np.asarray(signals, dtype=np.float64)))
        if s.ndim != 2:
            raise _abi.FusError(f"set_source_signals: signals must be [nchan, nsamp], got shape {s.shape}")
        nchan, nsamp = s.shape
        if channel is None:
            if nchan != 1:
                raise _abi.FusError("set_source_signals: channel=None needs exactly one channel")
            ch = None
        else:
            ch = np.ascontiguousarray(np.asarray(channel), dtype=np.int32)
            if ch.shape != (self.data.ndofs,):
                raise _abi.FusError(f"set_source_signals: expected {self.data.ndofs} channels, one per DOF, got shape {ch.shape}")
        a, d = (None if x is None else np.ascontiguousarray(_array(x), dtype=self.data.dtype) for x in (amplitude, delay))
        for x in (a, d):
            if x is not None and x.shape != (self.data.ndofs,):
                raise _abi.FusError(f"set_source_signals: expected {self.data.ndofs} values, one per DOF, got shape {x.shape}")
        check(lib().fus_model_set_source_signals(self.h, C.c_int64(nchan), C.c_int64(nsamp), C.c_double(t_first),
                                                 C.c_double(ds), ptr(s), ptr(ch), ptr(a), ptr(d), C.c_int(_abi.FUS_HOST)))

    # ---- relaxation absorption: power-law tissue absorption (fusmi.h; fits: fenicsxfus_amd.absorption) ----
    def set_relaxation(self, freqs_hz, strength):
        """Add ``R = len(freqs_hz)`` (at most 4) relaxation processes with the relaxation frequencies ``freqs_hz`` (Hz)
        and the strengths ``strength`` (1/s): [R] for a homogeneous medium, or [R, ncells] per cell (a CellFunction row
        each).  :func:`fenicsxfus_amd.absorption.fit_power_law` yields both for alpha = alpha0 f^y.  ``c0`` is then
        the high-frequency sound speed.  The memory variables start from 0; u and v are kept.  Several ranks: collective
        under RCCL; the members of an in-process group call :func:`group_relaxation_finish` afterwards."""
        f = np.ascontiguousarray(np.atleast_1d(np.asarray(freqs_hz, dtype=np.float64)))
        nc = self.mesh.num_cells
        try:
            a = np.array([np.broadcast_to(np.asarray(_array(row), dtype=np.float64), (nc,)) for row in strength])
        except (TypeError, ValueError) as e:
            raise _abi.FusError(f"set_relaxation: every process takes one strength or {nc} (one per cell): {e}") from None
        if f.ndim != 1 or a.shape != (len(f), nc):
            raise _abi.FusError(f"set_relaxation: {len(f)} frequencies but strengths of shape {a.shape}")
        a = np.ascontiguousarray(a, dtype=self.data.dtype)
        w = np.ascontiguousarray(2.0 * np.pi * f)
        check(lib().fus_model_set_relaxation(self.h, C.c_int(len(f)), ptr(w), ptr(a)))

    def clear_relaxation(self):
        """Relaxation off: the planes are freed, a step enqueues what it did before."""
        check(lib().fus_model_set_relaxation(self.h, C.c_int(0), None, None))

    def relaxation_state(self, nu: int):
        """The memory variable z_nu as an array over the model's DOFs (checkpoints, tests)."""
        z = np.zeros(self.data.ndofs, dtype=self.data.dtype)
        check(lib().fus_model_relaxation_get(self.h, C.c_int(nu), ptr(z), C.c_int(_abi.FUS_HOST)))
        return z

    def set_relaxation_state(self, nu: int, z):
        z = np.ascontiguousarray(_array(z), dtype=self.data.dtype)
        if z.shape != (self.data.ndofs,):
            raise _abi.FusError(f"set_relaxation_state: expected {self.data.ndofs} values, one per DOF, got shape {z.shape}")
        check(lib().fus_model_relaxation_set(self.h, C.c_int(nu), ptr(z), C.c_int(_abi.FUS_HOST)))

    def relaxation_strength(self, nu: int):
        """The per-DOF strength A_nu as the sub-step reads it (diagnostics, tests)."""
        a = np.zeros(self.data.ndofs, dtype=self.data.dtype)
        check(lib().fus_model_relaxation_strength(self.h, C.c_int(nu), ptr(a), C.c_int(_abi.FUS_HOST)))
        return a

    def relaxation_apply(self, h: float):
        """One relaxation sub-step of length ``h`` on the resident state (the stepping entries run two of dt / 2 per step)."""
        check(lib().fus_model_relaxation_apply(self.h, C.c_double(h)))

    # ---- absorbing layers: a split-step sponge (fusmi.h; profiles: fenicsxfus_amd.sponge) ----
    def set_sponge(self, sigma):
        """Damp u, v (and the relaxation memory variables) at the rate ``sigma`` (1/s) per DOF, zero outside the layers:
        an array or Function over the model's space, e.g. from :func:`fenicsxfus_amd.sponge.layer_sigma`.  Keep tag 2
        on the faces behind the layers.  u, v and z are kept; an all-zero ``sigma`` is :meth:`clear_sponge`.  Several
        ranks: the sharers of a DOF must pass the same value (a profile computed from coordinates does); no finish call."""
        s = np.ascontiguousarray(_array(sigma), dtype=self.data.dtype)
        if s.shape != (self.data.ndofs,):
            raise _abi.FusError(f"set_sponge: expected {self.data.ndofs} values, one per DOF, got shape {s.shape}")
        check(lib().fus_model_set_sponge(self.h, ptr(s), C.c_int(_abi.FUS_HOST)))

    def clear_sponge(self):
        """Sponge off: the plane and the tile list are freed, a step enqueues what it did before."""
        check(lib().fus_model_set_sponge(self.h, None, C.c_int(_abi.FUS_HOST)))

    def sponge(self):
        """The damping rate in force as an array over the model's DOFs."""
        s = np.zeros(self.data.ndofs, dtype=self.data.dtype)
        check(lib().fus_model_sponge_get(self.h, ptr(s), C.c_int(_abi.FUS_HOST)))
        return s

    def sponge_apply(self, h: float):
        """One sponge sub-step of length ``h`` on the resident state (the stepping entries run two of dt / 2 per step)."""
        check(lib().fus_model_sponge_apply(self.h, C.c_double(h)))

    def sponge_info(self):
        """(DOFs with sigma > 0, tiles the sub-step kernel visits, tiles of the whole internal vector)."""
        nd, na, nt = C.c_int64(), C.c_int64(), C.c_int64()
        check(lib().fus_model_sponge_info(self.h, C.byref(nd), C.byref(na), C.byref(nt)))
        return nd.value, na.value, nt.value

    def u_sol(self):
        self._pull()
        return self.u_n

    def number_of_dofs(self):
        return self.V.dofmap.index_map.size_global

    def mass_vector(self):
        out = np.empty(self.data.ndofs, dtype=self.data.dtype)
        check(lib().fus_model_get_mass(self.h, ptr(out)))
        return out

    def close(self):
        """Frees the model and the operator data it created (G, dofmaps, partial slab)."""
        if self.h:
            lib().fus_model_destroy(self.h)
            self.h = C.c_void_p()
        self.data.close()


class LinearSpectralExplicit(_SpectralExplicit):
    """``LinearSpectralExplicit(mesh, meshtags, k, c0, rho0, freq0, p0, s0, rk_order, dt)``
    (_linear.py:267).  ``meshtags`` carries boundary facets as (cell, local facet) pairs with
    ``values`` 1 = source, 2 = absorbing (what ``compute_integration_domains`` yields for the
    tagged facets, Linear.hpp:113-118)."""

    _kind = _abi.FUS_LINEAR

    def __init__(self, mesh, meshtags, k, c0, rho0, freq0, p0, s0, rk_order=4, dt=None, V=None,
                 ctx: Context | None = None):
        self._create(mesh, meshtags, k, c0, rho0, None, freq0, p0, s0, rk_order, dt, V, ctx)


class LossySpectralExplicit(_SpectralExplicit):
    """``LossySpectralExplicit(mesh, meshtags, k, c0, rho0, delta0, freq0, p0, s0, rk_order, dt)``
    (python/src/fenicsxfus/_lossy.py:21-23; C++ ``LossySpectral3D``, Lossy.hpp:56-62).
    ``delta0`` = diffusivity of sound (DG0).  The reference has two variants of the boundary forms:
    ``forms="cpp"`` (default) is the C++ one -- absorbing and delta-mass terms on every listed
    boundary facet (BM7-SC1/forms.py:37-42) and the source doubled (Lossy.hpp:216-220);
    ``forms="python"`` is the Python package's -- those terms on tag 2 only, source not doubled
    (_lossy.py:107-128, :186-189)."""

    _kind = _abi.FUS_LOSSY

    def __init__(self, mesh, meshtags, k, c0, rho0, delta0, freq0, p0, s0, rk_order=4, dt=None, V=None,
                 ctx: Context | None = None, forms="cpp"):
        self._create(mesh, meshtags, k, c0, rho0, delta0, freq0, p0, s0, rk_order, dt, V, ctx, forms=forms)


class WesterveltSpectralExplicit(_SpectralExplicit):
    """``WesterveltSpectralExplicit(mesh, meshtags, k, c0, rho0, delta0, beta0, freq0, p0, s0,
    rk_order, dt)`` (python/src/fenicsxfus/_westervelt.py:21-23; C++ ``WesterveltSpectral3D``,
    Westervelt.hpp:58-67).  ``beta0`` = coefficient of nonlinearity (DG0); ``forms`` as in
    :class:`LossySpectralExplicit` (_westervelt.py:107-142, :215)."""

    _kind = _abi.FUS_WESTERVELT

    def __init__(self, mesh, meshtags, k, c0, rho0, delta0, beta0, freq0, p0, s0, rk_order=4, dt=None, V=None,
                 ctx: Context | None = None, forms="cpp"):
        self._create(mesh, meshtags, k, c0, rho0, delta0, freq0, p0, s0, rk_order, dt, V, ctx, beta0=beta0,
                     forms=forms)


def compute_diffusivity_of_sound(w0: float, c0: float, alpha: float) -> float:
    """delta = 2 alpha c0^3 / w0^2 with alpha in Np/m (the C++ helper, Lossy.hpp:375-379).  The
    Python package's helper of the same name takes dB/m: :func:`fenicsxfus_amd.utils.compute_diffusivity_of_sound`."""
    return 2 * alpha * c0**3 / w0**2


def group_finish_setup(models):
    """In-process transport: add the sharers' parts of the mass / boundary vectors (tests)."""
    arr = (C.c_void_p * len(models))(*[m.h for m in models])
    check(lib().fus_group_finish_setup(arr, C.c_int(len(models))))


def group_rk4_steps(models, t0: float, dt: float, nsteps: int):
    """In-process transport: advance all slab models in lock-step (tests)."""
    arr = (C.c_void_p * len(models))(*[m.h for m in models])
    check(lib().fus_group_rk4_steps(arr, C.c_int(len(models)), C.c_double(t0), C.c_double(dt), C.c_int64(nsteps)))


def group_relaxation_finish(models):
    """In-process transport: after every member's set_relaxation, add the sharers' parts of the relaxation strengths."""
    arr = (C.c_void_p * len(models))(*[m.h for m in models])
    check(lib().fus_group_relaxation_finish(arr, C.c_int(len(models))))
