"""Reference and inputs for the phased / apodised source tests (test_source_host.py, test_gpu_source.py).

The oracle's steppers know only the uniform cosine source, so the reference of the model runs is ``rk_stepper``: a
numpy Runge-Kutta loop on ``Problem.K`` and the model vectors of tests/util.py, the source taken per DOF from
``fenicsxfus_amd.source.waveform``.  Right-hand sides (Linear.hpp:171-222, Lossy.hpp:231-245):
    Linear   f1 = (K(coef) u + src g(t) - absb v) / m
    Lossy    f1 = (K(lin) u + K(att) v + src g(t) + src2 dg(t) - absb v) / m
    Westervelt (vec["mn1"] = M(nlin1) 1, the diagonal of the nonlinear mass term; Westervelt.hpp:246-265):
             f1 = (the Lossy numerator - mn1 v^2) / (m + mn1 u)
Butcher tables as in wave.hip stage_scalars (_linear.py:286-311).  test_source_host.py pins it against the oracle's
steppers with the uniform source before anything on the device is compared with it."""
import numpy as np

import fenicsxfus_amd as fa
import fp32_budget as fb
from fenicsxfus_amd import source as fsrc
from util import Problem

S0 = 1500.0
NSTEPS = 20
STEPS_PER_PERIOD = 9     # the issue: a source period is 8-10 steps of the CFL dt

RK = {1: ([0.0], [1.0], [0.0]),
      2: ([0.0, 2 / 3], [1 / 4, 3 / 4], [0.0, 2 / 3]),
      3: ([0.0, 1 / 2, 3 / 4], [2 / 9, 1 / 3, 4 / 9], [0.0, 1 / 2, 3 / 4]),
      4: ([0.0, 0.5, 0.5, 1.0], [1 / 6, 1 / 3, 1 / 3, 1 / 6], [0.0, 0.5, 0.5, 1.0])}


class Case:
    """One mesh with its heterogeneous material, model vectors and a smooth aperture function over the source face."""

    def __init__(self, orc, n, P, perturb, source_axis=0, dtype=np.float64, spp=STEPS_PER_PERIOD, h=0.003):
        t = len(n)
        self.hi = [h * k for k in n]
        # fp32: the device gets the float problem, the reference runs in double on the same float-rounded coordinates
        self.pr_dev = Problem(orc, n, P, hi=self.hi, perturb=perturb, dtype=dtype)
        self.pr = pr = self.pr_dev if np.dtype(dtype) == np.float64 else fb.promoted(orc, self.pr_dev)
        self.n, self.P, self.tdim = n, P, t
        cx = pr.mesh.cell_centroids()[:, 0]
        sel = (cx > 0.4 * self.hi[0]) & (cx < 0.6 * self.hi[0])
        self.c, self.rho = np.where(sel, 2800.0, 1500.0), np.where(sel, 1850.0, 1000.0)
        self.dt = 0.5 * h / (self.c.max() * P**2)
        self.f0 = 1.0 / (spp * self.dt)
        w0 = 2 * np.pi * self.f0
        self.delta = np.where(sel, fa.compute_diffusivity_of_sound(w0, 2800.0, 400.0 / 20.0 * np.log(10.0)),
                              fa.compute_diffusivity_of_sound(w0, 1500.0, 0.2))
        self.beta = np.where(sel, 6.0, 3.5)
        self.tags = fa.tag_box_boundary(pr.mesh, source_axis=source_axis)
        self.source_axis = source_axis
        self.X = pr.V.tabulate_dof_coordinates()[:, :t].astype(np.float64)
        self.face = np.flatnonzero(pr.facet_diag(self.tags, 1, np.ones(pr.mesh.num_cells, pr.dtype)))

    def t0s(self):
        """Start times: onset, ramp end and (for the burst of duration D) burst end inside the 20 steps."""
        D = 10.0 / self.f0
        return {"onset": (0.0, 0.0), "ramp_end": (3.5 / self.f0, 0.0), "burst_end": (D - 1.0 / self.f0, D)}

    def aperture(self):
        """(amp, tau) over all DOFs (only the source face matters): amp smooth in [0, 1.5] with exact zeros towards
        the rim of the face, tau smooth in [0, 3 / f]."""
        ax = [a for a in range(self.tdim) if a != self.source_axis]
        xi = np.stack([self.X[:, a] / self.hi[a] - 0.5 for a in ax], axis=1)      # [-1/2, 1/2] over the face
        rho = 2.0 * np.linalg.norm(xi, axis=1)
        amp = 1.5 * np.maximum(0.0, 1.0 - (rho / 0.8) ** 2)
        phase = 2.3 * xi[:, 0] + (1.1 * xi[:, 1] if xi.shape[1] > 1 else 0.0)
        tau = (3.0 / self.f0) * (0.5 + 0.5 * np.sin(phase * 2.0))
        return amp, tau

    def vectors(self, kind, forms=0):
        """The model vectors as a dict (m, src, absb, lin [, att, src2]) and the source scale."""
        pr = self.pr
        if kind == "linear":
            m, src, absb, lin = pr.linear_model_vectors(self.c, self.rho, self.tags)
            return dict(m=m, src=src, absb=absb, lin=lin), 1.0
        c, rho, d = self.c, self.rho, self.delta
        if forms == 0:
            m, src, absb, src2, lin, att = pr.lossy_model_vectors(c, rho, d, self.tags)
            return dict(m=m, src=src, absb=absb, src2=src2, lin=lin, att=att), 2.0
        one = np.ones(pr.ndofs)
        m = pr.M(one, 1.0 / (rho * c * c)) + pr.facet_diag(self.tags, 2, d / (rho * c**3))   # _lossy.py:107-114
        return dict(m=m, src=pr.facet_diag(self.tags, 1, 1.0 / rho), absb=pr.facet_diag(self.tags, 2, 1.0 / (rho * c)),
                    src2=pr.facet_diag(self.tags, 1, d / (rho * c * c)), lin=-1.0 / rho, att=-d / (rho * c * c)), 1.0


def rk_stepper(pr, vec, scale, f0, p0, t0, dt, nsteps, amp=1.0, tau=0.0, duration=0.0, order=4, u=None, v=None,
               on_step=None):
    """``nsteps`` explicit RK steps of size dt from (u, v) (default: rest) at t0; returns (u, v).  float64 throughout.
    ``on_step(s, u, v)`` is called after step s = 1..nsteps."""
    a_r, b_r, c_r = RK[order]
    nd = pr.ndofs
    u0 = np.zeros(nd) if u is None else np.array(u, dtype=np.float64)
    v0 = np.zeros(nd) if v is None else np.array(v, dtype=np.float64)
    src, absb, m = (np.asarray(vec[k], dtype=np.float64) for k in ("src", "absb", "m"))
    src2, mn1 = vec.get("src2"), vec.get("mn1")
    t = t0
    for step in range(nsteps):
        ua, va = u0.copy(), v0.copy()
        ku, kv = np.zeros(nd), np.zeros(nd)
        for i in range(order):
            un, vn = u0 + dt * a_r[i] * ku, v0 + dt * a_r[i] * kv
            tn = t + c_r[i] * dt
            b = pr.K(un, vec["lin"]) + src * fsrc.waveform(tn, f0, p0, S0, amp, tau, duration, scale) - absb * vn
            if src2 is not None:
                b = b + pr.K(vn, vec["att"]) + src2 * fsrc.waveform(tn, f0, p0, S0, amp, tau, duration, scale,
                                                                    derivative=True)
            ku, kv = vn, (b / m if mn1 is None else (b - mn1 * vn * vn) / (m + mn1 * un))
            ua, va = ua + dt * b_r[i] * ku, va + dt * b_r[i] * kv
        u0, v0 = ua, va
        t += dt
        if on_step is not None:
            on_step(step + 1, u0, v0)
    return u0, v0


def rel(a, b):
    """max-norm of the difference over the max-norm of the reference."""
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max() / np.abs(b).max())


def case3d(orc, dtype=np.float64):
    return Case(orc, (4, 3, 3), 3, 0.1, dtype=dtype)


def case2d(orc, dtype=np.float64):
    return Case(orc, (6, 5), 4, 0.0, dtype=dtype)
