"""Reference of the relaxation-absorption tests (test_relaxation_host.py, test_gpu_relaxation.py), numpy.

Model (fusmi.h, "relaxation absorption"): R processes with angular relaxation frequencies w_nu and per-cell strengths
a_nu; per DOF A_nu = (M(a_nu/(rho c^2)) 1) / (M(1/(rho c^2)) 1) with the oracle's mass action (``lumped_strengths``).
``substep`` is the trapezoidal sub-step in closed form, ``stepper`` the Strang-split run: half a sub-step, one RK step
of source_ref.rk_stepper (Westervelt: volume_source_ref.rk_stepper with westervelt_vectors), half a sub-step."""
import numpy as np

import source_ref as sr
import volume_source_ref as vr


def lumped_strengths(pr, a_cells, c, rho):
    """A [R, ndofs] from the per-cell strengths a_cells [R, ncells]."""
    one = np.ones(pr.ndofs)
    mc = 1.0 / (np.asarray(rho, np.float64) * np.asarray(c, np.float64) ** 2)
    den = pr.M(one, mc)
    return np.stack([pr.M(one, np.asarray(a, np.float64) * mc) / den for a in a_cells])


def coefficients(omega, h, dtype=np.float64):
    """(p, e, g) of the sub-step of length h: formed in double, rounded once to ``dtype``."""
    hw = h * np.asarray(omega, np.float64)
    d = 1.0 + 0.5 * hw
    return tuple(np.asarray(x, dtype=dtype) for x in ((1.0 - 0.5 * hw) / d, (0.5 * h) / d, hw / d))


def substep(v, z, A, omega, h, dtype=np.float64, coef_dtype=None):
    """One sub-step: returns (v+, z+ [R, n]).  The arithmetic runs in ``dtype`` in the kernel's order (ascending nu);
    ``coef_dtype`` (default ``dtype``) is the type p, e, g are rounded to before that -- the long-double evaluation of a
    float kernel takes the float-rounded coefficients."""
    p, e, g = (x.astype(dtype) for x in coefficients(omega, h, coef_dtype or dtype))
    v, z, A = np.asarray(v, dtype), np.asarray(z, dtype), np.asarray(A, dtype)
    one = dtype(1)
    s, r = A[0] * e[0], (A[0] * g[0]) * z[0]
    for k in range(1, len(p)):
        s = s + A[k] * e[k]
        r = r + (A[k] * g[k]) * z[k]
    vp = ((one - s) * v + r) / (one + s)
    vs = v + vp
    return vp, np.stack([p[k] * z[k] + e[k] * vs for k in range(len(p))])


def energy(v, z, A, omega):
    """E = v^2/2 + sum_nu A_nu w_nu z_nu^2 / 2 per DOF, in long double."""
    v, z, A = (np.asarray(x, np.longdouble) for x in (v, z, A))
    w = np.asarray(omega, np.longdouble)[:, None]
    return 0.5 * v * v + 0.5 * (A * w * z * z).sum(axis=0)


def stepper(cs, kind, forms, A, omega, p0, t0, dt, nsteps, order=4, on_step=None, vectors=None):
    """``nsteps`` Strang-split steps from rest with the default source; returns (u, v, z [R, ndofs]).  ``vectors``:
    (vec, scale) instead of the case's; ``on_step(s, u, v, z)`` after step s."""
    pr = cs.pr
    if vectors is not None:
        vec, scale = vectors
    elif kind == "westervelt":
        vec, scale = vr.westervelt_vectors(cs, forms)
    else:
        vec, scale = cs.vectors(kind, forms)
    u, v, z = np.zeros(pr.ndofs), np.zeros(pr.ndofs), np.zeros((len(omega), pr.ndofs))
    g, dg = vr.analytic(cs.f0, p0, scale)
    t = t0
    relax = (lambda v, z: substep(v, z, A, omega, 0.5 * dt)) if len(omega) else (lambda v, z: (v, z))
    for s in range(nsteps):
        v, z = relax(v, z)
        if kind == "westervelt":
            u, v = vr.rk_stepper(pr, vec, vec["src"], g, dg, t, dt, 1, order, u=u, v=v)
        else:
            u, v = sr.rk_stepper(pr, vec, scale, cs.f0, p0, t, dt, 1, order=order, u=u, v=v)
        v, z = relax(v, z)
        t += dt
        if on_step is not None:
            on_step(s + 1, u, v, z)
    return u, v, z


# ---- physics: the absorption the model imposes on a plane wave --------------------------------------------------------
# A bar of ncells x 1 x 1 cells at p = 4 (cell edge a quarter wavelength at 0.5 MHz with 32 cells, at 1 MHz with 64),
# c = 1500, rho = 1000: source on x = 0, absorbing on x = L, natural side walls -- a plane wave.  Two processes at 0.25
# and 4 MHz fitted to f^1.1 and scaled so that the exact alpha(0.5 MHz) L is about 1.
BAR_C, BAR_RHO, BAR_L, BAR_P, BAR_P0 = 1500.0, 1000.0, 0.024, 4, 6e4


class Bar:
    def __init__(self, orc, ncells, f0):
        import fenicsxfus_amd as fa
        from fenicsxfus_amd import absorption as ab, monitor as fmon
        from util import Problem

        h = BAR_L / ncells
        self.f0, self.P = f0, BAR_P
        self.pr = pr = Problem(orc, (ncells, 1, 1), BAR_P, hi=[BAR_L, h, h])
        cells, lf, ax, sd = pr.mesh.exterior_facets()
        sel = ax == 0
        self.tags = fa.FacetTags(cells[sel], lf[sel], np.where(sd[sel] == 0, 1, 2))
        nc = pr.mesh.num_cells
        self.c, self.rho = np.full(nc, BAR_C), np.full(nc, BAR_RHO)
        self.freqs, a, _ = ab.fit_power_law(5.0, 1.1, 0.25e6, 4e6, BAR_C, 2)
        self.strength = a / (ab.relaxation_alpha(0.5e6, self.freqs, a, BAR_C) * BAR_L)
        self.omega = 2 * np.pi * self.freqs
        self.alpha_exact = float(ab.relaxation_alpha(f0, self.freqs, self.strength, BAR_C))
        lam = BAR_C / f0
        t_end = 4.0 / f0 + 2.0 * BAR_L / BAR_C + 2.0 / f0      # ramp + two transits, then the two monitored periods
        self.dt, self.nsteps, self.skip, self.spp = fmon.whole_period_window(f0, 0.5 * h / (BAR_C * BAR_P**2), t_end, 2, nharm=1)
        self.x = pr.V.tabulate_dof_coordinates()[:, 0]
        self.fit = np.flatnonzero((self.x >= 2 * lam * (1 - 1e-12)) & (self.x <= 6 * lam * (1 + 1e-12)))
        m, src, absb, lin = pr.linear_model_vectors(self.c, self.rho, self.tags)
        self.vec = dict(m=m, src=src, absb=absb, lin=lin)

    def alpha_from(self, cos1, sin1):
        """minus the least-squares slope of ln |amplitude of the first harmonic| over the DOFs in [2, 6] wavelengths"""
        amp = np.hypot(np.asarray(cos1, np.float64), np.asarray(sin1, np.float64))[self.fit]
        return float(-np.polyfit(self.x[self.fit], np.log(amp), 1)[0])

    def cpu_alpha(self):
        """The identical run through ``stepper``; the harmonic sums as the monitor forms them."""
        A = np.repeat(self.strength[:, None], self.pr.ndofs, axis=1)    # homogeneous: A_nu = a_nu at every DOF
        acc = np.zeros((2, self.pr.ndofs))
        w = 2 * np.pi * self.f0

        def on_step(s, u, v, z):
            if s > self.skip:
                acc[0] += u * np.cos(w * s * self.dt)
                acc[1] += u * np.sin(w * s * self.dt)
        stepper(self, "linear", 0, A, self.omega, BAR_P0, 0.0, self.dt, self.nsteps, on_step=on_step, vectors=(self.vec, 1.0))
        return self.alpha_from(acc[0], acc[1])
