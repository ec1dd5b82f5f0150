"""Reference of the perfusion-response and damage tests (fusmi.h "bioheat", perfusion response and damage), in numpy on
thermal_ref.Bioheat and sts_ref.py:

    P(T)   piecewise linear through the knots, constant outside;  S(D)  the linear shutdown between dose_lo and dose_hi
    phi = P(T_n) S(D_n)  from the state a step STARTS from, held through its stages:  m_Weff = m_W phi
    Omega += (dt / 2) (r(T_old) + r(T_new)),  r(T) = exp(log A - Ea / (R (T + 273.15)))

with its own statement of the laws (a loop over the segments, not the library's select chain nor thermal.py's
searchsorted), the stepper of both schemes with the dose rule each of them uses, and the power iteration with
phi_max m_W.  test_response_host.py pins it to closed forms before anything on the device is compared with it."""
import numpy as np

import sts_ref
from thermal_ref import Bioheat, cem43_step

R_GAS = 8.314462618
HENRIQUES = dict(A=3.1e98, Ea=6.28e5)            # Henriques' constants for skin, 1/s and J/mol
HOT_W = 4e5                                      # tissue perfusion of the response tests, W/m^3/K
KNOTS = ((37.0, 41.0, 45.0), (1.0, 4.0, 4.0))    # a four-fold rise over 4 K that then saturates


def hot_materials(mesh, hi):
    """thermal_ref.materials with the tissue perfusion raised to HOT_W, so that the response shows within 20 steps."""
    from thermal_ref import materials
    k, rho_c, w = materials(mesh, hi)
    return k, rho_c, np.where(w > 0, HOT_W, 0.0)


class Response:
    """One response law: knots (temps, factors) and the dose range (dose_hi <= 0: no shutdown)."""

    def __init__(self, temps=(), factors=(), dose_lo=0.0, dose_hi=0.0):
        self.temps, self.factors = np.asarray(temps, dtype=np.float64), np.asarray(factors, dtype=np.float64)
        self.dose_lo, self.dose_hi = float(dose_lo), float(dose_hi)
        assert len(self.temps) == len(self.factors) <= 8

    @property
    def phi_max(self):
        return float(self.factors.max()) if len(self.factors) else 1.0

    def P(self, T):
        T = np.asarray(T, dtype=np.float64)
        t, f = self.temps, self.factors
        if not len(t):
            return np.ones_like(T)
        out = np.full(T.shape, np.nan)
        out[T <= t[0]] = f[0]
        out[T >= t[-1]] = f[-1]
        for j in range(len(t) - 1):
            m = (T > t[0]) & (T >= t[j]) & (T < t[j + 1])
            out[m] = f[j] + (f[j + 1] - f[j]) * ((T[m] - t[j]) / (t[j + 1] - t[j]))
        return out

    def S(self, D):
        D = np.asarray(D, dtype=np.float64)
        out = np.ones_like(D)
        if self.dose_hi > 0:
            mid = (D > self.dose_lo) & (D < self.dose_hi)
            out[mid] = (self.dose_hi - D[mid]) / (self.dose_hi - self.dose_lo)
            out[(D >= self.dose_hi) & (D > self.dose_lo)] = 0.0
        return out

    def phi(self, T, D):
        return self.P(T) * self.S(D)


def rate(T, A, Ea):
    """r(T) in 1/s, every operation rounded by itself in the order fusmi.h states it."""
    T = np.asarray(T, dtype=np.float64)
    return np.exp(np.log(A) - Ea / (R_GAS * (T + 273.15)))


def damage_add(omega, th_old, th_new, dt, t_base, A, Ea):
    """One application of the damage rule."""
    ro, rn = rate(t_base + np.asarray(th_old, np.float64), A, Ea), rate(t_base + np.asarray(th_new, np.float64), A, Ea)
    return omega + (dt / 2.0) * (ro + rn)


def damage(states, dt, t_base, A, Ea):
    """``states``: the start state and the state after every step."""
    om = np.zeros(len(states[0]))
    for old, new in zip(states[:-1], states[1:]):
        om = damage_add(om, old, new, dt, t_base, A, Ea)
    return om


class BioheatResponse(Bioheat):
    """thermal_ref.Bioheat whose perfusion follows ``response``: ``step`` freezes m_Weff = m_W phi(theta_n, D_n) from the
    state it starts from (the dose it keeps in ``self.D``) and then runs the parent's stages on it; ``sts_step`` does the
    same for RKL2.  Both advance the dose by their scheme's rule (rectangle / trapezoid) and, with ``damage=(A, Ea)``,
    Omega by the trapezoid rule."""

    def __init__(self, pr, k, rho_c, w=None, t_base=37.0, response=None, damage=None):
        super().__init__(pr, k, rho_c, w)
        self.m_w0 = self.m_w.copy()
        self.t_base, self.response, self.dmg = float(t_base), response, damage
        self.reset()

    def reset(self, D=None):
        self.D = np.zeros(self.pr.ndofs) if D is None else np.array(D, dtype=np.float64)
        self.omega = np.zeros(self.pr.ndofs)
        self.m_w = self.m_w0.copy()

    def m_weff(self, theta, D):
        """m_W phi in the model's scalar type, phi in double from (t_base + theta, D)."""
        if self.response is None:
            return self.m_w0.copy()
        phi = self.response.phi(self.t_base + np.asarray(theta, dtype=np.float64), D)
        return (self.m_w0.astype(np.float64) * phi).astype(self.pr.dtype)

    def _after(self, old, new, dt):
        if self.dmg is not None:
            self.omega = damage_add(self.omega, old, new, dt, self.t_base, *self.dmg)

    def step(self, theta, dt, h=None, sigma=1.0):
        self.m_w = self.m_weff(theta, self.D)
        new = super().step(theta, dt, h, sigma)
        self.D = cem43_step(self.D, new, dt, self.t_base)
        self._after(theta, new, dt)
        return new

    def sts_step(self, theta, dt, s, h=None, sigma=1.0):
        self.m_w = self.m_weff(theta, self.D)
        new = sts_ref.step(self, theta, dt, s, h, sigma)
        self.D = self.D + (dt / 120.0) * (sts_ref.dose_rate(theta, self.t_base) + sts_ref.dose_rate(new, self.t_base))
        self._after(theta, new, dt)
        return new

    def advance(self, theta0, dt, nsteps, h=None, sigma=1.0, stages=0, D0=None):
        """``nsteps`` steps of RK4 (``stages`` = 0) or RKL2 from (theta0, D0) with Omega = 0.  Returns the list of the
        states, the start included, and the list of the doses at those states; theta, D and Omega at the end are
        ``states[-1]``, ``doses[-1]`` and ``self.omega``."""
        self.reset(D0)
        th = self.vec(theta0)
        states, doses = [th.copy()], [self.D.copy()]
        for _ in range(nsteps):
            th = self.step(th, dt, h, sigma) if stages == 0 else self.sts_step(th, dt, stages, h, sigma)
            states.append(th.copy()), doses.append(self.D.copy())
        return states, doses

    def power_iteration(self, iters=20, x0=None):
        """The Rayleigh quotient of fus_thermal_lambda_max with a response set: m_W is replaced by phi_max m_W."""
        keep = self.m_w
        self.m_w = self.m_w0 * (1.0 if self.response is None else self.response.phi_max)
        try:
            return super().power_iteration(iters, x0)
        finally:
            self.m_w = keep
