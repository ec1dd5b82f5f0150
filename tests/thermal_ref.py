"""Reference of the bioheat tests (fusmi.h "bioheat"), in numpy on the oracle's operators (util.Problem.K / .M):

    m_C = M(rho C) 1,  m_W = M(W) 1,  h = (M(q_coef) 1) .* q
    dtheta/dt = f(theta) = (K(-k) theta - m_W .* theta + sigma h) ./ m_C

advanced by classical RK4 (a = 0, 1/2, 1/2, 1; b = 1/6, 1/3, 1/3, 1/6, as in source_ref.py), the CEM43 dose rule and
the power iteration behind the stable step, plus the materials, the heat field and the cases the tests share.  The model
runs in the scalar type of the Problem it is given: in double it is the reference, in float the yardstick of the fp32
budget tests (thermal_fp32_cases.py)."""
import functools

import numpy as np

from fp32_budget import promoted
from util import Problem

H_CELL = 0.003                      # 3 mm cells
BONE = dict(k=0.32, rho_c=1850.0 * 1300.0, w=0.0)
TISSUE = dict(k=0.52, rho_c=1040.0 * 3600.0, w=4e4)
A_RK = (0.0, 0.5, 0.5, 1.0)
B_RK = (1.0 / 6.0, 1.0 / 3.0, 1.0 / 3.0, 1.0 / 6.0)

# label -> cells, degree, perturbation, scalar type: the smallest shapes that reach each kernel family
CASES = {
    "A": dict(n=(4, 3, 3), P=3, perturb=0.1, dtype=np.float64),   # trilinear
    "B": dict(n=(6, 5), P=4, perturb=0.1, dtype=np.float64),      # quadrilaterals
    "C": dict(n=(4, 3, 3), P=2, perturb=0.0, dtype=np.float64),   # affine, diagonal metric
    "D": dict(n=(3, 2, 2), P=7, perturb=0.1, dtype=np.float64),   # index-1 contraction on the 4x4x4 MFMA
    "E": dict(n=(2, 2, 2), P=8, perturb=0.1, dtype=np.float64),   # two waves per element
    "F": dict(n=(4, 3, 3), P=4, perturb=0.1, dtype=np.float32),
}


def box_hi(n):
    return [H_CELL * k for k in n]


def materials(mesh, hi):
    """(k, rho_c, W) per cell: cells whose centroid x lies in (0.4, 0.6) of the box are bone, the rest tissue."""
    cx = mesh.cell_centroids()[:, 0] / hi[0]
    bone = (cx > 0.4) & (cx < 0.6)
    pick = lambda key: np.where(bone, BONE[key], TISSUE[key])   # noqa: E731
    return pick("k"), pick("rho_c"), pick("w")


def heat_field(V, hi):
    """q = 5e7 exp(-|x - centre|^2 / (2 (2 mm)^2)) at the DOFs."""
    X = V.tabulate_dof_coordinates()[:, :len(hi)].astype(np.float64)
    r2 = ((X - 0.5 * np.asarray(hi)) ** 2).sum(axis=1)
    return 5e7 * np.exp(-r2 / (2.0 * 0.002 ** 2))


def cem43_step(D, theta, dt, t_base):
    """One application of the dose rule, in the order fusmi.h states it."""
    T = t_base + np.asarray(theta, dtype=np.float64)
    c = np.where(T >= 43.0, 1.0, 2.0)
    return D + (dt / 60.0) * np.exp2(-(c * (43.0 - T)))


def dose(states, dt, t_base):
    D = np.zeros(len(states[0]))
    for x in states:
        D = cem43_step(D, x, dt, t_base)
    return D


class Bioheat:
    """The discrete Pennes model on a Problem ``pr`` with per-cell k, rho_c, W (arrays or scalars), in ``pr``'s scalar
    type T.  In double it is the reference.  In float it is the plain sequential restatement of what the library computes
    (the yardstick of fp32_budget.py): K and M are the float oracle's, every vector is float32, and every scalar is
    rounded where thermal.hip rounds it -- dt to T first and then times T(a), T(b) (thermal_rk4_end), sigma to T, and the
    stage multiplies by the stored vector 1 / m_C (k_reciprocal) where the double reference divides by m_C."""

    def __init__(self, pr, k, rho_c, w=None):
        nc = pr.mesh.num_cells
        self.T = pr.dtype.type
        self.exact = pr.dtype == np.float64
        full = lambda a: np.broadcast_to(np.asarray(a, dtype=pr.dtype), (nc,)).copy()   # noqa: E731
        self.pr, self.k, self.rho_c = pr, full(k), full(rho_c)
        self.w = full(0.0 if w is None else w)
        one = np.ones(pr.ndofs, pr.dtype)
        self.m_c = pr.M(one, self.rho_c)
        self.m_w = pr.M(one, self.w) if self.w.any() else np.zeros(pr.ndofs, pr.dtype)

    def vec(self, a):
        return np.array(a, dtype=self.pr.dtype)

    def load(self, q, coef=None):
        """h = (M(coef) 1) .* q"""
        one = np.ones(self.pr.ndofs, self.pr.dtype)
        return self.pr.M(one, None if coef is None else np.asarray(coef, dtype=self.pr.dtype)) * self.vec(q)

    def minv(self):
        """1 / m_C as the float stage kernels read it: a stored T vector."""
        return self.T(1) / self.m_c

    def b(self, theta):
        """K(-k) theta: the operator's part of a stage."""
        return self.pr.K(theta, -self.k)

    def f(self, theta, h=None, sigma=1.0):
        if not self.exact:
            hh = np.zeros_like(theta) if h is None else h
            assert theta.dtype == hh.dtype == self.pr.dtype
            return (self.b(theta) - self.m_w * theta + self.T(sigma) * hh) * self.minv()
        r = self.b(theta) - self.m_w * theta
        if h is not None and sigma != 0.0:
            r = r + sigma * h
        return r / self.m_c

    def finish_step(self, theta):
        """What a stepper does to the state after its last stage (the boundary reference's hook)."""
        return theta

    def step(self, theta, dt, h=None, sigma=1.0):
        acc, stage = theta.copy(), theta
        dt = self.T(dt)
        for i in range(4):
            ki = self.f(stage, h, sigma)
            acc = acc + dt * self.T(B_RK[i]) * ki
            if i < 3:
                stage = theta + dt * self.T(A_RK[i + 1]) * ki
        return self.finish_step(acc)

    def run(self, theta0, dt, nsteps, h=None, sigma=1.0, keep=False):
        """theta after ``nsteps`` steps; with ``keep`` the list of the states after every step."""
        th, states = self.vec(theta0), []
        for _ in range(nsteps):
            th = self.step(th, dt, h, sigma)
            if keep:
                states.append(th.copy())
        return states if keep else th

    def start_vector(self):
        return 1.0 + 0.5 * np.sin(37.0 * np.arange(self.pr.ndofs) + 1.0)

    def power_iteration(self, iters=20, x0=None):
        """The Rayleigh quotient of fus_thermal_lambda_max after ``iters`` iterations from its start vector."""
        x = self.start_vector() if x0 is None else np.array(x0, dtype=np.float64)
        rho = 0.0
        for _ in range(iters):
            y = (self.pr.K(x, self.k) + self.m_w * x) / self.m_c
            rho = (x @ (self.m_c * y)) / (x @ (self.m_c * x))
            x = y / np.sqrt(y @ (self.m_c * y))
        return float(rho)

    def dense_lambda_max(self):
        """Largest eigenvalue of the dense symmetric m_C^-1/2 (K(k) + m_W) m_C^-1/2, built column by column."""
        n = self.pr.ndofs
        A = np.empty((n, n))
        e = np.zeros(n)
        for j in range(n):
            e[j] = 1.0
            A[:, j] = self.pr.K(e, self.k)
            e[j] = 0.0
        A += np.diag(self.m_w)
        s = 1.0 / np.sqrt(self.m_c)
        A = s[:, None] * A * s[None, :]
        return float(np.linalg.eigvalsh(0.5 * (A + A.T))[-1])


class Case:
    """One of the cases A-F: the problem in its scalar type (``prt``, what the library gets), the double problem the
    reference runs on (for fp32: on the float-rounded coordinates), materials and heat rounded to the scalar type."""

    def __init__(self, orc, label):
        kw = CASES[label]
        self.label, self.n, self.P, self.dtype = label, kw["n"], kw["P"], np.dtype(kw["dtype"])
        self.hi = box_hi(self.n)
        self.prt = Problem(orc, self.n, self.P, hi=self.hi, perturb=kw["perturb"], dtype=self.dtype)
        self.pr = self.prt if self.dtype == np.float64 else promoted(orc, self.prt)
        rnd = lambda a: np.asarray(a).astype(self.dtype).astype(np.float64)   # noqa: E731
        self.k, self.rho_c, self.w = (rnd(a) for a in materials(self.prt.mesh, self.hi))
        self.q = rnd(heat_field(self.prt.V, self.hi))
        self.ref = Bioheat(self.pr, self.k, self.rho_c, self.w)
        self.h = self.ref.load(self.q)
        self.rho20 = self.ref.power_iteration(20)
        self.dt = 2.0 / self.rho20

    def model(self, fa, ctx, **kw):
        """The library's thermal object of this case, heat load set."""
        t = self.dtype
        th = fa.BioheatSpectralExplicit(self.prt.mesh, self.P, self.k.astype(t), self.rho_c.astype(t), self.w.astype(t),
                                        V=self.prt.V, ctx=ctx, **kw)
        th.set_heat(self.q.astype(t))
        return th


@functools.lru_cache(maxsize=None)
def case(orc, label) -> Case:
    return Case(orc, label)


def rel(a, ref):
    return float(np.abs(np.asarray(a, dtype=np.float64) - ref).max() / np.abs(ref).max())
