"""Reference of the super-time-stepping tests (fusmi.h "bioheat", fus_thermal_steps_sts), in numpy on thermal_ref.Bioheat:
the s-stage Runge-Kutta-Legendre scheme of second order (RKL2: Meyer, Balsara and Aslam, J. Comput. Phys. 257, 2014)

    b_0 = b_1 = b_2 = 1/3,   b_j = (j^2 + j - 2) / (2 j (j + 1)) for j >= 3,   a_j = 1 - b_j
    w1 = 4 / (s^2 + s - 2),  mut_1 = b_1 w1
    mu_j = (2j - 1)/j b_j / b_{j-1},  nu_j = -(j - 1)/j b_j / b_{j-2},  mut_j = mu_j w1,  gat_j = -a_{j-1} mut_j   (j = 2..s)
    Y_0 = theta,  F_0 = f(Y_0),  Y_1 = Y_0 + mut_1 dt F_0
    Y_j = mu_j Y_{j-1} + nu_j Y_{j-2} + (1 - mu_j - nu_j) Y_0 + mut_j dt f(Y_{j-1}) + gat_j dt F_0,   theta <- Y_s

with its own copy of the coefficient formulas, the scalar stability polynomial from the same recurrence, the stable
step and the trapezoid dose rule  D += (dt / 120) (R(T_old) + R(T_new)),  R(T) = exp2(-c (43 - T))."""
import numpy as np

S_MIN, S_MAX = 2, 32


def _b(j):
    j = float(j)
    return 1.0 / 3.0 if j < 3 else (j * j + j - 2.0) / (2.0 * j * (j + 1.0))


def coefficients(s):
    """(mu, nu, mut, gat): arrays of length s + 1 indexed by the stage j; entry 0 and mu, nu, gat of stage 1 are 0."""
    assert S_MIN <= s <= S_MAX
    sf = float(s)
    w1 = 4.0 / (sf * sf + sf - 2.0)
    mu, nu, mut, gat = np.zeros(s + 1), np.zeros(s + 1), np.zeros(s + 1), np.zeros(s + 1)
    mut[1] = _b(1) * w1
    for j in range(2, s + 1):
        jf = float(j)
        mu[j] = (2.0 * jf - 1.0) / jf * _b(j) / _b(j - 1)
        nu[j] = -((jf - 1.0) / jf) * _b(j) / _b(j - 2)
        mut[j] = mu[j] * w1
        gat[j] = -((1.0 - _b(j - 1)) * mut[j])
    return mu, nu, mut, gat


def beta(s):
    """The scheme is stable for dt lambda <= beta_s."""
    return (s * s + s - 2) / 2.0


def stable_dt(rho, s):
    """The library's rule: 0.72 beta_s / rho, rho the Rayleigh quotient of the power iteration."""
    return 0.72 * (s * s + s - 2) / (2.0 * rho)


def polynomial(s, z):
    """R(z) of the scalar problem y' = lambda y, z = dt lambda, from the recurrence itself."""
    mu, nu, mut, gat = coefficients(s)
    z = np.asarray(z, dtype=np.float64)
    y0 = np.ones_like(z)
    f0 = z * y0
    ym2, ym1 = y0, y0 + mut[1] * f0
    for j in range(2, s + 1):
        ym2, ym1 = ym1, mu[j] * ym1 + nu[j] * ym2 + (1.0 - mu[j] - nu[j]) * y0 + mut[j] * (z * ym1) + gat[j] * f0
    return ym1


def step(bio, theta, dt, s, h=None, sigma=1.0):
    """One RKL2 step of thermal_ref.Bioheat ``bio``, in its scalar type T.  In float the stage scalars are rounded as
    thermal_sts_end (thermal.hip) rounds them: mu_j, nu_j, 1 - mu_j - nu_j, mut_j dt and gat_j dt are each formed in
    double and rounded to T once; in double the rounding changes nothing."""
    mu, nu, mut, gat = coefficients(s)
    T = bio.T
    y0 = theta
    f0 = bio.f(y0, h, sigma)
    ym2, ym1 = y0, y0 + T(mut[1] * dt) * f0
    for j in range(2, s + 1):
        y = (T(mu[j]) * ym1 + T(nu[j]) * ym2 + T(1.0 - mu[j] - nu[j]) * y0 + T(mut[j] * dt) * bio.f(ym1, h, sigma)
             + T(gat[j] * dt) * f0)
        ym2, ym1 = ym1, y
    return bio.finish_step(ym1)


def run(bio, theta0, dt, nsteps, s, h=None, sigma=1.0, keep=False):
    """theta after ``nsteps`` steps; with ``keep`` the list of the states after every step."""
    th, states = bio.vec(theta0), []
    for _ in range(nsteps):
        th = step(bio, th, dt, s, h, sigma)
        if keep:
            states.append(th.copy())
    return states if keep else th


def dose_rate(theta, t_base):
    T = t_base + np.asarray(theta, dtype=np.float64)
    c = np.where(T >= 43.0, 1.0, 2.0)
    return np.exp2(-(c * (43.0 - T)))


def dose_trapezoid(states, dt, t_base):
    """``states``: the start state and the state after every step.  Every operation rounded by itself, in the order
    fusmi.h states it."""
    D = np.zeros(len(states[0]))
    for old, new in zip(states[:-1], states[1:]):
        D = D + (dt / 120.0) * (dose_rate(old, t_base) + dose_rate(new, t_base))
    return D
