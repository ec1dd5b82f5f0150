"""Reference of the per-harmonic heat load (fusmi.h "per-harmonic heat load"; fus_thermal_set_heat_from_harmonics), in
numpy on the oracle's mass operator, and the synthetic signal the host test checks the definition on:

    h = sum_k M(2 alpha_k / (rho c)) 1 .* 0.5 (COS_k^2 + SIN_k^2)

with COS_k, SIN_k the monitor's maps of harmonic k (2 / n times its accumulators)."""
import numpy as np


def harmonic_heat(pr, alphas, rho, c, cos_maps, sin_maps):
    """``pr``: a util.Problem (double); ``alphas``: (K, ncells), row k - 1 = absorption of harmonic k in Np/m; ``rho``,
    ``c``: per cell; ``cos_maps``, ``sin_maps``: K maps each, per DOF.  Summed in ascending k."""
    alphas = np.atleast_2d(np.asarray(alphas, dtype=np.float64))
    assert len(cos_maps) == len(sin_maps) == len(alphas)
    one = np.ones(pr.ndofs)
    h = np.zeros(pr.ndofs)
    for a, ck, sk in zip(alphas, cos_maps, sin_maps):
        ck, sk = np.asarray(ck, dtype=np.float64), np.asarray(sk, dtype=np.float64)
        h = h + pr.M(one, 2.0 * a / (rho * c)) * (0.5 * (ck ** 2 + sk ** 2))
    return h


def synthetic_signal(rng, ndof, nharm=3, freq=0.5e6, periods=2, spp=9):
    """x_j = mu + sum_{k <= nharm} (A_k cos + B_k sin)(2 pi k f t_j) at ``periods * spp`` uniform times over whole
    periods (``spp`` samples per period, more than 2 nharm): returns (times, x[sample, dof], mu, A, B)."""
    assert spp > 2 * nharm
    mu = rng.standard_normal(ndof)
    A = [rng.standard_normal(ndof) / k for k in range(1, nharm + 1)]
    B = [rng.standard_normal(ndof) / k for k in range(1, nharm + 1)]
    t = (1.0 + np.arange(periods * spp)) / (spp * freq)
    x = mu + sum(A[k - 1] * np.cos(2 * np.pi * k * freq * t[:, None]) + B[k - 1] * np.sin(2 * np.pi * k * freq * t[:, None])
                 for k in range(1, nharm + 1))
    return t, x, mu, A, B


def accumulate(x, t, freq, nharm):
    """The monitor's accumulation rule over the samples x[j] at the times t[j], sequentially in double: returns
    (n, S, Q, C, S_k) with S the sum, Q the sum of squares, C[k - 1] = sum x cos(2 pi k f t), S_k likewise with sin."""
    S, Q = np.zeros(x.shape[1]), np.zeros(x.shape[1])
    Ck = [np.zeros(x.shape[1]) for _ in range(nharm)]
    Sk = [np.zeros(x.shape[1]) for _ in range(nharm)]
    for xj, tj in zip(x, t):
        S += xj
        Q += xj * xj
        for k in range(1, nharm + 1):
            Ck[k - 1] += xj * np.cos(2.0 * np.pi * k * freq * tj)
            Sk[k - 1] += xj * np.sin(2.0 * np.pi * k * freq * tj)
    return len(t), S, Q, Ck, Sk


def mean_squares(n, Ck, Sk):
    """a_k = (2 / n^2) (C_k^2 + S_k^2), as fusmi.h defines it."""
    return [2.0 / n ** 2 * (c ** 2 + s ** 2) for c, s in zip(Ck, Sk)]
