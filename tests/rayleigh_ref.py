"""numpy restatement of the Rayleigh-integral kernel's documented arithmetic (fusmi.h "transducers", csrc/rayleigh.hip) and
the closed forms it is checked against.  ``dtype`` float64 is the yardstick, longdouble the reference; ``mixed`` emulates
the float stage of FUS_RAY_MIXED with correctly rounded float functions."""
import numpy as np


def _pi(dtype):
    return dtype(4) * np.arctan(dtype(1))


def rayleigh(points, q, targets, f, c, rho, alpha=0.0, dtype=np.float64, mixed=False):
    """(P [ntgt], gradP [ntgt, 3], rmin [ntgt]) of the surface ``points`` with complex volume velocities ``q``:
    d, r2, r in ``dtype``; the phase in revolutions t = r (f / c), u = t - rint(t); then sincospi(2 u), 1 / r, exp(-alpha r)
    and the products in ``dtype`` -- or, ``mixed``, in float32 from u, r, alpha r, q, d, k, alpha rounded to float32 -- the
    sums over the sources in ``dtype``, the factor -i f rho last.  A pair with r == 0 contributes nothing."""
    D = np.dtype(dtype).type
    xs, xt = np.asarray(points, dtype=np.float64).astype(D), np.asarray(targets, dtype=np.float64).astype(D)
    qc = np.asarray(q, dtype=np.complex128)
    d = xt[:, None, :] - xs[None, :, :]                    # [ntgt, nsrc, 3]
    r = np.sqrt((d * d).sum(axis=2))
    live = r > 0
    rs = np.where(live, r, D(1))
    rev = rs * (D(f) / D(c))
    u = rev - np.rint(rev)
    k = D(2) * _pi(D) * D(f) / D(c)
    if mixed:
        F = np.float32
        u32, r32, ar32 = u.astype(F), rs.astype(F), (D(alpha) * rs).astype(F)
        ang = np.float64(2.0 * np.pi) * u32.astype(np.float64)
        s, co = np.sin(ang).astype(F), np.cos(ang).astype(F)
        inv = F(1) / r32
        a = inv * np.exp(-ar32.astype(np.float64)).astype(F) if alpha != 0 else inv
        e_re, e_im = a * co, a * s
        q_re, q_im = qc.real.astype(F)[None, :], qc.imag.astype(F)[None, :]
        w_re, w_im = q_re * e_re - q_im * e_im, q_re * e_im + q_im * e_re
        cr, kk = -F(alpha) - inv, F(k)
        v_re, v_im = cr * w_re - kk * w_im, cr * w_im + kk * w_re
        n = d.astype(F) * inv[:, :, None]
        g_re, g_im = v_re[:, :, None] * n, v_im[:, :, None] * n
    else:
        ang = D(2) * _pi(D) * u
        s, co = np.sin(ang), np.cos(ang)
        inv = D(1) / rs
        a = inv * np.exp(-(D(alpha) * rs)) if alpha != 0 else inv
        e_re, e_im = a * co, a * s
        q_re, q_im = qc.real.astype(D)[None, :], qc.imag.astype(D)[None, :]
        w_re, w_im = q_re * e_re - q_im * e_im, q_re * e_im + q_im * e_re
        cr = -D(alpha) - inv
        v_re, v_im = cr * w_re - k * w_im, cr * w_im + k * w_re
        n = d * inv[:, :, None]
        g_re, g_im = v_re[:, :, None] * n, v_im[:, :, None] * n
    m, m3 = live.astype(D), live.astype(D)[:, :, None]
    S_re, S_im = (w_re.astype(D) * m).sum(axis=1), (w_im.astype(D) * m).sum(axis=1)
    G_re, G_im = (g_re.astype(D) * m3).sum(axis=1), (g_im.astype(D) * m3).sum(axis=1)
    K = D(f) * D(rho)
    # -i K (a + i b) = K (b - i a); kept as (re, im) pairs: numpy has no long-double complex arithmetic worth trusting
    return (K * S_im, -K * S_re), (K * G_im, -K * G_re), r.min(axis=1)


def as_complex(pair):
    return np.asarray(pair[0], dtype=np.float64) + 1j * np.asarray(pair[1], dtype=np.float64)


def planes(pair):
    """The (re, im) pair of one output group as one real vector (what the error measure runs over)."""
    return np.concatenate([np.ravel(pair[0]), np.ravel(pair[1])])


def oneil_axis(z, R, a, f, c, rho, v0):
    """|P| on the axis of a uniformly driven bowl (radius of curvature R, aperture radius a) at the distance z from the
    apex: rho c v0 |2 sin(k (B - z) / 2)| / |1 - z / R|, B = sqrt((z - h)^2 + a^2), h = R - sqrt(R^2 - a^2)."""
    z = np.asarray(z, dtype=np.float64)
    k = 2.0 * np.pi * f / c
    h = R - np.sqrt(R * R - a * a)
    B = np.sqrt((z - h) ** 2 + a * a)
    at_focus = np.abs(z - R) < 1e-12 * R            # 0 / 0 there: the limit is the focus value
    den = np.where(at_focus, 1.0, np.abs(1.0 - z / R))
    val = rho * c * v0 * np.abs(2.0 * np.sin(0.5 * k * (B - z))) / den
    return np.where(at_focus, bowl_focus(R, a, f, c, rho, v0), val)


def bowl_focus(R, a, f, c, rho, v0):
    """|P| at the geometric focus: rho c v0 k h."""
    return rho * c * v0 * (2.0 * np.pi * f / c) * (R - np.sqrt(R * R - a * a))


def piston_axis(z, a, f, c, rho, v0):
    """|P| on the axis of a piston of radius a: 2 rho c v0 |sin(k (sqrt(z^2 + a^2) - z) / 2)|."""
    z = np.asarray(z, dtype=np.float64)
    k = 2.0 * np.pi * f / c
    return 2.0 * rho * c * v0 * np.abs(np.sin(0.5 * k * (np.sqrt(z * z + a * a) - z)))
