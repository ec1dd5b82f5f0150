"""Host side of the transducer sources (fenicsxfus_amd.transducer): geometry helpers, the numpy reference of the Rayleigh
integral against the closed forms, the boundary drive, and the plane fit of ``set_transducer``.  No device."""
import numpy as np
import pytest

import fenicsxfus_amd as fa
from fenicsxfus_amd import source
from fenicsxfus_amd import transducer as td

import rayleigh_ref as rr

F, C0, RHO, V0 = 0.5e6, 1500.0, 1000.0, 1.0
R_BOWL, A_BOWL, A_PISTON = 0.064, 0.032, 0.010
Z_AXIS = np.linspace(0.020, 0.100, 81)          # includes the focus z = R


# ---- geometry -----------------------------------------------------------------------------------------------------------
def test_bowl_points_areas_normals():
    apex, focus = np.array([0.01, -0.02, 0.005]), np.array([0.03, 0.02, 0.05])
    R = np.linalg.norm(focus - apex)
    a = 0.45 * R
    p, dA, n = td.bowl(apex, focus, 2 * a, 1500)
    h = R - np.sqrt(R * R - a * a)
    assert p.shape == (1500, 3) and dA.shape == (1500,) and n.shape == (1500, 3)
    assert abs(dA.sum() - 2 * np.pi * R * h) <= 1e-14 * 2 * np.pi * R * h
    assert np.abs(np.linalg.norm(p - focus, axis=1) - R).max() <= 4e-16 * R * 8      # on the sphere, to rounding
    assert np.abs(p + R * n - focus).max() <= 1e-15 * R * 8                          # the normals pass through the focus
    assert np.abs(np.linalg.norm(n, axis=1) - 1).max() <= 1e-15
    height = (p - apex) @ ((focus - apex) / R)
    assert height.min() > 0 and height.max() < h                                     # inside the cap
    assert np.allclose(np.diff(height), h / 1500, rtol=1e-9)                         # equal-area rings


def test_disc_points_areas_normals():
    c, nv = np.array([0.0, 0.01, -0.01]), np.array([1.0, 2.0, -1.0])
    p, dA, n = td.disc(c, nv, 0.02, 777)
    assert abs(dA.sum() - np.pi * 0.01 ** 2) <= 1e-14 * np.pi * 0.01 ** 2
    e = nv / np.linalg.norm(nv)
    assert np.abs((p - c) @ e).max() <= 1e-17 and np.abs(n - e).max() <= 1e-16
    r = np.linalg.norm(p - c, axis=1)
    assert np.allclose(r, 0.01 * np.sqrt((np.arange(777) + 0.5) / 777), rtol=1e-12)


def test_inner_diameter_removes_exactly_the_inner_cap():
    R, a, ai = 0.05, 0.03, 0.012
    p, dA, _ = td.bowl([0, 0, 0], [0, 0, R], 2 * a, 400, inner_diameter=2 * ai)
    cap = lambda s: 2 * np.pi * R * (R - np.sqrt(R * R - s * s))  # noqa: E731
    assert abs(dA.sum() - (cap(a) - cap(ai))) <= 1e-13 * cap(a)
    rad = np.hypot(p[:, 0], p[:, 1])
    assert rad.min() > ai and rad.max() < a
    p, dA, _ = td.disc([0, 0, 0], [0, 0, 1], 2 * a, 400, inner_diameter=2 * ai)
    assert abs(dA.sum() - np.pi * (a * a - ai * ai)) <= 1e-13 * np.pi * a * a
    rad = np.hypot(p[:, 0], p[:, 1])
    assert rad.min() > ai and rad.max() < a


def test_points_needed_and_volume_velocity():
    lam = C0 / F
    area = 3.3e-3
    n = td.points_needed(area, F, C0)
    assert np.sqrt(area / n) <= lam / 2 < np.sqrt(area / (n - 1))
    assert td.points_needed(area, F, C0, per_wavelength=4.0) >= 4 * n - 4
    q = td.volume_velocity(np.full(3, 2e-6), v0=[1.0, 0.5, 2.0], phase=[0.0, np.pi / 2, np.pi])
    assert np.allclose(q, [2e-6, 1e-6j, -4e-6], atol=1e-20)


# ---- the float64 reference against the closed forms ---------------------------------------------------------------------
def _axis_field(points, areas, z, origin=(0.0, 0.0, 0.0)):
    T = np.asarray(origin) + np.stack([0 * z, 0 * z, z], axis=1)
    P, _, _ = rr.rayleigh(points, td.volume_velocity(areas, V0), T, F, C0, RHO)
    return np.abs(rr.as_complex(P))


def test_reference_meets_oneil_on_the_bowl_axis():
    p, dA, _ = td.bowl([0, 0, 0], [0, 0, R_BOWL], 2 * A_BOWL, 2000)
    ref = rr.oneil_axis(Z_AXIS, R_BOWL, A_BOWL, F, C0, RHO, V0)
    err = np.abs(_axis_field(p, dA, Z_AXIS) - ref).max() / ref.max()
    print(f"bowl axis: {err:.2e} of the peak")
    assert err <= 1e-5
    foc = _axis_field(p, dA, np.array([R_BOWL]))[0]
    assert abs(foc - rr.bowl_focus(R_BOWL, A_BOWL, F, C0, RHO, V0)) <= 1e-12 * foc


def test_reference_meets_the_piston_axis():
    p, dA, _ = td.disc([0, 0, 0], [0, 0, 1], 2 * A_PISTON, 2000)
    ref = rr.piston_axis(Z_AXIS, A_PISTON, F, C0, RHO, V0)
    err = np.abs(_axis_field(p, dA, Z_AXIS) - ref).max() / ref.max()
    print(f"piston axis: {err:.2e} of the peak")
    assert err <= 1e-5


def test_reference_gradient_is_the_derivative_of_the_field():
    """The gradient formula against central differences of P, with absorption, off the axis."""
    rng = np.random.default_rng(3)
    p, dA, _ = td.bowl([0, 0, 0], [0, 0, R_BOWL], 2 * A_BOWL, 300)
    q = td.volume_velocity(dA, rng.uniform(0.5, 1.5, 300), rng.uniform(0, 2 * np.pi, 300))
    x = np.array([[0.004, -0.003, 0.05], [-0.01, 0.002, 0.07]])
    _, G, rmin = rr.rayleigh(p, q, x, F, C0, RHO, alpha=5.0, dtype=np.longdouble)
    assert np.allclose(rmin, np.linalg.norm(x[:, None] - p[None], axis=2).min(axis=1), rtol=1e-14)
    G, h = rr.as_complex(G), 1e-6
    for d in range(3):
        e = np.zeros(3)
        e[d] = h
        Pp, _, _ = rr.rayleigh(p, q, x + e, F, C0, RHO, alpha=5.0, dtype=np.longdouble)
        Pm, _, _ = rr.rayleigh(p, q, x - e, F, C0, RHO, alpha=5.0, dtype=np.longdouble)
        fd = (rr.as_complex(Pp) - rr.as_complex(Pm)) / (2 * h)
        assert np.abs(fd - G[:, d]).max() <= 1e-5 * np.abs(G).max()


def test_reference_skips_a_pair_at_distance_zero():
    p = np.array([[0.0, 0.0, 0.0], [0.0, 0.0, 0.01]])
    q = np.array([1e-6 + 0j, 2e-6j])
    P, G, rmin = rr.rayleigh(p, q, p[:1], F, C0, RHO)
    P1, G1, _ = rr.rayleigh(p[1:], q[1:], p[:1], F, C0, RHO)
    assert rmin[0] == 0.0 and np.array_equal(rr.planes(P), rr.planes(P1)) and np.array_equal(rr.planes(G), rr.planes(G1))


# ---- the drive ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,scale", [("neumann", 1.0), ("transparent", 2.0)])
def test_drive_reproduces_the_steady_state_signal(mode, scale):
    """a C cos(w (t - tau)) through source.waveform equals Re[G exp(-i w t)] past the ramp."""
    rng = np.random.default_rng(11)
    n, p0, s0 = 200, 6.0e4, 1500.0
    P = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    gP = 2e3 * (rng.standard_normal((n, 3)) + 1j * rng.standard_normal((n, 3)))
    nv = np.array([-1.0, 0.0, 0.0])
    w = 2 * np.pi * F
    Cs = scale * p0 * w / s0
    G = gP @ nv - ((1j * w / C0) * P if mode == "transparent" else 0.0)
    amp, tau = td.drive(P, gP, nv, F, Cs, c=C0, mode=mode)
    assert amp.shape == (n,) and (amp >= 0).all() and (tau >= 0).all() and (tau < 1 / F).all()
    for t in (5.0 / F, 5.37 / F, 9.81 / F):
        g = source.waveform(t, F, p0, s0, amp=amp, tau=tau, scale=scale)
        assert np.abs(g - (G * np.exp(-1j * w * t)).real).max() <= 1e-12 * np.abs(G).max()
    # per-point normals give the same as the shared one
    amp2, tau2 = td.drive(P, gP, np.tile(nv, (n, 1)), F, Cs, c=C0, mode=mode)
    assert np.array_equal(amp, amp2) and np.array_equal(tau, tau2)
    # arrival: the nearest whole-period shift
    ta = rng.uniform(2.0 / F, 40.0 / F, n)
    amp3, tau3 = td.drive(P, gP, nv, F, Cs, c=C0, mode=mode, arrival=ta)
    assert np.array_equal(amp, amp3)
    assert (np.abs(tau3 - ta) <= 0.5 / F + 4 * np.spacing(ta)).all()      # + the rounding of this subtraction
    shift = (tau3 - tau) * F
    assert np.abs(shift - np.round(shift)).max() <= 1e-9                  # whole periods: the phase is unchanged
    t = 60.0 / F
    g = source.waveform(t, F, p0, s0, amp=amp3, tau=tau3, scale=scale)
    assert np.abs(g - (G * np.exp(-1j * w * t)).real).max() <= 1e-10 * np.abs(G).max()


def test_drive_rejects_bad_arguments():
    P, gP = np.ones(2, dtype=complex), np.ones((2, 3), dtype=complex)
    with pytest.raises(ValueError):
        td.drive(P, gP, [1, 0, 0], F, 1.0, mode="robin")
    with pytest.raises(ValueError):
        td.drive(P, gP, [1, 0, 0], F, 1.0, mode="transparent")          # no sound speed
    with pytest.raises(ValueError):
        td.drive(P, gP[:, :2], [1, 0, 0], F, 1.0)


# ---- the source boundary's DOFs and plane ---------------------------------------------------------------------------------
def _box():
    mesh = fa.BoxMesh([0, 0, 0], [0.01, 0.012, 0.014], (2, 3, 2))
    return mesh, fa.FunctionSpace(mesh, 3)


def test_facet_dofs_and_outward_normal_of_a_box_face():
    mesh, V = _box()
    x = V.tabulate_dof_coordinates()
    cells, lf, ax, sd = mesh.exterior_facets()
    for axis, side, nv in ((0, 0, [-1, 0, 0]), (1, 1, [0, 1, 0]), (2, 0, [0, 0, -1])):
        sel = (ax == axis) & (sd == side)
        dofs = td.facet_dofs(V, cells[sel], lf[sel])
        want = np.flatnonzero(np.abs(x[:, axis] - (mesh.hi[axis] if side else mesh.lo[axis])) < 1e-14)
        assert np.array_equal(dofs, want)
        got = td.outward_normal(x[dofs], mesh.geometry.x.mean(axis=0))
        assert np.abs(got - np.array(nv, dtype=float)).max() <= 1e-12


def test_set_transducer_raises_on_a_non_planar_source_boundary():
    """Two faces tagged as the source and no ``normal``: the plane fit refuses before anything reaches the device."""
    mesh, V = _box()
    cells, lf, ax, sd = mesh.exterior_facets()
    sel = (sd == 0) & ((ax == 0) | (ax == 1))
    m = object.__new__(fa.LinearSpectralExplicit)
    m.V, m.mesh, m._source_facets = V, mesh, (cells[sel], lf[sel])
    p, dA, _ = td.disc([-0.01, 0.006, 0.007], [1, 0, 0], 0.01, 10)
    with pytest.raises(ValueError, match="not planar"):
        m.set_transducer(p, td.volume_velocity(dA), C0, RHO)
    with pytest.raises(ValueError):
        td.outward_normal(np.array([[0.0, 0, 0], [1.0, 0, 0], [2.0, 0, 0]]), [0, 1, 0])   # a line
