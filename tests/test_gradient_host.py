"""The gradient operator's numpy reference (gradient_ref.py) against known answers, the host helpers of
fenicsxfus_amd.intensity, and the shape checks of the Python wrappers: no device needed."""
import numpy as np
import pytest

import fenicsxfus_amd as fa
import gradient_ref
from fenicsxfus_amd import intensity
from fenicsxfus_amd.operators import SpectralOperatorData
from fp32_budget import CAP_CEILING
from util import Problem

ULP64 = 2.0 ** -52


def _coords(pr, dtype=np.float64):
    return pr.V.tabulate_dof_coordinates()[:, :pr.tdim].astype(dtype)


def _poly(X):
    """u = x^2 y - 3 z^3 + x y z and its gradient, in X's precision."""
    x, y, z = X[:, 0], X[:, 1], X[:, 2]
    return x * x * y - 3 * z ** 3 + x * y * z, np.array([2 * x * y + y * z, x * x + x * z, -9 * z * z + x * y])


# ---- reference KATs ---------------------------------------------------------------------------------------------------
def test_polynomial_is_differentiated_exactly(orc):
    """Affine mesh, P = 3, u = x^2 y - 3 z^3 + x y z (degree <= 3 per variable): the nodal gradient is the analytic one.
    The long-double evaluation on long-double nodal values is held to CAP x the float64-vs-long-double error of the
    reference (floor: one double ulp); that yardstick itself must be a rounding error."""
    pr = Problem(orc, (3, 2, 2), 3, lo=[0.1, -0.2, 0.3], hi=[1.3, 0.7, 1.1])
    hi, r64 = gradient_ref.of_problem(pr, np.longdouble), gradient_ref.of_problem(pr, np.float64)
    X = _coords(pr, np.longdouble)
    u, exact = _poly(X)
    u64 = u.astype(np.float64)
    yard = gradient_ref.errors(r64.gradient(u64), hi.gradient(u64))
    err = gradient_ref.errors(hi.gradient(u), exact)
    print("polynomial: long-double reference against the analytic gradient", err, "yardstick", yard)
    for k in err:
        assert yard[k] < 1e-13, (k, yard[k])
        assert err[k] <= CAP_CEILING * max(yard[k], ULP64), (k, err[k], yard[k])
    # the weighted form and the denominator: M(1) 1
    w = hi.gradient(u, nodal=False)
    assert np.array_equal(w / hi.denominator(), hi.gradient(u))
    assert abs(float(hi.denominator().sum()) - 1.2 * 0.9 * 0.8) < 1e-15


@pytest.mark.parametrize("kw", [dict(n=(3, 2, 2), P=3, perturb=0.15), dict(n=(4, 3), P=4, perturb=0.15),
                                dict(n=(3, 2, 2), P=2, order=2,
                                     warp=lambda x: x + np.c_[0.2 * x[:, 1] ** 2, 0.15 * x[:, 2] ** 2, 0 * x[:, 0]])])
def test_constant_field_has_no_gradient(orc, kw):
    """On distorted and curved cells a constant field gives zero, relative to max|u| / hmin."""
    pr = Problem(orc, **kw)
    ref = gradient_ref.of_problem(pr, np.float64)
    g = ref.gradient(np.full(pr.ndofs, 3.5))
    assert np.abs(g).max() <= 64 * ULP64 * 3.5 / pr.mesh.hmin()
    lin = ref.gradient(_coords(pr) @ np.arange(1.0, pr.tdim + 1))     # u = x + 2 y (+ 3 z): in the space on every such cell
    assert np.abs(lin - np.arange(1.0, pr.tdim + 1)[:, None]).max() < 1e-11


def test_plane_wave_intensity(orc):
    """a = A cos(kappa x), b = A sin(kappa x) with coef = 1 / (2 rho w) give A^2 / (2 rho c) along x; the transverse
    components stay at the level of the interpolation error."""
    A, rho, c, f0 = 6e4, 1000.0, 1500.0, 0.5e6
    lam = c / f0
    pr = Problem(orc, (6, 2, 2), 6, hi=[lam, lam / 3, lam / 3])
    ref = gradient_ref.of_problem(pr, np.float64)
    x = _coords(pr)[:, 0]
    kap = 2 * np.pi / lam
    coef = intensity.intensity_coef(np.full(pr.mesh.num_cells, rho), f0, 1)
    I = ref.gradient_pairs(A * np.cos(kap * x), A * np.sin(kap * x), coef)
    I0 = A * A / (2 * rho * c)
    print(f"plane wave: I0 {I0:.6e}, error along x {np.abs(I[0] - I0).max() / I0:.2e}, transverse {np.abs(I[1:]).max() / I0:.2e}")
    assert np.abs(I[0] - I0).max() <= 1e-5 * I0          # P = 6, six elements per wavelength
    assert np.abs(I[1:]).max() <= 1e-5 * I0


@pytest.mark.parametrize("kw", [dict(n=(3, 2, 2), P=3, perturb=0.15), dict(n=(4, 3), P=2, perturb=0.1),
                                dict(n=(2, 2, 2), P=2, order=2,
                                     warp=lambda x: x + np.c_[0.2 * x[:, 1] ** 2, 0.15 * x[:, 2] ** 2, 0 * x[:, 0]]),
                                dict(quad2=True, n=(3, 2), P=3, warp=lambda x: x + np.c_[0.2 * x[:, 1] ** 2, 0.1 * x[:, 0] ** 2])])
def test_weights_are_the_oracles(orc, kw):
    """The reference's |det J| w is oracle.geometry's detJ: the new reference stands on the existing one."""
    kw = dict(kw)
    pr = gradient_ref.Quad2Problem(orc, **kw) if kw.pop("quad2", False) else Problem(orc, **kw)
    ref = gradient_ref.of_problem(pr, np.float64)
    d = np.asarray(pr.detJ).reshape(ref.W.shape)
    assert np.abs(ref.W - d).max() <= 16 * ULP64 * np.abs(d).max()
    # and K K^T |det J| w is its G (xx of it: the first entry)
    G = np.asarray(pr.G).reshape(ref.W.shape + (-1,))
    gxx = np.einsum("eqd,eqd->eq", ref.K[:, :, 0, :], ref.K[:, :, 0, :]) * ref.W
    assert np.abs(gxx - G[:, :, 0]).max() <= 1e-12 * np.abs(G[:, :, 0]).max()


def test_node_order_does_not_matter(orc):
    order = [2, 0, 3, 1]
    a = Problem(orc, (2, 2, 3), 3, perturb=0.1)
    b = Problem(orc, (2, 2, 3), 3, perturb=0.1, node_order=order)
    u = np.random.default_rng(3).standard_normal(a.ndofs)
    ga, gb = gradient_ref.of_problem(a, np.float64).gradient(u), gradient_ref.of_problem(b, np.float64).gradient(u)
    assert np.abs(ga - gb).max() <= 1e-12 * np.abs(ga).max()


# ---- intensity.py -----------------------------------------------------------------------------------------------------
def test_intensity_helpers():
    rho, c = np.array([1000.0, 1850.0, 1000.0]), np.array([1500.0, 2800.0, 1500.0])
    f0, K = 0.5e6, 3
    ic = intensity.intensity_coef(rho, f0, K)
    assert ic.shape == (K, 3) and ic.dtype == np.float64
    assert np.allclose(ic[1], 1.0 / (2 * rho * 2 * np.pi * 2 * f0), rtol=1e-15)
    alpha = np.array([[0.5, 20.0, 0.5], [1.1, 43.0, 1.1], [1.7, 67.0, 1.7]])
    fc = intensity.force_coef(alpha, rho, c, f0)
    assert fc.shape == (K, 3)
    assert np.allclose(fc, 2 * alpha / c * ic, rtol=4e-16, atol=0)
    assert intensity.force_coef(alpha[0], rho, c, f0).shape == (1, 3)
    # a plane wave of amplitude A has |w| = A / (rho c): gradients kappa A along x, in quadrature
    A, kap, w = 6e4, 2 * np.pi * f0 / 1500.0, 2 * np.pi * f0
    xs = np.linspace(0, 1e-3, 7)
    gc = np.array([-kap * A * np.sin(kap * xs), 0 * xs, 0 * xs])
    gs = np.array([kap * A * np.cos(kap * xs), 0 * xs, 0 * xs])
    v = intensity.velocity_amplitude(gc, gs, 1000.0, w)
    assert v.shape == (7,) and np.allclose(v, A / (1000.0 * 1500.0), rtol=1e-14)
    for bad in (lambda: intensity.intensity_coef(rho, 0.0, 1), lambda: intensity.intensity_coef(rho[:, None], f0, 1),
                lambda: intensity.force_coef(alpha[:, :2], rho, c, f0), lambda: intensity.force_coef(-alpha, rho, c, f0),
                lambda: intensity.velocity_amplitude(gc, gs[:2], 1000.0, w),
                lambda: intensity.velocity_amplitude(gc, gs, np.ones(3), w)):
        with pytest.raises(ValueError):
            bad()


def test_power_through_a_face(orc):
    """A uniform intensity I0 along x through the face x = hi of a box: I0 times the face's area."""
    pr = Problem(orc, (2, 2, 2), 3, hi=[0.02, 0.03, 0.05])
    tags = fa.tag_box_boundary(pr.mesh)
    cells, lf, ax, sd = pr.mesh.exterior_facets()
    sel = (ax == 0) & (sd == 1)
    w = pr.facet_diag(fa.FacetTags(cells[sel], lf[sel], np.ones(int(sel.sum()), np.int32)), 1, np.ones(pr.mesh.num_cells))
    dofs = np.flatnonzero(w)
    I = np.tile([40.0, 1.0, -2.0], (pr.ndofs, 1))
    got = intensity.power_through(pr.V, I, dofs, [1.0, 0.0, 0.0], w[dofs])
    assert abs(got - 40.0 * 0.03 * 0.05) <= 1e-12 * 40.0 * 0.03 * 0.05
    assert tags is not None
    with pytest.raises(ValueError):
        intensity.power_through(pr.V, I[:, :2], dofs, [1.0, 0.0, 0.0], w[dofs])
    with pytest.raises(ValueError):
        intensity.power_through(pr.V, I, dofs, [1.0, 0.0, 0.0], w[dofs][:-1])


def test_vector_fields_go_to_vtu(orc, tmp_path):
    """What model.intensity() returns, (ndofs, tdim), is written as a three-component point field beside scalar ones."""
    for pr in (Problem(orc, (2, 2, 2), 2), Problem(orc, (3, 2), 2)):
        I = np.arange(pr.ndofs * pr.tdim, dtype=np.float64).reshape(pr.ndofs, pr.tdim)
        path = str(tmp_path / f"i{pr.tdim}.vtu")
        fa.output.write_vtu(path, pr.V, {"I": I, "p": np.ones(pr.ndofs)})
        back = fa.output.read_vtu(path)
        assert back["I"].shape == (pr.ndofs, 3) and np.array_equal(back["I"][:, :pr.tdim], I)
        assert not back["I"][:, pr.tdim:].any() and back["p"].shape == (pr.ndofs,)


# ---- the wrappers reject wrong shapes before any device call ---------------------------------------------------------------
def test_wrappers_reject_wrong_shapes():
    d = object.__new__(SpectralOperatorData)       # no operator behind it: a device call would fail on the null handle
    d.h, d.ndofs, d.ncells, d.tdim, d.dtype = None, 10, 4, 3, np.dtype(np.float64)
    x, c = np.zeros(10), np.ones(4)
    for bad in (lambda: d.gradient(np.zeros(9)), lambda: d.gradient(x, np.ones(5)), lambda: d.gradient(np.zeros((2, 10))),
                lambda: d.gradient(x, c, out=np.zeros((2, 10))), lambda: d.gradient(x, c, out=np.zeros((3, 10), np.float32)),
                lambda: d.gradient_pairs(np.zeros((2, 10)), np.zeros((3, 10)), np.ones((2, 4))),
                lambda: d.gradient_pairs(np.zeros((2, 9)), np.zeros((2, 9)), np.ones((2, 4))),
                lambda: d.gradient_pairs(np.zeros((2, 10)), np.zeros((2, 10)), np.ones((1, 4))),
                lambda: d.gradient_pairs(np.zeros((9, 10)), np.zeros((9, 10)), np.ones((9, 4))),
                lambda: d.gradient_pairs(x, x, np.ones(5))):
        with pytest.raises(ValueError):
            bad()


def test_abi_lists_the_new_entry_points():
    from fenicsxfus_amd import _abi

    assert {"fus_op_gradient", "fus_op_gradient_pairs", "fus_op_gradient_plan", "fus_model_intensity"} <= set(_abi.SYMBOLS)
    assert (_abi.FUS_GRAD_WEIGHTED, _abi.FUS_GRAD_NODAL) == (0, 1)
