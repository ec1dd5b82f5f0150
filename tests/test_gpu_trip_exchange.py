"""The element trips of the fp64 per-cell geometry kernels at the degrees whose LDS reads are issued singly (2, 3, 4:
kernels.hpp lds_single_reads): every kernel family whose trip code reads the exchange tile or the per-cell geometry
that way -- trilinear map on a vertex-perturbed mesh, general affine form on a sheared mesh, diagonal metric on a box;
stiffness, mass and the two-input form of the lossy model; LDS atomics and deterministic rounds -- on meshes where each
partial shape of a trip occurs:

  1 element                            one active slot, the rest of its wave and every other wave idle
  3 x 1 x 1 in one block               an odd count, the last active wave part full
  (slots + 1) x 1 x 1 in one block     more elements than one trip has slots (17 at degrees 3 and 4, 29 at degree 2)
  2 x 2 x 2 with one-element blocks    every DOF on a block boundary

On every shape: operator action (stiffness, mass) against the oracle at 1e-12 relative, three RK4 steps of the linear
and of the lossy model (the two-input form is reached through it) at 1e-10, deterministic mode twice: bit-identical."""
import numpy as np
import pytest

import fenicsxfus_amd as fa
from fenicsxfus_amd import tag_box_boundary
from util import Problem

pytestmark = pytest.mark.gpu

TOL_OP = 1e-12
TOL_RK = 1e-10
DEGREES = [2, 3, 4]
GEOMETRIES = ["trilinear", "affine", "diag"]
SHEAR = np.array([[1.0, 0.3, 0.0], [0.0, 1.0, 0.2], [0.1, 0.0, 1.0]])


def relmax(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def shapes(P):
    """(cells, block_elems, waves) of the four partial trip shapes; None: the library's default."""
    long_row = {2: (29, 64, 4), 3: (17, 32, 4), 4: (17, 32, 8)}[P]
    return {"one": ((1, 1, 1), None, None), "three": ((3, 1, 1), None, None),
            "second_trip": ((long_row[0], 1, 1), long_row[1], long_row[2]), "block_per_element": ((2, 2, 2), 1, None)}


@pytest.fixture(scope="module")
def problems(orc):
    """One oracle problem per (degree, geometry, shape), built on first use and left unchanged."""
    cache = {}

    def get(P, geom, shape):
        key = (P, geom, shape)
        if key not in cache:
            n = shapes(P)[shape][0]
            hi = [0.004 * n[0], 0.004 * n[1], 0.004 * n[2]]
            pr = Problem(orc, n, P, hi=hi, perturb=0.2 if geom == "trilinear" else 0.0)
            tags = tag_box_boundary(pr.mesh)
            if geom == "affine":
                x = pr.mesh.geometry.x
                x[:] = x @ SHEAR.T
                pr.G, pr.detJ = orc.geometry(3, x, pr.mesh.geometry.dofmap, pr.nodes, pr.wts)
            cache[key] = (pr, tags)
        return cache[key]

    return get


def context(P, geom, shape, det):
    _, be, waves = shapes(P)[shape]
    return fa.Context(0, block_elems=be, waves=waves, deterministic=det, geometry="trilinear" if geom == "trilinear" else None)


def check_mode(d, geom):
    if geom == "trilinear":
        assert d.geometry_mode() == "trilinear"
    else:
        assert d.geometry_mode() == "affine" and d.uses_diag_metric() == (geom == "diag")


@pytest.mark.parametrize("shape", ["one", "three", "second_trip", "block_per_element"])
@pytest.mark.parametrize("geom", GEOMETRIES)
@pytest.mark.parametrize("P", DEGREES)
def test_operator_action(problems, P, geom, shape):
    pr, _ = problems(P, geom, shape)
    rng = np.random.default_rng(100 * P + len(shape))
    x, coef = rng.standard_normal(pr.ndofs), rng.uniform(0.5, 2.0, pr.mesh.num_cells)
    K, M = pr.K(x, coef), pr.M(x, coef)
    # the operators accumulate into y: start values of the size of the action (millimetre cells: |M x| ~ 1e-8 |x|)
    y0 = rng.standard_normal(pr.ndofs)
    yk0, ym0 = y0 * np.abs(K).max(), y0 * np.abs(M).max()
    for det in (0, 1):
        c = context(P, geom, shape, det)
        d = fa.SpectralOperatorData(pr.V, c)
        check_mode(d, geom)
        if shape == "block_per_element":
            assert d.info()["nblocks"] == pr.mesh.num_cells
        elif shape != "one":
            assert d.info()["nblocks"] == 1
        y = d.stiffness(x, coef, yk0.copy())
        ym = d.mass(x, coef, ym0.copy())
        ek, em = relmax(y, yk0 + K), relmax(ym, ym0 + M)
        print(f"P={P} {geom} {shape} det={det}: stiffness {ek:.2e} mass {em:.2e}")
        assert ek < TOL_OP and em < TOL_OP
        if det:
            assert np.array_equal(d.stiffness(x, coef, yk0.copy()), y)
            assert np.array_equal(d.mass(x, coef, ym0.copy()), ym)
        d.close()
        c.close()


@pytest.mark.parametrize("shape", ["one", "three", "second_trip", "block_per_element"])
@pytest.mark.parametrize("geom", GEOMETRIES)
@pytest.mark.parametrize("P", DEGREES)
def test_three_rk4_steps_linear_and_lossy(orc, problems, P, geom, shape):
    pr, tags = problems(P, geom, shape)
    nc = pr.mesh.num_cells
    cx = pr.mesh.cell_centroids()[:, 0]
    sel = cx > np.median(cx)
    c0, rho = np.where(sel, 2800.0, 1500.0), np.where(sel, 1850.0, 1000.0)
    f0, p0, s0 = 0.5e6, 6e4, 1500.0
    dt = 0.25 * 0.004 / (c0.max() * P**2)
    tf = 3 * dt * (1 - 1e-9)
    delta = np.where(sel, fa.compute_diffusivity_of_sound(2 * np.pi * f0, 2800.0, 46.0),
                     fa.compute_diffusivity_of_sound(2 * np.pi * f0, 1500.0, 0.2))
    m, src, absb, coeff = pr.linear_model_vectors(c0, rho, tags)
    ul, vl = np.zeros(pr.ndofs), np.zeros(pr.ndofs)
    orc.linear_rk4(3, pr.N, pr.dm, pr.G, pr.D, coeff, m, src, absb, f0, p0, s0, 0.0, tf, dt, ul, vl)
    m, src, absb, src2, lin, att = pr.lossy_model_vectors(c0, rho, delta, tags)
    uy, vy = np.zeros(pr.ndofs), np.zeros(pr.ndofs)
    orc.lossy_rk4(3, pr.N, pr.dm, pr.G, pr.D, lin, att, m, src, absb, src2, f0, p0, s0, 0.0, tf, dt, uy, vy)
    assert np.abs(ul).max() > 0 and np.abs(uy).max() > 0 and nc > 0
    for det in (0, 1):
        ctx = context(P, geom, shape, det)
        # the two-input form (NF = 2) sizes its blocks for two staged inputs; the shapes must hold there too
        d2 = fa.SpectralOperatorData(pr.V, ctx, fields=2)
        assert d2.info()["nblocks"] == (nc if shape == "block_per_element" else 1)
        d2.close()
        runs = []
        for _ in range(2 if det else 1):
            model = fa.LinearSpectralExplicit(pr.mesh, tags, P, c0, rho, f0, p0, s0, 4, dt, V=pr.V, ctx=ctx)
            check_mode(model.data, geom)
            model.init()
            un, vn, _ = model.rk(0.0, tf)
            lin_uv = (un.x.array.copy(), vn.x.array.copy())
            model.close()
            model = fa.LossySpectralExplicit(pr.mesh, tags, P, c0, rho, delta, f0, p0, s0, 4, dt, V=pr.V, ctx=ctx)
            check_mode(model.data, geom)
            model.init()
            un, vn, _ = model.rk(0.0, tf)
            runs.append(lin_uv + (un.x.array.copy(), vn.x.array.copy()))
            model.close()
        errs = [relmax(a, b) for a, b in zip(runs[0], (ul, vl, uy, vy))]
        print(f"P={P} {geom} {shape} det={det}: linear u {errs[0]:.2e} v {errs[1]:.2e} lossy u {errs[2]:.2e} v {errs[3]:.2e}")
        assert max(errs) < TOL_RK
        if det:
            assert all(np.array_equal(a, b) for a, b in zip(runs[0], runs[1]))
        ctx.close()
