"""CPU guards of the receiver tests (receiver_ref.py; the GPU side is test_gpu_receivers_matrix.py).

(1) the plain restatement in double against evaluate.evaluate, at the fp64 budget;
(2) evaluate.locate on points whose (cell, X) is known by construction: interior, face, edge, vertex and GLL-node
    points of distorted cells, the mesh boundary included, and points outside;
(3) negative controls: four ways in which a sampling kernel can be wrong, applied to the restatement, must each exceed
    the cap the GPU result is held to, in every case of the matrix and in both types;
(4) the yardstick of every fp32 case is small enough for the GPU assertion to mean something."""
import numpy as np
import pytest

import fp32_budget as fb
import receiver_ref as rr
from fenicsxfus_amd.evaluate import evaluate, locate

IDS = [f"{g}-p{P}" for g, P in rr.MATRIX]
# the restatement against evaluate.py: the Gmsh fixture at the lowest, a middle and the highest degree as well
EVAL = rr.MATRIX + [("gmsh", P) for P in (2, 7, 10)]
TYPES = {"f64": np.float64, "f32": np.float32}


def test_long_double_is_extended():
    rr.host_guard()


def test_default_floor_of_fp32_budget_is_unchanged():
    """fp32_budget.budget without ``floor`` is what it was: one float ulp."""
    rng = np.random.default_rng(0)
    r64 = rng.standard_normal(50)
    g, r32 = r64 * (1 + 3e-9), r64.copy()
    reg = {"a": np.arange(25)}
    w, _, tab = fb.budget(g, r32, r64, reg)
    assert all(y == fb.EPS32 for _, y in tab["y"].values()) and w == pytest.approx(3e-9 / fb.EPS32, rel=1e-6)
    w64, _, tab = fb.budget(g, r32, r64, reg, floor=2.0 ** -52)
    assert all(y == 2.0 ** -52 for _, y in tab["y"].values()) and w64 > w


@pytest.mark.parametrize("geom,P", EVAL, ids=[f"{g}-p{P}" for g, P in EVAL])
def test_restatement_against_evaluate(geom, P):
    """evaluate.evaluate (barycentric weights, einsum) and the direct-product restatement are two codes for the same
    interpolant at the same located pair: evaluate's values lie within the fp64 budget of the restatement's.
    evaluate.py moves a coordinate that lies within 1e-14 of a GLL node onto the node (its barycentric form divides by
    the distance); the restatement and the long-double reference of THIS test are taken at the coordinates so moved.
    (Against the interpolant at the unmoved located X evaluate.py differs by the field's slope times that distance:
    ratios of 10 ... 670 on these meshes, which says nothing about either code.)"""
    cs = rr.sample_case(geom, P)
    p = cs.points
    nodes = np.asarray(cs.V.nodes1d, dtype=np.float64)
    d = cs.loc_X[:, :, None] - nodes[None, None, :]
    k = np.abs(d).argmin(axis=2)
    Xs = np.where(np.abs(d).min(axis=2) < 1e-14, nodes[k], cs.loc_X)
    got = tuple(evaluate(cs.V, a, p.pts[:p.n_inside]) for a in (cs.u, cs.v))
    ref = tuple(np.asarray(rr.interp(cs.V, a, cs.loc_cell, Xs, np.longdouble), dtype=np.float64) for a in (cs.u, cs.v))
    yard = tuple(np.asarray(rr.interp(cs.V, a, cs.loc_cell, Xs, np.float64)) for a in (cs.u, cs.v))
    rr.check(f"evaluate.py {cs.label}", got, yard, ref, p.regions, np.float64)


@pytest.mark.parametrize("geom,P", rr.MATRIX, ids=IDS)
def test_locate_round_trip(geom, P):
    cs = rr.sample_case(geom, P)
    p, n = cs.points, cs.points.n_inside
    cell, X = cs.located
    missing = {k: int((cell[idx] < 0).sum()) for k, idx in p.regions.items() if (cell[idx] < 0).any()}
    assert not missing, f"constructed points that locate did not find: {missing}"
    assert np.all(cell[n:] == -1), "a point outside the mesh was located"
    back = rr.forward(cs.mesh, cell[:n], X[:n])
    per_class = {k: float(np.abs(back[idx] - p.pts[idx]).max()) for k, idx in p.regions.items()}
    print(f"locate {cs.label}: |x(X) - p| per class {per_class}")
    assert max(per_class.values()) <= 1e-9 * rr.extent(cs.mesh)
    assert np.all((X[:n] > -1e-9) & (X[:n] < 1 + 1e-9))
    ii = p.regions["interior"]
    assert np.array_equal(cell[ii], p.cell[ii])
    assert np.abs(X[ii] - p.X[ii]).max() <= 1e-9
    # a face / edge / vertex / node point may come back in any cell that contains it
    again = locate(cs.mesh, p.pts)
    assert np.array_equal(again[0], cell) and np.array_equal(again[1], X)


@pytest.mark.parametrize("geom,P", rr.COUNT_CASES)
def test_locate_does_not_depend_on_the_other_points(geom, P):
    """The receiver-count test on the GPU compares samples of point subsets bit for bit with rows of the full set's:
    the located pair of a point must not depend on which points are located with it."""
    cs = rr.sample_case(geom, P)
    cell, X = cs.located
    for n, idx in rr.SUBSETS.items():
        c, Y = locate(cs.mesh, cs.points.pts[idx])
        assert np.array_equal(c, cell[idx]) and np.array_equal(Y, X[idx]), n


def _controls(cs, T):
    """{name: (u, v) samples of a wrong kernel}: the restatement in T on the located pair with one defect each."""
    V, cell, X = cs.V, cs.loc_cell, cs.loc_X
    W = rr.weights(V, X, T)
    U = {f: rr.gather(V, a, cell, T) for f, a in (("u", cs.u), ("v", cs.v))}
    t = X.shape[1]
    swapped = rr.weights(V, X[:, [1, 0] + list(range(2, t))], T)        # b0 <-> b1
    shifted = rr.weights(V, X + 1e-3, T)

    def rot(a):
        a = a.copy()
        a[0] = np.roll(a[0], 1)                                        # receiver 0's DOF list rotated by one entry
        return a

    out = {
        "axes swapped": {f: rr.seqsum(swapped, U[f]) for f in U},
        "dof list rotated": {f: rr.seqsum(W, rot(U[f])) for f in U},
        "last entry dropped": {f: rr.seqsum(W[:, :-1], U[f][:, :-1]) for f in U},
        "basis at X + 1e-3": {f: rr.seqsum(shifted, U[f]) for f in U},
    }
    return {k: {f: np.asarray(a, dtype=np.float64) for f, a in d.items()} for k, d in out.items()}


@pytest.mark.parametrize("tname", list(TYPES))
@pytest.mark.parametrize("geom,P", rr.MATRIX, ids=IDS)
def test_negative_controls_exceed_the_cap(geom, P, tname):
    T = TYPES[tname]
    cs = rr.sample_case(geom, P, T)
    p = cs.points
    # the restatement itself passes (ratio <= 1 by construction of the yardstick)
    w0, _, _ = rr.budget(cs.pair(cs.yard), cs.pair(cs.yard), cs.pair(cs.ref), p.regions, T)
    assert w0 <= 1.0
    for name, g in _controls(cs, T).items():
        if name == "axes swapped":        # on the random field
            worst, where, table = rr.budget(g["u"], cs.yard["u"], cs.ref["u"], p.regions, T)
        else:
            worst, where, table = rr.budget(cs.pair(g), cs.pair(cs.yard), cs.pair(cs.ref), p.regions, T)
        print(fb.report(f"[control {tname}] {cs.label} {name}", worst, where, table))
        assert worst > rr.cap(T), f"{name} would pass on the GPU: ratio {worst} <= cap {rr.cap(T)}"
        # and against the kernel-alone reference
        worst, where, table = rr.budget(cs.pair(g), cs.pair(cs.yard), cs.pair(cs.kref), p.regions, T)
        assert worst > rr.cap(T), f"{name} would pass the kernel-alone check: ratio {worst}"


@pytest.mark.parametrize("geom,P", rr.MATRIX, ids=IDS)
def test_fp32_yardstick_is_sane(geom, P):
    cs = rr.sample_case(geom, P, np.float32)
    for ref in (cs.ref, cs.kref):
        for f in ("u", "v"):
            y = fb.errors(cs.yard[f], ref[f], cs.points.regions)
            assert max(y.values()) <= fb.YARD_SANE, f"{cs.label} {f}: yardstick {max(y.values()) / fb.EPS32:.1f} ulp"
