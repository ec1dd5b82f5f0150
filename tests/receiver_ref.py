"""A plain reference for the receivers (k_sample, set_receivers / sample / record) that shares nothing with
fenicsxfus_amd.evaluate.

* Test points by construction: (cell, X) with X in the reference cell is mapped FORWARD through the cell's
  multilinear map to a physical point (numpy, double), so the truth is known without any inversion.
* ``interp(V, u, cell, X, dtype)``: the direct Lagrange product l_i(X) = prod_{j != i} (X - x_j) / (x_i - x_j) on
  V.nodes1d with the tensor sum over V.tensor_dofmap[cell].  In np.longdouble it is the reference; in float64 / float32
  it is the plain restatement of what the library does: basis values formed in double and rounded to T once (as
  fus_model_set_receivers does), w = b0 * b1 * b2 in T, a sequential sum in T.
* Error measure: fp32_budget's errors / budget with the point classes as regions, the longdouble values as the
  reference, the restatement in the model's own type as the yardstick and one ulp of that type as the floor.

The restatement is evaluated at the (cell, X) that ``locate`` returned, i.e. on what the library is handed, the
reference at the constructed pair.  The restatement cannot be taken at the constructed X: a random field of degree P
has dU/dX of the order of P^2 |U|, so even a located X that is the correctly rounded double of the true one moves
the sample by tens of ulp (degree 10: ~60), and the Newton inversion's own residual rounding (eps |x| / h) by more;
restating the library at the located X in double gives 11 ... 255 times the error of the restatement at the
constructed X on the meshes of the matrix, before any kernel has run.  No kernel could pass that.  What ``locate``
itself may be wrong by is bounded on the host (test_receivers_host.py: 1e-9 x extent, its own acceptance); the
kernel alone is held to the same cap against the long-double interpolant at the located pair (``kref``).
"""
import numpy as np

import fp32_budget as fb

FLOOR = {np.dtype(np.float32): 2.0 ** -23, np.dtype(np.float64): 2.0 ** -52}
# CAP64 follows the rule of fp32_budget.CAP with the 2^-52 floor: the smallest power of two
# >= 2 x the largest ratio measured on the MI355X (1.500: quadrilaterals, P = 2; table "Receivers" there), never below
# 2 and never above 8.
CAP64 = 4
N_INTERIOR = 257
# receiver counts 1, 2, 3 mod 4 (the tail waves of the last block leave early) and the 258 points they are taken from:
# rows of the first 258 constructed points (the interior points and one face point)
N_COUNTS = N_INTERIOR + 1
SUBSETS = {1: [257], 2: [3, 200], 3: [0, 1, 257], 5: [5, 64, 65, 130, 256], N_COUNTS: list(range(N_COUNTS))}
COUNT_CASES = [("hex", 3), ("hex", 5), ("quad", 2)]      # N^3 = 64, N^3 = 216, N^2 = 9


def cap(dtype):
    return fb.CAP if np.dtype(dtype) == np.float32 else CAP64


def host_guard():
    """The reference needs an extended long double (x87: eps = 2^-63)."""
    assert np.finfo(np.longdouble).eps < 2.0 ** -60, "np.longdouble is no wider than double on this host"


# ---- geometry: the forward multilinear map -----------------------------------------------------------------------------
def forward(mesh, cell, X):
    """Physical points x(X) of the first-order cells ``cell`` at reference coordinates X [m, t] (tensor vertex order
    v = vx + 2 vy + 4 vz), in double."""
    t = mesh.topology.dim
    x = np.asarray(mesh.geometry.x, dtype=np.float64)[:, :t]
    cd = x[np.asarray(mesh.geometry.dofmap)[cell]]                     # [m, 2^t, t]
    X = np.asarray(X, dtype=np.float64)
    out = np.zeros((len(cell), t))
    for v in range(1 << t):
        w = np.ones(len(cell))
        for d in range(t):
            w = w * (X[:, d] if (v >> d) & 1 else 1.0 - X[:, d])
        out += w[:, None] * cd[:, v, :]
    return out


def extent(mesh):
    t = mesh.topology.dim
    return float(np.ptp(np.asarray(mesh.geometry.x, dtype=np.float64)[:, :t], axis=0).max())


# ---- the interpolant ----------------------------------------------------------------------------------------------------
def lagrange(nodes, X, wide):
    """l_i(X) [m, N] by the direct product, in ``wide`` (double as the library forms them, long double for the
    reference)."""
    nodes = np.asarray(nodes, dtype=wide)
    X = np.asarray(X, dtype=wide)
    N = len(nodes)
    out = np.ones((len(X), N), dtype=wide)
    for i in range(N):
        for j in range(N):
            if j != i:
                out[:, i] = out[:, i] * ((X - nodes[j]) / (nodes[i] - nodes[j]))
    return out


def weights(V, X, dtype):
    """w[m, N^t] = b0[i0] * b1[i1] (* b2[i2]) in ``dtype``, entry k = (i0 N + i1) N + i2.  float32 / float64: the basis
    values are formed in double and rounded to the type once; long double: formed in long double."""
    dtype = np.dtype(dtype)
    X = np.asarray(X, dtype=np.float64)
    t = X.shape[1]
    wide = np.longdouble if dtype == np.longdouble else np.float64
    b = [lagrange(V.nodes1d, X[:, d], wide).astype(dtype) for d in range(t)]
    if t == 3:
        w = (b[0][:, :, None, None] * b[1][:, None, :, None]) * b[2][:, None, None, :]
    else:
        w = b[0][:, :, None] * b[1][:, None, :]
    assert w.dtype == dtype
    return w.reshape(len(X), -1)


def gather(V, u, cell, dtype):
    """u at the DOFs of each receiver's cell [m, N^t], in ``dtype`` (u is rounded to the model's type by the caller)."""
    return np.asarray(u)[np.asarray(V.tensor_dofmap)[cell]].astype(dtype)


def seqsum(W, U):
    """sum_k W[:, k] * U[:, k], one entry after the other in the arrays' own type."""
    assert W.dtype == U.dtype and W.shape == U.shape
    acc = np.zeros(len(W), dtype=W.dtype)
    for k in range(W.shape[1]):
        acc = acc + W[:, k] * U[:, k]
    assert acc.dtype == W.dtype
    return acc


def interp(V, u, cell, X, dtype):
    """u_h at the points (cell, X): the reference in np.longdouble, the library's plain restatement in float64 /
    float32."""
    return seqsum(weights(V, X, dtype), gather(V, u, cell, dtype))


# ---- fields -------------------------------------------------------------------------------------------------------------
def field_random(V, seed=11):
    """Independent normal DOF values: a transposed pair of tensor indices or a wrong DOF inside a cell changes it by
    its own size."""
    return np.random.default_rng(seed).standard_normal(V.num_dofs)


def field_smooth(V):
    Y = V.tabulate_dof_coordinates()
    z = Y[:, 2] if Y.shape[1] > 2 else 0.0
    return np.sin(3 * Y[:, 0]) * np.cos(2 * Y[:, 1]) + z


# ---- point classes ------------------------------------------------------------------------------------------------------
class Points:
    """The constructed receivers of one mesh: ``cell``, ``X`` (truth), ``pts`` (physical, the inside points first, then
    ``n_outside`` points outside the mesh), ``regions`` {class: indices into the inside points}."""

    def __init__(self, mesh, nodes1d, seed=5, max_cells=16):
        t = mesh.topology.dim
        nc = int(np.asarray(mesh.geometry.dofmap).shape[0])
        rng = np.random.default_rng(seed)
        some = np.unique(np.linspace(0, nc - 1, min(nc, max_cells)).astype(np.int64))   # cells of the edge classes
        cells, Xs, regions, n = [], [], {}, 0

        def add(name, c, X):
            nonlocal n
            cells.append(np.asarray(c, dtype=np.int64)), Xs.append(np.asarray(X, dtype=np.float64))
            regions[name] = np.arange(n, n + len(c))
            n += len(c)

        add("interior", rng.integers(0, nc, N_INTERIOR), rng.uniform(0.0, 1.0, (N_INTERIOR, t)))
        # face / edge / vertex: one / two / all components exactly 0 or 1; every such entity of the chosen cells, mesh
        # boundary included (2-D: a quadrilateral's edges are its "faces", two fixed components are a vertex)
        for name, nfix in (("face", 1), ("edge", 2), ("vertex", t)):
            if name == "edge" and t == 2:
                continue
            c_, X_ = [], []
            for mask in range(1 << t):
                fixed = [d for d in range(t) if (mask >> d) & 1]
                if len(fixed) != nfix:
                    continue
                for side in range(1 << nfix):
                    X = rng.uniform(0.0, 1.0, (len(some), t))
                    for k, d in enumerate(fixed):
                        X[:, d] = float((side >> k) & 1)
                    c_.append(some), X_.append(X)
            add(name, np.concatenate(c_), np.concatenate(X_))
        nodes = np.asarray(nodes1d, dtype=np.float64)
        per = 8
        add("node", np.repeat(some, per), nodes[rng.integers(0, len(nodes), (len(some) * per, t))])
        self.cell, self.X, self.regions = np.concatenate(cells), np.concatenate(Xs), regions
        self.n_inside = n
        x = np.asarray(mesh.geometry.x, dtype=np.float64)[:, :t]
        lo, hi = x.min(axis=0), x.max(axis=0)
        outside = np.stack([hi + 0.5 * (hi - lo), lo - 0.25 * (hi - lo), np.r_[hi[0] + 1e-6 * (hi[0] - lo[0]),
                                                                                 0.5 * (lo[1:] + hi[1:])]])
        self.n_outside = len(outside)
        self.pts = np.vstack([forward(mesh, self.cell, self.X), outside])
        self.inside = np.arange(n)


# ---- the meshes of the matrix ---------------------------------------------------------------------------------------------
GEOMETRIES = ("hex", "quad")       # perturbed hexahedra (3, 2, 2) / perturbed quadrilaterals (4, 3), perturb = 0.1
DEGREES = tuple(range(2, 11))
MATRIX = [(g, P) for g in GEOMETRIES for P in DEGREES] + [("gmsh", 4)]
_cases = {}


def build(geom, P, dtype=np.float64):
    """(mesh, V, tags, c0, rho0, dt) of one case; "gmsh" is the reference operator test's own mesh
    (tests/golden/ref_test_operators3d_mesh.npz, data only)."""
    import os

    import fenicsxfus_amd as fa
    if geom == "gmsh":
        from fenicsxfus_amd.unstructured import VTK_TO_TENSOR, HexFunctionSpace, HexMesh
        gold = np.load(os.path.join(os.path.dirname(__file__), "golden", "ref_test_operators3d_mesh.npz"))
        mesh = HexMesh(gold["geometry"], gold["topology_vtk"][:, VTK_TO_TENSOR], dtype=dtype)
        V = HexFunctionSpace(mesh, P)
        tags = mesh.facet_tags(gold["facet_topology"], gold["facet_values"])
        return mesh, V, tags, 1.5, 1.0, 1e-4
    if geom == "hex":
        mesh = fa.BoxMesh([0, 0, 0], [1.0, 0.8, 0.6], (3, 2, 2), perturb=0.1, dtype=dtype)
    else:
        mesh = fa.BoxMesh([0, 0], [1.0, 0.8], (4, 3), perturb=0.1, dtype=dtype)
    return mesh, fa.FunctionSpace(mesh, P), fa.tag_box_boundary(mesh), 1500.0, 1000.0, 1e-8


class SampleCase:
    """One cell of the sampling matrix: mesh, space, the constructed points and, for the fields u = random and
    v = smooth (rounded to ``dtype``), the longdouble reference and the restatement in ``dtype``.  Computed once and
    shared by the tests; nothing changes it afterwards."""

    def __init__(self, geom, P, dtype):
        host_guard()
        self.geom, self.P, self.dtype = geom, P, np.dtype(dtype)
        self.mesh, self.V, self.tags, self.c0, self.rho0, self.dt = build(geom, P, dtype)
        self.points = p = Points(self.mesh, self.V.nodes1d)
        self.u = field_random(self.V).astype(dtype)
        self.v = field_smooth(self.V).astype(dtype)
        # what set_receivers hands to the library: the located (cell, X) of the inside points (a point that is not
        # found keeps its constructed pair here; test_receivers_host.py asserts that there is none)
        from fenicsxfus_amd.evaluate import locate
        cell, X = locate(self.mesh, p.pts)
        self.located = (cell, X)
        found = cell[:p.n_inside] >= 0
        self.loc_cell = np.where(found, cell[:p.n_inside], p.cell)
        self.loc_X = np.where(found[:, None], X[:p.n_inside], p.X)
        self.ref, self.yard, self.kref = {}, {}, {}
        for f, a in (("u", self.u), ("v", self.v)):
            self.ref[f] = np.asarray(interp(self.V, a, p.cell, p.X, np.longdouble), dtype=np.float64)
            self.kref[f] = np.asarray(interp(self.V, a, self.loc_cell, self.loc_X, np.longdouble), dtype=np.float64)
            self.yard[f] = np.asarray(interp(self.V, a, self.loc_cell, self.loc_X, dtype), dtype=np.float64)
        for a in (self.u, self.v, p.pts, p.cell, p.X, cell, X, self.loc_cell, self.loc_X, *self.ref.values(),
                  *self.yard.values(), *self.kref.values()):
            a.setflags(write=False)

    def pair(self, d):
        return d["u"], d["v"]

    @property
    def label(self):
        return f"{self.geom}-p{self.P}"

    def model(self, ctx=None):
        import fenicsxfus_amd as fa
        nc, T = self.mesh.num_cells, self.dtype
        return fa.LinearSpectralExplicit(self.mesh, self.tags, self.P, np.full(nc, self.c0, T), np.full(nc, self.rho0, T),
                                         0.5e6, 60000.0, 1500.0, 4, self.dt, V=self.V, ctx=ctx or fa.Context(0))


def sample_case(geom, P, dtype=np.float64) -> SampleCase:
    key = (geom, P, np.dtype(dtype))
    if key not in _cases:
        _cases[key] = SampleCase(geom, P, dtype)
    return _cases[key]


# ---- the budget -----------------------------------------------------------------------------------------------------------
def budget(g, yard, ref, regions, dtype):
    return fb.budget(g, yard, ref, regions, floor=FLOOR[np.dtype(dtype)])


def check(label, g, yard, ref, regions, dtype):
    """Assert err(g, R) <= cap * max(err(yard, R), floor) in every point class R and over all points; prints the
    largest ratio and where it occurred."""
    worst, where, table = budget(g, yard, ref, regions, dtype)
    line = fb.report(f"[receivers {np.dtype(dtype).name}] {label}", worst, where, table)
    print(line)
    assert worst <= cap(dtype), f"{line} exceeds the cap {cap(dtype)}"
    return worst, where, table
