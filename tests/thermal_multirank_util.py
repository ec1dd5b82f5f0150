"""Helpers of the several-rank bioheat tests (test_gpu_thermal_multirank.py, test_thermal_multirank_host.py): the global
single-rank problem with the materials, heat and reference of thermal_ref.py, its x-slab parts and the 2 x 2 quadrant
partition of test_multirank.py, and the in-process group of thermal objects on them.  The reference is always the numpy
model on the GLOBAL problem; a rank takes its part by ``V.global_offset`` (slabs) or by its global DOF ids."""
import functools

import numpy as np

import fenicsxfus_amd as fa
from fp32_budget import promoted
from live_cases import live_state
from thermal_ref import Bioheat, box_hi, heat_field, materials
from util import Problem

TOL64, TOL32 = 1e-10, 1e-5          # BASELINE section 3: 20 RK4 steps in fp64 / fp32

# label -> cells, degree, perturbation, scalar type: the smallest shapes with interior, rank-local shared and interface
# DOFs on every rank of 2 (S3: also 3) slabs
SHAPES = {
    "S3": dict(n=(6, 3, 3), P=3, perturb=0.1, dtype=np.float64),
    "Q4": dict(n=(6, 5), P=4, perturb=0.1, dtype=np.float64),
    "F4": dict(n=(4, 3, 3), P=4, perturb=0.1, dtype=np.float32),
}


class Global:
    """The global problem of a shape, as thermal_ref.Case builds its cases: ``prt`` in the scalar type, ``pr`` the double
    problem the reference runs on, materials (``mats(mesh, hi)``: thermal_ref.materials) and heat rounded to the scalar type."""

    def __init__(self, orc, n, P, perturb, dtype, hi=None, mats=materials):
        self.n, self.P, self.perturb, self.dtype = tuple(n), P, perturb, np.dtype(dtype)
        self.hi = box_hi(n) if hi is None else hi
        self.prt = Problem(orc, n, P, hi=self.hi, perturb=perturb, dtype=self.dtype)
        self.pr = self.prt if self.dtype == np.float64 else promoted(orc, self.prt)
        self.rnd = lambda a: np.asarray(a).astype(self.dtype).astype(np.float64)   # noqa: E731
        self.k, self.rho_c, self.w = (self.rnd(a) for a in mats(self.prt.mesh, self.hi))
        self.q = self.rnd(heat_field(self.prt.V, self.hi))
        self.ref = Bioheat(self.pr, self.k, self.rho_c, self.w)
        self.h = self.ref.load(self.q)
        self.tol = TOL64 if self.dtype == np.float64 else TOL32

    @functools.cached_property
    def rho20(self):
        return self.ref.power_iteration(20)

    def start(self, seed=3, amp=5.0):
        """A rise that is live at every DOF, in the scalar type and in double."""
        u = live_state(self.prt, seed, amp)[0].astype(self.dtype)
        return u, u.astype(np.float64)


@functools.lru_cache(maxsize=None)
def shape(orc, label) -> Global:
    return Global(orc, **SHAPES[label])


class Part:
    """One rank's part of a Global: ``mesh``, ``V`` (with ``neighbours``), ``gids`` (global id of every local DOF) and
    ``cells`` (global cell of every local cell)."""

    def __init__(self, mesh, V, gids, cells):
        self.mesh, self.V, self.gids, self.cells = mesh, V, np.asarray(gids, dtype=np.int64), np.asarray(cells)


def slab_parts(g: Global, size):
    parts = []
    for r in range(size):
        mesh = fa.BoxMesh([0.0] * len(g.n), g.hi, g.n, rank=r, size=size, perturb=g.perturb, dtype=g.dtype)
        V = fa.FunctionSpace(mesh, g.P)
        gids = V.global_offset + np.arange(V.num_dofs)
        # the slab's cells in the global cell numbering: matched by centroid (the perturbation is the global mesh's)
        parts.append(Part(mesh, V, gids, _match_rows(g.prt.mesh.cell_centroids(), mesh.cell_centroids())))
    return parts


def _match_rows(big, small):
    from scipy.spatial import cKDTree
    d, i = cKDTree(np.asarray(big, dtype=np.float64)).query(np.asarray(small, dtype=np.float64))
    assert d.max() < 1e-6 * np.abs(big).max()
    return i


def quadrant_parts(g: Global):
    """The 2 x 2 partition in x-y of test_multirank.py::test_general_partition_four_quadrants_gpu: unstructured local
    meshes with their own DOF numbering, neighbour lists from global DOF identity ordered by global id; the DOFs of the
    central line are held by all four ranks."""
    from fenicsxfus_amd.unstructured import HexFunctionSpace, HexMesh
    pr = g.prt
    Xg = np.zeros((pr.ndofs, 3))
    Xg[pr.dm] = HexFunctionSpace(HexMesh(pr.mesh.geometry.x, pr.mesh.geometry.dofmap), g.P)._node_x
    cen = pr.mesh.cell_centroids()
    quad = (cen[:, 0] > 0.5 * g.hi[0]).astype(int) + 2 * (cen[:, 1] > 0.5 * g.hi[1]).astype(int)
    parts = []
    for r in range(4):
        cells = np.nonzero(quad == r)[0]
        used, inv = np.unique(pr.mesh.geometry.dofmap[cells], return_inverse=True)
        lmesh = HexMesh(pr.mesh.geometry.x[used], inv.reshape(len(cells), 8))
        V = HexFunctionSpace(lmesh, g.P)
        parts.append(Part(lmesh, V, _match_rows(Xg, V.tabulate_dof_coordinates()), cells))
    for r, p in enumerate(parts):
        mine = {int(gl): i for i, gl in enumerate(p.gids)}
        p.V.neighbours = []
        for q, other in enumerate(parts):
            shared = np.intersect1d(p.gids, other.gids)
            if q != r and len(shared):
                p.V.neighbours.append((q, np.array([mine[int(gl)] for gl in shared], dtype=np.int32)))
        assert len(p.V.neighbours) == 3
    return parts


def interface_ids(parts):
    """{(r, q): global ids both ranks hold} for r < q."""
    out = {}
    for r in range(len(parts)):
        for q in range(r + 1, len(parts)):
            s = np.intersect1d(parts[r].gids, parts[q].gids)
            if len(s):
                out[(r, q)] = s
    return out


class Group:
    """Thermal objects of the parts of ``g`` in an in-process group of deterministic contexts."""

    def __init__(self, g: Global, parts, heat=True, profile=False):
        t = g.dtype
        self.g, self.parts = g, parts
        self.ctxs = [fa.Context(0, deterministic=True) for _ in parts]
        fa.Context.init_local_group(self.ctxs)
        if profile:
            for c in self.ctxs:
                c.profile_enable(True)
        self.bios = [fa.BioheatSpectralExplicit(p.mesh, g.P, g.k[p.cells].astype(t), g.rho_c[p.cells].astype(t),
                                                g.w[p.cells].astype(t), V=p.V, ctx=c) for p, c in zip(parts, self.ctxs)]
        if heat:
            for b, p in zip(self.bios, parts):
                b.set_heat(g.q[p.gids].astype(t))

    def finish(self):
        fa.group_thermal_finish(self.bios)

    def set_rise(self, th):
        for b, p in zip(self.bios, self.parts):
            b.set_state(rise=np.ascontiguousarray(th[p.gids]))

    def steps(self, dt, n, **kw):
        fa.group_thermal_steps(self.bios, dt, n, **kw)

    def pull(self, what="rise"):
        return [getattr(b, what)().x.array.copy() for b in self.bios]

    def close(self):
        for b in self.bios:
            b.close()
        for c in self.ctxs:
            c.close()


def worst_rel(g, parts, got, ref):
    """max over the ranks of max|got_r - ref[gids_r]| / max|ref|."""
    top = np.abs(ref).max()
    return max(float(np.abs(np.asarray(a, dtype=np.float64) - ref[p.gids]).max() / top) for a, p in zip(got, parts))


def assert_interfaces_identical(parts, *fields):
    """Every field (a list of per-rank arrays) carries the same bits on every DOF two ranks hold."""
    pairs = interface_ids(parts)
    assert pairs
    for (r, q), ids in pairs.items():
        lr = {int(gl): i for i, gl in enumerate(parts[r].gids)}
        lq = {int(gl): i for i, gl in enumerate(parts[q].gids)}
        ir, iq = [lr[int(gl)] for gl in ids], [lq[int(gl)] for gl in ids]
        for f in fields:
            assert np.array_equal(f[r][ir], f[q][iq]), (r, q)
