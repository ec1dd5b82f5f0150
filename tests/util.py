"""Shared problem builders for the tests (inputs follow SURVEY 8d / the reference tests' recipes)."""
import functools
import subprocess
import sys

import numpy as np

from fenicsxfus_amd import BoxMesh, FunctionSpace, FacetTags


@functools.lru_cache(maxsize=None)
def gpu_present() -> bool:
    """torch.cuda.is_available(), asked in a child interpreter: torch's HIP runtime must not be loaded into a test
    process that holds libfusmi's (the in-process GPU tests then find no device)."""
    return subprocess.run([sys.executable, "-c", "import sys, torch; sys.exit(0 if torch.cuda.is_available() else 1)"],
                          capture_output=True).returncode == 0


class Problem:
    """Everything the oracle needs for one mesh: tables, geometry factors, dofmap."""

    def __init__(self, orc, n, P, lo=None, hi=None, perturb=0.0, node_order=None, dtype=np.float64,
                 rank=0, size=1, order=1, warp=None):
        t = len(n)
        lo = [0.0] * t if lo is None else lo
        hi = [1.0] * t if hi is None else hi
        self.mesh = BoxMesh(lo, hi, n, perturb=perturb, dtype=dtype, rank=rank, size=size, order=order, warp=warp)
        self.V = FunctionSpace(self.mesh, P, node_order=node_order)
        self.P, self.N, self.tdim, self.dtype = P, P + 1, t, np.dtype(dtype)
        self.nodes = self.V.nodes1d
        self.wts = orc.gll_weights_at(self.nodes)
        self.D = orc.dphi(self.nodes).astype(dtype)
        self.dm = self.V.tensor_dofmap
        self.ndofs = self.V.num_dofs
        self.G, self.detJ = orc.geometry(t, self.mesh.geometry.x, self.mesh.geometry.dofmap, self.nodes,
                                         self.wts, dtype=dtype)
        self.orc = orc

    def K(self, x, coeffs=None, dense=False, fast=False):
        c = np.ones(self.mesh.num_cells, self.dtype) if coeffs is None else coeffs
        y = np.zeros(self.ndofs, self.dtype)
        return self.orc.stiffness(self.tdim, self.N, self.dm, self.G, self.D, c, x, y, dtype=self.dtype,
                                  dense=dense, fast=fast)

    def M(self, x, coeffs=None):
        c = np.ones(self.mesh.num_cells, self.dtype) if coeffs is None else coeffs
        y = np.zeros(self.ndofs, self.dtype)
        return self.orc.mass(self.tdim, self.N, self.dm, self.detJ, c, x, y, dtype=self.dtype)

    def facet_diag(self, tags: FacetTags, tag, cellcoef):
        sel = tags.find(tag)
        return self.orc.facet_diag(self.tdim, tags.cells[sel], tags.local_facets[sel], cellcoef,
                                   self.mesh.geometry.x, self.mesh.geometry.dofmap, self.nodes, self.wts,
                                   self.dm, self.ndofs, dtype=self.dtype)

    def linear_model_vectors(self, c0, rho0, tags):
        """m, src, absb, coeff of the Linear model (Linear.hpp:127-134,154-155; forms.py:36-39)."""
        nc = self.mesh.num_cells
        c0 = np.broadcast_to(np.asarray(c0, self.dtype), (nc,)).copy()
        rho0 = np.broadcast_to(np.asarray(rho0, self.dtype), (nc,)).copy()
        m = self.M(np.ones(self.ndofs, self.dtype), 1.0 / (rho0 * c0 * c0))
        src = self.facet_diag(tags, 1, 1.0 / rho0)
        absb = self.facet_diag(tags, 2, 1.0 / (rho0 * c0))
        return m, src, absb, (-1.0 / rho0).astype(self.dtype)

    def lossy_model_vectors(self, c0, rho0, delta0, tags):
        """m, src, absb, src2, lin_coeff, att_coeff of the Lossy model (Lossy.hpp:133-141,166-169;
        BM7-SC1/forms.py:37-42): absorbing + delta mass term on every listed boundary facet."""
        nc = self.mesh.num_cells
        c0 = np.broadcast_to(np.asarray(c0, self.dtype), (nc,)).copy()
        rho0 = np.broadcast_to(np.asarray(rho0, self.dtype), (nc,)).copy()
        d0 = np.broadcast_to(np.asarray(delta0, self.dtype), (nc,)).copy()
        allf = FacetTags(tags.cells, tags.local_facets, np.full(len(tags.values), 7))
        m = self.M(np.ones(self.ndofs, self.dtype), 1.0 / (rho0 * c0 * c0))
        m = m + self.facet_diag(allf, 7, d0 / (rho0 * c0**3))
        src = self.facet_diag(tags, 1, 1.0 / rho0)
        absb = self.facet_diag(allf, 7, 1.0 / (rho0 * c0))
        src2 = self.facet_diag(tags, 1, d0 / (rho0 * c0 * c0))
        return m, src, absb, src2, (-1.0 / rho0).astype(self.dtype), (-d0 / (rho0 * c0 * c0)).astype(self.dtype)


# ---- live starts: every DOF of the compared state carries an O(1) value ---------------------------------------
def live_state(pr, seed, amp, f0=0.5e6):
    """(u0, v0) on the DOFs of the GLOBAL problem ``pr``: a few low-order cosine modes with random phases over the
    box plus 1 % seeded per-DOF noise, u ~ amp and v ~ 2 pi f0 amp, in the problem's dtype.  A rank takes its part
    by global offset (slabs) or by its global DOF ids, so sharers get identical values."""
    X = pr.V.tabulate_dof_coordinates()[:, :pr.tdim].astype(np.float64)
    lo, hi = X.min(axis=0), X.max(axis=0)
    xn = (X - lo) / np.where(hi > lo, hi - lo, 1.0)
    rng = np.random.default_rng(seed)
    out = []
    for scale in (amp, 2 * np.pi * f0 * amp):
        f = np.ones(len(X))
        for _ in range(4):
            k = rng.integers(0, 3, pr.tdim)
            f += rng.uniform(0.2, 0.5) * np.cos(np.pi * (xn @ k) + rng.uniform(0.0, 2 * np.pi))
        f += 0.01 * rng.standard_normal(len(X))
        out.append(np.ascontiguousarray(scale * f, dtype=pr.dtype))
    return out[0], out[1]


def layer_and_face_regions(pr):
    """Global DOF ids of every element layer along x and of each of the 2 tdim boundary faces of the box."""
    mesh = pr.mesh
    layer = mesh._cidx[0] + mesh.cx0
    regions = {f"layer{i}": np.unique(pr.dm[layer == i]) for i in range(mesh.n[0])}
    cells, lf, ax, sd = mesh.exterior_facets()
    for a in range(pr.tdim):
        for s in (0, 1):
            sel = (ax == a) & (sd == s)
            tags = FacetTags(cells[sel], lf[sel], np.ones(int(sel.sum()), np.int32))
            w = pr.facet_diag(tags, 1, np.ones(mesh.num_cells, pr.dtype))
            regions[f"face{'xyz'[a]}{'-+'[s]}"] = np.flatnonzero(w)
    return regions


def slab_interface_regions(pr, size):
    """Global DOF ids of the interface planes of ``size`` x-slabs of ``pr``'s box (what two slabs share)."""
    out = {}
    for r in range(1, size):
        mesh = BoxMesh(pr.mesh.lo, pr.mesh.hi, pr.mesh.n, rank=r, size=size)
        V = FunctionSpace(mesh, pr.P)
        nb, idx = V.neighbours[0]
        assert nb == r - 1
        out[f"cut{r - 1}|{r}"] = V.global_offset + idx.astype(np.int64)
    return out


def assert_live(ref, regions, floor=1e-2):
    """Precondition of a comparison with the oracle: every named region of the reference state carries at least
    ``floor`` of its max, so that a comparison at a relative tolerance checks that region at all."""
    for a in (ref if isinstance(ref, (tuple, list)) else (ref,)):
        a = np.abs(np.asarray(a, dtype=np.float64))
        top = a.max()
        assert np.isfinite(top) and top > 0
        weak = {k: float(a[idx].max() / top) for k, idx in regions.items() if len(idx) == 0 or a[idx].max() < floor * top}
        assert not weak, f"reference state below {floor} of its max in {weak}"
