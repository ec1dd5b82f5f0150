"""The 2 x 2 partition in x-y of test_multirank.py::test_general_partition_four_quadrants_gpu as a builder: every rank an
unstructured local mesh with its own (geometric) DOF numbering, neighbour lists built from global DOF identity and
ordered by it.  Interface faces are no contiguous index ranges, and the DOFs on the central line are held by all four
ranks."""
import numpy as np

import fenicsxfus_amd as fa
from fenicsxfus_amd.unstructured import HexFunctionSpace, HexMesh

SIZE = 4


class Part:
    """One rank's part: the global ids of its cells, its local mesh, space (neighbours set), facet tags and the global
    DOF id of every local DOF."""

    def __init__(self, cells, mesh, V, tags, gids):
        self.cells, self.mesh, self.V, self.tags, self.gids = cells, mesh, V, tags, gids


def quadrant_parts(pr, gtags):
    """The four parts of the global problem ``pr`` (util.Problem on a first-order hexahedral box) with the global
    boundary tags ``gtags``."""
    from scipy.spatial import cKDTree

    P = pr.P
    x, dofmap = pr.mesh.geometry.x, pr.mesh.geometry.dofmap
    # true (mapped) positions of the global dofs: the same trilinear map the local spaces use
    Xg = np.zeros((pr.ndofs, 3))
    Xg[pr.dm] = HexFunctionSpace(HexMesh(x, dofmap), P)._node_x
    tree = cKDTree(Xg)
    hi = x.max(axis=0)
    cen = pr.mesh.cell_centroids()
    quad = (cen[:, 0] > 0.5 * hi[0]).astype(int) + 2 * (cen[:, 1] > 0.5 * hi[1]).astype(int)
    parts = []
    for r in range(SIZE):
        cells = np.nonzero(quad == r)[0]
        used, inv = np.unique(dofmap[cells], return_inverse=True)
        lmesh = HexMesh(x[used], inv.reshape(len(cells), 8))
        V = HexFunctionSpace(lmesh, P)
        d, gids = tree.query(V.tabulate_dof_coordinates())
        assert d.max() < 1e-9 * hi.max() and len(np.unique(gids)) == len(gids)
        # global-boundary facets of this rank's cells, as (local cell, local facet, tag)
        loc_of = {g: i for i, g in enumerate(cells)}
        sel = np.isin(gtags.cells, cells)
        tags = fa.FacetTags(np.array([loc_of[g] for g in gtags.cells[sel]], np.int32), gtags.local_facets[sel],
                            gtags.values[sel])
        parts.append(Part(cells, lmesh, V, tags, gids))
    for r, p in enumerate(parts):       # neighbour lists: shared global dofs, ordered by global id on both sides
        p.V.neighbours = []
        mine = {g: i for i, g in enumerate(p.gids)}
        for q in range(SIZE):
            shared = np.intersect1d(p.gids, parts[q].gids) if q != r else []
            if len(shared):
                p.V.neighbours.append((q, np.array([mine[g] for g in shared], dtype=np.int32)))
        assert len(p.V.neighbours) == 3                   # every quadrant touches the central line
    return parts


def shared_sets(parts):
    """{"if<r>|<q>": global DOF ids that the ranks r < q both hold}."""
    return {f"if{r}|{q}": np.intersect1d(parts[r].gids, parts[q].gids)
            for r in range(len(parts)) for q in range(r + 1, len(parts))}


def held_by_all(parts):
    out = parts[0].gids
    for p in parts[1:]:
        out = np.intersect1d(out, p.gids)
    return out
