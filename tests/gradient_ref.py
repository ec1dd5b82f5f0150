"""numpy restatement of the gradient / pair-product operator (fusmi.h "gradient"), the yardstick of its tests.

Per element: the reference derivatives with ``dphi`` (one einsum per direction), J at every GLL node from the trilinear /
triquadratic (2-D: bilinear / biquadratic) map of ``mesh.geometry``, K = J^-1, W = |det J| w; the weighted sums go to the
DOFs with ``np.add.at`` and the nodal division follows.  Written once and evaluated in ``np.float32``, ``np.float64`` or
``np.longdouble`` (argument ``dtype``): the inputs are taken as given -- maps already rounded to T stay what they are -- and
promoted, every operation then runs in ``dtype``.

    gradient:  y_d[i] += sum_{(e,q)->i} c_e W_e(q) (grad x)_{e,d}(q)
    pairs:     y_d[i] += sum_{(e,q)->i} W_e(q) sum_k c_{k,e} [a_k(i) (grad b_k)_{e,d}(q) - b_k(i) (grad a_k)_{e,d}(q)]
    nodal:     g_d[i] = y_d[i] / sum_{(e,q)->i} W_e(q)
"""
import numpy as np

LETTERS = "abc"


def _basis1d(order, pts, dtype):
    """(B, dB)[m, q]: the 1-D Lagrange basis of the geometry (nodes 0, 1 or 0, 1/2, 1) and its derivative at ``pts``, formed in
    double (long double for the long-double evaluation) and rounded to ``dtype``, as the device does."""
    hi = np.longdouble if np.dtype(dtype) == np.longdouble else np.float64
    x = np.asarray(pts, dtype=hi)
    one = np.ones_like(x)
    if order == 1:
        B, dB = [1 - x, x], [-one, one]
    else:
        B = [(2 * x - 1) * (x - 1), 4 * x * (1 - x), x * (2 * x - 1)]
        dB = [4 * x - 3, 4 - 8 * x, 4 * x - 1]
    return np.array(B).astype(dtype), np.array(dB).astype(dtype)


def geometry(mesh, nodes, wts, dtype):
    """K [ncells, Nd, t, t] with K[.., j, d] = d xi_j / d x_d, and W = |det J| w [ncells, Nd]; point q = (i0, i1(, i2)) in
    tensor order, i0 along the first reference direction."""
    t = mesh.topology.dim
    gdm = np.asarray(mesh.geometry.dofmap)
    nc, nv = gdm.shape
    order = 1 if nv == 2 ** t else 2
    g = order + 1
    N = len(nodes)
    cd = np.asarray(mesh.geometry.x)[gdm][:, :, :t].astype(dtype)          # [e, n, i], n = nx + g ny + g^2 nz
    C = cd.reshape((nc,) + (g,) * t + (t,))                                  # [e, (nz,) ny, nx, i]
    B, dB = _basis1d(order, nodes, dtype)
    J = np.empty((nc,) + (N,) * t + (t, t), dtype=dtype)                     # [e, i0, i1(, i2), i, j]
    for j in range(t):
        tabs = [dB if d == j else B for d in range(t)]                       # direction d <-> node index n_d, point index i_d
        if t == 3:
            J[..., j] = np.einsum("ezyxi,xa,yb,zc->eabci", C, tabs[0], tabs[1], tabs[2])
        else:
            J[..., j] = np.einsum("eyxi,xa,yb->eabi", C, tabs[0], tabs[1])
    J = J.reshape(nc, N ** t, t, t)
    K = np.empty_like(J)
    if t == 3:
        c00 = J[:, :, 1, 1] * J[:, :, 2, 2] - J[:, :, 1, 2] * J[:, :, 2, 1]
        c01 = J[:, :, 1, 2] * J[:, :, 2, 0] - J[:, :, 1, 0] * J[:, :, 2, 2]
        c02 = J[:, :, 1, 0] * J[:, :, 2, 1] - J[:, :, 1, 1] * J[:, :, 2, 0]
        det = J[:, :, 0, 0] * c00 + J[:, :, 0, 1] * c01 + J[:, :, 0, 2] * c02
        K[:, :, 0, 0], K[:, :, 1, 0], K[:, :, 2, 0] = c00 / det, c01 / det, c02 / det
        K[:, :, 0, 1] = (J[:, :, 0, 2] * J[:, :, 2, 1] - J[:, :, 0, 1] * J[:, :, 2, 2]) / det
        K[:, :, 1, 1] = (J[:, :, 0, 0] * J[:, :, 2, 2] - J[:, :, 0, 2] * J[:, :, 2, 0]) / det
        K[:, :, 2, 1] = (J[:, :, 0, 1] * J[:, :, 2, 0] - J[:, :, 0, 0] * J[:, :, 2, 1]) / det
        K[:, :, 0, 2] = (J[:, :, 0, 1] * J[:, :, 1, 2] - J[:, :, 0, 2] * J[:, :, 1, 1]) / det
        K[:, :, 1, 2] = (J[:, :, 0, 2] * J[:, :, 1, 0] - J[:, :, 0, 0] * J[:, :, 1, 2]) / det
        K[:, :, 2, 2] = (J[:, :, 0, 0] * J[:, :, 1, 1] - J[:, :, 0, 1] * J[:, :, 1, 0]) / det
    else:
        det = J[:, :, 0, 0] * J[:, :, 1, 1] - J[:, :, 0, 1] * J[:, :, 1, 0]
        K[:, :, 0, 0], K[:, :, 0, 1] = J[:, :, 1, 1] / det, -J[:, :, 0, 1] / det
        K[:, :, 1, 0], K[:, :, 1, 1] = -J[:, :, 1, 0] / det, J[:, :, 0, 0] / det
    w = np.asarray(wts, dtype=np.float64)
    w3 = w
    for _ in range(t - 1):
        w3 = np.multiply.outer(w3, w)
    W = np.abs(det) * w3.reshape(-1).astype(dtype)[None, :]
    return K, W


class GradientRef:
    """The operator on one mesh and space: ``dm`` the tensor dofmap [ncells, Nd], ``D`` = dphi[q, i] = phi_i'(x_q), ``nodes``
    / ``wts`` the 1-D points and weights, all in the caller's node order."""

    def __init__(self, mesh, dm, nodes, wts, D, ndofs, dtype):
        self.dtype = np.dtype(dtype)
        self.t = mesh.topology.dim
        self.dm = np.asarray(dm)
        self.N, self.ndofs, self.nc = len(nodes), int(ndofs), self.dm.shape[0]
        self.D = np.asarray(D).astype(dtype)
        self.K, self.W = geometry(mesh, nodes, wts, dtype)

    def ref_grad(self, x):
        """[ncells, Nd, t]: the reference derivatives of the field at every node of every element."""
        t, N = self.t, self.N
        U = np.asarray(x).astype(self.dtype)[self.dm].reshape((self.nc,) + (N,) * t)
        out = np.empty((self.nc, N ** t, t), dtype=self.dtype)
        idx = LETTERS[:t]
        for j in range(t):
            src = idx.replace(idx[j], "m")
            out[:, :, j] = np.einsum(f"{idx[j]}m,e{src}->e{idx}", self.D, U).reshape(self.nc, -1)
        return out

    def _scatter(self, r):
        """r [ncells, Nd, t] in reference directions -> the weighted sums [t, ndofs] of W K^T r."""
        g = np.einsum("eqjd,eqj->eqd", self.K, r) * self.W[:, :, None]
        y = np.zeros((self.t, self.ndofs), dtype=self.dtype)
        for d in range(self.t):
            np.add.at(y[d], self.dm, g[:, :, d])
        return y

    def denominator(self):
        den = np.zeros(self.ndofs, dtype=self.dtype)
        np.add.at(den, self.dm, self.W)
        return den

    def _coef(self, c, rows):
        if c is None:
            return np.ones((rows, self.nc), dtype=self.dtype)
        return np.atleast_2d(np.asarray(c)).astype(self.dtype)

    def gradient(self, x, coeffs=None, nodal=True):
        c = self._coef(coeffs, 1)[0]
        y = self._scatter(c[:, None, None] * self.ref_grad(x))
        return y / self.denominator()[None, :] if nodal else y

    def gradient_pairs(self, a, b, coeffs, nodal=True):
        a, b = np.atleast_2d(np.asarray(a)).astype(self.dtype), np.atleast_2d(np.asarray(b)).astype(self.dtype)
        c = self._coef(coeffs, a.shape[0])
        r = np.zeros((self.nc, self.N ** self.t, self.t), dtype=self.dtype)
        for k in range(a.shape[0]):
            r += c[k][:, None, None] * (a[k][self.dm][:, :, None] * self.ref_grad(b[k])
                                        - b[k][self.dm][:, :, None] * self.ref_grad(a[k]))
        y = self._scatter(r)
        return y / self.denominator()[None, :] if nodal else y


def of_problem(pr, dtype, orc=None):
    """The reference on a util.Problem; ``D`` from the oracle's dphi (double)."""
    orc = orc or pr.orc
    return GradientRef(pr.mesh, pr.dm, pr.nodes, pr.wts, orc.dphi(pr.nodes), pr.ndofs, dtype)


class Quad2Problem:
    """An (nx, ny) box of second-order (9-node) quadrilaterals, bent by ``warp(x) -> x'`` (x: [nnodes, 2]), with the
    attributes of util.Problem that the gradient tests use (BoxMesh builds second-order cells for hexahedra only)."""

    def __init__(self, orc, n, P, hi=(1.0, 1.0), warp=None, dtype=np.float64):
        from fenicsxfus_amd import HexFunctionSpace, QuadMesh

        nx, ny = n
        gx, gy = np.meshgrid(np.linspace(0.0, hi[0], 2 * nx + 1), np.linspace(0.0, hi[1], 2 * ny + 1), indexing="ij")
        x = np.c_[gx.ravel(), gy.ravel()]                                    # node (ix, iy) -> ix (2 ny + 1) + iy
        if warp is not None:
            x = np.asarray(warp(x), dtype=np.float64)
        cx, cy = [a.ravel() for a in np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")]
        a, b = [v.ravel() for v in np.meshgrid(np.arange(3), np.arange(3), indexing="xy")]   # n = a + 3 b
        cells = (2 * cx[:, None] + a[None, :]) * (2 * ny + 1) + 2 * cy[:, None] + b[None, :]
        self.mesh = QuadMesh(x, cells.astype(np.int32), dtype=dtype)
        self.V = HexFunctionSpace(self.mesh, P)
        self.P, self.N, self.tdim, self.dtype, self.orc = P, P + 1, 2, np.dtype(dtype), orc
        self.nodes = self.V.nodes1d
        self.wts = orc.gll_weights_at(self.nodes)
        self.dm, self.ndofs = self.V.tensor_dofmap, self.V.num_dofs
        self.G, self.detJ = orc.geometry(2, self.mesh.geometry.x, self.mesh.geometry.dofmap, self.nodes, self.wts, dtype=dtype)


# ---- the error measure of fp32_budget.py, per component and for the whole vector ----
def errors(g, hi):
    """{"<d>": rms/rms, "<d>:max": max/max for every component d, "all", "all:max" for the whole vector} of g against hi."""
    g, hi = np.asarray(g, dtype=np.longdouble), np.asarray(hi, dtype=np.longdouble)
    assert g.shape == hi.shape and np.isfinite(g.astype(np.float64)).all(), "result not finite or of another shape"
    out = {}
    rows = {"xyz"[d]: (g[d], hi[d]) for d in range(g.shape[0])}
    rows["all"] = (g.reshape(-1), hi.reshape(-1))
    for name, (a, r) in rows.items():
        d = a - r
        out[name] = float(np.sqrt(np.mean(d * d)) / np.sqrt(np.mean(r * r)))
        out[name + ":max"] = float(np.abs(d).max() / np.abs(r).max())
    return out


def budget(g, ref_T, ref_hi, ulp):
    """(largest ratio err(g) / yard, where, {measure: (err, yard)}) with yard = max(err(ref_T, ref_hi), ulp)."""
    e, y = errors(g, ref_hi), errors(ref_T, ref_hi)
    table = {k: (e[k], max(y[k], ulp)) for k in e}
    where = max(table, key=lambda k: table[k][0] / table[k][1])
    return table[where][0] / table[where][1], where, table
