"""Problems of the live-start RK tests, defined once for the GPU tests (test_gpu_live_state.py) and for their CPU
guards (test_live_guards.py).  A case is a small box, one model family, materials, RK order and step count; it knows
its oracle run from any start, the regions its reference state must keep live, and the small changes of the problem
(far-face absorbing weight, last layer's coefficient) that the comparison must be able to see."""
import numpy as np

import fenicsxfus_amd as fa
from fenicsxfus_amd import tag_box_boundary
from util import Problem, layer_and_face_regions, live_state

F0, S0 = 0.5e6, 1500.0
TOL_RK = 1e-10
# fp32 against the fp32 / the fp64 oracle (test_gpu_config5_fp32.py)
TOL_F32_VS_F32, TOL_F32_VS_F64 = 1e-4, 1e-3


class Case:
    def __init__(self, orc, kind, n, P, L=0.012, perturb=0.1, nsteps=10, order=4, dtype=np.float64, mesh_order=1,
                 warp=None, seed=7, cfl=0.5, alpha=20.0):
        t = len(n)
        self.kind, self.P, self.nsteps, self.order, self.dtype, self.seed = kind, P, nsteps, order, np.dtype(dtype), seed
        self.hi = [L * k / n[0] for k in n]                 # cubic cells
        kw = dict(hi=self.hi, perturb=perturb, order=mesh_order, warp=warp)
        self.pr = Problem(orc, n, P, **kw)                   # fp64: the reference
        self.prt = self.pr if self.dtype == np.float64 else Problem(orc, n, P, dtype=dtype, **kw)
        self.tdim, self.orc = t, orc
        nc = self.pr.mesh.num_cells
        layer = self.pr.mesh._cidx[0]
        self.last_layer = layer == n[0] - 1
        bone = (layer == n[0] // 2)                         # one bone layer in the middle
        self.c = np.where(bone, 2800.0, 1500.0)
        self.rho = np.where(bone, 1850.0, 1000.0)
        w0 = 2 * np.pi * F0
        # strongly attenuating everywhere, so that a 1e-4 change of delta shows within the run
        self.delta = np.where(bone, fa.compute_diffusivity_of_sound(w0, 2800.0, 46.0),
                              fa.compute_diffusivity_of_sound(w0, 1500.0, alpha))
        self.beta = np.where(bone, 6.0, 3.5)
        self.p0 = 6e6 if kind == "westervelt" else 6e4     # Westervelt: amplitude where the nonlinearity shows
        self.tags = tag_box_boundary(self.pr.mesh)
        self.dt = cfl * (L / n[0]) / (self.c.max() * P**2)
        self.tf = nsteps * self.dt * (1 - 1e-9)
        self.regions = layer_and_face_regions(self.pr)
        # far-corner cells (the last of every axis): the negative controls change their coefficients
        cid = self.pr.mesh._cidx
        self.far_corner = np.all([cid[a] >= n[a] - 2 for a in range(t)], axis=0)
        assert 0 < self.far_corner.sum() <= 8 and nc > 0

    def start(self, seed=None):
        return live_state(self.pr, self.seed if seed is None else seed, self.p0)

    # ---- oracle ----------------------------------------------------------------------------------------------------
    def materials(self, scale_far_corner=None):
        """c0, rho0, delta0, beta0 per cell; ``scale_far_corner`` multiplies the family's own coefficient (c0 for
        Linear, delta for Lossy, beta for Westervelt) of the far-corner cells (the negative controls)."""
        c, rho, delta, beta = (a.copy() for a in (self.c, self.rho, self.delta, self.beta))
        if scale_far_corner is not None:
            a = {"linear": c, "lossy": delta, "westervelt": beta}[self.kind]
            a[self.far_corner] *= scale_far_corner
        return c, rho, delta, beta

    def vectors(self, pr, change=None, eps=1e-6, scale_far_corner=None):
        """The oracle's model vectors on ``pr``; ``change`` scales one of them by 1 + eps:
        "absb_far" the absorbing weight on the far face x = L, "coef_last" the stiffness coefficient of the last
        element layer along x."""
        c, rho, delta, beta = self.materials(scale_far_corner)
        if self.kind == "linear":
            m, src, absb, coeff = pr.linear_model_vectors(c, rho, self.tags)
            V = dict(m=m, src=src, absb=absb, coeff=coeff)
        else:
            m, src, absb, src2, lin, att = pr.lossy_model_vectors(c, rho, delta, self.tags)
            V = dict(m=m, src=src, absb=absb, src2=src2, coeff=lin, att=att)
            if self.kind == "westervelt":
                V["n1"] = (-2.0 * beta / rho**2 / c**4).astype(pr.dtype)
        if change == "absb_far":
            V["absb"] = V["absb"].copy()
            V["absb"][self.regions["facex+"]] *= 1 + eps
        elif change == "coef_last":
            V["coeff"] = np.where(self.last_layer, V["coeff"] * (1 + eps), V["coeff"]).astype(pr.dtype)
        else:
            assert change is None
        return V

    def oracle(self, u0, v0, dtype=np.float64, change=None, eps=1e-6, t0=0.0, nsteps=None, order=None,
               scale_far_corner=None, exact=False):
        """u, v after ``nsteps`` steps from (u0, v0) at t0: to tf = t0 + nsteps dt (1 - 1e-9) like model.rk(), or with
        ``exact`` to t0 + nsteps dt (1 + 1e-12), nsteps full steps like model.rk4_steps() (+ a ~1e-12 dt remainder
        step, far below the tolerance)."""
        pr = self.pr if np.dtype(dtype) == np.float64 else self.prt
        V = self.vectors(pr, change, eps, scale_far_corner)
        u, v = np.array(u0, dtype=dtype), np.array(v0, dtype=dtype)
        ns = self.nsteps if nsteps is None else nsteps
        tf = t0 + ns * self.dt * ((1 + 1e-12) if exact else (1 - 1e-9))
        a = (self.tdim, pr.N, pr.dm, pr.G)
        if self.kind == "linear":
            k = self.orc.linear_rk4(*a, pr.D, V["coeff"], V["m"], V["src"], V["absb"], F0, self.p0, S0, t0, tf,
                                    self.dt, u, v, dtype=dtype, order=self.order if order is None else order)
        elif self.kind == "lossy":
            k = self.orc.lossy_rk4(*a, pr.D, V["coeff"], V["att"], V["m"], V["src"], V["absb"], V["src2"], F0, self.p0,
                                   S0, t0, tf, self.dt, u, v, dtype=dtype)
        else:
            k = self.orc.westervelt_rk4(*a, pr.detJ, pr.D, V["coeff"], V["att"], V["n1"], -V["n1"], V["m"], V["src"],
                                        V["absb"], V["src2"], F0, self.p0, S0, t0, tf, self.dt, u, v, dtype=dtype)
        assert k == ns or (exact and k == ns + 1)
        return u, v

    # ---- GPU model ---------------------------------------------------------------------------------------------------
    def model(self, ctx, scale_far_corner=None, order=None):
        """The library's model of this case (``scale_far_corner``: see materials())."""
        pr, dt_ = self.prt, self.dtype
        c, rho, delta, beta = (np.array(a, dtype=dt_) for a in self.materials(scale_far_corner))
        o = self.order if order is None else order
        tags = tag_box_boundary(pr.mesh)
        if self.kind == "linear":
            return fa.LinearSpectralExplicit(pr.mesh, tags, self.P, c, rho, F0, self.p0, S0, o, self.dt, V=pr.V, ctx=ctx)
        if self.kind == "lossy":
            return fa.LossySpectralExplicit(pr.mesh, tags, self.P, c, rho, delta, F0, self.p0, S0, o, self.dt, V=pr.V,
                                            ctx=ctx)
        return fa.WesterveltSpectralExplicit(pr.mesh, tags, self.P, c, rho, delta, beta, F0, self.p0, S0, o, self.dt,
                                             V=pr.V, ctx=ctx)


# name -> (constructor keywords).  Non-cubic meshes so that blocks are ragged.
BOX = (6, 5, 4)
CASES = {}
for _kind in ("linear", "lossy", "westervelt"):
    CASES[f"{_kind}-p4"] = dict(kind=_kind, n=BOX, P=4)                       # perturbed: trilinear / stream
    CASES[f"{_kind}-p4-box"] = dict(kind=_kind, n=BOX, P=4, perturb=0.0)      # affine / diagonal metric
for _o in (1, 2, 3):
    CASES[f"linear-rk{_o}"] = dict(kind="linear", n=(5, 4, 4), P=3, order=_o, cfl=0.1, nsteps=20)
CASES["linear-walk"] = dict(kind="linear", n=(16, 12, 12), P=4, nsteps=10, L=0.016)
for _P in (2, 3, 5, 6, 7):
    CASES[f"linear-p{_P}"] = dict(kind="linear", n=(4, 3, 2) if _P <= 5 else (3, 2, 2), P=_P)
for _P in (8, 10):
    for _kind in ("linear", "westervelt"):
        CASES[f"{_kind}-p{_P}"] = dict(kind=_kind, n=(2, 2, 1), P=_P, nsteps=6)
for _P, _n in ((4, (5, 4, 3)), (6, (4, 3, 2))):
    CASES[f"linear-p{_P}-fp32"] = dict(kind="linear", n=_n, P=_P, dtype=np.float32)
for _P, _n in ((4, (9, 7)), (9, (4, 3))):
    for _kind in ("linear", "westervelt"):
        CASES[f"{_kind}-quad-p{_P}"] = dict(kind=_kind, n=_n, P=_P)
CASES["linear-q2"] = dict(kind="linear", n=(4, 3, 3), P=4, perturb=0.0, mesh_order=2, L=0.016,
                          warp=lambda x: x + np.c_[20.0 * x[:, 1] ** 2 - 12.0 * x[:, 2] ** 2, 15.0 * x[:, 2] ** 2,
                                                   0 * x[:, 0]])


_cache = {}


def case(orc, name) -> Case:
    if name not in _cache:
        _cache[name] = Case(orc, **CASES[name])
    return _cache[name]
