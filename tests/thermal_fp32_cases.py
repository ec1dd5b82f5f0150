"""The fp32 bioheat cases held to the float reference's own rounding error (fp32_budget.py), defined once for the GPU
tests (test_gpu_thermal_fp32_budget.py) and for their CPU guards (test_thermal_fp32_guards.py).

A case is a small mesh with the materials, heat field and start of thermal_ref.Case (bone where the centroid's x lies in
(0.4, 0.6) of the box, Gaussian heat, util.live_state of amplitude 5 K), all rounded to float.  It knows

* ``r32``: thermal_ref.Bioheat / sts_ref / thermal_bc_ref.BioheatBC instantiated in float on those inputs -- a plain
  sequential loop with every scalar rounded where the library rounds it;
* ``r64``: the same classes in double on the same inputs promoted (fp32_budget.promoted);
* its regions: every element layer along x and every boundary face (util.layer_and_face_regions), plus the interface
  planes (util.slab_interface_regions) for the cases that the GPU tests run as x-slabs;
* the small changes of the problem that the comparison must be able to see (``CONTROLS``).

A stepper is a tuple of segments (stages, steps), stages = 0 for RK4: ``RK4`` is 20 steps at 2 / rho_20, ``S(s, n)`` n RKL2
steps of s stages at 0.72 beta_s / rho_20, and a boundary case follows its 20 RK4 steps by ``S(5, 6)`` from their end.
rho_20 is the double reference's Rayleigh quotient, of the boundary operator where the case has a boundary.

Two fields are compared: the rise after the run, and the heat load h = (M(1) 1) .* q (the budget's "u" and "v")."""
import copy

import numpy as np

import fenicsxfus_amd as fa
import sts_ref
from fp32_budget import promoted
from live_cases import CASES as LIVE_CASES
from live_cases import _hex_n
from thermal_bc_ref import CONV_X, CONV_Y, FIXED, THETA_EXT, Boundary
from thermal_ref import BONE, H_CELL, Bioheat, heat_field, materials
from util import Problem, layer_and_face_regions, live_state, slab_interface_regions

# Every single-rank box is 18 mm long, as live_cases keeps its boxes' length: thermal_ref's 3 mm cells at degrees up to 4,
# 6 mm and 9 mm cells at the degrees whose meshes have 3 and 2 cells along x (2 mm and 4.5 mm quadrilaterals).  With 3 mm
# cells at every degree the stable step shrinks like P^-4, to a few milliseconds at degree 8-10, and perfusion (time
# constant rho C / W = 94 s) then changes a step by less than the float scheme loses in it: a 1e-3 change of m_W stayed at
# 3-6 x yard under RKL2, however long the run (measured: s = 8 at degree 10, 5 to 40 steps, ratio 3.1-3.3 throughout,
# because the yardstick of s = 8 grows in proportion to the number of steps as well).  The slab cases keep the 3 mm cells
# of thermal_multirank_util's shapes.
BOX = 0.018
TOL32 = 1e-5                         # the fixed bound of the existing fp32 thermal tests, asserted beside the budget
RK4 = ((0, 20),)


def S(s, n=5):
    return ((s, n),)


def stepper_name(stepper):
    return "+".join(f"rk4x{n}" if s == 0 else f"s{s}x{n}" for s, n in stepper)


# the boundary the interface cuts (test_gpu_thermal_multirank.py::test_boundaries_cut_by_the_interface)
FIX_X, FIX_Z, CUT_CONV_Y = 1, 2, 3
CUT_FACES = {FIX_X: (0, 0), FIX_Z: (2, 0), CUT_CONV_Y: (1, 0)}

BC_STEPPERS = (RK4, RK4 + S(5, 6))
CASES = {}     # name -> keywords of Case
for _P in range(2, 11):              # the shapes of the fp32 wave matrix: trilinear / stream, and diagonal metric / affine
    _st = (RK4, S(2), S(8)) + ((S(32),) if _P in (4, 7) else ())
    CASES[f"hex-p{_P}"] = dict(n=_hex_n(_P), P=_P, steppers=_st)
    CASES[f"hex-p{_P}-box"] = dict(n=_hex_n(_P), P=_P, perturb=0.0, steppers=(RK4, S(2), S(8)))
CASES["quad-p4"] = dict(n=(9, 7), P=4, steppers=(RK4, S(2), S(8), S(32)))
CASES["quad-p9"] = dict(n=(4, 3), P=9, steppers=(RK4, S(2), S(8)))
_q2 = LIVE_CASES["linear-q2"]       # second-order hexahedra, bent
CASES["hex-q2"] = dict(n=_q2["n"], P=_q2["P"], perturb=0.0, mesh_order=2, warp=_q2["warp"],
                       hi=[_q2["L"] * k / _q2["n"][0] for k in _q2["n"]], steppers=(RK4, S(2), S(8)))
PLAIN = list(CASES)
# a convective and a fixed face as test_gpu_thermal_bc.py sets them (thermal_bc_ref.standard)
CASES["hex-p4-bc"] = dict(n=_hex_n(4), P=4, boundary="standard", steppers=BC_STEPPERS)
CASES["hex-p8-bc"] = dict(n=_hex_n(8), P=8, boundary="standard", steppers=BC_STEPPERS)
CASES["quad-p4-bc"] = dict(n=(9, 7), P=4, boundary="standard", steppers=BC_STEPPERS)
BOUNDARY = [k for k in CASES if k.endswith("-bc")]
# x-slabs in an in-process group: thermal_multirank_util's "F4", and its "S3" in fp32 with two and three slabs
_slab_st = (RK4, S(2, 6), S(5, 6), S(8, 6))
for _name, _n, _P, _size in (("F4-2", (4, 3, 3), 4, 2), ("S3-2", (6, 3, 3), 3, 2), ("S3-3", (6, 3, 3), 3, 3)):
    CASES[f"slabs-{_name}"] = dict(n=_n, P=_P, slabs=_size, h_cell=H_CELL, steppers=_slab_st)
    CASES[f"slabs-{_name}-cut"] = dict(n=_n, P=_P, slabs=_size, h_cell=H_CELL, boundary="cut", steppers=BC_STEPPERS)
SLABS = [k for k in CASES if k.startswith("slabs-")]

# ---- negative controls --------------------------------------------------------------------------------------------------
# change -> what the float reference is run with:
#   "k_far"    the conductivity of the far-corner cells (the last two of every axis) scaled by 1 + eps
#   "mw_last"  m_W at the DOFs of the last element layer along x scaled by 1 + eps
#   "heat"     the heat scale sigma = 1 + eps
#   "h_c"      m_H of the convective faces scaled by 1 + eps                                      (boundary cases)
#   "drop"     the part of the last slab in b = K(-k) Theta at one DOF of its interface plane left out in one stage
#              (the first of the last step); no eps                                                (slab cases)
# EPS[change][stepper]: the smallest power of ten at which the changed run lands above 10 x yard(R) -- CAP_CEILING with a
# quarter of headroom, so that the guard does not hang on the last digit of a ratio -- in at least one region of EVERY
# case that runs the stepper.  Measured on the CPU; behind each value the smallest ratio over those cases at that eps
# (test_thermal_fp32_guards.py prints them all).  The guards hold eps to at most 1e-3, and 1e-2 for s = 32.
CONTROLS = ("k_far", "mw_last", "heat")
EPS_LIMIT = {32: 1e-2}               # by the largest stage count of the stepper; everything else 1e-3
EPS = {
    "k_far": {"rk4x20": 1e-4,          # 35.4
              "s2x5": 1e-4,            # 13.9
              "s8x5": 1e-3,            # 42.8
              "s32x5": 1e-3,           # 21.2
              "rk4x20+s5x6": 1e-4,     # 17.7
              "s2x6": 1e-4,            # 63.2
              "s5x6": 1e-4,            # 25.5
              "s8x6": 1e-4},           # 26.6
    "mw_last": {"rk4x20": 1e-3,        # 67.2
                "s2x5": 1e-3,          # 13.3
                "s8x5": 1e-3,          # 12.9
                "s32x5": 1e-3,         # 36.2
                "rk4x20+s5x6": 1e-3,   # 26.9
                "s2x6": 1e-3,          # 91.5
                "s5x6": 1e-3,          # 50.2
                "s8x6": 1e-3},         # 65.5
    "heat": {"rk4x20": 1e-5,           # 42.6
             "s2x5": 1e-5,             # 11.5
             "s8x5": 1e-4,             # 52.9
             "s32x5": 1e-4,            # 24.3
             "rk4x20+s5x6": 1e-4,      # 66.8
             "s2x6": 1e-5,             # 43.0
             "s5x6": 1e-4,             # 97.4
             "s8x6": 1e-4},            # 71.4
    "h_c": {"rk4x20": 1e-5,            # 80.5
            "rk4x20+s5x6": 1e-5},      # 10.9
}
# "drop" lands at 770 x yard(R) or above on every slab case and stepper.


def eps_limit(stepper):
    return EPS_LIMIT.get(max(s for s, _ in stepper), 1e-3)


class Case:
    """Duck-typed like thermal_multirank_util.Global (n, P, hi, perturb, dtype, prt, pr, k, rho_c, w, q), so that
    slab_parts, Group and thermal_bc_ref.Boundary take it."""

    def __init__(self, orc, name, n, P, steppers, perturb=0.1, mesh_order=1, warp=None, hi=None, boundary=None, slabs=0,
                 h_cell=None):
        self.name, self.n, self.P, self.perturb, self.steppers = name, tuple(n), P, perturb, steppers
        self.mesh_order, self.slabs, self.tdim = mesh_order, slabs, len(n)
        self.dtype = np.dtype(np.float32)
        h_cell = BOX / n[0] if h_cell is None else h_cell
        self.hi = [h_cell * k for k in n] if hi is None else hi
        # BoxMesh moves interior vertices only
        assert not perturb or all(k >= 2 for k in n)
        self.prt = Problem(orc, n, P, hi=self.hi, perturb=perturb, dtype=np.float32, order=mesh_order, warp=warp)
        self.pr = promoted(orc, self.prt)
        rnd = lambda a: np.asarray(a).astype(np.float32).astype(np.float64)   # noqa: E731
        self.k, self.rho_c, self.w = (rnd(a) for a in materials(self.prt.mesh, self.hi))
        self.q = rnd(heat_field(self.prt.V, self.hi))
        self.th0 = live_state(self.prt, 3, 5.0)[0].astype(np.float32)
        self.regions = layer_and_face_regions(self.pr)
        if slabs:
            self.regions.update(slab_interface_regions(self.pr, slabs))
        cid = self.prt.mesh._cidx
        self.far_corner = np.all([cid[a] >= n[a] - 2 for a in range(self.tdim)], axis=0)
        assert 0 < self.far_corner.sum() <= 8
        self.last_layer = self.regions[f"layer{n[0] - 1}"]
        self.bd = self._boundary(boundary)
        self.bio64 = self._bio(np.float64)
        self.bio32 = self._bio(np.float32)
        self.h64, self.h32 = self.bio64.load(self.q), self.bio32.load(self.q)
        self.rho20 = self.bio64.power_iteration(20)
        self._refs = {}

    # ---- the references ---------------------------------------------------------------------------------------------------
    def _boundary(self, kind):
        if kind is None:
            return None
        y = self.prt.V.tabulate_dof_coordinates()[:, 1].astype(np.float64)
        rise = 2.0 + np.sin(40.0 * y)            # nonzero everywhere: the fixed face is a region of the comparison
        if kind == "standard":                   # thermal_bc_ref.standard
            bone = materials(self.prt.mesh, self.hi)[0] == BONE["k"]
            return Boundary(self, {FIXED: (0, 0), CONV_X: (0, 1), CONV_Y: (1, 0)}, fixed={FIXED: rise},
                            convective={CONV_X: (np.where(bone, 200.0, 500.0), THETA_EXT), CONV_Y: (300.0, THETA_EXT)})
        assert kind == "cut"
        return Boundary(self, CUT_FACES, fixed={FIX_X: rise, FIX_Z: rise}, convective={CUT_CONV_Y: (500.0, THETA_EXT)})

    def _bio(self, dtype, k=None, h_c_scale=1.0):
        k = self.k if k is None else k
        if dtype == np.float64:
            return Bioheat(self.pr, k, self.rho_c, self.w) if self.bd is None else self.bd.ref(self)
        if self.bd is None:
            return Bioheat(self.prt, k, self.rho_c, self.w)
        return self.bd.ref_t(self, k=k, h_c_scale=h_c_scale)

    def dt(self, stages):
        return 2.0 / self.rho20 if stages == 0 else sts_ref.stable_dt(self.rho20, stages)

    def advance(self, bio, h, stepper, sigma=1.0):
        th = bio.impose(self.th0) if self.bd is not None else bio.vec(self.th0)
        for s, n in stepper:
            th = bio.run(th, self.dt(s), n, h, sigma) if s == 0 else sts_ref.run(bio, th, self.dt(s), n, s, h, sigma)
        return th

    def refs(self, stepper):
        """(r32, r64) of the rise after ``stepper`` from the start ``th0`` (the fixed values imposed), heat on."""
        if stepper not in self._refs:
            r32, r64 = self.advance(self.bio32, self.h32, stepper), self.advance(self.bio64, self.h64, stepper)
            assert r32.dtype == np.float32 and r64.dtype == np.float64
            self._refs[stepper] = (r32, r64)
        return self._refs[stepper]

    def changed(self, stepper, change, eps=None):
        """The float reference's rise with one of the CONTROLS' changes."""
        one = 1.0 + (eps or 0.0)
        if change == "heat":
            return self.advance(self.bio32, self.h32, stepper, sigma=one)
        if change == "k_far":
            return self.advance(self._bio(np.float32, k=np.where(self.far_corner, self.k * one, self.k)), self.h32, stepper)
        if change == "h_c":
            return self.advance(self._bio(np.float32, h_c_scale=one), self.h32, stepper)
        bio = copy.copy(self.bio32)
        if change == "mw_last":
            scale = np.ones(self.prt.ndofs)
            scale[self.last_layer] = one
            bio.m_w = (bio.m_w.astype(np.float64) * scale).astype(np.float32)
            return self.advance(bio, self.h32, stepper)
        assert change == "drop" and self.slabs
        # the cells of the last slab, and a free DOF in the middle of its interface plane
        mesh = fa.BoxMesh([0.0] * self.tdim, self.hi, self.n, rank=self.slabs - 1, size=self.slabs)
        theirs = self.prt.mesh._cidx[0] >= mesh.cx0
        plane = self.regions[f"cut{self.slabs - 2}|{self.slabs - 1}"]
        if self.bd is not None:
            plane = plane[~self.bd.mask[plane]]
        dof = int(plane[len(plane) // 2])
        # the first stage of the last step: an early stage's trace at one DOF has diffused away by the end of the run
        last = sum(n * (s or 4) for s, n in stepper) - (stepper[-1][0] or 4)
        whole, calls = bio.b, [0]

        def b(theta):
            out = whole(theta)
            if calls[0] == last:
                part = self.prt.K(theta, np.where(theirs, -bio.k, 0.0).astype(np.float32))
                assert part[dof] != 0
                out[dof] -= part[dof]
            calls[0] += 1
            return out

        bio.b = b
        return self.advance(bio, self.h32, stepper)

    def controls(self):
        return CONTROLS + (("h_c",) if self.bd is not None else ()) + (("drop",) if self.slabs else ())

    # ---- the library ------------------------------------------------------------------------------------------------------
    def model(self, ctx):
        """The library's thermal object of this case on one rank: heat load set, boundary set, start set."""
        t = np.float32
        th = fa.BioheatSpectralExplicit(self.prt.mesh, self.P, self.k.astype(t), self.rho_c.astype(t), self.w.astype(t),
                                        V=self.prt.V, ctx=ctx)
        th.set_heat(self.q.astype(t))
        if self.bd is not None:
            self.bd.apply(th)
        return th

    def expected_mode(self):
        if self.tdim == 2 or self.mesh_order == 2:
            return "stream"
        return "trilinear" if self.perturb > 0 else "affine"


_cache = {}


def case(orc, name) -> Case:
    if name not in _cache:
        _cache[name] = Case(orc, name, **CASES[name])
    return _cache[name]


def case_steppers(names=None):
    """[(case, stepper)] of the table, for parametrize."""
    return [(k, st) for k in (CASES if names is None else names) for st in CASES[k]["steppers"]]
