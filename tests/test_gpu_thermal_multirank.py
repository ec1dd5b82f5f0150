"""The bioheat model on several ranks (fusmi.h "bioheat", several ranks; fenicsxfus_amd.thermal group_thermal_*): mesh
parts in an in-process group on one device, against the numpy references of thermal_ref.py, sts_ref.py and
thermal_bc_ref.py run on the GLOBAL single-rank problem.

(1) the RK4 stepper across interfaces; (2) RKL2; (3) four sharers of one line of DOFs; (4) boundaries that an interface
cuts; (5) the step rule; (6) the heat load handed over from the field monitor of slab wave models; (7) the call sequence,
and the single-rank path's launches."""
import numpy as np
import pytest

import fenicsxfus_amd as fa
import sts_ref
import thermal_ref
from thermal_bc_ref import T_BASE, THETA_EXT, Boundary
from thermal_multirank_util import (TOL64, Global, Group, assert_interfaces_identical, quadrant_parts, shape, slab_parts,
                                    worst_rel)
from thermal_ref import rel

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -53


# ---- (1) RK4 across interfaces ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("label,size", [("S3", 2), ("S3", 3), ("Q4", 2), ("F4", 2)])
def test_rk4_across_interfaces(orc, label, size):
    """20 steps of dt = 2 / rho_20 from a live rise, heat on, one call each: every rank's rise within 1e-10 (fp32: 1e-5)
    of the global reference's slice in the max norm; rise and dose carry the same bits on every interface plane; the
    heat load h = (M(1) 1) .* q, whose weight is summed over the sharers like m_C and m_W, equals the reference's; one
    call of 20 steps gives the bits of 20 calls of one.  (m_C itself is checked through the state: the bone layer
    straddles the two-slab cut, so an interface DOF's m_C has different parts from the two sides.)"""
    g = shape(orc, label)
    parts = slab_parts(g, size)
    th0, th0d = g.start()
    dt = 2.0 / g.rho20
    ref = g.ref.run(th0d, dt, 20, g.h)
    grp = Group(g, parts)
    grp.finish()
    grp.set_rise(th0)
    for _ in range(20):
        grp.steps(dt, 1)
    got, D, h = grp.pull("rise"), grp.pull("dose"), grp.pull("heat")
    grp.close()
    err, herr = worst_rel(g, parts, got, ref), worst_rel(g, parts, h, g.h)
    print(f"{label}, {size} slabs: rel err after 20 steps {err:.3e}, heat load {herr:.3e} (dt = {dt:.4e} s)")
    assert all(a.dtype == g.dtype for a in got) and all(d.dtype == np.float64 for d in D)
    assert err <= g.tol
    assert herr <= (1e-12 if g.dtype == np.float64 else g.tol)
    assert rel(ref, th0d) > 1e-3                                  # the run moved the state
    assert_interfaces_identical(parts, got, D, h)
    assert min(d.min() for d in D) > 0
    grp = Group(g, parts)
    grp.finish()
    grp.set_rise(th0)
    grp.steps(dt, 20)
    again, D2 = grp.pull("rise"), grp.pull("dose")
    grp.close()
    for a, b in zip(got + D, again + D2):
        assert np.array_equal(a, b)


# ---- (2) RKL2 ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", [2, 5, 8])
def test_rkl2_across_interfaces(orc, s):
    """Two slabs, 6 steps of group_thermal_stable_dt(stages=s): s = 2 is the stage whose Y_{j-2} is Y_0, 5 and 8 end the
    rotation of the stage buffers on either side.  The rise within 1e-10 of sts_ref on the global problem.  The dose
    against the trapezoid rule on the reference's states: a rise off by d changes the dose rate by the factor
    2^(c d) - 1 <= 2 ln 2 d, so with d <= 1e-10 max|theta| the dose is within 2 ln 2 1e-10 max|theta| relative, plus
    the summation bound 16 (2 n) 2^-53 that test_gpu_sts.py holds the dose kernel to.  Then an RK4 segment on the same
    objects."""
    g = shape(orc, "S3")
    parts = slab_parts(g, 2)
    th0, th0d = g.start()
    n = 6
    grp = Group(g, parts)
    grp.finish()
    dt = fa.group_thermal_stable_dt(grp.bios, stages=s)
    assert abs(dt - sts_ref.stable_dt(g.rho20, s)) <= 0.05 * dt        # the same rule (start vectors differ: test 5)
    states = sts_ref.run(g.ref, th0d, dt, n, s, g.h, keep=True)
    grp.set_rise(th0)
    grp.steps(dt, n, stages=s)
    got, D = grp.pull("rise"), grp.pull("dose")
    err = worst_rel(g, parts, got, states[-1])
    Dref = sts_ref.dose_trapezoid([th0d] + states, dt, T_BASE)
    bound = 2.0 * np.log(2.0) * TOL64 * np.abs(states[-1]).max() + 16 * 2 * n * EPS
    derr = max(float((np.abs(d - Dref[p.gids]) / Dref[p.gids]).max()) for d, p in zip(D, parts))
    print(f"s = {s}: rel err after {n} steps {err:.3e}, dose {derr:.3e} (bound {bound:.3e}; dt = {dt:.4e} s)")
    assert err <= g.tol and rel(states[-1], th0d) > 1e-3
    assert Dref.min() > 0 and derr <= bound
    assert_interfaces_identical(parts, got, D)
    dt4 = 2.0 / g.rho20
    grp.steps(dt4, 3)
    after = grp.pull("rise")
    grp.close()
    assert worst_rel(g, parts, after, g.ref.run(states[-1], dt4, 3, g.h)) <= g.tol
    assert_interfaces_identical(parts, after)


# ---- (3) four sharers -------------------------------------------------------------------------------------------------
def _z_layers(mesh, hi):
    """The upper half in z bone, the lower tissue, as test_multirank.py cuts its quadrant case: every quadrant and
    every DOF of the central line touches both."""
    bone = mesh.cell_centroids()[:, 2] > 0.5 * hi[2]
    pick = lambda key: np.where(bone, thermal_ref.BONE[key], thermal_ref.TISSUE[key])   # noqa: E731
    return pick("k"), pick("rho_c"), pick("w")


def test_four_sharers(orc):
    """The 2 x 2 quadrant partition of test_multirank.py (unstructured local numbering, a line of DOFs held by all four
    ranks): 10 RK4 steps against the global reference, the central line bit-identical on all four ranks."""
    g = Global(orc, (4, 4, 3), 3, 0.1, np.float64, hi=[0.016, 0.016, 0.012], mats=_z_layers)
    parts = quadrant_parts(g)
    four = sorted(set.intersection(*[set(p.gids.tolist()) for p in parts]))
    assert len(four) == g.n[2] * g.P + 1
    th0, th0d = g.start()
    dt = 2.0 / g.rho20
    ref = g.ref.run(th0d, dt, 10, g.h)
    grp = Group(g, parts)
    grp.finish()
    grp.set_rise(th0)
    grp.steps(dt, 10)
    got, D = grp.pull("rise"), grp.pull("dose")
    grp.close()
    err = worst_rel(g, parts, got, ref)
    print(f"four quadrants: rel err after 10 steps {err:.3e}")
    assert err <= g.tol and rel(ref, th0d) > 1e-3
    assert_interfaces_identical(parts, got, D)
    local = [{int(gl): i for i, gl in enumerate(p.gids)} for p in parts]
    for gl in four:
        assert len({got[r][local[r][gl]].tobytes() for r in range(4)}) == 1
        assert len({D[r][local[r][gl]].tobytes() for r in range(4)}) == 1


# ---- (4) boundaries ---------------------------------------------------------------------------------------------------
FIX_X, FIX_Z, CONV_Y = 1, 2, 3
FACES = {FIX_X: (0, 0), FIX_Z: (2, 0), CONV_Y: (1, 0)}


def _rank_tags(part, tags):
    """The facets of the global ``tags`` that lie in the part's cells, in its cell numbering."""
    loc = {int(c): i for i, c in enumerate(part.cells)}
    sel = np.isin(tags.cells, part.cells)
    return fa.FacetTags(np.array([loc[int(c)] for c in tags.cells[sel]], np.int32), tags.local_facets[sel], tags.values[sel])


def _apply_boundary(grp, bd, skip=()):
    """bd on every member, each with the facets of its own cells; ``skip``: (rank, tag) pairs left out."""
    for r, (b, p) in enumerate(zip(grp.bios, grp.parts)):
        tags = _rank_tags(p, bd.tags)
        have = lambda tag: (r, tag) not in skip and (tags.values == tag).any()   # noqa: E731
        b.set_boundary(tags, fixed={t: temp[p.gids] for t, temp in bd.fixed.items() if have(t)} or None,
                       convective={t: (hc[p.cells], ext) for t, (hc, ext) in bd.convective.items() if have(t)} or None)


def _check_boundary(orc, g, parts, bd, ref, skip, what):
    th0, th0d = g.start()
    rho20 = ref.power_iteration(20)
    dt, dts = 2.0 / rho20, sts_ref.stable_dt(rho20, 5)
    want = ref.run(ref.impose(th0d), dt, 20, g.h)
    want2 = sts_ref.run(ref, want, dts, 6, 5, g.h)
    held = ref.fixed_rise.astype(g.dtype)
    grp = Group(g, parts)
    _apply_boundary(grp, bd, skip)
    grp.finish()
    for b, p in zip(grp.bios, parts):
        conv = (ref.m_h > 0) & ~ref.fixed
        assert b.boundary_info() == (int(ref.fixed[p.gids].sum()), int(conv[p.gids].sum()))
    grp.set_rise(th0)
    grp.steps(dt, 20)
    got = grp.pull("rise")
    grp.steps(dts, 6, stages=5)
    got2, D = grp.pull("rise"), grp.pull("dose")
    grp.close()
    err, err2 = worst_rel(g, parts, got, want), worst_rel(g, parts, got2, want2)
    print(f"{what}: rel err {err:.3e} after 20 RK4 steps, {err2:.3e} after 6 RKL2 steps more")
    assert err <= g.tol and err2 <= g.tol
    assert rel(want, g.ref.run(th0d, dt, 20, g.h)) > 1e-3        # the boundary is visible
    for a in (got, got2):
        for x, p in zip(a, parts):
            m = ref.fixed[p.gids]
            assert m.any() and np.array_equal(x[m], held[p.gids][m])
    assert_interfaces_identical(parts, got, got2, D)


def test_boundaries_cut_by_the_interface(orc):
    """Two slabs: a convective y face (h_c = 500, theta_ext = -17) and a fixed z face that the interface cuts, and a fixed
    face x = 0 wholly in rank 0; 20 RK4 steps, then 6 RKL2 steps (s = 5), against BioheatBC on the global problem.  The
    fixed DOFs hold their values bit for bit on both sharers, and boundary_info counts the global boundary's DOFs that
    the rank holds.  Then the fixed z face tagged on rank 0's facets only: rank 1 still holds the edge DOFs it shares
    -- a DOF is fixed if any sharer fixes it -- and drops its convective entry on the one that lies on the y face too;
    the reference fixes exactly those DOFs."""
    g = shape(orc, "S3")
    parts = slab_parts(g, 2)
    y = g.prt.V.tabulate_dof_coordinates()[:, 1].astype(np.float64)
    rise = 2.0 + np.sin(40.0 * y)
    bd = Boundary(g, FACES, fixed={FIX_X: rise, FIX_Z: rise}, convective={CONV_Y: (500.0, THETA_EXT)})
    ref = bd.ref(g)
    cut = np.intersect1d(parts[0].gids, parts[1].gids)
    assert ref.fixed[cut].any() and (ref.m_h[cut] > 0).any() and not ref.fixed[parts[1].gids].all()
    _check_boundary(orc, g, parts, bd, ref, (), "cut faces")
    # the z face on rank 0's facets alone
    half = Boundary(g, FACES, fixed={FIX_X: rise, FIX_Z: rise}, convective={CONV_Y: (500.0, THETA_EXT)})
    in0 = np.isin(half.tags.cells, parts[0].cells) | (half.tags.values != FIX_Z)
    half.tags = fa.FacetTags(half.tags.cells[in0], half.tags.local_facets[in0], half.tags.values[in0])
    from thermal_bc_ref import face_dofs
    half.mask = face_dofs(g.pr, half.tags, FIX_X) | face_dofs(g.pr, half.tags, FIX_Z)
    half.rise = np.where(half.mask, ((T_BASE + rise) - T_BASE).astype(g.dtype).astype(np.float64), 0.0)   # as set_boundary forms it
    ref1 = half.ref(g)
    edge = ref1.fixed[parts[1].gids]
    assert edge.sum() == 3 * g.P + 1 and np.array_equal(parts[1].gids[edge], cut[ref1.fixed[cut]])
    assert (bd.m_h[cut[ref1.fixed[cut]]] > 0).sum() == 1         # fixed over convective across ranks, at one corner
    _check_boundary(orc, g, parts, half, ref1, ((1, FIX_Z),), "z face fixed by rank 0 alone")


# ---- (5) step rule ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [2, 3])
def test_step_rule(orc, size):
    """group_thermal_lambda_max against Bioheat.power_iteration on the global problem from the documented start -- every
    rank's 1 + 0.5 sin(37 d + 1) over its own DOF numbers, added on the shared planes -- within 1e-10; the steps derived
    from it; and the same with forced water cooling on the face x = hi (the recipe of thermal_bc_ref.cooled_face).  The
    group call hands one double to all members: the scalars are summed before the quotient is formed."""
    g = shape(orc, "S3")
    parts = slab_parts(g, size)
    x0 = np.zeros(g.pr.ndofs)
    for p in parts:
        x0[p.gids] += 1.0 + 0.5 * np.sin(37.0 * np.arange(len(p.gids)) + 1.0)
    grp = Group(g, parts)
    grp.finish()
    lam20, lam3 = fa.group_thermal_lambda_max(grp.bios, 20), fa.group_thermal_lambda_max(grp.bios, 3)
    again = fa.group_thermal_lambda_max(grp.bios[::-1], 20)
    dt0, dt8 = fa.group_thermal_stable_dt(grp.bios), fa.group_thermal_stable_dt(grp.bios, stages=8)
    want20, want3 = g.ref.power_iteration(20, x0=x0), g.ref.power_iteration(3, x0=x0)
    print(f"{size} slabs: lambda_max(20) {lam20:.9e} against {want20:.9e}; (3) {lam3:.9e} against {want3:.9e}")
    assert abs(lam20 - want20) <= TOL64 * want20 and abs(lam3 - want3) <= TOL64 * want3 and lam3 < lam20
    assert abs(again - want20) <= TOL64 * want20                  # the order of the members does not matter
    assert abs(dt0 - 2.0 / want20) <= TOL64 * dt0
    assert abs(dt8 - 0.72 * sts_ref.beta(8) / want20) <= TOL64 * dt8
    bd = Boundary(g, {1: (0, 1)}, convective={1: (5000.0, THETA_EXT)})
    ref = bd.ref(g)
    _apply_boundary(grp, bd)
    grp.finish()
    cool = fa.group_thermal_lambda_max(grp.bios, 20)
    grp.close()
    wantc = ref.power_iteration(20, x0=x0)
    print(f"{size} slabs, cooled face: {cool:.9e} against {wantc:.9e}")
    assert abs(cool - wantc) <= TOL64 * wantc and wantc > want20 * (1 + 1e-3)


# ---- (6) monitor hand-over --------------------------------------------------------------------------------------------
def test_heat_from_the_monitors_of_slab_models(orc):
    """Two slab Linear models advanced by group_rk4_steps with the monitor on, as test_gpu_monitor.py runs them; every
    rank's thermal object takes its heat from its model's monitor, group_thermal_finish adds the weights: heat() equals
    the slice of the single-rank object's -- the one-rank path test_gpu_thermal.py checks, fed by the single-rank wave
    run -- within 1e-10 of its max, with the same bits on the interface; 5 thermal steps follow the numpy reference
    driven by that heat."""
    import test_multirank as tm
    from util import Problem, live_state
    pr = Problem(orc, tm.N_GLOBAL, tm.P, hi=tm.HI, perturb=0.1)
    wdt = tm.dt_value()
    u0, v0 = live_state(pr, tm.SEED, tm.P0, tm.F0)
    k, rho_c, w = thermal_ref.materials(pr.mesh, tm.HI)
    alpha = np.where(k == thermal_ref.BONE["k"], 20.0, 0.5)

    def wave(mesh, V, ctx):
        c, rho = tm.material(mesh)
        return fa.LinearSpectralExplicit(mesh, fa.tag_box_boundary(mesh), tm.P, c, rho, tm.F0, tm.P0, tm.S0, 4, wdt, V=V, ctx=ctx)

    ctx = fa.Context(0, deterministic=True)
    one = wave(pr.mesh, pr.V, ctx)
    one.init()
    one.set_state(u0, v0)
    one.monitor(which="u", every=1)
    one.rk4_steps(0.0, wdt, tm.NSTEPS)
    th = fa.BioheatSpectralExplicit(pr.mesh, tm.P, k, rho_c, w, model=one)
    th.init()
    th.set_heat_from(one, alpha)
    href = th.heat().x.array.astype(np.float64)
    th.close(), one.close(), ctx.close()
    bio = thermal_ref.Bioheat(pr, k, rho_c, w)
    dt = 2.0 / bio.power_iteration(20)
    ref = bio.run(np.zeros(pr.ndofs), dt, 5, href)
    assert href.max() > 0 and np.abs(ref).max() > 0

    ctxs = [fa.Context(0, deterministic=True) for _ in range(2)]
    fa.Context.init_local_group(ctxs)
    models, bios, gids, meshes = [], [], [], []
    for r, cx in enumerate(ctxs):
        mesh = fa.BoxMesh([0, 0, 0], tm.HI, tm.N_GLOBAL, rank=r, size=2, perturb=0.1)
        V = fa.FunctionSpace(mesh, tm.P)
        meshes.append(mesh)
        models.append(wave(mesh, V, cx))
        gids.append(V.global_offset + np.arange(V.num_dofs))
    fa.group_finish_setup(models)
    for mdl, gl in zip(models, gids):
        mdl.init()
        mdl.set_state(u0[gl], v0[gl])
        mdl.monitor(which="u", every=1)
    fa.group_rk4_steps(models, 0.0, wdt, tm.NSTEPS)
    for mdl, mesh in zip(models, meshes):
        kr, rcr, wr = thermal_ref.materials(mesh, tm.HI)
        bios.append(fa.BioheatSpectralExplicit(mesh, tm.P, kr, rcr, wr, model=mdl))
    fa.group_thermal_finish(bios)
    for b, mdl, mesh in zip(bios, models, meshes):
        b.init()
        b.set_heat_from(mdl, np.where(thermal_ref.materials(mesh, tm.HI)[0] == thermal_ref.BONE["k"], 20.0, 0.5))
    fa.group_thermal_finish(bios)
    h = [b.heat().x.array.copy() for b in bios]
    fa.group_thermal_steps(bios, dt, 5)
    got = [b.rise().x.array.copy() for b in bios]
    for b in bios:
        b.close()
    for mdl in models:
        mdl.close()
    for cx in ctxs:
        cx.close()
    herr = max(float(np.abs(a - href[gl]).max()) for a, gl in zip(h, gids)) / href.max()
    err = max(float(np.abs(a - ref[gl]).max()) for a, gl in zip(got, gids)) / np.abs(ref).max()
    print(f"heat from the slab monitors: error / max {herr:.3e}; 5 steps {err:.3e}")
    assert herr <= 1e-10 and err <= TOL64
    plane = len(np.intersect1d(gids[0], gids[1]))
    assert plane > 0 and np.array_equal(h[0][-plane:], h[1][:plane]) and np.array_equal(got[0][-plane:], got[1][:plane])
    assert np.abs(h[0][-plane:]).max() > 0


# ---- (7) call sequence, and the single rank's launches ----------------------------------------------------------------
def test_call_sequence(orc):
    g = shape(orc, "S3")
    parts = slab_parts(g, 2)
    th0 = g.start()[0]
    dt = 2.0 / g.rho20
    grp = Group(g, parts)
    missing = "error -4: .*fus_group_thermal_finish"
    for call in (lambda b: b.init(), lambda b: b.set_state(rise=th0[parts[0].gids]), lambda b: b.steps(dt, 1),
                 lambda b: b.steps(dt, 1, stages=3), lambda b: b.lambda_max(2), lambda b: b.stable_dt()):
        with pytest.raises(fa.FusError, match=missing):
            call(grp.bios[0])
    for call in (lambda: grp.steps(dt, 1), lambda: fa.group_thermal_lambda_max(grp.bios, 2),
                 lambda: fa.group_thermal_stable_dt(grp.bios)):
        with pytest.raises(fa.FusError, match=missing):
            call()
    grp.finish()
    grp.finish()                                                   # nothing pending: nothing happens
    with pytest.raises(fa.FusError, match="error -4: .*fus_thermal_init"):
        grp.steps(dt, 1)
    grp.set_rise(th0)
    for stages in (0, 3):
        with pytest.raises(fa.FusError, match="error -4: .*use fus_group_thermal_steps"):
            grp.bios[1].steps(dt, 1, stages=stages)
    with pytest.raises(fa.FusError, match="error -4: .*fus_group_thermal_lambda_max"):
        grp.bios[1].lambda_max(2)
    for bad in (0.0, np.nan):
        with pytest.raises(fa.FusError, match="error -1: .*dt"):
            grp.steps(bad, 1)
    with pytest.raises(fa.FusError, match="error -1: .*stages"):
        grp.steps(dt, 1, stages=33)
    with pytest.raises(fa.FusError, match="error -1"):
        fa.group_thermal_steps(grp.bios[:1], dt, 1)                # a member's neighbour is missing from the group
    for r, p in enumerate(parts):
        assert np.array_equal(grp.bios[r].rise().x.array, th0[p.gids])          # the state is as it was
    grp.steps(dt, 2)
    for b, p in zip(grp.bios, parts):                               # set_heat after finish needs finish again
        b.set_heat(2.0 * g.q[p.gids])
    with pytest.raises(fa.FusError, match=missing):
        grp.steps(dt, 1)
    grp.finish()
    grp.steps(dt, 2)
    got = grp.pull("rise")
    ref = g.ref.run(g.ref.run(th0.astype(np.float64), dt, 2, g.h), dt, 2, 2.0 * g.h)
    assert worst_rel(g, parts, got, ref) <= g.tol
    # closing in any order: a member first, then its context, then the rest
    grp.bios[1].close(), grp.ctxs[1].close()
    grp.bios[0].close(), grp.bios[0].close(), grp.ctxs[0].close()
    # a context without a transport still refuses operator data with neighbours (test_gpu_thermal.py), also when the
    # caller drives the exchange itself
    ctx = fa.Context(0, deterministic=True)
    ctx.init_external(0, 2)
    with pytest.raises(fa.FusError, match="error -4: .*several ranks.*communicator.*in-process group.*external"):
        fa.BioheatSpectralExplicit(parts[0].mesh, g.P, 0.5, 3.6e6, V=parts[0].V, ctx=ctx)
    ctx.close()


def test_single_rank_launches_are_unchanged(orc):
    """One rank, profiling on: 3 RK4 steps count 4 launches each of "thermal", "stiffness" and "shared" per step and
    none of the interface kernel ("thermal_if") or of "halo"; 2 RKL2 steps of 5 stages count 5 per step.  Two slabs
    count one "thermal_if" and one "halo" (the pack) per stage and member on top of the same three."""
    g = shape(orc, "S3")
    th0 = g.start()[0]
    dt = 2.0 / g.rho20
    names = ("thermal", "thermal_sts", "stiffness", "shared", "thermal_if", "halo")
    ctx = fa.Context(0, deterministic=True)
    t = g.dtype
    th = fa.BioheatSpectralExplicit(g.prt.mesh, g.P, g.k.astype(t), g.rho_c.astype(t), g.w.astype(t), V=g.prt.V, ctx=ctx)
    th.set_heat(g.q.astype(t))
    th.set_state(rise=th0)
    ctx.profile_enable(True)
    th.steps(dt, 3)
    c4 = {nm: ctx.profile_get(nm)[1] for nm in names}
    th.steps(dt, 2, stages=5)
    c5 = {nm: ctx.profile_get(nm)[1] for nm in names}
    th.close(), ctx.close()
    assert c4 == dict(thermal=12, thermal_sts=0, stiffness=12, shared=12, thermal_if=0, halo=0)
    assert c5 == dict(thermal=12, thermal_sts=10, stiffness=22, shared=22, thermal_if=0, halo=0)
    parts = slab_parts(g, 2)
    grp = Group(g, parts, profile=True)
    grp.finish()
    grp.set_rise(th0)
    for c in grp.ctxs:
        c.profile_enable(True)                                      # counts from here
    grp.steps(dt, 3)
    grp.steps(dt, 2, stages=5)
    for c in grp.ctxs:
        assert {nm: c.profile_get(nm)[1] for nm in names} == dict(thermal=12, thermal_sts=10, stiffness=22, shared=22,
                                                                   thermal_if=22, halo=22)
    grp.close()
