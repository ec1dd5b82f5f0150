"""Every RK stage kind and model family across rank interfaces.  The stage updates exist a third time in
k_if_unpack_stage, for the DOFs that several ranks hold; the single-rank matrices (test_gpu_live_state.py,
test_gpu_live_matrix.py) cannot see that copy, and the other multi-rank tests run it at the lean RK4 kinds only.
Here, from live starts: the accumulator kinds (rk_order 1-3 and RK4 with lean_rk4 = 0) and the families and
partitions that had no multi-rank run -- k_boundary_partial at every stage with the boundary slots of the interface
rim, and the (u_, v_) <-> (u0, v0) swap after a lower-order step in each of its places (fus_group_rk4_steps,
fus_model_stage_end).

The reference is always the oracle on the GLOBAL mesh with the fixed step count; u and v of every rank, at that
rank's global DOFs, lie within TOL_RK of it relative to its max, and every DOF that more than one rank holds is
bit-identical on all its holders.  Each test prints its worst error over the tolerance (pytest -s).  The CPU guards
of every case are in test_live_guards.py (fp64) and test_fp32_guards.py (fp32).

Measured on the MI355X, worst error / TOL_RK (linear, lossy, westervelt; the same on 2 and 3 slabs to three digits
except linear rk4-acc, 3.1e-5 on 2):
  hexahedral slabs     rk1 9.3e-6 6.7e-6 8.4e-6   rk2 9.4e-6 8.1e-6 5.9e-6   rk3 8.0e-6 6.7e-6 8.4e-6
                       rk4-acc 3.0e-5 1.5e-5 1.2e-5   rk4 - 2.9e-5 2.2e-5
  four quadrants       rk4 - 2.5e-5 1.9e-5   rk4-acc 1.6e-5 1.8e-5 1.5e-5   rk2 6.7e-6 6.7e-6 6.5e-6
  quadrilateral slabs  rk4 - 2.6e-5 4.0e-5   rk2 - 4.9e-6 5.3e-6   rk4-acc - 1.2e-5 1.3e-5
  options, external stage API: the figures of the same case and variant in the in-process group, to three digits
  fp32 (largest ratio to the float oracle's own error, of CAP = 8): lean_rk4 = 0 between 1.01 and 1.16, order 3 1.04"""
import ctypes as C

import numpy as np
import pytest

import fenicsxfus_amd as fa
import fp32_budget as fb
from live_cases import FP32_SLABS, KINDS, TOL_RK, fp32_case, mr_case, mr_partitions
from quadrant_partition import held_by_all, quadrant_parts
from util import assert_live, slab_interface_regions

pytestmark = pytest.mark.gpu

# variant -> (rk_order, lean_rk4 option or None for the default)
VARIANTS = {"rk1": (1, None), "rk2": (2, None), "rk3": (3, None), "rk4-acc": (4, 0), "rk4": (4, None)}
# blocks small enough that every rank has several, the last one shorter: DOFs shared by a rank's blocks next to DOFs
# shared by ranks
BLOCK_ELEMS = {"hex": 12, "quad": 8, "quadrants": 4}

_refs = {}


def reference(orc, shape, kind, variant):
    """(case, start, oracle state after the case's steps): computed once per case and left unchanged."""
    name = f"{kind}-{shape}-rk{VARIANTS[variant][0]}"
    if name not in _refs:
        cs = mr_case(orc, name)
        u0, v0 = cs.start()
        ref = cs.oracle(u0, v0, fixed=True)
        for _, planes, _ in mr_partitions(cs, name):
            assert_live(ref, {**cs.regions, **planes})
        for a in (u0, v0) + ref:
            a.setflags(write=False)
        _refs[name] = cs, (u0, v0), ref
    cs = _refs[name][0]
    assert cs.order == VARIANTS[variant][0] and cs.dtype == np.float64
    return _refs[name]


def context(variant, block_elems=None, ckw=None, opts=None):
    cx = fa.Context(0, block_elems=block_elems, **(ckw or {}))
    if VARIANTS[variant][1] is not None:
        cx.set_option("lean_rk4", VARIANTS[variant][1])
    for k, val in (opts or {}).items():
        cx.set_option(k, val)
    return cx


def slab_models(cs, ctxs):
    """The case's x-slab models on ``ctxs`` and the global DOF ids of each one's DOFs."""
    size = len(ctxs)
    models = [cs.model(ctxs[r], rank=r, size=size) for r in range(size)]
    gids = [m.data.V.global_offset + np.arange(m.data.ndofs) for m in models]
    return models, gids


def quadrant_models(cs, ctxs):
    parts = quadrant_parts(cs.pr, cs.tags)
    assert len(held_by_all(parts)) == cs.n[2] * cs.P + 1      # the central line: held by all four ranks
    mats = cs.materials()
    models = [cs.model_on(ctxs[r], p.mesh, p.V, p.tags, tuple(a[p.cells] for a in mats))
              for r, p in enumerate(parts)]
    return models, [p.gids for p in parts]


def set_start(models, gids, start):
    for m, g in zip(models, gids):
        m.init()
        m.set_state(start[0][g], start[1][g])


def states(models):
    return [(m.u_sol().x.array.copy(), m.v_n.x.array.copy()) for m in models]


def assert_sharers_bit_identical(got, gids):
    """Every DOF that two ranks hold has the same bits on both (so on all its holders), in u and in v."""
    nshared = 0
    for r in range(len(gids)):
        for q in range(r + 1, len(gids)):
            _, ir, iq = np.intersect1d(gids[r], gids[q], return_indices=True)
            nshared += len(ir)
            for f in (0, 1):
                a, b = got[r][f][ir], got[q][f][iq]
                assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), (r, q, "uv"[f])
    assert nshared > 0
    return nshared


def check(label, got, gids, ref):
    """Both fields of every rank within TOL_RK of the global reference, relative to the reference's max."""
    worst = 0.0
    for g, ids in zip(got, gids):
        for f in (0, 1):
            assert g[f].dtype == np.float64 and np.isfinite(g[f]).all()
            worst = max(worst, np.abs(g[f] - ref[f][ids]).max() / np.abs(ref[f]).max())
    print(f"multirank {label}: err / TOL_RK = {worst / TOL_RK:.3e}")
    assert worst < TOL_RK, f"{label}: err / TOL_RK = {worst / TOL_RK:.3e}"
    assert_sharers_bit_identical(got, gids)


def close(models, ctxs):
    for m in models:
        m.close()
    for cx in ctxs:
        cx.close()


def run_group(orc, shape, kind, variant, size, ckw=None, opts=None, label=""):
    """One in-process group of ``size`` ranks on the case's partition, stepped with fus_group_rk4_steps."""
    cs, start, ref = reference(orc, shape, kind, variant)
    ctxs = [context(variant, BLOCK_ELEMS[shape], ckw, opts) for _ in range(size)]
    fa.Context.init_local_group(ctxs)
    models, gids = quadrant_models(cs, ctxs) if shape == "quadrants" else slab_models(cs, ctxs)
    for m in models:
        info = m.data.info()
        assert info["nblocks"] >= 2 and info["shared_dofs"] > 0, info
        assert len(m.data.halo_layout()[0]) >= 1
    fa.group_finish_setup(models)
    set_start(models, gids, start)
    fa.group_rk4_steps(models, 0.0, cs.dt, cs.nsteps)
    check(f"[{shape} x{size}{label}] {kind} {variant}", states(models), gids, ref)
    close(models, ctxs)


# ---- in-process groups ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [2, 3])
@pytest.mark.parametrize("variant", ["rk1", "rk2", "rk3", "rk4-acc"])
@pytest.mark.parametrize("kind", KINDS)
def test_hex_slabs_accumulator_kinds(orc, kind, variant, size):
    """Stage kinds 0, 1 and 3 of k_if_unpack_stage, every family; orders 1-3: the boundary slots of the interface rim
    summed by k_if_reduce_pack at every stage, and the swap in fus_group_rk4_steps."""
    run_group(orc, "hex", kind, variant, size)


@pytest.mark.parametrize("kind,size", [("lossy", 2), ("lossy", 3), ("westervelt", 3)])
def test_hex_slabs_lean_kinds(orc, kind, size):
    """The lean kinds where no fp64 test ran them: Lossy across interfaces, Westervelt on three slabs."""
    run_group(orc, "hex", kind, "rk4", size)


@pytest.mark.parametrize("kind,variant", [(k, v) for k in ("lossy", "westervelt") for v in ("rk4", "rk4-acc", "rk2")]
                         + [("linear", "rk4-acc"), ("linear", "rk2")])
def test_four_quadrants(orc, kind, variant):
    """One line of DOFs held by four ranks, unstructured local numbering: each adds four totals in rank order."""
    run_group(orc, "quadrants", kind, variant, 4)


@pytest.mark.parametrize("variant", ["rk4", "rk2", "rk4-acc"])
@pytest.mark.parametrize("kind", ["lossy", "westervelt"])
def test_quad_slabs(orc, kind, variant):
    run_group(orc, "quad", kind, variant, 3)


OPTIONS = {"planes=0": ({}, dict(planes=0)), "deterministic=1": (dict(deterministic=1), {}),
           "overlap_blocks=1": ({}, dict(overlap_blocks=1))}


@pytest.mark.parametrize("option", list(OPTIONS))
@pytest.mark.parametrize("kind", ["linear", "lossy"])
def test_options_across_the_interface(orc, kind, option):
    """The shared-DOF stage kernel on the CSR, the stage kernels without atomics and the interface blocks launched
    first, each with the accumulator kinds of order 3 on three slabs."""
    ckw, opts = OPTIONS[option]
    run_group(orc, "hex", kind, "rk3", 3, ckw, opts, label=f" {option}")


# ---- the external stage API -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["rk3", "rk4-acc"])
@pytest.mark.parametrize("kind", KINDS)
def test_external_stage_api(orc, kind, variant):
    """Three slabs driven through setup_pack / setup_unpack / stage_begin / stage_end, the exchange done here by
    device-to-device copies between the ranks' send and receive buffers.  rk3: the only run of the swap in
    fus_model_stage_end."""
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    size = 3
    cs, start, ref = reference(orc, "hex", kind, variant)
    ctxs = []
    for r in range(size):
        cx = context(variant, BLOCK_ELEMS["hex"])
        cx.init_external(r, size)
        ctxs.append(cx)
    models, gids = slab_models(cs, ctxs)
    layouts = [m.data.halo_layout() for m in models]
    bufs = [m.data.halo_buffers() for m in models]
    assert [len(lay[0]) for lay in layouts] == [1, 2, 1]

    def exchange():
        """rank r's send range for neighbour q -> q's receive range for neighbour r (8-byte values)."""
        for r in range(size):
            for q, cnt, off in zip(*layouts[r]):
                k = list(layouts[q][0]).index(r)
                assert layouts[q][1][k] == cnt and 0 <= off and off + cnt <= bufs[r][2]
                assert int(layouts[q][2][k]) + cnt <= bufs[q][2]
                rc = hip.hipMemcpy(bufs[q][1] + 8 * int(layouts[q][2][k]), bufs[r][0] + 8 * int(off), 8 * int(cnt), 3)
                assert rc == 0

    assert models[0].setup_count() == (2 if kind == "westervelt" else 1)
    for k in range(models[0].setup_count()):
        for m in models:
            m.setup_pack(k)
        exchange()
        for m in models:
            m.setup_unpack(k)
    for m in models:
        m.setup_finish()
    set_start(models, gids, start)
    t = 0.0
    for _ in range(cs.nsteps):
        for i in range(cs.order):
            for m in models:
                m.stage_begin(i, t, cs.dt)
            exchange()
            for m in models:
                m.stage_end(i, t, cs.dt)
        t += cs.dt
    check(f"[hex x{size} external] {kind} {variant}", states(models), gids, ref)
    close(models, ctxs)


# ---- fp32: held to the float oracle's own rounding error (fp32_budget.py) -------------------------------------------
FP32 = [(name, 0) for name in FP32_SLABS] + [("lossy-slabs-p4-rk3", None)]


@pytest.mark.parametrize("name,lean", FP32)
def test_fp32_two_slabs(orc, name, lean):
    """test_gpu_fp32_budget.py::test_two_slabs_in_process at the accumulator kinds: its four cases with
    lean_rk4 = 0, and Lossy at order 3."""
    size = 2
    cs = fp32_case(orc, name)
    (u0, v0), r32, r64 = cs.fp32_refs()
    regions = {**cs.regions, **slab_interface_regions(cs.pr, size)}
    assert_live(r64, regions)
    ctxs = [fa.Context(0) for _ in range(size)]
    if lean is not None:
        assert cs.order == 4
        for cx in ctxs:
            cx.set_option("lean_rk4", lean)
    else:
        assert cs.order == 3
    fa.Context.init_local_group(ctxs)
    models, gids = slab_models(cs, ctxs)
    for m in models:
        assert m.data.geometry_mode() == "trilinear" and m.data.dtype == np.float32
    fa.group_finish_setup(models)
    set_start(models, gids, (u0, v0))
    fa.group_rk4_steps(models, 0.0, cs.dt, cs.nsteps)
    got = states(models)
    for r, ids in enumerate(gids):
        off, k = ids[0], len(ids)
        mine = {}
        for rname, idx in regions.items():
            sel = idx[(idx >= off) & (idx < off + k)] - off
            if len(sel):
                mine[rname] = sel
        assert any(rname.startswith("cut") for rname in mine)
        part = lambda a: tuple(b[off:off + k] for b in a)  # noqa: E731
        assert got[r][0].dtype == np.float32
        fb.check(f"[slabs-{cs.kind}] {name} lean_rk4={lean} rank {r}", got[r], part(r32), part(r64), mine)
    assert_sharers_bit_identical(got, gids)
    close(models, ctxs)


# ---- group members must agree ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("differ", ["rk_order", "kind", "dtype"])
def test_group_members_must_agree(orc, differ):
    """fus_group_rk4_steps steps every member by one stage loop: members of another order, model kind or scalar type
    are an argument error before any launch, and every member keeps its state bit for bit."""
    cs, start, _ = reference(orc, "hex", "linear", "rk4")
    other = {"rk_order": mr_case(orc, "linear-hex-rk2"), "kind": mr_case(orc, "lossy-hex-rk4"),
             "dtype": fp32_case(orc, "lossy-slabs-p4")}[differ]
    if differ == "dtype":
        cs = mr_case(orc, "lossy-hex-rk4")
    ctxs = [fa.Context(0) for _ in range(2)]
    fa.Context.init_local_group(ctxs)
    if differ == "dtype":    # (two meshes: the setup exchange needs members of one scalar type, so each is alone)
        models = [cs.model(ctxs[0]), other.model(ctxs[1])]
        starts = [cs.start(), tuple(a.astype(np.float32) for a in other.start())]
        for m in models:
            fa.group_finish_setup([m])
    else:
        models = [cs.model(ctxs[0], rank=0, size=2), other.model(ctxs[1], rank=1, size=2)]
        gids = [m.data.V.global_offset + np.arange(m.data.ndofs) for m in models]
        starts = [(start[0][g], start[1][g]) for g in gids]
        fa.group_finish_setup(models)
    for m, s in zip(models, starts):
        m.init()
        m.set_state(*s)
    before = states(models)
    with pytest.raises(fa.FusError, match=r"libfusmi error -1:.*differ"):
        fa.group_rk4_steps(models, 0.0, cs.dt, 2)
    for (u, v), (ub, vb) in zip(states(models), before):
        assert np.array_equal(u.view(np.uint8), ub.view(np.uint8)) and np.array_equal(v.view(np.uint8), vb.view(np.uint8))
    close(models, ctxs)
