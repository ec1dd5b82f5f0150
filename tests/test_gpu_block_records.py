"""The block kernel reading one 64-byte record per block (layout.hpp BlockRecord), its boundary range requested ahead
of the barrier that ends the element trips, and the plane form of the shared-dof stage kernel with 16-byte accesses
(two dofs per thread in fp64, four in fp32), on meshes chosen so that every path of those changes runs: blocks with
and without boundary entries, blocks with an odd interior count, a shared range whose length is no multiple of four
and planes of odd length.  Those facts are asserted from the layout, which a stand-alone host driver
(tests/cpp/block_records_driver.cpp) builds from the same dofmap; its statistics must be the operator's own info().

Tolerances: fp64 as tests/test_gpu_parity.py (1e-12 stiffness, 1e-14 mass, 1e-10 RK); fp32 against the float
oracle's own rounding error (fp32_budget.py), like tests/test_gpu_fp32_budget.py."""
import numpy as np
import pytest

import fenicsxfus_amd as fa
import fp32_budget as fb
from fenicsxfus_amd import FacetTags
from live_cases import TOL_RK, Case
from test_block_records_host import build_driver, run_driver
from util import assert_live

pytestmark = pytest.mark.gpu

TOL_OP, TOL_MASS = 1e-12, 1e-14
# name -> (cells, degree, tagged faces).  4-element blocks.  With every face of such a small box tagged each block
# holds a boundary entry (the small box has three cells without a boundary face, and in the larger one every block
# of four reaches a face): only the source face x = 0 and the far face are tagged, the blocks in between have none.
MESHES = {"5x3x3-p2": ((5, 3, 3), 2, "x"), "6x5x4-p4": ((6, 5, 4), 4, "x")}
NSTEPS = 6


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return build_driver(tmp_path_factory.mktemp("rec"), sanitize=False)


def end_faces_only(mesh):
    cells, lf, ax, sd = mesh.exterior_facets()
    keep = ax == 0
    return FacetTags(cells[keep], lf[keep], np.where(sd[keep] == 0, 1, 2).astype(np.int32))


_cases = {}


def case_of(orc, kind, n, P, dtype, faces="all", order=4, perturb=0.1, nsteps=NSTEPS):
    key = (kind, n, P, np.dtype(dtype).name, faces, order, nsteps)
    if key not in _cases:
        cs = Case(orc, kind, n, P, perturb=perturb, nsteps=nsteps, order=order, dtype=dtype,
                  cfl=0.5 if order == 4 else 0.1)
        if faces == "x":
            cs.tags = end_faces_only(cs.pr.mesh)
        _cases[key] = cs
    return _cases[key]


def model_of(cs, cx):
    """The library's model of the case with the case's own facet tags."""
    return cs.model_on(cx, cs.prt.mesh, cs.prt.V, cs.tags, cs.materials())


def layout_facts(driver, tmp_path, cs, block_elems):
    V = cs.vectors(cs.pr)
    bnd = np.flatnonzero((V["src"] != 0) | (V["absb"] != 0))
    facts, _, _ = run_driver(driver, tmp_path / "in.bin", cs.tdim, cs.P, cs.pr.dm, cs.pr.mesh.cell_centroids(),
                             block_elems, 4, bnd)
    return facts


def same_layout(facts, info):
    return (facts["blocks"], facts["interior"], facts["shared"], facts["pairs"], facts["shapes"]) == (
        info["nblocks"], info["interior_dofs"], info["shared_dofs"], info["pairs"], info["shapes"])


def references(cs):
    """(start, reference(s)) after NSTEPS exact steps: fp64 the double oracle, fp32 the float and the double oracle."""
    if cs.dtype == np.float32:
        start, r32, r64 = cs.fp32_refs()
        assert_live(r64, cs.regions)
        return start, (r32, r64)
    start = cs.start()
    ref = cs.oracle(*start, fixed=True)
    assert_live(ref, cs.regions)
    return start, ref


def run(cs, cx, start):
    model = model_of(cs, cx)
    model.init()
    model.set_state(*start)
    model.rk4_steps(0.0, cs.dt, cs.nsteps)
    out = model.u_sol().x.array.copy(), model.v_n.x.array.copy()
    model.close()
    return out


def relmax(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["fp64", "fp32"])
@pytest.mark.parametrize("name", list(MESHES))
def test_block_kernel_on_records(orc, driver, tmp_path, name, dtype):
    """Stiffness and mass actions and 6 RK4 steps of the linear model against the oracle on 4-element blocks
    (trilinear geometry) that do and do not hold boundary entries and have odd interior counts; in deterministic
    mode one workgroup per block and walking workgroups (option "walk" = 2) give the same bits."""
    n, P, faces = MESHES[name]
    cs = case_of(orc, "linear", n, P, dtype, faces)
    facts = layout_facts(driver, tmp_path, cs, 4)
    assert facts["with_bnd"] > 0 and facts["without_bnd"] > 0, facts
    assert facts["odd_int"] > 0, facts
    pr, pr64 = cs.prt, cs.pr64r
    rng = np.random.default_rng(P)
    x = rng.standard_normal(pr.ndofs).astype(dtype)
    coef = rng.uniform(0.5, 2.0, pr.mesh.num_cells).astype(dtype)
    refK, refM = pr.K(x, coef), pr.M(x, coef)
    if dtype == np.float32:
        x64, c64 = x.astype(np.float64), coef.astype(np.float64)
        refK64, refM64 = pr64.K(x64, c64), pr64.M(x64, c64)
        assert_live((refK64, refM64), cs.regions)
    start, ref = references(cs)
    bits = {}
    # deterministic with one workgroup per block and with walking workgroups, and the default LDS-atomic kernels
    for det, walk in ((1, 0), (1, 2), (0, 0)):
        label = f"{name} deterministic={det} walk={walk}"
        cx = fa.Context(0, geometry="trilinear", block_elems=4, deterministic=det)
        cx.set_option("walk", walk)
        d = fa.SpectralOperatorData(pr.V, cx)
        assert d.geometry_mode() == "trilinear" and d.dtype == np.dtype(dtype)
        assert same_layout(facts, d.info()), (facts, d.info())
        y = d.stiffness(x, coef, np.zeros(pr.ndofs, dtype))
        ym = d.mass(x, coef, np.zeros(pr.ndofs, dtype))
        d.close()
        g = run(cs, cx, start)
        cx.close()
        if dtype == np.float64:
            assert relmax(y, refK) < TOL_OP and relmax(ym, refM) < TOL_MASS, label
            assert relmax(g[0], ref[0]) < TOL_RK and relmax(g[1], ref[1]) < TOL_RK, label
        else:
            fb.check(f"[records-stiffness] {label}", y, refK, refK64, cs.regions)
            fb.check(f"[records-mass] {label}", ym, refM, refM64, cs.regions)
            fb.check(f"[records-rk4] {label}", g, ref[0], ref[1], cs.regions)
        bits[det, walk] = (y, ym, *g)
    for a, b in zip(bits[1, 0], bits[1, 2]):
        assert np.array_equal(a, b)


# RK order 4 without accumulators (stage kinds 4-7), order 4 with them (lean_rk4 = 0: kinds 0, 1, 1, 3), order 3
STEPPERS = {"rk4-lean": (4, 1), "rk4-acc": (4, 0), "rk3": (3, 1)}


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["fp64", "fp32"])
@pytest.mark.parametrize("stepper", list(STEPPERS))
@pytest.mark.parametrize("kind", ["linear", "lossy", "westervelt"])
@pytest.mark.parametrize("block_elems,P", [(1, 2), (4, 3)])
def test_stage_kernel_planes_and_csr_agree_bitwise(orc, driver, tmp_path, block_elems, P, kind, stepper, dtype):
    """The plane form of the shared-dof stage kernel (16-byte accesses) against the CSR form (one dof per thread),
    deterministic block kernels: the same bits after 5 steps, for every model family and stage kind.  The shared
    range is no multiple of four dofs long (the last thread's vector is cut short in fp64 and in fp32) and at least
    one plane has an odd length (a plane ends inside a vector); one-element blocks at P = 2 give 8 planes."""
    order, lean = STEPPERS[stepper]
    cs = case_of(orc, kind, (6, 5, 4), P, dtype, order=order, perturb=0.15, nsteps=5)
    facts = layout_facts(driver, tmp_path, cs, block_elems)
    assert facts["shared_local"] % 4 != 0 and facts["odd_planes"] > 0, facts
    assert facts["planes"] == 8 or block_elems != 1
    start = tuple(a.astype(dtype) for a in cs.start())
    outs = {}
    for planes in (1, 0):
        cx = fa.Context(0, deterministic=1, block_elems=block_elems)
        cx.set_option("planes", planes)
        cx.set_option("lean_rk4", lean)
        model = model_of(cs, cx)
        assert same_layout(facts, model.data.info()), (facts, model.data.info())
        model.close()
        outs[planes] = run(cs, cx, start)
        cx.close()
    assert np.abs(outs[0][0]).max() > 0 and np.isfinite(outs[0][0]).all() and np.isfinite(outs[0][1]).all()
    assert np.array_equal(outs[1][0], outs[0][0]) and np.array_equal(outs[1][1], outs[0][1])
