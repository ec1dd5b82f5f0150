"""The straight-line block kernel of the fp64 per-cell geometry paths at the degrees <= 4 without its leftover loops
(profiles/block_issue.md), on perturbed boxes: all 21 map coefficients of every cell are non-trivial and differ per
component.  The cases also pin what that notebook measured and did not keep -- the odd last interior dof's one-dof
update (blocks with odd and with even interior counts) and the partial-sum stores of short shared ranges -- so that a
later attempt at either finds its test here.

  stiffness action, P = 2, 3, 4 on 5 x 4 x 3 cells against the oracle
  one RK4 step of the Linear model, P = 4 on 6 x 5 x 4 cells, at two block sizes that do not divide the 120 cells: blocks
      with odd and with even interior counts, a block with fewer than 512 shared dofs, source and absorbing entries on
      the two x faces only, so that blocks with and without boundary entries exist (asserted from the layout, which a
      stand-alone host driver builds from the same dofmap)
  a block size whose interior range is longer than the first batch: the library reports the kernel with the block loop,
      and the step matches the oracle all the same
  deterministic mode twice: the same bits

Tolerances: tests/test_gpu_parity.py's (1e-12 per stiffness action, 1e-10 for RK)."""
import numpy as np
import pytest

import fenicsxfus_amd as fa
from fenicsxfus_amd import FacetTags
from live_cases import TOL_RK, Case
from test_block_records_host import RECORD, build_driver, run_driver
from util import Problem, assert_live

pytestmark = pytest.mark.gpu

TOL_OP = 1e-12
N_RK, P_RK = (6, 5, 4), 4
BLOCK_SIZES = (7, 32)   # neither divides 120
BLOCK_TOO_LARGE = 64    # more than 2 x 512 16-byte interior vectors in a block: past the first batch at degree 4
WAVES = 8                # 512 threads, as the default layout of degree 4 has them
FIRST_BATCH_VECTORS = 2 * 64 * WAVES


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return build_driver(tmp_path_factory.mktemp("issue"), sanitize=False)


@pytest.fixture(scope="module")
def rk_case(orc):
    """The case, its live start and the oracle's state after one step: computed once, shared and left unchanged."""
    cs = Case(orc, "linear", N_RK, P_RK, perturb=0.1, nsteps=1)
    cells, lf, ax, sd = cs.pr.mesh.exterior_facets()
    keep = ax == 0   # source face x = 0 and absorbing face x = L only: the blocks in between hold no boundary entry
    cs.tags = FacetTags(cells[keep], lf[keep], np.where(sd[keep] == 0, 1, 2).astype(np.int32))
    start = cs.start()
    ref = cs.oracle(*start, fixed=True)
    assert_live(ref, cs.regions)
    for a in (*start, *ref):
        a.setflags(write=False)
    return cs, start, ref


def relmax(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def layout(driver, tmp_path, cs, block_elems):
    V = cs.vectors(cs.pr)
    bnd = np.flatnonzero((V["src"] != 0) | (V["absb"] != 0))
    facts, raw, _ = run_driver(driver, tmp_path / "in.bin", cs.tdim, cs.P, cs.pr.dm, cs.pr.mesh.cell_centroids(),
                               block_elems, WAVES, bnd)
    return facts, raw.view(RECORD)


def step(cs, cx, start, facts):
    model = cs.model_on(cx, cs.pr.mesh, cs.pr.V, cs.tags, cs.materials())
    info = model.data.info()
    assert model.data.geometry_mode() == "trilinear"
    assert (facts["blocks"], facts["interior"], facts["shared"]) == (info["nblocks"], info["interior_dofs"], info["shared_dofs"])
    model.init()
    model.set_state(*start)
    model.rk4_steps(0.0, cs.dt, cs.nsteps)
    out = model.u_sol().x.array.copy(), model.v_n.x.array.copy()
    model.close()
    return out, info


@pytest.mark.parametrize("P", [2, 3, 4])
def test_stiffness_action(orc, P):
    """Pins the layout of the 21 map coefficients in LDS as the trips read it (a transposed or shifted coefficient gives
    errors of order one).  The component-major layout with 16-byte reads (profiles/block_issue.md, Part 2) passed this
    test and was not kept; the layout here is the one it was."""
    pr = Problem(orc, (5, 4, 3), P, hi=[1.5, 1.0, 0.8], perturb=0.15)
    rng = np.random.default_rng(P)
    x = rng.standard_normal(pr.ndofs)
    coef = rng.uniform(0.5, 2.0, pr.mesh.num_cells)
    ref = pr.K(x, coef)
    # 8-element blocks (the default block of degree 2 would hold all 60 cells): eight blocks, the last one ragged, each
    # of at most 9^3 dofs -- within the first batches at every degree
    cx = fa.Context(0, geometry="trilinear", block_elems=8)
    d = fa.SpectralOperatorData(pr.V, cx)
    assert d.geometry_mode() == "trilinear" and d.info()["nblocks"] == 8 and d.info()["block_loop"] == 0
    y = d.stiffness(x, coef, np.zeros(pr.ndofs))
    d.close()
    cx.close()
    print(f"P={P}: stiffness {relmax(y, ref):.2e}")
    assert relmax(y, ref) < TOL_OP


def test_one_rk4_step_at_two_block_sizes(rk_case, driver, tmp_path):
    cs, start, ref = rk_case
    odd = even = small_shared = with_bnd = without_bnd = 0
    for be in BLOCK_SIZES:
        facts, rec = layout(driver, tmp_path, cs, be)
        nint, nsh = rec["nint"].astype(np.int64), (rec["nloc"] - rec["nint"]).astype(np.int64)
        assert cs.pr.mesh.num_cells % be != 0 and facts["blocks"] > 1
        assert (nint // 2 <= FIRST_BATCH_VECTORS).all() and (nsh <= 3 * 64 * WAVES).all(), (nint, nsh)
        with_bnd, without_bnd = with_bnd + facts["with_bnd"], without_bnd + facts["without_bnd"]
        odd += int((nint % 2 == 1).sum())
        even += int((nint % 2 == 0).sum())
        small_shared += int(((nsh < 512) & (nsh % 512 != 0)).sum())
        cx = fa.Context(0, geometry="trilinear", block_elems=be, waves=WAVES)
        g, info = step(cs, cx, start, facts)
        cx.close()
        print(f"block_elems={be}: u {relmax(g[0], ref[0]):.2e} v {relmax(g[1], ref[1]):.2e}, odd interior counts "
              f"{facts['odd_int']}, even {facts['even_int']}")
        assert info["block_loop"] == 0, info
        assert relmax(g[0], ref[0]) < TOL_RK and relmax(g[1], ref[1]) < TOL_RK, be
    # (7-element blocks: 6 odd and 12 even interior counts, 8 of the 18 blocks without a boundary entry, every shared
    # range shorter than 512; blocks of 30: interior ranges of up to 1016 vectors, 8 short of the first batch)
    assert odd > 0 and even > 0 and small_shared > 0 and with_bnd > 0 and without_bnd > 0, (odd, even, small_shared, with_bnd,
                                                                                          without_bnd)


def test_a_layout_that_does_not_fit_runs_the_block_loop(rk_case, driver, tmp_path):
    cs, start, ref = rk_case
    facts, rec = layout(driver, tmp_path, cs, BLOCK_TOO_LARGE)
    assert (rec["nint"] // 2 > FIRST_BATCH_VECTORS).any(), rec["nint"]
    cx = fa.Context(0, geometry="trilinear", block_elems=BLOCK_TOO_LARGE, waves=WAVES)
    g, info = step(cs, cx, start, facts)
    cx.close()
    print(f"block_elems={BLOCK_TOO_LARGE}: u {relmax(g[0], ref[0]):.2e} v {relmax(g[1], ref[1]):.2e}")
    assert info["block_loop"] == 1, info
    assert relmax(g[0], ref[0]) < TOL_RK and relmax(g[1], ref[1]) < TOL_RK


def test_deterministic_twice_the_same_bits(rk_case, driver, tmp_path):
    cs, start, ref = rk_case
    be = BLOCK_SIZES[0]
    facts, _ = layout(driver, tmp_path, cs, be)
    outs = []
    for _ in range(2):
        cx = fa.Context(0, geometry="trilinear", block_elems=be, waves=WAVES, deterministic=1)
        g, info = step(cs, cx, start, facts)
        cx.close()
        assert info["block_loop"] == 0
        outs.append(g)
    assert relmax(outs[0][0], ref[0]) < TOL_RK and relmax(outs[0][1], ref[1]) < TOL_RK
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])
