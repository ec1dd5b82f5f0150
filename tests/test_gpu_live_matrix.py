"""The fp64 block kernels against the double oracle from LIVE starts (test_gpu_live_state.py's docstring says why),
over the whole matrix: family x degree 2-10 (4: test_gpu_live_state.py) x geometry path x {lean stage kinds 4-7,
accumulator kinds 0/1/3} x two block settings, and Lossy / Westervelt at the RK orders 1-3.  The stage epilogue of
k_block_op is different code across these: ranges per pass (EPI2 / epiu_of), operands requested before the barrier
(epi_early), the Westervelt division, the one-DOF tail, the two-waves-per-element kernels of the degrees 8-10.

Block settings, each proven through model.data.info():
  split  block_elems = cells / 4: at least three blocks and shared DOFs (the shared-DOF stage kernel, the
         pseudo-partials of shared boundary DOFs);
  long   block_elems = cells: ONE block whose interior range -- the whole mesh; (2 P + 1)^3 DOFs on the (2, 2, 2)
         meshes, an odd number, so the one-DOF tail runs too -- needs a second epilogue pass: interior_dofs >
         2 EPIU threads (a thread takes EPIU ranges of two DOFs per pass).  Where the library shrinks that block to
         fit LDS (SHRUNK), the blocks it makes instead still average more than that.
The CPU guards of every case are in test_live_guards.py."""
import pytest

import fenicsxfus_amd as fa
from live_cases import CASES, TOL_RK
from test_gpu_live_state import check, live_reference, run_gpu

pytestmark = pytest.mark.gpu

KINDS = ("linear", "lossy", "westervelt")
DEGREES = (2, 3, 5, 6, 7, 8, 9, 10)
NF = {"linear": 1, "lossy": 2, "westervelt": 2}        # operator inputs per stage (fus_op_create: nfields)
# an explicit block_elems keeps fus_op_create at four waves at every degree (eight only for its own 32-element blocks
# of degree 4)
THREADS = 256

# (kind, degree) whose one block of the whole (2, 2, 2) mesh does not fit 160 KB of LDS, so that fus_op_create halves
# block_elems until it does: 8 bytes per local DOF and operator input plus 8 for the accumulator, (2 P + 1)^3 DOFs.
SHRUNK = {
    ("lossy", 9): "6859 DOFs x 24 B = 161 KB",
    ("westervelt", 9): "6859 DOFs x 24 B = 161 KB",
    ("linear", 10): "9261 DOFs x 16 B = 145 KB + 22 KB of exchange tiles + 21 KB of local dofmaps",
    ("lossy", 10): "9261 DOFs x 24 B = 217 KB",
    ("westervelt", 10): "9261 DOFs x 24 B = 217 KB",
}


def epiu(P, mode, nf):
    """Interior ranges per epilogue pass of the fp64 k_block_op (kernels.hpp: EPI2, epiu_of<double>)."""
    if P <= 4 and nf == 1:
        return 2
    if nf != 1 or mode == "stream" or P <= 5 or (P == 6 and mode == "affine"):
        return 1
    return 4


def case_name(kind, P, box):
    if box:
        return f"{kind}-p{P}-box"
    return f"{kind}-p{P}-long" if f"{kind}-p{P}-long" in CASES else f"{kind}-p{P}"


def paths(P, box):
    """(context keywords, options, geometry mode, diagonal metric or None) of a case's geometry paths."""
    if box:
        if P <= 7:
            return [(dict(), {"diag_metric": 1}, "affine", True), (dict(), {"diag_metric": 0}, "affine", False)]
        return [(dict(), {}, "affine", False)]
    out = [(dict(), {}, "trilinear", None)]
    if P in (5, 7, 9):
        out.append((dict(geometry="stream"), {}, "stream", None))
    return out


def context(be, ckw, opts, lean=None):
    cx = fa.Context(0, block_elems=be, **ckw)
    if lean is not None:
        cx.set_option("lean_rk4", lean)
    for k, val in opts.items():
        cx.set_option(k, val)
    return cx


def assert_blocks(cs, info, setting, mode):
    if setting == "split":
        assert info["nblocks"] >= 3 and info["shared_dofs"] > 0, info
        return
    need = 2 * epiu(cs.P, mode, NF[cs.kind]) * THREADS
    if cs.tdim == 3 and (cs.kind, cs.P) in SHRUNK:
        assert info["nblocks"] > 1 and info["interior_dofs"] > need * info["nblocks"], (info, need)
    else:
        assert info["nblocks"] == 1 and info["shared_dofs"] == 0, info
        assert info["interior_dofs"] == cs.pr.ndofs > need, (info, need)
        assert cs.n != (2, 2, 2) or cs.pr.ndofs % 2 == 1          # (2 P + 1)^3: the one-DOF tail


def run_settings(cs, u0, v0, ref, ckw, opts, mode, diag, leans, settings):
    ncells = cs.pr.mesh.num_cells
    for setting in settings:
        be = {"default": None, "split": ncells // 4, "long": ncells}[setting]
        for lean in leans:
            cx = context(be, ckw, opts, lean)
            model = cs.model(cx)
            assert model.data.geometry_mode() == mode
            if diag is not None:
                assert model.data.uses_diag_metric() == diag
            if setting != "default":
                assert_blocks(cs, model.data.info(), setting, mode)
            model.close()
            check(run_gpu(cs, cx, u0, v0), ref, TOL_RK)
            cx.close()


@pytest.mark.parametrize("box", [False, True], ids=["perturbed", "box"])
@pytest.mark.parametrize("P", DEGREES)
@pytest.mark.parametrize("kind", KINDS)
def test_matrix(orc, kind, P, box):
    cs, u0, v0, ref = live_reference(orc, case_name(kind, P, box))
    assert (cs.perturb == 0) == box and cs.order == 4
    for ckw, opts, mode, diag in paths(P, box):
        run_settings(cs, u0, v0, ref, ckw, opts, mode, diag, (1, 0), ("split", "long"))


@pytest.mark.parametrize("P", [4, 9])
def test_lossy_quadrilaterals(orc, P):
    """(no LDS budget to exhaust in 2-D: the one block holds the whole mesh at both degrees)"""
    cs, u0, v0, ref = live_reference(orc, f"lossy-quad-p{P}")
    assert cs.perturb > 0
    run_settings(cs, u0, v0, ref, dict(), {}, "stream", None, (1, 0), ("default", "split", "long"))


@pytest.mark.parametrize("order", [1, 2, 3])
@pytest.mark.parametrize("kind", ["lossy", "westervelt"])
def test_lower_rk_orders_two_inputs(orc, kind, order):
    """rk_order 1-3 of the two-input models: stage kinds 0 and 1 with NF == 2, k_boundary_partial at every stage and
    the (u_, v_) -> (u0, v0) copy after the step, against the oracle's tables of the same orders."""
    cs, u0, v0, ref = live_reference(orc, f"{kind}-rk{order}")
    assert cs.order == order
    run_settings(cs, u0, v0, ref, dict(), {}, "trilinear", None, (None,), ("default", "split"))


@pytest.mark.parametrize("order", [2, 3])
@pytest.mark.parametrize("kind", KINDS)
def test_lower_rk_orders_degree_8(orc, kind, order):
    cs, u0, v0, ref = live_reference(orc, f"{kind}-p8-rk{order}")
    assert cs.order == order
    run_settings(cs, u0, v0, ref, dict(), {}, "trilinear", None, (None,), ("default", "split"))
