"""The block kernel on the shapes where a range guard of its prologue or epilogue can go wrong, with one workgroup per
block (the straight-line kernel, template parameter WALK = 0 of k_block_op) and with walking workgroups (WALK = 1):

  be1-p2     one-element blocks at degree 2: a block whose interior range is ONE dof -- no 16-byte vector, only the odd tail
  one-block  the whole mesh (2 x 2 x 1 cells) in one block: no shared dof, no partial sum
  p4-be64    degree 4, the 4 x 4 x 4 box as one 64-element block: interior range, dofmaps and coefficients longer than
             the first batch of the prologue, several passes of the epilogue
  p7         degree 7, default blocks on the 4 x 4 x 4 box: interior ranges longer than the first batch (of even length,
             where p4-be64's is odd), shared ranges within it

each with perturbed (trilinear), affine or streamed geometry, LDS atomics and deterministic rounds, and the two-input
models on two of them; quadrilaterals; 320 two-element blocks walked and not walked, bit for bit; two x-slabs with the
interface blocks launched first, so that a launch starts at a block other than 0.

Tolerances: fp64 as tests/test_gpu_parity.py (1e-12 stiffness, 1e-14 mass, 1e-10 RK); fp32 against the float oracle's
own rounding error (fp32_budget.py), like tests/test_gpu_fp32_budget.py."""
import numpy as np
import pytest

import fenicsxfus_amd as fa
import fp32_budget as fb
from live_cases import TOL_RK, Case
from test_block_records_host import RECORD, build_driver, run_driver
from util import assert_live

pytestmark = pytest.mark.gpu

TOL_OP, TOL_MASS = 1e-12, 1e-14
NSTEPS = 6
# name -> (cells, degree, block_elems, perturb, geometry paths)
SHAPES = {
    "be1-p2": ((3, 3, 3), 2, 1, 0.1, ("trilinear", "stream")),
    "one-block": ((2, 2, 1), 4, 4, 0.0, ("affine", "diag", "trilinear", "stream")),
    "p4-be64": ((4, 4, 4), 4, 64, 0.1, ("trilinear", "stream")),
    "p7": ((4, 4, 4), 7, 8, 0.1, ("trilinear",)),   # 8 elements: the default block of the degree (asserted)
}
# path -> (context keywords, options, geometry mode)
GEOMETRY = {
    "stream": (dict(geometry="stream"), {}, "stream"),
    "trilinear": (dict(geometry="trilinear"), {}, "trilinear"),
    "affine": (dict(), {"diag_metric": 0}, "affine"),
    "diag": (dict(), {"diag_metric": 1}, "affine"),
}
# threads of a workgroup (at most) and 16-byte interior vectors per thread in the prologue's first batch (kernels.hpp: UI)
FIRST_BATCH = {4: 512 * 2, 7: 256 * 5}


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return build_driver(tmp_path_factory.mktemp("addr"), sanitize=False)


_cases = {}


def case_of(orc, kind, shape, dtype=np.float64):
    key = (kind, shape, np.dtype(dtype).name)
    if key not in _cases:
        n, P, _, perturb, _ = SHAPES[shape]
        _cases[key] = Case(orc, kind, n, P, perturb=perturb, nsteps=NSTEPS, dtype=dtype)
    return _cases[key]


def context(path, block_elems, deterministic, walk=0):
    ckw, opts, mode = GEOMETRY[path]
    cx = fa.Context(0, block_elems=block_elems, deterministic=deterministic, **ckw)
    for k, v in opts.items():
        cx.set_option(k, v)
    cx.set_option("walk", walk)
    return cx, mode


def records(driver, tmp_path, cs, block_elems):
    """The layout's facts and its per-block records, from the host driver on the case's dofmap."""
    facts, raw, _ = run_driver(driver, tmp_path / "in.bin", cs.tdim, cs.P, cs.pr.dm, cs.pr.mesh.cell_centroids(),
                               block_elems, 4)
    return facts, raw.view(RECORD)


def check_shape(shape, facts, rec):
    nint, nsh = rec["nint"].astype(np.int64), (rec["nloc"] - rec["nint"]).astype(np.int64)
    if shape == "be1-p2":
        assert (rec["nelem"] == 1).all() and (nint == 1).any(), nint
    elif shape == "one-block":
        assert facts["blocks"] == 1 and facts["shared"] == 0 and nsh[0] == 0
    else:
        P = SHAPES[shape][1]
        assert (nint // 2 > FIRST_BATCH[P]).any(), nint
        if shape == "p7":      # even interior ranges, shared ranges within the first batch
            assert (nint % 2 == 0).all() and (nsh > 0).all() and (nsh <= 256 * 5).all(), (nint, nsh)
        else:                  # an odd one
            assert facts["blocks"] == 1 and rec["nelem"][0] == 64 and nint[0] % 2 == 1


def relmax(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def run(cs, model, start):
    model.init()
    model.set_state(*start)
    model.rk4_steps(0.0, cs.dt, cs.nsteps)
    out = model.u_sol().x.array.copy(), model.v_n.x.array.copy()
    model.close()
    return out


def fp64_reference(cs):
    start = cs.start()
    ref = cs.oracle(*start, fixed=True)
    assert_live(ref, cs.regions)
    return start, ref


@pytest.mark.parametrize("shape", list(SHAPES))
def test_operator_actions(orc, driver, tmp_path, shape):
    """Stiffness and mass actions on every geometry path of the shape, LDS atomics and deterministic rounds."""
    _, P, be, _, paths = SHAPES[shape]
    cs = case_of(orc, "linear", shape)
    facts, rec = records(driver, tmp_path, cs, be)
    check_shape(shape, facts, rec)
    pr = cs.pr
    rng = np.random.default_rng(P)
    x = rng.standard_normal(pr.ndofs)
    coef = rng.uniform(0.5, 2.0, pr.mesh.num_cells)
    refK, refM = pr.K(x, coef), pr.M(x, coef)
    if shape == "p7":
        cx = fa.Context(0)
        d = fa.SpectralOperatorData(pr.V, cx)
        assert d.info()["nblocks"] == facts["blocks"] and d.info()["interior_dofs"] == facts["interior"]
        d.close()
        cx.close()
    for path in paths:
        for det in (0, 1):
            cx, mode = context(path, be, det)
            d = fa.SpectralOperatorData(pr.V, cx)
            assert d.geometry_mode() == mode
            info = d.info()
            assert (info["nblocks"], info["interior_dofs"], info["shared_dofs"]) == (
                facts["blocks"], facts["interior"], facts["shared"]), (info, facts)
            y = d.stiffness(x, coef, np.zeros(pr.ndofs))
            ym = d.mass(x, coef, np.zeros(pr.ndofs))
            d.close()
            cx.close()
            print(f"{shape} {path} deterministic={det}: stiffness {relmax(y, refK):.2e} mass {relmax(ym, refM):.2e}")
            assert relmax(y, refK) < TOL_OP and relmax(ym, refM) < TOL_MASS, (shape, path, det)


@pytest.mark.parametrize("kind,shape", [("linear", s) for s in SHAPES] + [(k, s) for k in ("lossy", "westervelt")
                                                                         for s in ("be1-p2", "p4-be64")])
def test_rk4_steps(orc, kind, shape):
    """Six RK4 steps from a live start against the oracle: the fused stage epilogue on every geometry path of the
    shape, with one and (lossy, Westervelt) two operator inputs."""
    _, _, be, _, paths = SHAPES[shape]
    cs = case_of(orc, kind, shape)
    start, ref = fp64_reference(cs)
    for path in paths:
        for det in (0, 1):
            cx, mode = context(path, be, det)
            model = cs.model(cx)
            assert model.data.geometry_mode() == mode
            g = run(cs, model, start)
            cx.close()
            print(f"{kind} {shape} {path} deterministic={det}: u {relmax(g[0], ref[0]):.2e} v {relmax(g[1], ref[1]):.2e}")
            assert relmax(g[0], ref[0]) < TOL_RK and relmax(g[1], ref[1]) < TOL_RK, (kind, shape, path, det)


@pytest.mark.parametrize("shape", ["be1-p2", "p4-be64"])
def test_fp32(orc, shape):
    """The fp32 kernels on the same shapes (trilinear geometry), held to the float oracle's own rounding error."""
    _, P, be, _, _ = SHAPES[shape]
    cs = case_of(orc, "linear", shape, np.float32)
    pr, pr64 = cs.prt, cs.pr64r
    rng = np.random.default_rng(P)
    x = rng.standard_normal(pr.ndofs).astype(np.float32)
    coef = rng.uniform(0.5, 2.0, pr.mesh.num_cells).astype(np.float32)
    refK, refM = pr.K(x, coef), pr.M(x, coef)
    x64, c64 = x.astype(np.float64), coef.astype(np.float64)
    refK64, refM64 = pr64.K(x64, c64), pr64.M(x64, c64)
    assert_live((refK64, refM64), cs.regions)
    start, r32, r64 = cs.fp32_refs()
    assert_live(r64, cs.regions)
    for det in (0, 1):
        label = f"{shape} deterministic={det}"
        cx, _ = context("trilinear", be, det)
        d = fa.SpectralOperatorData(pr.V, cx)
        assert d.dtype == np.dtype(np.float32)
        y = d.stiffness(x, coef, np.zeros(pr.ndofs, np.float32))
        ym = d.mass(x, coef, np.zeros(pr.ndofs, np.float32))
        d.close()
        g = run(cs, cs.model(cx), start)
        cx.close()
        fb.check(f"[addressing-stiffness] {label}", y, refK, refK64, cs.regions)
        fb.check(f"[addressing-mass] {label}", ym, refM, refM64, cs.regions)
        fb.check(f"[addressing-rk4] {label}", g, r32, r64, cs.regions)


@pytest.mark.parametrize("kind", ["linear", "westervelt"])
def test_quadrilaterals(orc, kind):
    """TD = 2: the same prologue and epilogue on a 9 x 7 quadrilateral mesh, default blocks and one-element blocks."""
    key = (kind, "quad")
    if key not in _cases:
        _cases[key] = Case(orc, kind, (9, 7), 4, nsteps=NSTEPS)
    cs = _cases[key]
    start, ref = fp64_reference(cs)
    for be in (None, 1):
        for det in (0, 1):
            cx = fa.Context(0, block_elems=be, deterministic=det)
            g = run(cs, cs.model(cx), start)
            cx.close()
            assert relmax(g[0], ref[0]) < TOL_RK and relmax(g[1], ref[1]) < TOL_RK, (kind, be, det)


# cells -> (blocks of two elements, the settings of option "walk" compared with 0)
WALK_MESHES = {(10, 8, 8): (320, (1, 2)), (12, 12, 8): (576, (2,))}


def compute_units():
    """Compute units of device 0 (hipDeviceAttributeMultiprocessorCount = 63 in hip_runtime_api.h)."""
    import ctypes as C
    n = C.c_int(0)
    assert C.CDLL("libamdhip64.so").hipDeviceGetAttribute(C.byref(n), C.c_int(63), C.c_int(0)) == 0
    assert 0 < n.value <= 1024, n.value
    return n.value


@pytest.mark.parametrize("n", list(WALK_MESHES), ids=["320-blocks", "576-blocks"])
def test_walked_and_not_walked_blocks_agree_bitwise(orc, n):
    """Two-element blocks, deterministic: one workgroup per block (the straight-line kernel) and walking workgroups
    (option "walk" = w: w workgroups per compute unit, the kernel with the block loop) give the oracle's state and the
    same bits.  A launch walks only where w x compute units is below the number of blocks: that is asserted for
    walk = 1 on 320 blocks and walk = 2 on 576; walk = 2 on 320 blocks is compared as well, walking or not."""
    nblocks, walks = WALK_MESHES[n]
    if n not in _cases:
        _cases[n] = Case(orc, "linear", n, 4, L=0.02, nsteps=NSTEPS)
    cs = _cases[n]
    start, ref = fp64_reference(cs)
    cus = compute_units()
    assert min(walks) * cus < nblocks, (cus, nblocks)       # fewer workgroups than blocks: the launch walks
    outs = {}
    for walk in (0, *walks):
        cx, _ = context("trilinear", 2, 1, walk)
        model = cs.model(cx)
        assert model.data.info()["nblocks"] == nblocks
        outs[walk] = run(cs, model, start)
        cx.close()
        assert relmax(outs[walk][0], ref[0]) < TOL_RK and relmax(outs[walk][1], ref[1]) < TOL_RK, walk
    for walk in walks:
        assert np.array_equal(outs[0][0], outs[walk][0]) and np.array_equal(outs[0][1], outs[walk][1]), walk


def test_two_slabs_interface_blocks_first(orc):
    """Two x-slabs with option "overlap_blocks" = 1: each rank's interface blocks are launched first and the rest
    after them, so that a launch of the block kernel starts at a block other than 0."""
    cs = Case(orc, "linear", (8, 2, 2), 3, L=0.032, nsteps=NSTEPS)
    start, ref = fp64_reference(cs)
    ctxs = [fa.Context(0, block_elems=4) for _ in range(2)]
    for cx in ctxs:
        cx.set_option("overlap_blocks", 1)
    fa.Context.init_local_group(ctxs)
    models = [cs.model(ctxs[r], rank=r, size=2) for r in range(2)]
    assert all(m.data.info()["nblocks"] == 4 for m in models)
    fa.group_finish_setup(models)
    for m in models:
        off = m.V.global_offset
        m.init()
        m.set_state(start[0][off:off + m.data.ndofs], start[1][off:off + m.data.ndofs])
    fa.group_rk4_steps(models, 0.0, cs.dt, cs.nsteps)
    for m in models:
        off, k = m.V.global_offset, m.data.ndofs
        assert np.abs(m.u_sol().x.array - ref[0][off:off + k]).max() < TOL_RK * np.abs(ref[0]).max()
        assert np.abs(m.v_n.x.array - ref[1][off:off + k]).max() < TOL_RK * np.abs(ref[1]).max()
    for m in models:
        m.close()
    for cx in ctxs:
        cx.close()
