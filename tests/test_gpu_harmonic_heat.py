"""The per-harmonic heat load on the device (fusmi.h "per-harmonic heat load"; BioheatSpectralExplicit.set_heat_from with
a 2-D absorption) against the numpy reference of harmonic_heat_ref.py evaluated on the device's own monitor maps.

(1) the load against the reference, and what must not move; (2) arguments and call sequence; (3) two slabs in one
process; (4) the Fubini case: the harmonics' share of the heat; (5) the C++ example."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
from scipy.special import jv

import fenicsxfus_amd as fa
import thermal_ref
from fenicsxfus_amd import _abi, monitor
from harmonic_heat_ref import harmonic_heat
from thermal_ref import case, materials, rel
from util import Problem, live_state

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL64 = 1e-10                       # test_gpu_thermal.py's fp64 tolerance of the stepper
F0, P0, S0 = 0.5e6, 6e4, 1500.0
NHARM, Y = 3, 1.1


def _wave_model(cs, ctx, westervelt=False, nharm=NHARM):
    """The wave run of test_gpu_thermal.py::_wave_model with the monitor keeping ``nharm`` harmonics: live start, 18
    steps.  ``westervelt``: a Westervelt model with the same materials."""
    pr = cs.prt
    bone = materials(pr.mesh, cs.hi)[0] == 0.32
    c = np.where(bone, 2800.0, 1500.0).astype(cs.dtype)
    rho = np.where(bone, 1850.0, 1000.0).astype(cs.dtype)
    dt = 0.5 * 0.003 / (2800.0 * cs.P ** 2)
    tags = fa.tag_box_boundary(pr.mesh)
    if westervelt:
        w0 = 2 * np.pi * F0
        delta = np.where(bone, fa.compute_diffusivity_of_sound(w0, 2800.0, 400.0 / 20.0 * np.log(10.0)),
                         fa.compute_diffusivity_of_sound(w0, 1500.0, 0.2)).astype(cs.dtype)
        beta = np.where(bone, 6.0, 3.5).astype(cs.dtype)
        mdl = fa.WesterveltSpectralExplicit(pr.mesh, tags, cs.P, c, rho, delta, beta, F0, P0, S0, 4, dt, V=pr.V, ctx=ctx)
    else:
        mdl = fa.LinearSpectralExplicit(pr.mesh, tags, cs.P, c, rho, F0, P0, S0, 4, dt, V=pr.V, ctx=ctx)
    u0, v0 = live_state(pr, 11, P0, F0)
    mdl.init()
    mdl.set_state(u0, v0)
    mdl.monitor(which="u", nharm=nharm, every=1)
    mdl.rk4_steps(0.0, dt, 18)
    return mdl, dt, bone, c.astype(np.float64), rho.astype(np.float64)


def _wave_maps(mdl, nharm=NHARM):
    mdl.u_sol()
    out = {"u": mdl.u_n.x.array.copy(), "v": mdl.v_n.x.array.copy()}
    for q in ("max", "min", "mean", "rms"):
        out[q] = mdl.monitor_get(q).x.array.copy()
    for k in range(1, nharm + 1):
        out[f"cos{k}"] = mdl.monitor_get("cos", k).x.array.copy()
        out[f"sin{k}"] = mdl.monitor_get("sin", k).x.array.copy()
    return out


def _rows(bone, K, dtype):
    """alpha_k per cell, bone and tissue apart, alpha ~ f^1.1, rounded to the scalar type (returned in double too)."""
    a = monitor.power_law(np.where(bone, 20.0, 0.5), Y, K).astype(dtype)
    return a, a.astype(np.float64)


def _reference(cs, maps, rows64, rho, c):
    K = len(rows64)
    return harmonic_heat(cs.pr, rows64, rho, c, [maps[f"cos{k}"] for k in range(1, K + 1)],
                         [maps[f"sin{k}"] for k in range(1, K + 1)])


# ---- (1) the load ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [3, 2])
@pytest.mark.parametrize("label", ["A", "B", "F"])
def test_load_against_the_reference(orc, label, K):
    """Cases A (trilinear P3 fp64, 1300 DOFs), B (quadrilaterals with bone cells, 525 DOFs: the vector tail is live; on a
    Westervelt model) and F (fp32); monitor(nharm=3) over 18 steps from a live start; K = 3 and K = 2, fewer harmonics
    than the monitor holds.  h against sum_k M(2 alpha_k / (rho c)) 1 .* (COS_k^2 + SIN_k^2) / 2 on the pulled maps: error
    / max <= 1e-12 in fp64 (K <= 8 positive products summed in double, about (K + 4) 2^-53, and the maps' own rounding),
    1e-5 in fp32 (the rms path's bound).  Five thermal steps follow the reference driven by that vector (fp64), then
    five steps with heat_scale = 0 cool.  The wave state and every monitor map keep their bits; the rms path gives the
    same bits before and after the harmonic call, and the harmonic call gives its own bits again after it."""
    cs = case(orc, label)
    t = cs.dtype
    ctx = fa.Context(0, deterministic=True)
    mdl, wdt, bone, c, rho = _wave_model(cs, ctx, westervelt=label == "B")
    before = _wave_maps(mdl)
    th = fa.BioheatSpectralExplicit(cs.prt.mesh, cs.P, cs.k.astype(t), cs.rho_c.astype(t), cs.w.astype(t), model=mdl)
    th.init()
    alpha1 = np.where(bone, 20.0, 0.5).astype(t)
    rows, rows64 = _rows(bone, K, t)
    th.set_heat_from(mdl, alpha1)
    rms1 = th.heat().x.array.copy()
    th.set_heat_from(mdl, rows)
    h = th.heat().x.array.copy()
    th.set_heat_from(mdl, alpha1)
    rms2 = th.heat().x.array.copy()
    th.set_heat_from(mdl, rows)
    again = th.heat().x.array.copy()
    href = _reference(cs, before, rows64, rho, c)
    err = float(np.abs(h - href).max() / href.max())
    print(f"case {label}, K = {K}: per-harmonic load, error / max {err:.3e}; max h {href.max():.3e} W, "
          f"rms load max {rms1.max():.3e} W")
    assert h.dtype == t and href.max() > 0
    assert err <= (1e-12 if t == np.float64 else 1e-5)
    assert np.array_equal(rms1, rms2) and rms1.max() > 0 and np.array_equal(h, again)
    assert not np.array_equal(h, rms1)
    if K < NHARM:                                                  # the third harmonic is live: leaving it out shows
        full = _reference(cs, before, _rows(bone, NHARM, t)[1], rho, c)
        assert np.abs(full - href).max() > 1e-3 * href.max()
    th.steps(cs.dt, 5)
    got = th.rise().x.array.astype(np.float64)
    th.steps(cs.dt, 5, heat_scale=0.0)
    cooled = th.rise().x.array.astype(np.float64)
    if t == np.float64:
        ref = cs.ref.run(np.zeros(cs.pr.ndofs), cs.dt, 5, h.astype(np.float64))
        assert np.abs(ref).max() > 0 and rel(got, ref) <= TOL64
        assert rel(cooled, cs.ref.run(ref, cs.dt, 5, h.astype(np.float64), 0.0)) <= TOL64
    assert 0 < cs.ref.m_c @ cooled < cs.ref.m_c @ got               # perfusion carries energy away, nothing adds any
    after = _wave_maps(mdl)
    for key in before:
        assert np.array_equal(before[key], after[key]), key
    th.close(), mdl.close(), ctx.close()


# ---- (2) arguments and call sequence ------------------------------------------------------------------------------------
def test_errors_leave_the_load_in_place(orc):
    cs = case(orc, "A")
    pr, nc = cs.prt, cs.prt.mesh.num_cells
    ctx = fa.Context(0, deterministic=True)
    mdl, wdt, bone, _, _ = _wave_model(cs, ctx)
    other = _wave_model(cs, ctx)[0]                                 # its own operator data
    th = fa.BioheatSpectralExplicit(pr.mesh, cs.P, cs.k, cs.rho_c, cs.w, model=mdl)
    th.init()
    rows = _rows(bone, 2, cs.dtype)[0]
    th.set_heat_from(mdl, rows)
    h0 = th.heat().x.array.copy()
    assert h0.max() > 0
    L = _abi.lib()

    def refused(code, what, call):
        with pytest.raises(fa.FusError, match=f"error {code}: .*fus_thermal_set_heat_from_harmonics.*{what}"):
            call()
        assert np.array_equal(th.heat().x.array, h0)                # the load is as it was

    assert L.fus_thermal_set_heat_from_harmonics(th.h, mdl.h, C.c_int(2), None) == -1
    refused(-1, "null", lambda: _abi.check(L.fus_thermal_set_heat_from_harmonics(th.h, None, C.c_int(2), _abi.ptr(rows))))
    refused(-1, "another fus_op", lambda: th.set_heat_from(other, rows))
    refused(-1, r"1\.\.8", lambda: th.set_heat_from(mdl, monitor.power_law(np.full(nc, 0.5), Y, 9)))
    refused(-1, r"1\.\.8", lambda: _abi.check(L.fus_thermal_set_heat_from_harmonics(th.h, mdl.h, C.c_int(0), _abi.ptr(rows))))
    neg, nan, inf = rows.copy(), rows.copy(), rows.copy()
    neg[1, nc // 2], nan[0, 0], inf[1, nc - 1] = -1.0, np.nan, np.inf
    for bad in (neg, nan, inf):
        refused(-1, "absorption", lambda bad=bad: th.set_heat_from(mdl, bad))
    refused(-4, "fewer harmonics", lambda: th.set_heat_from(mdl, _rows(bone, NHARM + 1, cs.dtype)[0]))
    with pytest.raises(fa.FusError, match="absorption: expected"):
        th.set_heat_from(mdl, np.zeros((2, nc + 1)))
    mdl.monitor(which="v", nharm=NHARM, every=1)
    mdl.rk4_steps(0.0, wdt, 1)
    refused(-4, "FUS_V", lambda: th.set_heat_from(mdl, rows))
    mdl.monitor(which="u", nharm=NHARM, every=1)
    refused(-4, "no sample", lambda: th.set_heat_from(mdl, rows))
    mdl.monitor_off()
    refused(-4, "monitor is off", lambda: th.set_heat_from(mdl, rows))
    # K = 1 and K = the monitor's own 8 run (the first touches no scratch plane, the second every plane of the monitor)
    mdl.monitor(which="u", nharm=8, every=1)
    mdl.rk4_steps(0.0, wdt, 2)
    maps = _wave_maps(mdl, 8)
    c = np.where(bone, 2800.0, 1500.0)
    rho = np.where(bone, 1850.0, 1000.0)
    for K in (1, 8):
        a = _rows(bone, K, cs.dtype)
        th.set_heat_from(mdl, a[0])
        href = _reference(cs, maps, a[1], rho, c)
        assert href.max() > 0 and np.abs(th.heat().x.array - href).max() <= 1e-12 * href.max()
    th.set_heat(None)
    assert np.array_equal(th.heat().x.array, np.zeros(pr.ndofs))
    th.close(), other.close(), mdl.close(), ctx.close()


# ---- (3) two slabs ------------------------------------------------------------------------------------------------------
def test_two_slabs_in_one_process(orc):
    """Set up as test_gpu_thermal_multirank.py::test_heat_from_the_monitors_of_slab_models, monitors with two harmonics,
    K = 2: every member's heat() equals the slice of the single-rank object's within 1e-10 of its max, with identical
    bits on the interface plane; five group steps follow the reference driven by the single-rank load; a load set on one
    member only makes group_thermal_finish fail."""
    import test_multirank as tm
    K = 2
    pr = Problem(orc, tm.N_GLOBAL, tm.P, hi=tm.HI, perturb=0.1)
    wdt = tm.dt_value()
    u0, v0 = live_state(pr, tm.SEED, tm.P0, tm.F0)
    k, rho_c, w = materials(pr.mesh, tm.HI)

    def rows_of(mesh):
        return monitor.power_law(np.where(materials(mesh, tm.HI)[0] == thermal_ref.BONE["k"], 20.0, 0.5), Y, K)

    def wave(mesh, V, ctx):
        c, rho = tm.material(mesh)
        return fa.LinearSpectralExplicit(mesh, fa.tag_box_boundary(mesh), tm.P, c, rho, tm.F0, tm.P0, tm.S0, 4, wdt, V=V, ctx=ctx)

    ctx = fa.Context(0, deterministic=True)
    one = wave(pr.mesh, pr.V, ctx)
    one.init()
    one.set_state(u0, v0)
    one.monitor(which="u", nharm=K, every=1)
    one.rk4_steps(0.0, wdt, tm.NSTEPS)
    th = fa.BioheatSpectralExplicit(pr.mesh, tm.P, k, rho_c, w, model=one)
    th.init()
    th.set_heat_from(one, rows_of(pr.mesh))
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
        mdl.monitor(which="u", nharm=K, every=1)
    fa.group_rk4_steps(models, 0.0, wdt, tm.NSTEPS)
    for mdl, mesh in zip(models, meshes):
        kr, rcr, wr = materials(mesh, tm.HI)
        bios.append(fa.BioheatSpectralExplicit(mesh, tm.P, kr, rcr, wr, model=mdl))
    fa.group_thermal_finish(bios)
    for b in bios:
        b.init()
    bios[0].set_heat_from(models[0], rows_of(meshes[0]))
    with pytest.raises(fa.FusError, match="error -4: .*a heat load waits on some members only"):
        fa.group_thermal_finish(bios)
    assert np.array_equal(bios[0].heat().x.array, np.zeros(len(gids[0])))       # nothing has become the load yet
    bios[1].set_heat_from(models[1], rows_of(meshes[1]))
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
    print(f"per-harmonic load of two slabs: error / max {herr:.3e}; 5 steps {err:.3e}")
    assert herr <= 1e-10 and err <= TOL64
    plane = len(np.intersect1d(gids[0], gids[1]))
    assert plane > 0 and np.array_equal(h[0][-plane:], h[1][:plane]) and np.array_equal(got[0][-plane:], got[1][:plane])
    assert np.abs(h[0][-plane:]).max() > 0


# ---- (4) the harmonics' share of the heat: Fubini ---------------------------------------------------------------------------
FUBINI_ORACLE_ERR = 1.705497e-4     # the CPU oracle through the same procedure (docstring of test_fubini_heat)


def test_fubini_heat(orc):
    """The Westervelt validation case of test_gpu_monitor.py::test_harmonics_against_fubini at degree 4, epw = 8, nharm = 4
    over a whole-period window, with the thermoviscous law alpha_k = alpha k^2: the load summed over the DOFs against the
    same numpy reference evaluated on the exact series maps COS_k = -p0 B_k sin(k w0 X / c0), SIN_k = p0 B_k cos(k w0 X / c0).
    The CPU oracle, stepped one step at a time over the same 2592 steps and accumulated in numpy by the monitor's rule
    (288 samples), gives the total 1.705151899e-04 against the series' 1.704861136e-04: relative error 1.705497e-04.  The
    bound is twice that, 3.410994e-04, far below 0.21, the squared form of the reference's 1e-1 field threshold.  The
    load also exceeds the fundamental-only load (K = 1) by the series' own ratio (1.155656; the oracle: 1.155759) minus
    that bound: the harmonics' share of the heat is there."""
    from test_gpu_reference_python_tests import interval_as_box
    degree, epw = 4, 8
    f0, c0, rho0, beta0, L, nharm = 10.0, 1.0, 1.0, 0.01, 1.0, 4
    w0, u0 = 2 * np.pi * f0, 1.0
    p0 = rho0 * c0 * u0
    bound = 2.0 * FUBINI_ORACLE_ERR
    assert bound < 0.21
    pr, tags, h = interval_as_box(orc, degree, epw, f0, c0, L)
    nc = pr.mesh.num_cells
    dt, nsteps, skip, spp = monitor.whole_period_window(f0, 0.9 * h / (c0 * degree**2), L / c0 + 8 / f0, 2, nharm=nharm)
    ctx = fa.Context(0)
    mdl = fa.WesterveltSpectralExplicit(pr.mesh, tags, degree, np.full(nc, c0), np.full(nc, rho0), np.zeros(nc),
                                        np.full(nc, beta0), f0, p0, c0, 4, dt, V=pr.V, ctx=ctx, forms="python")
    mdl.init()
    mdl.monitor(nharm=nharm, skip=skip, every=1)
    mdl.rk4_steps(0.0, dt, nsteps)
    assert mdl.monitor_info()[0] == 2 * spp
    rows = monitor.power_law(np.full(nc, 1.0), 2.0, nharm)
    th = fa.BioheatSpectralExplicit(pr.mesh, degree, 0.52, 3.6e6, model=mdl)
    th.set_heat_from(mdl, rows)
    total = float(th.heat().x.array.sum())
    th.set_heat_from(mdl, rows[:1])
    first = float(th.heat().x.array.sum())
    th.close(), mdl.close(), ctx.close()
    X = pr.V.tabulate_dof_coordinates()[:, 0]
    sigma = (X + 0.0000001) / (c0**2 / w0 / beta0 / u0)
    ex_c, ex_s = [], []
    for k in range(1, nharm + 1):
        B = p0 * 2 / (k * sigma) * jv(k, k * sigma)
        ex_c.append(-B * np.sin(k * w0 * X / c0)), ex_s.append(B * np.cos(k * w0 * X / c0))
    rho, c = np.full(nc, rho0), np.full(nc, c0)
    want = float(harmonic_heat(pr, rows, rho, c, ex_c, ex_s).sum())
    want1 = float(harmonic_heat(pr, rows[:1], rho, c, ex_c[:1], ex_s[:1]).sum())
    err = abs(total - want) / want
    print(f"Fubini heat: total {total:.9e} against the series' {want:.9e}, relative error {err:.6e} (bound {bound:.6e}); "
          f"over the fundamental {total / first:.6f}, the series {want / want1:.6f}")
    assert want > 0 and err <= bound
    assert want / want1 > 1.1 and total / first >= want / want1 - bound


# ---- (5) the C++ example ------------------------------------------------------------------------------------------------
def test_cpp_example(orc, tmp_path):
    """examples/cpp_bioheat_harmonics.cpp, built as test_gpu_thermal.py::test_cpp_example builds its example, on case A
    with a Westervelt model from a live start: it prints a positive load, larger than the fundamental's alone, and that
    load is the Python object's."""
    cs = case(orc, "A")
    libdir = os.path.join(ROOT, "fenicsx-fus_amd", "fenicsxfus_amd")
    exe = tmp_path / "cpp_bioheat_harmonics"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "cpp_bioheat_harmonics.cpp"), "-L", libdir, "-lfusmi",
                           f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)])
    pr, m = cs.pr, cs.pr.mesh
    bone = materials(m, cs.hi)[0] == 0.32
    c, rho = np.where(bone, 2800.0, 1500.0), np.where(bone, 1850.0, 1000.0)
    w0 = 2 * np.pi * F0
    delta = np.where(bone, fa.compute_diffusivity_of_sound(w0, 2800.0, 400.0 / 20.0 * np.log(10.0)),
                     fa.compute_diffusivity_of_sound(w0, 1500.0, 0.2))
    beta = np.where(bone, 6.0, 3.5)
    alpha = np.where(bone, 20.0, 0.5)
    wdt = 0.5 * 0.003 / (2800.0 * cs.P ** 2)
    tags = fa.tag_box_boundary(m)
    u0, v0 = live_state(pr, 11, P0, F0)
    nwave, nheat = 18, 3
    with open(tmp_path / "in.bin", "wb") as f:
        np.array([pr.tdim, pr.P, m.num_cells, pr.ndofs, m.geometry.x.shape[0], len(tags.values), nwave, NHARM, nheat],
                 dtype=np.int64).tofile(f)
        np.array([F0, P0, S0, wdt, Y, cs.dt], dtype=np.float64).tofile(f)
        pr.dm.astype(np.int32).tofile(f)
        np.asarray(pr.nodes, dtype=np.float64).tofile(f)
        np.ascontiguousarray(m.geometry.x, dtype=np.float64).tofile(f)
        np.ascontiguousarray(m.geometry.dofmap, dtype=np.int32).tofile(f)
        for a in (tags.cells, tags.local_facets, tags.values):
            np.ascontiguousarray(a, dtype=np.int32).tofile(f)
        for a in (c, rho, delta, beta, cs.k, cs.rho_c, cs.w, alpha, u0, v0):
            np.ascontiguousarray(a, dtype=np.float64).tofile(f)
    out = subprocess.run([str(exe), str(tmp_path / "in.bin")], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    w = out.stdout.split()
    val = lambda key: float(w[w.index(key) + 1])   # noqa: E731
    assert val("load") > val("fundamental") > 0 and val("peak_rise") > 0
    ctx = fa.Context(0)
    mdl = fa.WesterveltSpectralExplicit(m, tags, cs.P, c, rho, delta, beta, F0, P0, S0, 4, wdt, V=pr.V, ctx=ctx)
    mdl.init()
    mdl.set_state(u0, v0)
    mdl.monitor(which="u", nharm=NHARM, every=1)
    mdl.rk4_steps(0.0, wdt, nwave)
    th = fa.BioheatSpectralExplicit(m, cs.P, cs.k, cs.rho_c, cs.w, model=mdl)
    th.set_heat_from(mdl, monitor.power_law(alpha, Y, NHARM))
    load = float(th.heat().x.array.sum())
    th.close(), mdl.close(), ctx.close()
    assert abs(val("load") - load) <= 1e-9 * load
