"""examples/cpp_sponge.cpp against include/fusmi.hpp: compiled and linked without a GPU, run on one against the
Strang-split stepper of tests/sponge_ref.py (the 4 x 3 x 3 case of test_gpu_sponge.py, 20 steps)."""
import os
import subprocess

import numpy as np
import pytest

import source_ref as sr
import sponge_ref as spr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P0 = 6e4


def build_example(tmp_path):
    libdir = os.path.join(ROOT, "fenicsx-fus_amd", "fenicsxfus_amd")
    exe = tmp_path / "cpp_sponge"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "cpp_sponge.cpp"), "-L", libdir, "-lfusmi",
                           f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)])
    return exe


def test_cpp_example_compiles(tmp_path):
    assert os.path.exists(build_example(tmp_path))


@pytest.mark.gpu
def test_cpp_example_runs(orc, tmp_path):
    from test_gpu_sponge import case, case_sigma

    exe = build_example(tmp_path)
    cs = case(orc, "3d")
    pr, m = cs.pr, cs.pr.mesh
    sigma = case_sigma(cs)
    with open(tmp_path / "in.bin", "wb") as f:
        np.array([3, pr.P, m.num_cells, pr.ndofs, m.geometry.x.shape[0], len(cs.tags.cells), sr.NSTEPS], dtype=np.int64).tofile(f)
        np.array([cs.dt, cs.f0, P0, sr.S0], dtype=np.float64).tofile(f)
        pr.dm.astype(np.int32).tofile(f)
        np.asarray(pr.nodes, dtype=np.float64).tofile(f)
        np.ascontiguousarray(m.geometry.x, dtype=np.float64).tofile(f)
        np.ascontiguousarray(m.geometry.dofmap, dtype=np.int32).tofile(f)
        for x in (cs.tags.cells, cs.tags.local_facets, cs.tags.values):
            np.ascontiguousarray(x, dtype=np.int32).tofile(f)
        for x in (cs.c, cs.rho, sigma):
            np.ascontiguousarray(x, dtype=np.float64).tofile(f)
    out = subprocess.run([str(exe), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    raw = np.fromfile(tmp_path / "out.bin", dtype=np.float64).reshape(4, pr.ndofs)
    ur, vr, _ = spr.stepper(cs, "linear", 0, sigma, None, [], P0, 0.0, cs.dt, sr.NSTEPS)
    errs = [sr.rel(raw[0], ur), sr.rel(raw[1], vr)]
    print("cpp_sponge: rel err u, v = " + ", ".join(f"{e:.3e}" for e in errs))
    assert all(e < 1e-10 for e in errs), errs
    assert abs(float(out.stdout.split()[-1]) - np.abs(raw[1]).max()) <= 1e-15 * np.abs(raw[1]).max()
    # clear_sponge and set_sponge keep the state; sponge_apply(dt) then scales it by exp(-sigma dt)
    u2, v2, _ = spr.substep(raw[0], raw[1], None, sigma, cs.dt)
    assert sr.rel(raw[2], u2) < 1e-14 and sr.rel(raw[3], v2) < 1e-14 and not np.array_equal(raw[2], raw[0])
