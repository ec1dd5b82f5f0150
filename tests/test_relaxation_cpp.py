"""examples/cpp_relaxation.cpp against include/fusmi.hpp: compiled and linked without a GPU, run on one against the
Strang-split stepper of tests/relaxation_ref.py (the 4 x 3 x 3 case of test_gpu_relaxation.py, R = 2, 20 steps)."""
import os
import subprocess

import numpy as np
import pytest

import relaxation_ref as rr
import source_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P0 = 6e4


def build_example(tmp_path):
    libdir = os.path.join(ROOT, "fenicsx-fus_amd", "fenicsxfus_amd")
    exe = tmp_path / "cpp_relaxation"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "cpp_relaxation.cpp"), "-L", libdir, "-lfusmi",
                           f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)])
    return exe


def test_cpp_example_compiles(tmp_path):
    assert os.path.exists(build_example(tmp_path))


@pytest.mark.gpu
def test_cpp_example_runs(orc, tmp_path):
    from test_gpu_relaxation import case, cell_strengths

    exe = build_example(tmp_path)
    cs = case(orc, "3d")
    pr, m = cs.pr, cs.pr.mesh
    freqs, a = cell_strengths(cs, 2)
    with open(tmp_path / "in.bin", "wb") as f:
        np.array([3, pr.P, m.num_cells, pr.ndofs, m.geometry.x.shape[0], len(cs.tags.cells), sr.NSTEPS, 2], dtype=np.int64).tofile(f)
        np.array([cs.dt, cs.f0, P0, sr.S0, *freqs], dtype=np.float64).tofile(f)
        pr.dm.astype(np.int32).tofile(f)
        np.asarray(pr.nodes, dtype=np.float64).tofile(f)
        np.ascontiguousarray(m.geometry.x, dtype=np.float64).tofile(f)
        np.ascontiguousarray(m.geometry.dofmap, dtype=np.int32).tofile(f)
        for x in (cs.tags.cells, cs.tags.local_facets, cs.tags.values):
            np.ascontiguousarray(x, dtype=np.int32).tofile(f)
        for x in (cs.c, cs.rho, a):
            np.ascontiguousarray(x, dtype=np.float64).tofile(f)
    out = subprocess.run([str(exe), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    raw = np.fromfile(tmp_path / "out.bin", dtype=np.float64).reshape(4, pr.ndofs)
    A = rr.lumped_strengths(pr, a, cs.c, cs.rho)
    ur, vr, zr = rr.stepper(cs, "linear", 0, A, 2 * np.pi * freqs, P0, 0.0, cs.dt, sr.NSTEPS)
    errs = [sr.rel(raw[0], ur), sr.rel(raw[1], vr), sr.rel(raw[2], zr[0]), sr.rel(raw[3], zr[1])]
    print("cpp_relaxation: rel err u, v, z0, z1 = " + ", ".join(f"{e:.3e}" for e in errs))
    assert all(e < 1e-10 for e in errs), errs
    assert abs(float(out.stdout.split()[-1]) - np.abs(raw[1]).max()) <= 1e-15 * np.abs(raw[1]).max()
