"""Cost of the per-entry source kernel (fusmi.h "phased and apodised sources"), one process: 64^3 hexahedra, degree 4,
fp64, the face x = 0 focused with source.focus_delays.  Prints the "source" and "stiffness" kernel times and counts per
step (library event timers, profile level 1) and the step time (profile off, wall clock around synchronised runs of
`steps` steps) with the default source and with the delayed one, alternated.

    python tools/gpu_source_cost.py [n] [P] [steps] [repeats]"""
import sys
import time

import numpy as np

sys.path.insert(0, "fenicsx-fus_amd")
import fenicsxfus_amd as fa  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 64
P = int(sys.argv[2]) if len(sys.argv) > 2 else 4
steps = int(sys.argv[3]) if len(sys.argv) > 3 else 40
repeats = int(sys.argv[4]) if len(sys.argv) > 4 else 5
L = 0.12 * n / 64
mesh = fa.BoxMesh([0, 0, 0], [L, L, L], (n, n, n), perturb=0.1)
V = fa.FunctionSpace(mesh, P)
nc = mesh.num_cells
dt = 0.5 * (L / n) / (1500.0 * P**2)
ctx = fa.Context(0)
m = fa.LinearSpectralExplicit(mesh, fa.tag_box_boundary(mesh), P, np.full(nc, 1500.0), np.full(nc, 1000.0), 0.5e6, 6e4,
                              1500.0, 4, dt, V=V, ctx=ctx)
tau = fa.source.focus_delays(V.tabulate_dof_coordinates(), [0.5 * L, 0.5 * L, 0.5 * L], 1500.0)
m.init()
m.rk4_steps(0.0, dt, 5)                      # warm-up


def timed():
    ctx.synchronize()
    t0 = time.perf_counter()
    m.rk4_steps(0.0, dt, steps)              # synchronises
    return (time.perf_counter() - t0) / steps * 1e3


res = {"default": [], "delayed": []}
for _ in range(repeats):
    m.clear_source()
    m.rk4_steps(0.0, dt, 2)
    res["default"].append(timed())
    m.set_source(delay=tau)
    m.rk4_steps(0.0, dt, 2)
    res["delayed"].append(timed())
for k, v in res.items():
    print(f"step time, {k} source: median {np.median(v):.4f} ms, min {min(v):.4f}, max {max(v):.4f} over {repeats} runs of {steps} steps")
ctx.profile_enable(True)
m.rk4_steps(0.0, dt, steps)
for name in ("source", "stiffness", "stage", "boundary"):
    ms, cnt = ctx.profile_get(name)
    print(f"profile {name}: {cnt / steps:.2f} launches per step, {ms / max(cnt, 1) * 1e3:.2f} us each, {ms / steps:.4f} ms per step")
ctx.profile_enable(False)
print(f"{n}^3 P={P} fp64: {V.num_dofs} dofs, blocks {m.data.info()['nblocks']}, geometry {m.data.geometry_mode()}")
m.close()
ctx.close()
