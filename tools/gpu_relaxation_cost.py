"""Cost of the relaxation sub-step (fusmi.h "relaxation absorption"), one process: 64^3 hexahedra, degree 4, fp64.
Alternates runs without relaxation and with R processes and prints the step time of each (wall clock around synchronised
runs of `steps` steps, profile off); then, with the library's event timers (profile level 1), the time of one "relax"
launch, its rate on the bytes it is counted to move, (3 R + 2) * 8 per DOF of the internal vector, and the device's
streaming-copy rate (fus_measure_bandwidth) beside it.

    python tools/gpu_relaxation_cost.py [n] [P] [steps] [repeats] [R]"""
import sys
import time

import numpy as np

sys.path.insert(0, "fenicsx-fus_amd")
import fenicsxfus_amd as fa  # noqa: E402
from fenicsxfus_amd import absorption  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 64
P = int(sys.argv[2]) if len(sys.argv) > 2 else 4
steps = int(sys.argv[3]) if len(sys.argv) > 3 else 40
repeats = int(sys.argv[4]) if len(sys.argv) > 4 else 5
R = int(sys.argv[5]) if len(sys.argv) > 5 else 2
L = 0.12 * n / 64
mesh = fa.BoxMesh([0, 0, 0], [L, L, L], (n, n, n), perturb=0.1)
V = fa.FunctionSpace(mesh, P)
nc = mesh.num_cells
dt = 0.5 * (L / n) / (1500.0 * P**2)
ctx = fa.Context(0)
m = fa.LinearSpectralExplicit(mesh, fa.tag_box_boundary(mesh), P, np.full(nc, 1500.0), np.full(nc, 1000.0), 0.5e6, 6e4,
                              1500.0, 4, dt, V=V, ctx=ctx)
freqs, strengths, fit_err = absorption.fit_power_law(5.0, 1.1, 0.25e6, 4e6, 1500.0, R)
m.init()
m.rk4_steps(0.0, dt, 5)                      # warm-up


def timed():
    ctx.synchronize()
    t0 = time.perf_counter()
    m.rk4_steps(0.0, dt, steps)              # synchronises
    return (time.perf_counter() - t0) / steps * 1e3


res = {"off": [], f"R={R}": []}
for _ in range(repeats):
    m.clear_relaxation()
    m.rk4_steps(0.0, dt, 2)
    res["off"].append(timed())
    m.set_relaxation(freqs, strengths)
    m.rk4_steps(0.0, dt, 2)
    res[f"R={R}"].append(timed())
for k, v in res.items():
    print(f"step time, relaxation {k}: median {np.median(v):.4f} ms, min {min(v):.4f}, max {max(v):.4f} over {repeats} runs of {steps} steps")
info = m.data.info()
n_internal = int(info["internal_len"])
ctx.profile_enable(True)
m.rk4_steps(0.0, dt, steps)
for name in ("relax", "stiffness", "stage", "boundary"):
    ms, cnt = ctx.profile_get(name)
    print(f"profile {name}: {cnt / steps:.2f} launches per step, {ms / max(cnt, 1) * 1e3:.2f} us each, {ms / steps:.4f} ms per step")
ms, cnt = ctx.profile_get("relax")
ctx.profile_enable(False)
nbytes = (3 * R + 2) * 8 * n_internal
print(f"relax kernel: {nbytes / 1e6:.1f} MB counted per launch ({n_internal} slots), {nbytes / (ms / cnt * 1e-3) / 1e9:.0f} GB/s; "
      f"streaming copy {ctx.measure_bandwidth():.0f} GB/s")
print(f"{n}^3 P={P} fp64: {V.num_dofs} dofs, blocks {info['nblocks']}, geometry {m.data.geometry_mode()}, fit error {fit_err:.3f}")
m.close()
ctx.close()
