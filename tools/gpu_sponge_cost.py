"""Cost of the sponge sub-step (fusmi.h "absorbing layers"), one process: 64^3 hexahedra, degree 4, fp64, quadratic
layers of `cells` cells on the five tag-2 faces.  Alternates runs without and with the layers and prints the step time of
each (wall clock around synchronised runs of `steps` steps, profile off); then, with the library's event timers (profile
level 1), the time of one "sponge" launch and its rate on the bytes it is counted to move, 5 * 8 per DOF of the listed
tiles, once with the layers' own tile list and once with every tile listed (sigma made tiny but nonzero outside the
layers), and the device's streaming-copy rate (fus_measure_bandwidth) beside them.

    python tools/gpu_sponge_cost.py [n] [P] [steps] [repeats] [cells]"""
import sys
import time

import numpy as np

sys.path.insert(0, "fenicsx-fus_amd")
import fenicsxfus_amd as fa  # noqa: E402
from fenicsxfus_amd import sponge  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 64
P = int(sys.argv[2]) if len(sys.argv) > 2 else 4
steps = int(sys.argv[3]) if len(sys.argv) > 3 else 40
repeats = int(sys.argv[4]) if len(sys.argv) > 4 else 5
cells = int(sys.argv[5]) if len(sys.argv) > 5 else 8
L = 0.12 * n / 64
mesh = fa.BoxMesh([0, 0, 0], [L, L, L], (n, n, n), perturb=0.1)
V = fa.FunctionSpace(mesh, P)
nc = mesh.num_cells
dt = 0.5 * (L / n) / (1500.0 * P**2)
ctx = fa.Context(0)
m = fa.LinearSpectralExplicit(mesh, fa.tag_box_boundary(mesh), P, np.full(nc, 1500.0), np.full(nc, 1000.0), 0.5e6, 6e4,
                              1500.0, 4, dt, V=V, ctx=ctx)
sigma = sponge.layer_sigma(V.tabulate_dof_coordinates(), [0, 0, 0], [L, L, L],
                           {f: cells * L / n for f in sponge.FACES[1:]}, 1500.0)
m.init()
m.rk4_steps(0.0, dt, 5)                      # warm-up


def timed():
    ctx.synchronize()
    t0 = time.perf_counter()
    m.rk4_steps(0.0, dt, steps)              # synchronises
    return (time.perf_counter() - t0) / steps * 1e3


res = {"off": [], "on": []}
for _ in range(repeats):
    m.clear_sponge()
    m.rk4_steps(0.0, dt, 2)
    res["off"].append(timed())
    m.set_sponge(sigma)
    m.rk4_steps(0.0, dt, 2)
    res["on"].append(timed())
for k, v in res.items():
    print(f"step time, sponge {k}: median {np.median(v):.4f} ms, min {min(v):.4f}, max {max(v):.4f} over {repeats} runs of {steps} steps")
info = m.data.info()
n_internal = int(info["internal_len"])
bw = ctx.measure_bandwidth()
for label, s in (("layers", sigma), ("every tile", np.maximum(sigma, 1e-300))):
    m.set_sponge(s)
    n_active, nt_active, nt_total = m.sponge_info()
    ctx.profile_enable(True)
    m.rk4_steps(0.0, dt, steps)
    ms, cnt = ctx.profile_get("sponge")
    for name in ("sponge", "stiffness", "stage", "boundary"):
        t, c = ctx.profile_get(name)
        print(f"[{label}] profile {name}: {c / steps:.2f} launches per step, {t / max(c, 1) * 1e3:.2f} us each, {t / steps:.4f} ms per step")
    ctx.profile_enable(False)
    ndof = min(nt_active * 512, n_internal)
    nbytes = 5 * 8 * ndof
    print(f"[{label}] sponge kernel: {n_active} DOFs with sigma > 0, {nt_active} of {nt_total} tiles, {nbytes / 1e6:.1f} MB counted per "
          f"launch, {ms / cnt * 1e3:.2f} us, {nbytes / (ms / cnt * 1e-3) / 1e9:.0f} GB/s; streaming copy {bw:.0f} GB/s")
print(f"{n}^3 P={P} fp64: {V.num_dofs} dofs, {n_internal} internal slots, blocks {info['nblocks']}, geometry {m.data.geometry_mode()}, "
      f"layers of {cells} cells")
m.close()
ctx.close()
