"""Cost of the gradient / pair-product kernel (fusmi.h "gradient", "intensity"), one process: n^3 hexahedra (default 64),
degree 4, fp64, the benchmark's trilinear mesh.  Prints the median wall time of the synchronous calls

    fus_op_gradient (device space, nodal)      fus_model_intensity, nharm = 1 and nharm = 4 (device space)

and, from the library's event timers (profile level 1) in the same process, the device time of their "gradient" scope
(block kernel and shared-DOF reductions, without the numbering passes around them) and of one operator-only
fus_stiffness_apply on the same operator; then fus_measure_bandwidth, the bytes the design moves per DOF from the
operator's own layout counts, and the fraction of the streaming rate that implies.

    python tools/gradient_profile.py [n] [repeats]

Run without --child it starts itself as a child process under `timeout` and returns the child's status: a step that
hangs ends there, nothing is started after a failure."""
import ctypes as C
import subprocess
import sys
import time

import numpy as np

LIMIT_S = 420

if "--child" not in sys.argv:
    args = [a for a in sys.argv[1:]]
    sys.exit(subprocess.run(["timeout", "-k", "10", str(LIMIT_S), sys.executable, sys.argv[0], "--child", *args]).returncode)

sys.path.insert(0, "fenicsx-fus_amd")
import fenicsxfus_amd as fa  # noqa: E402
from fenicsxfus_amd import _abi  # noqa: E402

argv = [a for a in sys.argv[1:] if a != "--child"]
n = int(argv[0]) if len(argv) > 0 else 64
repeats = int(argv[1]) if len(argv) > 1 else 20
P, WARM = 4, 3
L = 0.12 * n / 64
mesh = fa.BoxMesh([0, 0, 0], [L, L, L], (n, n, n), perturb=0.1)
V = fa.FunctionSpace(mesh, P)
nc, nd = mesh.num_cells, V.num_dofs
dt = 0.5 * (L / n) / (1500.0 * P**2)
ctx = fa.Context(0)
m = fa.LinearSpectralExplicit(mesh, fa.tag_box_boundary(mesh), P, np.full(nc, 1500.0), np.full(nc, 1000.0), 0.5e6, 6e4,
                              1500.0, 4, dt, V=V, ctx=ctx)
data, lib = m.data, _abi.lib()
hip = C.CDLL("libamdhip64.so")


def dev(nbytes, src=None):
    p = C.c_void_p()
    assert hip.hipMalloc(C.byref(p), C.c_size_t(nbytes)) == 0, "hipMalloc"
    if src is not None:
        assert hip.hipMemcpy(p, src.ctypes.data_as(C.c_void_p), C.c_size_t(nbytes), C.c_int(1)) == 0, "hipMemcpy"
    return p


rng = np.random.default_rng(0)
x = rng.standard_normal(nd)
d_x, d_out = dev(8 * nd, x), dev(8 * 3 * nd)
m.init()
m.set_state(6e4 * x, 2 * np.pi * 0.5e6 * 6e4 * rng.standard_normal(nd))
m.monitor(which="u", nharm=4, every=1)
m.rk4_steps(0.0, dt, 3)
DEVICE = C.c_int(_abi.FUS_DEVICE)
calls = {
    "fus_op_gradient (nodal)": lambda: lib.fus_op_gradient(data.h, d_x, None, d_out, C.c_int(_abi.FUS_GRAD_NODAL), DEVICE),
    "fus_model_intensity nharm=1": lambda: lib.fus_model_intensity(m.h, C.c_int(1), None, d_out, DEVICE),
    "fus_model_intensity nharm=4": lambda: lib.fus_model_intensity(m.h, C.c_int(4), None, d_out, DEVICE),
}
wall, devt = {}, {}
for name, fn in calls.items():
    for _ in range(WARM):
        _abi.check(fn())
    ts = []
    for _ in range(repeats):
        ctx.synchronize()
        t0 = time.perf_counter()
        _abi.check(fn())                       # synchronises the stream before it returns
        ts.append((time.perf_counter() - t0) * 1e3)
    wall[name] = ts
    ctx.profile_enable(True)
    for _ in range(repeats):
        _abi.check(fn())
    t, c = ctx.profile_get("gradient")
    devt[name] = t / max(c, 1)
    ctx.profile_enable(False)
    print(f"{name}: wall median {np.median(ts):.3f} ms (min {min(ts):.3f}, max {max(ts):.3f}, {repeats} calls after {WARM}); "
          f"device, kernel + shared reductions: {devt[name]:.3f} ms", flush=True)

coef, y = np.ones(nc), np.zeros(nd)
data.stiffness(x, coef, y)                         # warm-up
ctx.profile_enable(True)
for _ in range(5):
    data.stiffness(x, coef, y)
t, c = ctx.profile_get("stiffness")
t_sh, c_sh = ctx.profile_get("shared")
ctx.profile_enable(False)
stiff = t / max(c, 1) + t_sh / max(c_sh, 1)
print(f"operator-only fus_stiffness_apply: block kernel {t / max(c, 1):.3f} ms + shared reduction {t_sh / max(c_sh, 1):.3f} ms "
      f"= {stiff:.3f} ms ({c} launches)")
bw = ctx.measure_bandwidth()
info = data.info()
n_int, pairs, shared = int(info["interior_dofs"]), int(info["pairs"]), int(info["shared_dofs"])
Nd = (P + 1) ** 3
for name, K in (("fus_op_gradient (nodal)", 0), ("fus_model_intensity nharm=1", 1), ("fus_model_intensity nharm=4", 4)):
    nin = 2 * K if K else 1
    kern = (8 * nin + 8 * 3) * (n_int + pairs) + 2 * nc * Nd * max(K, 1) + 8 * pairs      # gathers, sums out, local dofmaps, shared indices
    red = (8 * 3 + 8 * 3) * pairs + 8 * 3 * shared                                         # partial sums in (index + value), totals out
    outp = (8 * 3 + 8 + 4 + 8 * 3) * nd                                                    # sums, denominator, permutation in; result out
    floor = (8 * nin + 8 * 3) * nd
    print(f"{name}: bytes per DOF -- floor {floor / nd:.0f}, design {(kern + red) / nd:.1f} in the gradient scope + {outp / nd:.0f} in the "
          f"numbering pass; scope at {(kern + red) / (devt[name] * 1e-3) / 1e9:.0f} GB/s = {(kern + red) / (devt[name] * 1e-3) / 1e9 / bw:.2f} "
          f"of the streaming copy ({bw:.0f} GB/s); scope / stiffness action = {devt[name] / stiff:.2f}, call / stiffness action = "
          f"{np.median(wall[name]) / stiff:.2f}")
print(f"{n}^3 P={P} fp64: {nd} dofs, {info['internal_len']} internal slots, {info['nblocks']} blocks, {shared} shared dofs in {pairs} "
      f"(block, dof) pairs, geometry {data.geometry_mode()}")
m.close()
ctx.close()
