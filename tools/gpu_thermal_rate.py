"""Rate of the bioheat stage kernel (fusmi.h "bioheat") beside the device's streaming bandwidth, one process: 64^3
hexahedra, degree 4, fp64, 50 RK4 steps.  The kernels are timed by the library's own HIP-event timers (profile scopes
"thermal", "stiffness", "shared").  Counted bytes of k_thermal_stage per DOF and step, T = scalar type: stage 0 reads 5
vectors and writes 2, the two middle stages read 7 and write 2, the last reads 6 and writes 1 and reads and writes the
double dose plane: 32 sizeof(T) + 16.  Prints the stage kernel's GB/s, the measured copy bandwidth, their ratio, and the
share of a thermal step spent in the operator.

    python tools/gpu_thermal_rate.py [n] [P] [f64|f32]"""
import sys

import numpy as np

sys.path.insert(0, "fenicsx-fus_amd")
import fenicsxfus_amd as fa  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 64
P = int(sys.argv[2]) if len(sys.argv) > 2 else 4
dtype = np.float32 if len(sys.argv) > 3 and sys.argv[3] == "f32" else np.float64
L = 0.12 * n / 64
mesh = fa.BoxMesh([0, 0, 0], [L, L, L], (n, n, n), dtype=dtype)
V = fa.FunctionSpace(mesh, P)
nc = mesh.num_cells
ctx = fa.Context(0)
th = fa.BioheatSpectralExplicit(mesh, P, 0.52, 1040.0 * 3600.0, 4e4, V=V, ctx=ctx)
th.init()
X = V.tabulate_dof_coordinates()
th.set_heat((5e7 * np.exp(-((X - 0.5 * L) ** 2).sum(axis=1) / (2 * (0.1 * L) ** 2))).astype(dtype))
dt = 1.0 / th.lambda_max(5)          # well inside the stable range; the rate does not depend on it
th.steps(dt, 5)
ctx.profile_enable(True)
steps = 50
th.steps(dt, steps)
ms_t, cnt_t = ctx.profile_get("thermal")
ms_k, cnt_k = ctx.profile_get("stiffness")
ms_s, cnt_s = ctx.profile_get("shared")
ctx.profile_enable(False)
assert cnt_t == 4 * steps and cnt_k == 4 * steps
ts = np.dtype(dtype).itemsize
nint = th.data.info()["internal_len"]
per_dof = 32 * ts + 16
rate = nint * per_dof / (ms_t / steps * 1e-3) / 1e9
triads = [ctx.measure_bandwidth(1 << 30, 10) for _ in range(3)]
triad = float(np.median(triads))
step_ms = (ms_t + ms_k + ms_s) / steps
print(f"thermal stage kernel: {n}^3 P={P} {np.dtype(dtype).name}: {V.num_dofs} dofs, internal length {nint}, "
      f"{per_dof} B/DOF/step over four launches")
print(f"thermal stage kernel: {ms_t / cnt_t:.4f} ms/launch, {ms_t / steps:.4f} ms/step -> {rate:.0f} GB/s")
print(f"streaming bandwidth (fus_measure_bandwidth, 1 GiB, best of 10; three runs {[round(x) for x in triads]}): {triad:.0f} GB/s")
print(f"ratio stage kernel / streaming: {rate / triad:.3f}")
print(f"thermal step (kernel time): {step_ms:.4f} ms = operator {ms_k / steps:.4f} + shared {ms_s / steps:.4f} + stage "
      f"{ms_t / steps:.4f}; operator share {(ms_k + ms_s) / (ms_t + ms_k + ms_s):.3f}")
print(f"peak rise after {5 + steps} steps of {dt:.3e} s: {th.rise().x.array.max():.4f} K")
th.close()
ctx.close()
