"""Rate of the field-monitor kernel (fusmi.h "field monitor") beside the device's streaming bandwidth, one process:
64^3 hexahedra, degree 4, fp64, nharm = 4.  The kernel is timed by the library's own HIP-event timers (profile scope
"monitor"); its bytes are one read of the state plus a read and a write of every accumulator plane,
n_internal * (sizeof(T) + 2 * (2 sizeof(T) + (2 + 2 nharm) * 8)).  Prints both numbers and their ratio.

    python tools/gpu_monitor_rate.py [n] [P] [nharm] [f64|f32]"""
import sys

import numpy as np

sys.path.insert(0, "fenicsx-fus_amd")
import fenicsxfus_amd as fa  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 64
P = int(sys.argv[2]) if len(sys.argv) > 2 else 4
nharm = int(sys.argv[3]) if len(sys.argv) > 3 else 4
dtype = np.float32 if len(sys.argv) > 4 and sys.argv[4] == "f32" else np.float64
L = 0.12 * n / 64
mesh = fa.BoxMesh([0, 0, 0], [L, L, L], (n, n, n), dtype=dtype)
V = fa.FunctionSpace(mesh, P)
nc = mesh.num_cells
dt = 0.5 * (L / n) / (1500.0 * P**2)
ctx = fa.Context(0)
m = fa.LinearSpectralExplicit(mesh, fa.tag_box_boundary(mesh), P, np.full(nc, 1500.0, dtype), np.full(nc, 1000.0, dtype),
                              0.5e6, 6e4, 1500.0, 4, dt, V=V, ctx=ctx)
m.init()
m.monitor(nharm=nharm, every=1)
m.rk4_steps(0.0, dt, 5)
ctx.profile_enable(True)
steps = 30
m.rk4_steps(5 * dt, dt, steps)
ms, cnt = ctx.profile_get("monitor")
ctx.profile_enable(False)
assert cnt == steps and m.monitor_info()[0] == 5 + steps
ts = np.dtype(dtype).itemsize
nint = m.data.info()["internal_len"]
per_dof = ts + 2 * (2 * ts + (2 + 2 * nharm) * 8)
rate = nint * per_dof / (ms / cnt * 1e-3) / 1e9
triads = [ctx.measure_bandwidth(1 << 30, 10) for _ in range(3)]
triad = float(np.median(triads))
print(f"monitor kernel: {n}^3 P={P} {np.dtype(dtype).name} nharm={nharm}: {V.num_dofs} dofs, internal length {nint}, "
      f"{per_dof} B/DOF/sample, accumulators {nint * (2 * ts + (2 + 2 * nharm) * 8) / 2**20:.0f} MiB")
print(f"monitor kernel: {ms / cnt:.4f} ms/sample over {cnt} samples -> {rate:.0f} GB/s")
print(f"streaming bandwidth (fus_measure_bandwidth, 1 GiB, best of 10; three runs {[round(x) for x in triads]}): {triad:.0f} GB/s")
print(f"ratio monitor / streaming: {rate / triad:.3f}")
m.close()
ctx.close()
