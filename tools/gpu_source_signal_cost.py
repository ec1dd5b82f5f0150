"""Cost of the sampled-signal source kernel beside the analytic one, and of dense source weights in the block kernel
(fusmi.h "sources anywhere in the mesh", "sampled drive signals"): one process, n^3 hexahedra, degree P, fp64.  Five
phases of `steps` RK4 steps each, in this order, nothing else launched in between:
    plain      default source, no weights
    blob       default source, weights on every DOF of one block's worth of neighbouring cells (a 4 x 4 x 4 cube of cells)
    analytic   per-DOF delays on the face x = 0 (k_source_entries)
    mirror     one channel per face DOF, equal delays: the time-reversal layout of the table (k_source_entries_signal)
    few        16 channels by position over the face, per-DOF delays: the element-group layout
Run it under `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/gpu_source_signal_cost.py`, then
`python tools/gpu_source_signal_cost.py --summarise DIR` splits the kernel trace by dispatch order into the phases and
prints the median duration per launch of the source kernels and of the block kernel.  Without the profiler the script
prints the library's own event timers per phase (profile level 1).

    python tools/gpu_source_signal_cost.py [n] [P] [steps]"""
import csv
import glob
import os
import sys

import numpy as np

PHASES = ("plain", "blob", "analytic", "mirror", "few")


def summarise(root, steps):
    paths = glob.glob(os.path.join(root, "**", "*kernel_trace.csv"), recursive=True)
    if not paths:
        sys.exit(f"no kernel trace under {root}")
    rows = []
    for p in paths:
        with open(p, newline="") as f:
            rows += list(csv.DictReader(f))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    dur = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3          # noqa: E731  (us)
    sig = [dur(r) for r in rows if "k_source_entries_signal" in r["Kernel_Name"]]
    ana = [dur(r) for r in rows if "k_source_entries" in r["Kernel_Name"] and "signal" not in r["Kernel_Name"]]
    blk = [dur(r) for r in rows if "k_block_op" in r["Kernel_Name"]][-len(PHASES) * 4 * steps:]
    per = 2 * steps + 1
    print(f"{len(ana)} analytic launches, {len(sig)} signal launches, expected {per} per phase")
    assert len(ana) == per and len(sig) == 2 * per and len(blk) == len(PHASES) * 4 * steps

    def line(name, v):
        v = np.asarray(v)
        print(f"{name:28s} median {np.median(v):8.2f} us   min {v.min():8.2f}   max {v.max():8.2f}   n {len(v)}")
    line("k_source_entries", ana)
    line("k_source_entries_signal mirror", sig[:per])
    line("k_source_entries_signal few", sig[per:])
    for i, ph in enumerate(PHASES):
        line(f"k_block_op, phase {ph}", blk[i * 4 * steps:(i + 1) * 4 * steps])


if "--summarise" in sys.argv:
    i = sys.argv.index("--summarise")
    summarise(sys.argv[i + 1], int(sys.argv[i + 2]) if len(sys.argv) > i + 2 else 20)
    sys.exit(0)

sys.path.insert(0, "fenicsx-fus_amd")
import fenicsxfus_amd as fa  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 64
P = int(sys.argv[2]) if len(sys.argv) > 2 else 4
steps = int(sys.argv[3]) if len(sys.argv) > 3 else 20
L = 0.12 * n / 64
mesh = fa.BoxMesh([0, 0, 0], [L, L, L], (n, n, n), perturb=0.1)
V = fa.FunctionSpace(mesh, P)
nc = mesh.num_cells
dt = 0.5 * (L / n) / (1500.0 * P**2)
ctx = fa.Context(0)
m = fa.LinearSpectralExplicit(mesh, fa.tag_box_boundary(mesh), P, np.full(nc, 1500.0), np.full(nc, 1000.0), 0.5e6, 6e4,
                              1500.0, 4, dt, V=V, ctx=ctx)
X = V.tabulate_dof_coordinates()
nd = V.num_dofs
tau = fa.source.focus_delays(X, [0.5 * L, 0.5 * L, 0.5 * L], 1500.0)
# the face x = 0 (perturbed vertices stay on the box's faces)
face = np.flatnonzero(np.abs(X[:, 0]) < 1e-9 * L)
# one block's worth of cells: the 4 x 4 x 4 cube of cells in the middle of the box
cen = mesh.cell_centroids()[:, :3]
h = L / n
cube = np.flatnonzero(np.all(np.abs(cen - 0.5 * L) < 2 * h, axis=1))
blob = np.zeros(nd)
dofs = np.unique(np.asarray(V.tensor_dofmap)[cube])
blob[dofs] = 1e-6 * np.exp(-((X[dofs] - 0.5 * L) ** 2).sum(axis=1) / (2 * h) ** 2)
rng = np.random.default_rng(0)
nsamp_m, nsamp_f = 64, 1024
chan_m = np.full(nd, -1, dtype=np.int32)
chan_m[face] = np.arange(len(face))
chan_f = np.full(nd, -1, dtype=np.int32)
chan_f[face] = (np.floor(4 * X[face, 1] / L).clip(0, 3) * 4 + np.floor(4 * X[face, 2] / L).clip(0, 3)).astype(np.int32)
sig_m, sig_f = rng.standard_normal((len(face), nsamp_m)), rng.standard_normal((16, nsamp_f))
print(f"{n}^3 P={P} fp64: {nd} dofs, {len(face)} face dofs, blob {len(cube)} cells / {len(dofs)} dofs, "
      f"blocks {m.data.info()['nblocks']}, geometry {m.data.geometry_mode()}", flush=True)


def setup(phase):
    m.set_source_weights(blob if phase == "blob" else None)
    if phase == "analytic":
        m.set_source(delay=tau)
    elif phase == "mirror":
        m.set_source_signals(sig_m, steps * dt / (nsamp_m - 8), 0.0, chan_m)
    elif phase == "few":
        m.set_source_signals(sig_f, steps * dt / (nsamp_f - 8), 0.0, chan_f, delay=tau)


ctx.profile_enable(True)
for phase in PHASES:
    setup(phase)
    m.init()
    ctx.profile_enable(True)
    m.rk4_steps(0.0, dt, steps)
    out = []
    for name in ("source", "source_signal", "stiffness"):
        ms, cnt = ctx.profile_get(name)
        if cnt:
            out.append(f"{name} {cnt / steps:.2f} launches per step, {ms / cnt * 1e3:.2f} us each")
    print(f"phase {phase}: " + "; ".join(out), flush=True)
ctx.profile_enable(False)
m.close()
ctx.close()
