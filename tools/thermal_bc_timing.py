"""Cost of the bioheat model's boundary conditions (fusmi.h "bioheat", fus_thermal_set_boundary): 64^3 hexahedra,
degree 4, fp64, tissue properties, 50 RK4 steps, timed by the library's own HIP-event timers (profile scopes "thermal",
"stiffness", "shared", "thermal_bc") and, in a pass of its own without them, by the host clock.

    python tools/thermal_bc_timing.py [--n 64] [--P 4] [--steps 50] [--repeats 3] [--mode none|bc] [--limit 300]

--mode none: no boundary is ever set (this also runs on a library from before the boundary conditions, named by
FUSMI_LIB, for the comparison with the parent commit).  --mode bc: the face x = lo fixed at body temperature, the five
other faces convective with h_c = 500 W/m^2/K and water at 20 degrees C.  The parent starts one worker process under a
time limit; the worker warms up with 10 steps, then runs `repeats` rounds of `steps` steps under the event timers and
`repeats` rounds without them.  Prints one JSON line with the per-round times per step and their medians."""
import argparse
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "fenicsx-fus_amd"))
SCOPES = ("thermal", "stiffness", "shared", "thermal_bc")


def worker(args):
    import numpy as np

    import fenicsxfus_amd as fa

    n, P = args.n, args.P
    L = 0.003 * n                     # 3 mm cells
    mesh = fa.BoxMesh([0, 0, 0], [L, L, L], (n, n, n))
    V = fa.FunctionSpace(mesh, P)
    ctx = fa.Context(0)
    th = fa.BioheatSpectralExplicit(mesh, P, 0.52, 1040.0 * 3600.0, 4e4, V=V, ctx=ctx)
    X = V.tabulate_dof_coordinates()
    th.set_heat(5e7 * np.exp(-((X - 0.5 * L) ** 2).sum(axis=1) / (2 * (0.1 * L) ** 2)))
    info = (0, 0)
    if args.mode == "bc":
        cells, lf, ax, sd = mesh.exterior_facets()
        lo_x = (ax == 0) & (sd == 0)
        tags = fa.FacetTags(cells, lf, np.where(lo_x, 1, 2))
        th.set_boundary(tags, fixed={1: 37.0}, convective={2: (500.0, 20.0)})
        info = th.boundary_info()
    th.init()
    dt = th.stable_dt()
    th.steps(dt, 10)
    rounds = []
    for _ in range(args.repeats):
        ctx.profile_enable(True)
        th.steps(dt, args.steps)
        got = {name: ctx.profile_get(name) for name in SCOPES}
        ctx.profile_enable(False)
        rounds.append({name: {"ms_per_step": ms / args.steps, "launches": cnt} for name, (ms, cnt) in got.items()})
    wall = []
    for _ in range(args.repeats):
        ctx.synchronize()
        t0 = time.perf_counter()
        th.steps(dt, args.steps)
        ctx.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3 / args.steps)
    kernel = [sum(r[name]["ms_per_step"] for name in SCOPES) for r in rounds]
    out = {"mode": args.mode, "n": n, "P": P, "steps": args.steps, "ndofs": int(V.num_dofs), "nfixed": info[0],
           "nconvective": info[1], "dt": dt, "lib": os.environ.get("FUSMI_LIB", "in-tree"),
           "kernel_ms_per_step": kernel, "kernel_ms_per_step_median": float(np.median(kernel)),
           "wall_ms_per_step": wall, "wall_ms_per_step_median": float(np.median(wall)), "rounds": rounds,
           "peak_rise": float(th.rise().x.array.max())}
    bc = [r["thermal_bc"] for r in rounds if r["thermal_bc"]["launches"]]
    if bc:
        per_launch = [r["ms_per_step"] * args.steps / r["launches"] * 1e3 for r in bc]
        out["thermal_bc_us_per_launch"] = per_launch
        out["thermal_bc_share_of_kernel_time"] = [r["thermal_bc"]["ms_per_step"] / k for r, k in zip(rounds, kernel)]
    th.close()
    ctx.close()
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--P", type=int, default=4)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--mode", choices=("none", "bc"), default="none")
    ap.add_argument("--limit", type=int, default=300)
    ap.add_argument("--worker", action="store_true")
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--n", str(args.n), "--P", str(args.P), "--steps",
           str(args.steps), "--repeats", str(args.repeats), "--mode", args.mode]
    r = subprocess.run(cmd, timeout=args.limit)
    sys.exit(r.returncode)


if __name__ == "__main__":
    main()
