"""Cost of the bioheat model's interface exchange (fusmi.h "bioheat", several ranks): two x-slabs of 32 x 64 x 64
hexahedra each (a 64^3 box), degree 4, fp64, tissue properties, in an in-process group on one device, 50 RK4 steps timed by
the library's own HIP-event timers: per launch the interface kernel ("thermal_if"), the streaming stage kernel over the
rank-local range ("thermal"), the pack of the interface totals ("halo"), and the operator's two ("stiffness", "shared").

    python tools/thermal_multirank_timing.py [--n 64] [--P 4] [--steps 50] [--repeats 3] [--limit 300]

The wall time of a group step is NOT a scaling number: the in-process exchange synchronises the host between the halves
of every stage, and both slabs share one device.  Only the per-launch kernel times say what the split costs.  The
single-rank step is timed by tools/thermal_bc_timing.py --mode none (also on the parent commit's library, FUSMI_LIB).
The parent starts one worker process under a time limit; prints one JSON line."""
import argparse
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "fenicsx-fus_amd"))
SCOPES = ("thermal_if", "thermal", "halo", "stiffness", "shared")


def worker(args):
    import numpy as np

    import fenicsxfus_amd as fa

    n, P = args.n, args.P
    L = 0.003 * n                     # 3 mm cells
    ctxs = [fa.Context(0) for _ in range(2)]
    fa.Context.init_local_group(ctxs)
    bios, spaces = [], []
    for r, ctx in enumerate(ctxs):
        mesh = fa.BoxMesh([0, 0, 0], [L, L, L], (n, n, n), rank=r, size=2)
        V = fa.FunctionSpace(mesh, P)
        th = fa.BioheatSpectralExplicit(mesh, P, 0.52, 1040.0 * 3600.0, 4e4, V=V, ctx=ctx)
        X = V.tabulate_dof_coordinates()
        th.set_heat(5e7 * np.exp(-((X - 0.5 * L) ** 2).sum(axis=1) / (2 * (0.1 * L) ** 2)))
        bios.append(th), spaces.append(V)
    fa.group_thermal_finish(bios)
    for th in bios:
        th.init()
    dt = fa.group_thermal_stable_dt(bios)
    fa.group_thermal_steps(bios, dt, 10)
    rounds = []
    for _ in range(args.repeats):
        for ctx in ctxs:
            ctx.profile_enable(True)
        fa.group_thermal_steps(bios, dt, args.steps)
        per_rank = []
        for ctx in ctxs:
            got = {name: ctx.profile_get(name) for name in SCOPES}
            ctx.profile_enable(False)
            per_rank.append({name: {"us_per_launch": 1e3 * ms / max(cnt, 1), "launches": cnt} for name, (ms, cnt) in got.items()})
        rounds.append(per_rank)
    plane = len(spaces[0].neighbours[0][1])
    out = {"n": n, "P": P, "steps": args.steps, "ndofs_per_rank": [int(V.num_dofs) for V in spaces], "interface_dofs": plane,
           "dt": dt, "rounds": rounds,
           "median_us_per_launch": {name: float(np.median([rk[name]["us_per_launch"] for rd in rounds for rk in rd]))
                                    for name in SCOPES},
           "peak_rise": float(max(th.rise().x.array.max() for th in bios))}
    for th in bios:
        th.close()
    for ctx in ctxs:
        ctx.close()
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--P", type=int, default=4)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--limit", type=int, default=300)
    ap.add_argument("--worker", action="store_true")
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--n", str(args.n), "--P", str(args.P), "--steps",
           str(args.steps), "--repeats", str(args.repeats)]
    r = subprocess.run(cmd, timeout=args.limit)
    sys.exit(r.returncode)


if __name__ == "__main__":
    main()
