"""Cost of the bioheat model's perfusion response and damage integral (fusmi.h "bioheat", fus_thermal_set_response /
fus_thermal_set_damage): 64^3 hexahedra, degree 4, fp64, tissue properties, RK4 (--stages 0) or RKL2 steps, timed by the
host clock and, in a pass of its own, by the library's HIP-event timers (profile scopes "thermal" / "thermal_sts",
"stiffness", "shared", "thermal_response").

    python tools/thermal_response_timing.py [--n 64] [--P 4] [--steps 30] [--repeats 3] [--stages 0] [--mode off|on]
                                            [--limit 300]

--mode off: neither is ever set (this also runs on a library from before they existed, named by FUSMI_LIB, for the
comparison with the parent commit).  --mode on: knots (37, 1), (41, 4), (45, 4), shutdown between 10 and 240 CEM43
minutes, Henriques' damage constants.  Both modes step at the step rule of the `on` operator (phi_max = 4), so that they
do the same number of operator applications on the same states' scale.  The parent starts one worker process under a time
limit; the worker warms up with 5 steps, then runs `repeats` rounds of `steps` steps by the host clock and `repeats`
rounds under the event timers.  Prints one JSON line with the per-round times per step and their medians."""
import argparse
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "fenicsx-fus_amd"))
KNOTS = ((37.0, 41.0, 45.0), (1.0, 4.0, 4.0))
DOSE_RANGE = (10.0, 240.0)
HENRIQUES = (3.1e98, 6.28e5)


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
    th.set_heat(1e6 * np.exp(-((X - 0.5 * L) ** 2).sum(axis=1) / (2 * (0.1 * L) ** 2)))
    # the step of the operator with phi_max = 4 m_W: lambda_max of the passive operator plus at most 3 max(m_W / m_C)
    lam = th.lambda_max(20) + 3.0 * 4e4 / (1040.0 * 3600.0)
    dt = 2.0 / lam if args.stages == 0 else 0.72 * (args.stages ** 2 + args.stages - 2) / (2.0 * lam)
    if args.mode == "on":
        th.set_response(*KNOTS, dose_range=DOSE_RANGE)
        th.set_damage(*HENRIQUES)
    th.init()
    scopes = ("thermal" if args.stages == 0 else "thermal_sts", "stiffness", "shared", "thermal_response")
    th.steps(dt, 5, stages=args.stages)
    wall = []
    for _ in range(args.repeats):
        ctx.synchronize()
        t0 = time.perf_counter()
        th.steps(dt, args.steps, stages=args.stages)
        ctx.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3 / args.steps)
    rounds = []
    for _ in range(args.repeats):
        ctx.profile_enable(True)
        th.steps(dt, args.steps, stages=args.stages)
        got = {name: ctx.profile_get(name) for name in scopes}
        ctx.profile_enable(False)
        rounds.append({name: {"ms_per_step": ms / args.steps, "launches": cnt} for name, (ms, cnt) in got.items()})
    kernel = [sum(r[name]["ms_per_step"] for name in scopes) for r in rounds]
    out = {"mode": args.mode, "stages": args.stages, "n": n, "P": P, "steps": args.steps, "ndofs": int(V.num_dofs),
           "dt": dt, "lib": os.environ.get("FUSMI_LIB", "in-tree"),
           "wall_ms_per_step": wall, "wall_ms_per_step_median": float(np.median(wall)),
           "kernel_ms_per_step": kernel, "kernel_ms_per_step_median": float(np.median(kernel)), "rounds": rounds,
           "peak_rise": float(th.rise().x.array.max())}
    rs = [r["thermal_response"] for r in rounds if r["thermal_response"]["launches"]]
    if rs:
        out["thermal_response_us_per_launch"] = [r["ms_per_step"] * args.steps / r["launches"] * 1e3 for r in rs]
        out["thermal_response_share_of_kernel_time"] = [r["thermal_response"]["ms_per_step"] / k
                                                        for r, k in zip(rounds, kernel)]
        out["peak_damage"] = float(th.damage().x.array.max())
    th.close()
    ctx.close()
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--P", type=int, default=4)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--stages", type=int, default=0)
    ap.add_argument("--mode", choices=("off", "on"), default="off")
    ap.add_argument("--limit", type=int, default=300)
    ap.add_argument("--worker", action="store_true")
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--n", str(args.n), "--P", str(args.P), "--steps",
           str(args.steps), "--repeats", str(args.repeats), "--stages", str(args.stages), "--mode", args.mode]
    r = subprocess.run(cmd, timeout=args.limit)
    sys.exit(r.returncode)


if __name__ == "__main__":
    main()
