"""Wall time of the bioheat model's two integrators for the same simulated duration (fusmi.h "bioheat"): 64^3 hexahedra,
degree 4, fp64, tissue properties.  Classical RK4 at stable_dt(), RKL2 with 8 and with 16 stages at stable_dt(stages),
each covering 200 * stable_dt() of simulated time in the fewest equal steps that stay inside its stable step.

    python tools/thermal_sts_timing.py [--n 64] [--P 4] [--repeats 5] [--limit 420] [--out results.json]

The parent starts two worker processes one after the other, each under its own time limit, and stops at the first that
fails.  Worker "wall": one warm-up run of every scheme, then `repeats` rounds that alternate the three schemes; a round
times fus_thermal_steps / fus_thermal_steps_sts with the host clock between two stream synchronisations (the calls end
in one themselves).  Worker "kernels": the same three runs once more under the library's HIP-event timers (profile
scopes "thermal", "thermal_sts", "stiffness", "shared"), which drain the queue between kernels and are therefore kept
out of the wall-time pass.  Prints one JSON line: medians, spreads, ratios, kernel times per launch."""
import argparse
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "fenicsx-fus_amd"))
SCHEMES = (0, 8, 16)
SPAN = 200          # simulated time in units of the RK4 step


def setup(n, P):
    import numpy as np

    import fenicsxfus_amd as fa

    L = 0.003 * n                     # 3 mm cells
    mesh = fa.BoxMesh([0, 0, 0], [L, L, L], (n, n, n))
    V = fa.FunctionSpace(mesh, P)
    ctx = fa.Context(0)
    th = fa.BioheatSpectralExplicit(mesh, P, 0.52, 1040.0 * 3600.0, 4e4, V=V, ctx=ctx)
    X = V.tabulate_dof_coordinates()
    th.set_heat(5e7 * np.exp(-((X - 0.5 * L) ** 2).sum(axis=1) / (2 * (0.1 * L) ** 2)))
    dts = {s: th.stable_dt(stages=s) for s in SCHEMES}
    total = SPAN * dts[0]
    plan = {}
    for s in SCHEMES:
        steps = int(np.ceil(total / dts[s] * (1 - 1e-12)))
        plan[s] = (total / steps, steps)
    return ctx, th, V, plan, dts


def run(th, ctx, plan, s):
    dt, steps = plan[s]
    th.init()
    ctx.synchronize()
    t0 = time.perf_counter()
    th.steps(dt, steps, stages=s)
    ctx.synchronize()
    return time.perf_counter() - t0


def worker(args):
    import numpy as np

    ctx, th, V, plan, dts = setup(args.n, args.P)
    out = {"ndofs": int(V.num_dofs), "stable_dt": {str(s): dts[s] for s in SCHEMES},
           "steps": {str(s): plan[s][1] for s in SCHEMES},
           "operator_applications": {str(s): plan[s][1] * (s or 4) for s in SCHEMES}}
    if args.worker == "wall":
        peak = {}
        for s in SCHEMES:                                  # warm-up: code objects, the F_0 vector
            run(th, ctx, plan, s)
            peak[str(s)] = float(th.rise().x.array.max())
        secs = {s: [] for s in SCHEMES}
        for _ in range(args.repeats):
            for s in SCHEMES:
                secs[s].append(run(th, ctx, plan, s))
        out["wall_s"] = {str(s): secs[s] for s in SCHEMES}
        out["median_s"] = {str(s): float(np.median(secs[s])) for s in SCHEMES}
        out["peak_rise"] = peak
    else:
        out["kernel_ms_per_launch"] = {}
        for s in SCHEMES:
            run(th, ctx, plan, s)
            ctx.profile_enable(True)
            run(th, ctx, plan, s)
            k = {}
            for name in ("thermal", "thermal_sts", "stiffness", "shared"):
                ms, cnt = ctx.profile_get(name)
                if cnt:
                    k[name] = {"ms": ms / cnt, "count": int(cnt)}
            ctx.profile_enable(False)
            out["kernel_ms_per_launch"][str(s)] = k
    th.close()
    ctx.close()
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--P", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--limit", type=int, default=420, help="time limit of each worker process in seconds")
    ap.add_argument("--out", default=None)
    ap.add_argument("--worker", choices=("wall", "kernels"), default=None)
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    res = {}
    for kind in ("wall", "kernels"):
        cmd = [sys.executable, os.path.abspath(__file__), "--worker", kind, "--n", str(args.n), "--P", str(args.P),
               "--repeats", str(args.repeats)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not lines:
            sys.stderr.write(r.stdout + r.stderr)
            sys.exit(f"worker {kind} failed with exit code {r.returncode}: nothing further is started")
        res.update(json.loads(lines[-1][7:]))
    med = res["median_s"]
    res["ratio_rk4_over_s8"] = med["0"] / med["8"]
    res["ratio_rk4_over_s16"] = med["0"] / med["16"]
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
