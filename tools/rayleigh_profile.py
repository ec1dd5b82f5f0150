"""Rate of the Rayleigh-integral kernel (fusmi.h "transducers"), one process: a bowl of 10^4 surface points (R = 64 mm,
aperture 64 mm, 0.5 MHz, water) against two target sets of the 64^3 p = 4 box of lambda / 2 cells,

    face    the 257^2 = 66 049 DOFs of its source face        volume    its 257^3 = 16 974 593 DOFs

in both precisions, device arrays in and out.  For every call it prints the plan (source chunks, launches, workspace), the
median wall time of the synchronous call, the device time of its "rayleigh" scope (main kernel and chunk reduction) from
the library's event timers, pairs per second from the scope, and the fraction of the fp64 vector rate (256 CUs x 128 flops
per clock x 2.4 GHz = 78.6 Tflop/s) that the flops the kernel's source spells per pair imply: 27 for P, + 22 with the
gradient (csrc/rayleigh.hip; a sine, a cosine, a square root, a reciprocal and a rint count 1 each, so the fraction says how
far the transcendental functions are from free, not how well the multipliers are used).  No number here is a target.

    python tools/rayleigh_profile.py [nsrc] [repeats] [--face-only]

Run without --child it starts itself as a child process under `timeout` and returns the child's status: a step that
hangs ends there, nothing is started after a failure."""
import ctypes as C
import subprocess
import sys
import time

import numpy as np

LIMIT_S = 420

if "--child" not in sys.argv:
    sys.exit(subprocess.run(["timeout", "-k", "10", str(LIMIT_S), sys.executable, sys.argv[0], "--child", *sys.argv[1:]]).returncode)

sys.path.insert(0, "fenicsx-fus_amd")
import fenicsxfus_amd as fa  # noqa: E402
from fenicsxfus_amd import _abi  # noqa: E402
from fenicsxfus_amd import transducer as td  # noqa: E402

argv = [a for a in sys.argv[1:] if not a.startswith("--")]
nsrc = int(argv[0]) if len(argv) > 0 else 10000
repeats = int(argv[1]) if len(argv) > 1 else 5
F, C0, RHO, WARM = 0.5e6, 1500.0, 1000.0, 1
PEAK64 = 256 * 128 * 2.4e9
FLOPS = {False: 27, True: 49}
lam = C0 / F
Lbox, ng = 64 * lam / 2, 257
ctx = fa.Context(0)
lib = _abi.lib()
hip = C.CDLL("libamdhip64.so")


def dev(nbytes, src=None):
    p = C.c_void_p()
    assert hip.hipMalloc(C.byref(p), C.c_size_t(nbytes)) == 0, "hipMalloc"
    if src is not None:
        assert hip.hipMemcpy(p, src.ctypes.data_as(C.c_void_p), C.c_size_t(nbytes), C.c_int(1)) == 0, "hipMemcpy"
    return p


pts, dA, _ = td.bowl([-0.03, Lbox / 2, Lbox / 2], [0.034, Lbox / 2, Lbox / 2], 0.064, nsrc)
q = td.volume_velocity(dA, 1e-3)
g = np.linspace(0.0, Lbox, ng)
face = np.stack(np.meshgrid([0.0], g, g, indexing="ij"), axis=-1).reshape(-1, 3)
sets = {"face": face}
if "--face-only" not in sys.argv:
    sets["volume"] = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
d_pts = dev(pts.nbytes, np.ascontiguousarray(pts))
d_q = dev(16 * nsrc, np.ascontiguousarray(q).view(np.float64))
DEVICE = C.c_int(_abi.FUS_DEVICE)
for sname, tgt in sets.items():
    ntgt = len(tgt)
    d_tgt, d_out = dev(tgt.nbytes, np.ascontiguousarray(tgt)), dev(8 * 9 * ntgt)
    for grad in ((False, True) if sname == "face" else (False,)):
        what = _abi.FUS_RAY_P | ((_abi.FUS_RAY_GRAD | _abi.FUS_RAY_RMIN) if grad else 0)
        pl = td.plan(ctx, nsrc, ntgt, grad, grad)
        for pname, prec in (("f64", _abi.FUS_RAY_F64), ("mixed", _abi.FUS_RAY_MIXED)):
            def fn():
                return lib.fus_rayleigh(ctx.h, C.c_int64(nsrc), d_pts, d_q, C.c_int64(ntgt), d_tgt, C.c_double(F), C.c_double(C0),
                                        C.c_double(RHO), C.c_double(0.0), C.c_int(what), C.c_int(prec), d_out, DEVICE)
            for _ in range(WARM):
                _abi.check(fn())
            ts = []
            for _ in range(repeats):
                ctx.synchronize()
                t0 = time.perf_counter()
                _abi.check(fn())                       # synchronises the stream before it returns
                ts.append((time.perf_counter() - t0) * 1e3)
            ctx.profile_enable(True)
            for _ in range(repeats):
                _abi.check(fn())
            t, c = ctx.profile_get("rayleigh")
            ctx.profile_enable(False)
            scope = t / max(c, 1)
            pairs = float(nsrc) * ntgt
            rate = pairs / (scope * 1e-3)
            print(f"{sname} ({ntgt} targets x {nsrc} sources) {'P+grad+rmin' if grad else 'P'} {pname}: chunks {pl[0]}, launches {pl[2]}, "
                  f"workspace {pl[3]} B; wall median {np.median(ts):.3f} ms (min {min(ts):.3f}, max {max(ts):.3f}, {repeats} calls after "
                  f"{WARM}); scope {scope:.3f} ms; {rate:.3e} pairs/s; {FLOPS[grad]} flops per pair -> {rate * FLOPS[grad] / 1e12:.2f} "
                  f"Tflop/s = {rate * FLOPS[grad] / PEAK64:.3f} of the fp64 vector rate", flush=True)
    assert hip.hipFree(d_tgt) == 0 and hip.hipFree(d_out) == 0
ctx.close()
