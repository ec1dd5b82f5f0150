"""The wave model's replaceable device arrays: replacing them neither accumulates memory nor disturbs a run.

1. ``fus_model_set_receivers`` + ``fus_model_record`` called over and over must not grow the device's used memory: one
   call pair allocates S bytes (worked out below from the array shapes), a model that kept every generation until it
   is destroyed grows by 7 S between the first and the eighth call, one that replaces them by nothing.  The bound, 2 S,
   follows from those sizes alone.  Used memory is device-wide and the device may be shared, so up to three windows of
   eight calls are taken and the first that meets the bound passes: a leak is monotone and shows in every window.
2. After cycling through every setter that replaces arrays (the three source setters and clear_source, the monitor
   with and without harmonics and off, the receivers), a run is bit-identical to that of a fresh model configured
   once with the final settings (option deterministic = 1: fixed summation order)."""
import ctypes as C

import numpy as np
import pytest

import fenicsxfus_amd as fa
from fenicsxfus_amd import _abi
from fenicsxfus_amd import source as fsrc
from fenicsxfus_amd._abi import check, lib, ptr

pytestmark = pytest.mark.gpu

F0, P0, S0 = 0.5e6, 60000.0, 1500.0
L, P = 0.012, 2
NPTS, CAP = 300_000, 30
ND, NB = (P + 1) ** 3, 3 * (P + 1)           # per receiver: dof indices (int32) and 1-D basis values (fp64)
S_BYTES = NPTS * (ND * 4 + NB * 8 + 8) + CAP * NPTS * 8   # idx + bas + out, and the record buffer: about 128 MB


def _model(deterministic=None):
    mesh = fa.BoxMesh([0, 0, 0], [L, L, L], (2, 2, 2))
    V = fa.FunctionSpace(mesh, P)
    nc = mesh.num_cells
    dt = 0.5 * (L / 2) / (1500.0 * P**2)
    ctx = fa.Context(0, deterministic=deterministic)
    mdl = fa.LinearSpectralExplicit(mesh, fa.tag_box_boundary(mesh), P, np.full(nc, 1500.0), np.full(nc, 1000.0), F0, P0, S0,
                                    4, dt, V=V, ctx=ctx)
    return mdl, V, dt


def _hip_runtime():
    """The HIP runtime libfusmi.so has loaded into this process."""
    lib()
    with open("/proc/self/maps") as f:
        paths = {ln.split()[-1] for ln in f if "libamdhip64" in ln}
    assert paths, "libfusmi.so is loaded but no libamdhip64 is mapped"
    return C.CDLL(sorted(paths)[0])


def _used_bytes(hip):
    free, total = C.c_size_t(), C.c_size_t()
    assert hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return total.value - free.value


def test_receivers_and_records_do_not_accumulate():
    mdl, V, _ = _model()
    hip = _hip_runtime()
    rng = np.random.default_rng(5)
    Xr = np.full((NPTS, 3), 0.3)                 # one interior reference point, in every cell
    growth = []
    for window in range(3):
        for it in range(1, 9):
            cells = np.ascontiguousarray(rng.integers(0, 8, NPTS), dtype=np.int32)
            check(lib().fus_model_set_receivers(mdl.h, C.c_int64(NPTS), ptr(cells), ptr(Xr)))
            check(lib().fus_model_record(mdl.h, C.c_int(_abi.FUS_U), C.c_int(1), C.c_int64(CAP)))
            mdl.ctx.synchronize()
            if it == 1:
                first = _used_bytes(hip)
        growth.append(_used_bytes(hip) - first)
        print(f"window {window}: used memory grew by {growth[-1] / S_BYTES:.3f} S between call 1 and call 8 (S = {S_BYTES} bytes)")
        if growth[-1] < 2 * S_BYTES:
            break
    assert growth[-1] < 2 * S_BYTES, f"growth over calls 1..8 in {len(growth)} windows: {[g / S_BYTES for g in growth]} S"
    # the arrays of the last call are the live ones: the basis values at any point sum to one
    mdl._nrecv = NPTS
    mdl.set_state(u=np.ones(V.num_dofs))
    assert np.abs(mdl.sample("u") - 1.0).max() < 1e-13
    mdl.close()
    mdl.ctx.close()


def _settings(V, dt, k):
    """The arguments of cycle k: they differ from cycle to cycle, so that every call replaces what the last one set."""
    X = V.tabulate_dof_coordinates()
    rng = np.random.default_rng(100 + k)
    t = dt * np.arange(64)
    return dict(delay=(2 + k) * dt * X[:, 1] / L, amplitude=1.0 + 0.1 * k * X[:, 2] / L,
                signals=np.vstack([np.sin(2 * np.pi * F0 * t) * (1 + k), np.cos(2 * np.pi * F0 * t) * t / t[-1]]),
                channel=np.ascontiguousarray(X[:, 1] > 0.5 * L, dtype=np.int32),
                weights=fsrc.point_weights(V, rng.uniform(0.2 * L, 0.8 * L, size=(1, 3)), 3e-6 * (1 + k)),
                points=rng.uniform(0.0, L, size=(100, 3)))


def _run(mdl, dt, nsteps=10):
    mdl.record(1, nsteps)
    mdl.init()
    mdl.rk4_steps(0.0, dt, nsteps)
    mdl.u_sol()
    times, rec = mdl.records()
    assert len(times) == nsteps and np.abs(mdl.u_n.x.array).max() > 0 and np.abs(rec).max() > 0
    return mdl.u_n.x.array.copy(), mdl.v_n.x.array.copy(), times, rec


def test_replacing_keeps_working():
    mdl, V, dt = _model(deterministic=True)
    mdl.init()
    for k in range(5):
        s = _settings(V, dt, k)
        for setter in (lambda: mdl.set_source(amplitude=s["amplitude"], delay=s["delay"]),
                       lambda: mdl.set_source_signals(s["signals"], dt, channel=s["channel"], delay=s["delay"]),
                       lambda: mdl.set_source_weights(s["weights"]),
                       mdl.clear_source,
                       lambda: mdl.monitor("u", nharm=3),
                       lambda: mdl.monitor("u", nharm=0),
                       mdl.monitor_off,
                       lambda: mdl.set_receivers(s["points"])):
            setter()
            mdl.rk4_steps(0.0, dt, 2)          # the replaced arrays are the ones the kernels read
    got = _run(mdl, dt)
    fresh, _, _ = _model(deterministic=True)
    fresh.set_source_weights(s["weights"])
    fresh.set_receivers(s["points"])
    want = _run(fresh, dt)
    for a, b in zip(got, want):
        assert np.array_equal(a, b)
    # and once more from the state that holds the most arrays: sampled signals over the point weight, monitor with harmonics
    maps = []
    for m in (mdl, fresh):
        m.set_source_signals(s["signals"], dt, channel=s["channel"], amplitude=s["amplitude"], delay=s["delay"])
        m.monitor("u", nharm=3)
        maps.append(_run(m, dt) + tuple(m.monitor_get(q, h).x.array.copy() for q, h in (("rms", None), ("cos", 3), ("sin", 1))))
    for a, b in zip(*maps):
        assert np.array_equal(a, b)
    for m in (mdl, fresh):
        m.close()
        m.ctx.close()
