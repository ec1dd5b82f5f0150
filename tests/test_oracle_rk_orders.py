"""The oracle's Lossy and Westervelt steppers at the RK orders 1-3 (oracle only, no GPU).  The order argument restates
the tables orc_linear_rk_n already held; here: at order 4 the new entries return the bits of the entry points that
existed before them (fp64 and fp32, 3-D and 2-D), and at every order the double oracle agrees with the numpy stepper
of source_ref.py, which shares with it only the stiffness action and the model vectors."""
import ctypes as C

import numpy as np
import pytest

import source_ref as sr
from live_cases import F0, S0, Case

SHAPES = {"3d": dict(n=(5, 4, 4), P=3, cfl=0.1, nsteps=20), "2d": dict(n=(6, 5), P=4, cfl=0.2, nsteps=20)}
_cases = {}


def _case(orc, kind, shape, dtype=np.float64):
    key = (kind, shape, np.dtype(dtype).name)
    if key not in _cases:
        _cases[key] = Case(orc, kind=kind, dtype=dtype, **SHAPES[shape])
    return _cases[key]


def _legacy(orc, cs, u0, v0, dtype, steps):
    """The entry points from before the order argument: orc_*_rk4_s (the tf-driven loop) or orc_*_rk4_n (``steps``)."""
    pr = cs.pr if np.dtype(dtype) == np.float64 else cs.prt
    V = cs.vectors(pr)
    suf = "f32" if np.dtype(dtype) == np.float32 else "f64"
    fn = getattr(orc.lib(), f"orc_{cs.kind}_rk4_{'s' if steps is None else 'n'}_{suf}")
    fn.restype = C.c_int64
    keep = [np.ascontiguousarray(x, dtype=dtype) for x in
            ([pr.G] + ([pr.detJ] if cs.kind == "westervelt" else []) + [pr.D, V["coeff"], V["att"]]
             + ([V["n1"], -V["n1"]] if cs.kind == "westervelt" else []) + [V["m"], V["src"], V["absb"], V["src2"]])]
    dm = np.ascontiguousarray(pr.dm, dtype=np.int32)
    u, v = np.array(u0, dtype=dtype), np.array(v0, dtype=dtype)
    tail = [C.c_double(2.0)] + ([] if steps is None else [C.c_int64(steps)])
    k = fn(C.c_int(cs.tdim), C.c_int64(dm.shape[0]), C.c_int64(len(u)), C.c_int(pr.N), dm.ctypes.data_as(C.c_void_p),
           *(x.ctypes.data_as(C.c_void_p) for x in keep), C.c_double(F0), C.c_double(cs.p0), C.c_double(S0),
           C.c_double(0.0), C.c_double(cs.tf), C.c_double(cs.dt), u.ctypes.data_as(C.c_void_p),
           v.ctypes.data_as(C.c_void_p), *tail)
    assert k == cs.nsteps
    return u, v


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("kind", ["lossy", "westervelt"])
def test_order_4_returns_the_same_bits(orc, kind, shape, dtype):
    cs = _case(orc, kind, shape, dtype)
    u0, v0 = (a.astype(dtype) for a in cs.start())
    for fixed in (False, True):
        if dtype == np.float32 and not fixed:
            continue                       # (the float tf-driven loop miscounts its steps: oracle.h)
        new = cs.oracle(u0, v0, dtype=dtype, fixed=fixed, order=4)
        old = _legacy(orc, cs, u0, v0, dtype, cs.nsteps if fixed else None)
        assert np.array_equal(new[0], old[0]) and np.array_equal(new[1], old[1])
        assert np.abs(new[0]).max() > 0 and not np.array_equal(new[0], u0)


@pytest.mark.parametrize("order", [1, 2, 3, 4])
@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("kind", ["lossy", "westervelt"])
def test_orders_against_the_numpy_stepper(orc, kind, shape, order):
    cs = _case(orc, kind, shape)
    u0, v0 = cs.start()
    V = cs.vectors(cs.pr)
    vec = dict(m=V["m"], src=V["src"], absb=V["absb"], src2=V["src2"], lin=V["coeff"], att=V["att"])
    if kind == "westervelt":
        vec["mn1"] = cs.pr.M(np.ones(cs.pr.ndofs), V["n1"])
    assert sr.S0 == S0
    ref = sr.rk_stepper(cs.pr, vec, 2.0, F0, cs.p0, 0.0, cs.dt, cs.nsteps, order=order, u=u0, v=v0)
    # exactly nsteps full steps: the tf-driven loop of the live cases ends 1e-9 nsteps dt early, by more than this bound
    got = cs.oracle(u0, v0, order=order, fixed=True)
    assert max(sr.rel(got[0], ref[0]), sr.rel(got[1], ref[1])) < 1e-12, (sr.rel(got[0], ref[0]), sr.rel(got[1], ref[1]))
    if order < 4:
        # the orders are different steppers: the next table moves the state far beyond that bound
        other = cs.oracle(u0, v0, order=order + 1, fixed=True)
        assert sr.rel(other[1], ref[1]) > 1e-9
    if kind == "westervelt":
        # ... and the nonlinear term is not a spectator of the comparison
        lin = sr.rk_stepper(cs.pr, {k: x for k, x in vec.items() if k != "mn1"}, 2.0, F0, cs.p0, 0.0, cs.dt,
                            cs.nsteps, order=order, u=u0, v=v0)
        assert sr.rel(lin[1], ref[1]) > 1e-9
