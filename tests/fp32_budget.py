"""The error measure of the fp32 tests: an fp32 result is held to the rounding error of the float oracle itself.

For one fp32 case (coordinates, materials, start state already rounded to float):

* the reference ``r64`` is the DOUBLE oracle on those same float inputs promoted to double (``promoted``: geometry
  factors rebuilt from the float-rounded vertex coordinates, not from the fp64 mesh, whose vertices differ by a
  rounding);
* the yardstick ``r32`` is the FLOAT oracle on them (model runs: with the fixed step count, oracle ``steps=``);
* regions: every element layer along x, every boundary face (util.layer_and_face_regions) and the whole vector;
* ``err(a, R) = rms((a - r64)[R]) / rms(r64[R])``; for the whole vector also ``max|a - r64| / max|r64|``;
* ``yard(R) = max(err(r32, R), 2^-23)``: one float ulp is the floor -- a correctly rounded result cannot be asked to
  be closer, and with its fp64 LDS accumulator the GPU may well beat a sequential float sum;
* the GPU result ``g`` passes when ``err(g, R) <= CAP * yard(R)`` in every region, for every field by itself.

CAP follows from the measured ratios by the rule of DESIGN.md section 2 ("fp32 error against the float oracle"):
the smallest power of two >= 2 x the largest ratio measured on the MI355X, never below 2 and never above 8.  The
factor 2 covers the run-to-run variation of the LDS-atomic summation order; the ceiling 8 is a condition, not a
measurement (a kernel three bits worse than a sequential float loop is losing accuracy somewhere)."""
import copy

import numpy as np

EPS32 = 2.0 ** -23
CAP_CEILING = 8          # the condition above; the CPU guards are written against it
# NOT MEASURED YET: the ratio table of DESIGN.md section 2 is still empty, so CAP stands at the ceiling, the one
# value that is a condition and needs no measurement; the rule lowers it once the table is filled.
CAP = 8
YARD_SANE = 128 * EPS32  # a yardstick above this would make the GPU assertion vacuous (test_fp32_guards.py)


def promoted(orc, pr32):
    """The float problem ``pr32`` (util.Problem) as a double problem on the SAME float-rounded coordinates."""
    pr = copy.copy(pr32)
    pr.mesh = copy.copy(pr32.mesh)
    pr.mesh.geometry = copy.copy(pr32.mesh.geometry)
    pr.mesh.geometry.x = np.ascontiguousarray(pr32.mesh.geometry.x, dtype=np.float64)
    pr.dtype = np.dtype(np.float64)
    pr.D = orc.dphi(pr.nodes)
    pr.G, pr.detJ = orc.geometry(pr.tdim, pr.mesh.geometry.x, pr.mesh.geometry.dofmap, pr.nodes, pr.wts)
    return pr


def _rms(a):
    return float(np.sqrt(np.mean(np.square(a)))) if len(a) else 0.0


def errors(a, r64, regions):
    """{measure: err} of one field: "<region>" (rms / rms) for every region, "all" and "all:max" for the vector."""
    a, r64 = np.asarray(a, dtype=np.float64), np.asarray(r64, dtype=np.float64)
    assert a.shape == r64.shape and np.isfinite(a).all(), "result not finite or of another length"
    d = a - r64
    out = {}
    for name, idx in regions.items():
        ref = _rms(r64[idx])
        assert ref > 0, f"reference is zero in {name}"
        out[name] = _rms(d[idx]) / ref
    out["all"] = _rms(d) / _rms(r64)
    out["all:max"] = float(np.abs(d).max() / np.abs(r64).max())
    return out


def yardstick(r32, r64, regions, floor=EPS32):
    return {k: max(e, floor) for k, e in errors(r32, r64, regions).items()}


def as_fields(x):
    """A lone vector is one field "y"; a pair is (u, v)."""
    if isinstance(x, (tuple, list)):
        assert len(x) == 2
        return {"u": x[0], "v": x[1]}
    return {"y": x}


def budget(g, r32, r64, regions, floor=EPS32):
    """(largest ratio err(g, R) / yard(R), (field, measure) where it occurred, {field: {measure: (err, yard)}}).
    ``floor``: one ulp of the type under test (the receivers' fp64 cases pass 2^-52, receiver_ref.py)."""
    g, r32, r64 = as_fields(g), as_fields(r32), as_fields(r64)
    worst, where, table = -1.0, None, {}
    for f in r64:
        e, y = errors(g[f], r64[f], regions), yardstick(r32[f], r64[f], regions, floor)
        table[f] = {k: (e[k], y[k]) for k in e}
        for k in e:
            if e[k] / y[k] > worst:
                worst, where = e[k] / y[k], (f, k)
    return worst, where, table


def report(label, worst, where, table):
    e, y = table[where[0]][where[1]]
    return f"fp32-budget {label}: ratio {worst:.3f} at {where[0]}/{where[1]} (err {e:.3e}, yard {y:.3e})"


def check(label, g, r32, r64, regions, cap=None):
    """Assert the budget; prints the largest ratio and where it occurred (pytest -s, or the failure message)."""
    cap = CAP if cap is None else cap
    worst, where, table = budget(g, r32, r64, regions)
    line = report(label, worst, where, table)
    print(line)
    assert worst <= cap, f"{line} exceeds CAP = {cap}"
    return worst, where, table
