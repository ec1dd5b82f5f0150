"""Sources anywhere in the mesh and sampled drive signals, host side (no device): the interpolant header
csrc/source_signal.hpp through a plain C++ driver (also under AddressSanitizer + UBSan, as a stand-alone program)
against its numpy mirror ``source.signal_value``; the helpers ``point_weights``, ``time_reversed`` and
``conjugate_delays``; the numpy stepper of tests/volume_source_ref.py pinned against tests/source_ref.py's; the exported
symbols; and the time-reversal set-up of the GPU test checked on the numpy reference alone."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import fenicsxfus_amd as fa
from fenicsxfus_amd import source as fsrc
import source_ref as sr
import volume_source_ref as vr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fenicsx-fus_amd", "csrc")
DRIVER = os.path.join(ROOT, "tests", "cpp", "source_signal_driver.cpp")
EPS = 2.0 ** -52


def _build(tmp, name, extra):
    exe = tmp / name
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", *extra, "-I", CSRC, DRIVER, "-o", str(exe)])
    return str(exe)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("sig"), "source_signal_driver", ["-O2"])


def run(exe, tmp_path, signals, t_first, ds, chan, t, a=1.0):
    """signals [nchan, nsamp] -> the driver's time-major table; returns (exit code, g, dg)."""
    sig = np.atleast_2d(np.asarray(signals, dtype=np.float64))
    nchan, nsamp = sig.shape
    np.ascontiguousarray(sig.T).tofile(tmp_path / "table.bin")
    np.ascontiguousarray(np.broadcast_to(chan, np.shape(t)), dtype=np.int32).tofile(tmp_path / "chan.bin")
    np.ascontiguousarray(t, dtype=np.float64).tofile(tmp_path / "t.bin")
    num = [float(x).hex() for x in (t_first, ds, a)]                   # exact: strtod reads hexadecimal floats
    out = subprocess.run([exe, str(nchan), str(nsamp), *num, *(str(tmp_path / f) for f in ("table.bin", "chan.bin", "t.bin"))],
                         capture_output=True, text=True)
    if out.returncode != 0:
        return out.returncode, None, None
    gd = np.array([[float(x) for x in line.split()] for line in out.stdout.splitlines()]).reshape(-1, 2)
    assert len(gd) == len(t)
    return 0, gd[:, 0], gd[:, 1]


def edge_times(t_first, ds, nsamp):
    """Times straddling both ends of the support, every joint of the first and last segments, and far outside."""
    out = []
    for j in (-2, -1, 0, 1, nsamp - 2, nsamp - 1, nsamp, nsamp + 1):
        x = t_first + j * ds
        out += [x, np.nextafter(x, -np.inf), np.nextafter(x, np.inf), x - 1e-9 * ds, x + 1e-9 * ds, x + 0.5 * ds]
    return np.array(out + [t_first - 1e6 * ds, t_first + 1e6 * ds, -1e300, 1e300])


def test_header_vs_numpy_mirror(driver, tmp_path):
    """A random table at random times and channels.  Both sides evaluate the same dozen double operations (four
    weights of a few operations each, a four-term sum), so the bound is a few ulp of the largest sample: 16 eps max|s|
    for the value, 32 eps max|s| / ds for the derivative (its weights sum to at most 3 in magnitude).  Measured with g++
    -O2 on x86-64: 0 and 0 -- without contraction both sides round alike; the bound leaves room for a compiler that fuses."""
    rng = np.random.default_rng(11)
    nchan, nsamp, t_first, ds, a = 5, 40, -3.1e-6, 0.37e-7, 1.75
    sig = rng.standard_normal((nchan, nsamp))
    t = np.concatenate([rng.uniform(t_first - 3 * ds, t_first + (nsamp + 3) * ds, 4000), edge_times(t_first, ds, nsamp)])
    chan = rng.integers(0, nchan, len(t))
    rc, g, dg = run(driver, tmp_path, sig, t_first, ds, chan, t, a)
    assert rc == 0
    gm = a * fsrc.signal_value(sig, ds, t_first, t)[chan, np.arange(len(t))]
    dgm = a * fsrc.signal_value(sig, ds, t_first, t, derivative=True)[chan, np.arange(len(t))]
    smax = a * np.abs(sig).max()
    eg, edg = np.abs(g - gm).max() / smax, np.abs(dg - dgm).max() / (smax / ds)
    print(f"source_signal.hpp vs signal_value: value {eg:.2e} max|s|, derivative {edg:.2e} max|s|/ds")
    assert eg <= 16 * EPS and edg <= 32 * EPS
    assert np.abs(g).max() > 0.5 * smax and np.abs(dg).max() > 0.5 * smax / ds
    # one channel, scalar and vector forms of the mirror agree with the table form
    assert np.array_equal(fsrc.signal_value(sig[2], ds, t_first, t), fsrc.signal_value(sig, ds, t_first, t)[2])
    assert fsrc.signal_value(sig[2], ds, t_first, float(t[7])) == fsrc.signal_value(sig, ds, t_first, t)[2, 7]


@pytest.mark.parametrize("nsamp", [2, 3, 17])
def test_exact_at_the_samples_and_zero_outside(driver, tmp_path, nsamp):
    """Dyadic t_first and ds: the sample times and u = 0 are exact, so S returns the sample itself; the derivative
    there is the centred difference of the neighbours; outside [t_first - ds, t_first + nsamp ds) both are exactly 0."""
    rng = np.random.default_rng(nsamp)
    t_first, ds = -0.375, 2.0 ** -4
    sig = rng.standard_normal((3, nsamp))
    j = np.arange(-1, nsamp + 1)
    pad = np.zeros((3, nsamp + 4))
    pad[:, 2:nsamp + 2] = sig
    for c in range(3):
        rc, g, dg = run(driver, tmp_path, sig, t_first, ds, c, t_first + j * ds)
        assert rc == 0
        assert np.array_equal(g, pad[c, j + 2])
        live = j < nsamp          # (t_first + nsamp ds is the first time past the support)
        central = (pad[c, j + 3] - pad[c, j + 1]) / (2 * ds)
        assert np.all(np.abs(dg - central)[live] <= 4 * EPS * np.abs(sig).max() / ds) and dg[~live].tolist() == [0.0]
        assert np.array_equal(fsrc.signal_value(sig[c], ds, t_first, t_first + j * ds), g)
        lo = np.array([np.nextafter(t_first - ds, -np.inf), t_first - 1.5 * ds, t_first - 2 * ds, -1e300, -np.inf])
        hi = np.array([t_first + nsamp * ds, t_first + (nsamp + 0.5) * ds, t_first + (nsamp + 2) * ds, 1e300, np.inf])
        for dead in (lo, hi, np.array([np.nan])):
            rc, g0, dg0 = run(driver, tmp_path, sig, t_first, ds, c, dead)
            assert rc == 0 and not g0.any() and not dg0.any()
            assert not fsrc.signal_value(sig[c], ds, t_first, dead).any()
            assert not fsrc.signal_value(sig[c], ds, t_first, dead, derivative=True).any()
    # inside the first and the last segment the padded zeros count as samples: not 0
    rc, g, _ = run(driver, tmp_path, sig, t_first, ds, 0, np.array([t_first - 0.5 * ds, t_first + (nsamp - 0.5) * ds]))
    assert rc == 0 and g[0] != 0.0 and g[1] != 0.0


def test_dg_is_the_derivative_of_g(driver, tmp_path):
    """Central difference of S with step h against S'.  On a segment S''' = 3 (-s0 + 3 s1 - 3 s2 + s3) / ds^3, at most
    24 max|s| / ds^3, so the truncation error is at most h^2 / 6 of that; the rounding error 2 x 16 eps max|s| / (2 h).
    Points within 2 h of a joint are left out: S is only C^1 there."""
    rng = np.random.default_rng(3)
    nsamp, t_first, ds = 25, 1.3e-6, 0.41e-7
    sig = rng.standard_normal((2, nsamp))
    h = 1e-4 * ds
    t = rng.uniform(t_first - 2 * ds, t_first + (nsamp + 1) * ds, 1500)
    x = (t - t_first) / ds
    t = t[np.abs(x - np.round(x)) > 2e-4]
    smax = np.abs(sig).max()
    for c in range(2):
        _, gp, _ = run(driver, tmp_path, sig, t_first, ds, c, t + h)
        _, gm, _ = run(driver, tmp_path, sig, t_first, ds, c, t - h)
        _, _, dg = run(driver, tmp_path, sig, t_first, ds, c, t)
        hh = ((t + h) - (t - h)) / 2
        bound = h * h / 6 * 24 * smax / ds**3 + 16 * EPS * smax / h
        assert np.all(np.abs((gp - gm) / (2 * hh) - dg) <= bound)
        assert bound < 1e-6 * smax / ds and np.abs(dg).max() > 0.5 * smax / ds      # the check resolves dg


def test_bad_table_shapes_are_refused(driver, tmp_path):
    sig = np.ones((1, 4))
    t = np.array([0.0])
    assert run(driver, tmp_path, sig, 0.0, 1.0, 0, t)[0] == 0
    assert run(driver, tmp_path, sig[:, :1], 0.0, 1.0, 0, t)[0] == 2            # nsamp < 2
    for ds in (0.0, -1.0, np.inf, np.nan):
        assert run(driver, tmp_path, sig, 0.0, ds, 0, t)[0] == 2
    for t_first in (np.inf, -np.inf, np.nan):
        assert run(driver, tmp_path, sig, t_first, 1.0, 0, t)[0] == 2


def test_driver_clean_under_sanitizers(tmp_path):
    """The header's host code as a stand-alone program under AddressSanitizer + UBSan (never loaded into python): the
    table sits in an allocation of exactly its size, the times run through both ends of the support and every joint of
    the end segments, for the smallest table and a larger one."""
    exe = _build(tmp_path, "source_signal_driver_san", ["-O1", "-g", "-fsanitize=address,undefined",
                                                         "-fno-sanitize-recover=all"])
    rng = np.random.default_rng(7)
    for nchan, nsamp in ((1, 2), (3, 2), (4, 9)):
        sig = rng.standard_normal((nchan, nsamp))
        for t_first, ds in ((0.0, 1.0), (-2.5e-6, 0.37e-7)):
            t = edge_times(t_first, ds, nsamp)
            for c in (0, nchan - 1):
                rc, g, dg = run(exe, tmp_path, sig, t_first, ds, c, t)
                assert rc == 0 and np.isfinite(g).all() and np.isfinite(dg).all()
                assert np.abs(g - fsrc.signal_value(sig[c], ds, t_first, t)).max() <= 16 * EPS * np.abs(sig).max()
    assert run(exe, tmp_path, np.ones((1, 1)), 0.0, 1.0, 0, np.array([0.0]))[0] == 2


# ---- helpers ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tdim,P,perturb", [(2, 4, 0.0), (2, 4, 0.15), (3, 3, 0.0), (3, 3, 0.1)])
def test_point_weights(tdim, P, perturb):
    """The weights are the transpose of point evaluation: they sum to the strength, and sum_d w_d f(X_d) = q f(X0) for
    every polynomial f of degree <= P per direction in the located cell's reference coordinates (X_d: the reference
    nodes of the cell's DOFs), also on a perturbed mesh.  Points outside the mesh are dropped."""
    from fenicsxfus_amd.evaluate import locate

    n = (3, 2) if tdim == 2 else (2, 2, 2)
    mesh = fa.BoxMesh([0.0] * tdim, [1.0] * tdim, n, perturb=perturb)
    V = fa.FunctionSpace(mesh, P)
    rng = np.random.default_rng(tdim * 10 + P)
    pts = rng.uniform(0.05, 0.95, (4, tdim))
    q = np.array([1.5, -2.0, 0.25, 3.0])
    nodes = np.asarray(V.nodes1d)
    grids = np.stack([g.ravel() for g in np.meshgrid(*([nodes] * tdim), indexing="ij")], axis=1)   # X_d per local dof
    for k in range(len(pts)):
        w = fsrc.point_weights(V, pts[k:k + 1], q[k])
        assert w.shape == (V.num_dofs,) and abs(w.sum() - q[k]) <= 64 * EPS * abs(q[k])
        cell, X = locate(mesh, pts[k:k + 1])
        dofs = np.asarray(V.tensor_dofmap)[cell[0]]
        assert np.count_nonzero(w) <= len(dofs) and not np.delete(w, dofs).any()
        for _ in range(6):
            e = rng.integers(0, P + 1, tdim)
            f = lambda Y: np.prod(Y ** e, axis=-1)                                                # noqa: E731
            lhs, rhs = w[dofs] @ f(grids), q[k] * f(X[0])
            assert abs(lhs - rhs) <= 1e-12 * abs(q[k]), (e, lhs, rhs)
    # several points accumulate; a point outside contributes nothing
    w_all = fsrc.point_weights(V, pts, q)
    assert np.allclose(w_all, sum(fsrc.point_weights(V, pts[k:k + 1], q[k]) for k in range(4)), rtol=0, atol=1e-14)
    out = np.vstack([pts[:1], np.full((1, tdim), 1.7)])
    assert np.array_equal(fsrc.point_weights(V, out, 1.5), fsrc.point_weights(V, pts[:1], 1.5))
    assert not fsrc.point_weights(V, np.full((1, tdim), -0.3)).any()
    # a point on a node: the unit vector of that DOF
    Xd = V.tabulate_dof_coordinates()[:, :tdim]
    d = int(np.argmin(np.linalg.norm(Xd - 0.4, axis=1)))
    wn = fsrc.point_weights(V, Xd[d:d + 1], 2.0)
    assert abs(wn[d] - 2.0) <= 1e-9 and np.abs(np.delete(wn, d)).max() <= 1e-9


def test_time_reversed():
    rng = np.random.default_rng(1)
    rec, times = rng.standard_normal((50, 3)), 0.25 + 0.125 * np.arange(50)
    sig, ds, t_first = fsrc.time_reversed(rec, times)
    assert sig.shape == (3, 50) and sig.flags.c_contiguous and ds == 0.125 and t_first == 0.0
    assert np.array_equal(sig[:, 0], rec[-1]) and np.array_equal(sig[:, -1], rec[0])
    # the sample recorded at times[-1] - s is played at time s
    for k in (0, 7, 49):
        assert np.array_equal(fsrc.signal_value(sig, ds, t_first, k * ds), rec[49 - k])
    with pytest.raises(ValueError):
        fsrc.time_reversed(rec, times[::-1])
    with pytest.raises(ValueError):
        fsrc.time_reversed(rec, np.r_[times[:-1], times[-1] + 0.01])
    with pytest.raises(ValueError):
        fsrc.time_reversed(rec[:, 0], times)


def test_conjugate_delays():
    """Synthetic maps of A cos(2 pi f t - phi): the delays lie in [0, 1 / f) and cos(2 pi f (t - tau)) has phase +phi."""
    rng = np.random.default_rng(2)
    f = 0.5e6
    A, phi = rng.uniform(0.1, 3.0, 500), rng.uniform(-np.pi, np.pi, 500)
    phi[:4] = [0.0, np.pi, -np.pi, 0.5 * np.pi]
    tau = fsrc.conjugate_delays(A * np.cos(phi), A * np.sin(phi), f)
    assert tau.shape == phi.shape and np.all(tau >= 0.0) and np.all(tau < 1.0 / f)
    assert np.ptp(tau) > 0.9 / f
    for t in (0.0, 0.3 / f, 7.77 / f):
        assert np.abs(np.cos(2 * np.pi * f * (t - tau)) - np.cos(2 * np.pi * f * t + phi)).max() <= 1e-12 * max(1.0, f * t) * 64
    assert tau[0] == 0.0 and abs(tau[3] - 0.75 / f) <= 1e-12 / f
    # a spherical wave from a target: conjugation undoes the travel time, tau + r / c is constant modulo a period
    c, x = 1500.0, rng.uniform(-0.02, 0.02, (300, 2))
    r = np.linalg.norm(x - np.array([0.03, 0.001]), axis=1)
    ph = 2 * np.pi * f * r / c                                      # field cos(2 pi f (t - r / c))
    tau = fsrc.conjugate_delays(np.cos(ph) / r, np.sin(ph) / r, f)
    arrival = np.mod(f * (tau + r / c) + 0.5, 1.0)
    assert np.ptp(arrival) <= 1e-9
    assert fsrc.conjugate_delays(np.zeros(3), np.zeros(3), f).tolist() == [0.0] * 3


def test_library_exports_the_new_entries():
    """Fails before the feature exists: the C ABI has both entries, the binding lists them, the wrappers exist."""
    from fenicsxfus_amd import _abi

    lib = ctypes.CDLL(_abi.LIB_PATH)
    for name in ("fus_model_set_source_weights", "fus_model_set_source_signals"):
        assert hasattr(lib, name) and name in _abi.SYMBOLS
    for cls in (fa.LinearSpectralExplicit, fa.LossySpectralExplicit, fa.WesterveltSpectralExplicit):
        assert callable(cls.set_source_weights) and callable(cls.set_source_signals)
    with open(os.path.join(ROOT, "include", "fusmi.hpp")) as f:
        text = f.read()
    assert "set_source_weights(" in text and "set_source_signals(" in text


# ---- the reference stepper ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,forms", [("linear", 0), ("lossy", 0), ("lossy", 1), ("westervelt", 0)])
def test_stepper_is_source_refs_stepper(orc, kind, forms):
    """volume_source_ref.rk_stepper with w = the facet weights and g = the analytic waveform per DOF against
    source_ref.rk_stepper on the 3-D case of the GPU tests: the same formulas, 1e-14 relative."""
    cs = sr.case3d(orc)
    amp, tau = cs.aperture()
    t0, D = cs.t0s()["burst_end"]
    vec, scale = vr.westervelt_vectors(cs, forms) if kind == "westervelt" else cs.vectors(kind, forms)
    p0 = 6e6 if kind == "westervelt" else 6e4
    for order in ((4, 2) if kind == "linear" else (4,)):
        ref = sr.rk_stepper(cs.pr, vec, scale, cs.f0, p0, t0, cs.dt, sr.NSTEPS, amp, tau, D, order)
        g, dg = vr.analytic(cs.f0, p0, scale, amp, tau, D)
        got = vr.rk_stepper(cs.pr, vec, vec["src"], g, dg, t0, cs.dt, sr.NSTEPS, order)
        assert np.abs(ref[0]).max() > 0
        assert sr.rel(got[0], ref[0]) <= 1e-14 and sr.rel(got[1], ref[1]) <= 1e-14


def test_sampled_source_of_the_stepper_is_signal_value():
    sig = np.random.default_rng(4).standard_normal((3, 12))
    ch = np.array([0, -1, 2, 2, 1, -1])
    amp, tau = np.array([1.0, 2.0, 0.5, 1.5, 1.0, 1.0]), np.array([0.0, 0.1, 0.2, 0.0, 0.3, 0.0])
    g, dg = vr.sampled(sig, 0.25, -0.5, ch, amp, tau)
    for t in (-1.0, 0.1, 1.37, 5.0):
        for fn, der in ((g, False), (dg, True)):
            want = [0.0 if c < 0 else a * fsrc.signal_value(sig[c], 0.25, -0.5, t - d, derivative=der)
                    for c, a, d in zip(ch, amp, tau)]
            assert np.array_equal(fn(t), np.array(want))
    g1, _ = vr.sampled(sig, 0.25, -0.5, ch)                       # equal delays: the one-call branch
    assert np.array_equal(g1(1.37), np.where(ch >= 0, fsrc.signal_value(sig, 0.25, -0.5, 1.37)[np.maximum(ch, 0)], 0.0))


# ---- time reversal on the numpy reference alone ----------------------------------------------------------------------
def test_time_reversal_guard(orc):
    """The conditions of the GPU time-reversal test, on the stepper: a point source at (4.2, 3.1) wavelengths (not a
    node, through point_weights) emits an 8-period burst, u is recorded on the 65 DOFs of the face x = 0 for 992 steps,
    the reversed recording is played back from that face for 992 steps.  Along the mesh column nearest the source the
    maximum of the playback's peak-|u| map lies within half a wavelength of the source's y, and the peak at the DOF
    nearest the source is at least 3 x the column's median.  Measured: 0.014 wavelengths and 9.96."""
    S = vr.tr_setup(orc)
    assert len(S["face"]) == 65 and S["pr"].ndofs == 65 * 65
    assert np.linalg.norm(S["X"][S["inear"]] - S["x0"]) > 0.02 * S["lam"]          # the point is not a node
    assert abs(S["w"].sum() - 1.0) < 1e-12 and np.count_nonzero(S["w"]) == 25
    times, rec = vr.tr_forward(orc)
    assert np.abs(rec).max() > 0
    sig, ds, t_first = fsrc.time_reversed(rec, times)
    assert abs(ds - S["dt"]) <= 1e-12 * S["dt"] and sig.shape == (65, vr.TR_STEPS)
    peak, _ = vr.tr_playback(orc, sig, ds, t_first)
    dist, ratio = vr.tr_conditions(S, peak)
    print(f"time reversal (numpy): |y_max - y_src| = {dist:.3f} wavelengths, peak / column median = {ratio:.2f}")
    assert dist <= 0.5
    assert ratio >= 3.0
