"""Phased / apodised source, host side (no device): the waveform header csrc/source_wave.hpp through a plain C++ driver
(also under AddressSanitizer + UBSan, as a stand-alone program), its numpy mirror ``source.waveform``, the delay
helpers, the exported symbol, and the numpy RK stepper the GPU tests use as their reference (tests/source_ref.py)
pinned against the oracle's steppers with the uniform source."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import fenicsxfus_amd as fa
from fenicsxfus_amd import source as fsrc
import source_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fenicsx-fus_amd", "csrc")
DRIVER = os.path.join(ROOT, "tests", "cpp", "source_wave_driver.cpp")

F, P0, S0, SCALE, A = 0.5e6, 6e4, 1500.0, 2.0, 1.25
LR = 4.0 / F
D_BURST = 10.0 / F
W0 = 2 * np.pi * F
C = SCALE * P0 * W0 / S0


def _build(tmp, name, extra):
    exe = tmp / name
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", *extra, "-I", CSRC, DRIVER, "-o", str(exe)])
    return str(exe)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("src"), "source_wave_driver", ["-O2"])


def run(exe, tmp_path, s, D, a=A, f=F):
    path = tmp_path / "s.bin"
    np.ascontiguousarray(s, dtype=np.float64).tofile(path)
    num = [float(x).hex() for x in (f, P0, S0, SCALE, D, a)]        # exact: strtod reads hexadecimal floats
    out = subprocess.run([exe, *num, str(path)], capture_output=True, text=True)
    if out.returncode != 0:
        return out.returncode, None, None
    gd = np.array([[float(x) for x in line.split()] for line in out.stdout.splitlines()]).reshape(-1, 2)
    assert len(gd) == len(s)
    return 0, gd[:, 0], gd[:, 1]


def grid(D):
    """Local times s: a uniform grid over the whole support and beyond, plus values straddling every joint."""
    joints = [0.0, LR] + ([D - LR, D] if D > 0 else [])
    end = (D if D > 0 else 2 * LR) + LR
    s = list(np.linspace(-LR, end, 1201))
    for j in joints:
        s += [j, np.nextafter(j, -np.inf), np.nextafter(j, np.inf), j - 1e-9 / F, j + 1e-9 / F, j - 1e-3 / F, j + 1e-3 / F]
    return np.array(sorted(s)), joints


@pytest.mark.parametrize("D", [0.0, D_BURST], ids=["continuous", "burst"])
def test_waveform_header_vs_numpy_mirror(driver, tmp_path, D):
    s, joints = grid(D)
    rc, g, dg = run(driver, tmp_path, s, D)
    assert rc == 0
    # the numpy mirror, to 1e-14 relative of C (resp. C w0); t = s with tau = 0, and through tau with t = 0.3 Lr
    for t, tau in ((s, 0.0), (0.3 * LR, 0.3 * LR - s)):
        gm = fsrc.waveform(t, F, P0, S0, A, tau, D, SCALE)
        dgm = fsrc.waveform(t, F, P0, S0, A, tau, D, SCALE, derivative=True)
        ulp_s = (np.abs(tau) + t) * 2.0 ** -52 if np.ndim(tau) else 0.0      # t - tau re-rounds s: an ulp of its terms
        assert np.all(np.abs(g - gm) <= 1e-14 * A * C + A * C * W0 * ulp_s)
        assert np.all(np.abs(dg - dgm) <= 1e-14 * A * C * W0 + A * C * W0 * W0 * ulp_s)
    # exactly zero before the delay has passed and after the burst
    dead = (s <= 0) | ((s >= D) if D > 0 else False)
    assert dead.any() and np.all(g[dead] == 0.0) and np.all(dg[dead] == 0.0)
    assert np.abs(g[~dead]).max() > 0.9 * A * C
    # continuity of g and dg at the joints: across one ulp of s both change by no more than their Lipschitz bounds
    # |g'| <= A C (W0 + q), |dg'| <= A C (W0 + q)^2 with q = pi f / 4, plus rounding
    q = np.pi * F / 4
    for j in joints:
        lo, hi = np.nextafter(j, -np.inf), np.nextafter(j, np.inf)
        i0, i1 = np.flatnonzero(s == lo)[0], np.flatnonzero(s == hi)[0]
        gap = hi - lo
        assert abs(g[i1] - g[i0]) <= A * C * (W0 + q) * gap + 1e-14 * A * C, j
        assert abs(dg[i1] - dg[i0]) <= A * C * (W0 + q) ** 2 * gap + 1e-14 * A * C * W0, j
    # amplitude 0: nothing at all
    rc, g0, dg0 = run(driver, tmp_path, s, D, a=0.0)
    assert rc == 0 and not g0.any() and not dg0.any()


@pytest.mark.parametrize("D", [0.0, D_BURST], ids=["continuous", "burst"])
def test_dg_is_the_derivative_of_g(driver, tmp_path, D):
    """Central difference of g with step h against dg: the truncation error is h^2/6 max|g'''| <= h^2/6 A C (W0 + q)^3
    (g is a product of a window with frequencies <= q and a carrier of frequency W0), the rounding error
    2 eps A C / (2 h).  Points within h of a joint are left out: g is only C^1 there."""
    h = 1e-4 / F
    end = (D if D > 0 else 2 * LR) + LR
    s = np.linspace(-0.5 * LR, end, 997)
    joints = [0.0, LR] + ([D - LR, D] if D > 0 else [])
    s = s[np.all(np.abs(s[:, None] - np.array(joints)[None, :]) > 2 * h, axis=1)]
    _, gp, _ = run(driver, tmp_path, s + h, D)
    _, gm, _ = run(driver, tmp_path, s - h, D)
    _, _, dg = run(driver, tmp_path, s, D)
    q = np.pi * F / 4
    hh = ((s + h) - (s - h)) / 2
    bound = h * h / 6 * A * C * (W0 + q) ** 3 + 4 * 2.0 ** -52 * A * C / h
    assert np.all(np.abs((gp - gm) / (2 * hh) - dg) <= bound)
    assert bound < 1e-6 * A * C * W0 and np.abs(dg).max() > 0.9 * A * C * W0     # the check resolves dg


def test_default_source_closed_formulas(driver, tmp_path):
    """tau = 0, D = 0, a = 1: the reference's window and source, Linear.hpp:185-192 / Lossy.hpp:216-220."""
    t = np.linspace(0.0, 2.5 * LR, 801)
    rc, g, dg = run(driver, tmp_path, t, 0.0, a=1.0)
    assert rc == 0
    win = np.where(t < LR, 0.5 * (1.0 - np.cos(F * np.pi * t / 4.0)), 1.0)
    dwin = np.where(t < LR, 0.5 * np.pi * F / 4.0 * np.sin(F * np.pi * t / 4.0), 0.0)
    gref = win * SCALE * P0 * W0 / S0 * np.cos(W0 * t)
    dgref = dwin * SCALE * P0 * W0 / S0 * np.cos(W0 * t) - win * SCALE * P0 * W0 * W0 / S0 * np.sin(W0 * t)
    assert np.all(np.abs(g - gref) <= 1e-14 * C) and np.all(np.abs(dg - dgref) <= 1e-14 * C * W0)


def test_short_burst_is_refused(driver, tmp_path):
    s = np.array([0.5 * LR])
    assert run(driver, tmp_path, s, 2 * LR)[0] == 0                   # D = 2 Lr: the ramps just fit
    assert run(driver, tmp_path, s, np.nextafter(2 * LR, 0))[0] == 2
    assert run(driver, tmp_path, s, 0.5 * LR)[0] == 2
    with pytest.raises(ValueError):
        fsrc.waveform(s, F, P0, S0, duration=0.5 * LR)


def test_waveform_driver_clean_under_sanitizers(tmp_path):
    """The header's host code as a stand-alone program under AddressSanitizer + UBSan (never loaded into python)."""
    exe = _build(tmp_path, "source_wave_driver_san", ["-O1", "-g", "-fsanitize=address,undefined",
                                                       "-fno-sanitize-recover=all"])
    for D in (0.0, D_BURST):
        s, _ = grid(D)
        rc, g, dg = run(exe, tmp_path, s, D)
        assert rc == 0 and np.isfinite(g).all() and np.isfinite(dg).all()
    assert run(exe, tmp_path, np.array([1.0]), 0.5 * LR)[0] == 2


def test_focus_delays():
    rng = np.random.default_rng(5)
    for d in (2, 3):
        x = rng.uniform(-0.02, 0.02, (200, d))
        x[:, 0] = 0.0                                                   # a flat aperture
        focus = np.array([0.03, 0.004, -0.002][:d])
        c = 1500.0
        tau = fsrc.focus_delays(x, focus, c)
        assert tau.shape == (200,) and np.all(tau >= 0) and tau.min() == 0.0
        arrival = tau + np.linalg.norm(x - focus, axis=1) / c
        assert np.ptp(arrival) <= 4 * np.finfo(float).eps * arrival.max()
        assert np.ptp(tau) > 1e-7                                       # the aperture is really curved in time


def test_steer_delays():
    rng = np.random.default_rng(6)
    x = rng.uniform(-0.02, 0.02, (300, 3))
    n, c = np.array([1.0, 0.4, -0.2]), 1500.0
    tau = fsrc.steer_delays(x, n, c)
    assert np.all(tau >= 0) and tau.min() == 0.0
    # affine in x: a least-squares affine fit leaves nothing, and its gradient is n / (|n| c)
    Amat = np.hstack([x, np.ones((len(x), 1))])
    coef, *_ = np.linalg.lstsq(Amat, tau, rcond=None)
    assert np.abs(Amat @ coef - tau).max() <= 1e-12 * tau.max()
    assert np.allclose(coef[:3], n / np.linalg.norm(n) / c, rtol=1e-9)


def test_library_exports_set_source():
    """Fails before the feature exists: the C ABI has fus_model_set_source, the binding lists it, the wrappers exist."""
    from fenicsxfus_amd import _abi

    lib = ctypes.CDLL(_abi.LIB_PATH)
    assert hasattr(lib, "fus_model_set_source")
    assert "fus_model_set_source" in _abi.SYMBOLS
    assert lib.fus_version() == 1
    for cls in (fa.LinearSpectralExplicit, fa.LossySpectralExplicit, fa.WesterveltSpectralExplicit):
        assert callable(cls.set_source) and callable(cls.clear_source)
    with open(os.path.join(ROOT, "include", "fusmi.hpp")) as f:
        assert "set_source(" in f.read()


@pytest.mark.parametrize("name", ["3d", "2d"])
def test_stepper_reproduces_the_oracle_with_the_uniform_source(orc, name):
    """amp = 1, tau = 0, D = 0: the numpy stepper against orc.linear_rk4 / lossy_rk4 over 20 steps on every case of
    the GPU tests, 1e-12 relative (the same arithmetic in another order)."""
    cs = sr.case3d(orc) if name == "3d" else sr.case2d(orc)
    pr, t = cs.pr, cs.tdim
    p0 = 6e4
    vec, scale = cs.vectors("linear")
    for order in (4, 3, 2):
        u, v = np.zeros(pr.ndofs), np.zeros(pr.ndofs)
        orc.linear_rk4(t, pr.N, pr.dm, pr.G, pr.D, vec["lin"], vec["m"], vec["src"], vec["absb"], cs.f0, p0, S0, 0.0, 0.0,
                       cs.dt, u, v, order=order, steps=sr.NSTEPS)
        us, vs = sr.rk_stepper(pr, vec, scale, cs.f0, p0, 0.0, cs.dt, sr.NSTEPS, order=order)
        assert np.abs(u).max() > 0 and sr.rel(us, u) < 1e-12 and sr.rel(vs, v) < 1e-12, order
    if name == "3d":
        for forms in (0, 1):
            vec, scale = cs.vectors("lossy", forms)
            u, v = np.zeros(pr.ndofs), np.zeros(pr.ndofs)
            orc.lossy_rk4(t, pr.N, pr.dm, pr.G, pr.D, vec["lin"], vec["att"], vec["m"], vec["src"], vec["absb"],
                          vec["src2"], cs.f0, p0, S0, 0.0, 0.0, cs.dt, u, v, source_scale=scale, steps=sr.NSTEPS)
            us, vs = sr.rk_stepper(pr, vec, scale, cs.f0, p0, 0.0, cs.dt, sr.NSTEPS)
            assert np.abs(u).max() > 0 and sr.rel(us, u) < 1e-12 and sr.rel(vs, v) < 1e-12, forms


def test_aperture_inputs_are_what_the_issue_asks(orc):
    """amp in [0, 1.5] with exact zeros and live entries on the face, tau in [0, 3 / f], a period of 8-10 steps."""
    for cs in (sr.case3d(orc), sr.case2d(orc)):
        amp, tau = cs.aperture()
        a, t = amp[cs.face], tau[cs.face]
        assert a.min() == 0.0 and (a == 0).sum() >= 2 and 1.0 < a.max() <= 1.5
        assert t.min() >= 0 and t.max() <= 3.0 / cs.f0 and np.ptp(t) > 1.0 / cs.f0
        assert 8 <= 1.0 / (cs.f0 * cs.dt) <= 10
        assert len(cs.face) % 64 != 0
