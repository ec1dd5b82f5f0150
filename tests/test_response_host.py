"""Perfusion response and damage of the bioheat model, host side (no device): the numpy reference of tests/response_ref.py
against closed forms, the laws of csrc/thermal_response.hpp and its argument checks through a plain C++ driver under
AddressSanitizer + UBSan (a stand-alone program), thermal.py's numpy restatements, and the ABI -- before anything on the
device is compared with them (test_gpu_thermal_response.py)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from fenicsxfus_amd import _abi
from fenicsxfus_amd.thermal import arrhenius_rate, perfusion_factor
from response_ref import HENRIQUES, KNOTS, BioheatResponse, Response, damage, rate
from thermal_ref import TISSUE, box_hi
from util import Problem

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fenicsx-fus_amd", "csrc")
DRIVER = os.path.join(ROOT, "tests", "cpp", "thermal_response_driver.cpp")
NEW = ["fus_thermal_set_response", "fus_thermal_set_damage"]
EPS = 2.0 ** -53


# ---- closed forms -------------------------------------------------------------------------------------------------------
def test_uniform_decay_follows_the_start_states_phi(orc):
    """k = 0, uniform coefficients and fields, no heat: f = -(W phi / rho C) theta with phi of the state the step starts
    from, so one RK4 step multiplies theta by RK4's polynomial R(-dt W phi / rho C).  theta = 2 at t_base = 37 lies
    half-way up the first segment of KNOTS: phi = 2.5.  The next step starts from another temperature and takes its phi."""
    pr = Problem(orc, (3, 2, 2), 3, hi=box_hi((3, 2, 2)), perturb=0.1)
    W, rc = 4e5, TISSUE["rho_c"]
    ref = BioheatResponse(pr, 0.0, rc, W, t_base=37.0, response=Response(*KNOTS))
    dt = 0.5
    R = lambda z: 1 + z + z**2 / 2 + z**3 / 6 + z**4 / 24   # noqa: E731
    th0 = np.full(pr.ndofs, 2.0)
    th1 = ref.step(th0, dt)
    want1 = 2.0 * R(-dt * W * 2.5 / rc)
    assert np.abs(th1 - want1).max() <= 1e-13
    phi1 = 1.0 + 3.0 * (want1 / 4.0)
    th2 = ref.step(th1, dt)
    assert np.abs(th2 - want1 * R(-dt * W * phi1 / rc)).max() <= 1e-13
    # and the check can fail: the passive model decays more slowly
    passive = BioheatResponse(pr, 0.0, rc, W).step(th0, dt)
    assert np.abs(passive - 2.0 * R(-dt * W / rc)).max() <= 1e-13 and passive.min() - th1.max() > 1e-2
    # a dose above dose_hi shuts the perfusion: nothing is left of f
    ref = BioheatResponse(pr, 0.0, rc, W, response=Response(*KNOTS, dose_lo=1.0, dose_hi=2.0))
    ref.reset(D=np.full(pr.ndofs, 3.0))
    assert np.array_equal(ref.step(th0, dt), th0)


def test_rkl2_freezes_phi_too(orc):
    """The same decay through RKL2: theta is multiplied by the scheme's own polynomial of -dt W phi / rho C."""
    import sts_ref
    pr = Problem(orc, (3, 2, 2), 3, hi=box_hi((3, 2, 2)), perturb=0.1)
    W, rc, dt = 4e5, TISSUE["rho_c"], 0.5
    ref = BioheatResponse(pr, 0.0, rc, W, response=Response(*KNOTS))
    for s in (2, 8):
        ref.reset()
        th = ref.sts_step(np.full(pr.ndofs, 2.0), dt, s)
        assert np.abs(th - 2.0 * sts_ref.polynomial(s, -dt * W * 2.5 / rc)).max() <= 1e-13


def test_P_hits_every_knot_and_is_constant_outside():
    temps, factors = (30.0, 37.0, 41.0, 41.5, 60.0), (0.5, 1.0, 4.0, 0.25, 3.0)
    r = Response(temps, factors)
    assert np.array_equal(r.P(np.array(temps)), np.array(factors))
    assert np.array_equal(r.P(np.array([-300.0, 29.999, 60.001, 1e4])), np.array([0.5, 0.5, 3.0, 3.0]))
    assert np.array_equal(r.P(np.array([39.0, 41.25, 50.75])), np.array([2.5, 2.125, 0.25 + 2.75 * 0.5]))
    assert r.phi_max == 4.0 and Response().phi_max == 1.0
    assert np.array_equal(Response().P(np.array([10.0, 90.0])), np.ones(2))
    assert np.array_equal(Response((40.0,), (3.0,)).P(np.array([10.0, 40.0, 90.0])), np.full(3, 3.0))


def test_S_at_its_ends_and_midpoint():
    r = Response(dose_lo=10.0, dose_hi=250.0)
    assert np.array_equal(r.S(np.array([0.0, 10.0, 130.0, 250.0, 1e9])), np.array([1.0, 1.0, 0.5, 0.0, 0.0]))
    step = Response(dose_lo=240.0, dose_hi=240.0)
    assert np.array_equal(step.S(np.array([0.0, 240.0, np.nextafter(240.0, 1e3), 1e3])), np.array([1.0, 1.0, 0.0, 0.0]))
    assert np.array_equal(Response(dose_lo=5.0, dose_hi=0.0).S(np.array([0.0, 1e9])), np.ones(2))      # no shutdown
    assert np.array_equal(Response(*KNOTS, 10.0, 250.0).phi(np.array([39.0, 45.0]), np.array([130.0, 0.0])),
                          np.array([1.25, 4.0]))


def test_damage_of_a_constant_temperature():
    """Omega of a constant temperature is n dt r(T) (the additions round: n ulps), and r is Henriques' rate: Omega = 1
    after about a second at 60 degrees C."""
    A, Ea = HENRIQUES["A"], HENRIQUES["Ea"]
    n, dt, th = 9, 0.25, np.array([13.0, 23.0, 28.0])
    om = damage([th] * (n + 1), dt, 37.0, A, Ea)
    want = n * dt * rate(37.0 + th, A, Ea)
    assert np.abs(om - want).max() <= n * EPS * want.max() and (om > 0).all()
    assert 0.1 < rate(60.0, A, Ea) < 10.0 and rate(43.0, A, Ea) < 1e-3 * rate(60.0, A, Ea)
    ref_rate = A * np.exp(-Ea / (8.314462618 * (37.0 + th + 273.15)))
    assert np.abs(rate(37.0 + th, A, Ea) / ref_rate - 1.0).max() <= 1e-12


def test_numpy_restatements_match_the_reference():
    """thermal.py's perfusion_factor and arrhenius_rate against the reference's own statement, bit for bit."""
    rng = np.random.default_rng(5)
    T, D = rng.uniform(30.0, 70.0, 4000), rng.uniform(0.0, 300.0, 4000)
    T[:5] = (37.0, 41.0, 45.0, 30.0, 70.0)
    D[:3] = (10.0, 250.0, 130.0)
    for knots in (None, KNOTS, ((30.0, 37.0, 41.0, 41.5, 60.0), (0.5, 1.0, 4.0, 0.25, 3.0)), ((40.0,), (3.0,))):
        for rng_ in (None, (10.0, 250.0), (240.0, 240.0), (5.0, 0.0)):
            r = Response(*(knots or ((), ())), *(rng_ or (0.0, 0.0)))
            got = perfusion_factor(T, D, *(knots or (None, None)), dose_range=rng_)
            assert np.array_equal(got, r.phi(T, D)), (knots, rng_)
    assert np.array_equal(arrhenius_rate(T, **HENRIQUES), rate(T, **HENRIQUES))


def test_power_iteration_takes_phi_max(orc):
    """The step rule's operator carries phi_max m_W: with phi_max = 4 the quotient grows, with factors <= 1 it does not,
    and steps at 2 / rho_20 of the passive operator blow up under a strong response where the rule's own step holds."""
    pr = Problem(orc, (3, 2, 2), 3, hi=box_hi((3, 2, 2)), perturb=0.1)
    args = (pr, TISSUE["k"], TISSUE["rho_c"], 4e5)
    passive = BioheatResponse(*args).power_iteration(20)
    up = BioheatResponse(*args, response=Response(*KNOTS)).power_iteration(20)
    down = BioheatResponse(*args, response=Response((37.0, 45.0), (1.0, 0.25))).power_iteration(20)
    assert up > passive >= down
    strong = Response((37.0, 38.0), (1.0, 4000.0))
    ref = BioheatResponse(*args, response=strong)
    th0 = np.full(pr.ndofs, 5.0)
    bad = ref.advance(th0, 2.0 / passive, 20)[0][-1]
    good = ref.advance(th0, 2.0 / ref.power_iteration(20), 20)[0][-1]
    assert np.abs(bad).max() > 1e10 and np.abs(good).max() <= 5.0


# ---- the ABI ------------------------------------------------------------------------------------------------------------
def test_abi_declares_and_exports_the_response_symbols():
    hdr = open(os.path.join(ROOT, "include", "fusmi.h")).read()
    declared = set(re.findall(r"\b(fus_[a-z0-9_]+)\s*\(", hdr))
    L = _abi.lib()
    for s in NEW:
        assert s in declared and s in _abi.SYMBOLS and hasattr(L, s), s
    assert (_abi.FUS_TH_DAMAGE, _abi.FUS_TH_PERFUSION) == (3, 4)
    assert re.search(r"FUS_TH_DAMAGE = 3, FUS_TH_PERFUSION = 4", hdr)
    # null handles are refused before any device call
    assert L.fus_thermal_set_response(None, 0, None, None, C.c_double(0.0), C.c_double(0.0)) == -1
    assert b"null" in L.fus_last_error()
    assert L.fus_thermal_set_damage(None, C.c_double(1.0), C.c_double(1.0)) == -1
    assert b"null" in L.fus_last_error()


def test_cpp_example_compiles(tmp_path):
    """examples/cpp_bioheat_response.cpp against include/fusmi.hpp (compile and link only; it runs in the GPU tests)."""
    libdir = os.path.join(ROOT, "fenicsx-fus_amd", "fenicsxfus_amd")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "cpp_bioheat_response.cpp"), "-L", libdir, "-lfusmi",
                           f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib", "-o", str(tmp_path / "cpp_bioheat_response")])


# ---- the header under sanitizers ----------------------------------------------------------------------------------------
def _drive(exe, path, temps, factors, dose, dmg, T, D, arrays=True, nknots=None):
    temps, factors = np.asarray(temps, dtype=np.float64), np.asarray(factors, dtype=np.float64)
    with open(path, "wb") as f:
        np.array([len(temps) if nknots is None else nknots, int(arrays), len(T)], dtype=np.int64).tofile(f)
        np.array([*dose, *dmg], dtype=np.float64).tofile(f)
        if arrays:
            temps.tofile(f), factors.tofile(f)
        np.asarray(T, dtype=np.float64).tofile(f), np.asarray(D, dtype=np.float64).tofile(f)
    out = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert out.returncode == 0 and out.stderr == "", out.stdout + out.stderr
    rows = [ln.split() for ln in out.stdout.splitlines()]
    res, i = {}, 0
    for key in ("err", "derr"):
        assert rows[i][0] == key
        res[key] = int(rows[i][1])
        head = rows[i + 1]
        i += 2
        if res[key]:
            assert head[:2] == ["untouched", "1"], head
            res[key + "_message"] = " ".join(head[3:])
            continue
        res[key + "_head"] = {k: (float.fromhex(v) if "x" in v else int(v)) for k, v in zip(head[::2], head[1::2])}
        tag = "V" if key == "err" else "R"
        vals = []
        while i < len(rows) and rows[i][0] == tag:
            vals.append([float.fromhex(w) for w in rows[i][1:]])
            i += 1
        res[tag] = np.array(vals)
    return res


def test_laws_and_argument_checks_under_sanitizers(tmp_path):
    """csrc/thermal_response.hpp as a stand-alone program under AddressSanitizer + UBSan (never loaded into python): P, S
    and r equal the reference's bit for bit (r: within an ulp of exp, the C library's against numpy's) -- at every knot,
    at both ends of the dose range and at random points -- for 0, 1, 3, 5 and 8 knots; every argument error named in
    fusmi.h is reported and leaves the struct untouched."""
    exe = str(tmp_path / "thermal_response_driver")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-O1", "-g", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", CSRC, DRIVER, "-o", exe])
    path = tmp_path / "in.bin"
    rng = np.random.default_rng(11)
    A, Ea = HENRIQUES["A"], HENRIQUES["Ea"]
    eight = (np.linspace(35.0, 63.0, 8), np.array([1.0, 1.5, 4.0, 4.0, 2.0, 0.0, 0.5, 0.25]))
    for knots in (((), ()), ((40.0,), (3.0,)), KNOTS, ((30.0, 37.0, 41.0, 41.5, 60.0), (0.5, 1.0, 4.0, 0.25, 3.0)), eight):
        for dose in ((0.0, 0.0), (10.0, 250.0), (240.0, 240.0), (0.0, 7.0), (5.0, -1.0)):
            T = np.concatenate([rng.uniform(20.0, 80.0, 300), np.asarray(knots[0], dtype=np.float64), [-400.0, 1e5]])
            D = np.concatenate([rng.uniform(0.0, 300.0, len(T) - 6), [0.0, 10.0, 250.0, 240.0, 7.0, 1e12]])
            got = _drive(exe, path, *knots, dose, (A, Ea), T, D)
            r = Response(*knots, *dose)
            assert got["err"] == 0 and got["derr"] == 0
            assert got["err_head"] == dict(active=int(len(knots[0]) > 0 or dose[1] > 0), nknots=len(knots[0]),
                                           phi_max=r.phi_max)
            assert np.array_equal(got["V"][:, 0], r.P(T)) and np.array_equal(got["V"][:, 1], r.S(D))
            assert got["derr_head"] == dict(on=1, lnA=float(np.log(A)))
            want = rate(T, A, Ea)
            ok = T > -200.0
            assert np.abs(got["R"][ok, 0] - want[ok]).max() <= 2 * EPS * want[ok].max()
            assert (np.abs(got["R"][ok, 0] - want[ok]) <= 4 * EPS * want[ok]).all()
    # the argument errors
    pts = ([40.0], [1.0])
    bad = lambda **kw: _drive(exe, path, *kw.pop("knots", KNOTS), kw.pop("dose", (0.0, 0.0)), kw.pop("dmg", (A, Ea)), *pts, **kw)   # noqa: E731
    assert bad(nknots=9, knots=(np.arange(9.0), np.ones(9)))["err"] == 1
    assert bad(nknots=-1)["err"] == 1
    assert bad(arrays=False, nknots=2)["err"] == 1
    for t in ((37.0, 37.0, 45.0), (37.0, 36.0, 45.0), (37.0, np.nan, 45.0), (37.0, 41.0, np.inf)):
        assert bad(knots=(t, KNOTS[1]))["err"] == 2, t
    for fct in ((1.0, -0.5, 4.0), (1.0, np.nan, 4.0), (np.inf, 1.0, 4.0)):
        assert bad(knots=(KNOTS[0], fct))["err"] == 3, fct
    for dose in ((-1.0, 5.0), (6.0, 5.0), (np.nan, 5.0), (0.0, np.inf), (0.0, np.nan)):
        assert bad(dose=dose)["err"] == 4, dose
    assert bad(dose=(np.nan, 0.0))["err"] == 0                    # dose_hi <= 0: dose_lo is never read
    assert "strictly ascending" in bad(knots=((2.0, 1.0), (1.0, 1.0)))["err_message"]
    for dmg in ((-1.0, Ea), (np.nan, Ea), (np.inf, Ea), (A, 0.0), (A, -Ea), (A, np.nan), (A, np.inf)):
        assert bad(dmg=dmg)["derr"] == 5, dmg
    off = bad(dmg=(0.0, 0.0))
    assert off["derr"] == 0 and off["derr_head"]["on"] == 0 and len(off["R"]) == 0
