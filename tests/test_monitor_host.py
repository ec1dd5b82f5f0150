"""Host side of the field monitor (fusmi.h, fenicsxfus_amd/monitor.py): the C ABI carries the three entry points, and
the numpy helpers recover what they are defined to recover on synthetic signals.  No GPU."""
import os
import re

import numpy as np
import pytest

import fenicsxfus_amd as fa
from fenicsxfus_amd import _abi, monitor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMS = ("fus_model_monitor", "fus_model_monitor_get", "fus_model_monitor_info")


def test_library_and_header_carry_the_monitor():
    hdr = open(os.path.join(ROOT, "include", "fusmi.h")).read()
    declared = set(re.findall(r"\b(fus_[a-z0-9_]+)\s*\(", hdr))
    L = _abi.lib()
    for s in SYMS:
        assert s in declared and s in _abi.SYMBOLS and hasattr(L, s), s
    for i, name in enumerate(("MAX", "MIN", "MEAN", "RMS", "COS", "SIN")):
        assert re.search(rf"\bFUS_MON_{name}\s*=\s*{i}\b", hdr) and getattr(_abi, f"FUS_MON_{name}") == i
    assert L.fus_version() == 1
    assert fa.monitor is monitor


def test_null_model_is_an_argument_error():
    L = _abi.lib()
    assert L.fus_model_monitor(None, 0, 0, _abi.C.c_double(0.0), _abi.C.c_int64(0), 1, _abi.C.c_int64(0)) == -1
    assert L.fus_model_monitor_get(None, 0, 0, None, 0) == -1
    assert L.fus_model_monitor_info(None, None, None, None) == -1


def _signal(rng, ndof, nharm):
    mean = rng.standard_normal(ndof)
    cos = [rng.standard_normal(ndof) / k for k in range(1, nharm + 1)]
    sin = [rng.standard_normal(ndof) / k for k in range(1, nharm + 1)]
    return mean, cos, sin


def test_accumulation_over_two_periods_recovers_the_coefficients():
    """The monitor's definitions, accumulated directly in numpy over two whole periods of a signal built from known
    MEAN, COS_k, SIN_k: the coefficients come back to 1e-12 and reconstruct() returns the signal."""
    rng = np.random.default_rng(5)
    freq, nharm, ndof = 0.5e6, 3, 11
    mean, cos, sin = _signal(rng, ndof, nharm)
    dt, nsteps, skip, spp = monitor.whole_period_window(freq, 1.0 / freq / 23.5, 7.3 / freq, 2, nharm=nharm)
    assert spp == 24 and nsteps - skip == 2 * spp
    t, ts = 0.0, []
    for s in range(1, nsteps + 1):
        t += dt
        if s > skip:
            ts.append(t)
    ts = np.array(ts)
    n = len(ts)
    assert n == 2 * spp
    x = mean + sum(cos[k - 1] * np.cos(2 * np.pi * k * freq * ts[:, None])
                   + sin[k - 1] * np.sin(2 * np.pi * k * freq * ts[:, None]) for k in range(1, nharm + 1))
    assert np.abs(x.sum(axis=0) / n - mean).max() < 1e-12
    for k in range(1, nharm + 1):
        ck = 2.0 / n * (x * np.cos(2 * np.pi * k * freq * ts[:, None])).sum(axis=0)
        sk = 2.0 / n * (x * np.sin(2 * np.pi * k * freq * ts[:, None])).sum(axis=0)
        assert np.abs(ck - cos[k - 1]).max() < 1e-12 and np.abs(sk - sin[k - 1]).max() < 1e-12
        amp, ph = monitor.amplitude(ck, sk), monitor.phase(ck, sk)
        assert np.abs(amp * np.cos(ph) - cos[k - 1]).max() < 1e-12
        assert np.abs(amp * np.sin(ph) - sin[k - 1]).max() < 1e-12
    rms2 = mean**2 + 0.5 * sum(c**2 + s**2 for c, s in zip(cos, sin))       # Parseval over whole periods
    assert np.abs((x**2).sum(axis=0) / n - rms2).max() < 1e-12 * rms2.max()
    rec = monitor.reconstruct(mean, cos, sin, freq, ts)
    assert rec.shape == x.shape and np.abs(rec - x).max() < 1e-12
    one = monitor.reconstruct(mean, cos, sin, freq, ts[3])
    assert one.shape == mean.shape and np.abs(one - x[3]).max() < 1e-12


def test_amplitude_and_phase_take_functions():
    V = fa.FunctionSpace(fa.BoxMesh([0, 0, 0], [1, 1, 1], (1, 1, 1)), 2)
    c, s = fa.Function(V), fa.Function(V)
    c.x.array[:], s.x.array[:] = 3.0, -4.0
    assert np.allclose(monitor.amplitude(c, s), 5.0) and np.allclose(monitor.phase(c, s), np.arctan2(-4.0, 3.0))


@pytest.mark.parametrize("freq,dt_max,t_end,nper,every", [(10.0, 0.9 / 16 / 9, 1.8, 2, 1), (0.5e6, 3.35e-8, 2.4e-5, 3, 2),
                                                          (1.0, 0.25, 4.0, 2, 1), (7.0, 1.0 / 7 / 11.5, 1.0, 1, 3)])
def test_whole_period_window(freq, dt_max, t_end, nper, every):
    dt, nsteps, skip, spp = monitor.whole_period_window(freq, dt_max, t_end, nper, every=every, nharm=1)
    assert isinstance(spp, int) and isinstance(nsteps, int) and isinstance(skip, int)
    assert dt <= dt_max * (1 + 1e-14) and abs(spp * dt * freq - 1.0) < 1e-14      # a period is spp steps exactly
    assert spp == int(np.ceil(1.0 / freq / dt_max - 1e-9)) and spp % every == 0
    assert nsteps * dt >= t_end * (1 - 1e-12) and (nsteps - 1) * dt < t_end
    assert skip >= 0 and nsteps - skip == nper * spp


def test_whole_period_window_rejects_aliasing():
    # 8 steps per period: harmonics up to 3 are resolved (8 > 6), 4 is not (8 <= 8); sampling every 2nd step halves that
    assert monitor.whole_period_window(1.0, 1.0 / 8, 4.0, 2, nharm=3)[3] == 8
    with pytest.raises(ValueError, match="samples per period"):
        monitor.whole_period_window(1.0, 1.0 / 8, 4.0, 2, nharm=4)
    with pytest.raises(ValueError, match="samples per period"):
        monitor.whole_period_window(1.0, 1.0 / 8, 4.0, 2, every=2, nharm=2)
    assert monitor.whole_period_window(1.0, 1.0 / 8, 4.0, 2, every=2, nharm=1)[3] == 8
    with pytest.raises(ValueError, match="do not fit"):
        monitor.whole_period_window(1.0, 1.0 / 8, 1.5, 2)
    with pytest.raises(ValueError, match="does not divide"):
        monitor.whole_period_window(1.0, 1.0 / 8, 4.0, 2, every=3)
