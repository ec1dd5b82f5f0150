"""The bioheat model on several ranks, host side (no device): the owner-mask header csrc/thermal_owner.hpp through a
plain C++ driver under AddressSanitizer + UBSan (a stand-alone program, tests/cpp/thermal_owner_driver.cpp), the parts
the device tests run on, the rule of the distributed start vector, and the ABI."""
import os
import re
import subprocess

import numpy as np
import pytest

import fenicsxfus_amd as fa
from fenicsxfus_amd import _abi
from thermal_multirank_util import Global, interface_ids, quadrant_parts, shape, slab_parts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fenicsx-fus_amd", "csrc")
DRIVER = os.path.join(ROOT, "tests", "cpp", "thermal_owner_driver.cpp")
NEW = ["fus_group_thermal_finish", "fus_group_thermal_steps", "fus_group_thermal_lambda_max", "fus_group_thermal_stable_dt"]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("owner") / "thermal_owner_driver")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-O1", "-g", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", CSRC, DRIVER, "-o", exe])
    return exe


def _drive(exe, path, parts, seed):
    rng = np.random.default_rng(seed)
    with open(path, "wb") as f:
        np.array([len(parts)], dtype=np.int64).tofile(f)
        for p in parts:
            n = len(p.gids)
            n_int = (n + 13 + 15) // 16 * 16
            np.array([n, n_int], dtype=np.int64).tofile(f)
            rng.permutation(n_int)[:n].astype(np.int32).tofile(f)      # injective into a padded internal range
            p.gids.astype(np.int64).tofile(f)
    out = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert out.returncode == 0 and out.stderr == "", out.stdout + out.stderr
    rows = [ln.split() for ln in out.stdout.splitlines()]
    assert rows[0][0] == "ok", out.stdout
    assert rows[1] == ["errors", "1", "2", "2", "1"], rows[1]      # index, no own value, empty list; mask untouched
    return [int(w) for w in rows[0][1:]]


def test_owner_mask_of_three_slabs_under_sanitizers(orc, driver, tmp_path):
    """Three x-slabs: every global DOF is owned exactly once and by its lowest sharer (the program checks both and
    fails otherwise); the counts it prints are the ones the slab layout gives: rank 0 owns all its DOFs, the others
    all but the plane they share with the rank below."""
    g = shape(orc, "S3")
    parts = slab_parts(g, 3)
    nglobal, nif, *owned = _drive(driver, tmp_path / "in.bin", parts, 5)
    plane = len(interface_ids(parts)[(0, 1)])
    assert nglobal == g.pr.ndofs and nif == 2 * plane and (0, 2) not in interface_ids(parts)
    assert owned == [len(parts[0].gids), len(parts[1].gids) - plane, len(parts[2].gids) - plane]


def test_owner_mask_of_four_quadrants_under_sanitizers(orc, driver, tmp_path):
    """The 2 x 2 partition with a line of DOFs held by all four ranks: owned once, by rank 0."""
    g = Global(orc, (4, 4, 3), 3, 0.1, np.float64, hi=[0.016, 0.016, 0.012])
    parts = quadrant_parts(g)
    four = set.intersection(*[set(p.gids.tolist()) for p in parts])
    assert len(four) == g.n[2] * g.P + 1
    nglobal, nif, *owned = _drive(driver, tmp_path / "in.bin", parts, 6)
    held = np.concatenate([p.gids for p in parts])
    assert nglobal == g.pr.ndofs == len(np.unique(held)) and sum(owned) == nglobal
    assert nif == int((np.bincount(held) > 1).sum())
    lower = [set().union(*[set(parts[q].gids.tolist()) for q in range(r)]) if r else set() for r in range(4)]
    assert owned == [len(set(p.gids.tolist()) - lower[r]) for r, p in enumerate(parts)]


def test_distributed_start_vector_rule(orc):
    """The documented start of the several-rank power iteration -- each rank's 1 + 0.5 sin(37 d + 1) over its OWN DOF
    numbers, added on the DOFs ranks share -- is positive everywhere and differs from the single-rank start, so a test
    that feeds it to the reference checks the rule and not the single-rank path."""
    g = shape(orc, "S3")
    top = g.ref.dense_lambda_max()
    for size in (2, 3):
        x0 = np.zeros(g.pr.ndofs)
        for p in slab_parts(g, size):
            x0[p.gids] += 1.0 + 0.5 * np.sin(37.0 * np.arange(len(p.gids)) + 1.0)
        assert x0.min() >= 0.5 and x0.max() <= 3.0 and x0.max() > 1.5
        assert np.abs(x0 - g.ref.start_vector()).max() > 0.1
        lam = g.ref.power_iteration(20, x0=x0)
        assert lam != g.rho20 and lam <= (1 + 1e-12) * top      # a Rayleigh quotient all the same


def test_abi_declares_the_group_calls():
    hdr = open(os.path.join(ROOT, "include", "fusmi.h")).read()
    declared = set(re.findall(r"\b(fus_[a-z0-9_]+)\s*\(", hdr))
    L = _abi.lib()
    for s in NEW:
        assert s in declared and s in _abi.SYMBOLS and hasattr(L, s), s
    for name in ("group_thermal_finish", "group_thermal_steps", "group_thermal_lambda_max", "group_thermal_stable_dt"):
        assert callable(getattr(fa, name))
    assert "Several ranks are not supported" not in fa.BioheatSpectralExplicit.__doc__
