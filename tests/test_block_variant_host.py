"""csrc/block_variant.hpp on the host (no device): the header through a plain C++ driver (a stand-alone program,
tests/cpp/block_variant_driver.cpp, built with -Wall -Wextra -Werror and once more under AddressSanitizer + UBSan) over
the whole input space, against tests/block_variant_ref.py -- the flag expressions and the launch cascade as fusmi.hip
held them before the header existed -- and against the properties the kernels themselves rely on."""
import itertools
import os
import subprocess

import pytest

import block_variant_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fenicsx-fus_amd", "csrc")
DRIVER = os.path.join(ROOT, "tests", "cpp", "block_variant_driver.cpp")
CXX = ["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", CSRC, DRIVER]
MODES = ((0, 0), (1, 1), (2, 2), (2, 1), (1, 2))   # (predicted, confirmed)


def _run(tmp, name, flags):
    exe = str(tmp / name)
    subprocess.check_call([*CXX, *flags, "-o", exe])
    return subprocess.run([exe], check=True, stdout=subprocess.PIPE, text=True).stdout.splitlines()


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("block_variant")
    plain = _run(tmp, "plain", ["-O1"])
    san = _run(tmp, "san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    assert plain == san
    return plain


def _space():
    return itertools.product(range(2, 11), (8, 4), (2, 3), (1, 2), MODES, (0, 1), (0, 1), (-1, 0, 1), (-1, 0, 1), (0, 1))


def _expected(flip=None):
    for P, nbytes, tdim, order, (pred, conf), ortho, det, mfma, pack32, dm in _space():
        d = ref.decide(P, nbytes, tdim, pred, conf, ortho, det, mfma, pack32, dm, flip)
        vs = []
        for OP in (ref.STIFFNESS, ref.MASS):
            for ST in ref.STAGES:
                v = d["variant"](OP, ST)
                vs.append("%d,%d,%d,%d,%d,%d" % (*v, int(ref.instantiated(P, nbytes, OP, ST, v))))
        yield "%d %d %d %d %d %d %d %d %d %d %d : %d %d : %d %d %d : %s" % (
            P, nbytes, tdim, order, pred, conf, ortho, det, mfma, pack32, dm, d["pk"], d["gcs_pred"], d["mfma"], d["diag"],
            d["gcs"], " ".join(vs))


def _mismatches(lines, flip=None):
    exp = list(_expected(flip))
    assert len(exp) == len(lines) == 9 * 2 * 2 * 2 * 5 * 2 * 2 * 3 * 3 * 2
    return [(a, b) for a, b in zip(lines, exp) if a != b]


def test_header_equals_the_former_expressions_and_cascade(lines):
    bad = _mismatches(lines)
    assert not bad, "%d lines differ, first (header, reference):\n%s\n%s" % (len(bad), *bad[0])


def test_a_flipped_rule_is_noticed(lines):
    """Negative control: a reference whose automatic pack32 choice also takes degree 6 on trilinear cells must disagree."""
    bad = _mismatches(lines, flip="pk_auto_p6")
    assert bad
    for got, _ in bad:   # ... and only where that rule decides
        f = got.split(" : ")[0].split()
        assert (f[0], f[1], f[4], f[9]) == ("6", "4", "2", "-1")


def test_properties_over_the_whole_space(lines):
    n = 0
    for line in lines:
        facts, pred, conf, variants = line.split(" : ")
        P, nbytes, tdim, order, mpred, mconf, ortho, det, mfma, pack32, dm = map(int, facts.split())
        layout_pk = int(pred.split()[0])
        vs = [tuple(map(int, v.split(","))) for v in variants.split()]
        assert len(vs) == 16
        for k, (geom, td, atomic, mf, pk, exists) in enumerate(vs):
            OP, ST = (ref.STIFFNESS, ref.MASS)[k // 8], ref.STAGES[k % 8]
            assert exists, line   # block_variant never names a kernel the library does not hold
            if pk:   # the kernel's own static_assert, and two exchange-tile slots in the layout
                assert nbytes == 4 and 5 <= P <= 7 and OP == ref.STIFFNESS and atomic == 1 and not mf, line
                assert geom in (ref.AFFINE, ref.TRILINEAR) and td == 3 and layout_pk == 1, line
            if mf:
                assert P in (6, 7) and OP == ref.STIFFNESS and (ST == ref.STAGE_NONE or ST >= 3) and atomic == 1, line
                assert geom in (ref.AFFINE, ref.TRILINEAR), line
            if geom == ref.DIAG:
                assert OP == ref.STIFFNESS and P <= 7 and mconf == ref.AFFINE, line
            if td == 2:
                assert geom == ref.STREAM, line
            assert td == tdim, line
            if P >= 8:
                assert not mf and not pk and geom != ref.DIAG, line
            if det:
                assert atomic == 0 and not mf and not pk, line
            else:
                assert atomic == 1, line
            n += 1
    assert n == 16 * len(lines)
