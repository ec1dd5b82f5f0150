"""csrc/block_variant.hpp on the host (no device): whether every block of a layout fits the unrolled first batches of the
straight-line block kernel, and the WALK argument that follows from it.  The header goes through a plain C++ driver (a
stand-alone program, tests/cpp/block_fits_driver.cpp, built with -Wall -Wextra -Werror and once more under
AddressSanitizer + UBSan); the driver prints the capacities it sees and its decisions around every capacity edge, and
the decisions are recomputed here from the extents alone."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fenicsx-fus_amd", "csrc")
DRIVER = os.path.join(ROOT, "tests", "cpp", "block_fits_driver.cpp")
CXX = ["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", CSRC, DRIVER]

# What one thread moves in the first batches at the degrees 2-4, as the kernels have had them since the batches were
# sized (interior 16-byte vectors, shared dofs, 16-byte dofmap vectors); the two-range stage update of one input.
FIRST_BATCHES = {2: (3, 4, 2), 3: (3, 4, 2), 4: (2, 3, 1)}


def _run(tmp, name, flags):
    exe = str(tmp / name)
    subprocess.check_call([*CXX, *flags, "-o", exe])
    return subprocess.run([exe], check=True, stdout=subprocess.PIPE, text=True).stdout.splitlines()


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("block_fits")
    plain = _run(tmp, "plain", ["-O1"])
    san = _run(tmp, "san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    assert plain == san
    return plain


@pytest.fixture(scope="module")
def caps(lines):
    out = {}
    for ln in lines:
        if ln.startswith("caps "):
            key, val = ln[5:].split(" : ")
            out[tuple(map(int, key.split()))] = dict(zip(("ui", "us", "ul", "gc", "gc_all", "cf", "epi"), map(int, val.split())))
    return out


def _cases(lines):
    for ln in lines:
        if ln.startswith("case "):
            ext, fits, walk = ln[5:].split(" : ")
            yield ln, tuple(map(int, ext.split())), tuple(map(int, fits.split())), tuple(map(int, walk.split()))


def _fits(c, P, gcs, nthr, nint, nsh, nelem, nd):
    """Nothing is left for a loop: every batch of `c` per thread times nthr threads holds the largest block's share."""
    nvec, n16 = nint // 2, (nelem * nd * 2 + 15) // 16
    return (nthr > 0 and nvec <= c["ui"] * nthr and (c["epi"] == 0 or nvec <= c["epi"] * nthr) and nsh <= c["us"] * nthr
            and n16 <= c["ul"] * nthr and (not c["gc_all"] or nelem * gcs <= c["gc"] * nthr) and nelem <= c["cf"] * nthr
            and (P + 1) ** 2 + 2 * (P + 1) <= nthr)


def test_capacities_are_the_kernels(caps):
    assert len(caps) == 9 * 3 * 2
    for (P, gcs, nf), c in caps.items():
        if P in FIRST_BATCHES:
            assert (c["ui"], c["us"], c["ul"]) == FIRST_BATCHES[P]
            assert c["epi"] == (2 if nf == 1 else 0)
        else:
            assert c["epi"] == 0   # the higher degrees keep their own epilogue forms and loops
        assert c["gc"] == (2 if gcs > 7 else 1) and c["cf"] == 1 and c["gc_all"] == (P == 4)
    # ... and the kernel takes them from the header: no second definition in kernels.hpp
    src = open(os.path.join(CSRC, "kernels.hpp")).read()
    assert re.search(r"constexpr BlockCaps CAPS = block_caps\(P, GCS, NF\);", src)
    assert re.search(r"constexpr int UI = CAPS\.ui, US = CAPS\.us, UL = CAPS\.ul;", src)
    assert "CAPS.epi" in src and "CAPS.gc" in src and "CAPS.cf" in src
    assert not re.search(r"#define FUS_UI_(P7|HI)", src)
    assert not re.search(r"constexpr int (UI|US|UL|EPIU) = \(?\(?P ", src)
    assert "straight_needs_fit(P, (int)sizeof(T), GEOM)" in src


def test_walk_0_exactly_when_every_block_fits(lines, caps):
    n = seen_fit = seen_unfit = 0
    for ln, (P, gcs, nthr, nint, nsh, nelem, nd), (fits1, fits2, tfits), (w1, w2, w1short, wstream) in _cases(lines):
        e1 = _fits(caps[P, gcs, 1], P, gcs, nthr, nint, nsh, nelem, nd)
        e2 = _fits(caps[P, gcs, 2], P, gcs, nthr, nint, nsh, nelem, nd)
        assert (fits1, fits2) == (int(e1), int(e2)), ln
        assert tfits == int(e1) | (int(e2) << 1), ln
        assert (w1, w2) == (0 if e1 else 1, 0 if e2 else 1), ln
        assert w1short == 1 and wstream == 1, ln   # fewer workgroups than blocks; the streamed kernels: the block loop
        seen_fit += e1
        seen_unfit += not e1
        n += 1
    assert n >= 3 * 3 * 3 * 28 and seen_fit > n // 4 and seen_unfit > n // 4


def test_every_limit_decides_alone(lines, caps):
    """Each of the limits is seen exactly fitting (WALK = 0) and one over (WALK = 1) with everything else far from its own."""
    edges = {k: set() for k in ("nint", "nsh", "gc", "cf", "ldm")}
    for ln, (P, gcs, nthr, nint, nsh, nelem, nd), (fits1, _, _), (w1, _, _, _) in _cases(lines):
        c = caps[P, gcs, 1]
        if nthr < 64:
            continue
        small = dict(nint=nint <= 8, nsh=nsh <= 8, ne=nelem <= 1, nd=nd <= 1)
        lim = min(c["ui"], c["epi"]) * nthr

        def only(*free):
            return all(v for k, v in small.items() if k not in free)

        for over in (0, 1):
            if only("nint") and nint // 2 == lim + over:
                edges["nint"].add((over, w1))
            if only("nsh") and nsh == c["us"] * nthr + over:
                edges["nsh"].add((over, w1))
            if gcs and c["gc_all"] and only("ne") and nelem == c["gc"] * nthr // gcs + over:
                edges["gc"].add((over, w1))
            if not (gcs and c["gc_all"]) and only("ne") and nelem == c["cf"] * nthr + over:
                edges["cf"].add((over, w1))
            if only("nd") and nelem == 1 and (nd * 2 + 15) // 16 == c["ul"] * nthr + over:
                edges["ldm"].add((over, w1))
    for name, seen in edges.items():
        assert seen == {(0, 0), (1, 1)}, (name, seen)


def test_the_headline_block_fits(lines, caps):
    """32 elements of degree 4 on 512 threads, 1575 interior and 1026 shared dofs, 21 geometry numbers per cell."""
    c = caps[4, 21, 1]
    assert _fits(c, 4, 21, 512, 1575, 1026, 32, 125)
    assert not _fits(c, 4, 21, 256, 1575, 1026, 32, 125)
    # the default blocks of the degrees 2 and 3 (64 and 32 elements, 256 threads) hold 1344 and 672 geometry numbers:
    # more than the first two batches, and they fit all the same -- those kernels keep that one loop
    assert _fits(caps[2, 21, 1], 2, 21, 256, 729, 400, 64, 27)
    assert _fits(caps[3, 21, 1], 3, 21, 256, 900, 600, 32, 64)
