"""The exchange-tile image of the re-mapped contractions (csrc/tile_index.hpp) on the host, under AddressSanitizer +
UBSan: a stand-alone driver (tests/cpp/tile_index_driver.cpp, its own main and process) checks for every N = 2..8 and
both scalar types that the image is injective over a slot and stays inside tile_slot_entries, that Layout::lds_bytes
covers the block kernel's LDS carve for blocks of the default size, of 17 elements and of one element, and that at
fp64 N = 5 the image in use costs no more under the bank model (csrc/tile_bank_model.hpp) than the linear image of
130-entry slots: 50 read and 85 store cycles per 15 accesses of each kind."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fenicsx-fus_amd", "csrc")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("san") / "tile_index_driver"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "tile_index_driver.cpp"),
                           os.path.join(CSRC, "layout.cpp"), "-o", str(exe)])
    return str(exe)


def test_tile_image_and_lds_reservation(driver):
    out = subprocess.run([driver], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("ok"), out.stdout + out.stderr
    r = dict(kv.split("=") for kv in out.stdout.split()[1:])
    assert int(r["checked"]) == 14                       # N = 2..8, fp32 and fp64
    assert int(r["read15"]) <= 50 and int(r["store15"]) <= 85
