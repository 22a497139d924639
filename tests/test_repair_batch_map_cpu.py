"""The column map of the batch k_bs_repair (clay_amd/csrc/repair_batch_map.hpp) on the host: no GPU.

tests/host/repair_batch_map_check.cpp includes the header the kernel uses and walks the map as the
kernel does for 64, 9 and 4 lanes per plane layer (the (4,2,5), (9,3,11) and (10,4,13) kernels),
sub-chunk sizes 1..300, 2048 +- {0, 5, 8} and 4101, and 1..70 and 300 stripes.  It checks that every
byte of every stripe is owned by exactly one (tile, lane), that a lane's valid byte count is in
0..32, that the full-tile predicate (the unmasked kernel variant) holds only where every lane has 32
valid bytes, that every tile is run by exactly one workgroup of the XCD-contiguous launch order,
and that the tile count matches the launcher's formula.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "repair_batch_map_check.cpp")
INC = os.path.join(ROOT, "clay_amd", "csrc")


def _compiler():
    for cxx in (os.environ.get("CXX"), "c++", "g++", "clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        if cxx and shutil.which(cxx):
            return shutil.which(cxx)
    pytest.fail("no C++ compiler found (set CXX)")


def test_column_map_owns_every_byte_once(tmp_path):
    exe = str(tmp_path / "repair_batch_map_check")
    subprocess.run([_compiler(), "-std=c++17", "-O2", "-Wall", "-Werror", "-I", INC, "-o", exe, SRC], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert r.stdout.startswith("repair batch map ok:"), r.stdout[-2000:]
