"""The batch tile map of k_stream_encode (BatchMap, clay_amd/csrc/stream_tile_map.hpp) on the host:
no GPU.

tests/host/stream_batch_map_check.cpp includes the header the kernel uses and walks the map for
every sub-chunk size that is a multiple of 8 in [16, 4096] plus 6560, 8200, 8216, 26216, 66176,
66184 and 419432, for 1 / 2 / 3 / 31 / 32 / 33 / 70 stripes and 1 / 2 / 13 / 32 / 38 workgroups per
XCD.  It checks that the tiles of all launched workgroups partition [0, sc) of every stripe exactly
once, that within a stripe they are exactly BalancedMap's for (sc, region, nsS), that each
workgroup's stripes are strictly ascending, that no workgroup at or past the grid has a tile, that
two groups' stripe counts differ by at most one, and the group shapes of a 256-CU device: sc 2048
gives 32 groups of 1, 2288 gives 16 of 2, 8216 gives 6 of 5 with 2 idle slots, 66176 gives 1 group
of 32 with two rounds.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "stream_batch_map_check.cpp")
INC = os.path.join(ROOT, "clay_amd", "csrc")


def _compiler():
    for cxx in (os.environ.get("CXX"), "c++", "g++", "clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        if cxx and shutil.which(cxx):
            return shutil.which(cxx)
    pytest.fail("no C++ compiler found (set CXX)")


def test_batch_tile_map_partitions_every_stripe(tmp_path):
    exe = str(tmp_path / "stream_batch_map_check")
    subprocess.run([_compiler(), "-std=c++17", "-O2", "-Wall", "-Werror", "-I", INC, "-o", exe, SRC], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert r.stdout.startswith("batch map ok:"), r.stdout[-2000:]
