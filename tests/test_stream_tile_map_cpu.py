"""The tile map of k_stream_encode (clay_amd/csrc/stream_tile_map.hpp) on the host: no GPU.

tests/host/stream_tile_map_check.cpp includes the header the kernel uses and walks the map for
every sub-chunk size that is a multiple of 8 up to 20000, sizes around whole rounds
(k * ns * 2048 +- {0, 8, 16, 24, 40}, k = 1..8), the benchmark's 419,432, and 1 / 2 / 13 / 32 / 38
workgroups per XCD.  It checks that the tiles of all XCDs and workgroups partition [0, sc) with no
gap or overlap, that tile starts are multiples of 16, widths at most 256 and multiples of 16 except
at a region's end, that no workgroup runs more passes than ceil(len / (ns * 256)), that the
workgroups of an XCD stream the same number of bytes to within one round width, and that the
benchmark shape gets five rounds of 240 bytes and two of 224 with at most 3 short or empty last
tiles per XCD.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "stream_tile_map_check.cpp")
INC = os.path.join(ROOT, "clay_amd", "csrc")


def _compiler():
    for cxx in (os.environ.get("CXX"), "c++", "g++", "clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        if cxx and shutil.which(cxx):
            return shutil.which(cxx)
    pytest.fail("no C++ compiler found (set CXX)")


def test_balanced_tile_map_partitions_every_row(tmp_path):
    exe = str(tmp_path / "stream_tile_map_check")
    subprocess.run([_compiler(), "-std=c++17", "-O2", "-Wall", "-Werror", "-I", INC, "-o", exe, SRC], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert r.stdout.startswith("tile map ok:"), r.stdout[-2000:]
