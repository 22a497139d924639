"""The tile map of the batched k_stream_fused2 (BatchMapOf<RoundRobinMap>,
clay_amd/csrc/stream_tile_map.hpp) on the host: no GPU.

tests/host/fused2_batch_map_check.cpp includes the header the kernel uses and walks the map for
every sub-chunk size that is a multiple of 8 in [512, 4096] plus 16904 and 66184, for 2 / 3 / 17 /
34 / 70 stripes and 1 / 2 / 13 / 32 / 38 workgroups per XCD.  It checks that every byte of a row of
every stripe is owned by exactly one (workgroup, tile), that within a stripe the tiles are exactly
the one-stripe kernel's (region = ceil(sc / 8) rounded up to 64, nslots = min(per_xcd, region / 64),
64-byte tiles round robin over the slots), that the map's Walk equals tile(k), that 8 x G x nslots
workgroups are launched and none at or past that grid has a tile, and that every tile is one the
kernel can take.  With 32 workgroups per XCD it pins the shapes the GPU tests
(tests/test_gpu_decode_batch_fused2.py) are chosen for:

    sc x stripes  region  nslots  G   what it covers
    512 x 2       64      1       2   full tiles only
    520 x 34      128     2       16  groups run 2-3 stripes; XCD 4's tile is 8 bytes; XCDs 5-7 none
    2056 x 17     320     5       6   groups of 3, 3, 3, 3, 3, 2; XCD 6 ends in an 8-byte tile; XCD 7 none
    16904 x 3     2176    32      1   34 tiles per XCD: slots 0 and 1 run two tiles per stripe

If one of these facts does not hold the program says so, rather than the GPU tests silently covering
less.  The second test compiles the header alone as plain C++ with -Wall -Werror.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "fused2_batch_map_check.cpp")
INC = os.path.join(ROOT, "clay_amd", "csrc")


def _compiler():
    for cxx in (os.environ.get("CXX"), "c++", "g++", "clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        if cxx and shutil.which(cxx):
            return shutil.which(cxx)
    pytest.fail("no C++ compiler found (set CXX)")


def test_fused2_batch_map_owns_every_byte_once(tmp_path):
    exe = str(tmp_path / "fused2_batch_map_check")
    subprocess.run([_compiler(), "-std=c++17", "-O2", "-Wall", "-Werror", "-I", INC, "-o", exe, SRC], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert r.stdout.startswith("fused2 batch map ok:"), r.stdout[-2000:]


def test_round_robin_map_is_plain_cxx(tmp_path):
    """stream_tile_map.hpp with RoundRobinMap and its batch map: no HIP needed, no warnings."""
    src = tmp_path / "plain.cpp"
    src.write_text('#include "stream_tile_map.hpp"\n'
                   "int main() {\n"
                   "    const clay::bs::StreamCut cut = clay::bs::round_robin_cut(520, 32);\n"
                   "    const clay::bs::RoundRobinMap one(520, cut.region, cut.nslots, 4, 0);\n"
                   "    const clay::bs::BatchMapOf<clay::bs::RoundRobinMap> bm(520, cut.region, cut.nslots, 16, 34, 4, 2);\n"
                   "    const clay::bs::StreamTile t = bm.tile(2, 0, 0);\n"
                   "    return cut.region == 128 && cut.nslots == 2 && one.ntile() == 1 && bm.ntile() == 3 && t.stripe == 33 &&\n"
                   "                   t.b0 == 512 && t.vend == 520\n"
                   "               ? 0\n"
                   "               : 1;\n"
                   "}\n")
    exe = str(tmp_path / "plain")
    subprocess.run([_compiler(), "-std=c++17", "-O2", "-Wall", "-Werror", "-I", INC, "-o", exe, str(src)],
                   check=True)
    assert subprocess.run([exe], timeout=60).returncode == 0
