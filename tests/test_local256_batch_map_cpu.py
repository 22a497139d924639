"""The tile map of the batched k_stream_local256 (BatchMapOf<StreamMap>,
clay_amd/csrc/stream_tile_map.hpp) on the host: no GPU.

tests/host/local256_batch_map_check.cpp includes the header the kernel uses and walks the map for
every sub-chunk size that is a multiple of 8 in [512, 4096] plus 8216, 66176, 66184 and 419432, for
2 / 3 / 31 / 32 / 33 / 70 stripes and 1 / 2 / 13 / 32 / 38 workgroups per XCD.  It checks that the
tiles of all launched workgroups partition [0, sc) of every stripe exactly once, that within a
stripe they are exactly StreamMap's for (sc, region, nsS) -- the cut of the one-stripe kernel --,
that each workgroup's stripes are strictly ascending, that no workgroup at or past the grid has a
tile, that two groups' stripe counts differ by at most one, that every tile is one the kernel can
take, and the shapes of a 256-CU device (32 workgroups per XCD):

    sc      nsS  groups  tiles of one stripe                      tile with the row's 8-byte tail
    512     1    32      8 partial                                none
    520     1    32      6 partial, 2 empty XCDs                  [480, 520)
    2048    1    32      8 full                                   none
    2056    2    16      16 partial                               [2048, 2056)
    2288    2    16      partial only                             none
    8216    5    6       partial only, 2 idle slots per XCD       [8160, 8216)
    66184   32   1       up to two per workgroup, full first      [65952, 66184)

The loader and the compute waves of a workgroup count their tiles with ntile() of this one map, so
they agree on it by construction; the walk shows that the count is the concatenation of one-stripe
sequences.  The loader takes tile k with tile(k), the compute waves with the map's division-free
Walk: the program checks that both give the same tile, in the same order, for every workgroup.

The second test compiles the header alone, StreamMap included, as plain C++ with -Wall -Werror.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "local256_batch_map_check.cpp")
INC = os.path.join(ROOT, "clay_amd", "csrc")


def _compiler():
    for cxx in (os.environ.get("CXX"), "c++", "g++", "clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        if cxx and shutil.which(cxx):
            return shutil.which(cxx)
    pytest.fail("no C++ compiler found (set CXX)")


def test_local256_batch_map_partitions_every_stripe(tmp_path):
    exe = str(tmp_path / "local256_batch_map_check")
    subprocess.run([_compiler(), "-std=c++17", "-O2", "-Wall", "-Werror", "-I", INC, "-o", exe, SRC], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert r.stdout.startswith("local256 batch map ok:"), r.stdout[-2000:]


def test_tile_map_header_is_plain_cxx(tmp_path):
    """stream_tile_map.hpp with StreamMap and the generic batch map: no HIP needed, no warnings."""
    src = tmp_path / "plain.cpp"
    src.write_text('#include "stream_tile_map.hpp"\n'
                   "int main() {\n"
                   "    const clay::bs::StreamCut cut = clay::bs::stream_cut(2056, 32);\n"
                   "    const clay::bs::StreamMap one(2056, cut.region, cut.nslots, 7, 1);\n"
                   "    const clay::bs::BatchMapOf<clay::bs::StreamMap> bm(2056, cut.region, cut.nslots, 16, 17, 7, 1);\n"
                   "    const clay::bs::BatchMap enc(2056, cut.region, cut.nslots, 16, 17, 7, 1);\n"
                   "    const clay::bs::StreamTile t = bm.tile(1, 0, 0);\n"
                   "    return one.ntile() == 1 && bm.ntile() == 2 && enc.ntile() == 2 && t.stripe == 16 && t.b0 == 2048 &&\n"
                   "                   t.vend == 2056\n"
                   "               ? 0\n"
                   "               : 1;\n"
                   "}\n")
    exe = str(tmp_path / "plain")
    subprocess.run([_compiler(), "-std=c++17", "-O2", "-Wall", "-Werror", "-I", INC, "-o", exe, str(src)],
                   check=True)
    assert subprocess.run([exe], timeout=60).returncode == 0
