"""The tests' own restatement of the XCD cut of the streaming kernels, and the tile dump built on it.

The library cuts a row of sc bytes with xcd_region / stream_cut / batch_groups
(clay_amd/csrc/stream_tile_map.hpp).  The arithmetic is written out again here, on purpose without
reading it from the library or the header, so that the tests that derive their shapes from it do
not follow the library when it drifts; tests/test_stream_cut_cpu.py compares the two line by line.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "tests", "host")
INC = os.path.join(ROOT, "clay_amd", "csrc")


def xcd_region(sc):
    """Bytes of every row an XCD owns: sc / 8 rounded up to 32."""
    return ((sc + 7) // 8 + 31) // 32 * 32


def stream_cut(sc, per_xcd, tile=256):
    """(region, workgroups per XCD): one per tile of the region, from 1 to per_xcd."""
    region = xcd_region(sc)
    return region, min(per_xcd, max(1, (region + tile - 1) // tile))


def batch_groups(per_xcd, ns, n):
    """Groups of ns workgroups per XCD that a batch of n stripes runs side by side."""
    return min(max(1, per_xcd // ns), n)


def compiler():
    for cxx in (os.environ.get("CXX"), "c++", "g++", "clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        if cxx and shutil.which(cxx):
            return shutil.which(cxx)
    pytest.fail("no C++ compiler found (set CXX)")


def build_host(workdir, name):
    """tests/host/<name>.cpp compiled into `workdir`; the program's path."""
    exe = os.path.join(str(workdir), name)
    subprocess.run([compiler(), "-std=c++17", "-O2", "-Wall", "-Werror", "-I", INC, "-o", exe,
                    os.path.join(HOST, name + ".cpp")], check=True)
    return exe


def dump_tiles(workdir, sizes, per_xcd=32):
    """sc -> list of (xcd, slot, round, b0, vend): stream_tile_dump compiled into `workdir` and run
    on `sizes` at the cut of a device with per_xcd workgroups per XCD (also the tile boundaries of
    the flip sweeps, tests/scrub_sweeps.py)."""
    exe = build_host(workdir, "stream_tile_dump")
    args = []
    for sc in sizes:
        args += [str(sc), *map(str, stream_cut(sc, per_xcd))]
    r = subprocess.run([exe, *args], capture_output=True, text=True, timeout=60, check=True)
    out = {sc: [] for sc in sizes}
    for line in r.stdout.split("\n"):
        if line:
            sc, *t = map(int, line.split())
            out[sc].append(tuple(t))
    return out
