"""The library's XCD cut (xcd_region, stream_cut and batch_groups, clay_amd/csrc/stream_tile_map.hpp)
against the tests' restatement (tests/stream_cut.py): no GPU.

tests/host/stream_cut_check.cpp prints the header's cut for every sub-chunk size that is a multiple
of 8 in [16, 4096] and the sizes the GPU tests and the gates' sweeps sit at, for 1, 2, 13, 32 and 38
workgroups per XCD, tiles of 256 and 512 bytes, and batches of 1, 2, 3, 33 and 70 stripes; every
line is compared with this side's arithmetic.  The tests that derive their shapes from
tests/stream_cut.py therefore run the shapes the library launches.
"""
import subprocess

import pytest

import stream_cut as cut

SIZES = list(range(16, 4097, 8)) + [6560, 8200, 8216, 26216, 66176, 66184, 262152, 419432]
PER_XCD = [1, 2, 13, 32, 38]
TILES = [256, 512]
STRIPES = [1, 2, 3, 33, 70]
PINNED = {16: (32, 1), 1064: (160, 1), 2048: (256, 1), 2288: (288, 2), 66176: (8288, 32)}  # 32 per XCD, 256-byte tiles


@pytest.fixture(scope="module")
def printed(tmp_path_factory):
    exe = cut.build_host(tmp_path_factory.mktemp("stream_cut"), "stream_cut_check")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    *lines, last = r.stdout.strip().split("\n")
    assert last == f"stream cut ok: {len(lines)} cases", last
    return [tuple(map(int, line.split())) for line in lines]


def test_header_cut_is_the_restated_cut(printed):
    want = []
    for sc in SIZES:
        for per_xcd in PER_XCD:
            for tile in TILES:
                region, ns = cut.stream_cut(sc, per_xcd, tile)
                assert region == cut.xcd_region(sc)
                want.append((sc, per_xcd, tile, region, ns, *(cut.batch_groups(per_xcd, ns, n) for n in STRIPES)))
    assert len(printed) == len(want) == len(SIZES) * len(PER_XCD) * len(TILES)
    diff = [(g, w) for g, w in zip(printed, want) if g != w]
    assert not diff, f"{len(diff)} lines differ, the first (header, restatement): {diff[0]}"


def test_pinned_shapes_on_256_cus(printed):
    got = {line[0]: line[3:5] for line in printed if line[1:3] == (32, 256)}
    for sc, shape in PINNED.items():
        assert got[sc] == shape and cut.stream_cut(sc, 32) == shape, (sc, got[sc], cut.stream_cut(sc, 32))
