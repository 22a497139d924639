"""What the sub-chunk sizes of tests/test_gpu_scrub_stream.py exercise in the streaming scrub: no GPU.

tests/host/stream_tile_dump.cpp includes the tile map the kernel uses (stream_tile_map.hpp) and
prints every workgroup's tiles; the XCD region and the workgroups per XCD are the host's
arithmetic (stream_cut, stream_tile_map.hpp) restated in tests/stream_cut.py, here for 32
workgroups per XCD.  A tile is
"ragged" when its width is no multiple of 16 (the plain compare path), "narrow" when it is below
256 (lanes past its end masked off).
"""
from collections import Counter

import pytest

from stream_cut import dump_tiles, stream_cut

SIZES = [16, 24, 264, 1064, 2048, 2288, 66176, 66184]
PER_XCD = 32


def _launch_shape(sc):
    return stream_cut(sc, PER_XCD)


@pytest.fixture(scope="module")
def tiles(tmp_path_factory):
    """sc -> list of (xcd, slot, round, b0, vend)"""
    return dump_tiles(tmp_path_factory.mktemp("tiles"), SIZES, PER_XCD)


def _widths(ts, xcd=None, rnd=None):
    return Counter(v - b for x, _, r, b, v in ts if (xcd is None or x == xcd) and (rnd is None or r == rnd))


@pytest.mark.parametrize("sc", SIZES)
def test_tiles_partition_the_row(tiles, sc):
    spans = sorted((b, v) for _, _, _, b, v in tiles[sc])
    assert spans[0][0] == 0 and spans[-1][1] == sc
    assert all(a[1] == b[0] for a, b in zip(spans, spans[1:]))
    assert all(b % 16 == 0 and 0 < v - b <= 256 for b, v in spans)
    # at most one ragged tile, and it holds the row end
    ragged = [(b, v) for b, v in spans if (v - b) % 16]
    assert ragged == ([spans[-1]] if sc % 16 else [])


def test_what_each_size_is_there_for(tiles):
    assert _launch_shape(16) == (32, 1) and tiles[16] == [(0, 0, 0, 0, 16)]  # seven empty XCDs
    assert tiles[24] == [(0, 0, 0, 0, 24)]  # one ragged tile
    # the smoke size: 64-byte DPP tiles and a ragged 8-byte one (no 16-byte compare in it)
    assert _launch_shape(264)[1] == 1 and _widths(tiles[264]) == {64: 4, 8: 1}
    # 160-byte DPP tiles plus a ragged 104-byte tile on XCD 6
    assert _launch_shape(1064) == (160, 1)
    assert [(x, v - b) for x, _, _, b, v in tiles[1064]] == [(x, 160) for x in range(6)] + [(6, 104)]
    # one full tile per XCD: no lane masked
    assert _launch_shape(2048) == (256, 1) and _widths(tiles[2048]) == {256: 8}
    # two slots per XCD, 144-byte tiles, the last clipped to 128; bytes 143 / 144 in two tiles
    assert _launch_shape(2288) == (288, 2)
    assert _widths(tiles[2288]) == {144: 15, 128: 1} and _widths(tiles[2288], xcd=7) == {144: 1, 128: 1}
    assert (0, 0, 0, 0, 144) in tiles[2288] and (0, 1, 0, 144, 288) in tiles[2288]
    for sc, last in ((66176, 224), (66184, 232)):
        assert _launch_shape(sc) == (8288, 32)
        for x in range(7):  # two rounds: 32 x 144, then 28 x 128 and a clipped 96: 61 tiles
            assert _widths(tiles[sc], xcd=x, rnd=0) == {144: 32}
            assert _widths(tiles[sc], xcd=x, rnd=1) == {128: 28, 96: 1}
            assert sum(_widths(tiles[sc], xcd=x).values()) == 61
        assert _widths(tiles[sc], xcd=7) == {256: 31, last: 1}  # one round, its end ragged for 66,184
        # round 0 of XCD 0 ends at byte 4,608, where slot 0's round-1 tile starts
        assert (0, 31, 0, 4464, 4608) in tiles[sc] and (0, 0, 1, 4608, 4736) in tiles[sc]
