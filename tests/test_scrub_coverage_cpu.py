"""The flip schedules of the exhaustive scrub tests (tests/scrub_sweeps.py), without a GPU.

A schedule that skipped bytes would defeat the sweeps, so: the (slab, pass, stripe) -> (j, pos) map
of the batch sweep and the loops of the one-stripe, streaming and clay_verify sweeps enumerate
every (parity chunk, byte) exactly once, the parametrized cases partition them, and the subsets
swept at the larger streaming sizes hold what they are there for -- every tile's edge bytes, all
four layer groups G, the lane-group columns c -- by the tile dump of the kernel's own tile map."""
from collections import Counter

import numpy as np
import pytest

import scrub_sweeps as sw
from clay_amd import ClayCode
from stream_cut import dump_tiles
from test_gpu_scrub import TILE


def _once(jj, pos, m, chunk):
    """Every (j, pos) of m chunks exactly once."""
    hits = np.bincount(np.asarray(jj) * chunk + np.asarray(pos), minlength=m * chunk)
    return hits.size == m * chunk and bool(np.all(hits == 1))


@pytest.mark.parametrize("size", sw.BS_SIZES, ids=[s[0] for s in sw.BS_SIZES])
@pytest.mark.parametrize("cfg", sorted({r[0] for r in sw.BS_ROWS}))
def test_batch_schedule_flips_every_byte_once(cfg, size):
    c = ClayCode(*cfg)
    W = TILE[cfg]
    sc = W + size[1]
    chunk = c.sub_chunk_no * sc
    assert 14 * 1024 <= chunk <= 27 * 1024
    # what the size is there for: one full tile, then a whole 32-byte unit and a shorter one
    assert sc // W == 1 and (sc - W) // 32 == 1 and (sc - W) % 32 == (8 if size[2] == 0 else 5)
    assert (sc % 8 == 0 and size[2] == 0) or (sc % 8 != 0 and size[2] % 8 != 0)
    slabs = sw.slabs(c.m, chunk)
    assert slabs[0][0] == 0 and sum(ns for _, ns in slabs) == chunk
    assert all(a[0] + a[1] == b[0] for a, b in zip(slabs, slabs[1:]))
    assert all(0 < ns and ns * c.m * chunk <= sw.SLAB_BYTES for _, ns in slabs)
    jj, pos = [], []
    for p0, ns in slabs:
        for r in range(c.m):
            j, p = sw.batch_pass(c.m, p0, ns, r)
            assert np.array_equal(p, p0 + np.arange(ns))  # stripe s is byte p0 + s, one flip per stripe
            assert np.array_equal(j, (np.arange(ns) + r) % c.m)
            jj.append(j)
            pos.append(p)
    jj, pos = np.concatenate(jj), np.concatenate(pos)
    assert _once(jj, pos, c.m, chunk)
    # one bit per flip, and all eight bit planes in every 8-byte piece of a lane's 32-byte unit, in every chunk
    bits = sw.flip_bits(pos, jj)
    assert set(bits.tolist()) == {1 << b for b in range(8)}
    planes = Counter(zip(jj.tolist(), (pos % sc % 32 // 8).tolist(), bits.tolist()))
    assert len(planes) == c.m * 4 * 8


def test_largest_batch_sweep_is_eleven_slabs():
    c = ClayCode(10, 4, 13)
    chunk = c.sub_chunk_no * (TILE[10, 4, 13] + 40)
    assert chunk == 26624 and len(sw.slabs(c.m, chunk)) == 11


def test_rows_are_the_kernels_of_the_issue():
    assert [(r[0], r[1]) for r in sw.BS_ROWS] == [((4, 2, 5), "auto"), ((4, 2, 5), "grouped"), ((6, 3, 8), "auto"),
                                                  ((8, 4, 11), "auto"), ((9, 3, 11), "auto"), ((10, 4, 13), "auto")]
    assert [r[2] for r in sw.BS_ROWS] == ["bs-scrub1"] + ["bs-scrub"] * 5
    assert [(s[1], s[2]) for s in sw.BS_SIZES] == [(40, 0), (37, 3)]
    assert sw.ONE_SC == 40 and (sw.VERIFY_CFG, sw.VERIFY_SC) == ((9, 3, 11), 37)


@pytest.mark.parametrize("cfg", sorted({r[0] for r in sw.BS_ROWS}))
def test_one_stripe_and_verify_loops_flip_every_byte_once(cfg):
    c = ClayCode(*cfg)
    for sc in {sw.ONE_SC} | ({sw.VERIFY_SC} if cfg == sw.VERIFY_CFG else set()):
        chunk = c.sub_chunk_no * sc
        jj, pos = sw.all_flips(c.m, chunk)
        assert _once(jj, pos, c.m, chunk)
        if sc == sw.VERIFY_SC:  # the GPU test's cases: one per parity chunk
            assert chunk == 2997 and chunk % 8 != 0
            assert sum(int(np.sum(jj == j)) for j in range(sw.VERIFY_CFG[1])) == len(jj)


@pytest.fixture(scope="module")
def tiles(tmp_path_factory):
    return dump_tiles(tmp_path_factory.mktemp("tiles"), sorted({case[0] for case in sw.stream_cases()}))


def test_expected_masks_come_from_the_parity():
    ref = np.arange(24, dtype=np.uint8).reshape(3, 8)
    jj, pos = sw.all_flips(3, 8)
    assert sw.expected_masks(ref, jj, pos, sw.flip_bits(pos, jj)).tolist() == [1] * 8 + [2] * 8 + [4] * 8
    assert not sw.expected_masks(ref, jj, pos, np.zeros(24, np.uint8)).any()  # no flip: no bit


def test_stream_cases_partition_the_full_products(tiles):
    cases = sw.stream_cases()
    assert len(set(cases)) == len(cases) and len({sw.case_id(k) for k in cases}) == len(cases)
    assert {k[0] for k in cases} == {16, 24, 264, 1064, 2288, 66176, 66184}
    for sc in (16, 24, 264):
        mine = [k for k in cases if k[0] == sc]
        assert all(k[1] == "full" for k in mine)
        flips = [sw.stream_flips(k, tiles[sc]) for k in mine]
        assert _once(np.concatenate([f[0] for f in flips]), np.concatenate([f[1] for f in flips]), 4, 256 * sc)
    assert sum(len(sw.stream_flips(k, tiles[264])[0]) for k in cases if k[0] == 264) == 4 * 67584


def _zx(at, sc):
    return set(zip((at // sc).tolist(), (at % sc).tolist()))


@pytest.mark.parametrize("sc", sw.STREAM_MID)
def test_mid_sizes_sweep_rows_and_edges(tiles, sc):
    cases = [k for k in sw.stream_cases() if k[0] == sc]
    assert sorted((k[1], k[2]) for k in cases) == sorted((kind, j) for kind in ("rows", "edges") for j in range(4))
    # eight layers holding all four G and, among them, the columns 0, 7, 8 and 63
    assert len(set(sw.ROW_LAYERS)) == 8
    assert {z % 4 for z in sw.ROW_LAYERS} == {0, 1, 2, 3} and {z // 4 for z in sw.ROW_LAYERS} == {0, 7, 8, 63}
    for kind, j, _ in [k[1:] for k in cases]:
        jj, at = sw.stream_flips((sc, kind, j, 0), tiles[sc])
        assert set(jj.tolist()) == {j} and len(set(at.tolist())) == len(at)
        got = _zx(at, sc)
        if kind == "rows":
            assert got == {(z, x) for z in sw.ROW_LAYERS for x in range(sc)}
        else:
            xs = {x for _, x in got}
            assert got == {(z, x) for z in range(256) for x in xs}
            for _, _, _, b0, vend in tiles[sc]:
                assert b0 in xs and vend - 1 in xs
                if (vend - b0) % 16:
                    assert all(b - 1 in xs and b in xs for b in range(b0 + 16, vend, 16))
    ragged = [(b0, vend) for _, _, _, b0, vend in tiles[sc] if (vend - b0) % 16]
    assert ragged == ([(960, 1064)] if sc == 1064 else [])


@pytest.mark.parametrize("sc", sw.STREAM_BIG)
def test_big_sizes_sweep_every_tile_edge(tiles, sc):
    cases = [k for k in sw.stream_cases() if k[0] == sc]
    assert cases == [(sc, "tile-edges", None, 0)]
    assert sorted(z % 4 for z in sw.BIG_LAYERS) == [0, 1, 2, 3] and {z // 4 for z in sw.BIG_LAYERS} == {0, 7, 8, 63}
    jj, at = sw.stream_flips(cases[0], tiles[sc])
    assert len(tiles[sc]) == 7 * 61 + 32
    edges = {x for _, _, _, b0, vend in tiles[sc] for x in (b0, vend - 1)}
    want = {(z, x) for z in sw.BIG_LAYERS for x in edges}
    for j in range(4):
        assert _zx(at[jj == j], sc) == want and int(np.sum(jj == j)) == len(want)
    assert 14000 <= len(jj) <= 17000
