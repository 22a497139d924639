"""k_stream_encode on the balanced tile map (clay_amd/csrc/stream_tile_map.hpp), bit for bit
against the oracle, at the smallest sub-chunk sizes that reach each path of the sub-256 tiles.

The classes (R = rounds per XCD, widths of the rounds' tiles):
  r1_w112_w128   R = 1, tiles 112 and 128 bytes wide: the odd lanes of the paired store all masked
  r1_straddle    R = 1, a tile of 128 + 8 bytes (sc % 16 == 8: patched piece, plain stores)
  r2_equal       R = 2, both rounds the same width (< 256)
  r2_diff16      R = 2, widths 16 apart
  r2_straddle    R = 2 with sc % 16 == 8
  r3_clipped     R = 3, a workgroup's share of the region is not a multiple of 16: the last round
                 holds a clipped tile and empty slots
  r3_full        R = 3, every tile exactly 256 bytes
The sizes are searched with a Python restatement of the map for the device's workgroups per XCD
(multi_processor_count // 8), so every case is the smallest sc of its class on that device.  R = 2
needs more than 256 bytes and R = 3 more than 512 bytes of every row per workgroup, which on 256
CUs is 190 MB, 340 MB (r3_clipped) and 500 MB (r3_full) of data.  The oracle's parity is computed
once per (code, sc) and shared by the loader variants.
"""
import functools

import numpy as np
import pytest

from clay_amd import ClayCode, set_encode_path, last_encode_path
from stream_cut import stream_cut


def layout(sc, ns_dev):
    """Per XCD: (workgroups, rounds, round widths, widths of the last round's tiles after clipping),
    as launch_stream (engine.hip: stream_cut) and BalancedMap cut a row of sc bytes."""
    region, ns = stream_cut(sc, ns_dev)
    out = []
    for x in range(8):
        x0, x1 = x * region, min((x + 1) * region, sc)
        if x0 >= x1:
            continue
        ln = x1 - x0
        rounds = -(-ln // (ns * 256))
        q, rem = divmod(-(-ln // (ns * 16)), rounds)
        widths = [(q + (r < rem)) * 16 for r in range(rounds)]
        before = ns * sum(widths[:-1])
        last = [max(0, min(widths[-1], ln - before - s * widths[-1])) for s in range(ns)]
        out.append((ns, rounds, widths, last, ln))
    return out


def _all_tiles(lay):
    for ns, rounds, widths, last, _ in lay:
        for w in widths[:-1]:
            yield w
        for w in last:
            if w:
                yield w


CLASSES = {
    "r1_w112_w128": lambda sc, lay: all(r == 1 for _, r, _, _, _ in lay) and set(_all_tiles(lay)) == {112, 128},
    "r1_straddle": lambda sc, lay: all(r == 1 for _, r, _, _, _ in lay) and 136 in set(_all_tiles(lay)),
    "r2_equal": lambda sc, lay: sc % 16 == 0 and all(r == 2 and w[0] == w[1] < 256 for _, r, w, _, _ in lay),
    "r2_diff16": lambda sc, lay: sc % 16 == 0 and all(r == 2 for _, r, _, _, _ in lay)
    and any(w[0] - w[1] == 16 for _, _, w, _, _ in lay),
    "r2_straddle": lambda sc, lay: sc % 16 == 8 and all(r == 2 for _, r, _, _, _ in lay),
    "r3_clipped": lambda sc, lay: sc % 16 == 0 and all(r == 3 for _, r, _, _, _ in lay)
    and any(ln % (ns * 16) and 0 in last and any(0 < w < ws[-1] for w in last) for ns, _, ws, last, ln in lay),
    "r3_full": lambda sc, lay: all(r == 3 for _, r, _, _, _ in lay) and set(_all_tiles(lay)) == {256},
}


@functools.lru_cache(maxsize=None)
def class_sc(name, ns_dev):
    """Smallest sc (a multiple of 8, >= 16) of the class for ns_dev workgroups per XCD."""
    pred = CLASSES[name]
    rounds = int(name[1])
    # R rounds on every XCD need more than (R - 1) * 256 bytes per workgroup in the last region
    sc = 16 if rounds == 1 else 8 * ns_dev * 256 * (rounds - 1) - 2048
    limit = 8 * (ns_dev * 256 * rounds + 32)
    while sc <= limit:
        if pred(sc, layout(sc, ns_dev)):
            return sc
        sc += 8
    raise AssertionError(f"no sub-chunk size of class {name} for {ns_dev} workgroups per XCD")


def test_class_sizes_on_256_cus():
    """The class search on the MI355X's 32 workgroups per XCD (no GPU: a check of the test's own
    search: every class has a size, of the row length its round count implies)."""
    got = {name: class_sc(name, 32) for name in CLASSES}
    assert got["r1_w112_w128"] == 6 * 128 + 112 and got["r1_straddle"] == 6 * 160 + 136, got
    for name, sc in got.items():
        assert sc % 8 == 0 and 8 * 32 * 256 * (int(name[1]) - 1) < sc <= 8 * 32 * 256 * int(name[1]), (name, sc)


@functools.lru_cache(maxsize=1)
def _reference(cfg, sc):
    """(data, oracle codeword) of one (code, sc); the cases of one size run back to back."""
    from oracle import oracle
    oracle.build()
    k, m, d = cfg
    c, o = ClayCode(k, m, d), oracle.OracleClay(k, m, d)
    data = np.random.default_rng(sc + 1000 * k).integers(0, 256, k * c.sub_chunk_no * sc - 7, dtype=np.uint8)
    ref = o.encode_array(data)
    assert ref.shape[1] == c.sub_chunk_no * sc
    data.setflags(write=False)
    ref.setflags(write=False)
    return data, ref


CASES = [((10, 4, 13), 0), ((10, 4, 13), 1), ((10, 4, 13), 2), ((9, 4, 12), 0)]


@pytest.mark.gpu
@pytest.mark.parametrize("cfg,loaders", CASES)
@pytest.mark.parametrize("name", list(CLASSES))
def test_balanced_stream_encode_matches_oracle(torch_cuda, name, cfg, loaders):
    ns_dev = max(1, torch_cuda.cuda.get_device_properties(0).multi_processor_count // 8)
    sc = class_sc(name, ns_dev)
    k, m, d = cfg
    data, ref = _reference(cfg, sc)
    set_encode_path("stream", loaders)
    try:
        got = ClayCode(k, m, d).encode_array(data)
        assert last_encode_path().startswith("stream-"), last_encode_path()
    finally:
        set_encode_path("auto", 0)
    assert got.shape == ref.shape
    assert np.array_equal(got, ref), (name, cfg, sc, loaders)
