"""OracleClay.decode_chunks (oc_decode_chunks): the oracle's decode with every chunk returned, the
rebuilt parity chunks included -- the CPU reference for the parity outputs of the device decodes
on non-codeword input (clay.h: "the value the reference computes internally, decode.rs:213-253").

It shares its body with oc_decode, so the checks here are the ones that tie the extra rows down:
the data rows are decode()'s, on a codeword every row is encode_array's (any correct decoder
returns the codeword), present nodes come back as given, and the errors are decode()'s."""
import itertools

import numpy as np
import pytest

from test_gpu_parity import CONFIGS as PARITY_CONFIGS

CONFIGS = PARITY_CONFIGS + [(9, 4, 12)]
EXHAUSTIVE = [(4, 2, 5), (6, 3, 8), (5, 3, 6), (3, 3, 4)]
SC = 2  # the reference's smallest sub-chunk (encode.rs:33-39)


def patterns(o, cfg):
    """Every erasure pattern of the small codes; a seeded sample of 30 of the larger ones'."""
    pats = [list(e) for r in range(1, o.m + 1) for e in itertools.combinations(range(o.n), r)]
    if cfg in EXHAUSTIVE:
        return pats
    idx = np.random.default_rng([cfg[0], cfg[1], 41]).permutation(len(pats))[:30]
    return [pats[i] for i in sorted(idx)]


def test_configs_are_the_parity_configs_plus_9_4_12():
    assert len(PARITY_CONFIGS) == 8 and len(set(CONFIGS)) == 9 and set(EXHAUSTIVE) <= set(CONFIGS)


@pytest.mark.parametrize("cfg", CONFIGS)
def test_data_rows_equal_decode_on_random_chunks(oracle_mod, cfg):
    o = oracle_mod.OracleClay(*cfg)
    chunk = o.sub_chunk_no * SC
    rng = np.random.default_rng(300 + cfg[0])
    for er in patterns(o, cfg):
        chunks = rng.integers(0, 256, (o.n, chunk), dtype=np.uint8)
        av = {i: chunks[i] for i in range(o.n) if i not in er}
        got = o.decode_chunks(av, er)
        assert got.shape == (o.n, chunk) and got.dtype == np.uint8
        assert got[:o.k].tobytes() == o.decode(av, er), (cfg, er)
        for i in av:
            assert np.array_equal(got[i], chunks[i]), ("present node changed", cfg, er, i)
        # the availability map's order is the reference's HashMap order: no effect on the result
        rev = {i: av[i] for i in reversed(list(av))}
        assert np.array_equal(o.decode_chunks(rev, er), got), (cfg, er)


@pytest.mark.parametrize("cfg", CONFIGS)
def test_codeword_comes_back_whole(oracle_mod, cfg):
    o = oracle_mod.OracleClay(*cfg)
    chunk = o.sub_chunk_no * SC
    ref = o.encode_array(np.random.default_rng(400 + cfg[0]).integers(0, 256, o.k * chunk, dtype=np.uint8))
    assert ref.shape == (o.n, chunk)
    n_parity = 0
    for er in patterns(o, cfg):
        got = o.decode_chunks({i: ref[i] for i in range(o.n) if i not in er}, er)
        assert np.array_equal(got, ref), (cfg, er, [i for i in range(o.n) if not np.array_equal(got[i], ref[i])])
        n_parity += sum(1 for e in er if e >= o.k)
    assert n_parity > 0


def test_no_erasures_and_errors_as_decode(oracle_mod):
    o = oracle_mod.OracleClay(4, 2, 5)
    chunk = o.sub_chunk_no * SC
    chunks = np.random.default_rng(5).integers(0, 256, (o.n, chunk), dtype=np.uint8)
    assert np.array_equal(o.decode_chunks({i: chunks[i] for i in range(o.n)}, []), chunks)
    assert o.decode_chunks({}, []).shape == (o.n, 0) and o.decode({}, []) == b""
    bad = [({i: chunks[i] for i in range(3, 6)}, [0, 1, 2]),           # TooManyErasures
           ({i: chunks[i] for i in range(6)}, [0]),                     # both available and erased
           ({i: chunks[i] for i in range(2, 6)}, [0]),                  # a node neither given nor erased
           ({i: chunks[i][:chunk - 1] for i in range(1, 6)}, [0]),      # InvalidChunkSize
           ({}, [0])]
    for av, er in bad:
        with pytest.raises(oracle_mod.OracleError) as a:
            o.decode(av, er)
        with pytest.raises(oracle_mod.OracleError) as b:
            o.decode_chunks(av, er)
        assert (a.value.kind, a.value.fields, a.value.msg) == (b.value.kind, b.value.fields, b.value.msg)
