"""Batched decode entry points (clay_decode_device_strided / clay_decode_device_batch) without a
GPU: the symbols are bound, the ABI version is unchanged, and validation -- which runs once,
before any device work -- gives exactly what clay_decode_device gives for the same arguments.
The pointers are never dereferenced: every call here returns before the device is touched."""
import pytest

from clay_amd import ClayCode, ClayError, InvalidParameters, TooManyErasures, _lib

FAKE = 0x10000  # a non-NULL "device pointer"; validation never reads through it


def _err(fn, *args):
    with pytest.raises(ClayError) as ei:
        fn(*args)
    return ei.value


def _single(c, erasures, chunk):
    """What decode_device raises for stripe 0 of the strided layout (every node outside
    `erasures` available, every erased node wanted)."""
    gone = set(e for e in erasures if e < c.n)
    chunks = [None if i in gone else FAKE + i * chunk for i in range(c.n)]
    outs = [FAKE + i * chunk if i in gone else None for i in range(c.n)]
    return _err(c.decode_device, chunks, erasures, outs, chunk)


def test_symbols_bound_and_abi_version():
    L = _lib.lib()
    for name in ("clay_decode_device_strided", "clay_decode_device_batch"):
        assert hasattr(L, name) and name in _lib.SIGNATURES, name
    assert L.clay_abi_version() == 4


@pytest.mark.parametrize("cfg", [(4, 2, 5), (10, 4, 13), (5, 3, 6)])
def test_strided_too_many_erasures(cfg):
    c = ClayCode(*cfg)
    chunk = c.sub_chunk_no * 32
    er = list(range(c.m + 1))
    e = _err(c.decode_device_strided, FAKE, er, FAKE, 7, chunk)
    assert isinstance(e, TooManyErasures)
    assert e.fields[:2] == (c.m, c.m + 1)  # TooManyErasures { max, actual } (error.rs)
    ref = _single(c, er, chunk)
    assert (type(e), e.msg, e.fields) == (type(ref), ref.msg, ref.fields)


@pytest.mark.parametrize("what", ["index", "chunk_size", "duplicate"])
def test_strided_validation_matches_decode_device(what):
    c = ClayCode(4, 2, 5)
    chunk = c.sub_chunk_no * 32
    er = [0]
    if what == "index":
        er = [c.n]
    elif what == "chunk_size":
        chunk += 1
    else:
        er = [1, 1]
    e = _err(c.decode_device_strided, FAKE, er, FAKE, 5, chunk)
    ref = _single(c, er, chunk)
    assert (type(e), e.msg, e.fields) == (type(ref), ref.msg, ref.fields), what
    # the pointer-array form validates the same way
    gone = set(x for x in er if x < c.n)
    chunks = [None if i in gone else FAKE for _ in range(5) for i in range(c.n)]
    outs = [FAKE if i in gone else None for _ in range(5) for i in range(c.n)]
    e2 = _err(c.decode_device_batch, chunks, er, outs, 5, chunk)
    assert (type(e2), e2.msg, e2.fields) == (type(ref), ref.msg, ref.fields), what


def test_zero_stripes_is_ok_and_touches_no_device():
    c = ClayCode(4, 2, 5)
    chunk = c.sub_chunk_no * 32
    c.decode_device_strided(FAKE, [0], FAKE, 0, chunk)
    c.decode_device_batch([], [0], [], 0, chunk)
    # ... but the arguments are still validated
    assert isinstance(_err(c.decode_device_strided, FAKE, [0, 1, 2], FAKE, 0, chunk), TooManyErasures)


def test_batch_null_pattern_must_agree():
    c = ClayCode(4, 2, 5)
    chunk = c.sub_chunk_no * 32
    s0 = [None if i == 0 else FAKE for i in range(c.n)]
    s1 = [None if i == 1 else FAKE for i in range(c.n)]  # stripe 1 lost another node
    o0 = [FAKE if i == 0 else None for i in range(c.n)]
    e = _err(c.decode_device_batch, s0 + s1, [0], o0 + o0, 2, chunk)
    assert isinstance(e, InvalidParameters)
    # same chunks pattern, but stripe 1 has no output buffer for the erased node
    o1 = [None] * c.n
    e = _err(c.decode_device_batch, s0 + s0, [0], o0 + o1, 2, chunk)
    assert isinstance(e, InvalidParameters)


def test_strided_null_base_is_invalid():
    c = ClayCode(4, 2, 5)
    e = _err(c.decode_device_strided, 0, [0], FAKE, 4, c.sub_chunk_no * 32)
    assert isinstance(e, InvalidParameters)
