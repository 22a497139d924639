"""The batched encode entry points (clay_encode_device_batch / _strided) at shapes the streaming
batch takes on a GPU ((10,4,13) and (9,4,12), stripes above 4 MiB, and small ones under "stream"),
without a GPU: validation still runs in the encode's order with its messages, before any device
work, so every error here is the validation's and never a DeviceError.  The pointers are never
dereferenced.  The streaming batch adds no export and no encode path: the ABI version and the set
of paths clay_set_encode_path accepts are unchanged."""
import pytest

import clay_amd
from clay_amd import ClayCode, ClayError, DeviceError, InvalidChunkSize, InvalidParameters, _lib

FAKE = 0x10000  # a non-NULL "device pointer"; validation never reads through it
CODES = [(10, 4, 13), (9, 4, 12)]
N = 5
SC_BIG, SC_SMALL = 6560, 24  # a 16 MiB stripe of (10,4,13); a tile of one ragged piece


def _err(fn, *args, **kw):
    with pytest.raises(ClayError) as ei:
        fn(*args, **kw)
    assert not isinstance(ei.value, DeviceError), ei.value.msg
    return ei.value


def _same(e, ref):
    assert (type(e), e.msg, e.fields) == (type(ref), ref.msg, ref.fields), (e.msg, ref.msg)


@pytest.fixture(params=["auto", "stream"])
def path(request):
    clay_amd.set_encode_path(request.param, 0)
    yield request.param
    clay_amd.set_encode_path("auto", 0)


@pytest.mark.parametrize("cfg", CODES)
@pytest.mark.parametrize("sc", [SC_BIG, SC_SMALL])
def test_batch_forms_validate_as_the_encode(cfg, sc, path):
    c = ClayCode(*cfg)
    chunk = c.sub_chunk_no * sc
    # chunk size first: not divisible by the sub-chunk count, then zero
    ref = _err(c.encode_device, [FAKE] * c.k, [FAKE] * c.m, chunk + 1)
    assert isinstance(ref, InvalidChunkSize)
    _same(_err(c.encode_device_batch, [FAKE] * (c.k * N), [FAKE] * (c.m * N), N, chunk + 1), ref)
    _same(_err(c.encode_device_strided, FAKE, FAKE, N, chunk + 1), ref)
    _same(_err(c.encode_device_strided, 0, FAKE, N, chunk + 1), _err(c.encode_device_strided, 0, FAKE, N, chunk))
    assert isinstance(_err(c.encode_device_strided, FAKE, FAKE, N, 0), InvalidChunkSize)
    # null bases and null entries: the encode's messages
    for d, p in ((0, FAKE), (FAKE, 0)):
        e = _err(c.encode_device_strided, d, p, N, chunk)
        assert isinstance(e, InvalidParameters) and e.msg == "Invalid parameters: null chunk array"
    ref = _err(c.encode_device, [0] * c.k, [FAKE] * c.m, chunk)
    assert ref.msg == "Invalid parameters: null data chunk"
    d = [FAKE] * (c.k * N)
    d[c.k * 3 + 1] = 0  # one NULL entry deep in the batch
    _same(_err(c.encode_device_batch, d, [FAKE] * (c.m * N), N, chunk), ref)
    ref = _err(c.encode_device, [FAKE] * c.k, [0] * c.m, chunk)
    assert ref.msg == "Invalid parameters: null parity chunk"
    p = [FAKE] * (c.m * N)
    p[c.m * (N - 1)] = 0
    _same(_err(c.encode_device_batch, [FAKE] * (c.k * N), p, N, chunk), ref)
    # a null data entry is reported before a null parity entry
    assert _err(c.encode_device_batch, d, p, N, chunk).msg == "Invalid parameters: null data chunk"


@pytest.mark.parametrize("cfg", CODES)
def test_zero_stripes_is_ok_and_touches_no_device(cfg, path):
    c = ClayCode(*cfg)
    chunk = c.sub_chunk_no * SC_BIG
    c.encode_device_strided(FAKE, FAKE, 0, chunk)
    c.encode_device_batch([], [], 0, chunk)
    assert isinstance(_err(c.encode_device_strided, FAKE, FAKE, 0, chunk + 1), InvalidChunkSize)


def test_no_new_export_and_no_new_path():
    L = _lib.lib()
    assert L.clay_abi_version() == 4
    assert not [n for n in _lib.SIGNATURES if "stream_batch" in n or "batch_stream" in n]
    # the encode paths are auto, staged, fused, bitsliced (3) and stream (5), as before: nothing
    # new is accepted, and "stream" keeps its variants 0, 1, 2, 4, 7
    prev = L.clay_set_encode_path(0)
    try:
        accepted = [p for p in range(0, 16) if L.clay_set_encode_path(p) >= 0]
        assert accepted == [0, 1, 2, 3, 5], accepted
        variants = [v for v in range(0, 16) if L.clay_set_encode_path(5 | (v << 8)) >= 0]
        assert variants == [0, 1, 2, 4, 7], variants
        with pytest.raises(ValueError):
            clay_amd.set_encode_path("stream-batch")
    finally:
        L.clay_set_encode_path(0)
    assert prev >= 0
