"""Scrub entry points (clay_scrub_device / _batch / _strided, clay_verify) without a GPU: the
symbols are bound, the ABI version is unchanged, and validation -- the encode's, in the encode's
order and with its messages, then the scrub's own two checks -- runs before any device work, so
every error here is the validation's and never a DeviceError.  The pointers are never
dereferenced: every call returns before the device is touched."""
import numpy as np
import pytest

from clay_amd import ClayCode, ClayError, DeviceError, InvalidChunkSize, InvalidParameters, _lib

FAKE = 0x10000  # a non-NULL "device pointer"; validation never reads through it
SCRUB_CODES = [(4, 2, 5), (6, 3, 8), (8, 4, 11), (9, 3, 11), (10, 4, 13)]
NO_KERNEL = [(5, 3, 6), (9, 4, 12), (6, 3, 7), (10, 4, 12), (12, 4, 15)]  # d < n - 1, or no v1 instantiation
N = 5


def _err(fn, *args, **kw):
    with pytest.raises(ClayError) as ei:
        fn(*args, **kw)
    assert not isinstance(ei.value, DeviceError), ei.value.msg
    return ei.value


def _forms(c, chunk, data=FAKE, par=FAKE, res=FAKE, n=N):
    """The error of each device form for one argument set."""
    return [_err(c.scrub_device, [data] * c.k, [par] * c.m, res, chunk),
            _err(c.scrub_device_batch, [data] * (c.k * n), [par] * (c.m * n), res, n, chunk),
            _err(c.scrub_device_strided, data, par, res, n, chunk)]


def test_symbols_bound_and_abi_version():
    L = _lib.lib()
    for name in ("clay_scrub_device", "clay_scrub_device_batch", "clay_scrub_device_strided", "clay_verify"):
        assert hasattr(L, name) and name in _lib.SIGNATURES, name
    assert L.clay_abi_version() == 4


@pytest.mark.parametrize("cfg", SCRUB_CODES + [(5, 3, 6)])
def test_chunk_size_is_the_encodes_check(cfg):
    c = ClayCode(*cfg)
    chunk = c.sub_chunk_no * 32 + 1
    ref = _err(c.encode_device, [FAKE] * c.k, [FAKE] * c.m, chunk)
    assert isinstance(ref, InvalidChunkSize)
    for e in _forms(c, chunk) + _forms(c, chunk, res=0):  # before the null-result check
        assert (type(e), e.msg, e.fields) == (type(ref), ref.msg, ref.fields)
    e = _err(c.verify, [bytes(chunk)] * c.n)
    assert (type(e), e.msg, e.fields) == (type(ref), ref.msg, ref.fields)
    for e in _forms(c, 0):
        assert isinstance(e, InvalidChunkSize)


@pytest.mark.parametrize("cfg", SCRUB_CODES)
def test_null_arguments(cfg):
    c = ClayCode(*cfg)
    chunk = c.sub_chunk_no * 32
    for e in _forms(c, chunk, res=0):
        assert isinstance(e, InvalidParameters) and e.msg == "Invalid parameters: null scrub result", e.msg
    # null entries and null bases: the encode's messages
    ref = _err(c.encode_device, [0] * c.k, [FAKE] * c.m, chunk)
    e1, eb, es = _forms(c, chunk, data=0)
    assert (e1.msg, eb.msg) == (ref.msg, ref.msg) and isinstance(e1, InvalidParameters)
    assert isinstance(es, InvalidParameters) and es.msg == "Invalid parameters: null chunk array"
    ref = _err(c.encode_device, [FAKE] * c.k, [0] * c.m, chunk)
    e1, eb, es = _forms(c, chunk, par=0)
    assert (e1.msg, eb.msg) == (ref.msg, ref.msg) == ("Invalid parameters: null parity chunk",) * 2
    assert es.msg == "Invalid parameters: null chunk array"
    # one NULL entry deep in a batch
    d = [FAKE] * (c.k * N)
    d[c.k * 3 + 1] = 0
    e = _err(c.scrub_device_batch, d, [FAKE] * (c.m * N), FAKE, N, chunk)
    assert e.msg == "Invalid parameters: null data chunk"


@pytest.mark.parametrize("cfg", NO_KERNEL)
def test_codes_without_a_scrub_kernel(cfg):
    c = ClayCode(*cfg)
    chunk = c.sub_chunk_no * 32
    errs = _forms(c, chunk) + [_err(c.verify, [bytes(chunk)] * c.n)]
    for e in errs:
        assert isinstance(e, InvalidParameters), e.msg
        for name in ("(4,2,5)", "(6,3,8)", "(8,4,11)", "(9,3,11)", "(10,4,13)"):
            assert name in e.msg, e.msg
    # no stripes: still validated
    assert isinstance(_err(c.scrub_device_strided, FAKE, FAKE, FAKE, 0, chunk), InvalidParameters)


@pytest.mark.parametrize("cfg", SCRUB_CODES)
def test_zero_stripes_is_ok_and_touches_no_device(cfg):
    c = ClayCode(*cfg)
    chunk = c.sub_chunk_no * 32
    c.scrub_device_strided(FAKE, FAKE, FAKE, 0, chunk)
    c.scrub_device_batch([], [], FAKE, 0, chunk)
    c.scrub_device_strided(FAKE, FAKE, 0, 0, chunk)  # no stripes: no result word to define
    c.scrub_device_batch([], [], 0, 0, chunk)
    assert isinstance(_err(c.scrub_device_strided, FAKE, FAKE, FAKE, 0, chunk + 1), InvalidChunkSize)


def test_verify_checks_its_chunk_list():
    c = ClayCode(4, 2, 5)
    chunk = c.sub_chunk_no * 4
    with pytest.raises(ClayError):
        c.verify([bytes(chunk)] * (c.n - 1))
    with pytest.raises(ClayError):
        c.verify([bytes(chunk)] * (c.n - 1) + [bytes(chunk + c.sub_chunk_no)])
    # NULL chunk array / NULL mask through the C ABI
    import ctypes as C
    err = _lib.ClayErrorStruct()
    mask = C.c_uint32(0)
    arr = np.zeros(chunk, np.uint8)
    ptrs = (C.POINTER(C.c_uint8) * c.n)(*[arr.ctypes.data_as(C.POINTER(C.c_uint8))] * c.n)
    L = _lib.lib()
    assert L.clay_verify(C.byref(c.struct), None, chunk, C.byref(mask), C.byref(err)) == InvalidParameters.kind
    assert L.clay_verify(C.byref(c.struct), ptrs, chunk, None, C.byref(err)) == InvalidParameters.kind
    ptrs[c.k] = None
    assert L.clay_verify(C.byref(c.struct), ptrs, chunk, C.byref(mask), C.byref(err)) == InvalidParameters.kind
    assert err.msg == b"Invalid parameters: null parity chunk"
