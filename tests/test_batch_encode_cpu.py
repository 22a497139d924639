"""Device encode entry points (clay_encode_device / clay_encode_device_batch /
clay_encode_device_strided) without a GPU: the symbols are bound, the ABI version is unchanged, and
validation -- which runs once, before any device work -- reports the same errors in the same order
for all three forms.  The pointers are never dereferenced: every call here returns before the
device is touched (an error, or zero stripes)."""
import ctypes as C

import pytest

from clay_amd import ClayCode, ClayError, InvalidChunkSize, InvalidParameters, _lib
from clay_amd._lib import ClayErrorStruct

FAKE = 0x10000  # a non-NULL "device pointer"; validation never reads through it
CODES = [(4, 2, 5), (10, 4, 13), (5, 3, 6)]
N_STRIPES = 5

NULL_ARRAY = "Invalid parameters: null chunk array"
NULL_DATA = "Invalid parameters: null data chunk"
NULL_PARITY = "Invalid parameters: null parity chunk"


def _err(fn, *args, **kw):
    with pytest.raises(ClayError) as ei:
        fn(*args, **kw)
    return ei.value


def _is(e, kind, msg, fields=(0, 0, 0)):
    return type(e) is kind and e.msg == msg and e.fields == fields


def _raw(name, c, *args):
    """A C ABI call with the arguments as given (None: a NULL array) -> (rc, kind, msg, fields)."""
    err = ClayErrorStruct()
    rc = getattr(_lib.lib(), name)(C.byref(c._c), *args, C.byref(err))
    return rc, int(err.kind), err.msg.decode(), (int(err.a), int(err.b), int(err.c))


def _arr(vals):
    return (C.c_void_p * max(1, len(vals)))(*[v or None for v in vals])


def _chunk_msg(c, chunk):
    return f"Invalid chunk size: expected divisible by {c.sub_chunk_no}, got {chunk}"


def test_symbols_bound_and_abi_version():
    L = _lib.lib()
    for name in ("clay_encode_device", "clay_encode_device_batch", "clay_encode_device_strided"):
        assert hasattr(L, name) and name in _lib.SIGNATURES, name
    assert L.clay_abi_version() == 4


@pytest.mark.parametrize("cfg", CODES)
def test_null_arrays_and_null_bases(cfg):
    c = ClayCode(*cfg)
    chunk = c.sub_chunk_no * 32
    d1, p1 = _arr([FAKE] * c.k), _arr([FAKE] * c.m)
    dn, pn = _arr([FAKE] * (c.k * N_STRIPES)), _arr([FAKE] * (c.m * N_STRIPES))
    want = (InvalidParameters.kind, InvalidParameters.kind, NULL_ARRAY, (0, 0, 0))
    for data, par in ((None, p1), (d1, None), (None, None)):
        assert _raw("clay_encode_device", c, data, par, chunk, 0, None) == want
    for n in (N_STRIPES, 0):  # also with no stripe to encode
        for data, par in ((None, pn), (dn, None), (None, None)):
            assert _raw("clay_encode_device_batch", c, data, par, n, chunk, 0, None) == want
        for data, par in ((0, FAKE), (FAKE, 0), (0, 0)):
            e = _err(c.encode_device_strided, data, par, n, chunk)
            assert _is(e, InvalidParameters, NULL_ARRAY), (e.msg, e.fields)


@pytest.mark.parametrize("cfg", CODES)
def test_chunk_not_divisible_by_alpha(cfg):
    c = ClayCode(*cfg)
    for chunk in (c.sub_chunk_no * 32 + 1, 0):
        want = (c.sub_chunk_no, chunk, 0)  # InvalidChunkSize { expected, actual } (error.rs)
        errs = [_err(c.encode_device, [FAKE] * c.k, [FAKE] * c.m, chunk)]
        for n in (N_STRIPES, 0):
            errs.append(_err(c.encode_device_batch, [FAKE] * (c.k * n), [FAKE] * (c.m * n), n, chunk))
            errs.append(_err(c.encode_device_strided, FAKE, FAKE, n, chunk, data_node_stride=64,
                             data_stripe_stride=1024, parity_node_stride=64, parity_stripe_stride=1024))
        for e in errs:
            assert _is(e, InvalidChunkSize, _chunk_msg(c, chunk), want), (e.msg, e.fields)


@pytest.mark.parametrize("cfg", CODES)
def test_null_entry_in_the_middle(cfg):
    c = ClayCode(*cfg)
    chunk = c.sub_chunk_no * 32
    # one stripe
    data, par = [FAKE] * c.k, [FAKE] * c.m
    data[c.k // 2] = 0
    e = _err(c.encode_device, data, par, chunk)
    assert _is(e, InvalidParameters, NULL_DATA), e.msg
    par[c.m - 1] = 0
    e = _err(c.encode_device, [FAKE] * c.k, par, chunk)
    assert _is(e, InvalidParameters, NULL_PARITY), e.msg
    # a batch: the NULL entry in a stripe after the first
    n = N_STRIPES
    data, par = [FAKE] * (c.k * n), [FAKE] * (c.m * n)
    data[2 * c.k + 1] = 0
    e = _err(c.encode_device_batch, data, par, n, chunk)
    assert _is(e, InvalidParameters, NULL_DATA), e.msg
    par[3 * c.m + c.m - 1] = 0
    e = _err(c.encode_device_batch, [FAKE] * (c.k * n), par, n, chunk)
    assert _is(e, InvalidParameters, NULL_PARITY), e.msg


@pytest.mark.parametrize("cfg", CODES)
def test_order_of_the_checks(cfg):
    """code, NULL array / base, chunk size, NULL data entry, NULL parity entry."""
    c = ClayCode(*cfg)
    chunk, bad = c.sub_chunk_no * 32, c.sub_chunk_no * 32 + 1
    n = N_STRIPES
    hole_d, hole_p = [FAKE] * (c.k * n), [FAKE] * (c.m * n)
    hole_d[c.k + 1] = 0
    hole_p[c.m] = 0
    # a NULL array wins over a bad chunk size
    rc, kind, msg, _ = _raw("clay_encode_device_batch", c, None, _arr(hole_p), n, bad, 0, None)
    assert (rc, kind, msg) == (InvalidParameters.kind, InvalidParameters.kind, NULL_ARRAY)
    rc, kind, msg, _ = _raw("clay_encode_device", c, _arr(hole_d[:c.k]), None, bad, 0, None)
    assert (rc, kind, msg) == (InvalidParameters.kind, InvalidParameters.kind, NULL_ARRAY)
    e = _err(c.encode_device_strided, 0, FAKE, n, bad)
    assert _is(e, InvalidParameters, NULL_ARRAY), e.msg
    # a bad chunk size wins over NULL entries
    e = _err(c.encode_device_batch, hole_d, hole_p, n, bad)
    assert _is(e, InvalidChunkSize, _chunk_msg(c, bad), (c.sub_chunk_no, bad, 0)), e.msg
    e = _err(c.encode_device, hole_d[c.k:2 * c.k], hole_p[c.m:2 * c.m], bad)
    assert _is(e, InvalidChunkSize, _chunk_msg(c, bad), (c.sub_chunk_no, bad, 0)), e.msg
    # a NULL data entry wins over a NULL parity entry, wherever the two are
    e = _err(c.encode_device_batch, hole_d, hole_p, n, chunk)
    assert _is(e, InvalidParameters, NULL_DATA), e.msg
    late_d = [FAKE] * (c.k * n)
    late_d[-1] = 0
    e = _err(c.encode_device_batch, late_d, hole_p, n, chunk)
    assert _is(e, InvalidParameters, NULL_DATA), e.msg
    e = _err(c.encode_device, hole_d[c.k:2 * c.k], hole_p[c.m:2 * c.m], chunk)
    assert _is(e, InvalidParameters, NULL_DATA), e.msg
    # a code struct that clay_new did not produce is refused before anything else
    broken = ClayCode(*cfg)
    broken._c.q += 1
    e = _err(broken.encode_device_strided, 0, 0, n, bad)
    assert type(e) is InvalidParameters and e.msg != NULL_ARRAY, e.msg
    e2 = _err(broken.encode_device_batch, hole_d, hole_p, n, bad)
    e1 = _err(broken.encode_device, hole_d[:c.k], hole_p[:c.m], bad)
    assert (e.msg, e.fields) == (e1.msg, e1.fields) == (e2.msg, e2.fields)


@pytest.mark.parametrize("cfg", CODES)
def test_zero_stripes_is_ok_and_touches_no_device(cfg):
    c = ClayCode(*cfg)
    chunk = c.sub_chunk_no * 32
    c.encode_device_strided(FAKE, FAKE, 0, chunk)
    c.encode_device_batch([], [], 0, chunk)
    # zero stripes: no entry of the arrays is read
    assert _raw("clay_encode_device_batch", c, _arr([0]), _arr([0]), 0, chunk, 0, None) == (0, 0, "", (0, 0, 0))
    # ... but the arguments are still validated
    assert isinstance(_err(c.encode_device_strided, FAKE, FAKE, 0, chunk + 1), InvalidChunkSize)
    assert isinstance(_err(c.encode_device_batch, [], [], 0, chunk + 1), InvalidChunkSize)
    assert isinstance(_err(c.encode_device_strided, FAKE, 0, 0, chunk), InvalidParameters)
