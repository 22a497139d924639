"""Batched repair entry points (clay_repair_device_strided / clay_repair_device_batch) without a
GPU: the symbols are bound, the ABI version is unchanged, and validation -- which runs once,
before any device work -- gives exactly what clay_repair_device gives for the same arguments.
The pointers are never dereferenced: every call here returns before the device is touched.

clay_repair_device has no NULL check of its helper buffers (only of its output), so there is no
single-stripe error to compare a NULL helper base with: the batch forms report it as
InvalidParameters, "null helper buffer", after the checks they share with clay_repair_device."""
import pytest

from clay_amd import (ClayCode, ClayError, InsufficientHelpers, InvalidChunkSize, InvalidParameters,
                      MissingYSectionHelper, _lib)

FAKE = 0x10000  # a non-NULL "device pointer"; validation never reads through it
CODES = [(4, 2, 5), (10, 4, 13), (5, 3, 6)]
N_STRIPES = 5


def _err(fn, *args, **kw):
    with pytest.raises(ClayError) as ei:
        fn(*args, **kw)
    return ei.value


def _same(a, b):
    return (type(a), a.msg, a.fields) == (type(b), b.msg, b.fields)


def _helpers(c, lost):
    return [h for h, _ in c.minimum_to_repair(lost, [i for i in range(c.n) if i != lost])]


def _all_forms(c, lost, ids, chunk, out=FAKE, base=FAKE, n=N_STRIPES):
    """The error of each batch form and layout for one argument set -> list of ClayError."""
    errs = []
    for full in (False, True):
        errs.append(_err(c.repair_device_strided, lost, ids, base, out, n, chunk, full_chunks=full))
        errs.append(_err(c.repair_device_batch, lost, ids, [base or None] * (n * len(ids)), [out or None] * n, n, chunk,
                         full_chunks=full))
    return errs


def test_symbols_bound_and_abi_version():
    L = _lib.lib()
    for name in ("clay_repair_device_strided", "clay_repair_device_batch"):
        assert hasattr(L, name) and name in _lib.SIGNATURES, name
    assert L.clay_abi_version() == 4


@pytest.mark.parametrize("cfg", CODES)
@pytest.mark.parametrize("what", ["lost_index", "too_few", "chunk_size", "duplicate", "missing_y"])
def test_validation_matches_repair_device(cfg, what):
    c = ClayCode(*cfg)
    lost, chunk = 0, c.sub_chunk_no * 32
    ids = _helpers(c, lost)
    assert len(ids) == c.d
    kind = None
    if what == "lost_index":
        lost, kind = c.n, InvalidParameters
    elif what == "too_few":
        ids, kind = ids[:-1], InsufficientHelpers
    elif what == "chunk_size":
        chunk, kind = chunk + 1, InvalidChunkSize
    elif what == "duplicate":
        ids, kind = ids + [ids[0]], InvalidParameters
    else:
        # node 1 shares node 0's y-section in every code here; the list stays d entries long
        assert 1 in ids
        rest = [h for h in ids if h != 1]
        ids, kind = rest + [rest[0]], MissingYSectionHelper
    ref = _err(c.repair_device, lost, ids, [FAKE] * len(ids), chunk, FAKE)
    assert isinstance(ref, kind), (what, ref)
    ref_full = _err(c.repair_device_full_chunks, lost, ids, [FAKE] * len(ids), chunk, FAKE)
    assert _same(ref, ref_full)
    for e in _all_forms(c, lost, ids, chunk):
        assert _same(e, ref), (what, e.msg, ref.msg, e.fields, ref.fields)
    if what == "too_few":
        assert ref.fields[:2] == (c.d, c.d - 1)  # InsufficientHelpers { needed, provided } (error.rs)
    if what == "missing_y":
        assert ref.fields[:2] == (0, 1)  # MissingYSectionHelper { lost_node, missing_helper }


@pytest.mark.parametrize("cfg", CODES)
def test_null_output_and_null_base(cfg):
    c = ClayCode(*cfg)
    lost, chunk = 0, c.sub_chunk_no * 32
    ids = _helpers(c, lost)
    ref = _err(c.repair_device, lost, ids, [FAKE] * len(ids), chunk, 0)
    assert isinstance(ref, InvalidParameters) and ref.msg == "Invalid parameters: null output"
    for e in _all_forms(c, lost, ids, chunk, out=0):
        assert _same(e, ref), (e.msg, ref.msg)
    for e in _all_forms(c, lost, ids, chunk, base=0):
        assert isinstance(e, InvalidParameters) and e.msg == "Invalid parameters: null helper buffer", e.msg
        assert e.fields == (0, 0, 0)
    # the shared checks come first, as in clay_repair_device: a bad chunk size with a NULL output
    ref = _err(c.repair_device, lost, ids, [FAKE] * len(ids), chunk + 1, 0)
    assert isinstance(ref, InvalidChunkSize)
    for e in _all_forms(c, lost, ids, chunk + 1, out=0, base=0):
        assert _same(e, ref), (e.msg, ref.msg)
    # one NULL entry of the pointer form
    bufs = [FAKE] * (N_STRIPES * len(ids))
    bufs[len(ids) + 1] = None
    e = _err(c.repair_device_batch, lost, ids, bufs, [FAKE] * N_STRIPES, N_STRIPES, chunk)
    assert isinstance(e, InvalidParameters) and e.msg == "Invalid parameters: null helper buffer"
    outs = [FAKE] * N_STRIPES
    outs[3] = None
    e = _err(c.repair_device_batch, lost, ids, [FAKE] * (N_STRIPES * len(ids)), outs, N_STRIPES, chunk)
    assert isinstance(e, InvalidParameters) and e.msg == "Invalid parameters: null output"


@pytest.mark.parametrize("cfg", CODES)
def test_zero_stripes_is_ok_and_touches_no_device(cfg):
    c = ClayCode(*cfg)
    lost, chunk = 0, c.sub_chunk_no * 32
    ids = _helpers(c, lost)
    for full in (False, True):
        c.repair_device_strided(lost, ids, FAKE, FAKE, 0, chunk, full_chunks=full)
        c.repair_device_batch(lost, ids, [], [], 0, chunk, full_chunks=full)
    # ... but the arguments are still validated
    ref = _err(c.repair_device, c.n, ids, [FAKE] * len(ids), chunk, FAKE)
    for e in _all_forms(c, c.n, ids, chunk, n=0):
        assert _same(e, ref)
    assert isinstance(_err(c.repair_device_strided, lost, ids[:-1], FAKE, FAKE, 0, chunk), InsufficientHelpers)
