"""clay_set_scrub_path / clay_amd.set_scrub_path without a GPU: the symbol is exported and bound,
the ABI version is unchanged, the setter validates its argument (previous value returned, unknown
values rejected with the setting unchanged), and it does not disturb validation: under
'stream-batch' every error of test_scrub_cpu.py's forms still arrives before any device work."""
import pytest

import clay_amd
from clay_amd import ClayCode, InvalidChunkSize, InvalidParameters, _lib
from test_scrub_cpu import FAKE, N, NO_KERNEL, SCRUB_CODES, _err, _forms


@pytest.fixture
def scrub_path():
    """set_scrub_path for the test, 'auto' afterwards."""
    yield clay_amd.set_scrub_path
    _lib.lib().clay_set_scrub_path(0)


def test_symbol_bound_and_abi_version():
    L = _lib.lib()
    assert hasattr(L, "clay_set_scrub_path") and "clay_set_scrub_path" in _lib.SIGNATURES
    assert "set_scrub_path" in clay_amd.__all__ and callable(clay_amd.set_scrub_path)
    assert L.clay_abi_version() == 4


def test_setter_c_abi(scrub_path):
    L = _lib.lib()
    assert L.clay_set_scrub_path(0) in (0, 1)
    assert L.clay_set_scrub_path(1) == 0  # the previous value
    assert L.clay_set_scrub_path(1) == 1
    for bad in (-1, 2, 3, 5, 255, 256, 257, 1 << 16, -(1 << 31)):
        assert L.clay_set_scrub_path(bad) == -1, bad
        assert L.clay_set_scrub_path(1) == 1, bad  # unchanged by the rejected value
    assert L.clay_set_scrub_path(0) == 1
    for bad in (2, -1):
        assert L.clay_set_scrub_path(bad) == -1
        assert L.clay_set_scrub_path(0) == 0


def test_setter_python(scrub_path):
    scrub_path("auto")
    assert scrub_path("stream-batch") == "auto"
    assert scrub_path("stream-batch") == "stream-batch"
    for bad in ("stream", "batch", "", "AUTO", "stream_batch", None, 1):
        with pytest.raises(ValueError):
            scrub_path(bad)
        assert scrub_path("stream-batch") == "stream-batch", bad
    assert scrub_path("auto") == "stream-batch"
    assert scrub_path("auto") == "auto"


def test_setter_leaves_the_other_setters_alone(scrub_path):
    prev_exec = clay_amd.set_exec_mode("stream")
    try:
        scrub_path("stream-batch")
        assert clay_amd.set_exec_mode("stream") == "stream"
        assert clay_amd.set_encode_path("auto") == "auto"
        assert scrub_path("auto") == "stream-batch"
    finally:
        clay_amd.set_exec_mode(prev_exec)


@pytest.mark.parametrize("mode", ["auto", "stream", "stream-local", "stream-fused2", "grouped"])
def test_validation_comes_first_under_stream_batch(scrub_path, mode):
    """The errors of test_scrub_cpu.py's forms, message for message, with the streaming batch
    selected: never a DeviceError (_err), so nothing reached the device."""
    prev_exec = clay_amd.set_exec_mode(mode)
    scrub_path("stream-batch")
    try:
        for cfg in SCRUB_CODES:
            c = ClayCode(*cfg)
            chunk = c.sub_chunk_no * 32
            ref = _err(c.encode_device, [FAKE] * c.k, [FAKE] * c.m, chunk + 1)
            assert isinstance(ref, InvalidChunkSize)
            for e in _forms(c, chunk + 1) + _forms(c, chunk + 1, res=0):
                assert (type(e), e.msg, e.fields) == (type(ref), ref.msg, ref.fields)
            for e in _forms(c, 0):
                assert isinstance(e, InvalidChunkSize)
            for e in _forms(c, chunk, res=0):
                assert isinstance(e, InvalidParameters) and e.msg == "Invalid parameters: null scrub result"
            e1, eb, es = _forms(c, chunk, data=0)
            assert e1.msg == eb.msg == "Invalid parameters: null data chunk"
            assert es.msg == "Invalid parameters: null chunk array"
            e1, eb, es = _forms(c, chunk, par=0)
            assert e1.msg == eb.msg == "Invalid parameters: null parity chunk"
            assert es.msg == "Invalid parameters: null chunk array"
            d = [FAKE] * (c.k * N)
            d[c.k * 3 + 1] = 0
            e = _err(c.scrub_device_batch, d, [FAKE] * (c.m * N), FAKE, N, chunk)
            assert e.msg == "Invalid parameters: null data chunk"
            # no stripes: nothing to do, no device
            c.scrub_device_strided(FAKE, FAKE, FAKE, 0, chunk)
            c.scrub_device_batch([], [], 0, 0, chunk)
        for cfg in NO_KERNEL:  # (9,4,12) among them: still no scrub kernel
            c = ClayCode(*cfg)
            for e in _forms(c, c.sub_chunk_no * 32):
                assert isinstance(e, InvalidParameters) and "(10,4,13)" in e.msg, e.msg
    finally:
        clay_amd.set_exec_mode(prev_exec)
