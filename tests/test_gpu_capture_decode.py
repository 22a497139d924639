"""A decode inside a stream capture: prepared by one eager call it allocates nothing and replays
bit-exact; a pattern the process has never decoded fails inside the capture with a clear error.

This file runs before tests/test_gpu_decode_all_patterns.py (pytest runs the files in name order)
because of that last step: the plan uploads and the streaming-decode pattern tables are cached for
the life of the process, so once that file has decoded every erasure pattern of (10,4,13) no
pattern is left that was "never run before"."""
import numpy as np
import pytest

import clay_amd
from clay_amd import ClayCode
from test_gpu_runtime import _stripe

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("mode,path,er,er2", [("grouped", "grouped", [0, 4, 8, 12], [1, 5, 9, 13]),
                                              ("auto", "stream-fused2", [0, 4, 8, 12], [1, 5, 9, 13]),
                                              ("auto", "stream-local256", [0, 4], [1, 5])])
def test_decode_graph_capture_after_prepare(oracle_mod, torch_cuda, mode, path, er, er2):
    """A (10,4,13) decode inside a stream capture, on the grouped executor (its U workspace lease
    covered by the reserved workspace), on the fused decode v2 and on the local decode on 256-byte
    runs (no workspace): one eager call of the pattern prepared its tables, so the capture
    allocates nothing (the pool does not grow) and replays bit-exact on new data.  A pattern never
    run before fails inside the capture with a clear error instead of invalidating it."""
    prev = clay_amd.set_exec_mode(mode)
    try:
        _decode_graph_capture(oracle_mod, torch_cuda, path, er, er2)
    finally:
        clay_amd.set_exec_mode(prev)


def _decode_graph_capture(oracle_mod, torch_cuda, path, er, er2):
    torch = torch_cuda
    c, o = ClayCode(10, 4, 13), oracle_mod.OracleClay(10, 4, 13)
    sc = 1024
    chunk = c.sub_chunk_no * sc
    st = torch.cuda.Stream()
    clay_amd.release_captured(0)
    clay_amd.release_workspace(0)
    c.reserve_workspace(chunk)
    reserved = clay_amd.workspace_bytes(0)
    assert reserved >= c.q * c.t * chunk
    full = torch.from_numpy(_stripe(o, 10, chunk, 77)).cuda()
    outs = torch.zeros((14, chunk), dtype=torch.uint8, device="cuda")
    args = ([None if j in er else full[j] for j in range(14)], er, [outs[j] if j in er else None for j in range(14)])
    c.decode_device(*args, chunk, 0, st.cuda_stream)  # prepares the pattern's tables
    st.synchronize()
    assert clay_amd.last_exec_path() == path
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=st):
        c.decode_device(*args, chunk, 0, torch.cuda.current_stream().cuda_stream)
    assert clay_amd.workspace_bytes(0) == reserved
    for rep in range(2):
        ref = _stripe(o, 10, chunk, 780 + rep)
        full.copy_(torch.from_numpy(ref))
        outs.fill_(0xA5)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        for e in er:
            assert np.array_equal(outs[e].cpu().numpy(), ref[e]), (rep, e)
    g2 = torch.cuda.CUDAGraph()
    with pytest.raises(clay_amd.DeviceError, match="not prepared"):
        with torch.cuda.graph(g2, stream=st):
            c.decode_device([None if j in er2 else full[j] for j in range(14)], er2,
                            [outs[j] if j in er2 else None for j in range(14)], chunk, 0,
                            torch.cuda.current_stream().cuda_stream)
    del g, g2
    torch.cuda.synchronize()
    clay_amd.release_captured(0)
