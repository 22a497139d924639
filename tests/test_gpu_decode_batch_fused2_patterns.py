"""Every pattern of (10,4,13) that exec mode "stream" runs on k_stream_fused2, through the batch of
that kernel ("stream-fused2-batch"): 352 of the 364 three-erasure and 878 of the 1,001 four-erasure
patterns at sc 520 x 34 stripes, the one launch under "stream" bit-equal on the device to a loop of
decode_device per stripe under "stream-fused2" (the parent's path, which
tests/test_gpu_decode_all_patterns.py pins to the oracle at this size).

Parametrized by (erasure count, whether a y-section holds two erasures -- the TWO instantiation) so
that each case stays at a few seconds.  The other tests of the batch are in
tests/test_gpu_decode_batch_fused2.py; both files sort after tests/test_gpu_decode_all_patterns.py
(the pattern tables this sweep uploads stay cached for the life of the process, and
tests/test_gpu_capture_decode.py needs cold patterns)."""
import itertools

import pytest

import clay_amd
import decode_pattern
from clay_amd import ClayCode
from test_gpu_batch_decode_stream import CFG, FILL, stripes, to_dev

pytestmark = pytest.mark.gpu

SC, N = 520, 34
BATCH = "stream-fused2-batch"


def _patterns(r):
    c = decode_pattern.code(10)
    return [list(er) for er in itertools.combinations(range(c.n), r)
            if decode_pattern.expected_kernel(c, list(er), "stream") == "fused2"]


def test_pattern_counts():
    assert (len(_patterns(3)), len(_patterns(4))) == (352, 878)


@pytest.mark.parametrize("r,two", [(3, False), (3, True), (4, False), (4, True)])
def test_every_pattern_equals_the_per_stripe_loop(torch_cuda, r, two):
    torch = torch_cuda
    c = ClayCode(*CFG)
    pats = [er for er in _patterns(r) if (max(decode_pattern.per_section(c, er)) == 2) == two]
    assert pats
    chunk = c.sub_chunk_no * SC
    host = stripes(SC, N)
    dev = to_dev(torch, host)
    pristine = dev.clone()
    out = torch.empty((N, c.n, chunk), dtype=torch.uint8, device="cuda")
    loop = torch.empty((N, c.n, chunk), dtype=torch.uint8, device="cuda")
    prev = clay_amd.set_exec_mode("stream")
    try:
        for er in pats:
            out.fill_(FILL)
            loop.fill_(FILL)
            clay_amd.set_exec_mode("stream")
            c.decode_device_strided(dev, er, out, N, chunk)
            assert (clay_amd.last_exec_path(), clay_amd.last_launch_count()) == (BATCH, 1), er
            clay_amd.set_exec_mode("stream-fused2")
            for s in range(N):
                c.decode_device([None if i in er else dev[s, i] for i in range(c.n)], er,
                                [loop[s, i] if i in er else None for i in range(c.n)], chunk)
                assert clay_amd.last_exec_path() == "stream-fused2", (er, s)
            torch.cuda.synchronize()
            assert torch.equal(out, loop), (er, "batch differs from the per-stripe loop")
            keep = [i for i in range(c.n) if i not in er]
            assert bool((out[:, keep] == FILL).all().item()), (er, "a row outside the erased slots was written")
            assert bool((out[:, er] != FILL).any().item()), (er, "nothing written")
        assert torch.equal(dev, pristine), "a decode wrote to its input"
    finally:
        clay_amd.set_exec_mode(prev)
