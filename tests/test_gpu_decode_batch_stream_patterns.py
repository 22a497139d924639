"""Every one- and two-erasure pattern of (10,4,13) through the streaming decode batch
("stream-local256-batch"): all 14 + 91 patterns at sc 520 x 34 stripes, the one launch under exec
mode "stream" bit-equal to a loop of decode_device per stripe under "stream-local"
("stream-local256", the parent's path, which tests/test_gpu_decode_all_patterns.py pins to the
oracle at this size).  Compared on the device.

The other tests of the batch are in tests/test_gpu_batch_decode_stream.py.  This sweep has a file
of its own, named to run after tests/test_gpu_capture_decode.py: that file needs erasure patterns
the process has never decoded, and the pattern tables this sweep uploads stay cached for the life
of the process."""
import itertools

import pytest

import clay_amd
from clay_amd import ClayCode
from test_gpu_batch_decode_stream import BATCH, CFG, FILL, stripes, to_dev

pytestmark = pytest.mark.gpu

SC, N = 520, 34


@pytest.mark.parametrize("r", [1, 2])
def test_every_pattern_equals_the_per_stripe_loop(torch_cuda, r):
    torch = torch_cuda
    c = ClayCode(*CFG)
    assert len(list(itertools.combinations(range(c.n), r))) == (14, 91)[r - 1]
    chunk = c.sub_chunk_no * SC
    host = stripes(SC, N)
    dev = to_dev(torch, host)
    pristine = dev.clone()
    out = torch.empty((N, c.n, chunk), dtype=torch.uint8, device="cuda")
    loop = torch.empty((N, c.n, chunk), dtype=torch.uint8, device="cuda")
    prev = clay_amd.set_exec_mode("stream")
    try:
        for er in itertools.combinations(range(c.n), r):
            er = list(er)
            out.fill_(FILL)
            loop.fill_(FILL)
            clay_amd.set_exec_mode("stream")
            c.decode_device_strided(dev, er, out, N, chunk)
            assert (clay_amd.last_exec_path(), clay_amd.last_launch_count()) == (BATCH, 1), er
            clay_amd.set_exec_mode("stream-local")
            for s in range(N):
                c.decode_device([None if i in er else dev[s, i] for i in range(c.n)], er,
                                [loop[s, i] if i in er else None for i in range(c.n)], chunk)
                assert clay_amd.last_exec_path() == "stream-local256", (er, s)
            torch.cuda.synchronize()
            assert torch.equal(out, loop), (er, "batch differs from the per-stripe loop")
            keep = [i for i in range(c.n) if i not in er]
            assert bool((out[:, keep] == FILL).all().item()), (er, "a row outside the erased slots was written")
            assert bool((out[:, er] != FILL).any().item()), (er, "nothing written")
        assert torch.equal(dev, pristine), "a decode wrote to its input"
    finally:
        clay_amd.set_exec_mode(prev)
