"""GPU parity of the batch of the fused decode v2: many (10,4,13) stripes with the same three or
four erasures in ONE launch of k_stream_fused2's BATCH variant (last exec path
"stream-fused2-batch", clay_last_launch_count() 1 for any number of stripes).

Every stripe gets its own seeded random (NON-codeword) chunks, so a stripe mix-up shows; outputs go
into 0xA5-filled buffers; every test checks that nothing outside the erased slots was written and
that the inputs are unchanged.  The reference of a stripe is OracleClay.decode_chunks of that stripe
alone (data and parity rows), or the per-stripe loop under "stream-fused2" (the parent's path, which
tests/test_gpu_decode_all_patterns.py pins to the oracle at sc 520).

Erasure indices are external: 10..13 are parity (internal 12..15), section = internal node / 4.

Shapes (sc x stripes, 32 workgroups per XCD; tests/test_fused2_batch_map_cpu.py pins them):
512 x 2 (full tiles only), 520 x 34 (16 groups of 2 workgroups run 2-3 stripes each, XCD 4's tile is
8 bytes -- the straddle path --, XCDs 5-7 have none), 2056 x 17 (6 groups of 5, 3 or 2 stripes each,
XCD 6 ends in an 8-byte tile), 16,904 x 3 (one group: slots 0 and 1 run two tiles per stripe and
every workgroup crosses two stripe boundaries with the ring streaming).

This file sorts after tests/test_gpu_decode_all_patterns.py, which decodes every pattern: the
pattern tables are cached for the life of the process and tests/test_gpu_capture_decode.py needs
cold ones.  The every-pattern sweep of the batch is in tests/test_gpu_decode_batch_fused2_patterns.py."""
import numpy as np
import pytest

import clay_amd
from clay_amd import ClayCode
from test_gpu_batch_decode_stream import FILL, check_rows, oracle_rows, stripes, to_dev

pytestmark = pytest.mark.gpu

CFG = (10, 4, 13)
BATCH = "stream-fused2-batch"
LOCAL_BATCH = "stream-local256-batch"
STAGED_MAX = 4 << 20  # the staged batch's bound on a stripe's data (engine.hip kBatchMaxStripeBytes)

# non-TWO with 4 and 3 erasures, parity among the lost, TWO with (2,1,1) and (2,2) sections; the
# last one is a (2,1,1) pattern with a split step (sections 0 and 1 keep 4 + 3 nodes, the ring has
# 6 buffers): its second barrier runs across stripe boundaries
# (tests/test_fused2_batch_gate_cpu.py checks these statements against tests/decode_pattern.py)
PATTERNS = [(0, 4, 8, 12), (1, 5, 9, 13), (0, 4, 8), (3, 7, 10), (0, 1, 4, 8), (0, 1, 4, 5), (8, 9, 0, 4), (4, 8, 9, 10)]
SIZES = [(512, 2), (520, 34), (2056, 17)]


def run_strided(torch, c, host, er, chunk, mode):
    """decode_device_strided of a contiguous [n][14][chunk] batch into a separate 0xA5-filled buffer
    of the same layout under exec mode `mode` -> (out on the host, path, launches)."""
    prev = clay_amd.set_exec_mode(mode)
    try:
        n = host.shape[0]
        dev = to_dev(torch, host)
        out = torch.full((n, c.n, chunk), FILL, dtype=torch.uint8, device="cuda")
        c.decode_device_strided(dev, list(er), out, n, chunk)
        torch.cuda.synchronize()
        path, launches = clay_amd.last_exec_path(), clay_amd.last_launch_count()
        assert np.array_equal(dev.cpu().numpy(), host), "inputs changed"
        return out.cpu().numpy(), path, launches
    finally:
        clay_amd.set_exec_mode(prev)


# ---------------------------------------------------------------------------
# 1. path and bytes against the oracle
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("er", PATTERNS, ids=lambda e: "e" + "_".join(map(str, e)))
@pytest.mark.parametrize("sc,n", SIZES)
def test_batch_path_and_oracle(oracle_mod, torch_cuda, sc, n, er):
    c = ClayCode(*CFG)
    chunk = c.sub_chunk_no * sc
    host = stripes(sc, n)
    got, path, launches = run_strided(torch_cuda, c, host, er, chunk, "stream")
    assert path == BATCH, (sc, n, er, path)
    assert launches == 1, (sc, n, er, launches)
    ref = oracle_rows(oracle_mod, host, er, key=(sc, n, er) if sc == 520 else None)
    check_rows(got, ref, er, (sc, n, er))


# ---------------------------------------------------------------------------
# 2. two tiles per workgroup and stripe
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("er", [(0, 4, 8, 12), (0, 1, 4, 8)], ids=lambda e: "e" + "_".join(map(str, e)))
def test_large_shape(oracle_mod, torch_cuda, er):
    """16,904 x 3: one group of 32 workgroups per XCD; slots 0 and 1 run two tiles per stripe, every
    workgroup crosses two stripe boundaries.  Bit-equal to the per-stripe loop under
    "stream-fused2" for all three stripes, and to the oracle for stripe 1."""
    torch = torch_cuda
    sc, n = 16904, 3
    c = ClayCode(*CFG)
    chunk = c.sub_chunk_no * sc
    host = stripes(sc, n)
    got, path, launches = run_strided(torch, c, host, er, chunk, "stream")
    assert (path, launches) == (BATCH, 1), (path, launches)
    loop, path, launches = run_strided(torch, c, host, er, chunk, "stream-fused2")
    assert (path, launches) == ("stream-fused2", n), (path, launches)
    assert np.array_equal(got, loop), "batch differs from the per-stripe loop"
    keep = [i for i in range(c.n) if i not in er]
    assert bool((got[:, keep] == FILL).all()), "a row outside the erased slots was written"
    ref = oracle_rows(oracle_mod, host[1:2], er)
    for j, e in enumerate(er):
        assert np.array_equal(got[1, e], ref[0, j]), ("stripe 1", "node", e)


# ---------------------------------------------------------------------------
# 3. layouts
# ---------------------------------------------------------------------------
def test_layouts(oracle_mod, torch_cuda):
    """Own input and output strides with gaps, in place, the pointer-array form on rows of one tensor
    (one launch each); separately allocated stripes, a stripe stride off 8 bytes and sc 516 (not the
    batch, the same bytes)."""
    torch = torch_cuda
    sc, n, er = 520, 34, (0, 4, 8, 12)
    c = ClayCode(*CFG)
    chunk = c.sub_chunk_no * sc
    host = stripes(sc, n)
    ref = oracle_rows(oracle_mod, host, er, key=(sc, n, er))
    prev = clay_amd.set_exec_mode("stream")
    try:
        def lay(ns_, ss_):
            """Input buffer: the stripes at these strides, 0xA5 elsewhere (the erased nodes' slots
            too: they must never be read)."""
            b = np.full(n * ss_, FILL, np.uint8)
            for s in range(n):
                for i in range(c.n):
                    if i not in er:
                        p = s * ss_ + i * ns_
                        b[p:p + chunk] = host[s, i]
            return b

        def expect_out(ons, oss):
            b = np.full(n * oss, FILL, np.uint8)
            for s in range(n):
                for j, e in enumerate(er):
                    p = s * oss + e * ons
                    b[p:p + chunk] = ref[s, j]
            return b

        ns_, ss_ = chunk + 24, c.n * (chunk + 24) + 40   # input node / stripe strides (multiples of 8)
        ons, oss = chunk + 8, c.n * (chunk + 8) + 16     # output strides
        src = lay(ns_, ss_)
        buf = torch.from_numpy(src).cuda()
        out = torch.full((n * oss,), FILL, dtype=torch.uint8, device="cuda")
        c.decode_device_strided(buf, list(er), out, n, chunk, ns_, ss_, ons, oss)
        torch.cuda.synchronize()
        assert (clay_amd.last_exec_path(), clay_amd.last_launch_count()) == (BATCH, 1)
        assert np.array_equal(buf.cpu().numpy(), src), "input buffer changed"
        assert np.array_equal(out.cpu().numpy(), expect_out(ons, oss)), "separate output with its own strides"
        # in place: out == chunks, same strides; only the erased slots change
        c.decode_device_strided(buf, list(er), buf, n, chunk, ns_, ss_, ns_, ss_)
        torch.cuda.synchronize()
        assert (clay_amd.last_exec_path(), clay_amd.last_launch_count()) == (BATCH, 1)
        want = src.copy()
        for s in range(n):
            for j, e in enumerate(er):
                p = s * ss_ + e * ns_
                want[p:p + chunk] = ref[s, j]
        assert np.array_equal(buf.cpu().numpy(), want), "in place"

        # pointer arrays on rows of one tensor: uniform strides -> one launch
        dev = to_dev(torch, host)
        out = torch.full((n, len(er), chunk), FILL, dtype=torch.uint8, device="cuda")
        c.decode_device_batch([None if i in er else dev[s, i] for s in range(n) for i in range(c.n)], list(er),
                              [out[s, er.index(i)] if i in er else None for s in range(n) for i in range(c.n)], n, chunk)
        torch.cuda.synchronize()
        assert (clay_amd.last_exec_path(), clay_amd.last_launch_count()) == (BATCH, 1)
        assert np.array_equal(out.cpu().numpy(), ref)
        assert np.array_equal(dev.cpu().numpy(), host), "inputs changed"

        # separately allocated stripes in a shuffled order: no common stride -> not the one launch
        order = np.random.default_rng(7).permutation(n)
        parts = {int(s): to_dev(torch, host[s]) for s in order}
        outs = {int(s): torch.full((len(er), chunk + 16 * (int(s) % 3)), FILL, dtype=torch.uint8, device="cuda")
                for s in order}
        c.decode_device_batch([None if i in er else parts[s][i] for s in range(n) for i in range(c.n)], list(er),
                              [outs[s][er.index(i), :chunk] if i in er else None for s in range(n) for i in range(c.n)],
                              n, chunk)
        torch.cuda.synchronize()
        path, launches = clay_amd.last_exec_path(), clay_amd.last_launch_count()
        assert path != BATCH and launches > 1, (path, launches)
        for s in range(n):
            assert np.array_equal(outs[s][:, :chunk].cpu().numpy(), ref[s]), s
            assert bool((outs[s][:, chunk:] == FILL).all().item()), s
            assert np.array_equal(parts[s].cpu().numpy(), host[s]), ("inputs changed", s)

        # a stripe stride that is not a multiple of 8: stripes 1, 3, ... are off 8-byte rows
        ns_, ss_ = chunk, c.n * chunk + 12
        src = lay(ns_, ss_)
        buf = torch.from_numpy(src).cuda()
        out = torch.full((n * ss_,), FILL, dtype=torch.uint8, device="cuda")
        c.decode_device_strided(buf, list(er), out, n, chunk, ns_, ss_, ns_, ss_)
        torch.cuda.synchronize()
        path, launches = clay_amd.last_exec_path(), clay_amd.last_launch_count()
        assert path != BATCH and launches > 1, (path, launches)
        assert np.array_equal(buf.cpu().numpy(), src), "input buffer changed"
        assert np.array_equal(out.cpu().numpy(), expect_out(ns_, ss_)), "stripe stride off 8 bytes"
    finally:
        clay_amd.set_exec_mode(prev)

    # sc 516: rows off 8-byte multiples
    sc = 516
    chunk = c.sub_chunk_no * sc
    host = stripes(sc, n)
    ref = oracle_rows(oracle_mod, host, er)
    got, path, launches = run_strided(torch, c, host, er, chunk, "stream")
    assert path != BATCH and launches > 1, (path, launches)
    check_rows(got, ref, er, ("sc 516",))


# ---------------------------------------------------------------------------
# 4. modes
# ---------------------------------------------------------------------------
def test_modes(oracle_mod, torch_cuda):
    torch = torch_cuda
    sc, n, er = 2048, 8, (0, 4, 8, 12)
    c = ClayCode(*CFG)
    chunk = c.sub_chunk_no * sc
    assert c.k * chunk > STAGED_MAX  # 5 MiB of data per stripe: above the staged batch
    host = stripes(sc, n)
    ref = oracle_rows(oracle_mod, host, er)
    loop, path, launches = run_strided(torch, c, host, er, chunk, "stream-fused2")
    assert (path, launches) == ("stream-fused2", n), (path, launches)
    check_rows(loop, ref, er, "stream-fused2")
    batch, path, launches = run_strided(torch, c, host, er, chunk, "stream")
    assert (path, launches) == (BATCH, 1), (path, launches)
    # above 4 MiB the staged batch does not apply: "grouped" is its per-stripe loop
    grouped, path, launches = run_strided(torch, c, host, er, chunk, "grouped")
    assert path == "grouped" and launches >= n and launches % n == 0, (path, launches)
    assert np.array_equal(batch, loop) and np.array_equal(batch, grouped)
    # the modes that never take it
    for mode in ("stream-local", "tile"):
        got, path, launches = run_strided(torch, c, host, er, chunk, mode)
        assert path != BATCH and launches >= n, (mode, path, launches)
        assert np.array_equal(got, batch), mode
    # auto: whatever the committed gate says (clay_amd.DECODE_FUSED2_BATCH_AUTO_MAX_SC restates the
    # engine's constant: tests/test_fused2_batch_gate_cpu.py)
    auto, path, launches = run_strided(torch, c, host, er, chunk, "auto")
    if sc <= clay_amd.DECODE_FUSED2_BATCH_AUTO_MAX_SC:
        assert (path, launches) == (BATCH, 1), (path, launches)
    else:
        assert (path, launches) == ("stream-fused2", n), (path, launches)
    assert np.array_equal(auto, batch)
    # auto at 520 x 34 (1.3 MiB stripes): the staged batch, as before
    sc, n = 520, 34
    chunk = c.sub_chunk_no * sc
    host = stripes(sc, n)
    got, path, _ = run_strided(torch, c, host, er, chunk, "auto")
    assert path == "grouped-batch", path
    check_rows(got, oracle_rows(oracle_mod, host, er, key=(sc, n, er)), er, "auto 520 x 34")
    # one and two erasures under "stream": still the local decode's batch
    for few in ((0,), (0, 4)):
        got, path, launches = run_strided(torch, c, host, few, chunk, "stream")
        assert (path, launches) == (LOCAL_BATCH, 1), (few, path, launches)
        check_rows(got, oracle_rows(oracle_mod, host, few, key=(sc, n, few)), few, ("stream", few))


# ---------------------------------------------------------------------------
# 5. capture
# ---------------------------------------------------------------------------
def test_graph_capture(oracle_mod, torch_cuda):
    """After one warm call of the pattern (its table upload) the batch is captured on a side stream
    as one launch and replayed on fresh inputs written into the same buffers, bit-exact against the
    oracle.  There is no cold-pattern case here: this file runs after
    tests/test_gpu_decode_all_patterns.py, which decodes every pattern, and the pattern tables are
    cached for the life of the process, so no pattern is cold."""
    torch = torch_cuda
    sc, n, er = 520, 34, (0, 4, 8, 12)
    c = ClayCode(*CFG)
    chunk = c.sub_chunk_no * sc
    data = torch.zeros((n, c.n, chunk), dtype=torch.uint8, device="cuda")
    out = torch.full((n, c.n, chunk), FILL, dtype=torch.uint8, device="cuda")
    st = torch.cuda.Stream()
    prev = clay_amd.set_exec_mode("stream")
    try:
        with torch.cuda.stream(st):  # warm call outside the capture
            c.decode_device_strided(data, list(er), out, n, chunk, device=0, stream=st.cuda_stream)
        st.synchronize()
        assert clay_amd.last_exec_path() == BATCH
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=st):
            c.decode_device_strided(data, list(er), out, n, chunk, device=0,
                                    stream=torch.cuda.current_stream().cuda_stream)
        assert (clay_amd.last_exec_path(), clay_amd.last_launch_count()) == (BATCH, 1)
        host = stripes(sc, n)
        data.copy_(to_dev(torch, host))
        out.fill_(FILL)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        check_rows(out.cpu().numpy(), oracle_rows(oracle_mod, host, er, key=(sc, n, er)), er, "replay")
        assert np.array_equal(data.cpu().numpy(), host), "inputs changed"
        del g
        torch.cuda.synchronize()
    finally:
        clay_amd.set_exec_mode(prev)
