"""GPU parity of the batched decode (clay_decode_device_strided / clay_decode_device_batch): many
stripes with the same erasure set in one call.

 * line batch: (4,2,5) with one erasure runs ONE launch of the column-flattened k_bs_decode1
   ("bs-decode1-batch") at any sub-chunk size and alignment;
 * staged batch: every other code / pattern / layout runs the cached decode plan as one k_gexec
   launch per level for the whole batch ("grouped-batch");
 * stripes of more than 4 MiB of data, and fewer than 4 stripes off the line batch, run stripe by
   stripe.

Every stripe gets its own seeded random (NON-codeword) chunks, so a stripe mix-up shows, and every
erased data node is compared with the oracle's decode of that stripe alone.  The oracle's decode
returns data nodes only: erased parity nodes are compared with the per-stripe clay_decode_device
under "grouped" on the same random inputs, and with the oracle's encode on codewords (even
sub-chunks only: the oracle pads odd ones)."""
import numpy as np
import pytest

import clay_amd
from clay_amd import ClayCode

pytestmark = pytest.mark.gpu

FILL = 0xA5

# (sc, n_stripes) of the line batch: one full column per stripe (64 stripes per workgroup); one
# partial column and a last workgroup with 3 of 64 columns; two columns, the second partial; 10
# columns per stripe (stripes straddle workgroups); byte tails; more than one tile per stripe with
# a partial last column; byte tails across tiles
LINE_CASES = [(32, 300), (8, 67), (40, 67), (320, 37), (777, 5), (2048 + 8 * 37, 5), (2 * 2048 + 5, 3)]

_inputs = {}
_refs = {}


def stripes(cfg, sc, n):
    """(n, nodes, chunk) random bytes, stripe s from its own seed.  Shared, never modified."""
    key = (cfg, sc, n)
    if key not in _inputs:
        c = ClayCode(*cfg)
        chunk = c.sub_chunk_no * sc
        a = np.stack([np.random.default_rng([sc, n, s, cfg[0]]).integers(0, 256, (c.n, chunk), dtype=np.uint8)
                      for s in range(n)])
        a.setflags(write=False)
        _inputs[key] = a
    return _inputs[key]


def oracle_data(oracle_mod, cfg, sc, n, er):
    """(n, k, chunk): the oracle's decode of every stripe of stripes(cfg, sc, n) with `er` erased."""
    key = (cfg, sc, n, tuple(er))
    if key not in _refs:
        c, o = ClayCode(*cfg), oracle_mod.OracleClay(*cfg)
        a = stripes(cfg, sc, n)
        r = np.stack([np.frombuffer(o.decode({i: a[s, i] for i in range(c.n) if i not in er}, list(er)),
                                    np.uint8).reshape(c.k, -1) for s in range(n)])
        r.setflags(write=False)
        _refs[key] = r
    return _refs[key]


def to_dev(torch, a):
    return torch.from_numpy(np.array(a)).cuda()  # a writable copy: the shared inputs are read-only


def run_strided(torch, c, host, er, chunk, mode=None):
    """decode_device_strided of a contiguous [n][nodes][chunk] batch into a separate 0xA5-filled
    buffer of the same layout -> (out, path, launches)."""
    prev = clay_amd.set_exec_mode(mode) if mode else None
    try:
        n = host.shape[0]
        dev = to_dev(torch, host)
        out = torch.full((n, c.n, chunk), FILL, dtype=torch.uint8, device="cuda")
        c.decode_device_strided(dev, er, out, n, chunk)
        torch.cuda.synchronize()
        path, launches = clay_amd.last_exec_path(), clay_amd.last_launch_count()
        assert np.array_equal(dev.cpu().numpy(), host), "inputs changed"
        return out.cpu().numpy(), path, launches
    finally:
        if prev is not None:
            clay_amd.set_exec_mode(prev)


def per_stripe(torch, c, host, er, chunk, mode=None):
    """The parent's only way: one decode_device per stripe -> (out [n][nodes][chunk], last path)."""
    prev = clay_amd.set_exec_mode(mode) if mode else None
    try:
        n = host.shape[0]
        dev = to_dev(torch, host)
        out = torch.full((n, c.n, chunk), FILL, dtype=torch.uint8, device="cuda")
        for s in range(n):
            c.decode_device([None if i in er else dev[s, i] for i in range(c.n)], er,
                            [out[s, i] if i in er else None for i in range(c.n)], chunk)
        torch.cuda.synchronize()
        return out.cpu().numpy(), clay_amd.last_exec_path()
    finally:
        if prev is not None:
            clay_amd.set_exec_mode(prev)


def untouched(out, er):
    keep = [i for i in range(out.shape[1]) if i not in er]
    return bool((out[:, keep] == FILL).all())


# ---------------------------------------------------------------------------
# 1. line batch, data nodes
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("sc,n", LINE_CASES)
def test_line_batch_data_nodes(oracle_mod, torch_cuda, sc, n):
    cfg = (4, 2, 5)
    c = ClayCode(*cfg)
    chunk = c.sub_chunk_no * sc
    host = stripes(cfg, sc, n)
    for e in range(c.k):
        got, path, launches = run_strided(torch_cuda, c, host, [e], chunk)
        assert path == "bs-decode1-batch", (e, path)
        assert launches == 1, (e, launches)
        ref = oracle_data(oracle_mod, cfg, sc, n, [e])
        for s in range(n):
            assert np.array_equal(got[s, e], ref[s, e]), (sc, n, e, s)
        assert untouched(got, [e]), (sc, n, e)


# ---------------------------------------------------------------------------
# 2. line batch, parity nodes
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("sc,n", LINE_CASES)
def test_line_batch_parity_nodes(oracle_mod, torch_cuda, sc, n):
    cfg = (4, 2, 5)
    c, o = ClayCode(*cfg), oracle_mod.OracleClay(*cfg)
    chunk = c.sub_chunk_no * sc
    host = stripes(cfg, sc, n)
    if sc % 2 == 0:  # codewords (the oracle pads odd sub-chunks to the next even one)
        cw = np.stack([o.encode_array(host[s, :c.k].reshape(-1).tobytes()) for s in range(n)])
        assert cw.shape == (n, c.n, chunk)
        for e in (c.k, c.k + 1):
            got, path, launches = run_strided(torch_cuda, c, cw, [e], chunk)
            assert (path, launches) == ("bs-decode1-batch", 1), (e, path, launches)
            assert np.array_equal(got[:, e], cw[:, e]), (sc, n, e)
    for e in (c.k, c.k + 1):  # random inputs: the per-stripe grouped executor
        got, path, launches = run_strided(torch_cuda, c, host, [e], chunk)
        assert (path, launches) == ("bs-decode1-batch", 1), (e, path, launches)
        ref, rpath = per_stripe(torch_cuda, c, host, [e], chunk, mode="grouped")
        assert rpath == "grouped", rpath
        assert np.array_equal(got, ref), (sc, n, e)


# ---------------------------------------------------------------------------
# 3. layouts
# ---------------------------------------------------------------------------
def test_line_batch_layouts(oracle_mod, torch_cuda):
    """Padded node / stripe strides, a separate output buffer with its own strides, in place,
    an unaligned base (byte-tail instantiation), and the pointer-array form."""
    torch = torch_cuda
    cfg, sc, n, e = (4, 2, 5), 40, 67, 1
    c = ClayCode(*cfg)
    chunk = c.sub_chunk_no * sc
    host = stripes(cfg, sc, n)
    ref = oracle_data(oracle_mod, cfg, sc, n, [e])[:, e]
    ns_, ss_ = chunk + 24, c.n * (chunk + 24) + 40   # input node / stripe strides
    ons, oss = chunk + 8, c.n * (chunk + 8) + 16     # output strides

    def lay(off):
        """Input buffer: the stripes at the strides above from byte `off`, 0xA5 elsewhere (the
        erased node's slot too: it must never be read)."""
        b = np.full(off + n * ss_, FILL, np.uint8)
        for s in range(n):
            for i in range(c.n):
                if i != e:
                    p = off + s * ss_ + i * ns_
                    b[p:p + chunk] = host[s, i]
        return b

    def expect_out(off):
        b = np.full(off + n * oss, FILL, np.uint8)
        for s in range(n):
            p = off + s * oss + e * ons
            b[p:p + chunk] = ref[s]
        return b

    for off in (0, 3):  # 3: every pointer off 8-byte alignment -> the byte-tail instantiation
        src = lay(off)
        buf = torch.from_numpy(src).cuda()
        out = torch.full((off + n * oss,), FILL, dtype=torch.uint8, device="cuda")
        c.decode_device_strided(buf[off:], [e], out[off:], n, chunk, ns_, ss_, ons, oss)
        torch.cuda.synchronize()
        assert clay_amd.last_exec_path() == "bs-decode1-batch" and clay_amd.last_launch_count() == 1
        assert np.array_equal(buf.cpu().numpy(), src), ("input buffer changed", off)
        assert np.array_equal(out.cpu().numpy(), expect_out(off)), ("separate output", off)
        # in place: out == chunks, same strides; only the erased slots change
        c.decode_device_strided(buf[off:], [e], buf[off:], n, chunk, ns_, ss_, ns_, ss_)
        torch.cuda.synchronize()
        assert clay_amd.last_exec_path() == "bs-decode1-batch" and clay_amd.last_launch_count() == 1
        want = src.copy()
        for s in range(n):
            p = off + s * ss_ + e * ns_
            want[p:p + chunk] = ref[s]
        assert np.array_equal(buf.cpu().numpy(), want), ("in place", off)

    # pointer arrays: rows of one tensor are uniform strides -> the line batch
    dev = to_dev(torch, host)
    out = torch.full((n, chunk), FILL, dtype=torch.uint8, device="cuda")
    c.decode_device_batch([None if i == e else dev[s, i] for s in range(n) for i in range(c.n)], [e],
                          [out[s] if i == e else None for s in range(n) for i in range(c.n)], n, chunk)
    torch.cuda.synchronize()
    assert clay_amd.last_exec_path() == "bs-decode1-batch" and clay_amd.last_launch_count() == 1
    assert np.array_equal(out.cpu().numpy(), ref)
    # separately allocated stripes in a shuffled order: not affine -> the device pointer table
    order = np.random.default_rng(7).permutation(n)
    parts = {int(s): to_dev(torch, host[s]) for s in order}
    outs = {int(s): torch.full((chunk + 16 * (int(s) % 3),), FILL, dtype=torch.uint8, device="cuda") for s in order}
    c.decode_device_batch([None if i == e else parts[s][i] for s in range(n) for i in range(c.n)], [e],
                          [outs[s] if i == e else None for s in range(n) for i in range(c.n)], n, chunk)
    torch.cuda.synchronize()
    assert clay_amd.last_exec_path() == "grouped-batch"
    for s in range(n):
        assert np.array_equal(outs[s][:chunk].cpu().numpy(), ref[s]), s


# ---------------------------------------------------------------------------
# 4. staged batch, other codes
# ---------------------------------------------------------------------------
STAGED = [((10, 4, 13), (0, 4, 8, 12), 32, 37), ((10, 4, 13), (0, 4, 8, 12), 2, 300),
          ((10, 4, 13), (0,), 32, 37), ((10, 4, 13), (0,), 2, 300),
          ((9, 3, 11), (0, 1), 320, 9), ((6, 3, 8), (0, 8), 16 * 70 + 6, 5), ((5, 3, 6), (1,), 32, 301)]


@pytest.mark.parametrize("cfg,er,sc,n", STAGED)
def test_staged_batch_other_codes(oracle_mod, torch_cuda, cfg, er, sc, n):
    c = ClayCode(*cfg)
    er = list(er)  # (6,3,8): {0, n - 1}
    chunk = c.sub_chunk_no * sc
    host = stripes(cfg, sc, n)
    got, path, _ = run_strided(torch_cuda, c, host, er, chunk)
    assert path == "grouped-batch", path
    ref = oracle_data(oracle_mod, cfg, sc, n, er)
    for e in er:
        if e < c.k:
            assert np.array_equal(got[:, e], ref[:, e]), (cfg, er, e)
    if any(e >= c.k for e in er):
        single, spath = per_stripe(torch_cuda, c, host, er, chunk, mode="grouped")
        assert spath == "grouped", spath
        for e in er:
            if e >= c.k:
                assert np.array_equal(got[:, e], single[:, e]), (cfg, er, e)
    assert untouched(got, er), (cfg, er)


@pytest.mark.parametrize("cfg,er", [((10, 4, 13), (0, 4, 8, 12)), ((10, 4, 13), (0,)), ((9, 3, 11), (0, 1)),
                                    ((6, 3, 8), (0, 8)), ((5, 3, 6), (1,))])
def test_staged_batch_launches_independent_of_stripes(torch_cuda, cfg, er):
    c = ClayCode(*cfg)
    sc = 32
    chunk = c.sub_chunk_no * sc
    counts = []
    for n in (5, 37):
        _, path, launches = run_strided(torch_cuda, c, stripes(cfg, sc, n), list(er), chunk)
        assert path == "grouped-batch", path
        counts.append(launches)
    assert counts[0] == counts[1] and counts[0] >= 1, counts


# ---------------------------------------------------------------------------
# 5. A/B: the line batch's partner
# ---------------------------------------------------------------------------
def test_grouped_mode_is_the_ab_partner(torch_cuda):
    cfg, sc, n = (4, 2, 5), 320, 37
    c = ClayCode(*cfg)
    chunk = c.sub_chunk_no * sc
    host = stripes(cfg, sc, n)
    for e in (0, 3, 5):
        auto, apath, _ = run_strided(torch_cuda, c, host, [e], chunk)
        grouped, gpath, _ = run_strided(torch_cuda, c, host, [e], chunk, mode="grouped")
        assert (apath, gpath) == ("bs-decode1-batch", "grouped-batch"), (apath, gpath)
        assert np.array_equal(auto, grouped), e


# ---------------------------------------------------------------------------
# 6. fallback: few stripes, large stripes
# ---------------------------------------------------------------------------
def test_fallback_few_or_large_stripes(torch_cuda):
    cfg = (4, 2, 5)
    c = ClayCode(*cfg)
    # two stripes: the line batch has no minimum (one launch), the staged batch starts at four
    sc, n = 320, 2
    chunk = c.sub_chunk_no * sc
    host = stripes(cfg, sc, n)
    got, path, launches = run_strided(torch_cuda, c, host, [2], chunk)
    ref, rpath = per_stripe(torch_cuda, c, host, [2], chunk)
    assert (path, launches, rpath) == ("bs-decode1-batch", 1, "bs-decode1"), (path, launches, rpath)
    assert np.array_equal(got, ref)
    c2 = ClayCode(6, 3, 8)
    chunk = c2.sub_chunk_no * sc
    host = stripes((6, 3, 8), sc, n)
    got, path, _ = run_strided(torch_cuda, c2, host, [0, 8], chunk)
    ref, rpath = per_stripe(torch_cuda, c2, host, [0, 8], chunk)
    assert path == rpath != "grouped-batch", (path, rpath)
    assert np.array_equal(got, ref)
    # four stripes of more than 4 MiB of data each
    sc, n = (1 << 17) + 8, 4
    chunk = c.sub_chunk_no * sc
    assert c.k * chunk > 4 << 20
    host = stripes(cfg, sc, n)
    got, path, launches = run_strided(torch_cuda, c, host, [0], chunk)
    ref, rpath = per_stripe(torch_cuda, c, host, [0], chunk)
    assert path == rpath == "bs-decode1" and launches == n, (path, rpath, launches)
    assert np.array_equal(got, ref)


# ---------------------------------------------------------------------------
# 7. capture
# ---------------------------------------------------------------------------
def test_line_batch_graph_capture(oracle_mod, torch_cuda):
    """The line batch allocates nothing and needs no pointer table: after one warm call it is
    captured on a side stream (one kernel node) and replayed on fresh input written into the same
    buffers, bit-exact against the oracle."""
    torch = torch_cuda
    cfg, sc, n, e = (4, 2, 5), 32, 300, 0
    c = ClayCode(*cfg)
    chunk = c.sub_chunk_no * sc
    data = torch.zeros((n, c.n, chunk), dtype=torch.uint8, device="cuda")
    out = torch.full((n, c.n, chunk), FILL, dtype=torch.uint8, device="cuda")
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):  # warm call outside the capture
        c.decode_device_strided(data, [e], out, n, chunk, device=0, stream=st.cuda_stream)
    st.synchronize()
    assert clay_amd.last_exec_path() == "bs-decode1-batch"
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=st):
        c.decode_device_strided(data, [e], out, n, chunk, device=0,
                                stream=torch.cuda.current_stream().cuda_stream)
    assert clay_amd.last_exec_path() == "bs-decode1-batch" and clay_amd.last_launch_count() == 1
    host = stripes(cfg, sc, n)
    data.copy_(to_dev(torch, host))
    out.fill_(FILL)
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    ref = oracle_data(oracle_mod, cfg, sc, n, [e])
    assert np.array_equal(got[:, e], ref[:, e])
    assert untouched(got, [e])
