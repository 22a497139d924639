"""GPU parity of the batched repair (clay_repair_device_strided / clay_repair_device_batch): many
stripes with the same lost node and helper set in one call.

 * repair batch: (4,2,5), (10,4,13) and (9,3,11) repaired from all n - 1 other nodes run ONE launch
   of the column-flattened k_bs_repair ("bs-repair-batch") at any sub-chunk size and alignment, from
   gathered repair sub-chunks and from whole chunks;
 * staged batch: every other code / helper set / layout, and every batch under "grouped", runs the
   cached repair plan as one k_gexec launch per level for the whole batch ("grouped-batch");
 * stripes of more than 4 MiB of data, and fewer than 4 stripes off the repair batch, run stripe by
   stripe.

Every stripe gets its own seeded random (NON-codeword) chunks, so a stripe mix-up shows, and every
rebuilt chunk is compared with the oracle's repair of that stripe alone.  The gathered layout is
gathered on the host from the same chunks by minimum_to_repair's indices, so both layouts share
one reference.  Outputs go into 0xA5-filled buffers and inputs are compared after the call."""
import numpy as np
import pytest

import clay_amd
from clay_amd import ClayCode

pytestmark = pytest.mark.gpu

FILL = 0xA5
GUARD = 32  # 0xA5 bytes kept before and after every output buffer

# (sc, n_stripes).  (4,2,5), 64 columns per workgroup: one full column per stripe; one partial
# column and a last workgroup with 3 of 64 columns; two columns, the second partial; 10 columns per
# stripe (stripes straddle workgroups); byte tails; more than one tile per stripe with a partial
# last column; byte tails across tiles
S425 = [(32, 300), (8, 67), (40, 67), (320, 37), (777, 5), (2048 + 8 * 37, 5), (2 * 2048 + 5, 3)]
# (10,4,13), 4 columns per workgroup: a last workgroup with 1 of 4 columns; partial columns;
# stripes straddle workgroups, second column partial; byte tails; 300 two-byte sub-chunks
S1013 = [(32, 9), (8, 7), (40, 5), (128 + 37, 3), (2, 300)]
# (9,3,11), 9 columns per workgroup with 243 live lanes
S911 = [(32, 20), (8, 11), (40, 7), (288 + 29, 4)]
# one lost node per y-section with varying x (each y-section is its own instantiation, x only
# moves addresses); at a code's first shape every node is lost in turn
ONE_PER_SECTION = {(4, 2, 5): [1, 2, 5], (10, 4, 13): [1, 6, 8, 13], (9, 3, 11): [2, 3, 7, 11]}
BS_CASES = ([((4, 2, 5), sc, n, i == 0) for i, (sc, n) in enumerate(S425)] +
            [((10, 4, 13), sc, n, i == 0) for i, (sc, n) in enumerate(S1013)] +
            [((9, 3, 11), sc, n, i == 0) for i, (sc, n) in enumerate(S911)])

_inputs = {}
_refs = {}


def stripes(cfg, sc, n):
    """(n, nodes, chunk) random bytes, stripe s from its own seed.  Shared, never modified."""
    key = (cfg, sc, n)
    if key not in _inputs:
        c = ClayCode(*cfg)
        chunk = c.sub_chunk_no * sc
        a = np.stack([np.random.default_rng([sc, n, s, cfg[0], 77]).integers(0, 256, (c.n, chunk), dtype=np.uint8)
                      for s in range(n)])
        a.setflags(write=False)
        _inputs[key] = a
    return _inputs[key]


def helpers_of(c, lost):
    """(helper ids, repair sub-chunk indices) in minimum_to_repair's order."""
    info = c.minimum_to_repair(lost, [i for i in range(c.n) if i != lost])
    return [h for h, _ in info], info[0][1]


def laid_out(c, host, lost, full):
    """(n, nodes, hb) helper buffers of `host` indexed by node id: the whole chunks (full), or the
    beta repair sub-chunks of every node gathered in minimum_to_repair order.  The lost node's
    slot is 0xA5: it is never read."""
    n, _, chunk = host.shape
    if full:
        a = np.array(host)
    else:
        idx = helpers_of(c, lost)[1]
        sc = chunk // c.sub_chunk_no
        a = np.ascontiguousarray(host.reshape(n, c.n, c.sub_chunk_no, sc)[:, :, idx, :]).reshape(n, c.n, len(idx) * sc)
    a[:, lost] = FILL
    return a


def oracle_repair(oracle_mod, cfg, sc, n, lost):
    """(n, chunk): the oracle's repair of node `lost` in every stripe of stripes(cfg, sc, n)."""
    key = (cfg, sc, n, lost)
    if key not in _refs:
        c, o = ClayCode(*cfg), oracle_mod.OracleClay(*cfg)
        chunk = c.sub_chunk_no * sc
        ids = helpers_of(c, lost)[0]
        g = laid_out(c, stripes(cfg, sc, n), lost, False)
        r = np.stack([np.frombuffer(o.repair(lost, {h: g[s, h] for h in ids}, chunk), np.uint8) for s in range(n)])
        r.setflags(write=False)
        _refs[key] = r
    return _refs[key]


def guarded(torch, n, chunk):
    """A 0xA5-filled flat buffer with GUARD bytes around n * chunk output bytes -> (flat, view)."""
    flat = torch.full((GUARD + n * chunk + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    return flat, flat[GUARD:GUARD + n * chunk]


def guards_intact(flat):
    h = flat.cpu().numpy()
    return bool((h[:GUARD] == FILL).all() and (h[-GUARD:] == FILL).all())


def run_strided(torch, c, host, lost, full, mode=None):
    """repair_device_strided of a contiguous [n][nodes][hb] batch into a guarded contiguous
    [n][chunk] output -> (out, path, launches)."""
    prev = clay_amd.set_exec_mode(mode) if mode else None
    try:
        n, _, chunk = host.shape
        src = laid_out(c, host, lost, full)
        dev = torch.from_numpy(src).cuda()
        flat, out = guarded(torch, n, chunk)
        c.repair_device_strided(lost, helpers_of(c, lost)[0], dev, out, n, chunk, full_chunks=full)
        torch.cuda.synchronize()
        path, launches = clay_amd.last_exec_path(), clay_amd.last_launch_count()
        assert np.array_equal(dev.cpu().numpy(), src), "inputs changed"
        assert guards_intact(flat), "bytes written outside the output"
        return out.cpu().numpy().reshape(n, chunk), path, launches
    finally:
        if prev is not None:
            clay_amd.set_exec_mode(prev)


def per_stripe(torch, c, host, lost, full, mode=None):
    """The parent's only way: one repair_device(_full_chunks) per stripe -> (out, last path, launches)."""
    prev = clay_amd.set_exec_mode(mode) if mode else None
    try:
        n, _, chunk = host.shape
        ids = helpers_of(c, lost)[0]
        dev = torch.from_numpy(laid_out(c, host, lost, full)).cuda()
        out = torch.full((n, chunk), FILL, dtype=torch.uint8, device="cuda")
        fn = c.repair_device_full_chunks if full else c.repair_device
        launches = 0
        for s in range(n):
            fn(lost, ids, [dev[s, h] for h in ids], chunk, out[s])
            launches += clay_amd.last_launch_count()
        torch.cuda.synchronize()
        return out.cpu().numpy(), clay_amd.last_exec_path(), launches
    finally:
        if prev is not None:
            clay_amd.set_exec_mode(prev)


# ---------------------------------------------------------------------------
# 1. the repair batch: every shape, both layouts
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("cfg,sc,n,every", BS_CASES)
def test_repair_batch(oracle_mod, torch_cuda, cfg, sc, n, every):
    c = ClayCode(*cfg)
    host = stripes(cfg, sc, n)
    for lost in (range(c.n) if every else ONE_PER_SECTION[cfg]):
        ref = oracle_repair(oracle_mod, cfg, sc, n, lost)
        for full in (False, True):
            got, path, launches = run_strided(torch_cuda, c, host, lost, full)
            assert path == "bs-repair-batch", (lost, full, path)
            assert launches == 1, (lost, full, launches)
            for s in range(n):
                assert np.array_equal(got[s], ref[s]), (cfg, sc, n, lost, full, s)


# ---------------------------------------------------------------------------
# 2. layouts
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("cfg,sc,n,lost", [((4, 2, 5), 40, 67, 2), ((10, 4, 13), 40, 5, 6), ((9, 3, 11), 40, 7, 7)])
def test_repair_batch_layouts(oracle_mod, torch_cuda, cfg, sc, n, lost):
    """Padded node / stripe strides with a separate output of its own stride, in place into the
    lost slot (full chunks), a base off 8-byte alignment (byte tails), and the pointer forms."""
    torch = torch_cuda
    c = ClayCode(*cfg)
    chunk = c.sub_chunk_no * sc
    host = stripes(cfg, sc, n)
    ids = helpers_of(c, lost)[0]
    ref = oracle_repair(oracle_mod, cfg, sc, n, lost)
    oss = chunk + 24  # output stripe stride

    for full in (False, True):
        rows = laid_out(c, host, lost, full)
        hb = rows.shape[2]
        ns_, ss_ = hb + 24, c.n * (hb + 24) + 40  # input node / stripe strides
        for off in (0, 3):  # 3: every pointer off 8-byte alignment
            src = np.full(off + n * ss_, FILL, np.uint8)
            for s in range(n):
                for i in range(c.n):
                    if i != lost:
                        p = off + s * ss_ + i * ns_
                        src[p:p + hb] = rows[s, i]
            buf = torch.from_numpy(src).cuda()
            out = torch.full((off + n * oss,), FILL, dtype=torch.uint8, device="cuda")
            c.repair_device_strided(lost, ids, buf[off:], out[off:], n, chunk, full_chunks=full, node_stride=ns_,
                                    stripe_stride=ss_, out_stripe_stride=oss)
            torch.cuda.synchronize()
            assert clay_amd.last_exec_path() == "bs-repair-batch" and clay_amd.last_launch_count() == 1
            assert np.array_equal(buf.cpu().numpy(), src), ("input buffer changed", full, off)
            want = np.full(off + n * oss, FILL, np.uint8)
            for s in range(n):
                want[off + s * oss:off + s * oss + chunk] = ref[s]
            assert np.array_equal(out.cpu().numpy(), want), ("separate output", full, off)
            if full:
                # in place: the rebuilt chunk into the lost node's slot; nothing else changes
                c.repair_device_strided(lost, ids, buf[off:], buf[off + lost * ns_:], n, chunk, full_chunks=True,
                                        node_stride=ns_, stripe_stride=ss_, out_stripe_stride=ss_)
                torch.cuda.synchronize()
                assert clay_amd.last_exec_path() == "bs-repair-batch" and clay_amd.last_launch_count() == 1
                want = src.copy()
                for s in range(n):
                    p = off + s * ss_ + lost * ns_
                    want[p:p + chunk] = ref[s]
                assert np.array_equal(buf.cpu().numpy(), want), ("in place", off)

        # pointer arrays: rows of one tensor are uniform strides -> the repair batch
        src = rows
        dev = torch.from_numpy(src).cuda()
        flat, out = guarded(torch, n, chunk)
        out = out.view(n, chunk)
        c.repair_device_batch(lost, ids, [dev[s, h] for s in range(n) for h in ids], [out[s] for s in range(n)], n, chunk,
                              full_chunks=full)
        torch.cuda.synchronize()
        assert clay_amd.last_exec_path() == "bs-repair-batch" and clay_amd.last_launch_count() == 1
        assert np.array_equal(out.cpu().numpy(), ref), full
        assert guards_intact(flat) and np.array_equal(dev.cpu().numpy(), src)
        # separately allocated stripes in a shuffled order: not affine -> the device pointer table
        order = np.random.default_rng(7).permutation(n)
        parts = {int(s): torch.from_numpy(np.array(src[s])).cuda() for s in order}
        outs = {int(s): torch.full((chunk + 16 * (int(s) % 3),), FILL, dtype=torch.uint8, device="cuda") for s in order}
        c.repair_device_batch(lost, ids, [parts[s][h] for s in range(n) for h in ids], [outs[s] for s in range(n)], n,
                              chunk, full_chunks=full)
        torch.cuda.synchronize()
        assert clay_amd.last_exec_path() == "grouped-batch"
        for s in range(n):
            o = outs[s].cpu().numpy()
            assert np.array_equal(o[:chunk], ref[s]) and (o[chunk:] == FILL).all(), (full, s)
            assert np.array_equal(parts[s].cpu().numpy(), src[s]), (full, s)


# ---------------------------------------------------------------------------
# 3. staged batch: other codes, and "grouped" as the A/B partner
# ---------------------------------------------------------------------------
STAGED = [((5, 3, 6), 1, None), ((6, 3, 8), 0, None), ((10, 4, 13), 0, "grouped")]


@pytest.mark.parametrize("cfg,lost,mode", STAGED)
def test_staged_batch(oracle_mod, torch_cuda, cfg, lost, mode):
    c = ClayCode(*cfg)
    sc = 32
    counts = []
    for n in (5, 37):
        host = stripes(cfg, sc, n)
        ref = oracle_repair(oracle_mod, cfg, sc, n, lost)
        for full in (False, True):
            got, path, launches = run_strided(torch_cuda, c, host, lost, full, mode=mode)
            assert path == "grouped-batch", (path, full)
            assert np.array_equal(got, ref), (cfg, lost, n, full)
            counts.append((full, launches))
    # the launch count does not depend on the stripe count
    assert counts[0] == counts[2] and counts[1] == counts[3] and counts[0][1] >= 1, counts


def test_grouped_mode_is_the_ab_partner(oracle_mod, torch_cuda):
    cfg, sc, n = (4, 2, 5), 320, 37
    c = ClayCode(*cfg)
    host = stripes(cfg, sc, n)
    for lost in (0, 3, 5):
        ref = oracle_repair(oracle_mod, cfg, sc, n, lost)
        for full in (False, True):
            auto, apath, _ = run_strided(torch_cuda, c, host, lost, full)
            grouped, gpath, _ = run_strided(torch_cuda, c, host, lost, full, mode="grouped")
            assert (apath, gpath) == ("bs-repair-batch", "grouped-batch"), (apath, gpath)
            assert np.array_equal(auto, grouped) and np.array_equal(auto, ref), (lost, full)


# ---------------------------------------------------------------------------
# 4. fallback: few stripes, large stripes
# ---------------------------------------------------------------------------
def test_fallback_few_or_large_stripes(torch_cuda):
    # two stripes of a code without a repair kernel: the staged batch starts at four
    cfg, sc, n, lost = (6, 3, 8), 320, 2, 0
    c = ClayCode(*cfg)
    host = stripes(cfg, sc, n)
    for full in (False, True):
        got, path, launches = run_strided(torch_cuda, c, host, lost, full)
        ref, rpath, rl = per_stripe(torch_cuda, c, host, lost, full)
        assert path == rpath != "grouped-batch", (path, rpath)
        assert launches == rl, (launches, rl)
        assert np.array_equal(got, ref)
    # four stripes of more than 4 MiB of data each
    cfg, sc, n, lost = (4, 2, 5), (1 << 17) + 8, 4, 0
    c = ClayCode(*cfg)
    assert c.k * c.sub_chunk_no * sc > 4 << 20
    host = stripes(cfg, sc, n)
    for full in (False, True):
        got, path, launches = run_strided(torch_cuda, c, host, lost, full)
        ref, rpath, rl = per_stripe(torch_cuda, c, host, lost, full)
        assert path == rpath == "bs-repair" and launches == n == rl, (path, rpath, launches, rl)
        assert np.array_equal(got, ref)


# ---------------------------------------------------------------------------
# 5. capture
# ---------------------------------------------------------------------------
def test_repair_batch_graph_capture(oracle_mod, torch_cuda):
    """The repair batch allocates nothing and needs no pointer table: after one warm call it is
    captured on a side stream (one kernel node) and replayed on fresh input written into the same
    buffers, bit-exact against the oracle."""
    torch = torch_cuda
    cfg, sc, n, lost = (4, 2, 5), 32, 300, 0
    c = ClayCode(*cfg)
    chunk = c.sub_chunk_no * sc
    ids = helpers_of(c, lost)[0]
    data = torch.zeros((n, c.n, chunk), dtype=torch.uint8, device="cuda")
    flat, out = guarded(torch, n, chunk)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):  # warm call outside the capture
        c.repair_device_strided(lost, ids, data, out, n, chunk, full_chunks=True, device=0, stream=st.cuda_stream)
    st.synchronize()
    assert clay_amd.last_exec_path() == "bs-repair-batch"
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=st):
        c.repair_device_strided(lost, ids, data, out, n, chunk, full_chunks=True, device=0,
                                stream=torch.cuda.current_stream().cuda_stream)
    assert clay_amd.last_exec_path() == "bs-repair-batch" and clay_amd.last_launch_count() == 1
    host = stripes(cfg, sc, n)
    src = laid_out(c, host, lost, True)
    data.copy_(torch.from_numpy(src).cuda())
    flat.fill_(FILL)
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy().reshape(n, chunk), oracle_repair(oracle_mod, cfg, sc, n, lost))
    assert guards_intact(flat) and np.array_equal(data.cpu().numpy(), src)
