"""The batched streaming scrub (k_stream_encode SCRUB && BATCH: many (10,4,13) stripes in ONE
launch, exec path "stream-scrub-batch") against the oracle.

Every case runs under set_scrub_path('stream-batch') and restores 'auto'.  The buffers are
test_gpu_scrub.Stripes': chunks in garbage, the data stripe stride different from the parity
stripe stride, the inputs compared to the upload after every call; the result vector has GUARD
words behind the batch that must stay 0xFFFFFFFF.  The codewords are the oracle's
(test_gpu_stream_batch._reference, computed once per shape), so a parity flip's mask follows from
the flip schedule; the mask of a data flip is the oracle's parity of the column pair holding it
against the stored parity.

  test_shapes          the batched encode's shapes (test_gpu_stream_batch.case_shape), strided and
                       pointer-array form: clean; flips only in the stripes of a group's first pass
                       (s < G: a mismatch word that is not reset would leak into s + G); only in
                       the later ones; a mask per stripe distinct from its neighbours' plus one data
                       flip (a report into the wrong word, a parity address without the stripe)
  test_every_parity_byte  sc 16 (the DPP-pair compare) and sc 24 (the ragged compare): every stored
                       parity byte flipped alone, scrub_sweeps' slab scheme, data stripe stride 0
  test_tile_edges_2288 every layer at the tile edges of sc 2288, one flip per stripe of a batch
  test_not_taken       what the batch does not take keeps its path and launch count
  test_first_met_inside_a_capture  no warm call, three replays on changed bytes
  test_auto_gate*      scrub path 'auto': the measured gate of engine.hip, both sides
"""
import numpy as np
import pytest

import clay_amd
import scrub_sweeps as sw
from clay_amd import ClayCode
from stream_cut import dump_tiles, xcd_region
from test_gpu_scrub import Stripes, _codeword, _expected, _oracle_parity, _places
from test_gpu_stream_batch import _per_xcd, _reference, batch_shape, case_shape

pytestmark = pytest.mark.gpu

CFG = (10, 4, 13)
PATH = "stream-scrub-batch"
CASES = ["one_piece", "ragged", "full", "few2", "few3", "narrow", "idle_ragged", "two_rounds"]


@pytest.fixture
def stream_batch():
    prev = clay_amd.set_scrub_path("stream-batch")
    try:
        yield
    finally:
        clay_amd.set_scrub_path(prev)
        clay_amd.set_exec_mode("auto")


class Guarded(Stripes):
    """Stripes with sw.GUARD result words behind the batch; masks() checks them."""

    def __init__(self, torch, c, cws, shift=0, seed=0):
        super().__init__(torch, c, cws, shift=shift, seed=seed)
        self.res = torch.empty(self.ns + sw.GUARD, dtype=torch.int32, device="cuda")

    def masks(self):
        out = super().masks()
        assert out[self.ns:] == [0xFFFFFFFF] * sw.GUARD, "result words beyond the batch written"
        return out[:self.ns]


def _codewords(cfg, sc, n):
    data, par = _reference(cfg, sc, n)
    return [np.concatenate([data[s], par[s]]) for s in range(n)]


def _pair_mask(o, c, stored, sc, at):
    """Mask of a stored stripe that is a clean codeword outside the column pair holding chunk
    offset `at`: the oracle's parity of that pair of byte positions against the stored one."""
    col = (at % sc) & ~1
    cols = stored.reshape(c.n, c.sub_chunk_no, sc)[:, :, col:col + 2]
    par = _oracle_parity(o, c, np.ascontiguousarray(cols[:c.k]).reshape(c.k, -1), 2)
    return sum(1 << j for j in range(c.m) if not np.array_equal(cols[c.k + j].reshape(-1), par[j]))


def _run_both(st, want, what):
    for form, call in (("strided", st.scrub_strided), ("arrays", st.scrub_batch)):
        call()
        assert (clay_amd.last_exec_path(), clay_amd.last_launch_count()) == (PATH, 1), (what, form)
        got = st.masks()
        bad = [(s, got[s], want[s]) for s in range(st.ns) if got[s] != want[s]]
        assert not bad, (what, form, f"{len(bad)} of {st.ns} words wrong (stripe, got, want)", bad[:8])


@pytest.mark.parametrize("name", CASES)
def test_shapes(oracle_mod, torch_cuda, stream_batch, name):
    per_xcd = _per_xcd(torch_cuda)
    cfg, mode, sc, n = case_shape(name, per_xcd)
    assert cfg == CFG
    c, o = ClayCode(*cfg), oracle_mod.OracleClay(*cfg)
    G = batch_shape(sc, n, per_xcd)[1]
    st = Guarded(torch_cuda, c, _codewords(cfg, sc, n), seed=sc)
    places = _places(c, sc)
    clay_amd.set_exec_mode(mode)

    def one_bit(stripes):
        """One flipped parity bit per listed stripe, chunk s % 4, the place rotating with s."""
        for s in stripes:
            st.flip(s, c.k + s % c.m, places[s % 3], 1 << (s % 8))

    # (a) clean codewords, dirty gaps
    _run_both(st, [0] * n, "clean")
    # (b) only the stripes of every group's first pass
    one_bit(range(min(G, n)))
    _run_both(st, [1 << (s % c.m) if s < G else 0 for s in range(n)], "first pass")
    one_bit(range(min(G, n)))
    # (c) only the later ones
    if n > G:
        one_bit(range(G, n))
        _run_both(st, [1 << (s % c.m) if s >= G else 0 for s in range(n)], "later passes")
        one_bit(range(G, n))
    # (d) a parity chunk set per stripe, 1 .. 15 in turn; one stripe a data flip instead
    sd = n // 2
    masks = [s % 15 + 1 for s in range(n)]

    def chunk_sets():
        for s in range(n):
            for j in range(c.m):
                if s != sd and masks[s] >> j & 1:
                    st.flip(s, c.k + j, places[(s + j) % 3], 1 << ((s + j) % 8))

    chunk_sets()
    at = places[1] - 3
    st.flip(sd, 7, at, 0x04)
    masks[sd] = _pair_mask(o, c, st.stored(sd), sc, at)
    assert masks[sd] != 0
    if sc <= 2048 and name != "full":  # the whole-stripe oracle agrees (small stripes only: its time)
        assert masks[sd] == _expected(o, c, st.stored(sd), sc)
    assert all(masks[s] != masks[s + 1] for s in range(n - 1) if sd not in (s, s + 1))
    _run_both(st, masks, "a mask per stripe")
    st.flip(sd, 7, at, 0x04)
    chunk_sets()
    _run_both(st, [0] * n, "restored")


@pytest.mark.parametrize("sc", [16, 24])
def test_every_parity_byte(oracle_mod, torch_cuda, stream_batch, sc):
    """Stripe s of the slab has byte p0 + s of parity chunk (s + r) % 4 flipped in pass r; every
    stripe reads the same data chunks (a data stripe stride of 0).  One launch per pass."""
    torch = torch_cuda
    c, o = ClayCode(*CFG), oracle_mod.OracleClay(*CFG)
    cw = _codeword(o, c, sc, *CFG, sc, 41)
    ref = np.ascontiguousarray(cw[c.k:])
    st = Stripes(torch, c, [cw], seed=sc)
    m, chunk = c.m, st.chunk
    data_ptrs, _ = st.ptrs(0)
    par0 = torch.from_numpy(ref).cuda()
    slabs = sw.slabs(m, chunk)
    assert slabs == [(0, chunk)] and chunk == 256 * sc  # one slab holds the whole chunk
    for p0, ns in slabs:
        slab = torch.empty(ns * m * chunk, dtype=torch.uint8, device="cuda")
        slab.view(ns, m, chunk).copy_(par0.expand(ns, m, chunk))
        res = torch.empty(ns + sw.GUARD, dtype=torch.int32, device="cuda")
        par_ptrs = (slab.data_ptr() + np.arange(ns * m, dtype=np.int64) * chunk).tolist()
        for r in range(m):
            jj, pos = sw.batch_pass(m, p0, ns, r)
            bits = sw.flip_bits(pos, jj)
            want = sw.expected_masks(ref, jj, pos, bits)
            assert np.array_equal(want, np.uint32(1) << jj.astype(np.uint32))
            idx = torch.from_numpy(np.arange(ns, dtype=np.int64) * (m * chunk) + jj * chunk + pos).cuda()
            bits_d = torch.from_numpy(bits).cuda()
            slab[idx] ^= bits_d
            res.fill_(-1)
            c.scrub_device_batch(data_ptrs * ns, par_ptrs, res, ns, chunk)
            assert (clay_amd.last_exec_path(), clay_amd.last_launch_count()) == (PATH, 1)
            slab[idx] ^= bits_d
            got = res.cpu().numpy().view(np.uint32)
            assert np.all(got[ns:] == 0xFFFFFFFF), "result words beyond the batch written"
            wrong = sw.first_wrong(got[:ns], want, jj, pos, sc)
            assert wrong is None, (p0, r, wrong)
        assert torch.equal(slab.view(ns, m, chunk), par0.expand(ns, m, chunk)), "slab not restored"
    for fam in (0, 1):
        assert np.array_equal(st.dev[fam].cpu().numpy(), st.host[fam]), "scrub wrote to its inputs"


@pytest.fixture(scope="module")
def tiles_2288(tmp_path_factory):
    return dump_tiles(tmp_path_factory.mktemp("batch_tiles"), [2288])[2288]


@pytest.mark.parametrize("j", range(4))
def test_tile_edges_2288(oracle_mod, torch_cuda, stream_batch, tiles_2288, j):
    """scrub_sweeps' "edges" flips of sc 2288 in parity chunk j (every layer at the first and last
    byte of every tile and at a ragged tile's 16-byte boundaries), flip i alone in stripe i % ns of
    batch i // ns: as many stripes per batch as scrub_sweeps' slab cap holds, every batch one
    launch into its own result words, one read-back at the end."""
    torch = torch_cuda
    sc = 2288
    c, o = ClayCode(*CFG), oracle_mod.OracleClay(*CFG)
    cw = _codeword(o, c, sc, *CFG, sc, 42)
    ref = np.ascontiguousarray(cw[c.k:])
    st = Stripes(torch, c, [cw], seed=sc)
    m, chunk = c.m, st.chunk
    jj, pos = sw.stream_flips((sc, "edges", j, 0), tiles_2288)
    bits = sw.flip_bits(pos, jj)
    want = sw.expected_masks(ref, jj, pos, bits)
    assert np.all(want == 1 << j) and len(jj) >= 256 * 2 * len(tiles_2288) // 2
    ns = sw.slabs(m, chunk)[0][1]
    data_ptrs, _ = st.ptrs(0)
    par0 = torch.from_numpy(ref).cuda()
    slab = torch.empty(ns * m * chunk, dtype=torch.uint8, device="cuda")
    slab.view(ns, m, chunk).copy_(par0.expand(ns, m, chunk))
    par_ptrs = (slab.data_ptr() + np.arange(ns * m, dtype=np.int64) * chunk).tolist()
    res = torch.full((len(jj) + sw.GUARD,), -1, dtype=torch.int32, device="cuda")
    at_all = torch.from_numpy(jj * chunk + pos).cuda()
    bits_all = torch.from_numpy(bits).cuda()
    stripe0 = torch.arange(ns, dtype=torch.int64, device="cuda") * (m * chunk)
    for i0 in range(0, len(jj), ns):
        nb = min(ns, len(jj) - i0)
        if nb < 2:  # one flip left over: its stripe twice (a batch needs two)
            i0, nb = i0 - 1, 2
        idx = stripe0[:nb] + at_all[i0:i0 + nb]
        slab[idx] ^= bits_all[i0:i0 + nb]
        c.scrub_device_batch(data_ptrs * nb, par_ptrs[:nb * m], res.data_ptr() + 4 * i0, nb, chunk)
        assert (clay_amd.last_exec_path(), clay_amd.last_launch_count()) == (PATH, 1)
        slab[idx] ^= bits_all[i0:i0 + nb]
    got = res.cpu().numpy().view(np.uint32)
    assert np.all(got[len(jj):] == 0xFFFFFFFF), "result words beyond the last batch written"
    wrong = sw.first_wrong(got[:len(jj)], want, jj, pos, sc)
    assert wrong is None, wrong
    assert torch.equal(slab.view(ns, m, chunk), par0.expand(ns, m, chunk)), "slab not restored"
    for fam in (0, 1):
        assert np.array_equal(st.dev[fam].cpu().numpy(), st.host[fam]), "scrub wrote to its inputs"


def test_not_taken(oracle_mod, torch_cuda, stream_batch):
    """Each call the batch does not take runs as before: path name, launch count, masks."""
    torch = torch_cuda
    c, o = ClayCode(*CFG), oracle_mod.OracleClay(*CFG)
    n = 3

    def stripes(sc, shift=0, ns=n):
        st = Guarded(torch, c, [_codeword(o, c, sc, *CFG, sc, shift, i) for i in range(ns)], shift=shift, seed=sc)
        st.flip(0, c.k + 3, _places(c, sc)[2])
        if ns > 1:
            st.flip(ns - 1, c.k - 1, _places(c, sc)[1])
        want = [_expected(o, c, st.stored(s), sc) for s in range(ns)]
        assert want[0] == 8 and all(w == 0 for w in want[1:-1]) and want[-1] != 0
        return st, want

    def check(st, want, call, path, launches, what):
        call()
        assert (clay_amd.last_exec_path(), clay_amd.last_launch_count()) == (path, launches), what
        assert st.masks() == want, what

    st, want = stripes(1064)
    clay_amd.set_exec_mode("stream")
    check(st, want, st.scrub_strided, PATH, 1, "the eligible call")
    # one data chunk in an allocation of its own: off the stride
    d0 = st.dev[0][st.off(1, 0)[1]:][:st.chunk].clone()
    check(st, want, lambda: st.scrub_batch(swap=(1, d0)), "stream-scrub", n, "swap")
    # scrub path 'auto' under exec "stream": the per-stripe loop
    clay_amd.set_scrub_path("auto")
    check(st, want, st.scrub_strided, "stream-scrub", n, "auto under stream")
    check(st, want, st.scrub_batch, "stream-scrub", n, "auto under stream")
    clay_amd.set_scrub_path("stream-batch")
    # exec "grouped": v1
    clay_amd.set_exec_mode("grouped")
    check(st, want, st.scrub_strided, "bs-scrub-batch", 1, "grouped")
    check(st, want, st.scrub_batch, "bs-scrub-batch", 1, "grouped")
    # one stripe through the batch entry points
    st1, want1 = stripes(1064, ns=1)
    clay_amd.set_exec_mode("stream")
    check(st1, want1, st1.scrub_strided, "stream-scrub", 1, "one stripe")
    check(st1, want1, st1.scrub_batch, "stream-scrub", 1, "one stripe")
    # chunks shifted by 3 bytes, and an odd sub-chunk: v1
    for sc, shift in ((1064, 3), (133, 0)):
        st, want = stripes(sc, shift)
        for mode in ("stream", "auto"):
            clay_amd.set_exec_mode(mode)
            check(st, want, st.scrub_strided, "bs-scrub-batch", 1, (sc, shift, mode))
            check(st, want, st.scrub_batch, "bs-scrub-batch", 1, (sc, shift, mode))


def test_first_met_inside_a_capture(oracle_mod, torch_cuda, stream_batch):
    """No allocation, no pointer table: a batch of a shape never run before is captured without a
    warm call and replayed on the clean buffers, with one parity byte of the last stripe flipped,
    and with the byte restored."""
    torch = torch_cuda
    c, o = ClayCode(*CFG), oracle_mod.OracleClay(*CFG)
    sc, n = 2080, 4
    st = Guarded(torch, c, [_codeword(o, c, sc, *CFG, sc, 78, i) for i in range(n)], seed=78)
    # the device's own state exists before the capture: another code at another size
    small = ClayCode(4, 2, 5)
    z = torch.zeros((6, small.sub_chunk_no * 32), dtype=torch.uint8, device="cuda")
    small.encode_device([z[i] for i in range(4)], [z[4], z[5]], small.sub_chunk_no * 32)
    pool = clay_amd.workspace_bytes(0)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        st.scrub_strided(stream=torch.cuda.current_stream().cuda_stream)
    assert (clay_amd.last_exec_path(), clay_amd.last_launch_count()) == (PATH, 1)
    assert clay_amd.workspace_bytes(0) == pool  # nothing allocated
    j, at = 2, _places(c, sc)[1]
    for flip in (False, True, False):
        if flip:
            st.flip(n - 1, c.k + j, at, 0xFF)
        want = [_expected(o, c, st.stored(s), sc) for s in range(n)]
        assert want == [0] * (n - 1) + [1 << j if flip else 0]
        st.res.fill_(-1)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert st.masks() == want
        if flip:
            st.flip(n - 1, c.k + j, at, 0xFF)
    del g
    torch.cuda.synchronize()


# Auto's gate (engine.hip: kScrubBatchMinSc 2,048, kScrubBatchMaxSc 66,176, kScrubBatchMinFill 20
# 256-byte tiles per XCD over min(G, n) groups): (sc, n, inside) just inside and just outside on
# each side, at the smallest stripe counts the rule allows
def _fill_tiles(sc, n, per_xcd):
    return batch_shape(sc, n, per_xcd)[1] * xcd_region(sc) / 256


def _auto_gate_case(torch, oracle_mod, sc, n, inside, cws):
    """Scrub path and exec mode auto: path name, launch count and masks (from the flip schedule on
    the oracle's codewords) in both forms."""
    c = ClayCode(*CFG)
    st = Guarded(torch, c, [cws[s % len(cws)] for s in range(n)], seed=sc + n)
    prev_path, prev_exec = clay_amd.set_scrub_path("auto"), clay_amd.set_exec_mode("auto")
    try:
        if inside:
            path, launches = PATH, 1
        elif sc >= 65536:
            path, launches = "stream-scrub", n
        else:
            path, launches = "bs-scrub-batch", 1
        hits = {0: 3, n - 1: 1}  # stripe -> corrupted parity chunk
        for rnd in range(2):
            want = [1 << hits[s] if rnd and s in hits else 0 for s in range(n)]
            if rnd:
                for s, j in hits.items():
                    st.flip(s, c.k + j, _places(c, sc)[(s + 1) % 3], 0x02)
            for call in (st.scrub_strided, st.scrub_batch):
                call()
                assert (clay_amd.last_exec_path(), clay_amd.last_launch_count()) == (path, launches), (sc, n)
                assert st.masks() == want, (sc, n, path)
    finally:
        clay_amd.set_scrub_path(prev_path)
        clay_amd.set_exec_mode(prev_exec)


@pytest.mark.parametrize("sc,n,inside", [(2048, 20, True), (2048, 19, False), (2040, 20, False)])
def test_auto_gate(oracle_mod, torch_cuda, sc, n, inside):
    """The fill bound (20 tiles per XCD in, 19 out at the lower sub-chunk bound) and the lower
    sub-chunk bound (2,040 has the fill of 2,048 and stays on v1)."""
    per_xcd = _per_xcd(torch_cuda)
    if per_xcd >= 20:  # the MI355X's 32: the cases sit where the docstring says
        assert (_fill_tiles(sc, n, per_xcd) >= 20) == (n >= 20)
    c, o = ClayCode(*CFG), oracle_mod.OracleClay(*CFG)
    cws = [_codeword(o, c, sc, *CFG, sc, 90 + i) for i in range(3)]
    _auto_gate_case(torch_cuda, oracle_mod, sc, n, inside and per_xcd >= 20, cws)


@pytest.mark.slow
@pytest.mark.parametrize("sc,inside", [(66176, True), (66184, False)])
def test_auto_gate_upper(oracle_mod, torch_cuda, sc, inside):
    """The upper sub-chunk bound with 2 stripes: 66,176 is one launch, 66,184 the per-stripe loop."""
    c, o = ClayCode(*CFG), oracle_mod.OracleClay(*CFG)
    _auto_gate_case(torch_cuda, oracle_mod, sc, 2, inside, [_codeword(o, c, sc, *CFG, sc, 95)])
