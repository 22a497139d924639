"""Scrub on the GPU: clay_scrub_device / _batch / _strided and clay_verify against the oracle.

The reference is the oracle's encode.  A codeword is built with OracleClay.encode_array on random
data of exactly k * alpha * sc bytes; the oracle pads odd sub-chunks, so an odd sc is encoded at
sc + 1 and the last column of every sub-chunk dropped (each byte position of the sub-chunks is an
independent codeword).  The expected mask of every case is computed from the oracle, never
assumed: bit j = the stored parity chunk j differs from the oracle's parity of the stored data.

Every buffer has gaps of random bytes between its chunks, `result` is pre-filled with 0xFFFFFFFF
(the call defines it), and after every call the device buffers are byte-identical to what was
uploaded (nothing is written, gaps included)."""
import numpy as np
import pytest

import clay_amd
from clay_amd import ClayCode

pytestmark = pytest.mark.gpu

# code -> positions per tile of its scrub kernels (bitslice.hpp W = 32 * PG)
TILE = {(4, 2, 5): 2048, (6, 3, 8): 512, (8, 4, 11): 256, (9, 3, 11): 192, (10, 4, 13): 64}
GAP = 40  # bytes of garbage between chunks (a multiple of 8: alignment is the shift's business)


def _rng(*seed):
    return np.random.default_rng([20261020, *seed])


def _pad(rows, alpha, sc):
    """(r, alpha * sc) -> (r, alpha * sce) with a zero column appended to every odd sub-chunk."""
    sce = sc + (sc & 1)
    out = np.zeros((rows.shape[0], alpha, sce), np.uint8)
    out[:, :, :sc] = rows.reshape(rows.shape[0], alpha, sc)
    return out.reshape(rows.shape[0], alpha * sce)


def _oracle_parity(o, c, data, sc):
    """The oracle's m parity chunks for the k stored data chunks `data` (k, alpha * sc)."""
    alpha, sce = c.sub_chunk_no, sc + (sc & 1)
    cw = o.encode_array(_pad(data, alpha, sc).reshape(-1))
    assert cw.shape == (c.n, alpha * sce), cw.shape  # the oracle added no padding of its own
    assert np.array_equal(cw[:c.k], _pad(data, alpha, sc))
    return np.ascontiguousarray(cw[c.k:].reshape(c.m, alpha, sce)[:, :, :sc].reshape(c.m, alpha * sc))


def _codeword(o, c, sc, *seed):
    data = _rng(*seed).integers(0, 256, (c.k, c.sub_chunk_no * sc), dtype=np.uint8)
    return np.concatenate([data, _oracle_parity(o, c, data, sc)])


def _expected(o, c, stored, sc, ref_parity=None):
    """Mask of the stored stripe (n, chunk), from the oracle."""
    if ref_parity is None:
        ref_parity = _oracle_parity(o, c, stored[:c.k], sc)
    return sum(1 << j for j in range(c.m) if not np.array_equal(stored[c.k + j], ref_parity[j]))


def _places(c, sc):
    """First byte, last byte of a middle sub-chunk (the tail mask), very last byte of the chunk."""
    return [0, (c.sub_chunk_no // 2) * sc + sc - 1, c.sub_chunk_no * sc - 1]


class Stripes:
    """n_stripes stripes in two device buffers (data, parity) with garbage in every gap: node
    stride chunk + GAP, stripe stride per * (chunk + GAP) + GAP, everything shifted by `shift`."""

    def __init__(self, torch, c, cws, shift=0, seed=0):
        self.torch, self.c, self.ns = torch, c, len(cws)
        self.chunk = cws[0].shape[1]
        self.node = self.chunk + GAP
        self.host, self.dev, self.sstride = [], [], []
        for fam, (lo, per) in enumerate([(0, c.k), (c.k, c.m)]):
            ss = per * self.node + GAP
            h = _rng(seed, fam, 99).integers(0, 256, shift + self.ns * ss + 8, dtype=np.uint8)
            for s, cw in enumerate(cws):
                for i in range(per):
                    at = shift + s * ss + i * self.node
                    h[at:at + self.chunk] = cw[lo + i]
            self.host.append(h)
            self.dev.append(torch.from_numpy(h.copy()).cuda())
            self.sstride.append(ss)
        self.shift = shift
        self.res = torch.empty(self.ns, dtype=torch.int32, device="cuda")

    def off(self, s, node):
        fam, i = (0, node) if node < self.c.k else (1, node - self.c.k)
        return fam, self.shift + s * self.sstride[fam] + i * self.node

    def flip(self, s, node, at, bit=0x10):
        """XOR one bit of byte `at` of a chunk, on the device and in the host image."""
        fam, o = self.off(s, node)
        self.host[fam][o + at] ^= bit
        self.dev[fam][o + at] ^= bit

    def stored(self, s):
        rows = []
        for node in range(self.c.n):
            fam, o = self.off(s, node)
            rows.append(self.host[fam][o:o + self.chunk])
        return np.stack(rows)

    def ptrs(self, s):
        d = [self.dev[0].data_ptr() + self.off(s, i)[1] for i in range(self.c.k)]
        p = [self.dev[1].data_ptr() + self.off(s, self.c.k + j)[1] for j in range(self.c.m)]
        return d, p

    def masks(self):
        out = self.res.cpu().numpy().view(np.uint32).tolist()
        for fam in (0, 1):  # inputs untouched, gaps included
            assert np.array_equal(self.dev[fam].cpu().numpy(), self.host[fam]), "scrub wrote to its inputs"
        self.res.fill_(-1)
        return out

    def scrub_one(self, s=0):
        self.res.fill_(-1)
        d, p = self.ptrs(s)
        self.c.scrub_device(d, p, self.res.data_ptr() + 4 * s, self.chunk)
        return self.masks()[s]

    def scrub_strided(self, stream=0):
        self.res.fill_(-1)
        c = self.c
        c.scrub_device_strided(self.dev[0].data_ptr() + self.shift, self.dev[1].data_ptr() + self.shift, self.res,
                               self.ns, self.chunk, self.node, self.sstride[0], self.node, self.sstride[1], 0, stream)

    def scrub_batch(self, swap=None):
        """Pointer arrays over the rows of the two buffers; swap = (s, tensor): data chunk 0 of
        stripe s lives in `tensor`, a separate allocation."""
        self.res.fill_(-1)
        d, p = [], []
        for s in range(self.ns):
            ds, ps = self.ptrs(s)
            if swap and swap[0] == s:
                ds[0] = swap[1].data_ptr()
            d += ds
            p += ps
        self.c.scrub_device_batch(d, p, self.res, self.ns, self.chunk)


SHAPES = [("tile", lambda W: W, 0), ("part", lambda W: W + 40, 0), ("tiny", lambda W: 16, 0),
          ("odd", lambda W: 2 * W + 5, 0), ("shift3", lambda W: W + 40, 3)]
KERNELS = [((4, 2, 5), "auto", "bs-scrub1"), ((4, 2, 5), "stream", "bs-scrub1"), ((4, 2, 5), "grouped", "bs-scrub"),
           ((4, 2, 5), "tile", "bs-scrub"), ((6, 3, 8), "auto", "bs-scrub"), ((8, 4, 11), "auto", "bs-scrub"),
           ((9, 3, 11), "auto", "bs-scrub"), ((10, 4, 13), "auto", "bs-scrub")]


@pytest.mark.parametrize("shape", SHAPES, ids=[s[0] for s in SHAPES])
@pytest.mark.parametrize("cfg,mode,path", KERNELS, ids=["%d-%d-%d-%s" % (*k[0], k[1]) for k in KERNELS])
def test_one_stripe(oracle_mod, torch_cuda, cfg, mode, path, shape):
    """Clean codeword, one flipped bit in each parity chunk and in a data chunk at the first
    byte, the last byte of a middle sub-chunk and the last byte of the chunk."""
    c, o = ClayCode(*cfg), oracle_mod.OracleClay(*cfg)
    sc, shift = shape[1](TILE[cfg]), shape[2]
    cw = _codeword(o, c, sc, *cfg, sc)
    st = Stripes(torch_cuda, c, [cw], shift=shift, seed=sc)
    ref_parity = cw[c.k:].copy()
    prev = clay_amd.set_exec_mode(mode)
    try:
        assert st.scrub_one() == 0 == _expected(o, c, st.stored(0), sc)
        assert clay_amd.last_exec_path() == path and clay_amd.last_launch_count() == 1
        for pi, at in enumerate(_places(c, sc)):
            for j in range(c.m):
                st.flip(0, c.k + j, at, 1 << ((pi + j) % 8))
                want = _expected(o, c, st.stored(0), sc, ref_parity)
                assert want == 1 << j  # exactly one bit: the data are the codeword's
                got = st.scrub_one()
                st.flip(0, c.k + j, at, 1 << ((pi + j) % 8))
                assert got == want, (at, j, got, want)
            node = (pi * 3 + 1) % c.k
            st.flip(0, node, at, 0x04)
            want = _expected(o, c, st.stored(0), sc)
            assert want != 0
            got = st.scrub_one()
            st.flip(0, node, at, 0x04)
            assert got == want, (at, node, got, want)
            assert clay_amd.last_exec_path() == path
        assert st.scrub_one() == 0
    finally:
        clay_amd.set_exec_mode(prev)


BATCH = [((4, 2, 5), "auto", "bs-scrub1"), ((4, 2, 5), "grouped", "bs-scrub"), ((10, 4, 13), "auto", "bs-scrub")]


@pytest.mark.parametrize("ns", [1, 3, 70])
@pytest.mark.parametrize("small", [True, False], ids=["sc32", "part"])
@pytest.mark.parametrize("cfg,mode,path", BATCH, ids=["%d-%d-%d-%s" % (*k[0], k[1]) for k in BATCH])
def test_batches(oracle_mod, torch_cuda, cfg, mode, path, small, ns):
    """Batches at uniform strides run in one launch (strided form and pointer arrays over rows of
    one buffer); the first, a middle and the last stripe are corrupted, every other word is 0.
    One chunk in a separate allocation: n launches, the same masks."""
    torch = torch_cuda
    c, o = ClayCode(*cfg), oracle_mod.OracleClay(*cfg)
    sc = 32 if small else TILE[cfg] + 40
    # a few distinct codewords, cycled over the stripes (the oracle's time goes to these)
    base = [_codeword(o, c, sc, *cfg, sc, i) for i in range(min(ns, 3))]
    st = Stripes(torch, c, [base[s % len(base)] for s in range(ns)], seed=ns)
    prev = clay_amd.set_exec_mode(mode)
    try:
        def run_all(want):
            st.scrub_strided()
            assert clay_amd.last_exec_path() == path + "-batch" and clay_amd.last_launch_count() == 1
            assert st.masks() == want
            st.scrub_batch()
            assert clay_amd.last_exec_path() == path + "-batch" and clay_amd.last_launch_count() == 1
            assert st.masks() == want
            if ns > 1:
                s = ns // 2
                d0 = st.dev[0][st.off(s, 0)[1]:][:st.chunk].clone()
                st.scrub_batch(swap=(s, d0))
                assert clay_amd.last_exec_path() == path and clay_amd.last_launch_count() == ns
                assert st.masks() == want

        run_all([0] * ns)  # clean codewords, dirty gaps
        places = _places(c, sc)
        hit = {0: (c.k + c.m - 1, places[2])}  # first stripe: a parity flip (n = 1: the only one)
        if ns > 1:
            hit[ns - 1] = (c.k - 1, places[1])  # last stripe: a data flip
        if ns > 2:
            hit[ns // 2] = (c.k, places[0])  # a middle stripe: another parity flip
        for s, (node, at) in hit.items():
            st.flip(s, node, at)
        want = [_expected(o, c, st.stored(s), sc) if s in hit else 0 for s in range(ns)]
        for s, (node, at) in hit.items():
            assert want[s] != 0
            if node >= c.k:
                assert want[s] == 1 << (node - c.k)
        run_all(want)
        if ns == 1:  # the data flip the other sizes have in their last stripe
            st.flip(0, *hit[0])
            st.flip(0, c.k - 1, places[1])
            want = [_expected(o, c, st.stored(0), sc)]
            assert want[0] != 0
            run_all(want)
    finally:
        clay_amd.set_exec_mode(prev)


def test_capture_replays_on_changed_bytes(oracle_mod, torch_cuda):
    """One scrub_device_strided call captured on a side stream (a memset, then the kernel: a
    linear chain) and replayed on the clean buffer, with a parity byte flipped in place, and with
    the byte restored.  The batch call itself is unprepared: the eager one-stripe call before the
    capture only makes sure the process has opened the device."""
    torch = torch_cuda
    cfg = (4, 2, 5)
    c, o = ClayCode(*cfg), oracle_mod.OracleClay(*cfg)
    sc = TILE[cfg] + 40
    st = Stripes(torch, c, [_codeword(o, c, sc, 77, i) for i in range(3)], seed=77)
    assert st.scrub_one(2) == 0
    side = torch.cuda.Stream()
    pool = clay_amd.workspace_bytes(0)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        st.scrub_strided(stream=torch.cuda.current_stream().cuda_stream)
    assert clay_amd.last_exec_path() == "bs-scrub1-batch" and clay_amd.last_launch_count() == 1
    assert clay_amd.workspace_bytes(0) == pool  # nothing allocated
    for flip in (False, True, False):
        if flip:
            st.flip(1, c.k + 1, _places(c, sc)[1], 0xFF)
        want = [_expected(o, c, st.stored(s), sc) for s in range(3)]
        assert want == ([0, 2, 0] if flip else [0, 0, 0])
        st.res.fill_(-1)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert st.masks() == want
        if flip:
            st.flip(1, c.k + 1, _places(c, sc)[1], 0xFF)
    del g
    torch.cuda.synchronize()


@pytest.mark.parametrize("cfg,sc", [((4, 2, 5), 48), ((9, 3, 11), 37)])
def test_host_verify(oracle_mod, torch_cuda, cfg, sc):
    c, o = ClayCode(*cfg), oracle_mod.OracleClay(*cfg)
    cw = _codeword(o, c, sc, *cfg, sc, 5)
    assert c.verify([bytes(r) for r in cw]) == 0 == _expected(o, c, cw, sc)
    for j in range(c.m):
        bad = cw.copy()
        bad[c.k + j, _places(c, sc)[j % 3]] ^= 0x80
        want = _expected(o, c, bad, sc)
        assert want == 1 << j
        assert c.verify(list(bad)) == want
    bad = cw.copy()
    bad[1, _places(c, sc)[1]] ^= 0x01
    want = _expected(o, c, bad, sc)
    assert want != 0 and c.verify(list(bad)) == want
