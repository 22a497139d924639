"""Layout edges of the batched calls: what decides between a single-launch batch kernel (stripe 0's
pointers + one stride in its arguments) and the staged batch (a pointer table).

 (a) Pointer arrays that are rows of one buffer for every node but ONE, whose rows sit in a second
     buffer at another stripe stride -- once an input node, once an output (whose rows are
     irregular: the one output of a decode or repair has a stride of its own, so rows at any one
     stride would be uniform).  The stripes are not at one stride, so the single-launch kernel must
     not run: encode reports "staged-batch", decode and
     repair "grouped-batch", and the bytes are the oracle's.
 (b) The strided forms with ONE stripe and a stripe stride that is no multiple of 8 at 8-byte
     aligned node pointers: the caller's stride still reaches the kernel's arguments (and its
     byte-tail decision); path and launch count as recorded before the layouts were unified.

(4,2,5), 5 stripes, sub-chunks of 40 bytes (1024 for the encode, where the bit-sliced batch is
eligible).  Every stripe gets its own seeded random bytes, so a stripe mix-up shows."""
import numpy as np
import pytest

import clay_amd
from clay_amd import ClayCode

pytestmark = pytest.mark.gpu

CFG, N, SC, SC_ENC = (4, 2, 5), 5, 40, 1024
FILL = 0xA5
PAD = 24  # the odd node's rows sit PAD bytes further apart than everyone else's

_cache = {}


def stripes(sc):
    """(N, n, chunk) random (non-codeword) chunks, stripe s from its own seed.  Shared, read-only."""
    if ("in", sc) not in _cache:
        c = ClayCode(*CFG)
        a = np.stack([np.random.default_rng([sc, s, 91]).integers(0, 256, (c.n, c.sub_chunk_no * sc), dtype=np.uint8)
                      for s in range(N)])
        a.setflags(write=False)
        _cache["in", sc] = a
    return _cache["in", sc]


def ref_parity(oracle_mod):
    """(N, m, chunk): the oracle's parity of the data nodes of stripes(SC_ENC)."""
    if "enc" not in _cache:
        c, o = ClayCode(*CFG), oracle_mod.OracleClay(*CFG)
        a = stripes(SC_ENC)
        _cache["enc"] = np.stack([o.encode_array(a[s, :c.k].reshape(-1))[c.k:] for s in range(N)])
    return _cache["enc"]


def ref_decode(oracle_mod, er):
    """(N, chunk): the oracle's decode of data node er of every stripe of stripes(SC)."""
    if ("dec", er) not in _cache:
        c, o = ClayCode(*CFG), oracle_mod.OracleClay(*CFG)
        a = stripes(SC)
        _cache["dec", er] = np.stack([
            np.frombuffer(o.decode({i: a[s, i] for i in range(c.n) if i != er}, [er]), np.uint8).reshape(c.k, -1)[er]
            for s in range(N)])
    return _cache["dec", er]


def helpers_of(c, lost):
    info = c.minimum_to_repair(lost, [i for i in range(c.n) if i != lost])
    return [h for h, _ in info], info[0][1]


def ref_repair(oracle_mod, lost):
    """(N, chunk): the oracle's repair of node `lost` of every stripe of stripes(SC)."""
    if ("rep", lost) not in _cache:
        c, o = ClayCode(*CFG), oracle_mod.OracleClay(*CFG)
        a = stripes(SC)
        ids, idx = helpers_of(c, lost)
        chunk = c.sub_chunk_no * SC
        _cache["rep", lost] = np.stack([
            np.frombuffer(o.repair(lost, {h: np.concatenate([a[s, h, z * SC:(z + 1) * SC] for z in idx]) for h in ids},
                                   chunk), np.uint8) for s in range(N)])
    return _cache["rep", lost]


def split_rows(torch, host, odd):
    """The device rows of host [N][nodes][chunk]: one tensor for every node, but node `odd` (None:
    no node) in a second tensor whose rows are PAD bytes further apart -> row(s, i), both tensors."""
    main = torch.from_numpy(np.array(host)).cuda()
    chunk = host.shape[2]
    side = torch.full((N, chunk + PAD), FILL, dtype=torch.uint8, device="cuda")
    if odd is not None:
        side[:, :chunk] = main[:, odd]
        main[:, odd] = FILL  # never read: the call names the side rows
    return (lambda s, i: side[s, :chunk] if i == odd else main[s, i]), main, side


class OutRows:
    """N 0xA5-filled output rows of `chunk` bytes in one flat tensor: back to back, or (odd) PAD + 16
    bytes apart with the last row 8 bytes further still.  A single output has a stride of its own,
    so rows at ANY one stride are uniform: only an irregular row takes it off the stride."""

    def __init__(self, torch, chunk, odd):
        self.chunk = chunk
        step = chunk + (PAD + 16 if odd else 0)
        self.off = [s * step + (8 if odd and s == N - 1 else 0) for s in range(N)]
        self.flat = torch.full((N * step + 8,), FILL, dtype=torch.uint8, device="cuda")

    def row(self, s):
        return self.flat[self.off[s]:self.off[s] + self.chunk]

    def collect(self):
        """(the N rows, whether every byte outside them is still 0xA5)"""
        h = self.flat.cpu().numpy()
        rest = np.ones(h.size, bool)
        for o in self.off:
            rest[o:o + self.chunk] = False
        return np.stack([h[o:o + self.chunk] for o in self.off]), bool((h[rest] == FILL).all())


# ---------------------------------------------------------------------------
# (a) one operand off the common stride
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("odd", ["input", "output"])
def test_encode_one_node_off_the_stride(oracle_mod, torch_cuda, odd):
    torch = torch_cuda
    c = ClayCode(*CFG)
    chunk = c.sub_chunk_no * SC_ENC
    host = stripes(SC_ENC)[:, :c.k]
    ref = ref_parity(oracle_mod)
    row, main, side = split_rows(torch, host, 2 if odd == "input" else None)
    par = torch.full((N, c.m, chunk), FILL, dtype=torch.uint8, device="cuda")
    pside = OutRows(torch, chunk, True)
    odd_par = 1 if odd == "output" else None
    c.encode_device_batch([row(s, i) for s in range(N) for i in range(c.k)],
                          [pside.row(s) if j == odd_par else par[s, j] for s in range(N) for j in range(c.m)], N, chunk)
    torch.cuda.synchronize()
    path = clay_amd.last_encode_path()
    print(f"encode, odd {odd}: path {path}, launches {clay_amd.last_launch_count()}")
    assert path == "staged-batch", path
    got = par.cpu().numpy()
    if odd_par is not None:
        rows, clean = pside.collect()
        assert (got[:, odd_par] == FILL).all() and clean
        got[:, odd_par] = rows
    assert np.array_equal(got, ref), odd
    # control: the same rows of one tensor each are at one stride -> the single launch
    dev = torch.from_numpy(np.array(host)).cuda()
    par.fill_(FILL)
    c.encode_device_batch([dev[s, i] for s in range(N) for i in range(c.k)],
                          [par[s, j] for s in range(N) for j in range(c.m)], N, chunk)
    torch.cuda.synchronize()
    assert clay_amd.last_encode_path().startswith("bitsliced-batch-line"), clay_amd.last_encode_path()
    assert clay_amd.last_launch_count() == 1
    assert np.array_equal(par.cpu().numpy(), ref)


@pytest.mark.parametrize("odd", ["input", "output"])
def test_decode_one_node_off_the_stride(oracle_mod, torch_cuda, odd):
    torch = torch_cuda
    c = ClayCode(*CFG)
    chunk, er = c.sub_chunk_no * SC, 1
    host = stripes(SC)
    ref = ref_decode(oracle_mod, er)
    row, main, side = split_rows(torch, host, 3 if odd == "input" else None)
    out = OutRows(torch, chunk, odd == "output")
    before = main.cpu().numpy()
    c.decode_device_batch([None if i == er else row(s, i) for s in range(N) for i in range(c.n)], [er],
                          [out.row(s) if i == er else None for s in range(N) for i in range(c.n)], N, chunk)
    torch.cuda.synchronize()
    path = clay_amd.last_exec_path()
    print(f"decode, odd {odd}: path {path}, launches {clay_amd.last_launch_count()}")
    assert path == "grouped-batch", path
    rows, clean = out.collect()
    assert np.array_equal(rows, ref), odd
    assert clean and np.array_equal(main.cpu().numpy(), before)
    # control: rows of one tensor each -> the single launch
    dev = torch.from_numpy(np.array(host)).cuda()
    out2 = torch.full((N, chunk), FILL, dtype=torch.uint8, device="cuda")
    c.decode_device_batch([None if i == er else dev[s, i] for s in range(N) for i in range(c.n)], [er],
                          [out2[s] if i == er else None for s in range(N) for i in range(c.n)], N, chunk)
    torch.cuda.synchronize()
    assert (clay_amd.last_exec_path(), clay_amd.last_launch_count()) == ("bs-decode1-batch", 1)
    assert np.array_equal(out2.cpu().numpy(), ref)


@pytest.mark.parametrize("odd", ["input", "output"])
def test_repair_one_helper_off_the_stride(oracle_mod, torch_cuda, odd):
    torch = torch_cuda
    c = ClayCode(*CFG)
    chunk, lost = c.sub_chunk_no * SC, 0
    ids, _ = helpers_of(c, lost)
    assert len(ids) == c.n - 1
    host = stripes(SC)
    ref = ref_repair(oracle_mod, lost)
    row, main, side = split_rows(torch, host, ids[2] if odd == "input" else None)
    out = OutRows(torch, chunk, odd == "output")
    before = main.cpu().numpy()
    c.repair_device_batch(lost, ids, [row(s, h) for s in range(N) for h in ids], [out.row(s) for s in range(N)], N, chunk,
                          full_chunks=True)
    torch.cuda.synchronize()
    path = clay_amd.last_exec_path()
    print(f"repair, odd {odd}: path {path}, launches {clay_amd.last_launch_count()}")
    assert path == "grouped-batch", path
    rows, clean = out.collect()
    assert np.array_equal(rows, ref), odd
    assert clean and np.array_equal(main.cpu().numpy(), before)
    # control: rows of one tensor each -> the single launch
    dev = torch.from_numpy(np.array(host)).cuda()
    out2 = torch.full((N, chunk), FILL, dtype=torch.uint8, device="cuda")
    c.repair_device_batch(lost, ids, [dev[s, h] for s in range(N) for h in ids], [out2[s] for s in range(N)], N, chunk,
                          full_chunks=True)
    torch.cuda.synchronize()
    assert (clay_amd.last_exec_path(), clay_amd.last_launch_count()) == ("bs-repair-batch", 1)
    assert np.array_equal(out2.cpu().numpy(), ref)


# ---------------------------------------------------------------------------
# (b) one stripe, strided, odd stripe strides
# ---------------------------------------------------------------------------
def test_decode_strided_one_stripe_odd_stride(oracle_mod, torch_cuda):
    torch = torch_cuda
    c = ClayCode(*CFG)
    chunk, er = c.sub_chunk_no * SC, 1
    host = stripes(SC)[:1]
    dev = torch.from_numpy(np.array(host)).cuda()
    out = torch.full((c.n, chunk), FILL, dtype=torch.uint8, device="cuda")
    assert dev.data_ptr() % 8 == 0 and out.data_ptr() % 8 == 0 and chunk % 8 == 0
    c.decode_device_strided(dev, [er], out, 1, chunk, node_stride=chunk, stripe_stride=c.n * chunk + 13,
                            out_node_stride=chunk, out_stripe_stride=c.n * chunk + 5)
    torch.cuda.synchronize()
    path, launches = clay_amd.last_exec_path(), clay_amd.last_launch_count()
    print(f"decode strided, one stripe: path {path}, launches {launches}")
    assert (path, launches) == ("bs-decode1-batch", 1)
    got = out.cpu().numpy()
    assert np.array_equal(got[er], ref_decode(oracle_mod, er)[0])
    assert (np.delete(got, er, axis=0) == FILL).all() and np.array_equal(dev.cpu().numpy(), host)


def test_repair_strided_one_stripe_odd_stride(oracle_mod, torch_cuda):
    torch = torch_cuda
    c = ClayCode(*CFG)
    chunk, lost = c.sub_chunk_no * SC, 0
    ids, _ = helpers_of(c, lost)
    host = stripes(SC)[:1]
    dev = torch.from_numpy(np.array(host)).cuda()
    out = torch.full((chunk + 16,), FILL, dtype=torch.uint8, device="cuda")
    assert dev.data_ptr() % 8 == 0 and out.data_ptr() % 8 == 0 and chunk % 8 == 0
    c.repair_device_strided(lost, ids, dev, out, 1, chunk, full_chunks=True, node_stride=chunk,
                            stripe_stride=c.n * chunk + 13, out_stripe_stride=chunk + 5)
    torch.cuda.synchronize()
    path, launches = clay_amd.last_exec_path(), clay_amd.last_launch_count()
    print(f"repair strided, one stripe: path {path}, launches {launches}")
    assert (path, launches) == ("bs-repair-batch", 1)
    got = out.cpu().numpy()
    assert np.array_equal(got[:chunk], ref_repair(oracle_mod, lost)[0]) and (got[chunk:] == FILL).all()
    assert np.array_equal(dev.cpu().numpy(), host)
