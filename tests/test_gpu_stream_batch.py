"""The batched streaming encode (k_stream_encode BATCH: many (10,4,13) / (9,4,12) stripes in ONE
launch, path "stream-batch-k..."), bit for bit against the oracle, stripe by stripe.

Every case builds its buffers the same way: data and parity each in one allocation, chunks padded
apart (8 bytes between nodes, more between stripes, the data family's stripe stride different from
the parity family's), a guard band at both ends, the parity allocation pre-filled with 0xA5.  After
the call every byte outside the parity chunks must still be 0xA5, every parity chunk must equal the
oracle's, and the data allocation must be unchanged.

The shapes are derived from the device's workgroups per XCD (multi_processor_count // 8) with a
Python restatement of the batch map (BatchMap, clay_amd/csrc/stream_tile_map.hpp; values for the
MI355X's 32 in brackets):
  one_piece     "stream", sc 16: one 16-byte tile on XCD 0 only, loaded with clamped addresses;
                n = 2 * G + 6 [70]: groups run 3 and 2 stripes back to back
  ragged        "stream", sc 24: the row end is not a multiple of 16 (patched piece, plain stores,
                a wait for everything in flight), and another stripe's tile follows it directly
  full          auto, sc 2048: whole 256-byte tiles, one workgroup per stripe and XCD;
                n = G + 5 [37]: groups with 2 stripes and with 1; the prefetch crosses the stripe seam
  few3 / few2   auto, sc 2048, 3 and 2 stripes: fewer stripes than groups, the grid shrinks
  narrow        auto, sc 2288: 2 workgroups per stripe and XCD, tiles 144 bytes wide (masked store
                pairs); n = 2 * G + 3 [35, G = 16]
  idle_ragged   auto, sc 8216: 5 workgroups per stripe and XCD [G = 6, 2 unlaunched slots per XCD],
                sc = 8 mod 16; n = G + 1 [7]
  two_rounds    auto, sc = 2048 * per_xcd + 648 [66184], 2 stripes: one group of every workgroup,
                two tiles per stripe and workgroup, then the next stripe's, sc = 8 mod 16
  k9            auto, (9,4,12) at the narrow shape
The oracle's codewords are computed once per (code, sc, n) and shared by the cases of that shape.
"""
import functools

import numpy as np
import pytest

from clay_amd import ClayCode, last_encode_path, last_launch_count, set_encode_path
from stream_cut import batch_groups, stream_cut

FILL = 0xA5
GUARD = 4096


def batch_shape(sc, n, per_xcd):
    """(workgroups per stripe and XCD, groups per XCD, unlaunched slots per XCD, rounds of XCD 0,
    stripes per group) as launch_stream_batch (engine.hip: stream_cut, batch_groups) and BatchMap
    cut a batch."""
    region, ns = stream_cut(sc, per_xcd)
    groups = batch_groups(per_xcd, ns, n)
    rounds = -(-min(region, sc) // (ns * 256))
    return ns, groups, max(0, per_xcd - groups * ns), rounds, [len(range(j, n, groups)) for j in range(groups)]


def case_shape(name, per_xcd):
    """(cfg, mode, sc, n) of a named case on a device with per_xcd workgroups per XCD."""
    k10, k9 = (10, 4, 13), (9, 4, 12)
    g1 = per_xcd                    # groups of one workgroup
    g2 = max(1, per_xcd // 2)       # groups of two
    g5 = max(1, per_xcd // 5)       # groups of five
    return {
        "one_piece": (k10, "stream", 16, 2 * g1 + 6),
        "ragged": (k10, "stream", 24, 2 * g1 + 6),
        "full": (k10, "auto", 2048, g1 + 5),
        "few3": (k10, "auto", 2048, 3),
        "few2": (k10, "auto", 2048, 2),
        "narrow": (k10, "auto", 2288, 2 * g2 + 3),
        "idle_ragged": (k10, "auto", 8216, g5 + 1),
        "two_rounds": (k10, "auto", 2048 * per_xcd + 648, 2),
        "k9": (k9, "auto", 2288, 2 * g2 + 3),
    }[name]


CASES = ["one_piece", "ragged", "full", "few3", "few2", "narrow", "idle_ragged", "two_rounds", "k9"]


def test_case_shapes_on_256_cus():
    """The shapes on the MI355X's 32 workgroups per XCD (no GPU: a check of this file's own
    restatement of the map against the figures the kernel's host check pins)."""
    got = {name: case_shape(name, 32) for name in CASES}
    assert [got[n][2:] for n in CASES] == [(16, 70), (24, 70), (2048, 37), (2048, 3), (2048, 2), (2288, 35), (8216, 7),
                                           (66184, 2), (2288, 35)]
    assert batch_shape(16, 70, 32)[:4] == (1, 32, 0, 1) and sorted(set(batch_shape(16, 70, 32)[4])) == [2, 3]
    assert batch_shape(2048, 37, 32)[:4] == (1, 32, 0, 1) and sorted(set(batch_shape(2048, 37, 32)[4])) == [1, 2]
    assert batch_shape(2048, 3, 32)[:2] == (1, 3) and batch_shape(2048, 2, 32)[:2] == (1, 2)
    assert batch_shape(2288, 35, 32)[:4] == (2, 16, 0, 1) and sorted(set(batch_shape(2288, 35, 32)[4])) == [2, 3]
    assert batch_shape(8216, 7, 32)[:4] == (5, 6, 2, 1) and sorted(set(batch_shape(8216, 7, 32)[4])) == [1, 2]
    assert batch_shape(66184, 2, 32) == (32, 1, 0, 2, [2])
    for name in CASES:  # auto only takes stripes above the staged batch's 4 MiB
        cfg, mode, sc, n = got[name]
        assert mode == "stream" or cfg[0] * 256 * sc > 4 << 20, name


@functools.lru_cache(maxsize=2)
def _reference(cfg, sc, n):
    """(data [n, k, chunk], parity [n, m, chunk]) of n stripes of random data, the parity the
    oracle's; read-only, shared by the cases of one shape."""
    from oracle import oracle
    oracle.build()
    k, m, d = cfg
    o = oracle.OracleClay(k, m, d)
    chunk = 256 * sc
    rng = np.random.default_rng(7 * sc + n + 1000 * k)
    data = np.empty((n, k, chunk), np.uint8)
    par = np.empty((n, m, chunk), np.uint8)
    for s in range(n):
        data[s] = np.frombuffer(rng.bytes(k * chunk), np.uint8).reshape(k, chunk)
        cw = o.encode_array(data[s].reshape(-1))
        assert cw.shape == (k + m, chunk) and np.array_equal(cw[:k], data[s])
        par[s] = cw[k:]
    data.setflags(write=False)
    par.setflags(write=False)
    return data, par


class Buffers:
    """One family (data or parity) of n stripes x per chunks in one allocation: guard band, then
    stripe s at s * stripe, node i of it at i * node (node = chunk + pad), guard band."""

    def __init__(self, torch, n, per, chunk, pad, stripe_pad, fill):
        self.n, self.per, self.chunk = n, per, chunk
        self.node = chunk + pad
        self.stripe = per * self.node + stripe_pad
        self.host = np.full(2 * GUARD + n * self.stripe, fill, np.uint8)
        self.torch = torch
        self.dev = None

    def off(self, s, i):
        return GUARD + s * self.stripe + i * self.node

    def put(self, chunks):  # chunks[s][i]: bytes of node i of stripe s
        for s in range(self.n):
            for i in range(self.per):
                o = self.off(s, i)
                self.host[o:o + self.chunk] = chunks[s][i]

    def upload(self):
        self.dev = self.torch.from_numpy(self.host).cuda()
        return self

    def base(self):
        return self.dev[GUARD:]

    def ptrs(self):
        return [self.dev[self.off(s, i):] for s in range(self.n) for i in range(self.per)]

    def same_as_host(self):
        """Is the device allocation byte for byte the host image?  Else the first difference."""
        got = self.dev.cpu().numpy()
        if np.array_equal(got, self.host):
            return None
        at = int(np.flatnonzero(got != self.host)[0])
        rel = at - GUARD
        s, r = divmod(rel, self.stripe)
        return f"byte {at} (stripe {s}, node {r // self.node}, offset {r % self.node} of chunk {self.chunk}): " \
               f"{got[at]:#x}, expected {self.host[at]:#x}"


def encode_and_check(torch, cfg, sc, n, form="strided", pad=8, data_stripe_pad=40, par_stripe_pad=24, split=None):
    """Encode n stripes through one batched entry point and compare the whole parity allocation
    (chunks = the oracle's, everything else still FILL) and the data allocation.  split = (s, i):
    data chunk i of stripe s lives in an allocation of its own (pointer-array form only)."""
    k, m, d = cfg
    c = ClayCode(k, m, d)
    chunk = c.sub_chunk_no * sc
    data, ref = _reference(cfg, sc, n)
    D = Buffers(torch, n, k, chunk, pad, data_stripe_pad, 0x5A)
    D.put(data)
    D.upload()
    P = Buffers(torch, n, m, chunk, pad, par_stripe_pad, FILL).upload()
    P.put(ref)  # the host image is now what the device must hold afterwards
    if form == "strided":
        assert split is None
        c.encode_device_strided(D.base(), P.base(), n, chunk, D.node, D.stripe, P.node, P.stripe)
    else:
        dp = D.ptrs()
        if split is not None:
            s, i = split
            dp[s * k + i] = torch.from_numpy(data[s][i].copy()).cuda()
        c.encode_device_batch(dp, P.ptrs(), n, chunk)
    torch.cuda.synchronize()
    path, launches = last_encode_path(), last_launch_count()
    bad = P.same_as_host()
    assert bad is None, f"parity {cfg} sc {sc} n {n} via {path}: {bad}"
    bad = D.same_as_host()
    assert bad is None, f"data changed {cfg} sc {sc} n {n} via {path}: {bad}"
    return path, launches


def _per_xcd(torch):
    return max(1, torch.cuda.get_device_properties(0).multi_processor_count // 8)


@pytest.fixture
def encode_path():
    """set_encode_path for the test, auto afterwards."""
    yield set_encode_path
    set_encode_path("auto", 0)


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_stream_batch_matches_oracle(torch_cuda, encode_path, name):
    cfg, mode, sc, n = case_shape(name, _per_xcd(torch_cuda))
    encode_path(mode, 0)
    path, launches = encode_and_check(torch_cuda, cfg, sc, n)
    assert path == f"stream-batch-k{cfg[0]}m4-w256-l4", (name, path)
    assert launches == 1, (name, launches)


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["strided", "arrays"])
@pytest.mark.parametrize("mode,variant,sc", [("auto", 0, 2048), ("stream", 4, 24)])
def test_strided_and_pointer_array_forms(torch_cuda, encode_path, form, mode, variant, sc):
    """Rows of one allocation, named by strides or by pointer arrays: both are the batch.  The data
    stripe stride differs from the parity stripe stride, and the node pad of 8 bytes puts every
    other chunk on an address that is 8 but not 16 mod 16."""
    n = 5
    encode_path(mode, variant)
    path, launches = encode_and_check(torch_cuda, (10, 4, 13), sc, n, form=form, pad=8, data_stripe_pad=72, par_stripe_pad=8)
    assert path == "stream-batch-k10m4-w256-l4" and launches == 1, (path, launches)


@pytest.mark.gpu
def test_fallbacks_keep_their_paths(torch_cuda, encode_path):
    """What the batch does not take runs as before, and equals the oracle all the same."""
    torch = torch_cuda
    cfg, n = (10, 4, 13), 5
    # one data chunk in an allocation of its own: off the stride, one launch per stripe
    path, launches = encode_and_check(torch, cfg, 2048, n, form="arrays", split=(3, 7))
    assert "stream-batch" not in path and path == "stream-k10m4-w256-l4" and launches == n, (path, launches)
    # a pad of 4 bytes: every other chunk off 8-byte alignment
    path, launches = encode_and_check(torch, cfg, 2048, n, pad=4, data_stripe_pad=8, par_stripe_pad=8)
    assert "stream-batch" not in path, path
    # stripes of 2.6 MiB under auto: the staged batch (the 4 MiB rule)
    path, launches = encode_and_check(torch, cfg, 1064, n)
    assert path == "staged-batch", path
    # "stream" with 2 loader waves: one launch per stripe
    encode_path("stream", 2)
    path, launches = encode_and_check(torch, cfg, 2048, n)
    assert path == "stream-k10m4-w256-l2" and launches == n, (path, launches)


@pytest.mark.gpu
def test_auto_keeps_the_loop_above_its_gate(torch_cuda, encode_path):
    """Above kStreamBatchMaxSc (engine.hip: 262,152) auto keeps one launch per stripe; "stream"
    still takes the batch there, and both write the same parity (the per-stripe kernel's, which
    test_gpu_stream_encode_balanced.py holds to the oracle: no oracle run at 640 MiB per stripe)."""
    torch = torch_cuda
    c = ClayCode(10, 4, 13)
    sc, n = 262152 + 8, 2
    chunk = c.sub_chunk_no * sc
    g = torch.Generator(device="cuda")
    g.manual_seed(5)
    data = torch.randint(0, 256, (n, 10, chunk), dtype=torch.uint8, device="cuda", generator=g)
    pars = [torch.full((n, 4, chunk), FILL, dtype=torch.uint8, device="cuda") for _ in range(2)]
    c.encode_device_strided(data, pars[0], n, chunk)
    torch.cuda.synchronize()
    assert (last_encode_path(), last_launch_count()) == ("stream-k10m4-w256-l4", n)
    encode_path("stream", 0)
    c.encode_device_strided(data, pars[1], n, chunk)
    torch.cuda.synchronize()
    assert (last_encode_path(), last_launch_count()) == ("stream-batch-k10m4-w256-l4", 1)
    assert torch.equal(pars[0], pars[1])


@pytest.mark.gpu
def test_batch_first_met_inside_a_capture(torch_cuda):
    """No allocation, no pointer table: a batch of a shape never run before is captured without a
    warm call and replayed twice on changed data, each replay equal to the oracle."""
    torch = torch_cuda
    cfg, sc, n = (10, 4, 13), 2064, 4
    k, m, d = cfg
    c = ClayCode(k, m, d)
    chunk = c.sub_chunk_no * sc
    data, ref = _reference(cfg, sc, 2 * n)  # two batches' worth: one per replay
    D = Buffers(torch, n, k, chunk, 8, 40, 0x5A)
    P = Buffers(torch, n, m, chunk, 8, 24, FILL)
    D.upload()
    P.upload()
    # the device's own state (tables every call shares) exists before the capture; this is another
    # code at another size, not a call of the captured shape
    small = ClayCode(4, 2, 5)
    z = torch.zeros((6, small.sub_chunk_no * 32), dtype=torch.uint8, device="cuda")
    small.encode_device([z[i] for i in range(4)], [z[4], z[5]], small.sub_chunk_no * 32)
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=st):
        c.encode_device_strided(D.base(), P.base(), n, chunk, D.node, D.stripe, P.node, P.stripe, 0,
                                torch.cuda.current_stream().cuda_stream)
    assert last_encode_path() == "stream-batch-k10m4-w256-l4" and last_launch_count() == 1
    for rep in range(2):
        D.put(data[rep * n:(rep + 1) * n])
        D.dev.copy_(torch.from_numpy(D.host))
        P.dev.fill_(FILL)
        P.host[:] = FILL
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        P.put(ref[rep * n:(rep + 1) * n])
        bad = P.same_as_host()
        assert bad is None, f"replay {rep}: {bad}"
        assert D.same_as_host() is None
