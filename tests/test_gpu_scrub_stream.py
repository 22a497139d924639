"""The streaming scrub of (10,4,13) on the GPU: the compare-ending k_stream_encode ("stream-scrub").

As in test_gpu_scrub.py the expected mask of every case comes from the oracle (bit j = the stored
parity chunk j differs from the oracle's parity of the stored data), `result` is pre-filled with
0xFFFFFFFF, every buffer has gaps of random bytes between its chunks, and after every call the
device buffers are byte-identical to the upload.  Every byte position of the sub-chunks is an
independent codeword, so where one data byte is flipped in a large stripe the oracle is asked for
the parity of the column pair holding the flip only; the other columns are the clean codeword's.

What each sub-chunk size exercises in the kernel is asserted in test_scrub_stream_shapes_cpu.py.

test_every_parity_byte_stream flips stored parity bytes one at a time (schedules: scrub_sweeps.py,
checked in test_scrub_coverage_cpu.py): every byte at sc = 16, 24 and 264, the lane classes and
tile edges at the larger sizes.  Every case prints its wall time (-s); the slowest measured on an
MI355X: 1.09 s (66176-tile-edges, 14,688 calls at 74 us), 0.75 s for each of the 16 cases at 264
(16,896 calls at 44 us), 0.73 s for 2288-rows (18,304 calls at 40 us).
"""
import numpy as np
import pytest

import clay_amd
import scrub_sweeps as sw
from clay_amd import ClayCode
from stream_cut import dump_tiles
from test_gpu_scrub import Stripes, _codeword, _expected, _oracle_parity, _places

pytestmark = pytest.mark.gpu

CFG = (10, 4, 13)
SIZES = [16, 24, 1064, 2048, 2288, 66176, 66184]
LARGE = 60000  # from here on: the clean case, one flip per parity chunk, one data flip
# the last byte of one tile and the first byte of the next (test_scrub_stream_shapes_cpu.py):
# slots 0 / 1 of XCD 0, and round 0 / round 1 of XCD 0
BOUNDARY = {2288: 144, 66176: 4608}


def _expected_pair(o, c, stored, sc, at):
    """Mask of a stored stripe that is the clean codeword outside the column pair holding chunk
    offset `at`: the oracle's parity of that pair of byte positions against the stored one."""
    col = (at % sc) & ~1
    cols = stored.reshape(c.n, c.sub_chunk_no, sc)[:, :, col:col + 2]
    par = _oracle_parity(o, c, np.ascontiguousarray(cols[:c.k]).reshape(c.k, -1), 2)
    return sum(1 << j for j in range(c.m) if not np.array_equal(cols[c.k + j].reshape(-1), par[j]))


@pytest.fixture(scope="module")
def codewords(oracle_mod):
    """sc -> the oracle's codeword (n, 256 * sc), computed once and left unchanged."""
    c, o = ClayCode(*CFG), oracle_mod.OracleClay(*CFG)
    cache = {}

    def get(sc):
        if sc not in cache:
            cache[sc] = _codeword(o, c, sc, *CFG, sc, 11)
            cache[sc].setflags(write=False)
        return cache[sc]
    return get


@pytest.mark.parametrize("sc", SIZES)
def test_one_stripe_stream(oracle_mod, torch_cuda, codewords, sc):
    c, o = ClayCode(*CFG), oracle_mod.OracleClay(*CFG)
    cw = codewords(sc)
    st = Stripes(torch_cuda, c, [cw], seed=sc)
    ref_parity = cw[c.k:]
    large = sc >= LARGE
    prev = clay_amd.set_exec_mode("stream")
    try:
        assert st.scrub_one() == 0
        assert clay_amd.last_exec_path() == "stream-scrub" and clay_amd.last_launch_count() == 1
        places = _places(c, sc)
        flips = [(places[2], j) for j in range(c.m)] if large else [(at, j) for at in places for j in range(c.m)]
        if sc in BOUNDARY:  # both sides of the lane predicate, in a middle layer
            mid = (c.sub_chunk_no // 2) * sc + BOUNDARY[sc]
            flips += [(mid - 1, 1), (mid, 1), (mid - 1, 2), (mid, 2)]
        for n, (at, j) in enumerate(flips):
            st.flip(0, c.k + j, at, 1 << (n % 8))
            want = _expected(o, c, st.stored(0), sc, ref_parity)
            assert want == 1 << j  # exactly one bit: the data are the codeword's
            got = st.scrub_one()
            st.flip(0, c.k + j, at, 1 << (n % 8))
            assert got == want, (at, j, got, want)
        for pi, at in enumerate(places[1:2] if large else places):
            node = (pi * 3 + 1) % c.k
            st.flip(0, node, at, 0x04)
            want = _expected_pair(o, c, st.stored(0), sc, at) if large else _expected(o, c, st.stored(0), sc)
            assert want != 0
            got = st.scrub_one()
            st.flip(0, node, at, 0x04)
            assert got == want, (at, node, got, want)
        assert clay_amd.last_exec_path() == "stream-scrub"
        assert st.scrub_one() == 0
    finally:
        clay_amd.set_exec_mode(prev)


def test_batch_forms_stream(oracle_mod, torch_cuda):
    """3 stripes, strided and pointer-array forms: one launch per stripe, one path name."""
    c, o = ClayCode(*CFG), oracle_mod.OracleClay(*CFG)
    sc = 1064
    st = Stripes(torch_cuda, c, [_codeword(o, c, sc, *CFG, sc, i) for i in range(3)], seed=3)
    prev = clay_amd.set_exec_mode("stream")
    try:
        def run_all(want):
            for call in (st.scrub_strided, st.scrub_batch):
                call()
                assert clay_amd.last_exec_path() == "stream-scrub" and clay_amd.last_launch_count() == 3
                assert st.masks() == want

        run_all([0, 0, 0])
        places = _places(c, sc)
        st.flip(0, c.k + 3, places[2])  # first stripe: a parity flip
        st.flip(2, c.k - 1, places[1])  # last stripe: a data flip
        want = [_expected(o, c, st.stored(s), sc) for s in range(3)]
        assert want[0] == 8 and want[1] == 0 and want[2] != 0
        run_all(want)
    finally:
        clay_amd.set_exec_mode(prev)


def test_falls_back_when_not_eligible(oracle_mod, torch_cuda):
    """Odd sub-chunks and chunks off 8-byte alignment stay on v1 under "stream"; "grouped" is v1."""
    c, o = ClayCode(*CFG), oracle_mod.OracleClay(*CFG)
    for mode, sc, shift in (("stream", 133, 0), ("stream", 1064, 3), ("grouped", 2048, 0)):
        cw = _codeword(o, c, sc, *CFG, sc, shift)
        st = Stripes(torch_cuda, c, [cw], shift=shift, seed=sc)
        prev = clay_amd.set_exec_mode(mode)
        try:
            assert st.scrub_one() == 0
            assert clay_amd.last_exec_path() == "bs-scrub" and clay_amd.last_launch_count() == 1
            st.flip(0, c.k + 2, _places(c, sc)[1])
            want = _expected(o, c, st.stored(0), sc, cw[c.k:])
            assert want == 4 and st.scrub_one() == want
            st.flip(0, c.k + 2, _places(c, sc)[1])
            st.flip(0, 4, _places(c, sc)[2])
            want = _expected(o, c, st.stored(0), sc)
            assert want != 0 and st.scrub_one() == want
            assert clay_amd.last_exec_path() == "bs-scrub"
        finally:
            clay_amd.set_exec_mode(prev)


def test_capture_replay_stream(oracle_mod, torch_cuda):
    """A captured "stream" scrub (the clear, then the kernel) replays on changed bytes."""
    torch = torch_cuda
    c, o = ClayCode(*CFG), oracle_mod.OracleClay(*CFG)
    sc, j = 2288, 2
    cw = _codeword(o, c, sc, *CFG, sc, 77)
    st = Stripes(torch, c, [cw], seed=77)
    prev = clay_amd.set_exec_mode("stream")
    try:
        assert st.scrub_one() == 0  # warm: the device is open, the kernel's LDS attribute set
        side = torch.cuda.Stream()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            st.scrub_strided(stream=torch.cuda.current_stream().cuda_stream)
        assert clay_amd.last_exec_path() == "stream-scrub" and clay_amd.last_launch_count() == 1
        at = _places(c, sc)[1]
        for flip in (False, True, False):
            if flip:
                st.flip(0, c.k + j, at, 0xFF)
            want = [_expected(o, c, st.stored(0), sc, cw[c.k:])]
            assert want == ([1 << j] if flip else [0])
            st.res.fill_(-1)
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            assert st.masks() == want
            if flip:
                st.flip(0, c.k + j, at, 0xFF)
        del g
        torch.cuda.synchronize()
    finally:
        clay_amd.set_exec_mode(prev)


@pytest.fixture(scope="module")
def sweep_tiles(tmp_path_factory):
    """sc -> the tiles of the streaming kernel (stream_tile_dump, as test_scrub_stream_shapes_cpu.py)."""
    return dump_tiles(tmp_path_factory.mktemp("sweep_tiles"), sorted({case[0] for case in sw.stream_cases()}))


@pytest.mark.parametrize("case", sw.stream_cases(), ids=sw.case_id)
def test_every_parity_byte_stream(torch_cuda, codewords, sweep_tiles, case):
    """Every flip of the case (scrub_sweeps.stream_flips: the full product at 16, 24 and 264; at
    1064 and 2288 every byte of eight layers and every layer at the tile edges and the ragged
    tile's 16-byte boundaries; at 66176 and 66184 the tile edges in one layer per group) alone in
    the stored parity: the mask is exactly 1 << j.  One clay_scrub_device call per flip into its
    own result word, one synchronise at the end."""
    c = ClayCode(*CFG)
    sc = case[0]
    cw = codewords(sc)
    st = Stripes(torch_cuda, c, [cw], seed=sc)
    jj, at = sw.stream_flips(case, sweep_tiles[sc])
    prev = clay_amd.set_exec_mode("stream")
    try:
        sw.run_flip_loop(torch_cuda, clay_amd, st, jj, at, cw[c.k:], "stream-scrub", "stream sweep " + sw.case_id(case))
    finally:
        clay_amd.set_exec_mode(prev)


@pytest.mark.slow
def test_auto_at_benchmark_subchunk(oracle_mod, torch_cuda):
    """The 1 GiB stripe's sub-chunk (419,432) lies above auto's gate: the streaming kernel without
    any exec mode set.  Parity by clay_encode_device, column slices of it checked against the
    oracle; the masks of the flips come from the oracle's parity of the column pair holding them."""
    torch = torch_cuda
    c, o = ClayCode(*CFG), oracle_mod.OracleClay(*CFG)
    sc, alpha = 419_432, c.sub_chunk_no
    chunk = alpha * sc
    g = torch.Generator(device="cuda")
    g.manual_seed(20261020)
    full = torch.randint(0, 256, (c.n, chunk), dtype=torch.uint8, device="cuda", generator=g)
    dl, pl = [full[i] for i in range(c.k)], [full[c.k + j] for j in range(c.m)]
    res = torch.empty(1, dtype=torch.int32, device="cuda")

    def cols(col, w):
        """Positions [col, col + w) of every sub-chunk of every chunk: (n, alpha * w) on the host."""
        return full.view(c.n, alpha, sc)[:, :, col:col + w].contiguous().view(c.n, alpha * w).cpu().numpy()

    def expected(col, w):
        stored = cols(col, w)
        par = _oracle_parity(o, c, stored[:c.k], w)
        return sum(1 << j for j in range(c.m) if not np.array_equal(stored[c.k + j], par[j]))

    def scrub():
        res.fill_(-1)
        c.scrub_device(dl, pl, res, chunk)
        assert clay_amd.last_exec_path() == "stream-scrub" and clay_amd.last_launch_count() == 1
        return int(res.cpu().numpy().view(np.uint32)[0])

    prev = clay_amd.set_exec_mode("auto")
    try:
        c.encode_device(dl, pl, chunk)
        torch.cuda.synchronize()
        for col in (0, (sc // 2) & ~63, sc - 64):
            assert expected(col, 64) == 0, col
        assert scrub() == 0
        j, at = 2, 131 * sc + 200_001  # a parity byte in a middle layer
        full[c.k + j, at] ^= 0x20
        assert expected((at % sc) & ~1, 2) == 1 << j
        assert scrub() == 1 << j
        full[c.k + j, at] ^= 0x20
        at = 77 * sc + sc - 3  # a data byte near a row end
        full[6, at] ^= 0x01
        want = expected((at % sc) & ~1, 2)
        assert want != 0 and scrub() == want
        full[6, at] ^= 0x01
        assert scrub() == 0
    finally:
        clay_amd.set_exec_mode(prev)
