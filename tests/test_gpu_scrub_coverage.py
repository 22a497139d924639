"""Scrub on the GPU, exhaustively: every stored parity byte flipped alone must be reported.

A compare that skips some stored bytes is clean on a clean stripe and right for a flip anywhere
else, so the property here is: for a codeword taken from the oracle, one flipped bit in any single
byte of parity chunk j makes the mask exactly 1 << j.  The bit cycles with position and chunk
(scrub_sweeps.flip_bits); the expected masks are computed from the flip schedule and the oracle's
parity (scrub_sweeps.expected_masks).  The schedules are checked in test_scrub_coverage_cpu.py.

  test_batch_sweep     k_bs_encode1 / k_bs_encode SCRUB through clay_scrub_device_batch with pointer
                       arrays (every stripe the same k data pointers: a data stripe stride of 0),
                       one launch per pass: stripe s of a slab has byte p0 + s flipped, in parity
                       chunk (s + r) % m in pass r.  Sub-chunks W + 40 (full tile, whole unit, a
                       unit of one 8-byte piece) and W + 37 shifted by 3 (the byte-tail kernels).
  test_one_stripe_sweep  the same kernels, one stripe per call at sc = 40: stripe index 0, the
                       non-batch flattening, result + i.
  test_host_verify_sweep  clay_verify of (9,3,11) at sc = 37: the pooled staging buffer, every row
                       padded to 8 bytes.

The streaming kernel's sweeps are in test_gpu_scrub_stream.py.  Data-byte flips, flips of more
than one byte and other sizes stay sampled (test_gpu_scrub.py).

Every case prints its wall time (-s).  Slowest measured case of each part on an MI355X: batch
sweep 0.29 s ((4,2,5) auto W + 40, the module's first launch; (10,4,13) 0.19 s for 44 launches),
one-stripe sweep 0.92 s ((10,4,13): 40,960 calls at 22 us), clay_verify 0.35 s (2,997 calls at
118 us).
"""
import time

import numpy as np
import pytest

import clay_amd
import scrub_sweeps as sw
from clay_amd import ClayCode
from test_gpu_scrub import TILE, Stripes, _codeword

pytestmark = pytest.mark.gpu

_IDS = ["%d-%d-%d-%s" % (*r[0], r[1]) for r in sw.BS_ROWS]


@pytest.mark.parametrize("size", sw.BS_SIZES, ids=[s[0] for s in sw.BS_SIZES])
@pytest.mark.parametrize("cfg,mode,path", sw.BS_ROWS, ids=_IDS)
def test_batch_sweep(oracle_mod, torch_cuda, cfg, mode, path, size):
    torch = torch_cuda
    c, o = ClayCode(*cfg), oracle_mod.OracleClay(*cfg)
    sc, shift = TILE[cfg] + size[1], size[2]
    cw = _codeword(o, c, sc, *cfg, sc, 31)
    ref = np.ascontiguousarray(cw[c.k:])  # the oracle's parity of the stored data
    st = Stripes(torch, c, [cw], shift=shift, seed=sc)  # its data buffer: chunks in garbage, shifted
    m, chunk = c.m, st.chunk
    data_ptrs, _ = st.ptrs(0)
    par0 = torch.from_numpy(ref).cuda()
    t0, calls = time.perf_counter(), 0
    prev = clay_amd.set_exec_mode(mode)
    try:
        for p0, ns in sw.slabs(m, chunk):
            assert ns * m * chunk <= sw.SLAB_BYTES
            # the slab [ns][m][chunk] at `shift` bytes into its allocation, replicated on the device
            buf = torch.full((shift + ns * m * chunk,), 0xA5, dtype=torch.uint8, device="cuda")
            slab = buf[shift:]
            slab.view(ns, m, chunk).copy_(par0.expand(ns, m, chunk))
            res = torch.empty(ns + sw.GUARD, dtype=torch.int32, device="cuda")
            base = slab.data_ptr()
            par_ptrs = (base + np.arange(ns * m, dtype=np.int64) * chunk).tolist()
            for r in range(m):
                jj, pos = sw.batch_pass(m, p0, ns, r)
                bits = sw.flip_bits(pos, jj)
                want = sw.expected_masks(ref, jj, pos, bits)
                idx = torch.from_numpy(np.arange(ns, dtype=np.int64) * (m * chunk) + jj * chunk + pos).cuda()
                bits_d = torch.from_numpy(bits).cuda()
                slab[idx] ^= bits_d
                res.fill_(-1)
                c.scrub_device_batch(data_ptrs * ns, par_ptrs, res, ns, chunk)
                assert clay_amd.last_exec_path() == path + "-batch" and clay_amd.last_launch_count() == 1
                slab[idx] ^= bits_d
                got = res.cpu().numpy().view(np.uint32)
                assert np.all(got[ns:] == 0xFFFFFFFF), "result words beyond the batch written"
                wrong = sw.first_wrong(got[:ns], want, jj, pos, sc)
                assert wrong is None, (p0, r, wrong)
                calls += 1
            assert torch.equal(slab.view(ns, m, chunk), par0.expand(ns, m, chunk)), "slab not restored"
            assert bool((buf[:shift] == 0xA5).all())
            if p0 == 0:
                assert np.array_equal(slab[:m * chunk].cpu().numpy().reshape(m, chunk), ref)
            del buf, slab, res
        for fam in (0, 1):
            assert np.array_equal(st.dev[fam].cpu().numpy(), st.host[fam]), "scrub wrote to its inputs"
    finally:
        clay_amd.set_exec_mode(prev)
    print(f"batch sweep {cfg} {mode} sc={sc} shift={shift}: {m * chunk} flips in {calls} launches, "
          f"{time.perf_counter() - t0:.2f} s")


@pytest.mark.parametrize("cfg,mode,path", sw.BS_ROWS, ids=_IDS)
def test_one_stripe_sweep(oracle_mod, torch_cuda, cfg, mode, path):
    c, o = ClayCode(*cfg), oracle_mod.OracleClay(*cfg)
    sc = sw.ONE_SC
    cw = _codeword(o, c, sc, *cfg, sc, 32)
    st = Stripes(torch_cuda, c, [cw], seed=sc)
    jj, pos = sw.all_flips(c.m, st.chunk)
    prev = clay_amd.set_exec_mode(mode)
    try:
        sw.run_flip_loop(torch_cuda, clay_amd, st, jj, pos, np.ascontiguousarray(cw[c.k:]), path,
                         f"one-stripe sweep {cfg} {mode} sc={sc}")
    finally:
        clay_amd.set_exec_mode(prev)


@pytest.mark.parametrize("j", range(sw.VERIFY_CFG[1]))
def test_host_verify_sweep(oracle_mod, torch_cuda, j):
    cfg, sc = sw.VERIFY_CFG, sw.VERIFY_SC
    c, o = ClayCode(*cfg), oracle_mod.OracleClay(*cfg)
    cw = _codeword(o, c, sc, *cfg, sc, 33)
    ref = np.ascontiguousarray(cw[c.k:])
    chunk = cw.shape[1]
    assert chunk == 2997
    jj, pos = sw.all_flips(c.m, chunk)
    jj, pos = jj[jj == j], pos[jj == j]
    bits = sw.flip_bits(pos, jj)
    want = sw.expected_masks(ref, jj, pos, bits)
    rows = [cw[i].copy() for i in range(c.n)]
    assert c.verify(rows) == 0
    got = np.zeros(len(jj), np.uint32)
    t0 = time.perf_counter()
    for i, (p, b) in enumerate(zip(pos.tolist(), bits.tolist())):
        rows[c.k + j][p] ^= b
        got[i] = c.verify(rows)
        rows[c.k + j][p] ^= b
    dt = time.perf_counter() - t0
    print(f"verify sweep {cfg} sc={sc} j={j}: {len(jj)} calls, {dt:.2f} s, {1e6 * dt / len(jj):.0f} us per call")
    wrong = sw.first_wrong(got, want, jj, pos, sc)
    assert wrong is None, wrong
    assert np.array_equal(np.stack(rows), cw) and c.verify(rows) == 0
