"""Every erasure pattern of every listed code through each decode kernel it can reach, data AND
parity outputs against the oracle on non-codeword input.

Decode is where the erasure pattern changes the path: every pattern has its own cached plan
(plan.cpp), the streaming kernels a per-pattern device table, and k_stream_fused2 a per-pattern
loader-wave split, ring and split-step choice (decode_pattern.hpp f2_plan / fused2_shape).  The
other decode tests sample the 3- and 4-erasure patterns; here none is left out.

 * streaming codes ((10,4,13), (9,4,12)) at sc = 520 -- eight full 64-byte tiles (two 256-byte runs)
   plus an 8-byte ragged tail, the smallest size at which every pattern meets both the full-tile
   and the tail code of the streaming kernels (sc >= 512, sc % 8 == 0): exec modes "auto",
   "stream-local" and "stream-fused2", the kernel that ran asserted per mode from the predicates of
   tests/decode_pattern.py;
 * every code at sc = 22 (one 16-byte piece, one 4-byte piece, a 2-byte tail; below 512, so no
   streaming kernel applies): the plan executors, "grouped" and "tile".

The input of a case is ONE seeded random stripe, not a codeword, so only the reference's RS row
choice and iscore order reproduce the bytes.  The reference of a pattern is
OracleClay.decode_chunks: every erased chunk, the parity chunks included (decode.rs:213-253).
Outputs go into a 0xA5-filled (n, chunk) buffer between two guard bands: every erased row equals
the oracle's, every other byte is still 0xA5, and the device stripe is unchanged at the end.
Patterns with two or more erased parity nodes run once more with only one of them requested.

Sizes other than 520 and 22, batched decodes, clay_decode_device_codeword and repair stay with
the sampled patterns of the other files."""
import itertools
import math
import resource
import time
from collections import Counter

import numpy as np
import pytest

import clay_amd
from clay_amd import ClayCode
from decode_pattern import fused2_eligible, local_eligible, stream_path
from test_gpu_batch_repair import FILL, GUARD, guarded
from test_gpu_parity import CONFIGS as PARITY_CONFIGS

STREAM_CONFIGS = [(10, 4, 13), (9, 4, 12)]
PLAN_CONFIGS = PARITY_CONFIGS + [(9, 4, 12)]
SC_STREAM = 520
SC_PLAN = 22
PLAN_PATHS = ("tile", "grouped")
LOCAL_PATHS = ("stream-local256", "stream-local")
# codes with a decode or repair plan that the other files show on the tile-fused executor
# (test_gpu_parity.py: test_tile_executor_selected under "tile", test_small_decode_plan_executor)
TILE_CODES = [(9, 3, 11), (10, 4, 13), (4, 2, 5)]


def n_patterns(cfg):
    return sum(math.comb(cfg[0] + cfg[1], r) for r in range(1, cfg[1] + 1))


# Slices patterns[j::S] of a code's pattern list, one parametrized case each, at most 200 patterns
# a case: 8 slices for (10,4,13), 6 for (9,4,12), 4 for (8,4,11), 3 for (7,4,9), 2 for (9,3,11).
# A streaming case is the slower kind (four decodes, two plans and the path predicates in
# Python per pattern): 1.6 s measured for the slowest one, 0.3 s for the slowest plan-executor case.
STREAM_SLICES = {cfg: -(-n_patterns(cfg) // 200) for cfg in STREAM_CONFIGS}
PLAN_SLICES = {cfg: -(-n_patterns(cfg) // 200) for cfg in PLAN_CONFIGS}
STREAM_CASES = [(cfg, j) for cfg in STREAM_CONFIGS for j in range(STREAM_SLICES[cfg])]
PLAN_CASES = [(cfg, j) for cfg in PLAN_CONFIGS for j in range(PLAN_SLICES[cfg])]


def all_patterns(c):
    """Every erasure pattern, r = 1..m in that order."""
    return [list(e) for r in range(1, c.m + 1) for e in itertools.combinations(range(c.n), r)]


_expected = {}


def expected_paths(cfg, c, er):
    """Per exec mode, the paths the host may report for this pattern at SC_STREAM."""
    key = (cfg, tuple(er))
    if key not in _expected:
        auto = stream_path(c, er)
        _expected[key] = {
            "auto": (auto,) if auto else PLAN_PATHS,
            "stream-local": LOCAL_PATHS if local_eligible(c, er) else PLAN_PATHS,
            "stream-fused2": ("stream-fused2",) if fused2_eligible(c, er, two=True) else PLAN_PATHS,
        }
    return _expected[key]


_stripes = {}


def stripe(cfg, c, sc):
    """(n, alpha * sc) seeded random bytes: one non-codeword stripe per (code, size).  Read-only."""
    if (cfg, sc) not in _stripes:
        a = np.random.default_rng([sc, cfg[0], cfg[1], 23]).integers(0, 256, (c.n, c.sub_chunk_no * sc), dtype=np.uint8)
        a.setflags(write=False)
        _stripes[cfg, sc] = a
    return _stripes[cfg, sc]


def decode_into(torch, c, full, er, want, flat, outs, chunk):
    """One decode_device of pattern `er` with the outputs of nodes `want` requested, into the
    0xA5-refilled guarded buffer -> (the whole buffer on the host, the path that ran)."""
    flat.fill_(FILL)
    c.decode_device([None if i in er else full[i] for i in range(c.n)], er,
                    [outs[i] if i in want else None for i in range(c.n)], chunk)
    torch.cuda.synchronize()
    return flat.cpu().numpy(), clay_amd.last_exec_path()


def check_outputs(host, ref, want, ctx):
    """Rows `want` equal the oracle's, every other row and both guards are still 0xA5."""
    n, chunk = ref.shape
    exp = np.full(GUARD + n * chunk + GUARD, FILL, np.uint8)
    body = exp[GUARD:GUARD + n * chunk].reshape(n, chunk)
    for e in want:
        body[e] = ref[e]
    if np.array_equal(host, exp):
        return
    assert (host[:GUARD] == FILL).all() and (host[-GUARD:] == FILL).all(), ("bytes written outside the output", ctx)
    got = host[GUARD:GUARD + n * chunk].reshape(n, chunk)
    for i in range(n):
        bad = np.flatnonzero(got[i] != body[i])
        if bad.size:
            what = "erased chunk differs from the oracle" if i in want else "row written though not requested"
            raise AssertionError((what, ctx, "node", i, "bytes", int(bad.size), "first", int(bad[0])))


def report(torch, what, t0=None, paths=None):
    """The figures of one case, printed (pytest -s): wall time, path counts, peak RSS, device memory."""
    free, total = torch.cuda.mem_get_info()
    line = (f"{what}: peak RSS {resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 1024:.0f} MiB, "
            f"device free {free >> 20} of {total >> 20} MiB")
    if t0 is not None:
        line += f", {time.perf_counter() - t0:.2f} s, paths {dict(sorted(paths.items()))}"
    print(line)


# ---------------------------------------------------------------------------
# census (CPU): which kernel the predicates send every pattern to
# ---------------------------------------------------------------------------
# per r = 1, 2, 3, 4: the "auto" paths, the patterns "stream-local" takes, those "stream-fused2" takes
CENSUS = {
    (10, 4, 13): ([{"stream-local256": 14}, {"stream-local256": 91}, {"stream-fused2": 352, "stream-local": 12},
                   {"stream-fused2": 878, "stream-local": 123}], [14, 91, 204, 123], [0, 91, 352, 878]),
    (9, 4, 12): ([{"stream-local256": 13}, {"stream-local256": 78}, {"stream-fused2": 274, "stream-local": 12},
                  {"stream-fused2": 604, "stream-local": 111}], [13, 78, 174, 111], [0, 78, 274, 604]),
}


def test_census_and_slices_cover_every_pattern():
    """Computed from the predicates alone (a change to them shows here; the GPU cases check them
    against the host's own choice): per erasure count, the kernel of every pattern under each
    mode -- no pattern of the streaming codes falls to a plan executor under "auto" -- and the
    slices of both parts are the full pattern lists, nothing skipped or sampled."""
    for cfg in STREAM_CONFIGS:
        c = ClayCode(*cfg)
        pats = all_patterns(c)
        auto = [Counter() for _ in range(4)]
        local, fused2 = [0] * 4, [0] * 4
        for er in pats:
            exp = expected_paths(cfg, c, er)
            assert len(exp["auto"]) == 1, ("a plan executor under auto", cfg, er)
            auto[len(er) - 1][exp["auto"][0]] += 1
            local[len(er) - 1] += exp["stream-local"] is LOCAL_PATHS
            fused2[len(er) - 1] += exp["stream-fused2"] == ("stream-fused2",)
        assert ([dict(a) for a in auto], local, fused2) == CENSUS[cfg], cfg
    assert n_patterns((10, 4, 13)) == 1470 and n_patterns((9, 4, 12)) == 1092
    for cases, slices in ((STREAM_CASES, STREAM_SLICES), (PLAN_CASES, PLAN_SLICES)):
        for cfg in slices:
            c = ClayCode(*cfg)
            pats = all_patterns(c)
            assert len(pats) == n_patterns(cfg) and len({tuple(p) for p in pats}) == len(pats)
            S = slices[cfg]
            js = [j for g, j in cases if g == cfg]
            assert js == list(range(S))
            parts = [pats[j::S] for j in js]
            assert max(len(p) for p in parts) <= 200
            assert sorted(p for part in parts for p in part) == sorted(pats), cfg
    assert sorted(PLAN_SLICES) == sorted(set(PARITY_CONFIGS) | {(9, 4, 12)}) and len(PLAN_SLICES) == 9


# ---------------------------------------------------------------------------
# the streaming codes: auto, stream-local, stream-fused2
# ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("cfg,j", STREAM_CASES)
def test_stream_codes_every_pattern(oracle_mod, torch_cuda, cfg, j):
    torch = torch_cuda
    c, o = ClayCode(*cfg), oracle_mod.OracleClay(*cfg)
    S = STREAM_SLICES[cfg]
    pats = all_patterns(c)
    chunk = c.sub_chunk_no * SC_STREAM
    host = stripe(cfg, c, SC_STREAM)
    assert host.shape == (c.n, chunk)
    full = torch.from_numpy(host.copy()).cuda()
    flat, outs = guarded(torch, c.n, chunk)
    outs = outs.view(c.n, chunk)
    report(torch, f"stream {cfg} slice {j}/{S} start")
    t0 = time.perf_counter()
    ran = Counter()
    prev = clay_amd.set_exec_mode("auto")
    try:
        for idx in range(j, len(pats), S):
            er = pats[idx]
            ref = o.decode_chunks({i: host[i] for i in range(c.n) if i not in er}, er)
            exp = expected_paths(cfg, c, er)
            for mode in ("auto", "stream-local", "stream-fused2"):
                clay_amd.set_exec_mode(mode)
                got, path = decode_into(torch, c, full, er, er, flat, outs, chunk)
                ran[mode, path] += 1
                check_outputs(got, ref, er, (cfg, er, mode, path))
                assert path in exp[mode], (cfg, er, mode, path, exp[mode])
            # mixed want: the data outputs and exactly one of several erased parity chunks
            parity = [e for e in er if e >= c.k]
            if len(parity) >= 2:
                want = [e for e in er if e < c.k] + [parity[0] if idx % 2 == 0 else parity[-1]]
                clay_amd.set_exec_mode("auto")
                got, path = decode_into(torch, c, full, er, want, flat, outs, chunk)
                ran["auto, one parity of several", path] += 1
                check_outputs(got, ref, want, (cfg, er, "auto", path, "want", want))
                assert path in exp["auto"], (cfg, er, want, path)
        assert np.array_equal(full.cpu().numpy(), host), "a decode wrote to its input"
    finally:
        clay_amd.set_exec_mode(prev)
    report(torch, f"stream {cfg} slice {j}/{S} end", t0, {f"{m}: {p}": n for (m, p), n in ran.items()})


# ---------------------------------------------------------------------------
# every code: the plan executors
# ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("cfg,j", PLAN_CASES)
def test_plan_executors_every_pattern(oracle_mod, torch_cuda, cfg, j):
    torch = torch_cuda
    c, o = ClayCode(*cfg), oracle_mod.OracleClay(*cfg)
    S = PLAN_SLICES[cfg]
    pats = all_patterns(c)
    chunk = c.sub_chunk_no * SC_PLAN
    host = stripe(cfg, c, SC_PLAN)
    assert host.shape == (c.n, chunk)
    full = torch.from_numpy(host.copy()).cuda()
    flat, outs = guarded(torch, c.n, chunk)
    outs = outs.view(c.n, chunk)
    t0 = time.perf_counter()
    ran = Counter()
    prev = clay_amd.set_exec_mode("grouped")
    try:
        for er in pats[j::S]:
            ref = o.decode_chunks({i: host[i] for i in range(c.n) if i not in er}, er)
            for mode in ("grouped", "tile"):
                clay_amd.set_exec_mode(mode)
                got, path = decode_into(torch, c, full, er, er, flat, outs, chunk)
                ran[mode, path] += 1
                check_outputs(got, ref, er, (cfg, er, mode, path))
                assert path in (("grouped",) if mode == "grouped" else PLAN_PATHS), (cfg, er, mode, path)
        assert np.array_equal(full.cpu().numpy(), host), "a decode wrote to its input"
    finally:
        clay_amd.set_exec_mode(prev)
    report(torch, f"plan {cfg} slice {j}/{S}", t0, {f"{m}: {p}": n for (m, p), n in ran.items()})
    if cfg in TILE_CODES:
        assert ran["tile", "tile"] > 0, (cfg, dict(ran))
