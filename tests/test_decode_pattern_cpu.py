"""The library's decode dispatch (choose_decode, clay_amd/csrc/decode_pattern.hpp) against the tests'
restatement (tests/decode_pattern.py): no GPU.

tests/host/decode_pattern_check.cpp prints, for (10,4,13) and (9,4,12), the kernel the header names
for every erasure set of 1-4 nodes (1,470 + 1,092 patterns, every other node alive) under the exec
modes auto, stream, stream-local and stream-fused2, on 8-byte rows (sc 512 and 520) and off them
(sc 516; sc 512 at misaligned chunk pointers), with the arguments the pattern decides (G, g2, the
phase-A cases, the loader-wave plan, the split steps, the pair count), and a few declines; every
line is compared with this side's rule.  The GPU tests that assert the path of a decode from
tests/decode_pattern.py therefore assert what the library's dispatch names.  The pinned counts were
computed from the restatements the GPU tests carried before they moved to tests/decode_pattern.py.
"""
import itertools
import subprocess
from collections import Counter

import pytest

import decode_pattern as dp
import stream_cut as cut

CODES = {10: dp.code(10), 9: dp.code(9)}
ROWS = [(512, 1), (520, 1), (516, 1), (512, 0)]  # (sc, chunk pointers 8-byte aligned)
DECLINES = [(10, [0], 504, 10, -1), (10, [0, 4, 8, 12], 504, 10, -1), (9, [0, 4], 504, 10, -1),
            (10, [0], 520, 4, -1), (10, [0, 4, 8, 12], 520, 4, -1), (9, [0, 1, 4], 520, 4, -1),
            (10, [0, 4, 8, 12], 520, 10, 5)]  # (k, erased, sc, ring, a node without data)


def all_patterns(c):
    return [list(e) for r in range(1, c.m + 1) for e in itertools.combinations(range(c.n), r)]


@pytest.fixture(scope="module")
def printed(tmp_path_factory):
    exe = cut.build_host(tmp_path_factory.mktemp("decode_pattern"), "decode_pattern_check")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    *lines, last = r.stdout.strip().split("\n")
    assert last == f"decode pattern ok: {len(lines)} cases", last
    return lines


@pytest.fixture(scope="module")
def named(printed):
    """(k, pattern, mode, sc, ptrs8) -> the kernel the header names."""
    out = {}
    for line in printed:
        if not line.startswith("decline"):
            k, er, mode, sc, p8, kernel = line.split()[:6]
            out[int(k), tuple(map(int, er.split(","))), mode, int(sc), int(p8)] = kernel
    return out


def restated_line(k, c, er, mode, sc, p8):
    kernel = dp.expected_kernel(c, er, mode, sc, bool(p8))
    line = f"{k} {','.join(map(str, er))} {mode} {sc} {p8} {kernel or 'none'}"
    if kernel == "fused2":
        line += " " + " ".join(map(str, dp.phase_a_cases(c, er) + list(dp.fused2_args(c, er))))
    elif kernel:
        line += " " + " ".join(map(str, list(dp.local_sections(c, er)) + dp.phase_a_cases(c, er)))
    return line


def test_header_dispatch_is_the_restated_dispatch(printed):
    want = [restated_line(k, c, er, mode, sc, p8)
            for k, c in CODES.items() for er in all_patterns(c) for sc, p8 in ROWS for mode in dp.MODES]
    assert len(want) == (1470 + 1092) * len(ROWS) * len(dp.MODES)
    for k, er, sc, ring, dead in DECLINES:
        c = CODES[k]
        alive = sum(1 << dp.internal(c, i) for i in range(c.n) if i not in er and i != dead)
        want += [f"decline {k} {','.join(map(str, er))} {mode} {sc} 1 {ring} {alive:x} none" for mode in dp.MODES]
    assert len(printed) == len(want)
    diff = [(g, w) for g, w in zip(printed, want) if g != w]
    assert not diff, f"{len(diff)} lines differ, the first (header, restatement): {diff[0]}"


def test_declines_are_declines():
    """What the restatement says of the declines' sizes (a ring of 4 and a node without data are
    outside what it models: the library's validation admits neither)."""
    for k, er, sc, ring, dead in DECLINES:
        if sc < 512:
            assert all(dp.expected_kernel(CODES[k], er, mode, sc) is None for mode in dp.MODES)


@pytest.mark.parametrize("k, counts", [(10, {"local256": 105, "local": 135, "fused2": 1230, "none": 0}),
                                       (9, {"local256": 91, "local": 123, "fused2": 878, "none": 0})])
def test_kernel_counts_under_stream(named, k, counts):
    c = CODES[k]
    for sc in (512, 520):
        got = Counter(named[k, tuple(er), "stream", sc, 1] for er in all_patterns(c))
        assert {name: got[name] for name in counts} == counts and sum(got.values()) == sum(counts.values()), (sc, got)
        for er in all_patterns(c):
            assert named[k, tuple(er), "auto", sc, 1] == named[k, tuple(er), "stream", sc, 1], er
            path = dp.stream_path(c, er)  # what the GPU tests assert under "stream"
            assert path and path[len("stream-"):] == named[k, tuple(er), "stream", sc, 1], er
            if dp.local_eligible(c, er):  # and under auto / "stream-local"
                assert dp.local_path(c, er, "auto")[len("stream-"):] == named[k, tuple(er), "auto", sc, 1], er
                assert dp.local_path(c, er)[len("stream-"):] == named[k, tuple(er), "stream-local", sc, 1], er


@pytest.mark.parametrize("k, one, two", [(10, 360, 1321), (9, 236, 956)])
def test_fused2_eligible_counts(named, k, one, two):
    c = CODES[k]
    pats = all_patterns(c)
    assert sum(dp.fused2_eligible(c, er) for er in pats) == one
    assert sum(dp.fused2_eligible(c, er, two=True) for er in pats) == two
    assert sum(named[k, tuple(er), "stream-fused2", 520, 1] == "fused2" for er in pats) == two
    # one erasure per section: the same patterns as among those with up to two
    assert all(dp.fused2_eligible(c, er, two=True) for er in pats if dp.fused2_eligible(c, er))


@pytest.mark.parametrize("k, n", [(10, 192), (9, 162)])
def test_every_2_1_pattern_fits_the_fused_decode(named, k, n):
    """The claim of decode_pattern.local_path's docstring."""
    c = CODES[k]
    pats = [er for er in all_patterns(c) if len(er) == 3 and sorted(dp.per_section(c, er))[-2:] == [1, 2]]
    assert len(pats) == n
    assert sum(dp.fused2_eligible(c, er, two=True) for er in pats) == n
    assert all(named[k, tuple(er), "auto", 520, 1] == "fused2" for er in pats)
    assert all(named[k, tuple(er), "stream-local", 520, 1] == "local" for er in pats)


def test_further_pins(named):
    for (k, er, mode, sc, p8), kernel in named.items():
        if sc % 8 or not p8:  # off 8-byte rows only the ANY instantiation of the 256-byte-run kernel is left
            assert kernel in ("local256-any", "none"), (k, er, mode, sc, p8, kernel)
            on = named[k, er, mode, 512, 1]
            assert kernel == ("local256-any" if on == "local256" else "none"), (k, er, mode, sc, p8, kernel, on)
        else:
            assert kernel != "local256-any", (k, er, mode, sc, kernel)
        if mode == "stream-local":
            assert kernel != "fused2", (k, er, sc, p8)
        if mode == "stream-fused2":
            assert kernel in ("fused2", "none") and (len(er) > 1 or kernel == "none"), (k, er, sc, p8, kernel)
