"""The tests' own restatement of the decode dispatch: which streaming kernel an erasure pattern of a
q = 4, t = 4 code ((10,4,13), (9,4,12)) runs on.

The library decides it in clay_amd/csrc/decode_pattern.hpp (choose_decode).  The rule is written out
again here, on purpose without reading it from the library or the header, so that the GPU tests that
assert the path a decode took do not follow the library when it drifts;
tests/test_decode_pattern_cpu.py compares the two line by line, without a GPU.

`c` is any object with k, m, n, q, t and nu (clay_amd.ClayCode, stream_decode_emu.Code); `er` a list
of erased external nodes.  Every other node is taken as present.
"""
import itertools
from types import SimpleNamespace

import numpy as np

F2_ITERS = {False: (6, 4, 2, 1), True: (5, 4, 2, 1)}  # passes a loader wave holds per level (two: a section with two erasures)
MODES = ("auto", "stream", "stream-local", "stream-fused2")


def code(k, m=4):
    """The parameters of (k, 4, k + 3) that the predicates read, without the library."""
    return SimpleNamespace(k=k, m=m, n=k + m, q=4, t=4, nu=16 - k - m)


def internal(c, e):
    return e if e < c.k else e + c.nu


def per_section(c, er):
    per = [0] * c.t
    for e in er:
        per[internal(c, e) // c.q] += 1
    return per


def patterns(c, seed=None, n3=None, n4=None, pred=None):
    """Every pattern of 1 and 2 erasures, then those of 3 and 4 that `pred` accepts: all of them, or
    a seeded sample of n3 / n4."""
    pats = [list(e) for r in (1, 2) for e in itertools.combinations(range(c.n), r)]
    rng = np.random.default_rng(seed)
    for r, cnt in ((3, n3), (4, n4)):
        allp = [list(e) for e in itertools.combinations(range(c.n), r) if pred is None or pred(c, list(e))]
        pats += allp if cnt is None else [allp[i] for i in rng.permutation(len(allp))[:cnt]]
    return pats


def stream_eligible(c, er):
    return len(er) >= 1 and max(per_section(c, er)) <= 1


def local_eligible(c, er):
    """k_stream_local / k_stream_local256: erasures in one y-section plus at most one erasure in one
    other section."""
    busy = [n for n in per_section(c, er) if n]
    return 1 <= len(er) <= c.m and (len(busy) == 1 or (len(busy) == 2 and min(busy) == 1))


def local_path(c, er, mode="stream-local"):
    """The kernel a local-eligible pattern runs on (8-byte rows, sc >= 512): in auto, the (2,1)
    patterns take the fused decode v2 first (every one of them fits it for (10,4,13) and (9,4,12):
    tests/test_decode_pattern_cpu.py)."""
    per = per_section(c, er)
    busy = [n for n in per if n]
    if mode == "auto" and len(er) == 3 and sorted(busy) == [1, 2]:
        return "stream-fused2"
    return "stream-local256" if max(per) == 1 or busy == [2] else "stream-local"


def f2_waves(c, er, two=False):
    """The fused decode's round-capacity check: per section Y with an erasure and iscore level L,
    P(Y, L) = passes of 64 lanes x 8-byte pieces over the layers with z_Y in E_Y and L erased
    sections red; the four loader waves: at least one per section with an erasure, split to minimise
    the sum over levels of the busiest wave's passes (the first such split in lexicographic order);
    a wave holds at most F2_ITERS passes per level, and with two erasures in a section no section
    has a level-4 pass.  The waves per section, or None when the pattern does not fit."""
    key = (c.k, c.nu, tuple(er), two)
    if key not in _waves:
        _waves[key] = _f2_waves(c, er, two)
    return _waves[key]


_waves = {}


def _f2_waves(c, er, two):
    iters = F2_ITERS[two]
    em = [0] * c.t
    for e in er:
        i = internal(c, e)
        em[i // c.q] |= 1 << (i % c.q)
    act = [y for y in range(4) if em[y]]
    count = {(Y, L): 0 for Y in act for L in range(1, 5)}
    for z in range(256):
        red = [y for y in range(4) if (em[y] >> ((z >> (2 * (3 - y))) & 3)) & 1]
        for Y in red:
            count[Y, len(red)] += 1
    P = {k: (n * 8 + 63) // 64 for k, n in count.items()}
    if two and any(P[y, 4] for y in act):
        return None
    best, bcost = None, None
    for n in itertools.product(range(5), repeat=4):  # lexicographic
        if sum(n) != 4 or any((n[y] > 0) != (y in act) for y in range(4)):
            continue
        mx = [max(-(-P[y, L] // n[y]) for y in act) for L in range(1, 5)]
        if any(m > iters[L] for L, m in enumerate(mx)):
            continue
        if bcost is None or sum(mx) < bcost:
            best, bcost = n, sum(mx)
    return best


def f2_fits(c, er, two=False):
    return f2_waves(c, er, two) is not None


def _alive_per_section(c, er):
    alive = [0] * c.t
    for i in range(c.n):
        if i not in er:
            alive[internal(c, i) // c.q] += 1
    return alive


def fused2_eligible(c, er, two=False):
    """k_stream_fused2: 2-4 erasures in distinct y-sections (two=True: at most two per section, one
    section included) whose round targets fit the kernel's item registers, and a ring of 10 - e node
    buffers that holds any two neighbouring sections' surviving real nodes."""
    per = per_section(c, er)
    if not 2 <= len(er) <= c.t or max(per) > (2 if two else 1) or not f2_fits(c, er, two and max(per) == 2):
        return False
    alive = _alive_per_section(c, er)
    rb = 10 - len(er)
    if two:  # neighbouring sections beyond the ring run as split steps
        return max(alive) <= rb
    return all(alive[y] + alive[(y + 1) % c.t] <= rb for y in range(c.t))  # incl. section 3 -> next tile's 0


def stream_path(c, er):
    """The kernel exec mode "stream" runs a pattern on (None: the plan executor)."""
    per = sorted(per_section(c, er), reverse=True)
    if len(er) == 3 and per[:2] == [2, 1] and fused2_eligible(c, er, two=True):
        return "stream-fused2"  # (2,1) sections: the fused decode v2 first
    if local_eligible(c, er):
        return local_path(c, er)
    if fused2_eligible(c, er, two=True):
        return "stream-fused2"
    return None


def expected_kernel(c, er, mode, sc=520, ptrs8=True):
    """The kernel the library names for a decode under exec mode `mode` (ring of 10, CLAY_LOCAL_W64
    unset): None (the plan executor), "local", "local256", "local256-any" or "fused2".  The local
    decode is tried under auto, "stream" and "stream-local", the fused decode v2 under "stream" and
    "stream-fused2" and, from 3 erasures, under auto; where both take a pattern, the fused decode
    has the (2,1) patterns and the local decode the rest.  Sub-chunks from 512 bytes; off 8-byte
    rows (sc % 8, or a chunk pointer off 8-byte alignment) only the 256-byte-run kernel is left, as
    its ANY instantiation."""
    if sc < 512 or sc * 256 >= 1 << 32:
        return None
    rows8 = sc % 8 == 0 and ptrs8
    local = None
    if mode in ("auto", "stream", "stream-local") and local_eligible(c, er):
        local = local_path(c, er)[len("stream-"):]
        if not rows8:
            local = "local256-any" if local == "local256" else None
    fused = (mode in ("stream", "stream-fused2") or (mode == "auto" and len(er) >= 3)) and rows8 and \
        fused2_eligible(c, er, two=True)
    if fused and (local is None or sorted(per_section(c, er))[-2:] == [1, 2] and len(er) == 3):
        return "fused2"
    return local


def used_nodes(c, er):
    """Internal nodes whose RS rows the decode uses: the first k + nu that are not erased."""
    gone = {internal(c, e) for e in er}
    return [i for i in range(c.q * c.t) if i not in gone][:c.k + c.nu]


def phase_a_cases(c, er):
    """Per section, the phase-A copy the kernels dispatch on: x = node (y, x) erased and every other
    node used, 4 = none erased and all used, 5 / 6 = none erased and only node 0 / nodes 0-1 used,
    -1 = anything else."""
    gone = {internal(c, e) for e in er}
    used = set(used_nodes(c, er))
    out = []
    for y in range(c.t):
        sec = range(c.q * y, c.q * y + c.q)
        e = [i for i in sec if i in gone]
        u = [i - c.q * y for i in sec if i in used]
        if len(e) <= 1 and len(u) == c.q - len(e):
            out.append(e[0] - c.q * y if e else 4)
        elif not e and u in ([0], [0, 1]):
            out.append(4 + len(u))
        else:
            out.append(-1)
    return out


def local_sections(c, er):
    """(G, g2) of a local-eligible pattern: the first section with the most erasures, and the section
    of the one erasure outside it (-1: none)."""
    per = per_section(c, er)
    G = per.index(max(per))
    return G, next((y for y in range(c.t) if y != G and per[y]), -1)


def fused2_args(c, er):
    """(lwave, split, npair) of a fused2-eligible pattern: the loader waves' shares packed a byte a
    wave (bits 0-1 the section, 2-3 the part, 4-5 the section's waves - 1, bit 6 set), the sections
    whose loads run as a split step (only with two erasures in a section), the erased rows with an
    erased partner in their section."""
    per = per_section(c, er)
    two = max(per) == 2
    lwave, li = 0, 0
    for y, nw in enumerate(f2_waves(c, er, two)):
        for part in range(nw):
            lwave |= (y | part << 2 | (nw - 1) << 4 | 64) << (8 * li)
            li += 1
    alive = _alive_per_section(c, er)
    rb = 10 - len(er)
    split = sum(1 << y for y in range(1, c.t) if alive[y - 1] + alive[y] > rb) if two else 0
    return lwave, split, 2 * sum(1 for n in per if n == 2)
