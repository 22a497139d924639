"""Flip schedules of the exhaustive scrub tests (test_gpu_scrub_coverage.py, the sweep cases of
test_gpu_scrub_stream.py) and the loop those tests share.  The schedules are plain numpy and are
checked without a GPU in test_scrub_coverage_cpu.py: the GPU cases are parametrized from the lists
below, so a slab, pass or case that is dropped from a schedule fails there.

Every flip XORs one bit, flip_bits(pos, j) = 1 << ((pos + j) % 8), into one stored parity byte;
the expected mask of a flip is computed from the oracle's parity (expected_masks): bit j = the
stored parity chunk j differs from the oracle's parity of the stored data."""
import ctypes as C
import time

import numpy as np

SLAB_BYTES = 256 << 20  # most parity one slab of the batch sweep holds
GUARD = 4  # result words behind the last one a sweep may define, pre-filled with 0xFFFFFFFF

# ---- the bit-sliced kernels: (code, exec mode, path of one stripe) and the two sub-chunk sizes ----
BS_ROWS = [((4, 2, 5), "auto", "bs-scrub1"), ((4, 2, 5), "grouped", "bs-scrub"), ((6, 3, 8), "auto", "bs-scrub"),
           ((8, 4, 11), "auto", "bs-scrub"), ((9, 3, 11), "auto", "bs-scrub"), ((10, 4, 13), "auto", "bs-scrub")]
# (id, sc - W, shift): W + 40 on 8-byte rows: a full tile, then a whole 32-byte unit and a unit of
# one 8-byte piece; W + 37 shifted by 3 bytes: the byte-tail instantiation, its last unit 5 bytes
BS_SIZES = [("w40", 40, 0), ("w37s3", 37, 3)]
ONE_SC = 40  # the one-stripe loop: a partial tile only
VERIFY_CFG, VERIFY_SC = (9, 3, 11), 37  # clay_verify: an odd chunk, every staged row padded


def flip_bits(pos, j):
    return (1 << ((np.asarray(pos) + np.asarray(j)) % 8)).astype(np.uint8)


def expected_masks(ref, jj, pos, bits):
    """ref: the oracle's parity (m, chunk) of the stored data.  Mask of a stripe whose stored
    parity is ref with byte pos[i] of chunk jj[i] XORed with bits[i], for every i."""
    stored = ref[jj, pos] ^ bits
    return (stored != ref[jj, pos]).astype(np.uint32) << jj.astype(np.uint32)


def slabs(m, chunk):
    """The batch sweep's slabs [(p0, ns)]: stripe s of a slab is byte position p0 + s of the
    chunk; ns follows from the cap on a slab's parity."""
    cap = max(1, SLAB_BYTES // (m * chunk))
    return [(p0, min(cap, chunk - p0)) for p0 in range(0, chunk, cap)]


def batch_pass(m, p0, ns, r):
    """Pass r of a slab: stripe s has byte p0 + s of parity chunk (s + r) % m flipped: (j, pos)."""
    s = np.arange(ns, dtype=np.int64)
    return (s + r) % m, p0 + s


def all_flips(m, chunk):
    """The one-stripe and clay_verify loops: every (j, pos), chunk by chunk."""
    return np.repeat(np.arange(m, dtype=np.int64), chunk), np.tile(np.arange(chunk, dtype=np.int64), m)


# ---- the streaming scrub of (10,4,13): a lane group is column c = z / 4 of group G = z % 4 ----
STREAM_M, STREAM_ALPHA = 4, 256
STREAM_FULL = {16: 1, 24: 1, 264: 4}  # sc -> cases per parity chunk (layers z % parts == q)
STREAM_MID = (1064, 2288)
STREAM_BIG = (66176, 66184)
COLS = (0, 7, 8, 63)  # first / last lane group of a wave, first / last wave
ROW_LAYERS = tuple(4 * c + g for i, c in enumerate(COLS) for g in (i % 4, (i + 2) % 4))
BIG_LAYERS = tuple(4 * c + g for g, c in enumerate(COLS))


def stream_cases():
    """(sc, kind, j, q); j = None: every parity chunk in one case."""
    out = [(sc, "full", j, q) for sc, parts in STREAM_FULL.items() for j in range(STREAM_M) for q in range(parts)]
    out += [(sc, kind, j, 0) for sc in STREAM_MID for kind in ("rows", "edges") for j in range(STREAM_M)]
    out += [(sc, "tile-edges", None, 0) for sc in STREAM_BIG]
    return out


def case_id(case):
    sc, kind, j, q = case
    return f"{sc}-{kind}" + ("" if j is None else f"-j{j}") + (f"-q{q}" if kind == "full" and STREAM_FULL[sc] > 1 else "")


def edge_bytes(tiles, ragged16):
    """First and last byte of every tile (xcd, slot, round, b0, vend); ragged16: also the last byte
    before and the first after every 16-byte boundary inside a tile whose width is no multiple of 16."""
    xs = set()
    for _, _, _, b0, vend in tiles:
        xs |= {b0, vend - 1}
        if ragged16 and (vend - b0) % 16:
            for b in range(b0 + 16, vend, 16):
                xs |= {b - 1, b}
    return sorted(xs)


def stream_flips(case, tiles):
    """(j, chunk offset) of every flip of a case; tiles: the size's tile dump."""
    sc, kind, j, q = case
    if kind == "full":
        zs, xs = [z for z in range(STREAM_ALPHA) if z % STREAM_FULL[sc] == q], range(sc)
    elif kind == "rows":
        zs, xs = ROW_LAYERS, range(sc)
    elif kind == "edges":
        zs, xs = range(STREAM_ALPHA), edge_bytes(tiles, True)
    else:
        zs, xs = BIG_LAYERS, edge_bytes(tiles, False)
    at = (np.asarray(zs, dtype=np.int64)[:, None] * sc + np.asarray(xs, dtype=np.int64)[None, :]).reshape(-1)
    js = range(STREAM_M) if j is None else [j]
    return np.repeat(np.asarray(js, dtype=np.int64), at.size), np.tile(at, len(js))


def first_wrong(got, want, jj, pos, sc):
    """None, or the first wrong flip as (j, layer, byte in sub-chunk, got, want)."""
    bad = np.flatnonzero(got != want)
    if bad.size == 0:
        return None
    i = int(bad[0])
    return int(jj[i]), int(pos[i]) // sc, int(pos[i]) % sc, int(got[i]), int(want[i]), f"{bad.size} of {got.size} wrong"


def run_flip_loop(torch, clay_amd, st, jj, pos, ref, path, what):
    """The one-stripe loop on stripe 0 of `st` (test_gpu_scrub.Stripes, a clean codeword): flip
    byte pos[i] of parity chunk jj[i] on the device, clay_scrub_device into result word i, un-flip;
    no synchronisation inside the loop.  Then one synchronise, the whole vector against the
    expected masks, the guard words, the inputs against the upload, path and launch count."""
    from clay_amd import _lib
    c, sc = st.c, st.chunk // st.c.sub_chunk_no
    n = len(jj)
    bits = flip_bits(pos, jj)
    want = expected_masks(ref, jj, pos, bits)
    assert np.array_equal(want, np.uint32(1) << jj.astype(np.uint32))  # the data are the codeword's
    res = torch.full((n + GUARD,), -1, dtype=torch.int32, device="cuda")
    d, p = st.ptrs(0)
    dp, pp = (C.c_void_p * c.k)(*d), (C.c_void_p * c.m)(*p)
    code, err, call = C.byref(c.struct), _lib.ClayErrorStruct(), _lib.lib().clay_scrub_device
    par, r0 = st.dev[1], res.data_ptr()
    at = (np.asarray([st.off(0, c.k + j)[1] for j in range(c.m)], dtype=np.int64)[jj] + pos).tolist()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i, (a, b) in enumerate(zip(at, bits.tolist())):
        cell = par[a:a + 1]
        cell.bitwise_xor_(b)
        rc = call(code, dp, pp, st.chunk, r0 + 4 * i, 0, None, C.byref(err))
        assert rc == 0, (rc, err.msg)
        cell.bitwise_xor_(b)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print(f"{what}: {n} calls, {dt:.2f} s, {1e6 * dt / max(1, n):.1f} us per call")
    assert clay_amd.last_exec_path() == path and clay_amd.last_launch_count() == 1
    got = res.cpu().numpy().view(np.uint32)
    assert np.all(got[n:] == 0xFFFFFFFF), "result words past the last call written"
    assert first_wrong(got[:n], want, jj, pos, sc) is None, first_wrong(got[:n], want, jj, pos, sc)
    for fam in (0, 1):  # every flip undone, nothing written, gaps included
        assert np.array_equal(st.dev[fam].cpu().numpy(), st.host[fam]), "inputs differ from the upload"
    return dt
