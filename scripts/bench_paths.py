#!/usr/bin/env python3
"""Device-resident timing of every SURVEY.md §8 configuration on one GPU (inputs resident in
HBM, HIP events on the launch stream, median of N runs).  Algorithmic bytes per SURVEY §8(d):
encode  read k*chunk + write m*chunk
decode  read (n-e)*chunk + write (#erased data nodes)*chunk
repair  read d*beta*sc + write chunk
scrub   read n*chunk (ONLY=scrub; scrub10: the (10,4,13) 1 GiB leg alone; scrub_gate: the sweep behind
        auto's gate for the streaming scrub)
ONLY=batch_stream: many (10,4,13) stripes above 4 MiB per call, the streaming batch against a
per-stripe loop; batch_stream_gate: the sweep behind auto's upper gate for it.
ONLY=scrub_batch_stream: many (10,4,13) stripes scrubbed in one launch of the streaming batch, the
path without it and the batched encode alternated; scrub_batch_gate: the sweep behind auto's gate.
ONLY=batch_decode_fused2 / batch_decode_fused2_gate: the same with three and four lost nodes, one
launch of the fused decode v2's batch against the per-stripe loop, and the sweep behind auto's gate.
ONLY=batch_decode_stream: many (10,4,13) stripes with the same lost nodes decoded in one launch of
the local decode's batch variant against the per-stripe loop; batch_decode_stream_gate: the sweep
behind auto's gate for it.
Prints one JSON object per configuration."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import clay_amd  # noqa: E402
from clay_amd import ClayCode  # noqa: E402

RUNS = int(os.environ.get("RUNS", "10"))
EXEC = os.environ.get("CLAY_EXEC", "auto")  # exec mode: auto | grouped | tile | stream | stream-local | stream-fused2
clay_amd.set_exec_mode(EXEC)
stream = torch.cuda.current_stream()


B2B = int(os.environ.get("B2B", "8"))  # back-to-back calls per timed sample


def timed(fn):
    """Median / min per-call time of B2B back-to-back calls between two events: the host work of
    call i+1 (argument marshalling, validation, launch) overlaps the kernel of call i, so the
    sample is device time, not Python overhead (one call on an idle GPU would time both)."""
    ts = []
    for i in range(RUNS + 2):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        fn()  # queue one call ahead so e0 is recorded behind work, not on an idle GPU
        e0.record(stream)
        for _ in range(B2B):
            fn()
        e1.record(stream)
        torch.cuda.synchronize()
        if i >= 2:
            ts.append(e0.elapsed_time(e1) / B2B)
    return float(np.median(ts)), float(np.min(ts))


def report(name, ms, mn, algo, extra=None):
    d = {"config": name, "median_ms": round(ms, 4), "min_ms": round(mn, 4),
         "algorithmic_bytes": int(algo), "GBps": round(algo / (ms * 1e-3) / 1e9, 1),
         "frac_of_8TBps": round(algo / (ms * 1e-3) / 8e12, 4), "path": (clay_amd.last_encode_path() if name.startswith("encode")
                  else clay_amd.last_exec_path()),
         "launches": clay_amd.last_launch_count()}
    if extra:
        d.update(extra)
    print(json.dumps(d), flush=True)


def rnd(n, chunk, seed):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    return torch.randint(0, 256, (n, chunk), dtype=torch.uint8, device="cuda", generator=g)


def encode_cfg(k, m, d, stripe, path=None):
    if path:
        clay_amd.set_encode_path(path, 0)
    try:
        _encode_cfg(k, m, d, stripe)
    finally:
        if path:
            clay_amd.set_encode_path("auto", 0)


def _encode_cfg(k, m, d, stripe):
    c = ClayCode(k, m, d)
    chunk = c.encoded_chunk_size(stripe)
    data, par = rnd(k, chunk, 1), torch.empty((m, chunk), dtype=torch.uint8, device="cuda")
    ms, mn = timed(lambda: c.encode_device([data[i] for i in range(k)], [par[i] for i in range(m)], chunk, 0,
                                           stream.cuda_stream))
    report(f"encode ({k},{m},{d}) {stripe >> 20} MiB", ms, mn, (k + m) * chunk)


def encode_batch_cfg(k, m, d, stripe, n):
    """clay_bench.rs shape (1 MiB stripes) as one device batch call: n stripes per call."""
    c = ClayCode(k, m, d)
    chunk = c.encoded_chunk_size(stripe)
    data, par = rnd(n * k, chunk, 5), torch.empty((n * m, chunk), dtype=torch.uint8, device="cuda")
    dl, pl = [data[i] for i in range(n * k)], [par[i] for i in range(n * m)]
    ms, mn = timed(lambda: c.encode_device_batch(dl, pl, n, chunk, 0, stream.cuda_stream))
    report(f"encode ({k},{m},{d}) batch {n} x {stripe >> 10} KiB", ms, mn, n * (k + m) * chunk,
           {"input_GiBps": round(n * k * chunk / (ms * 1e-3) / 2**30, 1)})


def decode_cfg(k, m, d, stripe, er, mode=None, codeword=False):
    prev = clay_amd.set_exec_mode(mode) if mode else None
    try:
        _decode_cfg(k, m, d, stripe, er, codeword)
    finally:
        if prev:
            clay_amd.set_exec_mode(prev)


def _decode_cfg(k, m, d, stripe, er, codeword=False):
    c = ClayCode(k, m, d)
    chunk = c.encoded_chunk_size(stripe)
    full = rnd(c.n, chunk, 2)
    outs = torch.empty((c.n, chunk), dtype=torch.uint8, device="cuda")
    ins = [None if i in er else full[i] for i in range(c.n)]
    ous = [outs[i] if i in er else None for i in range(c.n)]
    ms, mn = timed(lambda: c.decode_device(ins, er, ous, chunk, 0, stream.cuda_stream, codeword=codeword))
    ndata = sum(1 for e in er if e < k)
    name = f"decode ({k},{m},{d}) {stripe >> 20} MiB erasures {er}"
    if codeword and clay_amd.last_exec_path() == "bs-repair-stream":
        # the repair route reads the beta = alpha / q layers of every other chunk and writes the
        # erased chunk: charged the bytes it moves (a decode's full-read bytes would put frac > 1)
        beta_bytes = chunk // c.q
        report(name + " codeword", ms, mn, (c.n - 1) * beta_bytes + chunk,
               {"bytes_counted": "repair route: (n-1) x chunk/q read + the erased chunk written"})
    else:
        report(name + (" codeword" if codeword else ""), ms, mn, (c.n - len(er)) * chunk + ndata * chunk,
               {"writes_counted": "erased data nodes only"})


def timed_alternating(fns):
    """timed() for several variants with their samples interleaved (A B A B ...), so clock and
    box drift hit all of them alike.  fns: callables; returns [(median, min)] in their order."""
    ts = [[] for _ in fns]
    for i in range(RUNS + 2):
        for j, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            fn()
            e0.record(stream)
            for _ in range(B2B):
                fn()
            e1.record(stream)
            torch.cuda.synchronize()
            if i >= 2:
                ts[j].append(e0.elapsed_time(e1) / B2B)
    return [(float(np.median(t)), float(np.min(t))) for t in ts]


def decode_batch_cfg(k, m, d, stripe, n, e, loop_stripes):
    """clay_bench.rs stripe sizes, one lost node in every stripe, about 64 MiB of input per call:
    clay_decode_device_strided under auto (the line batch for (4,2,5)) and under "grouped" (the
    staged batch), samples alternated; then the only way without a batch entry point, a loop of
    per-stripe clay_decode_device calls on the same buffers (the first loop_stripes stripes,
    reported per stripe; host and launch overhead included: that is what the caller pays).
    Bytes: what the algorithm moves per stripe -- the line kernel reads 4.5 chunks (half of the
    ignored node) and writes 1, not 5 + 1."""
    c = ClayCode(k, m, d)
    chunk = c.encoded_chunk_size(stripe)
    full = rnd(n * c.n, chunk, 6).view(n, c.n, chunk)
    outs = torch.empty((n, c.n, chunk), dtype=torch.uint8, device="cuda")
    algo = int(n * 5.5 * chunk)
    name = f"decode ({k},{m},{d}) batch {n} x {stripe >> 10} KiB erasure [{e}]"

    def call(mode):
        def fn():
            clay_amd.set_exec_mode(mode)
            c.decode_device_strided(full, [e], outs, n, chunk, 0, 0, 0, 0, 0, stream.cuda_stream)
        return fn

    prev = clay_amd.set_exec_mode("auto")
    try:
        modes = ("auto", "grouped")
        res = timed_alternating([call(mo) for mo in modes])
        for mo, (ms, mn) in zip(modes, res):
            call(mo)()
            torch.cuda.synchronize()
            report(f"{name} {mo}", ms, mn, algo,
                   {"bytes_counted": "per stripe 4.5 chunks read + 1 written", "per_stripe_us": round(ms * 1e3 / n, 6),
                    "stripe_data_GiBps": round(n * k * chunk / (ms * 1e-3) / 2**30, 1)})
        clay_amd.set_exec_mode("auto")
        nl = min(n, loop_stripes)
        ins = [[None if i == e else full[s, i] for i in range(c.n)] for s in range(nl)]
        ous = [[outs[s, i] if i == e else None for i in range(c.n)] for s in range(nl)]

        def loop():
            for s in range(nl):
                c.decode_device(ins[s], [e], ous[s], chunk, 0, stream.cuda_stream)

        ts = []
        for i in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            loop()
            e1.record(stream)
            torch.cuda.synchronize()
            if i >= 1:
                ts.append(e0.elapsed_time(e1))
        ms, mn = float(np.median(ts)), float(np.min(ts))
        report(f"{name} per-stripe loop of {nl}", ms, mn, int(nl * 5.5 * chunk),
               {"bytes_counted": "per stripe 4.5 chunks read + 1 written", "per_stripe_us": round(ms * 1e3 / nl, 4),
                "stripe_data_GiBps": round(nl * k * chunk / (ms * 1e-3) / 2**30, 1)})
    finally:
        clay_amd.set_exec_mode(prev)


def repair_batch_cfg(k, m, d, sc, n, lost, loop_stripes, full):
    """One lost node in every stripe, n stripes of sub-chunk size sc per call (about 64 MiB of
    chunks): clay_repair_device_strided under auto (the repair batch where the code has a
    k_bs_repair instantiation) and under "grouped" (the staged batch), samples alternated; then the
    only way without a batch entry point, a loop of per-stripe clay_repair_device(_full_chunks)
    calls on the same buffers (the first loop_stripes stripes, reported per stripe; host and launch
    overhead included: that is what the caller pays).  full: whole helper chunks, else the
    gathered beta repair sub-chunks.  Bytes: (n - 1) x beta x sc read + the chunk written."""
    c = ClayCode(k, m, d)
    chunk = c.sub_chunk_no * sc
    helpers = [h for h, _ in c.minimum_to_repair(lost, [i for i in range(c.n) if i != lost])]
    hb = chunk if full else c.beta * sc
    bufs = rnd(n * c.n, hb, 7).view(n, c.n, hb)
    outs = torch.empty((n, chunk), dtype=torch.uint8, device="cuda")
    per = len(helpers) * c.beta * sc + chunk
    lay = "full chunks" if full else "gathered"
    name = f"repair ({k},{m},{d}) batch {n} x sc {sc} ({c.k * chunk >> 10} KiB stripes) node {lost} {lay}"
    extra = {"bytes_counted": "per stripe (n-1) x beta x sc read + 1 chunk written",
             "lane_order": {"0": "part-fastest", "1": "j-fastest"}.get(os.environ.get("CLAY_REPAIR_BATCH_JFAST", ""), "default")}

    def call(mode):
        def fn():
            clay_amd.set_exec_mode(mode)
            c.repair_device_strided(lost, helpers, bufs, outs, n, chunk, full, 0, 0, 0, 0, stream.cuda_stream)
        return fn

    prev = clay_amd.set_exec_mode("auto")
    try:
        modes = ("auto", "grouped")
        res = timed_alternating([call(mo) for mo in modes])
        for mo, (ms, mn) in zip(modes, res):
            call(mo)()
            torch.cuda.synchronize()
            report(f"{name} {mo}", ms, mn, n * per, dict(extra, per_stripe_us=round(ms * 1e3 / n, 6)))
        clay_amd.set_exec_mode("auto")
        nl = min(n, loop_stripes)
        ins = [[bufs[s, h] for h in helpers] for s in range(nl)]
        fn1 = c.repair_device_full_chunks if full else c.repair_device

        def loop():
            for s in range(nl):
                fn1(lost, helpers, ins[s], chunk, outs[s], 0, stream.cuda_stream)

        ts = []
        for i in range(6):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            loop()
            e1.record(stream)
            torch.cuda.synchronize()
            if i >= 1:
                ts.append(e0.elapsed_time(e1))
        ms, mn = float(np.median(ts)), float(np.min(ts))
        report(f"{name} per-stripe loop of {nl}", ms, mn, nl * per,
               dict(extra, per_stripe_us=round(ms * 1e3 / nl, 4), per_stripe_us_min=round(mn * 1e3 / nl, 4),
                    per_stripe_us_max=round(float(np.max(ts)) * 1e3 / nl, 4)))
    finally:
        clay_amd.set_exec_mode(prev)


def _encode_and_compare(c, data, par, scratch, flags, chunk):
    """The only way to scrub without clay_scrub_device: encode into m scratch chunks, then compare
    them with the stored parity (one device-side reduction per chunk into `flags`; torch.equal
    would add a host synchronize per chunk)."""
    c.encode_device(data, scratch, chunk, 0, stream.cuda_stream)
    for j in range(c.m):
        torch.any(scratch[j] != par[j], out=flags[j])


def scrub_cfg(k, m, d, stripe, modes):
    """One stripe: the scrub under each exec mode of `modes` ("auto": the line kernel for (4,2,5),
    the streaming kernel for (10,4,13) above its gate, v1 elsewhere; "stream": the streaming kernel
    for (10,4,13); "grouped": v1), the encode into scratch plus a device compare, and the encode
    alone, samples alternated.  Bytes: the scrub reads n chunks; the encode reads k and writes m;
    encode + compare moves k read + m written + 2m read."""
    c = ClayCode(k, m, d)
    chunk = c.encoded_chunk_size(stripe)
    data, par = rnd(k, chunk, 11), torch.empty((m, chunk), dtype=torch.uint8, device="cuda")
    dl, pl = [data[i] for i in range(k)], [par[i] for i in range(m)]
    c.encode_device(dl, pl, chunk, 0, stream.cuda_stream)  # a codeword: the scrub's common case
    scratch = torch.empty((m, chunk), dtype=torch.uint8, device="cuda")
    sl = [scratch[i] for i in range(m)]
    res = torch.empty(1, dtype=torch.int32, device="cuda")
    flags = torch.empty(m, dtype=torch.bool, device="cuda")

    def scrub(mode):
        def fn():
            clay_amd.set_exec_mode(mode)
            c.scrub_device(dl, pl, res, chunk, 0, stream.cuda_stream)
        return fn

    prev = clay_amd.set_exec_mode("auto")
    try:
        fns = [scrub(mo) for mo in modes] + [lambda: _encode_and_compare(c, dl, pl, sl, flags, chunk),
                                             lambda: c.encode_device(dl, sl, chunk, 0, stream.cuda_stream)]
        out = timed_alternating(fns)
        name = f"({k},{m},{d}) {stripe >> 20} MiB"
        for mo, fn, (ms, mn) in zip(modes, fns, out):
            fn()
            torch.cuda.synchronize()
            assert int(res.item()) == 0
            report(f"scrub {name} {mo}", ms, mn, c.n * chunk, {"bytes_counted": "n chunks read"})
        ms, mn = out[len(modes)]
        assert not bool(flags.any().item())
        report(f"scrub {name} by encode_device + compare", ms, mn, (k + 3 * m) * chunk,
               {"bytes_counted": "k read + m written + 2m read", "path": clay_amd.last_encode_path(),
                "scratch_bytes": m * chunk})
        ms, mn = out[len(modes) + 1]
        report(f"scrub {name} encode_device alone", ms, mn, c.n * chunk,
               {"bytes_counted": "k read + m written", "path": clay_amd.last_encode_path()})
    finally:
        clay_amd.set_exec_mode(prev)


def scrub_gate_cfg(sizes=(2048, 8192, 16384, 32768, 65536, 131072, 419432), samples=5):
    """ONLY=scrub_gate: where does the streaming scrub of (10,4,13) overtake v1?  For every
    sub-chunk size, one stripe with a codeword in the buffers scrubbed under "stream"
    (stream-scrub) and under "grouped" (bs-scrub), `samples` samples each of B2B back-to-back
    calls, alternated.  A win: the streaming median is below v1's by more than the spread
    (max - min) of the v1 samples of the same call.  Auto's gate (engine.hip kScrubStreamMinSc) is
    the smallest size from which it wins at that size and every larger one."""
    global RUNS
    c = ClayCode(10, 4, 13)
    keep, RUNS = RUNS, samples
    prev = clay_amd.set_exec_mode("auto")
    try:
        for sc in sizes:
            chunk = c.sub_chunk_no * sc
            data, par = rnd(10, chunk, 13), torch.empty((4, chunk), dtype=torch.uint8, device="cuda")
            dl, pl = [data[i] for i in range(10)], [par[i] for i in range(4)]
            c.encode_device(dl, pl, chunk, 0, stream.cuda_stream)
            res = torch.empty(1, dtype=torch.int32, device="cuda")
            paths, ts = [], [[], []]

            def scrub(mode):
                def fn():
                    clay_amd.set_exec_mode(mode)
                    c.scrub_device(dl, pl, res, chunk, 0, stream.cuda_stream)
                return fn

            fns = [scrub("stream"), scrub("grouped")]
            for j, fn in enumerate(fns):
                res.fill_(-1)
                fn()
                torch.cuda.synchronize()
                assert int(res.item()) == 0
                paths.append(clay_amd.last_exec_path())
            for i in range(RUNS + 2):
                for j, fn in enumerate(fns):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    fn()
                    e0.record(stream)
                    for _ in range(B2B):
                        fn()
                    e1.record(stream)
                    torch.cuda.synchronize()
                    if i >= 2:
                        ts[j].append(e0.elapsed_time(e1) / B2B)
            s_med, v_med = float(np.median(ts[0])), float(np.median(ts[1]))
            v_spread = float(np.max(ts[1]) - np.min(ts[1]))
            print(json.dumps({"config": f"scrub gate (10,4,13) sc {sc}", "paths": paths,
                              "stream_us": [round(t * 1e3, 2) for t in ts[0]],
                              "v1_us": [round(t * 1e3, 2) for t in ts[1]],
                              "stream_median_us": round(s_med * 1e3, 2), "v1_median_us": round(v_med * 1e3, 2),
                              "v1_spread_us": round(v_spread * 1e3, 2),
                              "stream_wins": bool(v_med - s_med > v_spread)}), flush=True)
    finally:
        RUNS = keep
        clay_amd.set_exec_mode(prev)


def scrub_batch_cfg(k, m, d, stripe, n, loop_stripes):
    """n stripes of `stripe` bytes of data per call (about 64 MiB): clay_scrub_device_strided in one
    launch against a per-stripe loop of encode_device + compare on the same buffers (the first
    loop_stripes stripes, reported per stripe; host and launch overhead included: that is what the
    caller pays)."""
    c = ClayCode(k, m, d)
    chunk = c.encoded_chunk_size(stripe)
    data = rnd(n * k, chunk, 12).view(n, k, chunk)
    par = torch.empty((n, m, chunk), dtype=torch.uint8, device="cuda")
    c.encode_device_strided(data, par, n, chunk, 0, 0, 0, 0, 0, stream.cuda_stream)
    res = torch.empty(n, dtype=torch.int32, device="cuda")
    name = f"scrub ({k},{m},{d}) batch {n} x {stripe >> 10} KiB"
    ms, mn = timed(lambda: c.scrub_device_strided(data, par, res, n, chunk, 0, 0, 0, 0, 0, stream.cuda_stream))
    torch.cuda.synchronize()
    assert not bool(res.any().item())
    report(f"{name} one launch", ms, mn, n * c.n * chunk,
           {"bytes_counted": "n chunks read", "per_stripe_us": round(ms * 1e3 / n, 6),
            "stripe_data_GiBps": round(n * k * chunk / (ms * 1e-3) / 2**30, 1)})
    nl = min(n, loop_stripes)
    scratch = torch.empty((m, chunk), dtype=torch.uint8, device="cuda")
    sl = [scratch[j] for j in range(m)]
    flags = torch.empty((nl, m), dtype=torch.bool, device="cuda")
    dls = [[data[s, i] for i in range(k)] for s in range(nl)]
    pls = [[par[s, j] for j in range(m)] for s in range(nl)]

    def loop():
        for s in range(nl):
            _encode_and_compare(c, dls[s], pls[s], sl, flags[s], chunk)

    ts = []
    for i in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        loop()
        e1.record(stream)
        torch.cuda.synchronize()
        if i >= 1:
            ts.append(e0.elapsed_time(e1))
    ms, mn = float(np.median(ts)), float(np.min(ts))
    assert not bool(flags.any().item())
    report(f"{name} per-stripe loop of {nl}: encode_device + compare", ms, mn, nl * (k + 3 * m) * chunk,
           {"bytes_counted": "k read + m written + 2m read", "per_stripe_us": round(ms * 1e3 / nl, 4),
            "path": clay_amd.last_encode_path(),
            "stripe_data_GiBps": round(nl * k * chunk / (ms * 1e-3) / 2**30, 1)})


def batch_stream_cfg(sc, n, k=10, m=4, d=13, gate=False):
    """ONLY=batch_stream: n stripes of (10,4,13) above the staged batch's 4 MiB (sub-chunk sc, about
    1 GiB of data per call) through clay_encode_device_strided under auto -- one launch of the
    batched streaming kernel ("stream-batch-..."; a library without it runs its own loop of one
    launch per stripe inside the call) -- and through a loop of per-stripe clay_encode_device calls
    on the same buffers, samples alternated.  Per variant: median / min / spread (max - min) of the
    samples per call of n stripes, and GiB/s of stripe data."""
    c = ClayCode(k, m, d)
    chunk = c.sub_chunk_no * sc
    data = rnd(n * k, chunk, 21).view(n, k, chunk)
    par = torch.empty((n, m, chunk), dtype=torch.uint8, device="cuda")
    dls = [[data[s, i] for i in range(k)] for s in range(n)]
    pls = [[par[s, j] for j in range(m)] for s in range(n)]

    def batch():
        # ONLY=batch_stream_gate: under "stream", which takes the batch at any eligible size,
        # whatever auto's gate says
        if gate:
            clay_amd.set_encode_path("stream", 0)
        c.encode_device_strided(data, par, n, chunk, 0, 0, 0, 0, 0, stream.cuda_stream)
        if gate:
            clay_amd.set_encode_path("auto", 0)

    def loop():
        for s in range(n):
            c.encode_device(dls[s], pls[s], chunk, 0, stream.cuda_stream)

    fns, info = [batch, loop], []
    for fn in fns:
        fn()
        torch.cuda.synchronize()
        info.append((clay_amd.last_encode_path(), clay_amd.last_launch_count()))
    ts = [[] for _ in fns]
    for i in range(RUNS + 2):
        for j, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            fn()
            e0.record(stream)
            for _ in range(B2B):
                fn()
            e1.record(stream)
            torch.cuda.synchronize()
            if i >= 2:
                ts[j].append(e0.elapsed_time(e1) / B2B)
    out = {"config": f"encode ({k},{m},{d}) batch_stream {n} x {k * chunk / 2**20:.0f} MiB (sc {sc})",
           "stripe_data_bytes": n * k * chunk}
    for tag, t, (path, launches) in zip(("strided", "loop"), ts, info):
        med = float(np.median(t))
        out[tag] = {"path": path, "launches_per_call": launches if tag == "strided" else n * launches,
                    "median_ms": round(med, 4), "min_ms": round(float(np.min(t)), 4),
                    "spread_ms": round(float(np.max(t) - np.min(t)), 4),
                    "stripe_data_GiBps": round(n * k * chunk / (med * 1e-3) / 2**30, 1)}
    if gate:
        # a win: the batch's median is below the loop's by more than the spread of the loop's samples
        out["batch_wins"] = bool(out["loop"]["median_ms"] - out["strided"]["median_ms"] > out["loop"]["spread_ms"])
    print(json.dumps(out), flush=True)


def batch_decode_stream_cfg(sc, n, er, gate=False, samples=None, loop_mode="stream-local", name="batch_decode_stream"):
    """ONLY=batch_decode_fused2 / batch_decode_fused2_gate (loop_mode "stream-fused2"): the same A/B
    for three and four lost nodes -- ONE launch of the fused decode v2's batch variant (exec mode
    "stream", "stream-fused2-batch") against n launches of "stream-fused2".
    ONLY=batch_decode_stream / batch_decode_stream_gate: n stripes of (10,4,13) at sub-chunk sc
    with the nodes `er` lost in every stripe through clay_decode_device_strided, as ONE launch of the
    local decode's batch variant (exec mode "stream", "stream-local256-batch") and as the library's
    per-stripe loop (exec mode "stream-local", n launches of "stream-local256": the path without the
    batch), samples alternated in one run, B2B back-to-back calls per sample.  Per leg: the samples,
    median, min and spread (max - min) per call of n stripes, and GiB/s of stripe data.  gate: also
    "batch_no_slower" -- the batch's median is at most the loop's plus the spread of the loop's
    samples (the A/B's own run-to-run spread) -- and "batch_wins" -- below it by more than that."""
    global RUNS
    c = ClayCode(10, 4, 13)
    k = 10
    chunk = c.sub_chunk_no * sc
    full = rnd(n * c.n, chunk, 31).view(n, c.n, chunk)
    outs = torch.empty((n, c.n, chunk), dtype=torch.uint8, device="cuda")
    er = list(er)

    def call(mode):
        def fn():
            clay_amd.set_exec_mode(mode)
            c.decode_device_strided(full, er, outs, n, chunk, 0, 0, 0, 0, 0, stream.cuda_stream)
        return fn

    legs = [("batch", call("stream")), ("loop", call(loop_mode))]
    keep = RUNS
    if samples:
        RUNS = samples
    try:
        info, ref = {}, None
        for tag, fn in legs:
            outs.fill_(0)
            fn()
            torch.cuda.synchronize()
            info[tag] = (clay_amd.last_exec_path(), clay_amd.last_launch_count())
            if ref is None:
                ref = outs[:, er].clone()
            else:
                assert torch.equal(outs[:, er], ref), "the two legs differ"
        ts = {tag: [] for tag, _ in legs}
        for i in range(RUNS + 2):
            for tag, fn in legs:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                fn()
                e0.record(stream)
                for _ in range(B2B):
                    fn()
                e1.record(stream)
                torch.cuda.synchronize()
                if i >= 2:
                    ts[tag].append(e0.elapsed_time(e1) / B2B)
        out = {"config": f"decode (10,4,13) {name} {n} x {k * chunk / 2**20:.1f} MiB (sc {sc}) erasures {er}",
               "stripe_data_bytes": n * k * chunk}
        for tag, _ in legs:
            t = ts[tag]
            med = float(np.median(t))
            out[tag] = {"path": info[tag][0], "launches": info[tag][1],
                        "us": [round(x * 1e3, 2) for x in t], "median_us": round(med * 1e3, 2),
                        "min_us": round(float(np.min(t)) * 1e3, 2),
                        "spread_us": round(float(np.max(t) - np.min(t)) * 1e3, 2),
                        "stripe_data_GiBps": round(n * k * chunk / (med * 1e-3) / 2**30, 1)}
        if gate:
            d = out["loop"]["median_us"] - out["batch"]["median_us"]
            out["batch_no_slower"] = bool(d >= -out["loop"]["spread_us"])
            out["batch_wins"] = bool(d > out["loop"]["spread_us"])
        print(json.dumps(out), flush=True)
    finally:
        RUNS = keep
        clay_amd.set_exec_mode(EXEC)


def _scrub_partner(sc):
    """The exec mode under which scrub path 'auto' runs what a library without the streaming batch
    runs for a batch of (10,4,13) at sub-chunk sc under exec auto: from 65,536 the per-stripe
    "stream-scrub" loop ("stream"), below it one launch of v1, "bs-scrub-batch" ("grouped")."""
    return "stream" if sc >= 65536 else "grouped"


def scrub_batch_stream_cfg(sc, counts, with_encode=False, samples=None):
    """ONLY=scrub_batch_stream / scrub_batch_gate: n stripes of (10,4,13) at sub-chunk sc with
    codewords in the buffers through clay_scrub_device_strided, as ONE launch of the streaming batch
    (scrub path 'stream-batch', "stream-scrub-batch") and as its partner (_scrub_partner), with
    with_encode also the batched encode of the same shape into a second parity buffer; the legs'
    samples alternate in one run.  Per leg: the samples, median, min and spread (max - min) per
    call of n stripes.  A win: the batch's median is below the partner's by more than the spread
    of the partner's samples."""
    global RUNS
    c = ClayCode(10, 4, 13)
    k, m = 10, 4
    chunk = c.sub_chunk_no * sc
    nmax = max(counts)
    data = rnd(nmax * k, chunk, 23).view(nmax, k, chunk)
    par = torch.empty((nmax, m, chunk), dtype=torch.uint8, device="cuda")
    c.encode_device_strided(data, par, nmax, chunk, 0, 0, 0, 0, 0, stream.cuda_stream)
    par2 = torch.empty((nmax, m, chunk), dtype=torch.uint8, device="cuda") if with_encode else None
    res = torch.empty(nmax, dtype=torch.int32, device="cuda")
    partner = _scrub_partner(sc)
    keep = RUNS
    if samples:
        RUNS = samples
    try:
        for n in counts:
            def scrub(mode, path):
                def fn():
                    clay_amd.set_exec_mode(mode)
                    clay_amd.set_scrub_path(path)
                    c.scrub_device_strided(data, par, res, n, chunk, 0, 0, 0, 0, 0, stream.cuda_stream)
                return fn

            def encode():
                c.encode_device_strided(data, par2, n, chunk, 0, 0, 0, 0, 0, stream.cuda_stream)

            legs = [("batch", scrub("auto", "stream-batch")), ("partner", scrub(partner, "auto"))]
            if with_encode:
                legs.append(("encode", encode))
            info = {}
            for tag, fn in legs:
                res.fill_(-1)
                fn()
                torch.cuda.synchronize()
                if tag == "encode":
                    info[tag] = (clay_amd.last_encode_path(), clay_amd.last_launch_count())
                    assert torch.equal(par2[:n], par[:n])
                else:
                    info[tag] = (clay_amd.last_exec_path(), clay_amd.last_launch_count())
                    assert not bool(res[:n].any().item()) and bool((res[n:] == -1).all().item())
            ts = {tag: [] for tag, _ in legs}
            for i in range(RUNS + 2):
                for tag, fn in legs:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    fn()
                    e0.record(stream)
                    for _ in range(B2B):
                        fn()
                    e1.record(stream)
                    torch.cuda.synchronize()
                    if i >= 2:
                        ts[tag].append(e0.elapsed_time(e1) / B2B)
            out = {"config": f"scrub (10,4,13) batch_stream {n} x {k * chunk / 2**20:.1f} MiB (sc {sc})",
                   "stripe_data_bytes": n * k * chunk, "partner_exec_mode": partner}
            for tag, _ in legs:
                t = ts[tag]
                med = float(np.median(t))
                out[tag] = {"path": info[tag][0], "launches": info[tag][1],
                            "us": [round(x * 1e3, 2) for x in t], "median_us": round(med * 1e3, 2),
                            "min_us": round(float(np.min(t)) * 1e3, 2),
                            "spread_us": round(float(np.max(t) - np.min(t)) * 1e3, 2),
                            "stripe_data_GiBps": round(n * k * chunk / (med * 1e-3) / 2**30, 1)}
            out["batch_wins"] = bool(out["partner"]["median_us"] - out["batch"]["median_us"] > out["partner"]["spread_us"])
            print(json.dumps(out), flush=True)
    finally:
        RUNS = keep
        clay_amd.set_exec_mode(EXEC)
        clay_amd.set_scrub_path("auto")


def repair_cfg(k, m, d, chunk, lost):
    c = ClayCode(k, m, d)
    sc = chunk // c.sub_chunk_no
    info = c.minimum_to_repair(lost, [i for i in range(c.n) if i != lost])
    helpers = [h for h, _ in info]
    beta = len(info[0][1])
    hb = rnd(len(helpers), beta * sc, 3)
    out = torch.empty(chunk, dtype=torch.uint8, device="cuda")
    ms, mn = timed(lambda: c.repair_device(lost, helpers, [hb[i] for i in range(len(helpers))], chunk, out, 0,
                                           stream.cuda_stream))
    report(f"repair ({k},{m},{d}) chunk {chunk} node {lost}", ms, mn, len(helpers) * beta * sc + chunk)
    del hb
    # same repair straight from whole helper chunks in HBM (only the beta layers are read)
    full = rnd(len(helpers), chunk, 4)
    ms, mn = timed(lambda: c.repair_device_full_chunks(lost, helpers, [full[i] for i in range(len(helpers))],
                                                       chunk, out, 0, stream.cuda_stream))
    report(f"repair ({k},{m},{d}) chunk {chunk} node {lost} from full chunks", ms, mn,
           len(helpers) * beta * sc + chunk)


def prewarm(ms=250.0):
    """Untimed load so every configuration is timed at the GPU's sustained clock."""
    import time
    c = ClayCode(10, 4, 13)
    chunk = c.encoded_chunk_size(1 << 30)
    data, par = rnd(10, chunk, 9), torch.empty((4, chunk), dtype=torch.uint8, device="cuda")
    t0 = time.perf_counter()
    while (time.perf_counter() - t0) * 1e3 < ms:
        for _ in range(8):
            c.encode_device([data[i] for i in range(10)], [par[i] for i in range(4)], chunk, 0, stream.cuda_stream)
        torch.cuda.synchronize()


if __name__ == "__main__":
    prewarm(float(os.environ.get("PREWARM_MS", "250")))
    only = os.environ.get("ONLY", "encode,batch,decode,repair").split(",")
    jobs = [("encode", lambda: encode_cfg(10, 4, 13, 1 << 30)),
            ("encode", lambda: encode_cfg(4, 2, 5, 64 << 20)),
            ("encode", lambda: encode_cfg(9, 3, 11, 9 * (256 << 20))),
            ("batch", lambda: encode_batch_cfg(4, 2, 5, 1 << 20, 256)),
            # the clay_bench.rs stripe sizes with node 0 lost in every stripe, ~64 MiB per call
            # ONLY=batch_stream: many (10,4,13) stripes above 4 MiB, about 1 GiB of data per call, and
            # two stripes of the benchmark's sub-chunk (DESIGN.md 4.4 "Streaming batches")
            *[("batch_stream", (lambda a=a: batch_stream_cfg(*a))) for a in
              ((2048, 205), (6560, 64), (26216, 16), (66176, 6), (419432, 2))],
            # ONLY=batch_stream_gate: the sweep behind auto's gate for the streaming batch where one
            # stripe already fills the chip (one group: only the launch seams are saved)
            *[("batch_stream_gate", (lambda sc=sc, n=n: batch_stream_cfg(sc, n, gate=True)))
              for sc in (32776, 66176, 131080, 262152, 419432) for n in (2, 3, 4, 6)],
            # ONLY=batch_decode_stream: 1 GiB of (10,4,13) data as 64 stripes of 16 MiB, 205 of 5 MiB,
            # 16 of 64 MiB and, for scale, one stripe of 1 GiB (a one-stripe call: the same path in
            # both legs), node 0 and nodes 0 and 4 lost (DESIGN.md 4.11 "Streaming batches")
            *[("batch_decode_stream", (lambda sc=sc, n=n, er=er: batch_decode_stream_cfg(sc, n, er)))
              for er in ([0], [0, 4]) for sc, n in ((6560, 64), (2048, 205), (26216, 16), (419432, 1))],
            # ONLY=batch_decode_stream_gate: the sweep behind auto's gate: sub-chunks from just above the
            # staged batch's 4 MiB of data per stripe (sc 1,640) to the benchmark's 419,432, 2 / 4 / 16 /
            # 64 stripes (cells of more than 4 GiB of stripe data are left out: they do not fit the
            # run's time), both patterns, at least 5 samples per leg
            *[("batch_decode_stream_gate", (lambda sc=sc, n=n, er=er: batch_decode_stream_cfg(
                sc, n, er, gate=True, samples=max(5, RUNS // 2))))
              for sc in (1640, 2048, 6560, 26216, 66176, 131080, 262152, 419432) for n in (2, 4, 16, 64)
              if n * 2560 * sc <= 4 << 30 for er in ([0], [0, 4])],
            # ONLY=batch_decode_fused2: 1 GiB of (10,4,13) data as 64 stripes of 16 MiB, 205 of 5 MiB and
            # 16 of 64 MiB with four, three and (the TWO instantiation) two-in-a-section lost nodes:
            # the batch under "stream" against the per-stripe loop under "stream-fused2" 
            *[("batch_decode_fused2", (lambda sc=sc, n=n, er=er: batch_decode_stream_cfg(
                sc, n, er, loop_mode="stream-fused2", name="batch_decode_fused2")))
              for er in ([0, 4, 8, 12], [0, 4, 8], [0, 1, 4, 8]) for sc, n in ((6560, 64), (2048, 205), (26216, 16))],
            # ONLY=batch_decode_fused2_gate: the sweep behind auto's gate for that batch: the
            # sub-chunks, stripe counts and rule of batch_decode_stream_gate, patterns {0,4,8,12}
            # and {0,1,4,8}
            *[("batch_decode_fused2_gate", (lambda sc=sc, n=n, er=er: batch_decode_stream_cfg(
                sc, n, er, gate=True, samples=max(5, RUNS // 2), loop_mode="stream-fused2", name="batch_decode_fused2")))
              for sc in (1640, 2048, 6560, 26216, 66176, 131080, 262152, 419432) for n in (2, 4, 16, 64)
              if n * 2560 * sc <= 4 << 30 for er in ([0, 4, 8, 12], [0, 1, 4, 8])],
            ("batch_decode", lambda: decode_batch_cfg(4, 2, 5, 1 << 10, 65536, 0, 1024)),
            ("batch_decode", lambda: decode_batch_cfg(4, 2, 5, 10 << 10, 6553, 0, 1024)),
            ("batch_decode", lambda: decode_batch_cfg(4, 2, 5, 100 << 10, 655, 0, 655)),
            ("batch_decode", lambda: decode_batch_cfg(4, 2, 5, 1 << 20, 64, 0, 64)),
            # the same stripe sizes with node 0 lost and repaired from all others (sc = stripe / 32),
            # and the other two codes with a repair kernel at sc = 32 / 320; both helper layouts
            *[("batch_repair", (lambda a=a, f=f: repair_batch_cfg(*a, f))) for f in (False, True) for a in
              ((4, 2, 5, 32, 65536, 0, 1024), (4, 2, 5, 320, 6553, 0, 1024), (4, 2, 5, 3200, 655, 0, 655),
               (4, 2, 5, 32768, 64, 0, 64), (10, 4, 13, 32, 585, 0, 585), (10, 4, 13, 320, 58, 0, 58),
               (9, 3, 11, 32, 2157, 0, 1024), (9, 3, 11, 320, 215, 0, 215))],
            # ONLY=scrub: the scrub against the encode into scratch plus a compare
            ("scrub", lambda: scrub_cfg(4, 2, 5, 64 << 20, ["auto", "grouped"])),
            ("scrub", lambda: scrub_cfg(10, 4, 13, 1 << 30, ["auto", "stream", "grouped"])),
            ("scrub10", lambda: scrub_cfg(10, 4, 13, 1 << 30, ["auto", "stream", "grouped"])),
            # ONLY=scrub_gate: the sweep behind auto's gate for the streaming scrub
            ("scrub_gate", scrub_gate_cfg),
            # ONLY=scrub_batch_stream: many (10,4,13) stripes scrubbed in one launch of the streaming
            # batch, against the path without it and the batched encode of the same shape
            *[("scrub_batch_stream", (lambda sc=sc, n=n: scrub_batch_stream_cfg(sc, [n], with_encode=True)))
              for sc, n in ((6560, 64), (2048, 205), (26216, 16))],
            # ONLY=scrub_batch_gate: the sweep behind auto's gate for it: at least 5
            # samples per leg; the last count of the small sizes is about 1 GiB of data
            *[("scrub_batch_gate", (lambda sc=sc: scrub_batch_stream_cfg(
                sc, [2, 4, 8, 32, 64, round(2**30 / (2560 * sc))], samples=max(5, RUNS // 2))))
              for sc in (2048, 4096, 8192, 16384, 32768)],
            *[("scrub_batch_gate", (lambda sc=sc: scrub_batch_stream_cfg(sc, [2, 3, 4, 6], samples=max(5, RUNS // 2))))
              for sc in (65536, 66176, 131080, 262152, 419432)],
            # ONLY=scrub_batch_fill: between the sweep's 16 and 32 workgroups per XCD (of 32): 20, 24,
            # 28 at sc 2,048, 20, 25, 30 at sc 8,216 (5 per stripe), 26 at sc 26,216 (13 per stripe)
            *[("scrub_batch_fill", (lambda sc=sc, ns=ns: scrub_batch_stream_cfg(sc, ns, samples=max(5, RUNS // 2))))
              for sc, ns in ((2048, [20, 24, 28]), (8216, [4, 5, 6]), (26216, [2, 3, 4]))],
            ("scrub", lambda: scrub_batch_cfg(4, 2, 5, 1 << 10, 65536, 1024)),
            ("scrub", lambda: scrub_batch_cfg(4, 2, 5, 10 << 10, 6553, 1024)),
            ("scrub", lambda: scrub_batch_cfg(4, 2, 5, 100 << 10, 655, 655)),
            ("scrub", lambda: scrub_batch_cfg(4, 2, 5, 1 << 20, 64, 64)),
            ("decode", lambda: decode_cfg(4, 2, 5, 64 << 20, [0])),
            ("decode", lambda: decode_cfg(10, 4, 13, 1 << 30, [0, 4, 8, 12])),
            ("decode", lambda: decode_cfg(10, 4, 13, 1 << 30, [0, 4, 8, 12], "grouped")),
            ("cfg5", lambda: decode_cfg(10, 4, 13, 1 << 30, [0, 4, 8, 12])),  # under CLAY_EXEC
            ("c2e", lambda: encode_cfg(4, 2, 5, 64 << 20)),
            ("c2e", lambda: encode_cfg(4, 2, 5, 64 << 20, "bitsliced")),
            ("cfg2", lambda: decode_cfg(4, 2, 5, 64 << 20, [0])),  # under CLAY_EXEC
            ("cfg2", lambda: decode_cfg(4, 2, 5, 64 << 20, [5])),
            # the fused decode v2 for 3 and 2 erasures in distinct sections (auto: split / local)
            ("f2x", lambda: decode_cfg(10, 4, 13, 1 << 30, [0, 4, 8], "stream-fused2")),
            ("f2x", lambda: decode_cfg(10, 4, 13, 1 << 30, [0, 4, 8])),
            ("f2x", lambda: decode_cfg(10, 4, 13, 1 << 30, [1, 9, 13], "stream-fused2")),
            ("f2x", lambda: decode_cfg(10, 4, 13, 1 << 30, [1, 9, 13])),
            ("f2x", lambda: decode_cfg(10, 4, 13, 1 << 30, [0, 4], "stream-fused2")),
            ("f2x", lambda: decode_cfg(10, 4, 13, 1 << 30, [0, 4])),
            ("decode", lambda: decode_cfg(10, 4, 13, 1 << 30, [0])),
            ("decode23", lambda: decode_cfg(10, 4, 13, 1 << 30, [0, 4])),
            ("decode23", lambda: decode_cfg(10, 4, 13, 1 << 30, [0, 4, 8])),
            # same-section and mixed patterns (the local decode in auto)
            ("decodeL", lambda: decode_cfg(10, 4, 13, 1 << 30, [0, 1])),
            ("decodeL", lambda: decode_cfg(10, 4, 13, 1 << 30, [0, 1, 4])),
            ("decodeL", lambda: decode_cfg(10, 4, 13, 1 << 30, [0, 1, 2, 3])),
            ("decodeL", lambda: decode_cfg(10, 4, 13, 1 << 30, [12])),
            # the local decodes: 256-byte row runs ({0}, {12}, {0,4}) and 64-byte tiles ({0,1})
            ("local", lambda: decode_cfg(10, 4, 13, 1 << 30, [0])),
            ("local", lambda: decode_cfg(10, 4, 13, 1 << 30, [12])),
            ("local", lambda: decode_cfg(10, 4, 13, 1 << 30, [0, 4])),
            ("local", lambda: decode_cfg(10, 4, 13, 1 << 30, [0, 1])),
            ("local", lambda: decode_cfg(9, 4, 12, 1 << 30, [0])),
            ("local", lambda: decode_cfg(9, 4, 12, 1 << 30, [0, 4])),
            # round 6: 4-erasure patterns with two erasures in one section ((2,1,1) and (2,2)
            # sections: 750 of the 1,001 4-erasure patterns), k_stream_fused2 in auto, and the
            # grouped executor they ran on before; {0,8,9,10} runs a split step (neighbouring
            # sections beyond the ring)
            ("two", lambda: decode_cfg(10, 4, 13, 1 << 30, [0, 1, 4, 8])),
            ("two", lambda: decode_cfg(10, 4, 13, 1 << 30, [0, 1, 4, 12])),
            ("two", lambda: decode_cfg(10, 4, 13, 1 << 30, [0, 1, 4, 5])),
            ("two", lambda: decode_cfg(10, 4, 13, 1 << 30, [8, 9, 0, 4])),
            ("two", lambda: decode_cfg(10, 4, 13, 1 << 30, [0, 8, 9, 10])),
            ("two", lambda: decode_cfg(10, 4, 13, 1 << 30, [0, 1, 4, 8], "grouped")),
            ("two", lambda: decode_cfg(10, 4, 13, 1 << 30, [0, 1, 4, 5], "grouped")),
            # clay_decode_device_codeword: one erasure rebuilt by the repair kernel from whole
            # chunks (charged the repair route's bytes)
            ("codeword", lambda: decode_cfg(10, 4, 13, 1 << 30, [0], codeword=True)),
            ("codeword", lambda: decode_cfg(10, 4, 13, 1 << 30, [12], codeword=True)),
            ("codeword", lambda: decode_cfg(9, 3, 11, 9 * (256 << 20), [0])),
            ("codeword", lambda: decode_cfg(9, 3, 11, 9 * (256 << 20), [0], codeword=True)),
            ("repair", lambda: repair_cfg(9, 3, 11, 268_435_458, 0)),
            ("repair", lambda: repair_cfg(9, 3, 11, 268_435_458, 11)),
            ("repair", lambda: repair_cfg(10, 4, 13, 107_374_592, 0)),
            # alignment sensitivity: sub-chunk 3,314,048 (64-byte aligned rows) vs 3,314,018
            ("repair_align", lambda: repair_cfg(9, 3, 11, 81 * 3_314_048, 0))]
    for tag, fn in jobs:
        if tag in only:
            fn()
