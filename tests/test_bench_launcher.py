"""bench.py's own 1 -> N launcher, exercised on CPU (gloo, world_size 2).

`python bench.py --gpus N` without an external torchrun spawns N rank processes
(RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* = 127.0.0.1) before touching HIP; this is
the code the driver's `--gpus 8` run hits.  `--cpu-dry` swaps only the device encode
for the oracle and RCCL for gloo, so the launcher, the barrier-bracketed timing, the
per-rank gather and the JSON line are the production ones."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, timeout=240):
    env = {k: v for k, v in os.environ.items()
           if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env["OMP_NUM_THREADS"] = "1"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True,
                       text=True, timeout=timeout, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.parametrize("world", [1, 2])
def test_bench_launcher_cpu_dry(oracle_mod, world):
    stripe = 10 * 256 * 2 * 64  # sc = 128
    d = _run(["--gpus", str(world), "--cpu-dry", "--stripe-bytes", str(stripe), "--steps", "3",
              "--warmup", "1", "--cpu-seconds", "0"])
    assert d["n_gpus"] == world
    assert d["cpu_dry"] is True
    assert len(d["per_rank"]["wall_ms_per_step"]) == world
    assert all(d["per_rank"]["verified"])
    assert d["scaling"] == "weak" and d["steps"] == 3
    assert d["config"]["parallelism"] == f"stripe-per-gpu x{world}"
    # value = all ranks' bytes / the slowest rank's time
    padded = d["config"]["padded_stripe_bytes"]
    slowest = max(d["per_rank"]["wall_ms_per_step"]) * 1e-3 * d["steps"]
    assert d["value"] == pytest.approx(world * d["steps"] * padded / slowest / 2**30, rel=0.02)
    for key in ("metric", "value", "unit", "ms_per_step", "higher_is_better", "vs_baseline", "dtype",
                "data", "config", "roofline"):
        assert key in d


EXTRA_KEYS = ("cpu_baseline", "cpu_baseline_all_cores", "cpu_baseline_cfg1", "host")


def test_bench_plain_run_dumps_parity_and_skips_extras(oracle_mod, tmp_path):
    """A plain run measures the headline only (no CPU baselines even when --cpu-seconds asks
    for them) and --dump-outputs writes the last step's parity: float32, the whole (M, chunk)
    array at this size, equal to the oracle's parity of the seeded input."""
    import numpy as np
    stripe = 10 * 256 * 2 * 64
    d = _run(["--cpu-dry", "--stripe-bytes", str(stripe), "--steps", "2", "--warmup", "1",
              "--cpu-seconds", "0.3", "--dump-outputs", str(tmp_path / "dump")])
    assert d["steps"] == 2 and d["ms_per_step"] > 0
    for key in EXTRA_KEYS:
        assert key not in d
    for key in ("host_inclusive_GiBps", "gpu_small_stripes", "config_legs"):
        assert d[key] is None
    assert [p.name for p in (tmp_path / "dump").iterdir()] == ["parity.npy"]
    got = np.load(tmp_path / "dump" / "parity.npy")
    padded = d["config"]["padded_stripe_bytes"]
    host = np.random.default_rng(1234).integers(0, 256, padded, dtype=np.uint8)
    ref = oracle_mod.OracleClay(10, 4, 13).encode_array(host)[10:]
    assert got.dtype == np.float32 and got.shape == ref.shape
    assert np.array_equal(got, ref.astype(np.float32))


def test_bench_full_adds_cpu_baselines(oracle_mod):
    stripe = 10 * 256 * 2 * 64
    d = _run(["--cpu-dry", "--full", "--stripe-bytes", str(stripe), "--steps", "2", "--warmup", "1",
              "--cpu-seconds", "0.3"])
    for key in EXTRA_KEYS:
        assert key in d
    assert d["cpu_baseline"]["value"] > 0 and d["cpu_baseline"]["cores"] == 1
    assert d["cpu_baseline_cfg1"]["encode"]["single_thread"] > 0


def test_bench_dump_samples_a_large_parity_reproducibly(tmp_path):
    """A parity above the dump budget is sampled at fixed positions (both ends and seeded draws,
    the same for every parity chunk): two dumps of the same parity are identical, stay inside
    the budget and hold the parity's own bytes at those positions."""
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import bench
    assert bench.M == 4
    chunk = bench.DUMP_BUDGET_BYTES // 4 // bench.M + 100_003
    # byte p of parity chunk i is byte i of p, so a dumped column names the position it came from
    par = torch.from_numpy(np.arange(chunk, dtype="<u4").view(np.uint8).reshape(chunk, 4).T.copy())
    for sub in ("a", "b"):
        bench.dump_outputs(torch, str(tmp_path / sub), par, 1, 0)
    a, b = np.load(tmp_path / "a" / "parity.npy"), np.load(tmp_path / "b" / "parity.npy")
    assert a.dtype == np.float32 and a.shape[0] == bench.M and a.nbytes <= bench.DUMP_BUDGET_BYTES
    assert np.array_equal(a, b)
    pos = (a.astype(np.int64) * (256 ** np.arange(4))[:, None]).sum(axis=0)
    assert (np.diff(pos) > 0).all() and pos[-1] == chunk - 1 and pos.size > chunk // 2
    w = bench.VERIFY_W
    assert np.array_equal(pos[:w], np.arange(w)) and np.array_equal(pos[-w:], np.arange(chunk - w, chunk))


@pytest.mark.gpu
def test_bench_gpu_dump_matches_oracle(oracle_mod, torch_cuda, tmp_path):
    """The real device path at a small ragged stripe (sc = 8 mod 16): the dumped parity of a
    plain run is the oracle's parity of the same seeded device input."""
    import numpy as np
    torch = torch_cuda
    sc = 16 * 300 + 8
    stripe = 10 * 256 * sc
    d = _run(["--stripe-bytes", str(stripe), "--steps", "2", "--warmup", "1", "--prewarm-ms", "0",
              "--dump-outputs", str(tmp_path)])
    assert d["steps"] == 2 and d["ms_per_step"] > 0 and d["config"]["sub_chunk_bytes"] == sc
    assert d["verified_vs_oracle"] is None and d["per_rank"]["verified"] == [None]
    assert d["config_legs"] is None and "cpu_baseline" not in d
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev)
    g.manual_seed(1234)
    data = torch.randint(0, 256, (10, 256 * sc), dtype=torch.uint8, device=dev, generator=g)
    ref = oracle_mod.OracleClay(10, 4, 13).encode_array(data.cpu().numpy().reshape(-1))[10:]
    got = np.load(tmp_path / "parity.npy")
    assert got.dtype == np.float32 and got.shape == ref.shape
    assert np.array_equal(got, ref.astype(np.float32))


def test_bench_launcher_rank_failure_stops_job(oracle_mod):
    """A rank that dies before the rendezvous (bad ordinal, OOM ...) must not leave the
    other rank blocked in init / barrier: the launcher sees the first non-zero exit,
    terminates the rest and exits non-zero, well within 60 s."""
    import time
    stripe = 10 * 256 * 2 * 64
    env = {k: v for k, v in os.environ.items()
           if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env["OMP_NUM_THREADS"] = "1"
    t0 = time.monotonic()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--cpu-dry",
                        "--stripe-bytes", str(stripe), "--steps", "3", "--warmup", "1", "--cpu-seconds", "0",
                        "--fail-rank", "1"], capture_output=True, text=True, timeout=120, cwd=ROOT, env=env)
    el = time.monotonic() - t0
    assert r.returncode != 0
    assert "rank 1 exited with 3" in r.stderr, r.stderr[-2000:]
    assert not [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert el < 60, el


def test_bench_rank_rejects_missing_device():
    """A rank whose LOCAL_RANK has no GPU fails fast with a clear message (here: no GPU at
    all in the container, LOCAL_RANK 0)."""
    env = {k: v for k, v in os.environ.items()
           if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update({"WORLD_SIZE": "1", "RANK": "0", "LOCAL_RANK": "0"})
    import torch
    if torch.cuda.device_count() > 0:
        pytest.skip("a GPU is visible")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--cpu-seconds", "0"],
                       capture_output=True, text=True, timeout=120, cwd=ROOT, env=env)
    assert r.returncode == 2
    assert "only 0 GPU(s) visible" in r.stderr


def test_bench_launcher_builds_stale_oracle_once(oracle_mod, tmp_path):
    """With a stale liboracle.so (clay_oracle.c newer than it, as a fresh checkout can leave
    it), a world-2 run builds the checker exactly once -- in the launcher parent, before any
    rank starts -- instead of N ranks running make on, and loading, the same file at once."""
    src = os.path.join(ROOT, "oracle", "clay_oracle.c")
    so = os.path.join(ROOT, "oracle", "liboracle.so")
    src_st = os.stat(src)
    # make the library stale by moving it into the past (never the source into the future: a
    # future source mtime would keep every later build in other processes rebuilding)
    os.utime(so, (src_st.st_atime - 10, src_st.st_mtime - 10))
    log = tmp_path / "make.log"
    wrapper = tmp_path / "make"
    wrapper.write_text(f"#!/bin/sh\necho \"$@\" >> {log}\nexec /usr/bin/make \"$@\"\n")
    wrapper.chmod(0o755)
    env = {k: v for k, v in os.environ.items()
           if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env["OMP_NUM_THREADS"] = "1"
    env["PATH"] = f"{tmp_path}:{env.get('PATH', '')}"
    stripe = 10 * 256 * 2 * 64
    try:
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--cpu-dry",
                            "--stripe-bytes", str(stripe), "--steps", "2", "--warmup", "1", "--cpu-seconds", "0"],
                           capture_output=True, text=True, timeout=240, cwd=ROOT, env=env)
    finally:
        os.utime(src, (src_st.st_atime, src_st.st_mtime))  # the source's times are untouched
    assert r.returncode == 0, r.stderr[-2000:]
    d = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][0])
    assert all(d["per_rank"]["verified"])
    makes = log.read_text().splitlines() if log.exists() else []
    assert len(makes) == 1, makes
    assert os.path.getmtime(so) >= os.path.getmtime(src)
