#!/bin/bash
# GPU-box check: parity tests, smoke, bench, rocprof kernel stats.  Each GPU step
# has its own time limit; steps are chained so the first failure ends the run.
#   OUT_DIR=dir   where the logs go (default: out/ in the repository)
#   SKIP_SLOW=1   skip the BASELINE-size tests
#   PROBE_T=1     run the encode segment-timing probe (bench_tools/stream_probe <sc> t) first
#   PMC=1         PMC passes of the encode after the profile
set -o pipefail
R=${GRAFT_REPO_ROOT:-$(cd "$(dirname "$0")/.." && pwd)}
cd "$R" || exit 1
OUT=$(mkdir -p "${OUT_DIR:-out}" && cd "${OUT_DIR:-out}" && pwd) || exit 1
TAG=${1:-run}
PYT="python -u -m pytest -x -q --timeout 300 --timeout-method thread"
if [ -n "$PROBE_T" ]; then
echo "[$(date +%T)] encode segment timing"
timeout -k 10 120 ./bench_tools/stream_probe 419432 t > $OUT/${TAG}_timing.txt 2>&1 || { echo "probe failed rc=$?"; tail -20 $OUT/${TAG}_timing.txt; exit 1; }
cat $OUT/${TAG}_timing.txt
fi
echo "[$(date +%T)] pytest -m gpu (not slow)"
timeout -k 10 600 $PYT tests -m "gpu and not slow" > $OUT/${TAG}_pytest_fast.log 2>&1 || { echo "pytest fast failed rc=$?"; tail -40 $OUT/${TAG}_pytest_fast.log; exit 1; }
tail -3 $OUT/${TAG}_pytest_fast.log
if [ -z "$SKIP_SLOW" ]; then
echo "[$(date +%T)] pytest -m 'gpu and slow' (BASELINE sizes)"
timeout -k 10 900 $PYT tests -m "gpu and slow" > $OUT/${TAG}_pytest_slow.log 2>&1 || { echo "pytest slow failed rc=$?"; tail -40 $OUT/${TAG}_pytest_slow.log; exit 1; }
tail -3 $OUT/${TAG}_pytest_slow.log
fi
echo "[$(date +%T)] smoke"
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > $OUT/${TAG}_smoke.log 2>&1 || { echo "smoke failed"; tail -30 $OUT/${TAG}_smoke.log; exit 1; }
tail -2 $OUT/${TAG}_smoke.log
echo "[$(date +%T)] bench (--full: oracle check, host path, small stripes, config legs, CPU baselines)"
timeout -k 10 400 python bench.py --full --steps 20 --warmup 5 > $OUT/${TAG}_bench.log 2>&1 || { echo "bench failed"; tail -30 $OUT/${TAG}_bench.log; exit 1; }
tail -2 $OUT/${TAG}_bench.log
echo "[$(date +%T)] rocprofv3 kernel trace"
export TMPDIR=/tmp
( cd /tmp && timeout -k 10 400 rocprofv3 --kernel-trace --stats -d "$OUT/${TAG}_prof" -o enc --output-format csv -- python3 "$R/bench.py" --full --steps 20 --warmup 5 --no-verify --no-host-path --cpu-seconds 0 ) > $OUT/${TAG}_rocprof.log 2>&1 || { echo "rocprof failed"; tail -30 $OUT/${TAG}_rocprof.log; exit 1; }
find $OUT/${TAG}_prof -type f ! -name "*stats*" -delete
find $OUT/${TAG}_prof -name "*stats*"
if [ -n "$PMC" ]; then
echo "[$(date +%T)] PMC passes"
bash scripts/prof_pmc.sh ${TAG}_pmc auto 0 || { echo "pmc failed"; exit 1; }
fi
echo "[$(date +%T)] done"
