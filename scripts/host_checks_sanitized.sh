#!/bin/bash
# The stand-alone host check programs (tests/host/*_check.cpp: each includes a plain-integer header
# of clay_amd/csrc and has its own main) built with ASan + UBSan and run once.  CPU only, no GPU,
# nothing is loaded into Python.  Arguments: the checks to run (default: all), e.g.
#   scripts/host_checks_sanitized.sh stream_batch_map_check
set -eo pipefail
R=$(cd "$(dirname "$0")/.." && pwd)
CXX=${CXX:-c++}
OUT=$(mktemp -d)
trap 'rm -rf "$OUT"' EXIT
if [ $# -eq 0 ]; then
    set -- $(cd "$R/tests/host" && ls *_check.cpp | sed 's/\.cpp$//')
fi
export ASAN_OPTIONS=halt_on_error=1:abort_on_error=1 UBSAN_OPTIONS=halt_on_error=1:print_stacktrace=1
for name in "$@"; do
    "$CXX" -std=c++17 -O1 -g -Wall -Werror -fno-omit-frame-pointer -fsanitize=address,undefined \
        -fno-sanitize-recover=undefined -I "$R/clay_amd/csrc" -o "$OUT/$name" "$R/tests/host/$name.cpp"
    "$OUT/$name"
done
