#!/bin/bash
# The evidence of profiles/svr_search/, collected on the GPU box from the repository root:  tools/profile_svr_search.sh OUTDIR
# One time-bounded GPU step per measurement, chained: a step that fails, faults or runs into its limit ends the script.
#   batched / fallback wall times (fresh processes, in the order batched, fallback), the scoring comparison, and one kernel trace of
#   a batched fit (the program after `--` is python3 itself)
set -o pipefail
out=${1:?usage: tools/profile_svr_search.sh OUTDIR}
mkdir -p "$out"
export TMPDIR=/tmp
timeout -k 10 200 python3 tools/svr_search_probe.py batched 100 3 > "$out/batched.json" 2> "$out/batched.err" &&
timeout -k 10 400 python3 tools/svr_search_probe.py fallback 100 2 > "$out/fallback.json" 2> "$out/fallback.err" &&
timeout -k 10 200 python3 tools/svr_search_probe.py scoring 100 3 > "$out/scoring.json" 2> "$out/scoring.err" &&
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d "$out/trace" -- python3 tools/svr_search_probe.py batched 100 1 \
    > "$out/batched_under_rocprof.json" 2> "$out/trace.err"
rc=$?
if [ $rc -ne 0 ]; then tail -5 "$out"/*.err; exit $rc; fi
db=$(find "$out/trace" -name '*_results.db' | head -1)
if [ -n "$db" ]; then python3 tools/rocpd_stats.py "$db" > "$out/batched_kernel_stats.csv"; else cp "$(find "$out/trace" -name '*kernel_stats.csv' | head -1)" "$out/batched_kernel_stats.csv"; fi
rm -rf "$out/trace"   # the raw trace is large: keep the summary
head -8 "$out/batched_kernel_stats.csv"
cat "$out/batched.json" "$out/fallback.json" "$out/scoring.json"
