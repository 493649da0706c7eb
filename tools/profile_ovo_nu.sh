#!/bin/bash
# The single-library figures of profiles/ovo_nu/, collected on the GPU box from the repository root:  tools/profile_ovo_nu.sh OUTDIR
# One time-bounded GPU step per measurement, chained: a step that fails, faults or runs into its limit ends the script.
#   iteration.json     tools/bench_nu.py ovo: n = 100 000, d = 128, 10 equal classes, the 45 pair columns at nu = 0.5; three rounds of
#                      (the BLOCKS columns on the routed product, the same columns as LABELS columns on the 16-column product)
#   kernel_stats.csv   tools/bench_nu.py ovo_pairs under rocprofv3 --kernel-trace --stats, a run of its own: the product
#                      (symmp_*), the search (sx_tau_kernel), the direction pass (sx_dir_kernel) and the close (sx_close_kernel,
#                      sx_top_kernel, symmp_live_kernel)
# (timing.json compares two builds of the library, five processes a side; kernel_resources_*.txt and flavours_*.txt likewise.)
set -o pipefail
export TMPDIR=/tmp
out=${1:?usage: tools/profile_ovo_nu.sh OUTDIR}
mkdir -p "$out"
timeout -k 10 300 python3 tools/bench_nu.py ovo > "$out/iteration.json" 2> "$out/iteration.err" &&
timeout -k 10 240 rocprofv3 --kernel-trace --stats -d "$out/trace" -- python3 tools/bench_nu.py ovo_pairs > "$out/ovo_pairs_under_rocprof.json" 2> "$out/trace.err"
rc=$?
if [ $rc -ne 0 ]; then tail -5 "$out"/*.err; exit $rc; fi
db=$(find "$out/trace" -name '*_results.db' | head -1)
if [ -n "$db" ]; then python3 tools/rocpd_stats.py "$db" > "$out/kernel_stats.csv"
else cp "$(find "$out/trace" -name '*kernel_stats.csv' | head -1)" "$out/kernel_stats.csv"; fi
rm -rf "$out/trace"
rm -f "$out"/*.err
cat "$out/iteration.json"
head -12 "$out/kernel_stats.csv"
