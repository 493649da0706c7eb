#!/bin/bash
# The figures of profiles/nu/, collected on the GPU box from the repository root:  tools/profile_nu.sh OUTDIR
# One time-bounded GPU step per measurement, chained: a step that fails, faults or runs into its limit ends the script.
#   iteration.json               tools/bench_nu.py iter: n = 100 000, d = 128, RBF, 16 columns; three rounds of (one-class, LABELS, PAIRED),
#                                50 timed iterations after 5 each, on one panel
#   kernel_stats_oneclass.csv    tools/bench_nu.py oneclass under rocprofv3 --kernel-trace --stats, a run of its own
#   kernel_stats_labels.csv      the same for the two-group LABELS solve: the product / projection / closing split
#   kernel_resource_usage.txt    the compiler's register, LDS and scratch figures of bq_simplex.hip's kernels (no GPU)
set -o pipefail
export TMPDIR=/tmp
out=${1:?usage: tools/profile_nu.sh OUTDIR}
mkdir -p "$out"
stats() {   # the summary of the trace under $out/trace_$1, then the raw trace goes (it is large)
    db=$(find "$out/trace_$1" -name '*_results.db' | head -1)
    if [ -n "$db" ]; then python3 tools/rocpd_stats.py "$db" > "$out/kernel_stats_$1.csv"
    else cp "$(find "$out/trace_$1" -name '*kernel_stats.csv' | head -1)" "$out/kernel_stats_$1.csv"; fi
    rm -rf "$out/trace_$1"
}
timeout -k 10 300 python3 tools/bench_nu.py iter > "$out/iteration.json" 2> "$out/iteration.err" &&
timeout -k 10 240 rocprofv3 --kernel-trace --stats -d "$out/trace_oneclass" -- python3 tools/bench_nu.py oneclass > "$out/oneclass_under_rocprof.json" 2> "$out/trace_oneclass.err" &&
timeout -k 10 240 rocprofv3 --kernel-trace --stats -d "$out/trace_labels" -- python3 tools/bench_nu.py labels > "$out/labels_under_rocprof.json" 2> "$out/trace_labels.err" &&
{ echo "hipcc -O3 -std=c++17 --offload-arch=gfx950 -ffp-contract=on -Rpass-analysis=kernel-resource-usage (bq_simplex.hip)"
  hipcc -x hip -c optiml_amd/csrc/bq_simplex.hip -o /dev/null -O3 -std=c++17 -fPIC --offload-arch=gfx950 -ffp-contract=on \
      -Iinclude -Rpass-analysis=kernel-resource-usage 2>&1 |
      grep -E "Function Name|VGPRs:|AGPRs|TotalSGPRs|Spill|ScratchSize|LDS Size|Occupancy" |
      sed -E 's/^.*remark: +//; s/ \[-Rpass-analysis=kernel-resource-usage\]//'; } > "$out/kernel_resource_usage.txt"
rc=$?
if [ $rc -ne 0 ]; then tail -5 "$out"/*.err; exit $rc; fi
stats oneclass
stats labels
rm -f "$out"/*.err
cat "$out/iteration.json"
head -8 "$out/kernel_stats_oneclass.csv" "$out/kernel_stats_labels.csv"
