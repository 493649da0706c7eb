#!/bin/bash
# The figures of profiles/oneclass/, collected on the GPU box from the repository root:  tools/profile_oneclass.sh OUTDIR
# One time-bounded GPU step per measurement, chained: a step that fails, faults or runs into its limit ends the script.
#   iteration.json     tools/bench_oneclass.py iter: n = 100 000, d = 128, RBF, 16 columns, 50 timed iterations after 5
#   kernel_stats.csv   the same run under rocprofv3 --kernel-trace --stats, a run of its own: the product / projection / closing split
#   fit.json           OneClassSVM.fit to tol 1e-3 at that size, wall time
#   sklearn_cpu.json   sklearn.svm.OneClassSVM.fit on the CPU at n = 20 000 of the same data (no GPU; about two minutes)
#   kernel_resource_usage.txt   the compiler's register, LDS and scratch figures of bq_simplex.hip's kernels (no GPU)
set -o pipefail
export TMPDIR=/tmp
out=${1:?usage: tools/profile_oneclass.sh OUTDIR}
mkdir -p "$out"
timeout -k 10 240 python3 tools/bench_oneclass.py iter > "$out/iteration.json" 2> "$out/iteration.err" &&
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d "$out/trace" -- python3 tools/bench_oneclass.py iter > "$out/iteration_under_rocprof.json" 2> "$out/trace.err" &&
timeout -k 10 240 python3 tools/bench_oneclass.py fit > "$out/fit.json" 2> "$out/fit.err" &&
timeout -k 10 900 python3 tools/bench_oneclass.py sklearn > "$out/sklearn_cpu.json" 2> "$out/sklearn_cpu.err" &&
{ echo "hipcc -O3 -std=c++17 --offload-arch=gfx950 -ffp-contract=on -Rpass-analysis=kernel-resource-usage (bq_simplex.hip)"
  hipcc -x hip -c optiml_amd/csrc/bq_simplex.hip -o /dev/null -O3 -std=c++17 -fPIC --offload-arch=gfx950 -ffp-contract=on \
      -Rpass-analysis=kernel-resource-usage 2>&1 |
      grep -E "Function Name|VGPRs:|AGPRs|TotalSGPRs|Spill|ScratchSize|LDS Size|Occupancy" |
      sed -E 's/^.*remark: +//; s/ \[-Rpass-analysis=kernel-resource-usage\]//'; } > "$out/kernel_resource_usage.txt"
rc=$?
if [ $rc -ne 0 ]; then tail -5 "$out"/*.err; exit $rc; fi
db=$(find "$out/trace" -name '*_results.db' | head -1)
if [ -n "$db" ]; then python3 tools/rocpd_stats.py "$db" > "$out/kernel_stats.csv"
else cp "$(find "$out/trace" -name '*kernel_stats.csv' | head -1)" "$out/kernel_stats.csv"; fi
rm -rf "$out/trace"   # the raw trace is large: keep the summary
cat "$out/iteration.json" "$out/fit.json"
head -12 "$out/kernel_stats.csv"
