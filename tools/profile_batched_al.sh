#!/bin/bash
# The evidence of profiles/batched_al/, collected on the GPU box from the repository root:  tools/profile_batched_al.sh OUTDIR
# One time-bounded GPU step per measurement, chained: a step that fails, faults or runs into its limit ends the script.
#   wall times: the loop of k SVC.fit and OneVsRestSVC.fit alternate in fresh processes, two rounds of three warmed fits each
#   (tools/batched_al_probe.py: n = 20 000, d = 64, k = 8, hinge, reg_intercept=False, AdaGrad(1.), 200 iterations, fp64);
#   kernel traces: one run of each side with one fit, apart from the timing runs (the program after `--` is python3 itself)
set -o pipefail
out=${1:?usage: tools/profile_batched_al.sh OUTDIR}
mkdir -p "$out"
export TMPDIR=/tmp
timeout -k 10 150 python3 tools/batched_al_probe.py loop 200 3 > "$out/loop_1.json" 2> "$out/loop_1.err" &&
timeout -k 10 100 python3 tools/batched_al_probe.py batched 200 3 > "$out/batched_1.json" 2> "$out/batched_1.err" &&
timeout -k 10 150 python3 tools/batched_al_probe.py loop 200 3 > "$out/loop_2.json" 2> "$out/loop_2.err" &&
timeout -k 10 100 python3 tools/batched_al_probe.py batched 200 3 > "$out/batched_2.json" 2> "$out/batched_2.err" &&
timeout -k 10 200 rocprofv3 --kernel-trace --stats -d "$out/trace_loop" -- python3 tools/batched_al_probe.py loop 200 1 \
    > "$out/loop_under_rocprof.json" 2> "$out/trace_loop.err" &&
timeout -k 10 200 rocprofv3 --kernel-trace --stats -d "$out/trace_batched" -- python3 tools/batched_al_probe.py batched 200 1 \
    > "$out/batched_under_rocprof.json" 2> "$out/trace_batched.err"
rc=$?
if [ $rc -ne 0 ]; then tail -5 "$out"/*.err; exit $rc; fi
for side in loop batched; do
    db=$(find "$out/trace_$side" -name '*_results.db' | head -1)
    if [ -n "$db" ]; then python3 tools/rocpd_stats.py "$db" > "$out/${side}_kernel_stats.csv"
    else cp "$(find "$out/trace_$side" -name '*kernel_stats.csv' | head -1)" "$out/${side}_kernel_stats.csv"; fi
    rm -rf "$out/trace_$side"   # the raw trace is large: keep the summary
done
python3 - "$out" <<'PY'
import json, statistics, sys
out = sys.argv[1]
runs = {side: [json.load(open('%s/%s_%d.json' % (out, side, i))) for i in (1, 2)] for side in ('loop', 'batched')}
t = {side: [s for r in runs[side] for s in r['fit_s']] for side in runs}
rec = dict(config={key: runs['loop'][0][key] for key in ('n', 'd', 'k', 'max_iter')}, order='loop, batched, loop, batched (fresh processes)',
           loop_fit_s=t['loop'], batched_fit_s=t['batched'], loop_median_s=statistics.median(t['loop']),
           batched_median_s=statistics.median(t['batched']),
           ratio_of_medians=statistics.median(t['loop']) / statistics.median(t['batched']),
           separated=max(t['batched']) < min(t['loop']),
           loss_last_loop=runs['loop'][0]['loss_last'], loss_last_batched=runs['batched'][0]['loss_last'])
json.dump(rec, open(out + '/fit_timings.json', 'w'), indent=1)
print(json.dumps(rec))
PY
head -12 "$out/loop_kernel_stats.csv" "$out/batched_kernel_stats.csv"
