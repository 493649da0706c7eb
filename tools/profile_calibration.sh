#!/bin/bash
# The timing of profiles/calibration/, collected on the GPU box from the repository root:  tools/profile_calibration.sh OUTDIR
# One time-bounded GPU step per measurement, chained: a step that fails, faults or runs into its limit ends the script.
#   wall times: the written-out loop and CalibratedSVC.fit alternate in fresh processes, two rounds of three warmed fits each
#   (tools/calibration_probe.py: n = 20 000, d = 64, 3 classes, 5 folds, hinge, ProjectedGradient, 200 iterations, fp64)
set -o pipefail
out=${1:?usage: tools/profile_calibration.sh OUTDIR}
mkdir -p "$out"
timeout -k 10 150 python3 tools/calibration_probe.py loop 200 3 > "$out/loop_1.json" 2> "$out/loop_1.err" &&
timeout -k 10 100 python3 tools/calibration_probe.py batched 200 3 > "$out/batched_1.json" 2> "$out/batched_1.err" &&
timeout -k 10 150 python3 tools/calibration_probe.py loop 200 3 > "$out/loop_2.json" 2> "$out/loop_2.err" &&
timeout -k 10 100 python3 tools/calibration_probe.py batched 200 3 > "$out/batched_2.json" 2> "$out/batched_2.err"
rc=$?
if [ $rc -ne 0 ]; then tail -5 "$out"/*.err; exit $rc; fi
python3 - "$out" <<'PY'
import json, statistics, sys
out = sys.argv[1]
runs = {side: [json.load(open('%s/%s_%d.json' % (out, side, i))) for i in (1, 2)] for side in ('loop', 'batched')}
t = {side: [s for r in runs[side] for s in r['fit_s']] for side in runs}
rec = dict(config={key: runs['loop'][0][key] for key in ('n', 'd', 'k', 'folds', 'max_iter')},
           order='loop, batched, loop, batched (fresh processes)', loop_fit_s=t['loop'], batched_fit_s=t['batched'],
           loop_median_s=statistics.median(t['loop']), batched_median_s=statistics.median(t['batched']),
           ratio_of_medians=statistics.median(t['loop']) / statistics.median(t['batched']),
           separated=max(t['batched']) < min(t['loop']), loop_fold_fits_batched=runs['loop'][0]['fold_fits_batched'],
           A_loop=runs['loop'][0]['A'], A_batched=runs['batched'][0]['A'], iters_loop=runs['loop'][0]['iters'],
           iters_batched=runs['batched'][0]['iters'], flags_batched=runs['batched'][0]['flags'])
json.dump(rec, open(out + '/fit_timings.json', 'w'), indent=1)
print(json.dumps(rec))
PY
