"""Batched decision function against the loop over the estimators, at a size a user would run.

    python tools/decision_batch_probe.py --stage e2e  --work DIR [--n 20000] [--t 20000] [--d 128] [--classes 10] [--reps 5]
    python tools/decision_batch_probe.py --stage abi  --work DIR [--ks 2,4,16,45] [--reps 5]
    python tools/decision_batch_probe.py --stage stats --work DIR --csv KERNEL_STATS_CSV --out profiles/decision_batch/NAME.json

Three stages, each a process of its own (a caller puts each under its own time limit):

e2e    OneVsOneSVC (gaussian, numeric gamma, PG, max_iter 20) fitted on 10-class blobs; `decision_function` on t test points through
       the batched path (`bq_decision_function_multi`, one pass) and through the loop over `estimators_` (one `bq_decision_function`
       per pair), alternated in one process: median of `reps` after one warm-up each, and the largest deviation between the two.
       Leaves the stored batch (SV, W, b) and the test points in DIR.
abi    the raw call on that SV at the first k columns of W for each k in --ks, and the loop of k single-column calls on the same
       union SV for comparison; median of `reps` after one warm-up.  Also `bq_ctx_probe_mfma_f64` on the same card.
stats  joins the two with the per-kernel times of a `rocprofv3 --kernel-trace --stats` run of the abi stage (its *_kernel_stats.csv):
       the fused kernel's MFMA FLOP/s from shapes (2 tp mp dp for the dot products + 2 tp mp 16 groups for the contraction, padded
       sizes, as executed) over its kernel time, against the probe.

Every timed call ends in a device synchronise (the entry points copy their result to the host).
"""
import argparse
import csv
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _median_ms(fn, reps):
    fn()   # warm-up
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), ts


def _up(a, m):
    return -(-a // m) * m


def stage_e2e(a):
    from optiml_amd.datasets import make_multiclass_blobs
    from optiml_amd.ml.svm import OneVsOneSVC
    from optiml_amd.ml.svm.kernels import GaussianKernel
    from optiml_amd.ml.svm.losses import hinge
    from optiml_amd.ml.svm.onevsone import ovo_decision
    from optiml_amd.opti.constrained import ProjectedGradient
    X, y = make_multiclass_blobs(a.n + a.t, a.d, a.classes, seed=0)
    Xtr, ytr, Xte = X[:a.n], y[:a.n], np.ascontiguousarray(X[a.n:])
    t0 = time.perf_counter()
    est = OneVsOneSVC(loss=hinge, kernel=GaussianKernel(gamma=1.0 / a.d), C=1.0, reg_intercept=True, dual=True, max_iter=20,
                      optimizer=ProjectedGradient).fit(Xtr, ytr)
    fit_s = time.perf_counter() - t0
    assert est.batched_ and est.batched_decision_

    def loop():
        conf = np.stack([np.ravel(e.decision_function(Xte)) for e in est.estimators_], axis=1)
        return ovo_decision((conf > 0).astype(int), conf, len(est.classes_))

    out = {}
    new_ms, new_all, loop_ms, loop_all = [], [], [], []
    est.decision_function(Xte)
    loop()
    for _ in range(a.reps):   # alternated
        t0 = time.perf_counter()
        out['new'] = est.decision_function(Xte)
        new_all.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        out['loop'] = loop()
        loop_all.append((time.perf_counter() - t0) * 1e3)
    new_ms, loop_ms = statistics.median(new_all), statistics.median(loop_all)
    batch = est.decision_batch_
    res = dict(n=a.n, t=a.t, d=a.d, classes=a.classes, pairs=len(est.estimators_), max_iter=20, fit_s=fit_s,
               union_rows=int(batch.SV.shape[0]), sum_support=int(sum(len(e.support_) for e in est.estimators_)),
               batched_ms=new_ms, batched_runs_ms=new_all, loop_ms=loop_ms, loop_runs_ms=loop_all, speedup=loop_ms / new_ms,
               max_abs_diff=float(np.abs(out['new'] - out['loop']).max()),
               labels_equal=bool(np.array_equal(out['new'].argmax(1), out['loop'].argmax(1))))
    os.makedirs(a.work, exist_ok=True)
    np.savez(os.path.join(a.work, 'batch.npz'), SV=batch.SV, W=batch.W, b=batch.b, Xte=Xte, spec=np.array(batch.spec, dtype=float))
    with open(os.path.join(a.work, 'e2e.json'), 'w') as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res), flush=True)


def stage_abi(a):
    from optiml_amd import _lib
    from optiml_amd.device import get_context
    from optiml_amd.ml.svm._batched import batched_decision
    z = np.load(os.path.join(a.work, 'batch.npz'))
    SV, W, b, Xte = z['SV'], z['W'], z['b'], z['Xte']
    spec = (int(z['spec'][0]), float(z['spec'][1]), float(z['spec'][2]), int(z['spec'][3]))
    ctx = get_context()
    lib = _lib.load()
    m, d = SV.shape
    t = Xte.shape[0]
    res = dict(m=m, t=t, d=d, k={})

    def single(c):
        out = np.empty(t)
        w = np.ascontiguousarray(W[c])
        _lib.check(lib.bq_decision_function(ctx.handle, spec[0], spec[1], spec[2], spec[3], m, d, _lib.ptr(SV), _lib.ptr(w),
                                            float(b[c]), t, _lib.ptr(Xte), _lib.ptr(out)))
        return out

    for k in [int(v) for v in a.ks.split(',')]:
        k = min(k, W.shape[0])
        multi_ms, multi_all = _median_ms(lambda: batched_decision(spec, SV, W[:k], b[:k], Xte), a.reps)
        rec = dict(multi_ms=multi_ms, multi_runs_ms=multi_all)
        if not a.no_loop:
            loop_ms, loop_all = _median_ms(lambda: [single(c) for c in range(k)], a.reps)
            rec.update(loop_same_sv_ms=loop_ms, loop_same_sv_runs_ms=loop_all, speedup=loop_ms / multi_ms)
        res['k'][k] = rec
        print(json.dumps({k: rec}), flush=True)
    res['probe_mfma_f64_tflops'] = ctx.probe_mfma_f64(1.0)
    with open(os.path.join(a.work, 'abi.json'), 'w') as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(dict(probe_mfma_f64_tflops=res['probe_mfma_f64_tflops'])), flush=True)


def stage_stats(a):
    e2e = json.load(open(os.path.join(a.work, 'e2e.json')))
    abi = json.load(open(os.path.join(a.work, 'abi.json')))
    m, t, d = abi['m'], abi['t'], abi['d']
    mp, tp, dp = _up(m, 128), _up(t, 128), _up(d, 16)
    kernels = []
    for row in csv.DictReader(open(a.csv)):
        if 'decide_multi_kernel' in row['Name']:
            gmax = 1 if ', 1, ' in row['Name'] else 4
            kernels.append(dict(name=row['Name'], calls=int(row['Calls']), avg_ms=float(row['AverageNs']) * 1e-6,
                                min_ms=float(row['MinNs']) * 1e-6, gmax=gmax))
    probe = abi['probe_mfma_f64_tflops']
    for kr in kernels:
        # the traced run holds one k per instantiation (--ks 16,45): groups executed = 1, or 3 of the 4 a pass may hold
        groups = 1 if kr['gmax'] == 1 else a.traced_groups
        flops = 2.0 * tp * mp * dp + 2.0 * tp * mp * 16 * groups
        kr.update(groups=groups, mfma_flops=flops, tflops=flops / (kr['avg_ms'] * 1e-3) / 1e12,
                  frac_of_probe=flops / (kr['avg_ms'] * 1e-3) / 1e12 / probe)
    res = dict(e2e=e2e, abi=abi, kernels=kernels, padded=dict(mp=mp, tp=tp, dp=dp))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(dict(kernels=kernels)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--stage', required=True, choices=['e2e', 'abi', 'stats'])
    ap.add_argument('--work', required=True)
    ap.add_argument('--n', type=int, default=20000)
    ap.add_argument('--t', type=int, default=20000)
    ap.add_argument('--d', type=int, default=128)
    ap.add_argument('--classes', type=int, default=10)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--ks', default='2,4,16,45')
    ap.add_argument('--no-loop', action='store_true')
    ap.add_argument('--csv', default=None)
    ap.add_argument('--traced-groups', type=int, default=3)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    dict(e2e=stage_e2e, abi=stage_abi, stats=stage_stats)[a.stage](a)


if __name__ == '__main__':
    main()
