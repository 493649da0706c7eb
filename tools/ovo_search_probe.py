"""OneVsOneGridSearchCV measured: n = 20 000, d = 32, 10 classes, 3 folds x 4 C (540 columns), max_iter = 200, ProjectedGradient
(or `python tools/ovo_search_probe.py N D CLASSES [OUT.json]`).  OneVsOneGridSearchCV.fit against SVCGridSearchCV(OneVsOneSVC) (the
per-fold path), both refit=False, two passes (the first warms code objects and the panel cache); the batched solve's time per
iteration; one vote_heldout_pairs call; device memory in use before that call and the call's scratch computed from the shapes.
Prints one JSON record (profiles/ovo_search/)."""
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np

from optiml_amd.datasets import make_multiclass_blobs
from optiml_amd.ml.svm import OneVsOneGridSearchCV, OneVsOneSVC, SVCGridSearchCV
from optiml_amd.ml.svm import _batched, ovo_search
from optiml_amd.ml.svm.kernels import GaussianKernel
from optiml_amd.ml.svm.losses import hinge
from optiml_amd.opti.constrained import ProjectedGradient

n, d, classes = (int(a) for a in (sys.argv[1:4] if len(sys.argv) > 3 else (20000, 32, 10)))
X, y = make_multiclass_blobs(n, d, classes, seed=1)
kw = dict(loss=hinge, kernel=GaussianKernel(gamma=1.0 / d), reg_intercept=True, dual=True, max_iter=200, optimizer=ProjectedGradient)
grid = {'C': [0.1, 0.5, 1.0, 4.0]}
rec = dict(n=n, d=d, classes=classes, folds=3, candidates=4, max_iter=200)

free0 = _batched.device_free_bytes()
times = dict(solve=[], vote=[], in_use_before_vote=[])
solve_batched, vote = ovo_search.solve_batched, _batched._DeviceMultiSolver.vote_heldout_pairs


def timed_solve(*a, **k):
    t0 = time.perf_counter()
    out = solve_batched(*a, **k)
    times['solve'].append((time.perf_counter() - t0, max(r['iter'] for r in out), len(out)))
    return out


def timed_vote(self, *a, **k):
    times['in_use_before_vote'].append(free0 - _batched.device_free_bytes())
    t0 = time.perf_counter()
    out = vote(self, *a, **k)   # ends in a device synchronise
    times['vote'].append(time.perf_counter() - t0)
    return out


ovo_search.solve_batched = timed_solve
_batched._DeviceMultiSolver.vote_heldout_pairs = timed_vote

for rep in range(2):   # the first pass warms code objects and the panel cache
    t0 = time.perf_counter()
    ours = OneVsOneGridSearchCV(OneVsOneSVC(**kw), grid, cv=3, refit=False).fit(X, y)
    t_ours = time.perf_counter() - t0
    t0 = time.perf_counter()
    ref = SVCGridSearchCV(OneVsOneSVC(**kw), grid, cv=3, refit=False).fit(X, y)
    t_ref = time.perf_counter() - t0
    print('pass %d: batched %.2f s (batched_=%s), per-fold %.2f s' % (rep, t_ours, ours.batched_, t_ref), flush=True)
    rec['pass%d' % rep] = dict(batched_fit_s=t_ours, per_fold_fit_s=t_ref)

solve_s, iters, cols = times['solve'][-1]
n_pad = int(np.sum((np.bincount(y) + 255) // 256) * 256)
scratch = 8 * (2 * ((cols + 15) // 16 * 16) * (n_pad + 256) + 16 * (n_pad // 256) ** 2 * 256)
rec.update(batched_=bool(ours.batched_), columns=cols, n_pad=n_pad, solves=len(times['solve']) // 2,
           solve_s=solve_s, solve_iters=int(iters), ms_per_iteration=1e3 * (solve_s - times['vote'][-1]) / iters,
           vote_call_s=times['vote'][-1], vote_share_of_fit=times['vote'][-1] / t_ours,
           device_bytes_in_use_before_vote=int(times['in_use_before_vote'][-1]), vote_scratch_bytes_computed=int(scratch),
           peak_device_bytes_estimate=int(times['in_use_before_vote'][-1] + scratch),
           scores_equal=bool(all(np.array_equal(ours.cv_results_['split%d_test_score' % i], ref.cv_results_['split%d_test_score' % i])
                                 for i in range(3))),
           mean_test_score_batched=[float(v) for v in ours.cv_results_['mean_test_score']],
           mean_test_score_per_fold=[float(v) for v in ref.cv_results_['mean_test_score']],
           stopped_share=float((ours.status_ == 'stopped').mean()))
if len(sys.argv) > 4:
    with open(sys.argv[4], 'w') as fh:
        json.dump(rec, fh, indent=1)
print(json.dumps(rec, indent=1))
