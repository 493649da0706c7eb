"""tools/coupling_probe.py loop|batched [max_iter] [fits]: pairwise-coupled probabilities of a 6-class one-vs-one SVC at n = 20 000,
d = 64, 5 stratified folds, the hinge dual with the regularised intercept by ProjectedGradient, RBF (gamma = 1 / d), fp64, a fixed
max_iter (default 200), then predict_proba on 10 000 fresh points.  batched: PairwiseCoupledSVC as it runs (every (pair, fold) one
column on one class-sorted panel, bq_msolver_pairs_heldout; bq_decision_coupled); loop: the same class on the same build with its
batched path switched off — per pair and fold SVC.fit on the pair's training rows and decision_function on its held-out rows, the
sigmoids through bq_platt_fit, OneVsOneSVC.fit on all the data.  One JSON line: seconds of `fits` warmed fits and predictions, host
clock around each call (both end in a synchronising copy), and the sigmoids the last fit ended with
(profiles/coupling/timing.json)."""
import json
import os
import sys
import time
import warnings

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from optiml_amd.datasets import make_multiclass_blobs
from optiml_amd.ml.svm import OneVsOneSVC, PairwiseCoupledSVC
from optiml_amd.ml.svm import coupling
from optiml_amd.ml.svm.kernels import GaussianKernel
from optiml_amd.ml.svm.losses import hinge
from optiml_amd.opti.constrained import ProjectedGradient

mode = sys.argv[1]
max_iter = int(sys.argv[2]) if len(sys.argv) > 2 else 200
fits = int(sys.argv[3]) if len(sys.argv) > 3 else 3
n, d, k, folds, t = 20000, 64, 6, 5, 10000
X, y = make_multiclass_blobs(n + t, d, k, seed=1)
X, y, Xnew = X[:n], y[:n], X[n:]
kw = dict(loss=hinge, kernel=GaussianKernel(gamma=1. / d), C=1.0, reg_intercept=True, dual=True, optimizer=ProjectedGradient,
          max_iter=max_iter)
warnings.simplefilter('ignore')
if mode == 'loop':
    coupling.uses_batched_coupling = lambda estimator, world: False
PairwiseCoupledSVC(OneVsOneSVC(**dict(kw, max_iter=2)), cv=folds).fit(X[:3072], y[:3072]).predict_proba(Xnew[:256])   # warm-up
fit_s, predict_s = [], []
for rep in range(fits):
    t0 = time.perf_counter()
    est = PairwiseCoupledSVC(OneVsOneSVC(**kw), cv=folds).fit(X, y)
    t1 = time.perf_counter()
    P = est.predict_proba(Xnew)
    t2 = time.perf_counter()
    fit_s.append(t1 - t0)
    predict_s.append(t2 - t1)
    assert est.batched_ is (mode == 'batched')
print(json.dumps(dict(mode=mode, n=n, d=d, k=k, folds=folds, points=t, max_iter=max_iter, fit_s=fit_s, predict_proba_s=predict_s,
                      batched_decision=bool(est.batched_decision_),
                      row_sum_error=float(np.abs(P.sum(axis=1) - 1).max()), A=[float(a) for a in est.probA_],
                      B=[float(b) for b in est.probB_], iters=[int(i) for i in est.calibrators_['iters']],
                      flags=[int(i) for i in est.calibrators_['flags']])))
