"""tools/calibration_probe.py loop|batched [max_iter] [fits]: Platt calibration of a 3-class one-vs-rest SVC at n = 20 000, d = 64,
5 stratified folds, the hinge dual with the regularised intercept by ProjectedGradient, RBF (gamma = 1 / d), fp64, a fixed max_iter
(default 200), ensemble=True.  loop: the calls sklearn's CalibratedClassifierCV makes, written out on the same build — per fold
OneVsRestSVC.fit on the training rows and decision_function on the held-out rows, then the sigmoids through bq_platt_fit; batched:
CalibratedSVC.fit (every (fold, class) one column on one panel, bq_msolver_svc_heldout).  One JSON line: seconds of `fits` warmed
fits, host clock around the fit (it ends in a synchronising copy), and the sigmoids the last fit ended with
(profiles/calibration/fit_timings.json)."""
import json
import os
import sys
import time
import warnings

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from optiml_amd.datasets import make_multiclass_blobs
from optiml_amd.ml.svm import CalibratedSVC, OneVsRestSVC
from optiml_amd.ml.svm._batched import platt_fit
from optiml_amd.ml.svm.kernels import GaussianKernel
from optiml_amd.ml.svm.losses import hinge
from optiml_amd.ml.svm.model_selection import check_cv_splits
from optiml_amd.opti.constrained import ProjectedGradient

mode = sys.argv[1]
max_iter = int(sys.argv[2]) if len(sys.argv) > 2 else 200
fits = int(sys.argv[3]) if len(sys.argv) > 3 else 3
n, d, k, folds = 20000, 64, 3, 5
X, y = make_multiclass_blobs(n, d, k, seed=1)
kw = dict(loss=hinge, kernel=GaussianKernel(gamma=1. / d), C=1.0, reg_intercept=True, dual=True, optimizer=ProjectedGradient,
          max_iter=max_iter)
warnings.simplefilter('ignore')
CalibratedSVC(OneVsRestSVC(**dict(kw, max_iter=2)), cv=folds).fit(X[:2048], y[:2048])   # context, library, allocator warm-up
classes = np.unique(y)
times = []
for rep in range(fits):
    t0 = time.perf_counter()
    if mode == 'loop':
        splits = check_cv_splits(folds, X, y)
        D, L = np.zeros((folds * k, n)), np.zeros((folds * k, n))
        ests = []
        for f, (tr, te) in enumerate(splits):
            est = OneVsRestSVC(**kw).fit(X[tr], y[tr])
            D[f * k:(f + 1) * k, te] = est.decision_function(X[te]).T
            L[f * k:(f + 1) * k, te] = np.where(y[te][None, :] == classes[:, None], 1., -1.)
            ests.append(est)
        cal = platt_fit(D, L)
        batched = all(e.batched_ for e in ests)
    else:
        est = CalibratedSVC(OneVsRestSVC(**kw), cv=folds).fit(X, y)
        assert est.batched_ and est.batched_decision_
        cal = {key: est.calibrators_[key].ravel() for key in ('A', 'B', 'iters', 'flags')}
        batched = True
    times.append(time.perf_counter() - t0)
print(json.dumps(dict(mode=mode, n=n, d=d, k=k, folds=folds, max_iter=max_iter, fit_s=times, fold_fits_batched=bool(batched),
                      A=[float(a) for a in cal['A']], B=[float(b) for b in cal['B']], iters=[int(i) for i in cal['iters']],
                      flags=[int(i) for i in cal['flags']])))
