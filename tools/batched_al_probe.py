"""tools/batched_al_probe.py loop|batched [max_iter] [fits]: k = 8 classes at n = 20 000, d = 64, the hinge dual with the unregularised
intercept (equality row) by AdaGrad(1.) on the augmented Lagrangian, fp64, a fixed max_iter (default 200).  loop: k SVC.fit calls one
after another on the 0 / 1 labels (what OneVsRestSVC ran for this configuration before the batched solver); batched: OneVsRestSVC.fit
(bq_msolver_create_al).  One JSON line: seconds of `fits` warmed fits of the whole k-class problem, host clock around the fit (it ends
in a synchronising copy), and what the fits ended with (profiles/batched_al/fit_timings.json)."""
import json
import os
import sys
import time
import warnings

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from optiml_amd.datasets import make_multiclass_blobs
from optiml_amd.ml.svm import SVC, OneVsRestSVC
from optiml_amd.ml.svm.kernels import gaussian
from optiml_amd.ml.svm.losses import hinge
from optiml_amd.ml.svm.multiclass import binarize
from optiml_amd.opti.unconstrained.stochastic import AdaGrad

mode = sys.argv[1]
max_iter = int(sys.argv[2]) if len(sys.argv) > 2 else 200
fits = int(sys.argv[3]) if len(sys.argv) > 3 else 3
n, d, k = 20000, 64, 8
X, y = make_multiclass_blobs(n, d, k, seed=1)
_, Y = binarize(y)
kw = dict(loss=hinge, kernel=gaussian, C=1.0, reg_intercept=False, dual=True, optimizer=AdaGrad, learning_rate=1., max_iter=max_iter,
          random_state=1)
warnings.simplefilter('ignore')   # one ConvergenceWarning per class and fit
SVC(**dict(kw, max_iter=2)).fit(X[:2048], (Y[0, :2048] > 0).astype(int))   # context, library and allocator warm-up outside the timing
times = []
for rep in range(fits):
    t0 = time.perf_counter()
    if mode == 'loop':
        ests = [SVC(**kw).fit(X, (Yc > 0).astype(int)) for Yc in Y]
    else:
        est = OneVsRestSVC(**kw).fit(X, y)
        assert est.batched_ and est.lagrangian_
        ests = est.estimators_
    times.append(time.perf_counter() - t0)
print(json.dumps(dict(mode=mode, n=n, d=d, k=k, max_iter=max_iter, fit_s=times,
                      iters=[int(e.optimizer.iter) for e in ests], status=[e.optimizer.status for e in ests],
                      loss_last=[float(e.train_loss_history[-1]) for e in ests],
                      intercept=[float(e.intercept_) for e in ests])))
