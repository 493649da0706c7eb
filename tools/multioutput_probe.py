"""tools/multioutput_probe.py seq|batched [max_iter]: k = 8 targets at n = 20 000, d = 64 with bench.py --task svr's C4 kernel and
solver (poly(3, scale, 1), FrankWolfe) and a fixed max_iter.  seq: k SVR.fit calls one after another; batched: MultiOutputSVR.fit.
One JSON line: seconds of three fits of the whole k-target problem (profiles/multioutput/fit_timings.json)."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from optiml_amd.datasets import make_regression
from optiml_amd.ml.svm import SVR, MultiOutputSVR
from optiml_amd.ml.svm.kernels import PolyKernel
from optiml_amd.ml.svm.losses import epsilon_insensitive
from optiml_amd.opti.constrained import FrankWolfe

mode = sys.argv[1]
max_iter = int(sys.argv[2]) if len(sys.argv) > 2 else 200
n, d, k = 20000, 64, 8
X, _ = make_regression(n, d, seed=1)
rs = np.random.RandomState(7)
Y = np.tanh(X @ rs.standard_normal((d, k)) / np.sqrt(d) / 4) + 0.1 * rs.standard_normal((n, k))
kw = dict(loss=epsilon_insensitive, epsilon=0.1, kernel=PolyKernel(3, 'scale', 1.0), C=1.0, reg_intercept=True, dual=True,
          optimizer=FrankWolfe, max_iter=max_iter)
SVR(**dict(kw, max_iter=2)).fit(X[:2048], Y[:2048, 0])   # context, library and allocator warm-up outside the timing
times, hist = [], None
for rep in range(3):
    t0 = time.perf_counter()
    if mode == 'seq':
        ests = [SVR(**kw).fit(X, Y[:, c]) for c in range(k)]
    else:
        est = MultiOutputSVR(**kw).fit(X, Y)
        assert est.batched_
        ests = est.estimators_
    times.append(time.perf_counter() - t0)
print(json.dumps(dict(mode=mode, n=n, d=d, k=k, max_iter=max_iter, fit_s=times,
                      iters=[int(e.optimizer.iter) for e in ests], status=[e.optimizer.status for e in ests],
                      f_last=[float(e.train_loss_history[-1]) for e in ests],
                      intercept=[float(e.intercept_) for e in ests])))
