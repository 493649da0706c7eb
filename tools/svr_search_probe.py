"""tools/svr_search_probe.py batched|fallback|scoring [max_iter] [reps]: SVRGridSearchCV at n = 20 000, d = 128, 5 folds x 3 C x
3 epsilon (45 columns), FrankWolfe, a numeric gamma, refit off.
batched: the search as the class runs it (one panel, 45 columns, held-out scores from the device).
fallback: the same class on its per-(candidate, fold) path — the grid also names `tol` at its default, which changes no fit and takes
the search off the batched path.
scoring: one solve of the 45 columns, then the device scoring (`heldout`) beside the host scoring it replaces: download every
column's x, build W, one wide product, NumPy intercepts and squared errors.
One JSON line (profiles/svr_search/fit_timings.json collects them)."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from optiml_amd import _lib
from optiml_amd.datasets import make_regression
from optiml_amd.ml.svm import SVR, SVRGridSearchCV
from optiml_amd.ml.svm._batched import _DeviceSVRSolver, _gram_matmat, solve_batched, svr_intercept
from optiml_amd.ml.svm.kernels import GaussianKernel
from optiml_amd.ml.svm.losses import epsilon_insensitive
from optiml_amd.ml.svm.model_selection import check_cv_splits, parameter_grid, plan_svr_columns
from optiml_amd.opti import KernelQuadratic
from optiml_amd.opti.constrained import FrankWolfe

mode = sys.argv[1]
max_iter = int(sys.argv[2]) if len(sys.argv) > 2 else 100
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 2
n, d, folds = 20000, 128, 5
X, _ = make_regression(n, d, seed=1)
rs = np.random.RandomState(7)
y = np.tanh(X @ rs.standard_normal(d) / np.sqrt(d) / 4) + 0.1 * rs.standard_normal(n)
kernel = GaussianKernel(gamma=1.0 / d)
kw = dict(loss=epsilon_insensitive, epsilon=0.1, kernel=kernel, C=1.0, reg_intercept=True, dual=True, optimizer=FrankWolfe,
          max_iter=max_iter)
grid = {'C': [0.5, 1.0, 2.0], 'epsilon': [0.05, 0.1, 0.2]}
SVR(**dict(kw, max_iter=2)).fit(X[:2048], y[:2048])   # context, library and allocator warm-up outside the timing
out = dict(mode=mode, n=n, d=d, folds=folds, columns=folds * 9, max_iter=max_iter)

if mode in ('batched', 'fallback'):
    if mode == 'fallback':
        grid = dict(grid, tol=[SVR(**kw).tol])
    times = []
    for rep in range(reps):
        t0 = time.perf_counter()
        search = SVRGridSearchCV(SVR(**kw), grid, cv=folds, refit=False).fit(X, y)
        times.append(time.perf_counter() - t0)
        assert search.batched_ is (mode == 'batched')
    out.update(fit_s=times, mean_test_score=[float(v) for v in search.cv_results_['mean_test_score']],
               best_params={k: v for k, v in search.best_params_.items() if k != 'tol'}, n_iter=int(search.n_iter_.max()))
else:
    g, = plan_svr_columns(X, y, check_cv_splits(folds, X, y, stratified=False), parameter_grid(grid), 1.0, 0.1, kernel)
    eps = np.array([c[3] for c in g['cols']])
    k = len(eps)
    dev = KernelQuadratic(X, g['QL'][0], 'svr', kernel).device_problem()
    t = {}

    def score(solver, _):
        for rep in range(reps):
            t0 = time.perf_counter()
            b, n_sv, sse, n_held = solver.heldout(y, eps)
            t.setdefault('device_s', []).append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            xs = [solver.get(c, _lib.GET_X_NOW) for c in range(k)]
            t1 = time.perf_counter()
            W = np.zeros((k, n))
            svs = []
            for j, x in enumerate(xs):
                xp, xn = np.split(x, 2)
                sv = np.logical_or(xp > 1e-6, xn > 1e-6)
                W[j][sv] = xp[sv] - xn[sv]
                svs.append(sv)
            t2 = time.perf_counter()
            U = _gram_matmat(dev, W, wide=True)
            t3 = time.perf_counter()
            hb = np.array([svr_intercept(y, U[j], svs[j], eps[j]) for j in range(k)])
            hs = np.array([float(((y[te] - (U[j][te] + hb[j])) ** 2).sum())
                           for j in range(k) for te in [(g['UB'][j][:n] == 0)]])
            t4 = time.perf_counter()
            t.setdefault('host_s', []).append(dict(download_x=t1 - t0, build_w=t2 - t1, wide_product=t3 - t2, numpy=t4 - t3,
                                                   total=t4 - t0))
        t['max_abs_intercept_diff'] = float(np.max(np.abs(b - hb)))
        t['max_rel_sse_diff'] = float(np.max(np.abs(sse / hs - 1)))

    solve_batched(dev, _lib.FW, g['QL'], g['UB'], solver=_DeviceSVRSolver(dev, _lib.FW, g['QL'], g['UB'], 1e-6, max_iter),
                  before_close=score, vectors=False)
    out.update(t)
print(json.dumps(out))
