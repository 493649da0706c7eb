"""tools/nu_search_probe.py [n] [d]: what the nu-searches cost at size (profiles/nu_search/).  One JSON line.

scoring   n = 20 000, d = 128, RBF (gamma = 1 / d), fp64 panel built once, 48 columns (16 nu x 3 interleaved folds held out by a
          zero box), tol = 0, for each of the two layouts (LABELS: NuSVC columns; PAIRED: NuSVR columns): a fresh solver, 5 warm-up
          iterations, then 3 rounds of (20 iterations by the host clock around bq_msolver_run, 7 bq_msolver_simplex2_heldout calls
          by the host clock around each, after 2 untimed ones).  Both end in a synchronising copy.  Per layout the iteration's median
          over the rounds, the call's median over all 21 calls, their spreads and the ratio.
search    the same rows: NuSVCGridSearchCV over 4 nu x StratifiedKFold(3) (12 fits as columns of one solve on one panel) against the
          same 12 fits through sklearn's GridSearchCV(NuSVC) (one panel of the fold's rows and one solve per fit), tol 1e-3,
          max_iter 200, refit=False, wall clock; one untimed search of each first, then 3 alternated rounds; medians, spreads, the
          ratio, and the largest difference of the 12 split scores."""
import json
import os
import sys
import time
import warnings

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

n = int(sys.argv[1]) if len(sys.argv) > 1 else 20000
d = int(sys.argv[2]) if len(sys.argv) > 2 else 128
rs = np.random.RandomState(0)
# tools/bench_nu.py's rows: 8 latent Gaussian dimensions embedded isometrically in d; labels and targets from the latent rows
Z = rs.standard_normal((n, 8))
Z[::20] *= 3
X = Z @ (np.linalg.qr(rs.standard_normal((d, 8)))[0].T * np.sqrt(d))
y = np.where(Z[:, 0] + 0.5 * Z[:, 1] ** 2 + 0.6 * rs.standard_normal(n) > 0.4, 1., -1.)
t = np.sin(Z[:, 0]) + 0.5 * Z[:, 1] + 0.2 * rs.standard_normal(n)
warnings.simplefilter('ignore')

from sklearn.model_selection import GridSearchCV, StratifiedKFold   # noqa: E402

from optiml_amd.ml.svm import NuSVC, NuSVCGridSearchCV   # noqa: E402
from optiml_amd.ml.svm._batched import _DeviceSimplex2Solver   # noqa: E402
from optiml_amd.ml.svm.kernels import GaussianKernel   # noqa: E402
from optiml_amd.opti import KernelQuadratic   # noqa: E402

kernel = GaussianKernel(gamma=1.0 / d)
NuSVC(kernel=kernel, nu=0.5, max_iter=3).fit(X[:2048], y[:2048])   # context, library, allocator warm-up
out = dict(n=n, d=d)

# ---- scoring against an iteration --------------------------------------------------------------------------------------------------
k, warm, steps, rounds, calls = 48, 5, 20, 3, 7
nus = np.linspace(0.05, 0.6, k // 3).repeat(3)
mask = np.ones((k, n))
for c in range(k):
    mask[c, np.arange(n) % 3 == c % 3] = 0.
n_train = mask.sum(axis=1)
quad = KernelQuadratic(X, np.zeros(n), 'plain', kernel, tune_placement=True, expected_products=2 * 3 * (warm + rounds * steps))
dev = quad.device_problem()
for layout in ('labels', 'paired'):
    mass = np.repeat((nus * n_train / 2)[:, None], 2, axis=1)
    if layout == 'labels':
        solver, target = _DeviceSimplex2Solver(dev, np.tile(y, (k, 1)), mask, mass, None, 0.0, 10 ** 6), y
    else:
        solver = _DeviceSimplex2Solver(dev, None, np.hstack((mask, mask)), mass, np.tile(np.concatenate((-t, t)), (k, 1)), 0.0, 10 ** 6)
        target = t
    solver.run(warm)
    it_ms, call_ms = [], []
    for _ in range(rounds):
        t0 = time.perf_counter()
        _, status = solver.run(steps)
        it_ms.append(1e3 * (time.perf_counter() - t0) / steps)
        for j in range(2 + calls):
            t0 = time.perf_counter()
            held = solver.heldout(target)
            if j >= 2:
                call_ms.append(1e3 * (time.perf_counter() - t0))
    solver.close()
    out['scoring_' + layout] = dict(columns=k, iteration_ms=it_ms, iteration_median_ms=float(np.median(it_ms)),
                                    iteration_spread_ms=max(it_ms) - min(it_ms), heldout_ms=call_ms,
                                    heldout_median_ms=float(np.median(call_ms)), heldout_spread_ms=max(call_ms) - min(call_ms),
                                    heldout_over_iteration=float(np.median(call_ms) / np.median(it_ms)),
                                    live_at_the_end=int(sum(s == 'unknown' for s in status)), n_held=[int(v) for v in held[4][:3]])
quad.release()
del dev, quad

# ---- the search against the per-fit calls -------------------------------------------------------------------------------------------
grid = {'nu': [0.2, 0.3, 0.4, 0.5]}
kw = dict(kernel=kernel, tol=1e-3, max_iter=200)


def batched():
    return NuSVCGridSearchCV(NuSVC(**kw), grid, cv=3, refit=False).fit(X, y)


def per_fit():
    return GridSearchCV(NuSVC(**kw), grid, cv=StratifiedKFold(3), refit=False).fit(X, y)


a, b = batched(), per_fit()   # untimed
diff = max(float(np.abs(a.cv_results_['split%d_test_score' % i] - b.cv_results_['split%d_test_score' % i]).max()) for i in range(3))
times = dict(batched=[], per_fit=[])
for _ in range(3):
    for name, fn in (('batched', batched), ('per_fit', per_fit)):
        t0 = time.perf_counter()
        fn()
        times[name].append(time.perf_counter() - t0)
out['search'] = dict(grid=grid, folds=3, tol=kw['tol'], max_iter=kw['max_iter'], batched_path=bool(a.batched_),
                     n_iter=a.n_iter_.tolist(), status=a.status_.tolist(), mean_test_score=a.cv_results_['mean_test_score'].tolist(),
                     max_split_score_difference=diff, batched_s=times['batched'], per_fit_s=times['per_fit'],
                     batched_median_s=float(np.median(times['batched'])), per_fit_median_s=float(np.median(times['per_fit'])),
                     batched_spread_s=max(times['batched']) - min(times['batched']),
                     per_fit_spread_s=max(times['per_fit']) - min(times['per_fit']),
                     per_fit_over_batched=float(np.median(times['per_fit']) / np.median(times['batched'])))
print(json.dumps(out))
