"""The held-out scorers of the batched SMO walkers measured (`python tools/smo_heldout_probe.py [N D CLASSES [OUT.json]]`, default
20000 32 10).

(a) `SVRGridSearchCV(SVR(optimizer='smo', reg_intercept=False))`, RBF gamma = 1/D, tol 1e-3, 3 folds x (4 C x 3 epsilon) = 36
    columns, refit off: the batched search (`batch_smo = True`: one panel, one `bq_msmo` solve of row-list columns, scored by
    `bq_msmo_svr_heldout`) against the same commit forced to its per-fold calls (`batch_smo = False`: per candidate and fold
    `SVR.fit` on X[tr] and `score`, the path every earlier commit takes), and the scoring call's share of the batched search.
(b) `CalibratedSVC(OneVsRestSVC(optimizer='smo'), ensemble=True)`, CLASSES classes, 3 folds = 3 x CLASSES columns: `batch_smo = True`
    (one panel, one solve, `bq_msmo_svc_heldout`) against `batch_smo = False` (per fold `OneVsRestSVC.fit` — with its default
    dispatch over the classes — and `decision_function`, the sigmoids through `bq_platt_fit`), and the scoring call's share.
Host clock around calls that end in a device synchronise; three passes in one process, the two versions alternating, every pass
recorded; the first warms code objects, the other two give the figure and its spread.  Prints one JSON record
(profiles/smo_heldout/)."""
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np

from optiml_amd.datasets import make_multiclass_blobs, make_regression
from optiml_amd.ml.svm import SVR, CalibratedSVC, OneVsRestSVC, SVRGridSearchCV
from optiml_amd.ml.svm import _batched
from optiml_amd.ml.svm.kernels import GaussianKernel
from optiml_amd.ml.svm.losses import epsilon_insensitive, hinge

n, d, classes = (int(a) for a in (sys.argv[1:4] if len(sys.argv) > 3 else (20000, 32, 10)))
PASSES = 3
Xr, _ = make_regression(n, d, seed=1)
rs = np.random.RandomState(7)
yr = np.tanh(Xr @ rs.standard_normal(d) / np.sqrt(d) / 4) + 0.1 * rs.standard_normal(n)
Xc, yc = make_multiclass_blobs(n, d, classes, seed=1)
kernel = GaussianKernel(gamma=1.0 / d)
svr_kw = dict(loss=epsilon_insensitive, kernel=kernel, C=1., epsilon=0.1, dual=True, optimizer='smo', tol=1e-3, reg_intercept=False)
svc_kw = dict(loss=hinge, kernel=kernel, C=1., dual=True, optimizer='smo', tol=1e-3, reg_intercept=False)
grid = {'C': [0.25, 1., 4., 16.], 'epsilon': [0.05, 0.1, 0.2]}
idx = np.arange(n)
folds = [(np.setdiff1d(idx, idx[f::3]), idx[f::3]) for f in range(3)]
rec = dict(n=n, d=d, classes=classes, tol=1e-3, grid=grid, folds=3, search_columns=36, calibration_columns=3 * classes,
           default_batch_smo_search=bool(_batched.takes_batched_smo(36, SVRGridSearchCV.batch_smo)),
           default_batch_smo_calibration=bool(_batched.takes_batched_smo(3 * classes, CalibratedSVC.batch_smo)))


def clock(fn):
    t0 = time.perf_counter()
    out = fn()
    return time.perf_counter() - t0, out


score_s = []


def _timed(name):
    call = getattr(_batched._DeviceSMOSolver, name)

    def timed(self, *args, **kwargs):
        t, out = clock(lambda: call(self, *args, **kwargs))
        score_s.append(t)
        return out

    setattr(_batched._DeviceSMOSolver, name, timed)


_timed('svr_heldout')
_timed('svc_heldout')

for rep in range(PASSES):
    runs = {}
    for name, force in (('batched', True), ('per_fold', False)):
        search = SVRGridSearchCV(SVR(**svr_kw), grid, cv=folds, refit=False)
        search.batch_smo = force
        del score_s[:]
        t, _ = clock(lambda: search.fit(Xr, yr))
        runs[name] = (t, search, sum(score_s), len(score_s))
    (tb, sb, ts, ns), (tp, sp, _, _) = runs['batched'], runs['per_fold']
    scores = lambda s: np.array([s.cv_results_['split%d_test_score' % f] for f in range(3)]).T   # noqa: E731
    rec['search_pass%d' % rep] = dict(batched_search_s=tb, per_fold_search_s=tp, smo_=bool(sb.smo_), columns=int(sb.n_iter_.size),
                                      scoring_s=ts, scoring_calls=ns, scoring_share=ts / tb, batched_scores=scores(sb).tolist(),
                                      per_fold_scores=scores(sp).tolist(),
                                      largest_score_difference=float(np.abs(scores(sb) - scores(sp)).max()),
                                      same_best=bool(sb.best_index_ == sp.best_index_),
                                      outer_iterations=[int(sb.n_iter_.min()), int(sb.n_iter_.max())],
                                      outer_iterations_per_fold=[int(sp.n_iter_.min()), int(sp.n_iter_.max())])
    print('pass %d: SVR search batched %.3f s (scoring %.3f s in %d calls), per fold %.3f s, largest score difference %.3e' %
          (rep, tb, ts, ns, tp, rec['search_pass%d' % rep]['largest_score_difference']), flush=True)

Xnew = Xc[::50] + 0.01
for rep in range(PASSES):
    runs = {}
    for name, force in (('batched', True), ('per_fold', False)):
        est = CalibratedSVC(OneVsRestSVC(**svc_kw), cv=folds, ensemble=True)
        est.batch_smo = force
        del score_s[:]
        t, _ = clock(lambda: est.fit(Xc, yc))
        runs[name] = (t, est, sum(score_s), len(score_s))
    (tb, eb, ts, ns), (tp, ep, _, _) = runs['batched'], runs['per_fold']
    P, Q = eb.predict_proba(Xnew), ep.predict_proba(Xnew)
    rec['calibration_pass%d' % rep] = dict(batched_fit_s=tb, per_fold_fit_s=tp, smo_=bool(eb.smo_), scoring_s=ts, scoring_calls=ns,
                                           scoring_share=ts / tb, largest_probability_difference=float(np.abs(P - Q).max()),
                                           predictions_that_differ=int((eb.predict(Xnew) != ep.predict(Xnew)).sum()),
                                           rows_predicted=int(len(Xnew)),
                                           largest_A_difference=float(np.abs(eb.calibrators_['A'] - ep.calibrators_['A']).max()),
                                           largest_B_difference=float(np.abs(eb.calibrators_['B'] - ep.calibrators_['B']).max()))
    print('pass %d: calibration batched %.3f s (scoring %.3f s in %d calls), per fold %.3f s, largest probability difference %.3e' %
          (rep, tb, ts, ns, tp, rec['calibration_pass%d' % rep]['largest_probability_difference']), flush=True)

if len(sys.argv) > 4:
    with open(sys.argv[4], 'w') as fh:
        json.dump(rec, fh, indent=1)
print(json.dumps(rec, indent=1))
