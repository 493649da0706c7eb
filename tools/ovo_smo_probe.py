"""One-vs-one over the batched SMO walkers measured (`python tools/ovo_smo_probe.py [N D CLASSES [OUT.json]]`, default 20000 32 10).

(a) `OneVsOneSVC(optimizer='smo').fit`, RBF gamma = 1/D, C = 1, tol 1e-3: the pair columns on one panel (`batch_smo = True`) against
    the same commit forced to one `SVC.fit` per pair (`batch_smo = False`, the path every earlier commit takes), and how far the
    two fits' predictions on the training rows agree.
(b) `OneVsOneGridSearchCV` over it, 3 folds x 4 C (x pairs columns), refit=False: the batched search (`batch_smo = True`: one panel,
    the columns run to their end, the vote on the device) against its per-fold path (`batch_smo = False`: per candidate and fold
    `OneVsOneSVC.fit` — with the default dispatch over the pairs — and `score`), and the scoring call's share of the batched search
    (host clock around `vote_heldout`, which ends in a device synchronise).
Host clock around calls that end in a device synchronise; two passes in one process, the two versions alternating, both passes
recorded; the second is the one to quote (the first warms code objects).  Prints one JSON record (profiles/ovo_smo/)."""
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np

from optiml_amd.datasets import make_multiclass_blobs
from optiml_amd.ml.svm import OneVsOneGridSearchCV, OneVsOneSVC
from optiml_amd.ml.svm import _batched
from optiml_amd.ml.svm.kernels import GaussianKernel
from optiml_amd.ml.svm.losses import hinge

n, d, classes = (int(a) for a in (sys.argv[1:4] if len(sys.argv) > 3 else (20000, 32, 10)))
X, y = make_multiclass_blobs(n, d, classes, seed=1)
kw = dict(loss=hinge, kernel=GaussianKernel(gamma=1.0 / d), C=1., dual=True, optimizer='smo', tol=1e-3)
Cs = [0.25, 1., 4., 16.]
idx = np.arange(n)
folds = [(np.setdiff1d(idx, idx[f::3]), idx[f::3]) for f in range(3)]
rec = dict(n=n, d=d, classes=classes, pairs=classes * (classes - 1) // 2, tol=1e-3, C=1.0, search_C=Cs, folds=3,
           default_batch_smo=bool(_batched.takes_batched_smo(classes * (classes - 1) // 2, OneVsOneSVC.batch_smo)))


def clock(fn):
    t0 = time.perf_counter()
    out = fn()
    return time.perf_counter() - t0, out


vote_s = []
_vote = _batched._DeviceSMOSolver.vote_heldout


def _timed_vote(self, *args, **kwargs):
    t, out = clock(lambda: _vote(self, *args, **kwargs))
    vote_s.append(t)
    return out


_batched._DeviceSMOSolver.vote_heldout = _timed_vote

for rep in range(2):
    fits = {}
    for name, force in (('batched', True), ('per_pair', False)):
        est = OneVsOneSVC(**kw)
        est.batch_smo = force
        fits[name] = clock(lambda: est.fit(X, y))
    (tb, eb), (tp, ep) = fits['batched'], fits['per_pair']
    pb, pp = eb.predict(X), ep.predict(X)
    rec['fit_pass%d' % rep] = dict(batched_fit_s=tb, per_pair_fit_s=tp, smo_=bool(eb.smo_),
                                   same_alphas=bool(all(np.array_equal(a.alphas_, b.alphas_) for a, b in
                                                        zip(eb.estimators_, ep.estimators_))),
                                   predictions_that_differ=int((pb != pp).sum()), train_accuracy=float((pb == y).mean()),
                                   outer_iterations=[int(e.optimizer.iter) for e in eb.estimators_],
                                   outer_iterations_per_pair=[int(e.optimizer.iter) for e in ep.estimators_],
                                   n_sv=[int(len(e.support_)) for e in eb.estimators_])
    print('pass %d: OneVsOneSVC.fit batched %.3f s, per pair %.3f s, predictions that differ %d of %d' %
          (rep, tb, tp, int((pb != pp).sum()), n), flush=True)

for rep in range(2):
    runs = {}
    for name, force in (('batched', True), ('per_fold', False)):
        search = OneVsOneGridSearchCV(OneVsOneSVC(**kw), {'C': Cs}, cv=folds, refit=False)
        search.batch_smo = force
        del vote_s[:]
        t, _ = clock(lambda: search.fit(X, y))
        runs[name] = (t, search, sum(vote_s), len(vote_s))
    (tb, sb, tv, nv), (tp, sp, _, _) = runs['batched'], runs['per_fold']
    scores = lambda s: [[float(s.cv_results_['split%d_test_score' % f][c]) for f in range(3)] for c in range(len(Cs))]   # noqa: E731
    rec['search_pass%d' % rep] = dict(batched_search_s=tb, per_fold_search_s=tp, smo_=bool(sb.smo_), columns=int(sb.n_iter_.size),
                                      scoring_s=tv, scoring_calls=nv, scoring_share=tv / tb, batched_scores=scores(sb),
                                      per_fold_scores=scores(sp),
                                      largest_score_difference=float(np.abs(np.array(scores(sb)) - np.array(scores(sp))).max()),
                                      outer_iterations_max=int(sb.n_iter_.max()))
    print('pass %d: search batched %.3f s (scoring %.3f s in %d calls), per fold %.3f s' % (rep, tb, tv, nv, tp), flush=True)

if len(sys.argv) > 4:
    with open(sys.argv[4], 'w') as fh:
        json.dump(rec, fh, indent=1)
print(json.dumps(rec, indent=1))
