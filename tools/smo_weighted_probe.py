"""The per-row boxes of the SMO walker measured (`python tools/smo_weighted_probe.py [N D CLASSES [OUT.json]]`, default 20000 32 10),
set up as tools/smo_batch_probe.py: `make_multiclass_blobs(N, D, CLASSES, seed=1)`, RBF gamma = 1/D, C = 1, tol 1e-3, fp64 panel.

(a) What the box reads cost: class 0 against the rest on one panel, the unweighted single fit (`bq_smo_create`) against the weighted
    single fit on the constant vector C (`bq_smo_create_weighted`) — the same trajectory, bit for bit, so the time differs by the
    reads of Cw[i] alone — with the helper workgroups (the single solver) and without (one column of `bq_msmo_create` /
    `bq_msmo_create_weighted`).  Five fits each, alternating; the minimum and the median are recorded.
(b) The use case: `OneVsRestSVC(class_weight='balanced', optimizer='smo').fit`, batched (`batch_smo = True`) against the same commit
    forced to one weighted `SVC.fit` per class (`batch_smo = False`).
Host clock around calls that end in a device synchronise; two passes in one process, both recorded, the second is the one to quote.
Prints one JSON record (profiles/smo_weighted/)."""
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np

from optiml_amd import _lib
from optiml_amd.datasets import make_multiclass_blobs
from optiml_amd.ml.svm import OneVsRestSVC
from optiml_amd.ml.svm._batched import solve_batched_smo
from optiml_amd.ml.svm.kernels import GaussianKernel
from optiml_amd.ml.svm.losses import hinge
from optiml_amd.ml.svm.smo import SMOClassifier
from optiml_amd.opti import KernelQuadratic

n, d, classes = (int(a) for a in (sys.argv[1:4] if len(sys.argv) > 3 else (20000, 32, 10)))
X, y = make_multiclass_blobs(n, d, classes, seed=1)
kernel = GaussianKernel(gamma=1.0 / d)
kw = dict(loss=hinge, kernel=kernel, C=1., dual=True, optimizer='smo', tol=1e-3)
rec = dict(n=n, d=d, classes=classes, tol=1e-3, C=1.0)


def clock(fn):
    t0 = time.perf_counter()
    out = fn()
    return time.perf_counter() - t0, out


yb = np.where(y == 0, 1., -1.)
ones = np.ones(n)
for rep in range(2):
    quad = KernelQuadratic(X, -np.ones(n), 'svc', kernel, y=yb, rank_one=False, compact=False)
    dev = quad.device_problem()
    times = dict(single=[], single_rows=[], column=[], column_rows=[])
    for _ in range(5):
        t, one = clock(lambda: SMOClassifier(quad, X, yb, None, kernel, 1., 1e-3).minimize())
        times['single'].append(t)
        t, wone = clock(lambda: SMOClassifier(quad, X, yb, None, kernel, 1., 1e-3, box=ones).minimize())
        times['single_rows'].append(t)
        t, col = clock(lambda: solve_batched_smo(dev, _lib.SVC, yb[None], 1., None, 1e-3)[0])
        times['column'].append(t)
        t, wcol = clock(lambda: solve_batched_smo(dev, _lib.SVC, yb[None], 1., None, 1e-3, boxes=ones[None])[0])
        times['column_rows'].append(t)
    same = bool(np.array_equal(one.alphas, wone.alphas) and np.array_equal(col['alphas'], wcol['alphas']) and
                np.array_equal(one.alphas, col['alphas']) and one.steps == wone.steps == col['steps'] == wcol['steps'])
    r = {k: dict(min_s=min(v), median_s=float(np.median(v)), all_s=v) for k, v in times.items()}
    r.update(same_bits=same, outer_iterations=int(one.iter), pair_steps=int(one.steps), helpers=one.helper_stats['helpers'],
             ratio_with_helpers=float(np.median(times['single_rows']) / np.median(times['single'])),
             ratio_without_helpers=float(np.median(times['column_rows']) / np.median(times['column'])))
    rec['box_reads_pass%d' % rep] = r
    print('pass %d: single %.4f s, with row boxes %.4f s (x %.3f); lone column %.4f s, with row boxes %.4f s (x %.3f); same bits %s' % (
        rep, r['single']['median_s'], r['single_rows']['median_s'], r['ratio_with_helpers'], r['column']['median_s'],
        r['column_rows']['median_s'], r['ratio_without_helpers'], same), flush=True)
    quad.release()

for rep in range(2):
    fits = {}
    for name, force in (('batched', True), ('per_class', False)):
        est = OneVsRestSVC(class_weight='balanced', **kw)
        est.batch_smo = force
        fits[name] = clock(lambda: est.fit(X, y))
    (tb, eb), (tp, ep) = fits['batched'], fits['per_class']
    same = all(np.array_equal(a.alphas_, b.alphas_) and a.intercept_ == b.intercept_ for a, b in zip(eb.estimators_, ep.estimators_))
    rec['ovr_balanced_pass%d' % rep] = dict(batched_fit_s=tb, per_class_fit_s=tp, smo_=bool(eb.smo_), same_bits=bool(same),
                                            outer_iterations=[int(e.optimizer.iter) for e in eb.estimators_],
                                            pair_steps=[int(e.optimizer.steps) for e in eb.estimators_],
                                            n_sv=[int(len(e.support_)) for e in eb.estimators_],
                                            train_accuracy=float(eb.score(X, y)))
    print('pass %d: OneVsRestSVC(class_weight=balanced).fit batched %.3f s, per class %.3f s, same bits %s' % (rep, tb, tp, same),
          flush=True)

if len(sys.argv) > 4:
    with open(sys.argv[4], 'w') as fh:
        json.dump(rec, fh, indent=1)
print(json.dumps(rec, indent=1))
