#!/usr/bin/env python3
"""Every cross-validated search once on its batched path and once on its per-fold path, at small shapes, and a SHA-256 of what a
search leaves: the split scores, mean_test_score, rank_test_score, n_iter_ and status_; in clear, best_index_, batched_ and the
categories and texts of the warnings it raised.  Two checkouts that print the same file run the same searches:

    python3 tools/search_flavours.py > searches.txt

Only public names are used, so the file runs unchanged in an older checkout.  300 rows (360 for the one-vs-one search, three
classes), two kernels per grid, one of them gamma='scale' (the batched one-vs-one search takes no string gamma but 'auto', so its
second kernel is gamma='auto'), two or three folds.  A key outside a search's batched keys (max_iter; tol for the nu-searches) sends
the same grid down the per-fold path.  nu = 0.9517 is infeasible on the NuSVC data, so the failed-fit branch runs on both paths.
"""
import hashlib
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from optiml_amd.datasets import make_multiclass_blobs  # noqa: E402
from optiml_amd.ml.svm import (SVC, SVR, NuSVC, NuSVCGridSearchCV, NuSVR, NuSVRGridSearchCV, OneVsOneGridSearchCV,  # noqa: E402
                               OneVsOneSVC, OneVsRestSVC, SVCGridSearchCV, SVRGridSearchCV)
from optiml_amd.ml.svm.kernels import GaussianKernel  # noqa: E402
from optiml_amd.ml.svm.losses import epsilon_insensitive, hinge  # noqa: E402
from optiml_amd.opti.constrained import ProjectedGradient  # noqa: E402


def sha(a):
    a = np.asarray(a)
    if a.dtype == object:
        return hashlib.sha256('\x00'.join(str(v) for v in a.ravel()).encode() + str(a.shape).encode()).hexdigest()
    return hashlib.sha256(np.ascontiguousarray(a).tobytes() + str(a.shape).encode()).hexdigest()


def run(name, search, X, y, want_batched):
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter('always')
        try:
            search.fit(X, y)
        except ValueError as e:
            print('%-24s %-18s %s' % (name, 'ValueError', e))
            return
    assert bool(search.batched_) is want_batched, (name, search.batched_)
    res = search.cv_results_
    splits = np.stack([res['split%d_test_score' % i] for i in range(search.n_splits_)])
    for key, value in (('split_scores', splits), ('mean_test_score', res['mean_test_score']),
                       ('rank_test_score', res['rank_test_score']), ('n_iter_', search.n_iter_), ('status_', search.status_)):
        print('%-24s %-18s %s' % (name, key, sha(value)))
    print('%-24s %-18s %s' % (name, 'nan_scores', int(np.isnan(splits).sum())))
    print('%-24s %-18s %s' % (name, 'best_index_', search.best_index_))
    print('%-24s %-18s %s' % (name, 'batched_', bool(search.batched_)))
    for w in caught:
        print('%-24s %-18s %s: %s' % (name, 'warning', w.category.__name__, w.message))


def both(name, make, grid, off_key, X, y):
    """the grid on the batched path, and with a one-valued key outside the batched keys on the per-fold path"""
    run(name + '.batched', make(grid), X, y, True)
    run(name + '.per_fold', make(dict(grid, **off_key)), X, y, False)


if __name__ == '__main__':
    rs = np.random.RandomState(5)
    n = 300
    X = rs.standard_normal((n, 3))
    y = np.where(X[:, 0] + 0.5 * X[:, 1] ** 2 + 0.6 * rs.standard_normal(n) > 0.4, 1., -1.)
    t = np.sin(X[:, 0]) + 0.5 * X[:, 1] + 0.2 * rs.standard_normal(n)
    kernels = [GaussianKernel(gamma=0.3), GaussianKernel(gamma='scale')]
    svc = dict(loss=hinge, dual=True, reg_intercept=True, optimizer=ProjectedGradient, max_iter=60)
    svr = dict(loss=epsilon_insensitive, dual=True, reg_intercept=True, optimizer=ProjectedGradient, max_iter=60)
    nu = dict(tol=1e-3, max_iter=60)

    both('svc', lambda g: SVCGridSearchCV(SVC(**svc), g, cv=3), {'C': [0.3, 1.0], 'kernel': kernels}, {'max_iter': [60]}, X, y)
    X3, y3 = make_multiclass_blobs(360, 6, 3, seed=1)
    both('svc_ovr', lambda g: SVCGridSearchCV(OneVsRestSVC(**svc), g, cv=2), {'C': [0.3, 1.0], 'kernel': kernels},
         {'max_iter': [60]}, X3, y3)
    both('svr', lambda g: SVRGridSearchCV(SVR(**svr), g, cv=3), {'C': [0.5, 2], 'epsilon': [0.05, 0.2], 'kernel': kernels},
         {'max_iter': [60]}, X, t)
    both('nu_svc', lambda g: NuSVCGridSearchCV(NuSVC(**nu), g, cv=3), {'nu': [0.3517, 0.5017, 0.9517], 'kernel': kernels},
         {'tol': [1e-3]}, X, y)
    both('nu_svr', lambda g: NuSVRGridSearchCV(NuSVR(**nu), g, cv=2), {'C': [0.5, 1], 'nu': [0.2517, 0.8017], 'kernel': kernels},
         {'tol': [1e-3]}, X, t)
    ovo = dict(svc, kernel=GaussianKernel(gamma=0.5))
    run('ovo.batched', OneVsOneGridSearchCV(OneVsOneSVC(**ovo), {'C': [0.3, 1.0], 'kernel': [GaussianKernel(gamma=0.5),
                                                                                            GaussianKernel(gamma='auto')]}, cv=3),
        X3, y3, True)
    run('ovo.per_fold', OneVsOneGridSearchCV(OneVsOneSVC(**ovo), {'C': [0.3, 1.0], 'kernel': kernels}, cv=3), X3, y3, False)
