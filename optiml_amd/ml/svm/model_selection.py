"""Cross-validated grid search over `SVC` / `OneVsRestSVC`: the result of sklearn's
`GridSearchCV(estimator, param_grid, cv=cv, refit=refit)` with accuracy scoring, with every fold's fits solved together on ONE Gram
panel of all n rows.

Two facts make a search one batched solve.  The training-fold dual is the full-data dual with ub = 0 on the held-out rows: those
entries start at 0 (mid-box) and never move, so every sum of the iteration is the training fold's (bq_msolver.hip).  And C is only
the box: Q = diag(y)(K + 1)diag(y) and q = -1 do not depend on it.  So every (fold, C, class) triple is one column of
`bq_msolver_create_boxes` on one panel, and its held-out decision values and intercept come from one wide product
(`bq_problem_gram_matmat_wide`): rows of K w at the held-out points, plus the intercept.

The batched path applies when the estimator is on `OneVsRestSVC`'s batched path (`uses_batched_path`) and the grid varies only `C`
and `kernel`.  Candidates are grouped by resolved kernel: a numeric gamma (or a linear kernel) shares one panel across folds, a
string gamma is resolved on each fold's training rows as `SVC.fit` would, which gives one panel per fold.  Panels are built one at a
time.  Every other configuration runs exactly GridSearchCV's calls: `estimator.set_params(**p).fit(X[tr], y[tr]).score(X[te],
y[te])` per candidate and fold.
"""
import copy
import itertools

import numpy as np

from ... import _lib
from ...device import get_context
from ...opti import KernelQuadratic
from ._base import SVC
from ._batched import MEMORY_SHARE, _gram_matmat, column_bytes, device_free_bytes, intercept, solve_batched, solver_kind
from .kernels import BaseEstimator, LinearKernel
from .multiclass import OneVsRestSVC, uses_batched_path, binarize
from .onevsone import OneVsOneSVC

__all__ = ['SVCGridSearchCV', 'parameter_grid', 'check_cv_splits', 'plan_columns', 'aggregate_scores', 'uses_batched_search']

BATCHED_KEYS = frozenset({'C', 'kernel'})
MAX_COLUMNS = 4096   # columns per batched solve at most (see _column_cap)


def parameter_grid(param_grid):
    """The candidates of sklearn's ParameterGrid, in its order: per dict, keys sorted, the product of their values."""
    grids = [param_grid] if isinstance(param_grid, dict) else list(param_grid)
    out = []
    for g in grids:
        items = sorted(g.items())
        if not items:
            out.append({})
            continue
        keys, values = zip(*items)
        for v in itertools.product(*values):
            out.append(dict(zip(keys, v)))
    return out


def check_cv_splits(cv, X, y):
    """(train, test) index arrays: an int is StratifiedKFold(cv) without shuffling (what GridSearchCV gives a classifier), an object
    with `split` is called as split(X, y), anything else is an iterable of (train, test) pairs."""
    if isinstance(cv, (int, np.integer)) and not isinstance(cv, bool):
        from sklearn.model_selection import StratifiedKFold
        cv = StratifiedKFold(n_splits=int(cv))
    it = cv.split(X, y) if hasattr(cv, 'split') else cv
    splits = [(np.asarray(tr, dtype=np.intp), np.asarray(te, dtype=np.intp)) for tr, te in it]
    if not splits:
        raise ValueError('cv yields no splits')
    return splits


def _base_params(estimator):
    return {name: getattr(estimator, name) for name in estimator._kw} if isinstance(estimator, (OneVsRestSVC, OneVsOneSVC)) else \
        dict(estimator.get_params(deep=False))


def _make(estimator_type, base, params):
    kw = dict(base)
    kw.update(params)
    return estimator_type(**kw)


def _prototype(est):
    return est._prototype() if isinstance(est, OneVsRestSVC) else est


def uses_batched_search(estimator, candidates, world):
    """True when `SVCGridSearchCV` solves every (candidate, fold, class) on shared panels: the estimator (an `SVC` or an
    `OneVsRestSVC`) is on `OneVsRestSVC`'s batched path and the grid varies only C and kernel."""
    if not isinstance(estimator, (SVC, OneVsRestSVC)):
        return False
    if any(not set(p) <= BATCHED_KEYS for p in candidates):
        return False
    return uses_batched_path(_prototype(estimator), world)


def _resolved_kernel(kernel, Xfit):
    """The kernel as SVC.fit on Xfit builds its panel: a string gamma resolved on Xfit into a numeric one."""
    gamma = getattr(kernel, 'gamma', None)
    if not isinstance(gamma, str):
        return kernel
    k = copy.copy(kernel)
    k.gamma = kernel.device_spec(np.ascontiguousarray(Xfit, dtype=float))[1]
    return k


def _kernel_key(kernel):
    return (type(kernel).__name__,) + tuple(kernel.device_spec(np.zeros((1, 1)))) if not isinstance(kernel, LinearKernel) else \
        ('LinearKernel',)


def _fold_labels(y_train, multiclass):
    """(classes_, rows): the labels SVC.fit (binary: the larger label is +1) or OneVsRestSVC (binarize) gives the fold's classes."""
    if multiclass:
        classes, _ = binarize(y_train)
        rows = classes[1:] if len(classes) == 2 else classes
        return classes, list(rows)
    classes = np.unique(y_train)
    if len(classes) > 2:
        raise ValueError('use OneVsOneClassifier or OneVsRestClassifier from sklearn.multiclass '
                         'to train a model over more than two labels')
    return classes, [classes[-1]]


def plan_columns(X, y, splits, candidates, base_C, base_kernel, multiclass):
    """The batched search's panels and columns.  Returns (groups, folds): folds[f] = (classes_, positive labels per class row);
    groups: a list of dicts {kernel: the resolved kernel of the panel, cols: [(candidate, fold, class row, C)], Y: m x n labels +-1,
    UB: m x n boxes} — one group per resolved kernel (a string gamma resolves on every fold's training rows)."""
    X = np.ascontiguousarray(X, dtype=float)
    y = np.asarray(y)
    n = len(y)
    folds = [_fold_labels(y[tr], multiclass) for tr, _ in splits]
    groups, index = [], {}
    for ci, p in enumerate(candidates):
        C = p.get('C', base_C)
        kernel = p.get('kernel', base_kernel)
        for f, (tr, _) in enumerate(splits):
            rk = _resolved_kernel(kernel, X[tr])
            key = _kernel_key(rk)
            if key not in index:
                index[key] = len(groups)
                groups.append(dict(kernel=rk, cols=[], Y=[], UB=[]))
            g = groups[index[key]]
            ub = np.zeros(n)
            ub[tr] = C
            for r, pos in enumerate(folds[f][1]):
                g['cols'].append((ci, f, r, C))
                g['Y'].append(np.where(y == pos, 1., -1.))
                g['UB'].append(ub)
    for g in groups:
        g['Y'] = np.stack(g['Y'])
        g['UB'] = np.stack(g['UB'])
    return groups, folds


def aggregate_scores(candidates, scores):
    """cv_results_ as GridSearchCV builds it from test scores (candidates x splits): params, param_<key> (masked where a candidate
    has no such key), split<i>_test_score, mean / std (population) and rank ('min' method; nan ranks last)."""
    scores = np.asarray(scores, dtype=float)
    nc, ns = scores.shape
    res = {'params': list(candidates)}
    keys = sorted({k for p in candidates for k in p})
    for k in keys:
        col = np.ma.MaskedArray(np.empty(nc, dtype=object), mask=True)
        for i, p in enumerate(candidates):
            if k in p:
                col[i] = p[k]
        res['param_' + k] = col
    for i in range(ns):
        res['split%d_test_score' % i] = scores[:, i]
    means = np.average(scores, axis=1)
    stds = np.sqrt(np.average((scores - means[:, np.newaxis]) ** 2, axis=1))
    res['mean_test_score'] = means
    res['std_test_score'] = stds
    if np.isnan(means).all():
        rank = np.ones(nc, dtype=np.int32)
    else:
        m = np.nan_to_num(means, nan=np.nanmin(means) - 1)
        rank = np.array([1 + int(np.sum(m > v)) for v in m], dtype=np.int32)   # scipy rankdata(-m, 'min')
    res['rank_test_score'] = rank
    return res


def column_cap(n, free_bytes, slab_bytes):
    """Columns one batched solve may take with `free_bytes` of device memory free after the panel: MEMORY_SHARE of it, less the
    solver's 16-column slab (`slab_bytes`), over the device state of a column (`column_bytes`); at most MAX_COLUMNS, at least 16.
    Larger grids run in several solves; the split does not change any column's bits (the product is batch-invariant)."""
    budget = int(free_bytes * MEMORY_SHARE) - int(slab_bytes)
    return int(max(16, min(MAX_COLUMNS, budget // column_bytes(n))))


class SVCGridSearchCV(BaseEstimator):
    """Exhaustive search over `param_grid` for an `SVC` or `OneVsRestSVC` scored by accuracy, as sklearn's GridSearchCV.  A
    `OneVsOneSVC` runs GridSearchCV's per-fold calls, each fold's fit one batched one-vs-one solve.

    After `fit`: `cv_results_` (params, param_<key>, split<i>_test_score, mean / std / rank_test_score — no timing keys: the
    candidates' fits are one batched solve and have no fit time of their own), `best_index_` (first among ties), `best_params_`,
    `best_score_`, `n_splits_`, `best_estimator_` (a plain `fit` on all the data, refit=True), and per column `n_iter_` / `status_`
    of shape (candidates, splits, classes) (-1 / '' where a fit has no such record).  `batched_` says which path ran.
    `predict`, `decision_function` and `score` are the best estimator's.
    """

    def __init__(self, estimator, param_grid, scoring=None, cv=5, refit=True):
        self.estimator = estimator
        self.param_grid = param_grid
        self.scoring = scoring
        self.cv = cv
        self.refit = refit

    def fit(self, X, y):
        if self.scoring is not None:
            raise NotImplementedError('only accuracy scoring (scoring=None) is implemented')
        if not isinstance(self.estimator, (SVC, OneVsRestSVC, OneVsOneSVC)):
            raise TypeError('estimator must be an SVC, a OneVsRestSVC or a OneVsOneSVC')
        X = np.ascontiguousarray(X, dtype=float)
        y = np.asarray(y)
        candidates = parameter_grid(self.param_grid)
        splits = check_cv_splits(self.cv, X, y)
        etype, base = type(self.estimator), _base_params(self.estimator)
        protos = [_make(etype, base, p) for p in candidates]   # the estimator's own checks on every candidate
        self.batched_ = uses_batched_search(protos[0], candidates, get_context().world)
        if self.batched_:
            scores, n_iter, status = self._fit_batched(X, y, splits, candidates, protos[0])
        else:
            scores, n_iter, status = self._fit_fallback(X, y, splits, candidates, etype, base)
        self.n_splits_ = len(splits)
        self.cv_results_ = aggregate_scores(candidates, scores)
        self.n_iter_, self.status_ = n_iter, status
        self.best_index_ = int(self.cv_results_['rank_test_score'].argmin())
        self.best_params_ = candidates[self.best_index_]
        self.best_score_ = float(self.cv_results_['mean_test_score'][self.best_index_])
        if self.refit:
            self.best_estimator_ = _make(etype, base, self.best_params_).fit(X, y)
        return self

    def _fit_fallback(self, X, y, splits, candidates, etype, base):
        nc, ns = len(candidates), len(splits)
        scores = np.empty((nc, ns))
        recs = [[None] * ns for _ in range(nc)]
        for ci, p in enumerate(candidates):
            for f, (tr, te) in enumerate(splits):
                est = _make(etype, base, {}).set_params(**p).fit(X[tr], y[tr])
                scores[ci, f] = est.score(X[te], y[te])
                fits = est.estimators_ if isinstance(est, (OneVsRestSVC, OneVsOneSVC)) else [est]
                recs[ci][f] = [(int(getattr(e.optimizer, 'iter', -1)), str(getattr(e.optimizer, 'status', ''))) for e in fits]
        width = max(len(r) for row in recs for r in row)
        n_iter = np.full((nc, ns, width), -1, dtype=np.int64)
        status = np.full((nc, ns, width), '', dtype=object)
        for ci in range(nc):
            for f in range(ns):
                for c, (it, st) in enumerate(recs[ci][f]):
                    n_iter[ci, f, c], status[ci, f, c] = it, st
        return scores, n_iter, status

    def _fit_batched(self, X, y, splits, candidates, proto_est):
        multiclass = isinstance(proto_est, OneVsRestSVC)
        proto = _prototype(proto_est)
        n = len(y)
        nc, ns = len(candidates), len(splits)
        groups, folds = plan_columns(X, y, splits, candidates, proto.C, proto.kernel, multiclass)
        width = max(len(rows) for _, rows in folds)
        n_iter = np.full((nc, ns, width), -1, dtype=np.int64)
        status = np.full((nc, ns, width), '', dtype=object)
        dec = [[[None] * len(folds[f][1]) for f in range(ns)] for _ in range(nc)]   # held-out decision values per column
        kind = solver_kind(proto.optimizer)
        for g in groups:   # one panel at a time
            m = len(g['cols'])
            obj = KernelQuadratic(X, -np.ones(n), 'svc', g['kernel'], y=g['Y'][0], storage=proto.storage,
                                  tune_placement=proto._streams_panel(), expected_products=proto.max_iter * ((m + 15) // 16))
            dev = obj.device_problem()
            cap = column_cap(n, device_free_bytes(), _lib.load().bq_problem_wide_slab_bytes(dev.handle))
            for c0 in range(0, m, cap):
                cols = g['cols'][c0:c0 + cap]
                Y, UB = g['Y'][c0:c0 + cap], g['UB'][c0:c0 + cap]
                res = solve_batched(dev, kind, Y, UB, eps=1e-6, max_iter=proto.max_iter)
                W = np.zeros((len(cols), n))
                svs = []
                for j, r in enumerate(res):
                    sv = r['x'] > 1e-6
                    W[j][sv] = r['x'][sv] * Y[j][sv]
                    svs.append(sv)
                U = _gram_matmat(dev, W, wide=True)
                for j, (ci, f, row, C) in enumerate(cols):
                    sv = svs[j]
                    b = intercept(Y[j], U[j], sv)
                    n_iter[ci, f, row], status[ci, f, row] = res[j]['iter'], res[j]['status']
                    te = splits[f][1]
                    kernel = candidates[ci].get('kernel', proto.kernel)
                    if proto.storage == 'f64' and not isinstance(getattr(kernel, 'gamma', None), str):
                        dec[ci][f][row] = U[j][te] + b   # the fp64 panel holds the decision kernel's values
                    else:
                        # decision_function resolves a string gamma on the support vectors and evaluates the kernel in fp64,
                        # not from an fp32 panel: score through the fold's SVC
                        est = copy.copy(proto)
                        est.kernel, est.C = kernel, C
                        est.support_vectors_ = X[sv]
                        est.dual_coef_ = W[j][sv]
                        if isinstance(kernel, LinearKernel):
                            est.coef_ = np.dot(est.dual_coef_, est.support_vectors_)
                        est.intercept_ = b
                        dec[ci][f][row] = est.decision_function(X[te])
            del dev, obj
        self._cv_decisions = dec
        scores = np.empty((nc, ns))
        for ci in range(nc):
            for f, (_, te) in enumerate(splits):
                classes = folds[f][0]
                D = dec[ci][f]
                if len(D) == 1:
                    pred = np.where(D[0] > 0, classes[-1], classes[0])
                else:
                    pred = classes[np.argmax(np.stack(D, axis=1), axis=1)]
                scores[ci, f] = float(np.mean(pred == y[te]))
        return scores, n_iter, status

    def decision_function(self, X):
        return self.best_estimator_.decision_function(X)

    def predict(self, X):
        return self.best_estimator_.predict(X)

    def score(self, X, y):
        return self.best_estimator_.score(X, y)
