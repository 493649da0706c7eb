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

`SVRGridSearchCV` is the same search over `SVR` scored by R^2.  There C is only the box and epsilon only the linear term
[-y; y] + epsilon; the 'svr' panel depends on neither, so every (fold, C, epsilon) of one resolved kernel is one column of
`bq_msolver_create_svr_boxes` (ub = 0 on both halves of the held-out rows), and the columns are scored where the solver's state
lives (`bq_msolver_svr_heldout`): per column an intercept, a support count, a held-out squared error and a held-out count come
back, no k x n array.  Over an SMO estimator (`uses_batched_smo_svr_search`) every (fold, C, epsilon) is one walker column of
`bq_msmo_*` whose row list is the fold's training rows, and `bq_msmo_svr_heldout` scores it from the walkers' state the same way.
"""
import copy
import itertools
import warnings

import numpy as np

from ... import _lib
from ...device import get_context
from ._base import SVC, SVR, has_class_weight
from ._batched import (MAX_COLUMNS, MEMORY_SHARE, _DeviceSMOSolver, _DeviceSVRSolver, _gram_matmat, column_cap,  # noqa: F401
                       device_panel, fitted_svr, intercept, run_batched_smo, smo_column_cap, smo_failed_error,
                       smo_heldout_column_cap, solve_batched, solve_batched_smo, solver_kind, svr_intercept, takes_batched_smo)
from .kernels import BaseEstimator, LinearKernel
from .multiclass import OneVsRestSVC, uses_batched_path, uses_batched_smo_path, binarize
from .multioutput import uses_batched_smo_svr_path, uses_batched_svr_path
from .onevsone import OneVsOneSVC

__all__ = ['SVCGridSearchCV', 'SVRGridSearchCV', 'parameter_grid', 'check_cv_splits', 'plan_columns', 'plan_svr_columns',
           'plan_smo_columns', 'plan_smo_svr_columns', 'aggregate_scores', 'uses_batched_search', 'uses_batched_smo_search',
           'uses_batched_svr_search', 'uses_batched_smo_svr_search', 'r2_from_sse']

BATCHED_KEYS = frozenset({'C', 'kernel'})
SVR_BATCHED_KEYS = frozenset({'C', 'epsilon', 'kernel'})


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


def check_cv_splits(cv, X, y, stratified=True):
    """(train, test) index arrays: an int is StratifiedKFold(cv) without shuffling (what GridSearchCV gives a classifier;
    stratified=False: KFold(cv), what it gives a regressor), an object with `split` is called as split(X, y), anything else is an
    iterable of (train, test) pairs."""
    if isinstance(cv, (int, np.integer)) and not isinstance(cv, bool):
        from sklearn.model_selection import KFold, StratifiedKFold
        cv = StratifiedKFold(n_splits=int(cv)) if stratified else KFold(n_splits=int(cv))
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
    proto = _prototype(estimator)
    return bool(not has_class_weight(proto) and uses_batched_path(proto, world))


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


def _group_of(groups, index, kernel, Xtr, vectors):
    """the group of the kernel resolved on the fold's training rows Xtr, made on first use"""
    rk = _resolved_kernel(kernel, Xtr)
    key = _kernel_key(rk)
    if key not in index:
        index[key] = len(groups)
        groups.append(dict({name: [] for name in vectors}, kernel=rk, cols=[]))
    return groups[index[key]]


def _stacked(groups, vectors):
    for g in groups:
        for name in vectors:
            g[name] = np.stack(g[name])
    return groups


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
            g = _group_of(groups, index, kernel, X[tr], ('Y', 'UB'))
            ub = np.zeros(n)
            ub[tr] = C
            for r, pos in enumerate(folds[f][1]):
                g['cols'].append((ci, f, r, C))
                g['Y'].append(np.where(y == pos, 1., -1.))
                g['UB'].append(ub)
    return _stacked(groups, ('Y', 'UB')), folds


def uses_batched_smo_search(estimator, candidates, world):
    """True when `SVCGridSearchCV` can solve every (candidate, fold, class) as one batched-SMO column on shared panels: the
    estimator (an `SVC` or an `OneVsRestSVC`) is on `OneVsRestSVC`'s batched SMO path (`uses_batched_smo_path`) and the grid varies
    only C and kernel."""
    if not isinstance(estimator, (SVC, OneVsRestSVC)):
        return False
    if any(not set(p) <= BATCHED_KEYS for p in candidates):
        return False
    proto = _prototype(estimator)
    return bool(not has_class_weight(proto) and uses_batched_smo_path(proto, world))   # the search's columns carry one C each


def plan_smo_columns(X, y, splits, candidates, base_C, base_kernel, multiclass):
    """The batched SMO search's panels and columns, as `plan_columns` groups them: (groups, folds) with groups a list of dicts
    {kernel: the resolved kernel of the panel, cols: [(candidate, fold, class row, C)], Y: m x n labels +-1, rows: per column the
    fold's training rows, ascending} — a column trains on its row list instead of carrying a zero box.  None when a fold's
    training rows miss a class (its own fit has other `classes_`, or none): the search then runs the per-fold calls."""
    X = np.ascontiguousarray(X, dtype=float)
    y = np.asarray(y)
    classes = np.unique(y)
    if any(not np.array_equal(np.unique(y[tr]), classes) for tr, _ in splits):
        return None
    folds = [_fold_labels(y[tr], multiclass) for tr, _ in splits]
    groups, index = [], {}
    for ci, p in enumerate(candidates):
        C = p.get('C', base_C)
        kernel = p.get('kernel', base_kernel)
        for f, (tr, _) in enumerate(splits):
            g = _group_of(groups, index, kernel, X[tr], ('Y',))
            g.setdefault('rows', [])
            rows = np.unique(tr)
            if len(rows) != len(tr):
                return None   # a repeated training row is another problem than a row list's
            for r, pos in enumerate(folds[f][1]):
                g['cols'].append((ci, f, r, C))
                g['Y'].append(np.where(y == pos, 1., -1.))
                g['rows'].append(rows)
    return _stacked(groups, ('Y',)), folds


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


class _GridSearchCV(BaseEstimator):
    """The skeleton of the five searches (`SVCGridSearchCV`, `SVRGridSearchCV`, `NuSVCGridSearchCV`, `NuSVRGridSearchCV`,
    `OneVsOneGridSearchCV`): the candidates and splits, the estimator's own checks on every candidate, the batched path or
    GridSearchCV's per-fold calls, `cv_results_`, the best candidate and its refit.  A subclass says its estimator type(s), its
    messages, whether an int `cv` is stratified, how it checks the targets, when it batches (`_uses_batched`), its
    `_fit_batched`, what one fallback fit records (`_fallback_fit`) and whether 'failed' fits are counted."""
    _estimator_type = None      # a class: the candidates are of it; a tuple of classes: they are of the estimator's own type
    _type_error = ''
    _scoring = 'accuracy scoring'
    _stratified = True
    _column_records = False     # n_iter_ / status_ are (candidates, splits, columns) rather than (candidates, splits)
    _counts_failed = False      # a fit whose (first) status is 'failed' scores NaN under one RuntimeWarning for the search

    def __init__(self, estimator, param_grid, scoring=None, cv=5, refit=True):
        self.estimator = estimator
        self.param_grid = param_grid
        self.scoring = scoring
        self.cv = cv
        self.refit = refit

    def fit(self, X, y):
        if self.scoring is not None:
            raise NotImplementedError('only %s (scoring=None) is implemented' % self._scoring)
        if not isinstance(self.estimator, self._estimator_type):
            raise TypeError(self._type_error)
        X = np.ascontiguousarray(X, dtype=float)
        y = self._targets(X, y)
        candidates = parameter_grid(self.param_grid)
        splits = check_cv_splits(self.cv, X, y, stratified=self._stratified)
        etype = type(self.estimator) if isinstance(self._estimator_type, tuple) else self._estimator_type
        base = _base_params(self.estimator)
        protos = [_make(etype, base, p) for p in candidates]   # the estimator's own checks on every candidate
        self.batched_ = self._uses_batched(protos[0], candidates, splits, y)
        scores, self.n_iter_, self.status_ = self._fits(X, y, splits, candidates, etype, base, protos[0])
        self._account()
        self.n_splits_ = len(splits)
        self.cv_results_ = aggregate_scores(candidates, scores)
        self.best_index_ = int(self.cv_results_['rank_test_score'].argmin())
        self.best_params_ = candidates[self.best_index_]
        self.best_score_ = float(self.cv_results_['mean_test_score'][self.best_index_])
        if self.refit:
            self.best_estimator_ = _make(etype, base, self.best_params_).fit(X, y)
        return self

    @staticmethod
    def _targets(X, y):
        return np.asarray(y)

    def _fits(self, X, y, splits, candidates, etype, base, first):
        """(scores, n_iter, status) of every (candidate, fold), on the batched path or — also when `_fit_batched` declines with
        None before any solve — by the per-fold calls"""
        result = self._fit_batched(X, y, splits, candidates, base, first) if self.batched_ else None
        if result is None:
            self.batched_ = False
            result = self._fit_fallback(X, y, splits, candidates, etype, base)
        return result

    def _account(self):
        if not self._counts_failed:
            return
        fits = self.status_.reshape(self.status_.shape[:2] + (-1,))[:, :, 0]
        n_failed = int((fits == 'failed').sum())
        if n_failed == fits.size:
            raise ValueError('all the %d fits failed' % n_failed)
        if n_failed:
            warnings.warn('%d fits failed out of a total of %d: their scores are nan' % (n_failed, fits.size), RuntimeWarning)

    @staticmethod
    def _fallback_fit(est, Xtr, ytr, Xte, yte):
        """(score, [(iterations, status) per column]) of GridSearchCV's calls on one candidate and fold"""
        score = est.fit(Xtr, ytr).score(Xte, yte)
        fits = est.estimators_ if isinstance(est, (OneVsRestSVC, OneVsOneSVC)) else [est]
        return score, [(int(getattr(e.optimizer, 'iter', -1)), str(getattr(e.optimizer, 'status', ''))) for e in fits]

    def _fit_fallback(self, X, y, splits, candidates, etype, base):
        nc, ns = len(candidates), len(splits)
        scores = np.empty((nc, ns))
        recs = [[None] * ns for _ in range(nc)]
        for ci, p in enumerate(candidates):
            for f, (tr, te) in enumerate(splits):
                est = _make(etype, base, {}).set_params(**p)
                scores[ci, f], recs[ci][f] = self._fallback_fit(est, X[tr], y[tr], X[te], y[te])
        width = max(len(r) for row in recs for r in row)
        n_iter = np.full((nc, ns, width), -1, dtype=np.int64)
        status = np.full((nc, ns, width), '', dtype=object)
        for ci in range(nc):
            for f in range(ns):
                for c, (it, st) in enumerate(recs[ci][f]):
                    n_iter[ci, f, c], status[ci, f, c] = it, st
        return (scores, n_iter, status) if self._column_records else (scores, n_iter[:, :, 0], status[:, :, 0])

    def decision_function(self, X):
        return self.best_estimator_.decision_function(X)

    def predict(self, X):
        return self.best_estimator_.predict(X)

    def score(self, X, y):
        return self.best_estimator_.score(X, y)


class SVCGridSearchCV(_GridSearchCV):
    """Exhaustive search over `param_grid` for an `SVC` or `OneVsRestSVC` scored by accuracy, as sklearn's GridSearchCV.  A
    `OneVsOneSVC` runs GridSearchCV's per-fold calls, each fold's fit one batched one-vs-one solve.

    After `fit`: `cv_results_` (params, param_<key>, split<i>_test_score, mean / std / rank_test_score — no timing keys: the
    candidates' fits are one batched solve and have no fit time of their own), `best_index_` (first among ties), `best_params_`,
    `best_score_`, `n_splits_`, `best_estimator_` (a plain `fit` on all the data, refit=True), and per column `n_iter_` / `status_`
    of shape (candidates, splits, classes) (-1 / '' where a fit has no such record).  `batched_` says which path ran.
    `predict`, `decision_function` and `score` are the best estimator's.

    An estimator on the batched SMO path (`uses_batched_smo_search`) has every (candidate, fold, class) solved as one column of
    `bq_msmo_*` whose row list is the fold's training rows; `smo_` says so, and `batch_smo` (None, True, False) forces that choice
    where the configuration allows it (None: by the number of columns, `takes_batched_smo`).  A fold that misses a class runs the
    per-fold calls.
    """
    _estimator_type = (SVC, OneVsRestSVC, OneVsOneSVC)
    _type_error = 'estimator must be an SVC, a OneVsRestSVC or a OneVsOneSVC'
    _column_records = True
    batch_smo = None

    def _uses_batched(self, first, candidates, splits, y):
        world = get_context().world
        self.smo_ = False
        if uses_batched_smo_search(first, candidates, world):
            classes = 1 if len(np.unique(y)) == 2 or not isinstance(first, OneVsRestSVC) else len(np.unique(y))
            self.smo_ = takes_batched_smo(len(candidates) * len(splits) * classes, self.batch_smo)
        return self.smo_ or uses_batched_search(first, candidates, world)

    def _fit_batched_smo(self, X, y, splits, candidates, proto_est):
        """every (candidate, fold, class) one batched-SMO column on the panel of its resolved kernel; None (before any solve) when
        a fold misses a class"""
        multiclass = isinstance(proto_est, OneVsRestSVC)
        proto = _prototype(proto_est)
        n = len(y)
        nc, ns = len(candidates), len(splits)
        plan = plan_smo_columns(X, y, splits, candidates, proto.C, proto.kernel, multiclass)
        if plan is None:
            self.smo_ = False
            return None
        groups, folds = plan
        width = max(len(rows) for _, rows in folds)
        n_iter = np.full((nc, ns, width), -1, dtype=np.int64)
        status = np.full((nc, ns, width), '', dtype=object)   # an SMO fit records no status (`_fallback_fit`)
        dec = [[[None] * len(folds[f][1]) for f in range(ns)] for _ in range(nc)]
        for g in groups:   # one panel at a time, built as SVC.fit's SMO branch builds it
            m = len(g['cols'])
            with device_panel(X, -np.ones(n), 'svc', g['kernel'], y=g['Y'][0], storage=proto.storage, rank_one=False,
                              compact=False) as (_, dev, free, slab):
                cap = smo_column_cap(n, _lib.SVC, free - slab)
                res = solve_batched_smo(dev, _lib.SVC, g['Y'], [C for _, _, _, C in g['cols']], None, proto.tol, rows=g['rows'],
                                        cap=cap)
                W = np.zeros((m, n))
                for j, r in enumerate(res):
                    sv = r['alphas'] > 1e-6
                    W[j][sv] = r['alphas'][sv] * g['Y'][j][sv]
                U = _gram_matmat(dev, W, wide=True)   # without the rank-one term the panel is K: K w on every row
                for j, (ci, f, row, C) in enumerate(g['cols']):
                    n_iter[ci, f, row] = res[j]['iter']
                    te = splits[f][1]
                    kernel = candidates[ci].get('kernel', proto.kernel)
                    if proto.storage == 'f64' and not isinstance(getattr(kernel, 'gamma', None), str):
                        dec[ci][f][row] = U[j][te] + res[j]['b']   # the fp64 panel holds the decision kernel's values
                    else:
                        # decision_function resolves a string gamma on the support vectors and evaluates the kernel in fp64, not
                        # from an fp32 panel: score through the fold's SVC
                        sv = W[j] != 0
                        est = copy.copy(proto)
                        est.kernel, est.C = kernel, C
                        est.support_vectors_ = X[sv]
                        est.dual_coef_ = W[j][sv]
                        if isinstance(kernel, LinearKernel):
                            est.coef_ = np.dot(est.dual_coef_, est.support_vectors_)
                        est.intercept_ = res[j]['b']
                        dec[ci][f][row] = est.decision_function(X[te])
        self._cv_decisions = dec
        return self._scores(dec, folds, splits, y), n_iter, status

    @staticmethod
    def _scores(dec, folds, splits, y):
        """accuracy of every (candidate, fold) from its columns' held-out decision values"""
        scores = np.empty((len(dec), len(splits)))
        for ci in range(len(dec)):
            for f, (_, te) in enumerate(splits):
                classes = folds[f][0]
                D = dec[ci][f]
                if len(D) == 1:
                    pred = np.where(D[0] > 0, classes[-1], classes[0])
                else:
                    pred = classes[np.argmax(np.stack(D, axis=1), axis=1)]
                scores[ci, f] = float(np.mean(pred == y[te]))
        return scores

    def _fit_batched(self, X, y, splits, candidates, base, proto_est):
        if self.smo_:
            return self._fit_batched_smo(X, y, splits, candidates, proto_est)
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
            with device_panel(X, -np.ones(n), 'svc', g['kernel'], y=g['Y'][0], storage=proto.storage,
                              tune_placement=proto._streams_panel(),
                              expected_products=proto.max_iter * ((m + 15) // 16)) as (_, dev, free, slab):
                cap = column_cap(n, free, slab)
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
        self._cv_decisions = dec
        return self._scores(dec, folds, splits, y), n_iter, status


def uses_batched_svr_search(estimator, candidates, world):
    """True when `SVRGridSearchCV` solves every (candidate, fold) on shared panels: the estimator (an `SVR`) is on
    `MultiOutputSVR`'s batched path (`uses_batched_svr_path`) and the grid varies only C, epsilon and kernel."""
    if not isinstance(estimator, SVR):
        return False
    if any(not set(p) <= SVR_BATCHED_KEYS for p in candidates):
        return False
    return bool(not has_class_weight(estimator) and uses_batched_svr_path(estimator, world))


def plan_svr_columns(X, y, splits, candidates, base_C, base_epsilon, base_kernel):
    """The batched SVR search's panels and columns: a list of dicts {kernel: the resolved kernel of the panel, cols: [(candidate,
    fold, C, epsilon)], QL: m x 2n linear terms [-y; y] + epsilon, UB: m x 2n boxes, C on both halves of the fold's training rows
    and 0 on both halves of its held-out rows} — one group per resolved kernel, as `plan_columns` groups them."""
    X = np.ascontiguousarray(X, dtype=float)
    y = np.asarray(y, dtype=float)
    n = len(y)
    q0 = np.hstack((-y, y))
    groups, index = [], {}
    for ci, p in enumerate(candidates):
        C, epsilon = p.get('C', base_C), p.get('epsilon', base_epsilon)
        kernel = p.get('kernel', base_kernel)
        for f, (tr, _) in enumerate(splits):
            g = _group_of(groups, index, kernel, X[tr], ('QL', 'UB'))
            ub = np.zeros(2 * n)
            ub[tr] = C
            ub[n + tr] = C
            g['cols'].append((ci, f, C, epsilon))
            g['QL'].append(q0 + epsilon)
            g['UB'].append(ub)
    return _stacked(groups, ('QL', 'UB'))


def uses_batched_smo_svr_search(estimator, candidates, world):
    """True when `SVRGridSearchCV` can solve every (candidate, fold) as one batched-SMO column on shared panels and score it on the
    device (`bq_msmo_svr_heldout`): the estimator (an `SVR`) is on `MultiOutputSVR`'s batched SMO path
    (`uses_batched_smo_svr_path`), the grid varies only C, epsilon and kernel, the panel is 'f64' and no kernel of the search has a
    string gamma — the fp64 panel of a numeric gamma holds the decision kernel's values.  An fp32 panel or gamma='scale' keeps the
    per-fold calls."""
    if not isinstance(estimator, SVR):
        return False
    if any(not set(p) <= SVR_BATCHED_KEYS for p in candidates):
        return False
    kernels = [estimator.kernel] + [p['kernel'] for p in candidates if 'kernel' in p]
    if any(isinstance(getattr(k, 'gamma', None), str) for k in kernels):
        return False
    return bool(not has_class_weight(estimator) and uses_batched_smo_svr_path(estimator, world) and estimator.storage == 'f64')


def plan_smo_svr_columns(X, y, splits, candidates, base_C, base_epsilon, base_kernel):
    """The batched SMO SVR search's panels and columns, as `plan_svr_columns` groups them: a list of dicts {kernel: the resolved
    kernel of the panel, cols: [(candidate, fold, C, epsilon)], Y: m x n targets (every row is y: the held-out rows' targets are
    what the scorer compares with), rows: per column the fold's training rows, ascending}.  None when a fold repeats a training row
    or test row, or trains on a row it tests: that is another problem than a row list's."""
    X = np.ascontiguousarray(X, dtype=float)
    y = np.asarray(y, dtype=float)
    lists = []
    for tr, te in splits:
        rows = np.unique(tr)
        if len(rows) != len(tr) or len(np.unique(te)) != len(te) or len(np.intersect1d(rows, te)):
            return None
        lists.append(rows)
    groups, index = [], {}
    for ci, p in enumerate(candidates):
        C, epsilon = p.get('C', base_C), p.get('epsilon', base_epsilon)
        kernel = p.get('kernel', base_kernel)
        for f, (tr, _) in enumerate(splits):
            g = _group_of(groups, index, kernel, X[tr], ('Y',))
            g.setdefault('rows', [])
            g['cols'].append((ci, f, C, epsilon))
            g['Y'].append(y)
            g['rows'].append(lists[f])
    return _stacked(groups, ('Y',))


def svr_column_cap(n, free_bytes, slab_bytes):
    """`column_cap` for the columns of an SVR search on n rows, whose vectors have 2n entries: `column_bytes(2 * n)` per column.
    That budgets 16 vectors of 2n; a column holds 7 (x, g, d, Qd, both bounds, its linear term) and two n-vectors (product input
    and output), so the cap errs on the small side by about a half, which leaves room for the host's records and the scoring's
    few vectors."""
    return column_cap(2 * n, free_bytes, slab_bytes)


def r2_from_sse(sse, y_test):
    """sklearn's `r2_score` from the squared error of the predictions on y_test: 1 - sse / sum (y - mean(y))^2; a constant y_test
    scores 1 for a perfect prediction and 0 otherwise (r2_score's force_finite), and a NaN error scores NaN."""
    y_test = np.asarray(y_test, dtype=float)
    den = float(((y_test - np.average(y_test)) ** 2).sum())
    if np.isnan(sse):
        return float('nan')
    if den == 0.:
        return 1. if sse == 0. else 0.
    return 1. - float(sse) / den


class SVRGridSearchCV(_GridSearchCV):
    """Exhaustive search over `param_grid` for an `SVR` scored by R^2, as sklearn's GridSearchCV.  An int `cv` is KFold(cv)
    without shuffling.

    After `fit`: the attributes of `SVCGridSearchCV` — `cv_results_`, `best_index_`, `best_params_`, `best_score_`, `n_splits_`,
    `best_estimator_` (a plain `SVR.fit` on all the data, refit=True) — with `n_iter_` / `status_` of shape (candidates, splits),
    and `batched_`, which says which path ran.  A fit that ends without support vectors scores NaN on either path (`SVR.fit`
    divides by zero there; GridSearchCV's error_score).  `predict` and `score` are the best estimator's.

    An estimator on the batched SMO path (`uses_batched_smo_svr_search`) has every (candidate, fold) solved as one column of
    `bq_msmo_*` whose row list is the fold's training rows and scored on the device (`bq_msmo_svr_heldout`); `smo_` says so
    (`batched_` is True with it), and `batch_smo` (None, True, False) forces that choice where the configuration allows it (None:
    by the number of columns, `takes_batched_smo`).  An SMO fit without support vectors predicts its intercept and has a score.
    """
    batch_smo = None

    _estimator_type = SVR
    _type_error = 'estimator must be an SVR'
    _scoring = 'R^2 scoring'
    _stratified = False

    @staticmethod
    def _targets(X, y):
        y = np.asarray(y, dtype=float)
        if y.ndim != 1:
            raise ValueError('use MultiOutputSVR to train a model over more than one target')
        return y

    def _uses_batched(self, first, candidates, splits, y):
        world = get_context().world
        self.smo_ = False
        if uses_batched_smo_svr_search(first, candidates, world):
            self.smo_ = takes_batched_smo(len(candidates) * len(splits), self.batch_smo)
        return self.smo_ or uses_batched_svr_search(first, candidates, world)

    @staticmethod
    def _fallback_fit(est, Xtr, ytr, Xte, yte):
        try:
            score = est.fit(Xtr, ytr).score(Xte, yte)
        except ZeroDivisionError:   # no support vector
            score = np.nan
        return score, [(int(getattr(est.optimizer, 'iter', -1)), str(getattr(est.optimizer, 'status', '')))]

    def _fit_batched_smo(self, X, y, splits, candidates, proto):
        """every (candidate, fold) one batched-SMO column on the panel of its kernel, built as `MultiOutputSVR`'s SMO fit builds
        it, in solves of at most `smo_heldout_column_cap` columns, scored where the walkers' state lives (`svr_heldout`, one set
        per fold); None (before any solve) when the folds are no row lists"""
        groups = plan_smo_svr_columns(X, y, splits, candidates, proto.C, proto.epsilon, proto.kernel)
        if groups is None:
            self.smo_ = False
            return None
        n = len(y)
        nc, ns = len(candidates), len(splits)
        scores = np.empty((nc, ns))
        n_iter = np.full((nc, ns), -1, dtype=np.int64)
        status = np.full((nc, ns), '', dtype=object)   # an SMO fit records no status (`_fallback_fit`)
        held = np.zeros((ns, n), dtype=np.uint8)
        for f, (_, te) in enumerate(splits):
            held[f, te] = 1
        for g in groups:   # one panel at a time
            m = len(g['cols'])
            with device_panel(X, np.hstack((-y, y)) + proto.epsilon, 'svr', g['kernel'], storage=proto.storage, rank_one=False,
                              compact=False) as (_, dev, free, slab):
                cap = smo_heldout_column_cap(n, _lib.SVR, free, slab)
                for c0 in range(0, m, cap):
                    cols = g['cols'][c0:c0 + cap]
                    solver = _DeviceSMOSolver(dev, _lib.SVR, g['Y'][c0:c0 + cap], [C for _, _, C, _ in cols],
                                              [eps for _, _, _, eps in cols], proto.tol, rows=g['rows'][c0:c0 + cap])
                    try:
                        outer, failed = run_batched_smo(solver)
                        if failed.any():
                            raise smo_failed_error()
                        _, _, sse, _ = solver.svr_heldout([f for _, f, _, _ in cols], held)
                    finally:
                        solver.close()
                    for j, (ci, f, _, _) in enumerate(cols):
                        scores[ci, f] = r2_from_sse(sse[j], y[splits[f][1]])
                        n_iter[ci, f] = outer[j]
        return scores, n_iter, status

    def _fit_batched(self, X, y, splits, candidates, base, first):
        proto = _make(SVR, base, {})
        if self.smo_:
            return self._fit_batched_smo(X, y, splits, candidates, proto)
        n = len(y)
        nc, ns = len(candidates), len(splits)
        scores = np.empty((nc, ns))
        n_iter = np.full((nc, ns), -1, dtype=np.int64)
        status = np.full((nc, ns), '', dtype=object)
        kind = solver_kind(proto.optimizer)
        for g in plan_svr_columns(X, y, splits, candidates, proto.C, proto.epsilon, proto.kernel):   # one panel at a time
            m = len(g['cols'])
            # the 'svr' structure's own linear term is never used by the batched solver
            with device_panel(X, g['QL'][0], 'svr', g['kernel'], storage=proto.storage, tune_placement=proto._streams_panel(),
                              expected_products=proto.max_iter * ((m + 15) // 16)) as (obj, dev, free, slab):
                cap = svr_column_cap(n, free, slab)
                for c0 in range(0, m, cap):
                    cols = g['cols'][c0:c0 + cap]
                    QL, UB = g['QL'][c0:c0 + cap], g['UB'][c0:c0 + cap]
                    # the fp64 panel of a numeric gamma holds the decision kernel's values: such columns are scored on the device
                    on_device = [proto.storage == 'f64' and not isinstance(getattr(candidates[ci].get('kernel', proto.kernel), 'gamma',
                                                                                   None), str) for ci, _, _, _ in cols]
                    held = {}

                    def score(solver, _):
                        if any(on_device):
                            held['b'], _, held['sse'], _ = solver.heldout(y, [eps for _, _, _, eps in cols])

                    res = solve_batched(dev, kind, QL, UB, solver=_DeviceSVRSolver(dev, kind, QL, UB, 1e-6, proto.max_iter),
                                        before_close=score, vectors=not all(on_device))
                    ests, svs = {}, {}
                    for j, (ci, f, _, _) in enumerate(cols):
                        n_iter[ci, f], status[ci, f] = res[j]['iter'], res[j]['status']
                        if on_device[j]:
                            scores[ci, f] = r2_from_sse(held['sse'][j], y[splits[f][1]])
                        else:
                            # decision_function resolves a string gamma on the support vectors and evaluates the kernel in fp64, not
                            # from an fp32 panel: score through the fold's SVR
                            ests[j] = _make(SVR, base, candidates[ci])
                            svs[j] = fitted_svr(ests[j], obj, res[j], X, y)
                    if ests:
                        W = np.zeros((len(ests), n))
                        for r, j in enumerate(ests):
                            W[r][svs[j]] = ests[j].dual_coef_
                        U = _gram_matmat(dev, W, wide=True)
                        for r, j in enumerate(ests):
                            ci, f, _, eps = cols[j]
                            te = splits[f][1]
                            try:
                                ests[j].intercept_ = svr_intercept(y, U[r], svs[j], eps)
                                scores[ci, f] = ests[j].score(X[te], y[te])
                            except ZeroDivisionError:   # no support vector
                                scores[ci, f] = np.nan
        return scores, n_iter, status
