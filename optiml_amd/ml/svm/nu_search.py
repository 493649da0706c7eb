"""Cross-validated grid search over `NuSVC` (accuracy) and `NuSVR` (R^2): the result of sklearn's
`GridSearchCV(estimator, param_grid, cv=cv, refit=refit)`, with every (candidate, fold) of one resolved kernel a column of ONE
two-group simplex solve (`bq_msolver_create_simplex2`) on ONE Gram panel of all n rows.

nu and C enter the nu-duals only through the groups' masses and the boxes, and a row whose box is 0 is a row the column does not
train on: it starts at 0 and never moves, so every sum of the iteration is the training fold's.  The columns:

  NuSVC  (candidate, fold)  S = the +-1 labels (the larger label +1), UB = 1 on the fold's training rows and 0 elsewhere,
                            mass = nu n_train / 2 twice
  NuSVR  (candidate, fold)  UB = C on both halves of the training rows and 0 elsewhere, mass = C nu n_train / 2 twice, q = (-y, y)

An fp64 panel's columns are scored where the solver's state lives (`bq_msolver_simplex2_heldout`): per column the offsets, a held-out
count and the number of correct held-out predictions (or the held-out squared error) come back, no k x n array.  That includes a
string gamma, which the nu-estimators resolve at fit and keep in `kernel_`: the panel of a fold holds the decision kernel's values.
An fp32 panel holds K rounded to fp32 while `decision_function` evaluates the kernel in fp64, so its columns are scored through the
fold's estimator, built from the column without a refit.  A panel that serves a single fold — every panel of a string gamma — holds
the fold's training rows first, in the fold's order, so that its leading block is the panel `fit` builds on those rows and the
column follows the fold's own fit rather than a copy of it perturbed in the product's last bits.

A fit that `GridSearchCV` would record as failed — a nu that is infeasible on the fold's training labels, a fold with one class —
is not a column: it scores NaN (sklearn's error_score), has `n_iter_` -1 and `status_` 'failed', and one RuntimeWarning names the
number of such fits; if every fit fails the search raises ValueError, as GridSearchCV does.

The batched path applies when the grid varies only nu and kernel (NuSVC) or C, nu and kernel (NuSVR); the estimator's `tol`,
`max_iter` and `storage` are shared by all columns.  Every other key runs exactly GridSearchCV's calls per candidate and fold.
"""
import warnings

import numpy as np

from ...device import get_context
from ._base import ConvergenceWarning, has_class_weight
from ._batched import _DeviceSimplex2Solver, column_cap, device_panel, solve_batched
from .model_selection import _GridSearchCV, _group_of, _make, _stacked, r2_from_sse
from .nu import NuSVC, NuSVR, _check_feasible

__all__ = ['NuSVCGridSearchCV', 'NuSVRGridSearchCV', 'plan_nu_svc_columns', 'plan_nu_svr_columns', 'uses_batched_nu_search']

NU_SVC_BATCHED_KEYS = frozenset({'nu', 'kernel'})
NU_SVR_BATCHED_KEYS = frozenset({'C', 'nu', 'kernel'})


def uses_batched_nu_search(estimator, candidates):
    """True when the search solves every (candidate, fold) on shared panels: the estimator is a `NuSVC` and the grid varies only nu
    and kernel, or a `NuSVR` and the grid varies only C, nu and kernel."""
    if has_class_weight(estimator):   # the nu duals carry no per-row boxes
        return False
    if isinstance(estimator, NuSVC):
        keys = NU_SVC_BATCHED_KEYS
    elif isinstance(estimator, NuSVR):
        keys = NU_SVR_BATCHED_KEYS
    else:
        return False
    return all(set(p) <= keys for p in candidates)


def plan_nu_svc_columns(X, y, splits, candidates, base_nu, base_kernel):
    """The batched NuSVC search's panels and columns.  Returns (groups, classes, failed): classes, the two labels; groups, a list of
    dicts {kernel: the resolved kernel of the panel, cols: [(candidate, fold, nu)], S: m x n labels +-1 (the larger label +1), UB:
    m x n boxes, 1 on the fold's training rows and 0 elsewhere, mass: m x 2, nu n_train / 2 twice} — one group per resolved kernel (a
    string gamma resolves on every fold's training rows); failed: the (candidate, fold) pairs `NuSVC.fit` refuses on the fold's
    training rows (one class there, or a nu its smaller class cannot hold), which are no columns."""
    X = np.ascontiguousarray(X, dtype=float)
    y = np.asarray(y)
    n = len(y)
    classes = np.unique(y)
    if len(classes) > 2:
        raise ValueError('use OneVsOneClassifier or OneVsRestClassifier from sklearn.multiclass '
                         'to train a model over more than two labels')
    s = np.where(y == classes[-1], 1., -1.)
    groups, index, failed = [], {}, []
    for ci, p in enumerate(candidates):
        nu, kernel = p.get('nu', base_nu), p.get('kernel', base_kernel)
        for f, (tr, _) in enumerate(splits):
            try:
                if len(np.unique(y[tr])) < 2:
                    raise ValueError('NuSVC needs two classes')
                _check_feasible(s[tr], nu)
            except ValueError:
                failed.append((ci, f))
                continue
            g = _group_of(groups, index, kernel, X[tr], ('S', 'UB', 'mass'))
            ub = np.zeros(n)
            ub[tr] = 1.
            g['cols'].append((ci, f, nu))
            g['S'].append(s)
            g['UB'].append(ub)
            g['mass'].append([nu * len(tr) / 2] * 2)
    return _stacked(groups, ('S', 'UB', 'mass')), classes, failed


def plan_nu_svr_columns(X, y, splits, candidates, base_C, base_nu, base_kernel):
    """The batched NuSVR search's panels and columns: a list of dicts {kernel: the resolved kernel of the panel, cols: [(candidate,
    fold, C, nu)], UB: m x 2n boxes, C on both halves of the fold's training rows and 0 on both halves of its held-out rows, mass:
    m x 2, C nu n_train / 2 twice, q: m x 2n linear terms (-y, y)} — one group per resolved kernel, as `plan_nu_svc_columns` groups
    them."""
    X = np.ascontiguousarray(X, dtype=float)
    y = np.asarray(y, dtype=float)
    n = len(y)
    q = np.concatenate((-y, y))
    groups, index = [], {}
    for ci, p in enumerate(candidates):
        C, nu, kernel = p.get('C', base_C), p.get('nu', base_nu), p.get('kernel', base_kernel)
        for f, (tr, _) in enumerate(splits):
            g = _group_of(groups, index, kernel, X[tr], ('UB', 'mass', 'q'))
            ub = np.zeros(2 * n)
            ub[tr] = C
            ub[n + tr] = C
            g['cols'].append((ci, f, C, nu))
            g['UB'].append(ub)
            g['mass'].append([C * nu * len(tr) / 2] * 2)
            g['q'].append(q)
    return _stacked(groups, ('UB', 'mass', 'q'))


class _NuGridSearchCV(_GridSearchCV):
    """What the two searches share; a subclass names its estimator type, whether an int `cv` is stratified, and its columns."""
    _scoring = 'the estimator\'s own score'
    _counts_failed = True

    @staticmethod
    def _uses_batched(first, candidates, splits, y):
        return uses_batched_nu_search(first, candidates)

    def _fits(self, *args):
        with warnings.catch_warnings(record=True) as caught:   # one ConvergenceWarning for the search, not one per fit
            warnings.simplefilter('always')
            result = _GridSearchCV._fits(self, *args)
        for w in caught:
            if not issubclass(w.category, ConvergenceWarning):
                warnings.warn_explicit(w.message, w.category, w.filename, w.lineno)
        return result

    def _account(self):
        _GridSearchCV._account(self)
        if (self.status_ == 'stopped').any():
            warnings.warn('max_iter reached but the optimization has not converged yet', ConvergenceWarning)

    @staticmethod
    def _fallback_fit(est, Xtr, ytr, Xte, yte):
        try:
            est.fit(Xtr, ytr)
        except ValueError:   # GridSearchCV's error_score: the fit is recorded as failed and scores nan
            return np.nan, [(-1, 'failed')]
        return est.score(Xte, yte), [(est.n_iter_, est.status_)]

    def _fit_batched(self, X, y, splits, candidates, base, first):
        proto = _make(self._estimator_type, base, {})
        name = type(self).__name__
        if proto.storage == 'stream':
            raise NotImplementedError(f'{name} needs a resident panel: storage \'f64\' or \'f32\'')
        if get_context().world != 1:
            raise NotImplementedError(f'{name} runs on a single-rank context')
        n = X.shape[0]
        nc, ns = len(candidates), len(splits)
        scores = np.full((nc, ns), np.nan)
        n_iter = np.full((nc, ns), -1, dtype=np.int64)
        status = np.full((nc, ns), 'failed', dtype=object)
        on_device = proto.storage == 'f64'   # the fp64 panel holds the decision kernel's values
        groups, y_dev = self._plan(X, y, splits, candidates, proto)
        for g in groups:   # one panel at a time
            m = len(g['cols'])
            # A panel that serves one fold (a string gamma) has the fold's training rows first, in the fold's order: its leading
            # block is then the panel `fit` builds on those rows, tile for tile, the zero boxes behind it add exact zeros to every
            # product, and the column follows the fold's own fit instead of a rounding-perturbed copy of it
            folds = {col[1] for col in g['cols']}
            order = np.arange(n)
            if len(folds) == 1:
                tr = splits[folds.pop()][0]
                order = np.concatenate((tr, np.setdiff1d(order, tr)))
            wide = g['UB'].shape[1] == 2 * n
            var = np.concatenate((order, n + order)) if wide else order   # the variables in the panel's row order
            S = g['S'][:, order] if 'S' in g else None
            UB, q = g['UB'][:, var], g['q'][:, var] if 'q' in g else None
            with device_panel(X[order], np.zeros(n), 'plain', g['kernel'], storage=proto.storage,
                              tune_placement=bool(proto.tune_placement),
                              expected_products=proto.max_iter * ((m + 15) // 16)) as (_, dev, free, slab):
                cap = column_cap(n, free, slab)
                if wide:   # (a column of 2n variables holds twice the vectors the cap counts)
                    cap = max(1, cap // 2)
                for c0 in range(0, m, cap):
                    sl = slice(c0, c0 + cap)
                    cols = g['cols'][sl]
                    held = {}

                    def score(solver, _):
                        held['r1'], held['r2'], _, _, held['n_held'], held['n_correct'], held['sse'] = solver.heldout(y_dev[order])

                    solver = _DeviceSimplex2Solver(dev, None if S is None else S[sl], UB[sl], g['mass'][sl],
                                                   None if q is None else q[sl], proto.tol, proto.max_iter)
                    res = solve_batched(dev, None, UB[sl], None, solver=solver, before_close=score, vectors=not on_device)
                    for j, col in enumerate(cols):
                        ci, f = col[:2]
                        n_iter[ci, f], status[ci, f] = res[j]['iter'], res[j]['status']
                        if on_device:
                            scores[ci, f] = self._device_score(held, j, y[splits[f][1]])
                        else:
                            tr, te = splits[f]
                            x = np.empty_like(res[j]['x'])
                            x[var] = res[j]['x']   # back in the data's row order
                            est = self._fold_estimator(_make(self._estimator_type, base, candidates[ci]), X, y, tr, g['kernel'],
                                                       dict(res[j], x=x), float(held['r1'][j]), float(held['r2'][j]))
                            scores[ci, f] = est.score(X[te], y[te])
        return scores, n_iter, status


class NuSVCGridSearchCV(_NuGridSearchCV):
    """Exhaustive search over `param_grid` for a `NuSVC` scored by accuracy, as sklearn's GridSearchCV.  An int `cv` is
    StratifiedKFold(cv) without shuffling.  More than two labels raise `NuSVC`'s error before any device work.

    After `fit`: `cv_results_` (params, param_<key>, split<i>_test_score, mean / std / rank_test_score — no timing keys: the
    candidates' fits are one batched solve and have no fit time of their own), `best_index_` (first among ties), `best_params_`,
    `best_score_`, `n_splits_`, `best_estimator_` (a plain `NuSVC.fit` on all the data, refit=True), `n_iter_` / `status_` of shape
    (candidates, splits) and `batched_`, which says which path ran.  A fit `NuSVC.fit` refuses on a fold's training rows (an
    infeasible nu, one class) scores NaN with `n_iter_` -1 and `status_` 'failed' under one RuntimeWarning for the search; a search
    whose fits all fail raises ValueError.  One ConvergenceWarning is raised if any fit ends 'stopped'.  `predict`,
    `decision_function` and `score` are the best estimator's.
    """
    _estimator_type = NuSVC
    _type_error = 'estimator must be a NuSVC'

    @staticmethod
    def _targets(X, y):
        y = np.asarray(y)
        if len(np.unique(y)) > 2:
            raise ValueError('use OneVsOneClassifier or OneVsRestClassifier from sklearn.multiclass '
                             'to train a model over more than two labels')
        return y

    @staticmethod
    def _plan(X, y, splits, candidates, proto):
        groups, classes, _ = plan_nu_svc_columns(X, y, splits, candidates, proto.nu, proto.kernel)
        return groups, np.where(y == classes[-1], 1., -1.)

    @staticmethod
    def _device_score(held, j, y_test):
        return float(held['n_correct'][j]) / float(held['n_held'][j])   # (np.mean of the matches: their count over their number)

    @staticmethod
    def _fold_estimator(est, X, y, tr, kernel, r, r1, r2):
        s = est._labels(y[tr])
        return est._fitted(X[tr], s, kernel, dict(r, x=r['x'][tr]), r1, r2)


class NuSVRGridSearchCV(_NuGridSearchCV):
    """Exhaustive search over `param_grid` for a `NuSVR` scored by R^2, as sklearn's GridSearchCV.  An int `cv` is KFold(cv) without
    shuffling.  The attributes, warnings and errors after `fit` are `NuSVCGridSearchCV`'s, with `best_estimator_` a plain
    `NuSVR.fit` on all the data; `predict`, `decision_function` and `score` are the best estimator's."""
    _estimator_type = NuSVR
    _type_error = 'estimator must be a NuSVR'
    _stratified = False

    @staticmethod
    def _targets(X, y):
        return NuSVR._targets(X, y)

    @staticmethod
    def _plan(X, y, splits, candidates, proto):
        return plan_nu_svr_columns(X, y, splits, candidates, proto.C, proto.nu, proto.kernel), y

    @staticmethod
    def _device_score(held, j, y_test):
        return r2_from_sse(held['sse'][j], y_test)

    @staticmethod
    def _fold_estimator(est, X, y, tr, kernel, r, r1, r2):
        n = X.shape[0]
        return est._fitted(X[tr], kernel, dict(r, x=np.concatenate((r['x'][tr], r['x'][n + tr]))), r1, r2)
