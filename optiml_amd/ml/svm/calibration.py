"""Probability calibration of `SVC` / `OneVsRestSVC` by Platt's sigmoid: the result of sklearn's
`CalibratedClassifierCV(estimator, method='sigmoid', cv=cv, ensemble=ensemble)`, with every fold's fits solved together on ONE Gram
panel of all n rows.

The search's observation carries over (model_selection.py): a training-fold dual is the full-data dual with ub = 0 on the held-out
rows, so every (fold, class) fit is one column of `bq_msolver_create_boxes` on one panel, and the fit on all the data that
`ensemble=False` predicts with is one more column per class with ub = C everywhere.  The columns are scored where the solver's state
lives (`bq_msolver_svc_heldout`): per column an intercept and a support count, the held-out decision values of the fp64 panel into
one buffer row per calibrator, and on those rows the sigmoid fits (`platt_fit_kernel`, bq_platt.hip: Newton's iteration with
backtracking of Lin, Lin & Weng as libsvm's `sigmoid_train` states it, one workgroup per calibrator).

An estimator on the batched SMO path (`uses_batched_smo_calibration`: optimizer 'smo', an unregularised intercept, an 'f64' panel, a
numeric gamma) takes the same route with the walkers of `bq_msmo_*`: every (fold, class) fit is one column whose row list is the fold's
training rows, and `bq_msmo_svc_heldout` takes the intercepts, the held-out decision values and the sigmoids from the walkers' state.

The batched path applies under the conditions under which `SVCGridSearchCV` takes decision values from the panel: the estimator is
on `OneVsRestSVC`'s batched path (`uses_batched_path`), the panel is 'f64' and the kernel's gamma is not a string.  Every other
configuration runs the loop sklearn runs, `fit` on X[tr] and `decision_function` on X[te] per fold, and fits the sigmoids through
the same kernel (`bq_platt_fit`): the package has one Platt implementation, on the device.
"""
import warnings
from collections import namedtuple

import numpy as np

from ... import _lib
from ...device import get_context
from ...opti import KernelQuadratic
from ._base import SVC, ClassifierMixin, ConvergenceWarning, has_class_weight
from ._batched import (ClassQuadratic, DecisionBatch, _DeviceSMOSolver, device_free_bytes, fitted_smo_svc, fitted_svc, platt_fit,
                       run_batched_smo, smo_column_result, smo_failed_error, smo_heldout_column_cap, solve_batched,
                       solve_batched_smo, solver_kind, takes_batched_smo, uses_batched_decision)
from .kernels import BaseEstimator
from .model_selection import _base_params, _fold_labels, _make, _prototype, check_cv_splits, column_cap
from .multiclass import OneVsRestSVC, uses_batched_path, uses_batched_smo_path

__all__ = ['CalibratedSVC', 'CalibratedClassifier', 'uses_batched_calibration', 'uses_batched_smo_calibration',
           'sigmoid_probabilities', 'assemble_probabilities']

CalibratedClassifier = namedtuple('CalibratedClassifier', ['estimator', 'A', 'B'])
CalibratedClassifier.__doc__ = """A fitted classifier (an `SVC`, or an `OneVsRestSVC` with more than two classes) and the sigmoids of
its decision values: A, B with one entry per class (one entry, the positive class's, with two classes)."""


def uses_batched_calibration(estimator, world):
    """True when `CalibratedSVC` solves every (fold, class) on one panel and calibrates on the device: the estimator (an `SVC` or
    an `OneVsRestSVC`) is on `OneVsRestSVC`'s batched path, its panel is 'f64' and its kernel's gamma is not a string — the fp64
    panel of a numeric gamma holds the decision kernel's values."""
    if not isinstance(estimator, (SVC, OneVsRestSVC)):
        return False
    proto = _prototype(estimator)
    return bool(not has_class_weight(proto) and uses_batched_path(proto, world) and proto.storage == 'f64' and
                not isinstance(getattr(proto.kernel, 'gamma', None), str))


def uses_batched_smo_calibration(estimator, world):
    """True when `CalibratedSVC` can solve every (fold, class) as one batched-SMO column on one panel and calibrate on the device
    (`bq_msmo_svc_heldout`): the estimator (an `SVC` or an `OneVsRestSVC`) is on `OneVsRestSVC`'s batched SMO path
    (`uses_batched_smo_path`), its panel is 'f64' and its kernel's gamma is not a string."""
    if not isinstance(estimator, (SVC, OneVsRestSVC)):
        return False
    proto = _prototype(estimator)
    return bool(not has_class_weight(proto) and uses_batched_smo_path(proto, world) and proto.storage == 'f64' and
                not isinstance(getattr(proto.kernel, 'gamma', None), str))


def _row_lists(splits):
    """per fold its training rows as an ascending row list, or None when a fold repeats a training or test row or trains on a row
    it tests: that is another problem than a row list's"""
    lists = []
    for tr, te in splits:
        rows = np.unique(tr)
        if len(rows) != len(tr) or len(np.unique(te)) != len(te) or len(np.intersect1d(rows, te)):
            return None
        lists.append(rows)
    return lists


def sigmoid_probabilities(F, A, B):
    """One classifier's class probabilities from its decision values F (t, or t x k) and sigmoids A, B (k entries): with one
    column [1 - p, p], p = 1 / (1 + exp(A f + B)); with more, the per-class p divided by their row sum, 1 / k where the sum is 0."""
    F = np.asarray(F, dtype=float)
    F = F.reshape(len(F), -1)
    with np.errstate(over='ignore'):
        P = 1. / (1. + np.exp(np.asarray(A, dtype=float) * F + np.asarray(B, dtype=float)))
    if P.shape[1] == 1:
        return np.hstack((1. - P, P))
    total = P.sum(axis=1)[:, np.newaxis]
    return np.divide(P, total, out=np.full_like(P, 1. / P.shape[1]), where=total != 0)


def assemble_probabilities(per_classifier):
    """The mean over the calibrated classifiers' probabilities (each t x classes)."""
    return np.mean(np.stack(per_classifier), axis=0)


def _check_held_out_once(splits, n):
    counts = np.zeros(n, dtype=np.int64)
    for _, te in splits:
        np.add.at(counts, te, 1)
    if not np.all(counts == 1):
        raise ValueError('ensemble=False needs test folds that partition the rows: every row held out exactly once')


class CalibratedSVC(ClassifierMixin, BaseEstimator):
    """Platt-calibrated probabilities of an `SVC` (two classes) or an `OneVsRestSVC`, as sklearn's
    `CalibratedClassifierCV(estimator, method='sigmoid', cv=cv, ensemble=ensemble)`.  An int `cv` is StratifiedKFold(cv) without
    shuffling.

    ensemble=True: one classifier per fold, fitted on its training rows, and per class one sigmoid fitted on the fold's held-out
    decision values; `predict_proba` is the mean of the folds' probabilities.  ensemble=False: one sigmoid per class on the
    out-of-fold decision values of all rows (every row must be held out exactly once: else ValueError), and the classifier fitted
    on all the data.  A fold whose training rows miss a class raises ValueError on either path: its classifier has no column for
    that class.

    After `fit`: `classes_`; `calibrated_classifiers_`, a list of `CalibratedClassifier(estimator, A, B)`; `calibrators_`, a dict of
    the arrays A, B, iters, loss and flags of every sigmoid (shape (folds, classes) with ensemble=True, (classes,) without; one
    class column with two classes); `oof_decision_` (ensemble=False: n x classes, n with two classes); `batched_`, which says which
    path ran, and `batched_decision_`: `predict_proba` takes every (fold, class) decision value from one fused pass
    (`DecisionBatch`).  A sigmoid fit that ended on a failed line search or the iteration cap warns (`ConvergenceWarning`) and
    keeps the values reached.

    `smo_`: every (fold, class) fit was one column of the batched SMO solver, its row list the fold's training rows, calibrated on
    the device from the walkers' state (`uses_batched_smo_calibration`, `bq_msmo_svc_heldout`); `batched_` is True with it.
    `batch_smo` (None, True, False) forces that choice where the configuration allows it; None leaves it to the number of columns
    (`takes_batched_smo`).
    """
    batch_smo = None

    def __init__(self, estimator, cv=5, ensemble=True):
        self.estimator = estimator
        self.cv = cv
        self.ensemble = ensemble

    def fit(self, X, y):
        if not isinstance(self.estimator, (SVC, OneVsRestSVC)):
            raise TypeError('estimator must be an SVC or a OneVsRestSVC')
        X = np.ascontiguousarray(X, dtype=float)
        y = np.asarray(y)
        multiclass = isinstance(self.estimator, OneVsRestSVC)
        self.classes_, rows = _fold_labels(y, multiclass)
        if len(self.classes_) < 2:
            raise ValueError('the training data must hold at least two classes')
        splits = check_cv_splits(self.cv, X, y)
        if not self.ensemble:
            _check_held_out_once(splits, len(y))
        for f, (tr, _) in enumerate(splits):
            if not np.array_equal(_fold_labels(y[tr], multiclass)[0], self.classes_):
                raise ValueError('the training rows of fold %d miss a class' % f)
        world = get_context().world
        self.smo_ = False
        if uses_batched_smo_calibration(self.estimator, world) and _row_lists(splits) is not None:
            self.smo_ = takes_batched_smo((len(splits) + (0 if self.ensemble else 1)) * len(rows), self.batch_smo)
        self.batched_ = self.smo_ or uses_batched_calibration(self.estimator, world)
        fit = self._fit_batched_smo if self.smo_ else self._fit_batched if self.batched_ else self._fit_loop
        classifiers, cal, coefs = fit(X, y, splits, rows)
        kc = len(rows)
        shape = (len(splits), kc) if self.ensemble else (kc,)
        self.calibrators_ = {key: np.asarray(cal[key]).reshape(shape) for key in ('A', 'B', 'iters', 'loss', 'flags')}
        A, B = self.calibrators_['A'].reshape(-1, kc), self.calibrators_['B'].reshape(-1, kc)
        self.calibrated_classifiers_ = [CalibratedClassifier(est, A[i], B[i]) for i, est in enumerate(classifiers)]
        bad = np.argwhere(self.calibrators_['flags'] & (_lib.PLATT_LINE_SEARCH | _lib.PLATT_MAX_ITER))
        if len(bad):
            warnings.warn('the sigmoid fit of %d calibrator(s) ended on a failed line search or the iteration cap (first: %s)'
                          % (len(bad), tuple(int(i) for i in bad[0])), ConvergenceWarning)
        # one column suffices for the fused pass here (`uses_batched_decision` asks for two): the kernel's conditions decide
        kernel = _prototype(self.estimator).kernel
        self.batched_decision_ = uses_batched_decision(kernel, max(2, len(classifiers) * kc), world, self.batched_)
        self.decision_batch_ = None
        if self.batched_decision_:
            b = [e.intercept_ for est in classifiers for e in (est.estimators_ if multiclass else [est])]
            self.decision_batch_ = DecisionBatch(kernel, X, coefs, b)
        return self

    def _new(self):
        """A fresh, unfitted estimator of the configuration"""
        return _make(type(self.estimator), _base_params(self.estimator), {})

    def _fit_loop(self, X, y, splits, rows):
        """sklearn's calls: per fold `fit` on the training rows and `decision_function` on the held-out rows; the sigmoids through
        `bq_platt_fit`."""
        n, kc = len(y), len(rows)
        Ycls = np.stack([np.where(y == pos, 1., -1.) for pos in rows])
        classifiers = []
        if self.ensemble:
            D, L = np.zeros((len(splits) * kc, n)), np.zeros((len(splits) * kc, n))
        else:
            D, L = np.zeros((kc, n)), Ycls
        for f, (tr, te) in enumerate(splits):
            est = self._new().fit(X[tr], y[tr])
            F = np.asarray(est.decision_function(X[te]), dtype=float).reshape(len(te), -1)
            if self.ensemble:
                classifiers.append(est)
                D[f * kc:(f + 1) * kc, te] = F.T
                L[f * kc:(f + 1) * kc, te] = Ycls[:, te]
            else:
                D[:, te] = F.T
        if not self.ensemble:
            classifiers.append(self._new().fit(X, y))
            self.oof_decision_ = D[0].copy() if kc == 1 else D.T.copy()
        return classifiers, platt_fit(D, L), None

    def _fit_batched(self, X, y, splits, rows):
        """One panel of all n rows; the columns (fold, class) with the fold's box and, for ensemble=False, (all, class) with
        ub = C everywhere, in solves of at most `column_cap` columns; intercepts, held-out decision values and sigmoids from the
        device (`heldout_svc`)."""
        multiclass = isinstance(self.estimator, OneVsRestSVC)
        proto = _prototype(self.estimator)
        n, kc, ns = len(y), len(rows), len(splits)
        Ycls = np.stack([np.where(y == pos, 1., -1.) for pos in rows])
        folds = list(range(ns)) + ([] if self.ensemble else [None])   # None: the fit on all the data
        cols = [(f, r) for f in folds for r in range(kc)]
        boxes = {None: np.full(n, float(proto.C))}
        for f, (tr, _) in enumerate(splits):
            boxes[f] = np.zeros(n)
            boxes[f][tr] = proto.C
        m = len(cols)
        obj = KernelQuadratic(X, -np.ones(n), 'svc', proto.kernel, y=Ycls[0], storage=proto.storage,
                              tune_placement=proto._streams_panel(), expected_products=proto.max_iter * ((m + 15) // 16))
        dev = obj.device_problem()
        cap = column_cap(n, device_free_bytes(), _lib.load().bq_problem_wide_slab_bytes(dev.handle))
        kind = solver_kind(proto.optimizer)
        ests, fits = [], []
        oof = None if self.ensemble else np.zeros((kc, n))
        for c0 in range(0, m, cap):
            chunk = cols[c0:c0 + cap]
            Y = np.stack([Ycls[r] for _, r in chunk])
            UB = np.stack([boxes[f] for f, _ in chunk])
            # ensemble: a calibrator per column; else a calibrator per class, fed by its fold columns (the rows of every class
            # are held out once over the folds, so a solve's columns of one class hold out disjoint rows)
            cal_of = np.arange(len(chunk)) if self.ensemble else np.array([-1 if f is None else r for f, r in chunk])
            ncal = len(chunk) if self.ensemble else kc
            held = {}
            # the columns that become estimators: every one with ensemble, else only those of the fit on all the data — the
            # fold columns there leave their held-out decision values and nothing else, and their x and g stay on the device
            kept = [j for j, (f, _) in enumerate(chunk) if self.ensemble or f is None]

            def score(solver, out):
                held['b'], held['n_sv'], held['fit'] = solver.heldout_svc(cal_of, ncal, decisions=not self.ensemble)
                if not self.ensemble:
                    for j in kept:
                        out[j].update(x=solver.get(j, _lib.GET_X_NOW), g=solver.get(j, _lib.GET_G_NOW))

            res = solve_batched(dev, kind, Y, UB, eps=1e-6, max_iter=proto.max_iter, before_close=score, vectors=self.ensemble)
            if not held['n_sv'].all():
                raise ZeroDivisionError('a fit ended without support vectors')   # as SVC.fit's intercept
            fits.append(held['fit'])
            if not self.ensemble:
                oof += held['fit']['dec']   # the chunks' rows are disjoint and 0 elsewhere
            for j in kept:
                f, r = chunk[j]
                est = _make(SVC, _base_params(proto), {})
                if f is None:
                    fitted_svc(est, obj, res[j], X, Ycls[r])
                else:
                    tr = splits[f][0]
                    fitted_svc(est, obj, res[j], X[tr], Ycls[r][tr], pos=tr)
                est.intercept_ = float(held['b'][j])
                if not multiclass:
                    est.classes_ = self.classes_
                ests.append((f, est))
        del dev, obj
        if self.ensemble:
            cal = {key: np.concatenate([fit[key] for fit in fits]) for key in fits[0] if key != 'dec'}
        elif len(fits) == 1:
            cal = fits[0]   # every column of a class in one solve: the sigmoids came from the device's own buffers
        else:
            cal = platt_fit(oof, Ycls)   # a class's folds were spread over several solves: the same kernel on the gathered rows
        if not self.ensemble:
            self.oof_decision_ = oof[0].copy() if kc == 1 else oof.T.copy()
        # the (fold, class) estimators into one classifier per fold
        classifiers, coefs = [], []
        for f in folds if self.ensemble else [None]:
            mine = [est for g, est in ests if g == f]
            tr = np.arange(n) if f is None else splits[f][0]
            for est in mine:
                w = np.zeros(n)
                w[tr[est.support_]] = est.dual_coef_
                coefs.append(w)
            classifiers.append(self._one_vs_rest(mine) if multiclass else mine[0])
        return classifiers, cal, np.stack(coefs)

    def _fit_batched_smo(self, X, y, splits, rows):
        """One unsorted panel of all n rows, built as `SVCGridSearchCV`'s SMO search builds it; the columns (fold, class) with the
        fold's training rows as row list, in solves of at most `smo_heldout_column_cap` columns, scored where the walkers' state
        lives (`svc_heldout`, one set per fold: intercepts, held-out decision values and sigmoids from the device) and, for
        ensemble=False, the columns (all, class) without a list, one `solve_batched_smo` as `OneVsRestSVC` runs it.  An SMO fit
        without support vectors is not an error: its intercept is the solver's."""
        multiclass = isinstance(self.estimator, OneVsRestSVC)
        proto = _prototype(self.estimator)
        n, kc, ns = len(y), len(rows), len(splits)
        Ycls = np.stack([np.where(y == pos, 1., -1.) for pos in rows])
        lists = _row_lists(splits)
        held = np.zeros((ns, n), dtype=np.uint8)
        for f, (_, te) in enumerate(splits):
            held[f, te] = 1
        cols = [(f, r) for f in range(ns) for r in range(kc)]
        obj = KernelQuadratic(X, -np.ones(n), 'svc', proto.kernel, y=Ycls[0], storage=proto.storage, rank_one=False, compact=False)
        ests, fits = [], []
        oof = None if self.ensemble else np.zeros((kc, n))
        try:
            dev = obj.device_problem()
            cap = smo_heldout_column_cap(n, _lib.SVC, device_free_bytes(), _lib.load().bq_problem_wide_slab_bytes(dev.handle),
                                         calibrators=self.ensemble)
            for c0 in range(0, len(cols), cap):
                chunk = cols[c0:c0 + cap]
                # ensemble: a calibrator per column; else a calibrator per class, fed by its fold columns (the rows of every class
                # are held out once over the folds, so a solve's columns of one class score disjoint rows)
                cal_of = np.arange(len(chunk)) if self.ensemble else np.array([r for _, r in chunk])
                ncal = len(chunk) if self.ensemble else kc
                solver = _DeviceSMOSolver(dev, _lib.SVC, np.stack([Ycls[r] for _, r in chunk]), proto.C, None, proto.tol,
                                          rows=[lists[f] for f, _ in chunk])
                try:
                    outer, failed = run_batched_smo(solver)
                    if failed.any():
                        raise smo_failed_error()
                    _, _, fit = solver.svc_heldout([f for f, _ in chunk], held, cal_of, ncal, decisions=not self.ensemble)
                    # the columns that become estimators: every one with ensemble; else the fold columns leave their held-out
                    # decision values and nothing else
                    res = [smo_column_result(solver, j, outer[j]) for j in range(len(chunk))] if self.ensemble else []
                finally:
                    solver.close()
                fits.append(fit)
                if not self.ensemble:
                    oof += fit['dec']   # the chunks' rows are disjoint and 0 elsewhere
                for (f, r), res_j in zip(chunk, res):
                    tr = lists[f]
                    # the column's n-long state on the fold's rows; the threshold rows as positions among them
                    res_j['alphas'], res_j['errors'] = res_j['alphas'][tr], res_j['errors'][tr]
                    res_j['b_up_idx'], res_j['b_low_idx'] = (int(np.searchsorted(tr, res_j[name])) for name in ('b_up_idx', 'b_low_idx'))
                    est = _make(SVC, _base_params(proto), {})
                    fitted_smo_svc(est, obj, res_j, X[tr], Ycls[r][tr])
                    ests.append((f, est))
            if not self.ensemble:
                for r, res_r in enumerate(solve_batched_smo(dev, _lib.SVC, Ycls, proto.C, None, proto.tol)):
                    est = _make(SVC, _base_params(proto), {})
                    fitted_smo_svc(est, ClassQuadratic(obj, Ycls[r]), res_r, X, Ycls[r])
                    ests.append((None, est))
        except BaseException:
            obj.release()   # nothing keeps the panel: the estimators that would are dropped with this frame
            raise
        del dev
        if self.ensemble:
            cal = {key: np.concatenate([fit[key] for fit in fits]) for key in fits[0] if key != 'dec'}
        elif len(fits) == 1:
            cal = fits[0]   # every column of a class in one solve: the sigmoids came from the device's own buffers
        else:
            cal = platt_fit(oof, Ycls)   # a class's folds were spread over several solves: the same kernel on the gathered rows
        if not self.ensemble:
            self.oof_decision_ = oof[0].copy() if kc == 1 else oof.T.copy()
        classifiers, coefs = [], []
        for f in list(range(ns)) if self.ensemble else [None]:
            mine = [est for g, est in ests if g == f]
            tr = np.arange(n) if f is None else lists[f]
            for est in mine:
                if not multiclass:
                    est.classes_ = self.classes_
                w = np.zeros(n)
                w[tr[est.support_]] = est.dual_coef_
                coefs.append(w)
            classifiers.append(self._one_vs_rest(mine, smo=True) if multiclass else mine[0])
        return classifiers, cal, np.stack(coefs)

    def _one_vs_rest(self, ests, smo=False):
        """The `OneVsRestSVC` that a batched `fit` on a fold's rows leaves, from its per-class estimators.  It predicts through
        one call per estimator: a decision batch of its own would hold a second copy of its support rows beside the one
        `decision_batch_` of all folds that `predict_proba` uses."""
        ovr = self._new()
        ovr.classes_ = self.classes_
        ovr.estimators_ = ests
        ovr.lagrangian_, ovr.smo_, ovr.batched_ = False, smo, True
        ovr.batched_decision_, ovr.decision_batch_ = False, None
        return ovr

    def _decisions(self, X):
        """t x (classifiers * classes) decision values, classifier-major"""
        X = np.ascontiguousarray(X, dtype=float)
        if self.batched_decision_:
            return self.decision_batch_(X)
        return np.hstack([np.asarray(c.estimator.decision_function(X), dtype=float).reshape(len(X), -1)
                          for c in self.calibrated_classifiers_])

    def predict_proba(self, X):
        F = self._decisions(X)
        kc = len(self.calibrated_classifiers_[0].A)
        return assemble_probabilities([sigmoid_probabilities(F[:, i * kc:(i + 1) * kc], c.A, c.B)
                                       for i, c in enumerate(self.calibrated_classifiers_)])

    def predict(self, X):
        return self.classes_[np.argmax(self.predict_proba(X), axis=1)]
