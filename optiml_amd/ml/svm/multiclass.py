"""One-vs-rest multi-class SVC: the result of sklearn's `OneVsRestClassifier(SVC(**kw))`, with the k binary duals solved
together on ONE Gram panel.

The panel does not depend on the labels: for the 'svc' structure class c's Hessian is Q_c = diag(y_c) (K + 1) diag(y_c), so every
first-order iteration of every class is a product with the same K + 1.  The batched path (`bq_msolver_*`) streams the panel once
per iteration for every 4 classes still running (bq_symm.hip) instead of once per class, and takes the intercepts' k masked
products in one multi-column product (`bq_problem_gram_matmat`).  Each class follows the iteration of `SVC.fit` with the same
optimizer — same formulas, thresholds, stop tests and records — and its iterates have the same bits whatever the other classes do.

The augmented-Lagrangian branch of `SVC.fit` (a stochastic optimizer: the unregularised intercept's equality row, the squared
hinge) is batched the same way (`uses_batched_lagrangian_path`, `bq_msolver_create_al`): every class is the solver of the single fit,
started where that fit starts, and equals it to rounding — the 4-column product sums in another order than the one-column one.

Configurations neither batched path covers fit the k binary problems one after another with `SVC`: exactly what
`OneVsRestClassifier(SVC)` does.
"""
import numpy as np

from ...device import get_context
from ...opti import KernelQuadratic
from ...opti.constrained import FrankWolfe, ProjectedGradient
from ... import _lib
from ._batched import (ClassQuadratic, DecisionBatch, _DeviceALSolver, _DeviceMultiSolver, _MultiClassSVC, _gram_matmat,
                       _svc_attributes, fitted_lagrangian, fitted_smo_svc, fitted_svc, intercept, lagrangian_columns,
                       solve_batched, solve_batched_al, solve_batched_smo, solver_kind, takes_batched_smo, uses_batched_decision,
                       uses_batched_lagrangian, uses_batched_smo)
from ._base import has_class_weight, row_boxes
from .losses import Hinge, SquaredHinge

__all__ = ['OneVsRestSVC', 'uses_batched_path', 'uses_batched_lagrangian_path', 'uses_batched_smo_path', 'binarize']


def uses_batched_path(svc, world):
    """True when `OneVsRestSVC` solves the classes of `svc`'s configuration together on one panel: the hinge dual with a regularised
    intercept by ProjectedGradient or FrankWolfe, a resident panel ('f64' / 'f32') and a single-rank context (`world` ranks).
    Every other configuration, and every one with a `class_weight` (the batched solver's columns share one box), fits one `SVC`
    per class."""
    opt = svc.optimizer
    return bool(not has_class_weight(svc) and svc.dual and svc.reg_intercept and svc.loss == Hinge and isinstance(opt, type) and
                issubclass(opt, (ProjectedGradient, FrankWolfe)) and svc.storage in ('f64', 'f32') and int(world) == 1)


def uses_batched_lagrangian_path(svc, world, ndim=None):
    """True when `OneVsRestSVC` solves the classes of `svc`'s configuration together on one panel by the batched
    augmented-Lagrangian solver: `dual`, a `StochasticOptimizer` subclass, `momentum_type` 'none' or 'polyak' (constant momentum),
    the hinge or squared hinge loss, a resident panel ('f64' / 'f32'), a single-rank context (`world` ranks), either intercept;
    ndim (the number of samples, when given): more than 3, as the optimizers run step by step on smaller duals."""
    return uses_batched_lagrangian(svc, (Hinge, SquaredHinge), world, ndim)


def uses_batched_smo_path(svc, world):
    """True when `OneVsRestSVC` can solve the classes of `svc`'s configuration together by the batched SMO solver (`bq_msmo_*`, one
    walker workgroup per class on one panel): `dual`, optimizer 'smo' or `SMO`, the hinge loss, `reg_intercept=False`, a resident
    panel ('f64' / 'f32') and a single-rank context (`world` ranks).  Whether a fit then does is a matter of speed alone
    (`takes_batched_smo`): both ways give the same bits.  A `class_weight` stays on this path: every class's column gets the boxes
    of its own binary problem (`bq_msmo_create_weighted`)."""
    return uses_batched_smo(svc, Hinge, world, weighted=True)


def binarize(y):
    """(classes_, Y): classes_ = np.unique(y) and Y[c] = +1 where y == classes_[c], -1 elsewhere (the labels OneVsRestClassifier
    hands SVC.fit after its LabelBinarizer, mapped as SVC maps them); with two classes the single row of classes_[1]."""
    y = np.asarray(y)
    classes = np.unique(y)
    if len(classes) < 2:
        raise ValueError('the training data must hold at least two classes')
    rows = classes[1:] if len(classes) == 2 else classes
    Y = np.stack([np.where(y == c, 1., -1.) for c in rows])
    return classes, Y


class OneVsRestSVC(_MultiClassSVC):
    """One-vs-rest multi-class SVC; constructor arguments and their checks are SVC's.

    After `fit`: `classes_`, `estimators_` (one fitted SVC per class — per binary problem with two classes), `batched_` (the
    classes were solved together) with `lagrangian_` (by the augmented-Lagrangian solver, not ProjectedGradient / FrankWolfe), and
    `decision_function` (m x k; 1-D with two classes), `predict`, `score` as sklearn's OneVsRestClassifier(SVC(**kw)).

    `batched_decision_`: True when `decision_function` and `predict` take every class's values from one fused pass over the kernel
    values of the union of the support vectors (`uses_batched_decision`) instead of one call per estimator.  The stored batch
    (`decision_batch_`) describes the estimators as `fit` left them.

    `smo_`: the classes were solved together by the batched SMO solver (`uses_batched_smo_path`).  `batch_smo` (None, True,
    False) forces that choice where the configuration allows it; None leaves it to the number of classes (`takes_batched_smo`).
    """
    batch_smo = None

    def fit(self, X, y):
        X = np.ascontiguousarray(X, dtype=float)
        self.classes_, Y = binarize(y)
        proto = self._prototype()
        if isinstance(proto.class_weight, dict):
            # every class is fitted on the labels 0 / 1 of its own binary problem: a dict's keys, the data's labels, name none of them
            raise ValueError("OneVsRestSVC takes class_weight=None or 'balanced': the binary problems' labels are not the data's")
        self.lagrangian_ = uses_batched_lagrangian_path(proto, get_context().world, X.shape[0])
        self.smo_ = uses_batched_smo_path(proto, get_context().world) and takes_batched_smo(len(Y), self.batch_smo)
        self.batched_ = self.lagrangian_ or self.smo_ or uses_batched_path(proto, get_context().world)
        self.batched_decision_ = uses_batched_decision(proto.kernel, len(Y), get_context().world, self.batched_)
        self.decision_batch_ = None
        if not self.batched_:
            self.estimators_ = [self._prototype().fit(X, (Yc > 0).astype(int)) for Yc in Y]
            return self
        fit = self._fit_smo if self.smo_ else self._fit_lagrangian if self.lagrangian_ else self._fit_batched
        self.estimators_ = fit(proto, X, Y)
        return self

    def _fit_smo(self, proto, X, Y):
        """SVC.fit's SMO branch for every class on one panel: its KernelQuadratic (rank_one=False, compact=False), one batched
        solve; the intercepts are the solver's."""
        k, n = Y.shape
        obj = KernelQuadratic(X, -np.ones(n), 'svc', proto.kernel, y=Y[0], storage=proto.storage, rank_one=False, compact=False)
        # class_weight='balanced': column c's boxes are those SVC.fit gives the 0 / 1 labels of class c's binary problem
        boxes = None
        if has_class_weight(proto):
            boxes = np.stack([row_boxes(proto.C, (Yc > 0).astype(int), np.arange(2), proto.class_weight) for Yc in Y])
        res = solve_batched_smo(obj.device_problem(), _lib.SVC, Y, proto.C, None, proto.tol, boxes=boxes)
        ests = [self._prototype() for _ in range(k)]
        coefs = []
        for c, est in enumerate(ests):
            sv = fitted_smo_svc(est, ClassQuadratic(obj, Y[c]), res[c], X, Y[c], None if boxes is None else boxes[c])
            w = np.zeros(n)
            w[sv] = est.dual_coef_
            coefs.append(w)
            if self.verbose:
                print('class %r: %d outer iterations, %d pair steps' % (self.classes_[c if len(self.classes_) > 2 else 1],
                                                                        est.optimizer.iter, est.optimizer.steps))
        if self.batched_decision_:
            self.decision_batch_ = DecisionBatch(proto.kernel, X, coefs, [est.intercept_ for est in ests])
        return ests

    def _fit_batched(self, proto, X, Y):
        k, n = Y.shape
        ub = np.ones(n) * proto.C
        # one panel for every class: the 'svc' structure's own labels are never used by the batched solver
        obj = KernelQuadratic(X, -np.ones(n), 'svc', proto.kernel, y=Y[0], storage=proto.storage,
                              tune_placement=proto._streams_panel(), expected_products=proto.max_iter * ((k + 3) // 4))
        dev = obj.device_problem()
        kind = solver_kind(proto.optimizer)
        # the solver is created here, as OneVsOneSVC creates its pair solver, and handed over: solve_batched's own eps / max_iter
        # are not read on this call
        res = solve_batched(dev, kind, Y, ub, solver=_DeviceMultiSolver(dev, kind, Y, ub, 1e-6, proto.max_iter))
        return self._finish(proto, obj, X, Y, [self._prototype() for _ in range(k)],
                            lambda c, est: fitted_svc(est, obj, res[c], X, Y[c]))

    def _fit_lagrangian(self, proto, X, Y):
        """SVC.fit's stochastic branch for every class on one panel: its KernelQuadratic (diag = 1/(2C) for the squared hinge,
        rank_one = reg_intercept), per class the objective and optimizer it constructs, one batched solve."""
        k, n = Y.shape
        sq = proto.loss == SquaredHinge
        obj = KernelQuadratic(X, -np.ones(n), 'svc', proto.kernel, y=Y[0], storage=proto.storage,
                              diag=1. / (2 * proto.C) if sq else 0., rank_one=proto.reg_intercept,
                              tune_placement=proto._streams_panel(), expected_products=proto.max_iter * ((k + 3) // 4))
        dev = obj.device_problem()
        ests = [self._prototype() for _ in range(k)]
        ub = None if sq else np.ones(n) * proto.C
        a = None if proto.reg_intercept else Y
        cols, x0, dual0 = lagrangian_columns(ests, [ClassQuadratic(obj, Yc) for Yc in Y], a, ub)
        res = solve_batched_al(_DeviceALSolver(dev, cols[0][1]._params(), x0, Y=Y, a=a, lb=np.zeros(n), ub=ub, dual0=dual0))

        def fitted(c, est):
            fitted_lagrangian(est, *cols[c], res[c])
            return _svc_attributes(est, X, Y[c])
        return self._finish(proto, obj, X, Y, ests, fitted)

    def _finish(self, proto, obj, X, Y, ests, fitted):
        """The estimators from their columns' results (`fitted(c, est)`: the support mask), the intercepts from one multi-column
        product, the decision batch."""
        k, n = Y.shape
        dev = obj.device_problem()
        masks, coefs = [], []
        for c, est in enumerate(ests):
            sv = fitted(c, est)
            w = np.zeros(n)
            w[sv] = est.dual_coef_
            masks.append(sv)
            coefs.append(w)
            if self.verbose:
                print('class %r: %s after %d iterations, f = %1.6e' % (self.classes_[c if len(self.classes_) > 2 else 1],
                                                                         est.optimizer.status, est.optimizer.iter,
                                                                         est.optimizer.f_x))
        U = _gram_matmat(dev, np.stack(coefs))
        for c, est in enumerate(ests):
            est.intercept_ = intercept(Y[c], U[c], masks[c])
        if self.batched_decision_:
            self.decision_batch_ = DecisionBatch(proto.kernel, X, coefs, [est.intercept_ for est in ests])
        return ests

    def decision_function(self, X):
        if self.batched_decision_:
            return self.decision_batch_(X)   # k >= 2 columns: more than two classes
        scores = np.stack([e.decision_function(X) for e in self.estimators_], axis=1)
        return scores[:, 0] if len(self.classes_) == 2 else scores

    def predict(self, X):
        scores = self.decision_function(X)
        if len(self.classes_) == 2:
            return self.classes_[(scores > 0).astype(int)]
        return self.classes_[np.argmax(scores, axis=1)]
