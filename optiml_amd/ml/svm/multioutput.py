"""Multi-output SVR: the result of sklearn's `MultiOutputRegressor(SVR(**kw))`, with the k duals solved together on ONE Gram panel.

The panel of the 'svr' structure is K (+ 1 for the regularised intercept) and depends on neither the targets nor epsilon: target c
differs only in the linear term q_c = [-y_c; y_c] + epsilon.  The batched path (`bq_msolver_create_svr`) streams the panel once per
iteration for every 4 targets still running (bq_symm.hip) instead of once per target, and takes the intercepts' k masked products in
one multi-column product (`bq_problem_gram_matmat`).  Each target follows the iteration of `SVR.fit` with the same optimizer — same
formulas, thresholds, stop tests and records — and its iterates have the same bits whatever the other targets do.

The augmented-Lagrangian branch of `SVR.fit` (a stochastic optimizer: the unregularised intercept's equality row, the squared
epsilon-insensitive loss) is batched the same way (`uses_batched_lagrangian_svr_path`, `bq_msolver_create_al`): every target is the
solver of the single fit, started where that fit starts, and equals it to rounding — the 4-column product sums in another order
than the one-column one.

Configurations neither batched path covers fit the k targets one after another with `SVR`: exactly what
`MultiOutputRegressor(SVR)` does.
"""
import numpy as np

from ...device import get_context
from ...opti import KernelQuadratic
from ...opti.constrained import FrankWolfe, ProjectedGradient
from ... import _lib
from ._base import has_class_weight
from ._batched import (DecisionBatch, TargetQuadratic, _DeviceALSolver, _DeviceSVRSolver, _MultiTargetSVR, _gram_matmat,
                       _svr_attributes, fitted_lagrangian, fitted_smo_svr, fitted_svr, lagrangian_columns, solve_batched,
                       solve_batched_al, solve_batched_smo, solver_kind, svr_intercept, takes_batched_smo, uses_batched_decision,
                       uses_batched_lagrangian, uses_batched_smo)
from .losses import EpsilonInsensitive, SquaredEpsilonInsensitive

__all__ = ['MultiOutputSVR', 'uses_batched_svr_path', 'uses_batched_lagrangian_svr_path', 'uses_batched_smo_svr_path']


def uses_batched_svr_path(svr, world):
    """True when `MultiOutputSVR` solves the targets of `svr`'s configuration together on one panel: the epsilon-insensitive dual
    with a regularised intercept by ProjectedGradient or FrankWolfe, a resident panel ('f64' / 'f32') and a single-rank context
    (`world` ranks).  Every other configuration fits one `SVR` per target."""
    opt = svr.optimizer
    return bool(not has_class_weight(svr) and svr.dual and svr.reg_intercept and svr.loss == EpsilonInsensitive and isinstance(opt, type) and
                issubclass(opt, (ProjectedGradient, FrankWolfe)) and svr.storage in ('f64', 'f32') and int(world) == 1)


def uses_batched_lagrangian_svr_path(svr, world, ndim=None):
    """True when `MultiOutputSVR` solves the targets of `svr`'s configuration together on one panel by the batched
    augmented-Lagrangian solver: `dual`, a `StochasticOptimizer` subclass, `momentum_type` 'none' or 'polyak' (constant momentum),
    the epsilon-insensitive or squared epsilon-insensitive loss, a resident panel ('f64' / 'f32'), a single-rank context (`world`
    ranks), either intercept; ndim (the dual's 2n variables, when given): more than 3, as the optimizers run step by step on
    smaller duals."""
    return uses_batched_lagrangian(svr, (EpsilonInsensitive, SquaredEpsilonInsensitive), world, ndim)


def uses_batched_smo_svr_path(svr, world):
    """True when `MultiOutputSVR` can solve the targets of `svr`'s configuration together by the batched SMO solver (`bq_msmo_*`,
    one walker workgroup per target on one panel): `dual`, optimizer 'smo' or `SMO`, the epsilon-insensitive loss,
    `reg_intercept=False`, a resident panel ('f64' / 'f32') and a single-rank context (`world` ranks).  Whether a fit then does is
    a matter of speed alone (`takes_batched_smo`): both ways give the same bits."""
    return uses_batched_smo(svr, EpsilonInsensitive, world)


class MultiOutputSVR(_MultiTargetSVR):
    """Multi-output SVR; constructor arguments and their checks are SVR's.

    After `fit(X, Y)`, Y of shape n x k: `estimators_` (one fitted SVR per target), `batched_` (the targets were solved together)
    with `lagrangian_` (by the augmented-Lagrangian solver, not ProjectedGradient / FrankWolfe), and `predict`
    (m x k), `score` as sklearn's MultiOutputRegressor(SVR(**kw)).  On the batched path the estimators share one device panel;
    each one's `obj` / `optimizer.f` is its own target's dual on it (`TargetQuadratic`).

    `batched_decision_`: True when `predict` takes every target's values from one fused pass over the kernel values of the union
    of the support vectors (`uses_batched_decision`) instead of one call per estimator.  The stored batch (`decision_batch_`)
    describes the estimators as `fit` left them.

    `smo_`: the targets were solved together by the batched SMO solver (`uses_batched_smo_svr_path`).  `batch_smo` (None, True,
    False) forces that choice where the configuration allows it; None leaves it to the number of targets (`takes_batched_smo`).
    """
    batch_smo = None

    def fit(self, X, Y):
        X = np.ascontiguousarray(X, dtype=float)
        Y = np.asarray(Y, dtype=float)
        if Y.ndim == 1:
            raise ValueError('y must have at least two dimensions for multi-output regression but has only one.')
        proto = self._prototype()
        self.lagrangian_ = uses_batched_lagrangian_svr_path(proto, get_context().world, 2 * X.shape[0])
        self.smo_ = uses_batched_smo_svr_path(proto, get_context().world) and takes_batched_smo(Y.shape[1], self.batch_smo)
        self.batched_ = self.lagrangian_ or self.smo_ or uses_batched_svr_path(proto, get_context().world)
        self.batched_decision_ = uses_batched_decision(proto.kernel, Y.shape[1], get_context().world, self.batched_)
        self.decision_batch_ = None
        if not self.batched_:
            self.estimators_ = [self._prototype().fit(X, Y[:, c]) for c in range(Y.shape[1])]
            return self
        fit = self._fit_smo if self.smo_ else self._fit_lagrangian if self.lagrangian_ else self._fit_batched
        self.estimators_ = fit(proto, X, np.ascontiguousarray(Y.T))
        return self

    def _fit_smo(self, proto, X, Y):
        """SVR.fit's SMO branch for every target on one panel: its KernelQuadratic (rank_one=False, compact=False), one batched
        solve; the intercepts are the solver's."""
        k, n = Y.shape
        QL = np.hstack((-Y, Y)) + proto.epsilon   # row c: SVR.fit's q of target c
        obj = KernelQuadratic(X, QL[0], 'svr', proto.kernel, storage=proto.storage, rank_one=False, compact=False)
        res = solve_batched_smo(obj.device_problem(), _lib.SVR, Y, proto.C, proto.epsilon, proto.tol)
        ests = [self._prototype() for _ in range(k)]
        coefs = []
        for c, est in enumerate(ests):
            sv = fitted_smo_svr(est, TargetQuadratic(obj, QL[c]), res[c], X, Y[c])
            w = np.zeros(n)
            w[sv] = est.dual_coef_
            coefs.append(w)
            if self.verbose:
                print('target %d: %d outer iterations, %d pair steps' % (c, est.optimizer.iter, est.optimizer.steps))
        if self.batched_decision_:
            self.decision_batch_ = DecisionBatch(proto.kernel, X, coefs, [est.intercept_ for est in ests])
        return ests

    def _fit_batched(self, proto, X, Y):
        k, n = Y.shape
        ub = np.ones(2 * n) * proto.C
        QL = np.hstack((-Y, Y)) + proto.epsilon   # row c: SVR.fit's q of target c
        # one panel for every target: the 'svr' structure's own linear term is never used by the batched solver
        obj = KernelQuadratic(X, QL[0], 'svr', proto.kernel, storage=proto.storage, tune_placement=proto._streams_panel(),
                              expected_products=proto.max_iter * ((k + 3) // 4))
        dev = obj.device_problem()
        kind = solver_kind(proto.optimizer)
        res = solve_batched(dev, kind, QL, ub, solver=_DeviceSVRSolver(dev, kind, QL, ub, 1e-6, proto.max_iter))
        return self._finish(proto, obj, X, Y, [self._prototype() for _ in range(k)],
                            lambda c, est: fitted_svr(est, obj, res[c], X, Y[c]))

    def _fit_lagrangian(self, proto, X, Y):
        """SVR.fit's stochastic branch for every target on one panel: its KernelQuadratic (diag = 1/(2C) for the squared loss,
        rank_one = reg_intercept), per target the objective and optimizer it constructs, one batched solve."""
        k, n = Y.shape
        sq = proto.loss == SquaredEpsilonInsensitive
        QL = np.hstack((-Y, Y)) + proto.epsilon   # row c: SVR.fit's q of target c
        obj = KernelQuadratic(X, QL[0], 'svr', proto.kernel, storage=proto.storage, diag=1. / (2 * proto.C) if sq else 0.,
                              rank_one=proto.reg_intercept, tune_placement=proto._streams_panel(),
                              expected_products=proto.max_iter * ((k + 3) // 4))
        dev = obj.device_problem()
        ests = [self._prototype() for _ in range(k)]
        ub = None if sq else np.ones(2 * n) * proto.C
        e = None if proto.reg_intercept else np.hstack((np.ones(n), -np.ones(n)))   # equality row, the same for every target
        cols, x0, dual0 = lagrangian_columns(ests, [TargetQuadratic(obj, q) for q in QL], None if e is None else [e] * k, ub)
        res = solve_batched_al(_DeviceALSolver(dev, cols[0][1]._params(), x0, QL=QL, a=e, lb=np.zeros(2 * n), ub=ub, dual0=dual0))

        def fitted(c, est):
            fitted_lagrangian(est, *cols[c], res[c])
            return _svr_attributes(est, X, Y[c])
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
                print('target %d: %s after %d iterations, f = %1.6e' % (c, est.optimizer.status, est.optimizer.iter,
                                                                         est.optimizer.f_x))
        U = _gram_matmat(dev, np.stack(coefs))
        for c, est in enumerate(ests):
            est.intercept_ = svr_intercept(Y[c], U[c], masks[c], proto.epsilon)
        if self.batched_decision_:
            self.decision_batch_ = DecisionBatch(proto.kernel, X, coefs, [est.intercept_ for est in ests])
        return ests

    def predict(self, X):
        if self.batched_decision_:
            return self.decision_batch_(X)
        return np.stack([e.predict(X) for e in self.estimators_], axis=1)
