"""One-class SVM for novelty / outlier detection (Schoelkopf et al.; `sklearn.svm.OneClassSVM`), its nu-dual solved on the
resident Gram panel.

The dual is  min 1/2 a'Ka  s.t.  0 <= a_i <= 1, sum a = nu n  (libsvm's scaling: the solution is sklearn's `dual_coef_`).  Unlike
the SVC / SVR duals of this package its equality row cannot be regularised away — without it a = 0 is optimal — so the feasible
set is a capped simplex, and the device solver (`bq_msolver_create_simplex`, csrc/bq_simplex.hip) is a nonmonotone spectral
projected-gradient iteration around the Euclidean projection onto it.  It stops on libsvm's maximal-violating-pair measure, so `tol`
means what `sklearn.svm.OneClassSVM(tol=...)` means, and the offset rho is libsvm's `calculate_rho`.

Several nu on the same data (`one_class_nu_path`) are columns of ONE solve: one panel stream per iteration for every 16 nu still
running.  A single `fit` is the one-column case of the same code, and a column's bits do not depend on the other columns.
"""
import copy
import warnings

import numpy as np

from ... import _lib
from ...device import get_context
from ...opti import KernelQuadratic
from ._base import ConvergenceWarning
from ._batched import _DeviceSimplexSolver, column_cap, device_free_bytes, solve_batched
from .kernels import BaseEstimator, Kernel, gaussian

__all__ = ['OneClassSVM', 'one_class_nu_path']


def _check(kernel, nu, tol, max_iter, storage):
    if not isinstance(kernel, Kernel):
        raise TypeError(f'{kernel} is not an allowed kernel function')
    if not 0 < nu <= 1:
        raise ValueError('nu must be in (0, 1]')
    if not tol >= 0:
        raise ValueError('tol must be >= 0')
    if not max_iter > 0:
        raise ValueError('max_iter must be > 0')
    if storage not in _lib.STORAGE:
        raise ValueError(f'unknown storage {storage}')


def _resolved(kernel, X):
    """The kernel with a string gamma resolved on X (`model_selection._resolved_kernel`)."""
    if not isinstance(getattr(kernel, 'gamma', None), str):
        return kernel
    k = copy.copy(kernel)
    k.gamma = kernel.device_spec(X)[1]
    return k


def _solve(proto, X, nus):
    """The duals of every nu on one panel of X, in solves of at most `column_cap` columns: (kernel_, [(column result, rho), ...])."""
    if proto.storage == 'stream':
        raise NotImplementedError('OneClassSVM needs a resident panel: storage \'f64\' or \'f32\'')
    if get_context().world != 1:
        raise NotImplementedError('OneClassSVM runs on a single-rank context')
    n = X.shape[0]
    kernel = _resolved(proto.kernel, X)
    obj = KernelQuadratic(X, np.zeros(n), 'plain', kernel, storage=proto.storage, tune_placement=bool(proto.tune_placement),
                          expected_products=proto.max_iter * ((len(nus) + 15) // 16))
    try:
        dev = obj.device_problem()
        cap = column_cap(n, device_free_bytes(), _lib.load().bq_problem_wide_slab_bytes(dev.handle))
        out = []
        for c0 in range(0, len(nus), cap):
            chunk = nus[c0:c0 + cap]
            UB = np.ones((len(chunk), n))
            mass = np.array([nu * n for nu in chunk], dtype=float)
            held = {}

            def offsets(solver, _):
                held['rho'], _, _ = solver.offsets()

            res = solve_batched(dev, None, UB, None, solver=_DeviceSimplexSolver(dev, UB, mass, proto.tol, proto.max_iter),
                                before_close=offsets)
            out.extend((r, float(held['rho'][j])) for j, r in enumerate(res))
        return kernel, out
    finally:
        obj.release()


class OneClassSVM(BaseEstimator):
    """Unsupervised outlier detection, as `sklearn.svm.OneClassSVM`: `nu` in (0, 1] bounds the fraction of training errors from
    above and the fraction of support vectors from below; `tol` bounds libsvm's maximal-violating-pair measure of the dual's
    optimality conditions; `kernel` is any of this package's five kernels; `storage` 'f64' or 'f32' is the dtype of the resident
    Gram panel ('stream' and multi-rank contexts raise NotImplementedError).

    A string `gamma` ('scale' / 'auto') is resolved on the training X at `fit` and kept in `kernel_`, which every later call
    uses: sklearn's behaviour.  This is deliberately not `SVC.decision_function`'s way in this package, which follows the reference
    and resolves the string on the support vectors at prediction.

    After `fit(X)`: `alphas_` (n, 0 <= a <= 1, sum = nu n), `support_` (the rows with a > 0), `support_vectors_`, `dual_coef_` (1-D,
    the support rows' a), `offset_` (rho), `intercept_` (-rho), `n_iter_`, `status_` ('optimal' / 'stopped', the latter with a
    ConvergenceWarning), `kkt_violation_` (the measure at the last record) and `train_loss_history` (the records' dual values).
    `score_samples(X)` is sum_i a_i k(x_i, X), `decision_function` is that minus `offset_`, `predict` is +1 where it is > 0 and -1
    elsewhere.
    """

    tune_placement = True   # as SVM.tune_placement: every iteration streams the panel

    def __init__(self, kernel=gaussian, nu=0.5, tol=1e-3, max_iter=1000, storage='f64'):
        _check(kernel, nu, tol, max_iter, storage)
        self.kernel = kernel
        self.nu = nu
        self.tol = tol
        self.max_iter = max_iter
        self.storage = storage

    def _fitted(self, X, kernel, r, rho):
        self.kernel_ = kernel
        self.alphas_ = r['x']
        sv = self.alphas_ > 0
        self.support_ = np.flatnonzero(sv)
        self.support_vectors_ = X[sv]
        self.dual_coef_ = self.alphas_[sv]
        self.offset_ = rho
        self.intercept_ = -rho
        self.n_iter_ = int(r['iter'])
        self.status_ = r['status']
        self.kkt_violation_ = float(r['rows']['r1'][-1]) if len(r['rows']) else np.nan
        self.train_loss_history = [float(f) for f in r['rows']['f']]
        if self.status_ == 'stopped':
            warnings.warn('max_iter reached but the optimization has not converged yet', ConvergenceWarning)
        return self

    def fit(self, X, y=None):
        _check(self.kernel, self.nu, self.tol, self.max_iter, self.storage)   # set_params may have changed them
        X = np.ascontiguousarray(X, dtype=float)
        kernel, ((r, rho),) = _solve(self, X, [self.nu])
        return self._fitted(X, kernel, r, rho)

    def score_samples(self, X):
        X = np.ascontiguousarray(X, dtype=float)
        sv = np.ascontiguousarray(self.support_vectors_, dtype=float)
        kind, gamma, coef0, degree = self.kernel_.device_spec(sv)   # (gamma is numeric: resolved at fit)
        out = np.empty(X.shape[0])
        coef = _lib.as_f64(self.dual_coef_, sv.shape[0], 'dual_coef_')
        _lib.check(_lib.load().bq_decision_function(get_context().handle, kind, gamma, coef0, degree, sv.shape[0], sv.shape[1],
                                                    _lib.ptr(sv), _lib.ptr(coef), 0.0, X.shape[0], _lib.ptr(X), _lib.ptr(out)))
        return out

    def decision_function(self, X):
        return self.score_samples(X) - self.offset_

    def predict(self, X):
        return np.where(self.decision_function(X) > 0, 1, -1)

    def fit_predict(self, X, y=None):
        return self.fit(X).predict(X)


def one_class_nu_path(estimator, X, nus):
    """A list of fitted clones of `estimator`, one per nu of `nus`, all solved as columns of one batched solve on one Gram panel of
    X (in several solves where the device memory does not hold all columns at once).  Each clone equals its own
    `OneClassSVM(nu=nu, ...).fit(X)` bit for bit in `alphas_` and `offset_`."""
    nus = [float(nu) for nu in nus]
    ests = [type(estimator)(**dict(estimator.get_params(deep=False), nu=nu)) for nu in nus]   # (as sklearn's clone constructs)
    X = np.ascontiguousarray(X, dtype=float)
    if not ests:
        return ests
    kernel, res = _solve(estimator, X, nus)
    return [est._fitted(X, kernel, r, rho) for est, (r, rho) in zip(ests, res)]
