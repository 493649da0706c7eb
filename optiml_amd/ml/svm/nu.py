"""nu-SVC and nu-SVR (Schoelkopf et al.; `sklearn.svm.NuSVC`, `sklearn.svm.NuSVR`; libsvm's `solve_nu_svc` / `solve_nu_svr`), their
duals solved on the resident Gram panel.

Both duals carry two equality rows, sum_j s_j x_j = 0 and sum_j x_j = R, which together say that the variables with s = +1 and
those with s = -1 sum to R / 2 each: the feasible set is the product of two capped simplices over disjoint groups of variables,
and its Euclidean projection is the two projections taken independently.  The device solver (`bq_msolver_create_simplex2`,
csrc/bq_simplex.hip) is `OneClassSVM`'s nonmonotone spectral projected-gradient iteration around that projection, with the
signed gradient g_j = q_j + s_j (K b)_{j mod n}, b the signed, folded x, and one n x n panel product per iteration:

  NuSVC  x = alpha (n), s = y, box 1, each class's mass nu n / 2, q = 0
  NuSVR  x = (alpha, alpha*) (2n), s = (+1, -1), box C, each half's mass C nu n / 2, q = (-y, y)

It stops on libsvm's `Solver_NU` measure (the larger of the two groups' maximal-violating-pair values), so `tol` means what
sklearn's `tol` means — of the unscaled dual: NuSVC's decision function is that dual's divided by r = (r1 + r2) / 2, and its
values move by tol / r.  The offsets r1, r2 are libsvm's `Solver_NU::calculate_rho`.

Several parameters on the same data (`nu_svc_path`, `nu_svr_path`) are columns of ONE solve: one panel stream per iteration for
every 16 columns still running.  A single `fit` is the one-column case of the same code, and a column's bits do not depend on the
other columns.
"""
import warnings

import numpy as np

from ... import _lib
from ...device import get_context
from ...opti import KernelQuadratic
from ._base import ClassifierMixin, ConvergenceWarning, RegressorMixin
from ._batched import _DeviceSimplex2Solver, column_cap, device_free_bytes, solve_batched
from .kernels import BaseEstimator, Kernel, gaussian
from .oneclass import _resolved

__all__ = ['NuSVC', 'NuSVR', 'nu_svc_path', 'nu_svr_path']


def _check(kernel, nu, tol, max_iter, storage, C=1.0):
    if not isinstance(kernel, Kernel):
        raise TypeError(f'{kernel} is not an allowed kernel function')
    if not 0 < nu <= 1:
        raise ValueError('nu must be in (0, 1]')
    if not C > 0:
        raise ValueError('C must be > 0')
    if not tol >= 0:
        raise ValueError('tol must be >= 0')
    if not max_iter > 0:
        raise ValueError('max_iter must be > 0')
    if storage not in _lib.STORAGE:
        raise ValueError(f'unknown storage {storage}')


def _check_feasible(y, nu):
    """libsvm's check of nu-SVC (svm_check_parameter): each class must be able to hold its mass nu n / 2.  y: +-1."""
    n_pos, n_neg = int((y > 0).sum()), int((y < 0).sum())
    if nu * (n_pos + n_neg) / 2 > min(n_pos, n_neg):
        raise ValueError('specified nu is infeasible')


def _solve(proto, X, S, UB, mass, q):
    """The k two-group columns (S, UB, mass, q: `_DeviceSimplex2Solver`'s) on one panel of X, in solves of at most `column_cap`
    columns: (kernel_, [(column result, r1, r2), ...])."""
    name = type(proto).__name__
    if proto.storage == 'stream':
        raise NotImplementedError(f'{name} needs a resident panel: storage \'f64\' or \'f32\'')
    if get_context().world != 1:
        raise NotImplementedError(f'{name} runs on a single-rank context')
    n, k = X.shape[0], UB.shape[0]
    kernel = _resolved(proto.kernel, X)
    obj = KernelQuadratic(X, np.zeros(n), 'plain', kernel, storage=proto.storage, tune_placement=bool(proto.tune_placement),
                          expected_products=proto.max_iter * ((k + 15) // 16))
    try:
        dev = obj.device_problem()
        cap = column_cap(n, device_free_bytes(), _lib.load().bq_problem_wide_slab_bytes(dev.handle))
        if UB.shape[1] == 2 * n:   # (a column of 2n variables holds twice the vectors the cap counts)
            cap = max(1, cap // 2)
        out = []
        for c0 in range(0, k, cap):
            sl = slice(c0, c0 + cap)
            held = {}

            def offsets(solver, _):
                held['r1'], held['r2'], _, _ = solver.offsets()

            solver = _DeviceSimplex2Solver(dev, None if S is None else S[sl], UB[sl], mass[sl], None if q is None else q[sl],
                                           proto.tol, proto.max_iter)
            res = solve_batched(dev, None, UB[sl], None, solver=solver, before_close=offsets)
            out.extend((r, float(held['r1'][j]), float(held['r2'][j])) for j, r in enumerate(res))
        return kernel, out
    finally:
        obj.release()


def _kernel_sum(kernel, sv, coef, intercept, X):
    """sum_i coef_i k(sv_i, X) + intercept on the device (`bq_decision_function`)."""
    X = np.ascontiguousarray(X, dtype=float)
    sv = np.ascontiguousarray(sv, dtype=float)
    kind, gamma, coef0, degree = kernel.device_spec(sv)   # (gamma is numeric: resolved at fit)
    out = np.empty(X.shape[0])
    coef = _lib.as_f64(coef, sv.shape[0], 'dual_coef_')
    _lib.check(_lib.load().bq_decision_function(get_context().handle, kind, gamma, coef0, degree, sv.shape[0], sv.shape[1],
                                                _lib.ptr(sv), _lib.ptr(coef), float(intercept), X.shape[0], _lib.ptr(X),
                                                _lib.ptr(out)))
    return out


class _NuBase(BaseEstimator):
    tune_placement = True   # as SVM.tune_placement: every iteration streams the panel

    def _solved(self, kernel, r):
        self.kernel_ = kernel
        self.alphas_ = r['x']
        self.n_iter_ = int(r['iter'])
        self.status_ = r['status']
        self.kkt_violation_ = float(r['rows']['r1'][-1]) if len(r['rows']) else np.nan
        self.train_loss_history = [float(f) for f in r['rows']['f']]
        if self.status_ == 'stopped':
            warnings.warn('max_iter reached but the optimization has not converged yet', ConvergenceWarning)

    def decision_function(self, X):
        return _kernel_sum(self.kernel_, self.support_vectors_, self.dual_coef_, self.intercept_, X)


class NuSVC(ClassifierMixin, _NuBase):
    """Binary nu-support-vector classification, as `sklearn.svm.NuSVC`: `nu` in (0, 1] bounds the fraction of margin errors from
    above and the fraction of support vectors from below; `tol` bounds libsvm's `Solver_NU` measure of the unscaled dual's
    optimality conditions; `kernel` is any of this package's five kernels; `storage` 'f64' or 'f32' is the dtype of the resident
    Gram panel ('stream' and multi-rank contexts raise NotImplementedError).  Labels map as in `SVC` (`classes_`; the larger label
    is +1); more than two classes raise `SVC`'s error, and a nu with nu n / 2 above the smaller class raises
    ValueError('specified nu is infeasible') before any device work.  A string `gamma` is resolved on the training X at `fit` and
    kept in `kernel_`, as `OneClassSVM` does.

    After `fit(X, y)`: `alphas_` (libsvm's unscaled alpha in [0, 1], each class summing to nu n / 2), `margin_scale_` (r: the
    decision function is the unscaled dual's divided by it), `support_` (the rows with alpha > 0, in index order),
    `support_vectors_`, `dual_coef_` (y alpha / r on the support rows), `intercept_` (-rho / r), `n_iter_`, `status_` ('optimal' /
    'stopped', the latter with a ConvergenceWarning), `kkt_violation_` and `train_loss_history`.

    The iteration count grows as r -> 0 (a small nu on noisy data: r of 1e-3 ... 1e-5 and thousands of iterations at tol 1e-6).
    That limits the speed, not the result: raise `max_iter`."""

    def __init__(self, kernel=gaussian, nu=0.5, tol=1e-3, max_iter=1000, storage='f64'):
        _check(kernel, nu, tol, max_iter, storage)
        self.kernel = kernel
        self.nu = nu
        self.tol = tol
        self.max_iter = max_iter
        self.storage = storage

    def _labels(self, y):
        y = np.asarray(y)
        self.classes_ = np.unique(y)
        if len(self.classes_) > 2:
            raise ValueError('use OneVsOneClassifier or OneVsRestClassifier from sklearn.multiclass '
                             'to train a model over more than two labels')
        if len(self.classes_) < 2:
            raise ValueError('NuSVC needs two classes')
        return np.where(y == self.classes_[-1], 1., -1.)

    def _fitted(self, X, y, kernel, r, r1, r2):
        self._solved(kernel, r)
        self.margin_scale_ = (r1 + r2) / 2
        sv = self.alphas_ > 0
        self.support_ = np.flatnonzero(sv)
        self.support_vectors_ = X[sv]
        self.dual_coef_ = (y * self.alphas_)[sv] / self.margin_scale_
        self.intercept_ = -((r1 - r2) / 2) / self.margin_scale_
        return self

    def fit(self, X, y):
        _check(self.kernel, self.nu, self.tol, self.max_iter, self.storage)   # set_params may have changed them
        X = np.ascontiguousarray(X, dtype=float)
        y = self._labels(y)
        _check_feasible(y, self.nu)
        n = X.shape[0]
        kernel, ((r, r1, r2),) = _solve(self, X, y[None, :], np.ones((1, n)), np.full((1, 2), self.nu * n / 2), None)
        return self._fitted(X, y, kernel, r, r1, r2)

    def predict(self, X):
        return np.where(self.decision_function(X) > 0, self.classes_[-1], self.classes_[0])


class NuSVR(RegressorMixin, _NuBase):
    """nu-support-vector regression, as `sklearn.svm.NuSVR`: `nu` in (0, 1] bounds the fraction of rows outside the tube from above
    and the fraction of support vectors from below, and the tube's width is found, not given (`epsilon_`); `C`, `tol`, `kernel`,
    `storage` and a string `gamma` as in `NuSVC`.

    After `fit(X, y)`: `alphas_` (2n: alpha, then alpha*, in [0, C], each half summing to C nu n / 2), `support_` (the rows with
    alpha != alpha*), `support_vectors_`, `dual_coef_` (alpha - alpha* on the support rows), `intercept_` (-rho), `epsilon_`
    (-(r1 + r2) / 2), `n_iter_`, `status_`, `kkt_violation_` and `train_loss_history`.

    The iteration count grows with C (C = 10 on 600 noisy rows takes several thousand iterations at tol 1e-6).  That limits the
    speed, not the result: raise `max_iter`."""

    def __init__(self, kernel=gaussian, nu=0.5, C=1.0, tol=1e-3, max_iter=1000, storage='f64'):
        _check(kernel, nu, tol, max_iter, storage, C)
        self.kernel = kernel
        self.nu = nu
        self.C = C
        self.tol = tol
        self.max_iter = max_iter
        self.storage = storage

    @staticmethod
    def _columns(y, params):
        """UB, mass, q of the columns (C, nu) of `params` on the targets y"""
        n = len(y)
        UB = np.stack([np.full(2 * n, float(C)) for C, _ in params])
        mass = np.array([[C * nu * n / 2] * 2 for C, nu in params], dtype=float)
        q = np.tile(np.concatenate((-y, y)), (len(params), 1))
        return UB, mass, q

    def _fitted(self, X, kernel, r, r1, r2):
        self._solved(kernel, r)
        n = X.shape[0]
        coef = self.alphas_[:n] - self.alphas_[n:]
        sv = coef != 0
        self.support_ = np.flatnonzero(sv)
        self.support_vectors_ = X[sv]
        self.dual_coef_ = coef[sv]
        self.intercept_ = -((r1 - r2) / 2)
        self.epsilon_ = -((r1 + r2) / 2)
        return self

    @staticmethod
    def _targets(X, y):
        y = np.asarray(y, dtype=float)
        if y.ndim > 1:
            raise ValueError('use MultiOutputSVR to train a model over more than one target')
        if y.shape[0] != X.shape[0]:
            raise ValueError('X and y have different numbers of rows')
        return y

    def fit(self, X, y):
        _check(self.kernel, self.nu, self.tol, self.max_iter, self.storage, self.C)
        X = np.ascontiguousarray(X, dtype=float)
        y = self._targets(X, y)
        kernel, ((r, r1, r2),) = _solve(self, X, None, *self._columns(y, [(self.C, self.nu)]))
        return self._fitted(X, kernel, r, r1, r2)

    def predict(self, X):
        return self.decision_function(X)


def _clones(estimator, params):
    return [type(estimator)(**dict(estimator.get_params(deep=False), **p)) for p in params]   # (as sklearn's clone constructs)


def nu_svc_path(estimator, X, y, nus):
    """A list of fitted clones of the `NuSVC` `estimator`, one per nu of `nus`, all solved as columns of one batched solve on one Gram
    panel of X (in several solves where the device memory does not hold all columns at once).  Each clone equals its own
    `NuSVC(nu=nu, ...).fit(X, y)` bit for bit."""
    nus = [float(nu) for nu in nus]
    ests = _clones(estimator, [dict(nu=nu) for nu in nus])
    X = np.ascontiguousarray(X, dtype=float)
    if not ests:
        return ests
    ys = [est._labels(y) for est in ests]
    for nu in nus:
        _check_feasible(ys[0], nu)
    n, k = X.shape[0], len(nus)
    mass = np.array([[nu * n / 2] * 2 for nu in nus], dtype=float)
    kernel, res = _solve(estimator, X, np.tile(ys[0], (k, 1)), np.ones((k, n)), mass, None)
    return [est._fitted(X, ys[0], kernel, r, r1, r2) for est, (r, r1, r2) in zip(ests, res)]


def nu_svr_path(estimator, X, y, params):
    """A list of fitted clones of the `NuSVR` `estimator`, one per (C, nu) of `params`, all solved as columns of one batched solve on
    one Gram panel of X.  Each clone equals its own `NuSVR(C=C, nu=nu, ...).fit(X, y)` bit for bit."""
    params = [(float(C), float(nu)) for C, nu in params]
    ests = _clones(estimator, [dict(C=C, nu=nu) for C, nu in params])
    X = np.ascontiguousarray(X, dtype=float)
    if not ests:
        return ests
    y = NuSVR._targets(X, y)
    kernel, res = _solve(estimator, X, None, *NuSVR._columns(y, params))
    return [est._fitted(X, kernel, r, r1, r2) for est, (r, r1, r2) in zip(ests, res)]
