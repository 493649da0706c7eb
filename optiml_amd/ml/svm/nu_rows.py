"""Panel-free one-class SVM, nu-SVC and nu-SVR: libsvm's decomposition on kernel rows made on demand (`bq_rsmo_create_general`,
csrc/bq_rsmo.hip), for the sizes at which the resident panel of `OneClassSVM` / `NuSVC` / `NuSVR` no longer fits one device.

The three duals are libsvm's, from libsvm's starts (svm.cpp: solve_one_class, solve_nu_svc, solve_nu_svr):

  RowOneClassSVM  signs +1, lin 0, box 1; libsvm's Solver; the first floor(nu n) alpha are 1, the next is the remainder
  RowNuSVC        signs y, lin 0, box 1; Solver_NU; each class is filled in index order with min(1, remaining) from nu n / 2
  RowNuSVR        2n variables (alpha, alpha*), signs (+1, -1), lin (-y, y), box C; Solver_NU; both halves are filled in index order
                  with min(C, remaining) from C nu n / 2

The start gradient of a nonzero start is one streamed Gram product; every step then computes (or finds in an LRU cache of
`cache_rows` rows, 0 = as many as fit) the kernel rows it touches.  `tol` is libsvm's (sklearn's): the run ends when the largest
violation over the pair sets — for Solver_NU the larger of the two signs' — is below it.  The algorithm is NOT the spectral
projected gradient of the resident classes: same dual, same optimum, different trajectories.  Prediction is the resident classes'.

Batched (`RowSMOBatch` with `GeneralRowSMO` columns, `bq_mrsmo_create_general` / `_create_lists_general`, csrc/bq_mrsmo_nu.h): one
shared cache of kernel rows, the rows of a phase made 16 at a time, and every column's start gradient from one pass over the rows
that carry a start.  `RowOneVsOneNuSVC` solves every class pair as one row-list column; `row_nu_svc_path`, `row_nu_svr_path` and
`row_one_class_nu_path` solve every parameter as one full column.  A column's bits do not depend on the batch it runs in; they are
NOT the bits of the single fit, whose start gradient is a streamed product and whose rows are fma chains.

Shrinking is opt-in for the one dual here that runs under libsvm's plain Solver (`RowOneClassSVM(shrinking=True)`); Solver_NU's own
shrink rule is not built, so `RowNuSVC` / `RowNuSVR` and the batched paths run without.  Not here: the Laplacian kernel (a streamed
problem refuses it).
"""
import ctypes as C
import warnings

import numpy as np

from ... import _lib
from ...device import get_context
from ...opti import KernelQuadratic
from ._base import ConvergenceWarning
from .kernels import Kernel, gaussian
from ._base import ClassifierMixin
from ._batched import DecisionBatch, uses_batched_decision
from .kernels import BaseEstimator, LinearKernel
from .nu import NuSVC, NuSVR, _check_feasible, _clones
from .nu_ovo import OneVsOneNuSVC, _check_pairs_feasible
from .oneclass import OneClassSVM, _resolved
from .onevsone import ovo_pairs, pair_problem
from .smo_rows import RowSMO, RowSMOBatch

__all__ = ['RowOneClassSVM', 'RowNuSVC', 'RowNuSVR', 'RowOneVsOneNuSVC', 'row_nu_svc_path', 'row_nu_svr_path', 'row_one_class_nu_path',
           'GeneralRowSMO', 'one_class_start', 'nu_svc_start', 'nu_svr_start']


# ---- libsvm's starts ---------------------------------------------------------------------------------------------------------------------
def one_class_start(n, nu):
    a = np.zeros(n)
    m = int(nu * n)
    a[:m] = 1.0
    if m < n:
        a[m] = nu * n - m
    return a


def _fill(order, box, mass, out):
    """out[t] = min(box, remaining), remaining -= out[t] over t in `order`: libsvm's loop, without a Python loop.  The remaining mass
    before entry k is ((mass - box) - box) - ..., k sequential subtractions, which is what a cumulative sum computes; the entries
    before the first one with remaining < box hold the box, that one holds the remaining mass, the rest stay 0."""
    order = np.asarray(order)
    m = min(len(order), int(mass / box) + 2)
    if m == 0:
        return
    left = np.cumsum(np.concatenate(([mass], np.full(m - 1, -box))))
    short = np.flatnonzero(left < box)
    k = int(short[0]) if len(short) else m
    out[order[:k]] = box
    if k < len(order):
        out[order[k]] = left[k] if k < m else 0.0


def nu_svc_start(y, nu):
    n = len(y)
    a = np.zeros(n)
    _fill(np.flatnonzero(y > 0), 1.0, nu * n / 2, a)
    _fill(np.flatnonzero(y < 0), 1.0, nu * n / 2, a)
    return a


def nu_svr_start(n, C_, nu):
    half = np.zeros(n)
    _fill(np.arange(n), float(C_), C_ * nu * n / 2, half)
    return np.concatenate((half, half))


class GeneralRowSMO(RowSMO):
    """`RowSMO`'s run loop on `bq_rsmo_create_general`: the dual min 1/2 a'Qa + lin'a, 0 <= a <= boxes, Q = (s s') o K, from
    `alpha0`, under libsvm's Solver (`rule` 'plain') or Solver_NU ('nu').  After `minimize()`: `alphas`, `gradient`, `rho`, `iter`,
    `status`, `cache_stats`, `violation` (the stop measure at the last selection), and for 'nu' `r`."""

    def __init__(self, quad, X, signs, lin, boxes, alpha0, rule, tol=1e-3, max_steps=0, cache_rows=0, ctx=None, shrinking=False,
                 working_set=False):
        if rule not in ('plain', 'nu'):
            raise ValueError(f'unknown rule {rule}')
        if rule == 'nu' and shrinking:
            raise ValueError('shrinking is built for libsvm\'s Solver (rule \'plain\'), not for Solver_NU')
        if rule == 'nu' and working_set:
            raise ValueError('working sets are built for libsvm\'s Solver (rule \'plain\'), not for Solver_NU')
        if rule == 'nu' and cache_rows == 2:
            raise ValueError('a Solver_NU step holds three rows: cache_rows must be 0 or >= 3')
        N = len(signs)
        self._setup(quad, X, _lib.as_f64(signs, N, 'signs'), None, tol, False, cache_rows, ctx, shrinking, working_set)
        self.lin = _lib.as_f64(lin, N, 'lin')
        self.box = _lib.as_f64(boxes, N, 'boxes')
        self.alpha0 = _lib.as_f64(alpha0, N, 'alpha0')
        self.alphas = self.alpha0.copy()
        self.rule = rule
        self.max_steps = int(max_steps)
        self.r = 0.

    def _create(self, lib, dev, h):
        rule = _lib.RSMO_RULE_NU if self.rule == 'nu' else _lib.RSMO_RULE_PLAIN
        _lib.check(lib.bq_rsmo_create_general(dev.handle, rule, len(self.y), _lib.ptr(self.y), _lib.ptr(self.lin), _lib.ptr(self.box),
                                              _lib.ptr(self.alpha0), float(self.tol), self.max_steps, self._cache_rows(), C.byref(h)))

    def _pull(self, lib, h):
        _lib.check(lib.bq_rsmo_get(h, _lib.RSMO_ALPHAS, _lib.ptr(self.alphas)))
        self.gradient = self._gradient_now(lib, h)

    def _all_alphas(self):
        return self.alphas

    def _scalars(self, lib, h):
        if self.rule == 'nu':
            sc = np.empty(7)
            _lib.check(lib.bq_rsmo_get(h, _lib.RSMO_NU_SCALARS, _lib.ptr(sc)))
            self.rho, self.r, self.violation = sc[0], sc[1], max(sc[2], sc[3])
        else:
            sc = np.empty(6)
            _lib.check(lib.bq_rsmo_get(h, _lib.RSMO_SCALARS, _lib.ptr(sc)))
            self.rho, self.violation = sc[0], sc[1] + sc[2]
        self.b = -self.rho

    def _objective(self):
        return 0.5 * float(self.alphas @ (self.gradient + self.lin))

    def _dual(self):
        return self.y, self.lin, self.box

    def _take(self, alpha, gradient, scalars):
        """a column of a `RowSMOBatch`: the 7 NU scalars or the 6 plain ones"""
        self.alphas, self.gradient = alpha, gradient
        if self.rule == 'nu':
            self.rho, self.r, self.violation = scalars[0], scalars[1], max(scalars[2], scalars[3])
        else:
            self.rho, self.violation = scalars[0], scalars[1] + scalars[2]
        self.b = -self.rho


def _check(kernel, nu, tol, max_iter, cache_rows, C_=1.0, min_rows=2):
    if not isinstance(kernel, Kernel):
        raise TypeError(f'{kernel} is not an allowed kernel function')
    if not 0 < nu <= 1:
        raise ValueError('nu must be in (0, 1]')
    if not C_ > 0:
        raise ValueError('C must be > 0')
    if not tol > 0:
        raise ValueError('tol must be > 0')
    if max_iter is not None and not max_iter > 0:
        raise ValueError('max_iter must be None (libsvm\'s cap) or > 0')
    if not (cache_rows == 0 or cache_rows >= min_rows):   # (a Solver_NU step holds three rows, a Solver step two)
        raise ValueError(f'cache_rows must be 0 (as many as fit) or >= {min_rows}')


def _no_working_set(working_set):
    if working_set:
        raise ValueError('working sets are built for libsvm\'s Solver, not for Solver_NU: RowNuSVC / RowNuSVR run without')


class _RowFit:
    """what the three estimators share: the streamed problem, the run, the solver-independent fitted attributes"""

    def _run(self, X, signs, lin, boxes, alpha0, rule):
        if get_context().world != 1:
            raise NotImplementedError(f'{type(self).__name__} runs on a single-rank context')
        kernel = _resolved(self.kernel, X)
        quad = KernelQuadratic(X, np.zeros(X.shape[0]), 'plain', kernel, storage='stream')
        try:
            opt = GeneralRowSMO(quad, X, signs, lin, boxes, alpha0, rule, self.tol, self.max_iter or 0, self.cache_rows,
                                shrinking=getattr(self, 'shrinking', False), working_set=getattr(self, 'working_set', False)).minimize()
        finally:
            quad.release()
        return self._ran(kernel, opt)

    def _ran(self, kernel, opt):
        """the solver-independent fitted attributes from a finished `GeneralRowSMO` (its own run, or a column of a batch)"""
        self.kernel_ = kernel
        self.alphas_ = opt.alphas
        self.n_iter_ = int(opt.iter)
        self.status_ = opt.status
        self.kkt_violation_ = float(opt.violation)
        self.cache_stats_ = opt.cache_stats
        self.shrink_stats_ = opt.shrink_stats
        self.ws_stats_ = opt.ws_stats
        if self.status_ == 'stopped':
            warnings.warn('max_iter reached but the optimization has not converged yet', ConvergenceWarning)
        return opt


class RowOneClassSVM(_RowFit, OneClassSVM):
    """`OneClassSVM` without a Gram panel: libsvm's Solver on kernel rows made on demand.  `max_iter` None is libsvm's cap
    max(10^7, 100 n); `cache_rows` rows are kept in an LRU cache on the device (0: as many as fit).  Fitted attributes are
    `OneClassSVM`'s with the same meaning (`n_iter_` counts pair updates; no `train_loss_history`), plus `cache_stats_`
    ({'hits', 'misses', 'cache_rows'}).  `shrinking` (False, True = libsvm's interval of 1000 steps, or the interval) turns on
    libsvm's shrinking (`RowSMO`); `shrink_stats_` is then the solver's `shrink_stats`, else None.  `working_set` (False, True = 128,
    or an even size in 2 .. 128) switches to working-set decomposition (`RowSMO`): `n_iter_` then counts outer iterations and
    `ws_stats_` is the solver's `ws_stats`, else None.  `row_one_class_nu_path` runs the
    batched solver, which does not shrink.  A multi-rank context raises NotImplementedError."""

    def __init__(self, kernel=gaussian, nu=0.5, tol=1e-3, max_iter=None, cache_rows=0, shrinking=False, working_set=False):
        _check(kernel, nu, tol, max_iter, cache_rows)
        self.kernel = kernel
        self.nu = nu
        self.tol = tol
        self.max_iter = max_iter
        self.cache_rows = cache_rows
        self.shrinking = shrinking
        self.working_set = working_set

    def fit(self, X, y=None):
        _check(self.kernel, self.nu, self.tol, self.max_iter, self.cache_rows)   # set_params may have changed them
        X = np.ascontiguousarray(X, dtype=float)
        n = X.shape[0]
        return self._set(X, self._run(X, *self._dual(n)))

    def _dual(self, n):
        return np.ones(n), np.zeros(n), np.ones(n), one_class_start(n, self.nu), 'plain'

    def _set(self, X, opt):
        sv = self.alphas_ > 0
        self.support_ = np.flatnonzero(sv)
        self.support_vectors_ = X[sv]
        self.dual_coef_ = self.alphas_[sv]
        self.offset_ = float(opt.rho)
        self.intercept_ = -self.offset_
        return self


class RowNuSVC(_RowFit, NuSVC):
    """Binary `NuSVC` without a Gram panel: libsvm's Solver_NU on kernel rows made on demand.  Labels, the feasibility check (before
    any device work) and the fitted attributes are `NuSVC`'s (`margin_scale_` = r, `dual_coef_` = y alpha / r, `intercept_` =
    -rho / r), plus `cache_stats_`; `max_iter` and `cache_rows` (0 or >= 3) as in `RowOneClassSVM`."""

    def __init__(self, kernel=gaussian, nu=0.5, tol=1e-3, max_iter=None, cache_rows=0, working_set=False):
        _check(kernel, nu, tol, max_iter, cache_rows, min_rows=3)
        _no_working_set(working_set)
        self.working_set = working_set
        self.kernel = kernel
        self.nu = nu
        self.tol = tol
        self.max_iter = max_iter
        self.cache_rows = cache_rows

    def fit(self, X, y):
        _check(self.kernel, self.nu, self.tol, self.max_iter, self.cache_rows, min_rows=3)
        X = np.ascontiguousarray(X, dtype=float)
        y = self._labels(y)
        _check_feasible(y, self.nu)
        n = X.shape[0]
        return self._set(X, y, self._run(X, *self._dual(y)))

    def _dual(self, y):
        n = len(y)
        return y, np.zeros(n), np.ones(n), nu_svc_start(y, self.nu), 'nu'

    def _set(self, X, y, opt):
        self.margin_scale_ = float(opt.r)
        sv = self.alphas_ > 0
        self.support_ = np.flatnonzero(sv)
        self.support_vectors_ = X[sv]
        self.dual_coef_ = (y * self.alphas_)[sv] / self.margin_scale_
        self.intercept_ = -float(opt.rho) / self.margin_scale_
        return self


class RowNuSVR(_RowFit, NuSVR):
    """`NuSVR` without a Gram panel: libsvm's Solver_NU on kernel rows made on demand, the variables t and t + n sharing row t.
    Fitted attributes are `NuSVR`'s (`dual_coef_` = alpha - alpha*, `intercept_` = -rho, `epsilon_` = -r), plus `cache_stats_`;
    `max_iter` and `cache_rows` (0 or >= 3) as in `RowOneClassSVM`."""

    def __init__(self, kernel=gaussian, nu=0.5, C=1.0, tol=1e-3, max_iter=None, cache_rows=0, working_set=False):
        _check(kernel, nu, tol, max_iter, cache_rows, C, min_rows=3)
        _no_working_set(working_set)
        self.working_set = working_set
        self.kernel = kernel
        self.nu = nu
        self.C = C
        self.tol = tol
        self.max_iter = max_iter
        self.cache_rows = cache_rows

    def fit(self, X, y):
        _check(self.kernel, self.nu, self.tol, self.max_iter, self.cache_rows, self.C, min_rows=3)
        X = np.ascontiguousarray(X, dtype=float)
        y = self._targets(X, y)
        n = X.shape[0]
        return self._set(X, self._run(X, *self._dual(y)))

    def _dual(self, y):
        n = len(y)
        return (np.concatenate((np.ones(n), -np.ones(n))), np.concatenate((-y, y)), np.full(2 * n, float(self.C)),
                nu_svr_start(n, self.C, self.nu), 'nu')

    def _set(self, X, opt):
        n = X.shape[0]
        coef = self.alphas_[:n] - self.alphas_[n:]
        sv = coef != 0
        self.support_ = np.flatnonzero(sv)
        self.support_vectors_ = X[sv]
        self.dual_coef_ = coef[sv]
        self.intercept_ = -float(opt.rho)
        self.epsilon_ = -float(opt.r)
        return self


# ---- batched: every class pair, or every parameter, a column of one solve ---------------------------------------------------------------
def _solve_columns(proto, X, kernel, duals, rows=None):
    """The duals (signs, lin, boxes, alpha0, rule) — on the rows `rows[c]` of X each, or on all of X — as the columns of ONE
    `RowSMOBatch` on one streamed problem of X; the finished `GeneralRowSMO`s."""
    quad = KernelQuadratic(X, np.zeros(X.shape[0]), 'plain', kernel, storage='stream')
    try:
        cols = [GeneralRowSMO(quad, X if rows is None else X[rows[c]], *dual, proto.tol, proto.max_iter or 0)
                for c, dual in enumerate(duals)]
        held = 3 if duals[0][4] == 'nu' else 2
        if proto.cache_rows and proto.cache_rows < held * len(cols):
            raise ValueError(f'cache_rows must be 0 (as many as fit) or >= {held} per column of the batch')
        RowSMOBatch(cols, cache_rows=proto.cache_rows, rows=rows).minimize()
    finally:
        quad.release()
    return cols


class RowOneVsOneNuSVC(ClassifierMixin, BaseEstimator):
    """`OneVsOneNuSVC` without a Gram panel; constructor arguments and their checks are `RowNuSVC`'s (`cache_rows`: 0 or >= 3 per
    class pair).  Every class pair (i, j), i < j, is one Solver_NU row-list column of ONE batched solve (`bq_mrsmo_create_lists_general`)
    from libsvm's start on the pair's rows: a kernel row is made once for the k - 1 pairs of its class, and all pairs' start
    gradients come from one pass over the rows that carry a start.

    After `fit`: `classes_`, `n_classes_`, `estimators_` (one fitted `RowNuSVC` per pair in OneVsOneClassifier's order, on the rows
    of classes i and j in their original order with j as the positive class), `batched_`, `cache_stats_` (the shared cache's), and
    `decision_function` / `predict` / the fused decision batch as `OneVsOneNuSVC`.  libsvm's feasibility check runs on every pair
    before any device work (ValueError('specified nu is infeasible')).  gamma='scale' resolves on each pair's own rows and runs one
    `RowNuSVC` per pair.  A multi-rank context raises NotImplementedError."""

    def __init__(self, kernel=gaussian, nu=0.5, tol=1e-3, max_iter=None, cache_rows=0):
        _check(kernel, nu, tol, max_iter, cache_rows, min_rows=3)
        self.kernel = kernel
        self.nu = nu
        self.tol = tol
        self.max_iter = max_iter
        self.cache_rows = cache_rows

    n_classes_ = OneVsOneNuSVC.n_classes_
    decision_function = OneVsOneNuSVC.decision_function
    predict = OneVsOneNuSVC.predict

    def _binary(self):
        return RowNuSVC(kernel=self.kernel, nu=self.nu, tol=self.tol, max_iter=self.max_iter)

    def fit(self, X, y):
        _check(self.kernel, self.nu, self.tol, self.max_iter, self.cache_rows, min_rows=3)
        X = np.ascontiguousarray(X, dtype=float)
        y = np.asarray(y)
        self.classes_ = np.unique(y)
        ncls = len(self.classes_)
        if ncls == 1:
            raise ValueError('RowOneVsOneNuSVC can not be fit when only one class is present.')
        codes = np.searchsorted(self.classes_, y)
        _check_pairs_feasible(codes, ncls, [self.nu])
        if get_context().world != 1:
            raise NotImplementedError('RowOneVsOneNuSVC runs on a single-rank context')
        pairs = [pair_problem(codes, i, j) for i, j in ovo_pairs(ncls)]
        self.decision_batch_ = None
        self.batched_ = isinstance(self.kernel, LinearKernel) or getattr(self.kernel, 'gamma', None) != 'scale'
        if not self.batched_:   # gamma = 1 / (d var) of each pair's own rows: one streamed problem cannot serve every pair
            self.batched_decision_ = False
            self.estimators_ = [self._binary().fit(X[rows], (yp > 0).astype(int)) for rows, yp in pairs]
            return self
        kernel = _resolved(self.kernel, X)
        self.estimators_ = [self._binary() for _ in pairs]
        cols = _solve_columns(self, X, kernel, [est._dual(yp) for est, (_, yp) in zip(self.estimators_, pairs)],
                              rows=[rows for rows, _ in pairs])
        self.cache_stats_ = cols[0].cache_stats
        self.batched_decision_ = uses_batched_decision(self.kernel, len(pairs), get_context().world, True)
        coefs = np.zeros((len(pairs), X.shape[0])) if self.batched_decision_ else None
        for p, (est, opt, (rows, yp)) in enumerate(zip(self.estimators_, cols, pairs)):
            est.classes_ = np.array([0, 1])   # OneVsOneClassifier fits each NuSVC on 0 / 1 labels
            est._ran(kernel, opt)
            est._set(X[rows], yp, opt)
            if coefs is not None:
                coefs[p][rows[est.support_]] = est.dual_coef_
        if coefs is not None:
            self.decision_batch_ = DecisionBatch(kernel, X, coefs, [est.intercept_ for est in self.estimators_])
        return self


def _path(estimator, X, params, dual_of, set_of):
    """fitted clones of `estimator`, one per dict of `params`, each a full column of one batched solve on one streamed problem"""
    ests = _clones(estimator, params)
    if not ests:
        return ests
    if get_context().world != 1:
        raise NotImplementedError(f'{type(estimator).__name__} runs on a single-rank context')
    kernel = _resolved(estimator.kernel, X)
    for est, opt in zip(ests, _solve_columns(estimator, X, kernel, [dual_of(est) for est in ests])):
        est._ran(kernel, opt)
        set_of(est, opt)
    return ests


def row_nu_svc_path(estimator, X, y, nus):
    """A list of fitted clones of the `RowNuSVC` `estimator`, one per nu of `nus`, every nu a full column of ONE batched Solver_NU
    solve (`bq_mrsmo_create_general`).  Each clone's `alphas_` and `n_iter_` are those of its column run alone in a batch of one."""
    X = np.ascontiguousarray(X, dtype=float)
    ests = _clones(estimator, [dict(nu=float(nu)) for nu in nus])
    ys = [est._labels(y) for est in ests]
    for est, yy in zip(ests, ys):
        _check(est.kernel, est.nu, est.tol, est.max_iter, est.cache_rows, min_rows=3)
        _check_feasible(yy, est.nu)
    fitted = _path(estimator, X, [dict(nu=est.nu) for est in ests], lambda est: est._dual(ys[0]), lambda est, opt: est._set(X, ys[0], opt))
    for est in fitted:
        est.classes_ = ests[0].classes_.copy()
    return fitted


def row_nu_svr_path(estimator, X, y, params):
    """The same for `RowNuSVR`: `params` is a list of dicts with 'nu' and / or 'C'."""
    X = np.ascontiguousarray(X, dtype=float)
    yy = estimator._targets(X, y)
    ests = _clones(estimator, params)
    for est in ests:
        _check(est.kernel, est.nu, est.tol, est.max_iter, est.cache_rows, est.C, min_rows=3)
    return _path(estimator, X, params, lambda est: est._dual(yy), lambda est, opt: est._set(X, opt))


def row_one_class_nu_path(estimator, X, nus):
    """The same for `RowOneClassSVM` (libsvm's Solver from the one-class start), one column per nu."""
    X = np.ascontiguousarray(X, dtype=float)
    params = [dict(nu=float(nu)) for nu in nus]
    for est in _clones(estimator, params):
        _check(est.kernel, est.nu, est.tol, est.max_iter, est.cache_rows)
    return _path(estimator, X, params, lambda est: est._dual(X.shape[0]), lambda est, opt: est._set(X, opt))
