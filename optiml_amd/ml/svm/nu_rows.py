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

Not here: shrinking, a nu-path over the row solver, one-vs-one nu on rows, the Laplacian kernel (a streamed problem refuses it).
"""
import ctypes as C
import warnings

import numpy as np

from ... import _lib
from ...device import get_context
from ...opti import KernelQuadratic
from ._base import ConvergenceWarning
from .kernels import Kernel, gaussian
from .nu import NuSVC, NuSVR, _check_feasible
from .oneclass import OneClassSVM, _resolved
from .smo_rows import RowSMO

__all__ = ['RowOneClassSVM', 'RowNuSVC', 'RowNuSVR', 'GeneralRowSMO', 'one_class_start', 'nu_svc_start', 'nu_svr_start']


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

    def __init__(self, quad, X, signs, lin, boxes, alpha0, rule, tol=1e-3, max_steps=0, cache_rows=0, ctx=None):
        if rule not in ('plain', 'nu'):
            raise ValueError(f'unknown rule {rule}')
        if rule == 'nu' and cache_rows == 2:
            raise ValueError('a Solver_NU step holds three rows: cache_rows must be 0 or >= 3')
        N = len(signs)
        self._setup(quad, X, _lib.as_f64(signs, N, 'signs'), None, tol, False, cache_rows, ctx)
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
                                              _lib.ptr(self.alpha0), float(self.tol), self.max_steps, self.cache_rows, C.byref(h)))

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


class _RowFit:
    """what the three estimators share: the streamed problem, the run, the solver-independent fitted attributes"""

    def _run(self, X, signs, lin, boxes, alpha0, rule):
        if get_context().world != 1:
            raise NotImplementedError(f'{type(self).__name__} runs on a single-rank context')
        kernel = _resolved(self.kernel, X)
        quad = KernelQuadratic(X, np.zeros(X.shape[0]), 'plain', kernel, storage='stream')
        try:
            opt = GeneralRowSMO(quad, X, signs, lin, boxes, alpha0, rule, self.tol, self.max_iter or 0, self.cache_rows).minimize()
        finally:
            quad.release()
        self.kernel_ = kernel
        self.alphas_ = opt.alphas
        self.n_iter_ = int(opt.iter)
        self.status_ = opt.status
        self.kkt_violation_ = float(opt.violation)
        self.cache_stats_ = opt.cache_stats
        if self.status_ == 'stopped':
            warnings.warn('max_iter reached but the optimization has not converged yet', ConvergenceWarning)
        return opt


class RowOneClassSVM(_RowFit, OneClassSVM):
    """`OneClassSVM` without a Gram panel: libsvm's Solver on kernel rows made on demand.  `max_iter` None is libsvm's cap
    max(10^7, 100 n); `cache_rows` rows are kept in an LRU cache on the device (0: as many as fit).  Fitted attributes are
    `OneClassSVM`'s with the same meaning (`n_iter_` counts pair updates; no `train_loss_history`), plus `cache_stats_`
    ({'hits', 'misses', 'cache_rows'}).  A multi-rank context raises NotImplementedError."""

    def __init__(self, kernel=gaussian, nu=0.5, tol=1e-3, max_iter=None, cache_rows=0):
        _check(kernel, nu, tol, max_iter, cache_rows)
        self.kernel = kernel
        self.nu = nu
        self.tol = tol
        self.max_iter = max_iter
        self.cache_rows = cache_rows

    def fit(self, X, y=None):
        _check(self.kernel, self.nu, self.tol, self.max_iter, self.cache_rows)   # set_params may have changed them
        X = np.ascontiguousarray(X, dtype=float)
        n = X.shape[0]
        opt = self._run(X, np.ones(n), np.zeros(n), np.ones(n), one_class_start(n, self.nu), 'plain')
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

    def __init__(self, kernel=gaussian, nu=0.5, tol=1e-3, max_iter=None, cache_rows=0):
        _check(kernel, nu, tol, max_iter, cache_rows, min_rows=3)
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
        opt = self._run(X, y, np.zeros(n), np.ones(n), nu_svc_start(y, self.nu), 'nu')
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

    def __init__(self, kernel=gaussian, nu=0.5, C=1.0, tol=1e-3, max_iter=None, cache_rows=0):
        _check(kernel, nu, tol, max_iter, cache_rows, C, min_rows=3)
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
        opt = self._run(X, np.concatenate((np.ones(n), -np.ones(n))), np.concatenate((-y, y)), np.full(2 * n, float(self.C)),
                        nu_svr_start(n, self.C, self.nu), 'nu')
        coef = self.alphas_[:n] - self.alphas_[n:]
        sv = coef != 0
        self.support_ = np.flatnonzero(sv)
        self.support_vectors_ = X[sv]
        self.dual_coef_ = coef[sv]
        self.intercept_ = -float(opt.rho)
        self.epsilon_ = -float(opt.r)
        return self
