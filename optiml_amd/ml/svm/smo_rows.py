"""Panel-free SMO: libsvm's WSS2 decomposition on kernel rows made on demand (`bq_rsmo_*`, csrc/bq_rsmo.hip).

`RowSMOClassifier` / `RowSMORegression` take the constructor arguments of `SMOClassifier` / `SMORegression` plus `cache_rows`, and
`quad` is a `KernelQuadratic(storage='stream')`: no Gram panel exists, each step computes (or finds in an LRU cache of `cache_rows`
rows in HBM, 0 = as many as fit) the two kernel rows it touches from the k-major image of X.  This is what
`SVC` / `SVR(optimizer='smo', storage='stream').fit` run.

The algorithm is libsvm's `Solver::Solve` without shrinking, NOT the Keerthi / Shevade walker of `smo.py`, and `tol` is libsvm's
(sklearn's): the run ends when Gmax + Gmax2 < tol, the largest violation of the KKT conditions over the pair sets, where the
resident walker compares every example with its two thresholds b_up / b_low under 2 tol.  Same dual, same optimum, different
trajectories and different distances from it at equal `tol`.  `b` = -rho with libsvm's rho (`calculate_rho`).
"""
import ctypes as C
from abc import ABC

import numpy as np

from ... import _lib
from ...device import get_context
from ...opti import KernelQuadratic
from .kernels import LinearKernel

__all__ = ['RowSMO', 'RowSMOClassifier', 'RowSMORegression']


class RowSMO(ABC):
    _task = None
    run_steps = 512   # steps enqueued between two looks at the device's `finished` word

    def __init__(self, quad, X, y, K, kernel, C, tol=1e-3, verbose=False, box=None, cache_rows=0, ctx=None):
        self._setup(quad, X, y, kernel, tol, verbose, cache_rows, ctx)
        self.K = K
        self.C = C
        n = len(self.X)
        self.box = np.full(n, float(C)) if box is None else _lib.as_f64(box, n, 'box')

    def _setup(self, quad, X, y, kernel, tol, verbose, cache_rows, ctx):
        """what every dual on rows needs: the streamed problem, the data, the run's parameters and its (empty) results"""
        if not isinstance(quad, KernelQuadratic) or quad.storage != 'stream':
            raise TypeError("the row-based SMO needs a KernelQuadratic(storage='stream') as quad")
        if not (cache_rows == 0 or cache_rows >= 2):
            raise ValueError('cache_rows must be 0 (as many as fit) or >= 2')
        self.quad = quad
        self.X = np.ascontiguousarray(X, dtype=float)
        self.y = np.ascontiguousarray(y, dtype=float)
        self.kernel = kernel
        if isinstance(kernel, LinearKernel):
            self.w = 0.
        self.b = 0.
        self.rho = 0.
        self.tol = tol
        self.cache_rows = int(cache_rows)
        self.ctx = ctx   # None: the default context
        self.iter = 0
        self.status = 'unknown'
        self.cache_stats = {'hits': 0, 'misses': 0, 'cache_rows': 0}
        self.verbose = verbose

    def _epsilon(self):
        return 0.0

    def _coefficients(self):
        """the vector c with decision(x) = sum_j c_j k(x_j, x) + b"""
        raise NotImplementedError

    def _all_alphas(self):
        raise NotImplementedError

    def _pull(self, lib, h):
        raise NotImplementedError

    def _create(self, lib, dev, h):
        """the device solver of this dual on the problem `dev`, into the handle `h`"""
        _lib.check(lib.bq_rsmo_create(dev.handle, self._task, _lib.ptr(self.y), _lib.ptr(self.box), float(self._epsilon()),
                                      float(self.tol), self.cache_rows, C.byref(h)))

    def _scalars(self, lib, h):
        """the offsets and the stop measure of the finished run"""
        sc = np.empty(6)
        _lib.check(lib.bq_rsmo_get(h, _lib.RSMO_SCALARS, _lib.ptr(sc)))
        self.rho, self.gmax, self.gmax2 = sc[0], sc[1], sc[2]
        self.b = -self.rho

    def minimize(self):
        lib = _lib.load()
        ctx = self.ctx or get_context()
        if ctx.world != 1:   # before anything is built: a multi-rank problem is a collective
            raise NotImplementedError('the row-based SMO runs on a single-rank context')
        dev = self.quad.device_problem(ctx)
        h = C.c_void_p()
        self._create(lib, dev, h)
        try:
            if self.verbose:
                print('iter\t cost')
            steps, fin = C.c_int64(0), C.c_int(0)
            shown = -1
            while not fin.value:
                # one step per call only when the cost line has to be printed in between
                _lib.check(lib.bq_rsmo_run(h, 1 if self.verbose else self.run_steps, C.byref(steps), C.byref(fin)))
                if self.verbose and steps.value != shown:
                    shown = self.iter = steps.value
                    if not (self.iter - 1) % self.verbose:
                        self._pull(lib, h)
                        print('{:4d}\t{: 1.4e}'.format(self.iter - 1, self._objective()))
            self.iter = steps.value
            self.status = _lib.RSMO_STATUS[fin.value]
            self._pull(lib, h)
            self._scalars(lib, h)
            st = np.empty(3)
            _lib.check(lib.bq_rsmo_get(h, _lib.RSMO_STATS, _lib.ptr(st)))
            self.cache_stats = {'hits': int(st[0]), 'misses': int(st[1]), 'cache_rows': int(st[2])}
            if isinstance(self.kernel, LinearKernel):
                self.w = self._coefficients() @ self.X
            if self.verbose:
                print()
        finally:
            lib.bq_rsmo_destroy(h)
        return self

    def _objective(self):
        """1/2 a'Qa + p'a from the solver's own gradient: 1/2 a'(G + p), as libsvm reports it (no product with K)"""
        raise NotImplementedError

    def objective(self):
        """the dual objective at the solution"""
        return self._objective()

    def _gradient_now(self, lib, h):
        g = np.empty(len(self._all_alphas()))
        _lib.check(lib.bq_rsmo_get(h, _lib.RSMO_GRADIENT, _lib.ptr(g)))
        return g


class RowSMOClassifier(RowSMO):
    _task = _lib.SVC

    def __init__(self, quad, X, y, K, kernel, C, tol=1e-3, verbose=False, box=None, cache_rows=0, ctx=None):
        self.alphas = np.zeros(len(X))
        super(RowSMOClassifier, self).__init__(quad, X, y, K, kernel, C, tol, verbose, box, cache_rows, ctx)

    def _pull(self, lib, h):
        _lib.check(lib.bq_rsmo_get(h, _lib.RSMO_ALPHAS, _lib.ptr(self.alphas)))
        self.gradient = self._gradient_now(lib, h)

    def _all_alphas(self):
        return self.alphas

    def _coefficients(self):
        return self.alphas * self.y

    def _objective(self):
        return 0.5 * float(self.alphas @ (self.gradient - 1.0))


class RowSMORegression(RowSMO):
    _task = _lib.SVR

    def __init__(self, quad, X, y, K, kernel, C, epsilon, tol=1e-3, verbose=False, box=None, cache_rows=0, ctx=None):
        self.alphas_p = np.zeros(len(X))
        self.alphas_n = np.zeros(len(X))
        super(RowSMORegression, self).__init__(quad, X, y, K, kernel, C, tol, verbose, box, cache_rows, ctx)
        self.epsilon = epsilon

    def _epsilon(self):
        return self.epsilon

    def _pull(self, lib, h):
        both = np.empty(2 * len(self.alphas_p))
        _lib.check(lib.bq_rsmo_get(h, _lib.RSMO_ALPHAS, _lib.ptr(both)))
        self.alphas_p, self.alphas_n = both[:len(both) // 2].copy(), both[len(both) // 2:].copy()
        self.gradient = self._gradient_now(lib, h)

    def _all_alphas(self):
        return np.concatenate((self.alphas_p, self.alphas_n))

    def _coefficients(self):
        return self.alphas_p - self.alphas_n

    def _objective(self):
        p = np.concatenate((self.epsilon - self.y, self.epsilon + self.y))
        return 0.5 * float(self._all_alphas() @ (self.gradient + p))
