"""Panel-free SMO: libsvm's WSS2 decomposition on kernel rows made on demand (`bq_rsmo_*`, csrc/bq_rsmo.hip).

`RowSMOClassifier` / `RowSMORegression` take the constructor arguments of `SMOClassifier` / `SMORegression` plus `cache_rows`, and
`quad` is a `KernelQuadratic(storage='stream')`: no Gram panel exists, each step computes (or finds in an LRU cache of `cache_rows`
rows in HBM, 0 = as many as fit) the two kernel rows it touches from the k-major image of X.  This is what
`SVC` / `SVR(optimizer='smo', storage='stream').fit` run.

The algorithm is libsvm's `Solver::Solve`, shrinking opt-in (`shrinking=True`: libsvm's interval of 1000 steps; an int: the
interval; `bq_rsmo_set_shrinking`, csrc/bq_rsmo_shrink.h — variables at a bound that cannot become violators leave a device-side
active list, rows, selection and update run on the list, and the full gradient is rebuilt by one streamed product when libsvm
reconstructs it; `shrink_stats` reports the list's length, its smallest length, the shrink passes and the reconstructions), NOT the Keerthi / Shevade walker of `smo.py`, and `tol` is libsvm's
(sklearn's): the run ends when Gmax + Gmax2 < tol, the largest violation of the KKT conditions over the pair sets, where the
resident walker compares every example with its two thresholds b_up / b_low under 2 tol.  Same dual, same optimum, different
trajectories and different distances from it at equal `tol`.  `b` = -rho with libsvm's rho (`calculate_rho`).

`working_set` (False; True = 128; or an even size in 2 .. 128; `bq_rsmo_set_working_set`, csrc/bq_rsmo_ws.h) switches to working-set
decomposition: an outer iteration takes that many violators, solves the dual restricted to them in the LDS of one compute unit
and applies the whole change to the gradient in one matrix-core pass over the image.  `iter` then counts outer iterations,
`ws_stats` is {'working_set', 'outer', 'inner'} (inner: pair updates inside working sets), no kernel row is made or cached
(`cache_rows` 0 asks for the smallest cache), and the stop test is unchanged: the same optimum within `tol`, on another trajectory,
with the same bits on every run.  It excludes `shrinking` and is not built for Solver_NU.
"""
import ctypes as C
from abc import ABC

import numpy as np

from ... import _lib
from ...device import get_context
from ...opti import KernelQuadratic
from .kernels import LinearKernel

__all__ = ['RowSMO', 'RowSMOClassifier', 'RowSMORegression', 'RowSMOBatch']


class RowSMO(ABC):
    _task = None
    run_steps = 512   # steps enqueued between two looks at the device's `finished` word

    def __init__(self, quad, X, y, K, kernel, C, tol=1e-3, verbose=False, box=None, cache_rows=0, ctx=None, shrinking=False, working_set=False):
        self._setup(quad, X, y, kernel, tol, verbose, cache_rows, ctx, shrinking, working_set)
        self.K = K
        self.C = C
        n = len(self.X)
        self.box = np.full(n, float(C)) if box is None else _lib.as_f64(box, n, 'box')

    def _setup(self, quad, X, y, kernel, tol, verbose, cache_rows, ctx, shrinking=False, working_set=False):
        """what every dual on rows needs: the streamed problem, the data, the run's parameters and its (empty) results"""
        if working_set is not True and working_set is not False and not (
                isinstance(working_set, (int, np.integer)) and 2 <= working_set <= 128 and working_set % 2 == 0):
            raise ValueError('working_set must be False, True (128 variables) or an even size in 2 .. 128')
        if working_set and shrinking:
            raise ValueError('working_set and shrinking exclude each other')
        self.working_set = working_set
        if shrinking is not True and shrinking is not False and not (isinstance(shrinking, (int, np.integer)) and shrinking > 0):
            raise ValueError('shrinking must be False, True (libsvm\'s 1000 steps) or a positive interval')
        self.shrinking = shrinking
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
        self.shrink_stats = None   # with shrinking: {'active', 'min_active', 'shrinks', 'reconstructions'}
        self.ws_stats = None       # with a working set: {'working_set', 'outer', 'inner'}
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
                                      float(self.tol), self._cache_rows(), C.byref(h)))

    def _cache_rows(self):
        """a working-set run makes no kernel row: the smallest cache in place of the automatic one (half of the free memory)"""
        return 2 if self.working_set and self.cache_rows == 0 else self.cache_rows

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
            if self.shrinking:
                _lib.check(lib.bq_rsmo_set_shrinking(h, 0 if self.shrinking is True else int(self.shrinking)))
            if self.working_set:
                _lib.check(lib.bq_rsmo_set_working_set(h, 128 if self.working_set is True else int(self.working_set)))
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
            self._finished(st)
            if self.shrinking:
                sh = np.empty(4)
                _lib.check(lib.bq_rsmo_get(h, _lib.RSMO_SHRINK_STATS, _lib.ptr(sh)))
                self.shrink_stats = dict(zip(('active', 'min_active', 'shrinks', 'reconstructions'), (int(v) for v in sh)))
            if self.working_set:
                ws = np.empty(3)
                _lib.check(lib.bq_rsmo_get(h, _lib.RSMO_WS_STATS, _lib.ptr(ws)))
                self.ws_stats = dict(zip(('working_set', 'outer', 'inner'), (int(v) for v in ws)))
            if self.verbose:
                print()
        finally:
            lib.bq_rsmo_destroy(h)
        return self

    def _finished(self, st):
        """the read-back every run ends with: the cache's counts (hits, misses, rows) and the linear kernel's w"""
        self.cache_stats = {'hits': int(st[0]), 'misses': int(st[1]), 'cache_rows': int(st[2])}
        if isinstance(self.kernel, LinearKernel):
            self.w = self._coefficients() @ self.X

    def _dual(self):
        """(signs, linear term, boxes) of this dual on its N variables, as `bq_rsmo_create` builds them"""
        raise NotImplementedError

    def _take(self, alpha, gradient, scalars):
        """the solver's vectors and (rho, Gmax, Gmax2, ...) of this dual, from a solver that ran it as one of its columns"""
        raise NotImplementedError

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

    def __init__(self, quad, X, y, K, kernel, C, tol=1e-3, verbose=False, box=None, cache_rows=0, ctx=None, shrinking=False, working_set=False):
        self.alphas = np.zeros(len(X))
        super(RowSMOClassifier, self).__init__(quad, X, y, K, kernel, C, tol, verbose, box, cache_rows, ctx, shrinking, working_set)

    def _pull(self, lib, h):
        _lib.check(lib.bq_rsmo_get(h, _lib.RSMO_ALPHAS, _lib.ptr(self.alphas)))
        self.gradient = self._gradient_now(lib, h)

    def _all_alphas(self):
        return self.alphas

    def _dual(self):
        return self.y, -np.ones(len(self.y)), self.box

    def _take(self, alpha, gradient, scalars):
        self.alphas, self.gradient = alpha, gradient
        self.rho, self.gmax, self.gmax2 = scalars[:3]
        self.b = -self.rho

    def _coefficients(self):
        return self.alphas * self.y

    def _objective(self):
        return 0.5 * float(self.alphas @ (self.gradient - 1.0))


class RowSMORegression(RowSMO):
    _task = _lib.SVR

    def __init__(self, quad, X, y, K, kernel, C, epsilon, tol=1e-3, verbose=False, box=None, cache_rows=0, ctx=None, shrinking=False, working_set=False):
        self.alphas_p = np.zeros(len(X))
        self.alphas_n = np.zeros(len(X))
        super(RowSMORegression, self).__init__(quad, X, y, K, kernel, C, tol, verbose, box, cache_rows, ctx, shrinking, working_set)
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

    def _dual(self):
        n = len(self.y)
        return (np.concatenate((np.ones(n), -np.ones(n))), np.concatenate((self.epsilon - self.y, self.epsilon + self.y)),
                np.concatenate((self.box, self.box)))

    def _take(self, alpha, gradient, scalars):
        self.alphas_p, self.alphas_n = alpha[:len(alpha) // 2].copy(), alpha[len(alpha) // 2:].copy()
        self.gradient = gradient
        self.rho, self.gmax, self.gmax2 = scalars[:3]
        self.b = -self.rho

    def _coefficients(self):
        return self.alphas_p - self.alphas_n

    def _objective(self):
        p = np.concatenate((self.epsilon - self.y, self.epsilon + self.y))
        return 0.5 * float(self._all_alphas() @ (self.gradient + p))


class RowSMOBatch:
    """k `RowSMOClassifier` / `RowSMORegression` duals on ONE streamed problem, solved together (`bq_mrsmo_*`, csrc/bq_mrsmo.hip):
    one cache of kernel rows for all columns, the rows a step misses made 16 at a time by the fp64-MFMA row-block kernel.  `columns`
    are unrun solvers of one type on the same `quad`, X, kernel and tol; after `minimize()` each holds what its own `minimize()`
    would have set (alphas, gradient, rho / b, iter, status, w), from rows with the row-block kernel's bits, and `cache_stats` of
    the shared cache.  A column's trajectory does not depend on the other columns or on the cache.  The batched solver does not
    shrink: a column's `shrinking` is ignored here.

    `rows` (one strictly ascending list of rows of the quad per column) makes every column a row-list column
    (`bq_mrsmo_create_lists`): column c is a `RowSMOClassifier` built on `X[rows[c]], y[rows[c]]` — a class pair of one-vs-one — and
    is solved on the kernel values `K[rows[c]][:, rows[c]]` of the shared quad, its variables the positions of its list: the fit of
    those rows in their order.  Kernel rows are made and cached whole, so a row serves every column that lists it; the select and
    update kernels run over the lists only.  Each column holds m_c-long alphas and gradient afterwards.

    `alpha0` (one start per column, inside its boxes) and `rule` ('plain': libsvm's Solver; 'nu': Solver_NU, which keeps the mass of
    each sign) reach the general entries (`bq_mrsmo_create_general` / `_create_lists_general`), in both forms; `GeneralRowSMO`
    columns (nu_rows.py) bring their own start and rule.  The start gradient of every column is made from ONE pass over the rows
    that carry a nonzero start in any column.  After `minimize()` every column has `alphas`, `gradient`, `rho`, `iter`, `status`,
    `violation` (the stop measure at the last selection) and, for 'nu', `r`."""
    run_steps = RowSMO.run_steps

    def __init__(self, columns, cache_rows=0, ctx=None, rows=None, alpha0=None, rule='plain'):
        first = columns[0]
        if any(type(c) is not type(first) or c.quad is not first.quad for c in columns):
            raise TypeError('the columns of a batch are solvers of one type on one quad')
        if rule not in ('plain', 'nu'):
            raise ValueError(f'unknown rule {rule}')
        general = hasattr(first, 'alpha0')   # GeneralRowSMO columns: the dual as data, with its own start and rule
        if general:
            rule = first.rule if rule == 'plain' else rule
            if any(c.rule != rule for c in columns):
                raise ValueError('the columns of a batch run under one rule')
            alpha0 = [c.alpha0 for c in columns] if alpha0 is None else alpha0
        held = 3 if rule == 'nu' else 2   # rows a step holds per column
        if not (cache_rows == 0 or cache_rows >= held * len(columns)):
            raise ValueError(f'cache_rows must be 0 (as many as fit) or >= {held} per column')
        if rule == 'nu' and len(columns) > 512:
            raise ValueError('a Solver_NU batch holds at most 512 columns')
        if alpha0 is not None and len(alpha0) != len(columns):
            raise ValueError('alpha0 must hold one start per column')
        if rows is not None:
            if not (isinstance(first, RowSMOClassifier) or general):
                raise TypeError('row-list columns are RowSMOClassifier or GeneralRowSMO duals (N = m); the 2n form covers all rows')
            if len(rows) != len(columns) or any(len(r) != len(c.y) for r, c in zip(rows, columns)):
                raise ValueError('rows must hold one list per column, as long as the column')
            rows = [np.ascontiguousarray(r, dtype=np.int32) for r in rows]
        self.columns = list(columns)
        self.rows = rows
        self.cache_rows = int(cache_rows)
        self.ctx = ctx
        self.rule = rule
        self.alpha0 = None if alpha0 is None else [np.ascontiguousarray(a, dtype=float) for a in alpha0]
        self.max_steps = int(getattr(first, 'max_steps', 0))

    def _create(self, lib, dev, h):
        """create the device solver of the columns into `h`; returns every column's number of variables"""
        cols, k = self.columns, len(self.columns)
        duals = [c._dual() for c in cols]
        general = self.alpha0 is not None or self.rule == 'nu'   # anything else keeps the entries (and launches) it always had
        rule = _lib.RSMO_RULE_NU if self.rule == 'nu' else _lib.RSMO_RULE_PLAIN
        if general:
            duals = [d + (np.zeros(len(d[0])) if self.alpha0 is None else self.alpha0[c],) for c, d in enumerate(duals)]
            if any(len(d[3]) != len(d[0]) for d in duals):
                raise ValueError('a start is as long as its column')
        if self.rows is None:
            signs, lin, boxes, *start = (np.ascontiguousarray(np.stack(part), dtype=float) for part in zip(*duals))
            if general:
                _lib.check(lib.bq_mrsmo_create_general(dev.handle, rule, k, signs.shape[1], _lib.ptr(signs), _lib.ptr(lin),
                                                       _lib.ptr(boxes), _lib.ptr(start[0]), float(cols[0].tol), self.max_steps,
                                                       self.cache_rows, C.byref(h)))
            else:
                _lib.check(lib.bq_mrsmo_create(dev.handle, k, signs.shape[1], _lib.ptr(signs), _lib.ptr(lin), _lib.ptr(boxes),
                                               float(cols[0].tol), 0, self.cache_rows, C.byref(h)))
            return [signs.shape[1]] * k
        signs, lin, boxes, *start = (np.ascontiguousarray(np.concatenate(part), dtype=float) for part in zip(*duals))
        offsets = np.concatenate(([0], np.cumsum([len(r) for r in self.rows]))).astype(np.int64)
        rows = np.ascontiguousarray(np.concatenate(self.rows), dtype=np.int32)
        optr = offsets.ctypes.data_as(C.POINTER(C.c_int64))
        if general:
            _lib.check(lib.bq_mrsmo_create_lists_general(dev.handle, rule, k, optr, _lib.iptr(rows), _lib.ptr(signs), _lib.ptr(lin),
                                                         _lib.ptr(boxes), _lib.ptr(start[0]), float(cols[0].tol), self.max_steps,
                                                         self.cache_rows, C.byref(h)))
        else:
            _lib.check(lib.bq_mrsmo_create_lists(dev.handle, k, optr, _lib.iptr(rows), _lib.ptr(signs), _lib.ptr(lin), _lib.ptr(boxes),
                                                 float(cols[0].tol), 0, self.cache_rows, C.byref(h)))
        return [len(r) for r in self.rows]

    def minimize(self):
        lib = _lib.load()
        ctx = self.ctx or get_context()
        if ctx.world != 1:
            raise NotImplementedError('the row-based SMO runs on a single-rank context')
        cols, k = self.columns, len(self.columns)
        dev = cols[0].quad.device_problem(ctx)
        h = C.c_void_p()
        sizes = self._create(lib, dev, h)
        try:
            steps, fin = (C.c_int64 * k)(), (C.c_int * k)()
            while not all(fin):
                _lib.check(lib.bq_mrsmo_run(h, self.run_steps, steps, fin))
            st = np.empty(3)
            _lib.check(lib.bq_mrsmo_get(h, _lib.RSMO_STATS, 0, _lib.ptr(st)))
            for c, col in enumerate(cols):
                nu = self.rule == 'nu'
                alpha, grad, sc = np.empty(sizes[c]), np.empty(sizes[c]), np.empty(7 if nu else 6)
                for what, out in ((_lib.RSMO_ALPHAS, alpha), (_lib.RSMO_GRADIENT, grad),
                                  (_lib.RSMO_NU_SCALARS if nu else _lib.RSMO_SCALARS, sc)):
                    _lib.check(lib.bq_mrsmo_get(h, what, c, _lib.ptr(out)))
                col._take(alpha, grad, sc)
                col.violation = max(sc[2], sc[3]) if nu else sc[1] + sc[2]
                if nu:
                    col.r = sc[1]
                col.iter = int(steps[c])
                col.status = _lib.RSMO_STATUS[int(fin[c])]
                col._finished(st)
        finally:
            lib.bq_mrsmo_destroy(h)
        return self
