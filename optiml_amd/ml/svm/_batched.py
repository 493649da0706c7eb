"""What the batched SVM fits share (`OneVsRestSVC`, `OneVsOneSVC`, `SVCGridSearchCV`, `MultiOutputSVR`, `SVRGridSearchCV`,
`OneClassSVM`): the device solver of many columns on one Gram panel (`_DeviceMultiSolver`: ProjectedGradient / FrankWolfe;
`_DeviceALSolver`: the augmented-Lagrangian dual with the first-order rules; `_DeviceSimplexSolver`: the nu-one-class dual on its
capped simplex; `_DeviceSimplex2Solver`: the nu-SVC / nu-SVR duals on two of them; `_DeviceSimplexPairSolver`: the nu-SVC duals of class pairs on a
class-sorted panel), the one-off multi-column products, the device memory budget of a solve, and
the way a column's result becomes the `SVC` that `SVC.fit` (the `SVR` that `SVR.fit`) leaves.
"""
import ctypes as C
import warnings
from collections.abc import Iterable
from contextlib import contextmanager

import numpy as np

from ... import _lib
from ...device import get_context
from ...opti import KernelQuadratic
from ...opti.constrained import ProjectedGradient
from ...opti.unconstrained.stochastic import StochasticOptimizer, StochasticMomentumOptimizer
from ._base import SVC, SVR, ClassifierMixin, RegressorMixin, BaseEstimator, ConvergenceWarning, has_class_weight
from .kernels import GaussianKernel, LinearKernel, PolyKernel, SigmoidKernel, gaussian
from .losses import squared_hinge, squared_epsilon_insensitive
from .smo import SMOClassifier, SMORegression

MEMORY_SHARE = 0.5   # share of the device memory free after the panel that one solve's columns and slab may take
MAX_COLUMNS = 4096   # columns per batched solve at most (see column_cap)


def column_bytes(n):
    """Device state of one column on n rows: about 16 n-vectors (the solver's x, g, d, Qd, bounds, labels, product input and
    output), each padded by a tile."""
    return 16 * 8 * (n + 256)


def column_cap(length, free_bytes, slab_bytes):
    """Columns one batched solve may take with `free_bytes` of device memory free after the panel: MEMORY_SHARE of it, less the
    solver's 16-column slab (`slab_bytes`), over the device state of a column of `length` variables (`column_bytes`); at most
    MAX_COLUMNS, at least 16.  Larger grids run in several solves; the split does not change any column's bits (the product is
    batch-invariant)."""
    budget = int(free_bytes * MEMORY_SHARE) - int(slab_bytes)
    return int(max(16, min(MAX_COLUMNS, budget // column_bytes(length))))


def device_free_bytes():
    free, total = C.c_int64(0), C.c_int64(0)
    _lib.check(_lib.load().bq_ctx_mem_info(get_context().handle, C.byref(free), C.byref(total)))
    return free.value


@contextmanager
def device_panel(*args, **kwargs):
    """The Gram panel of `KernelQuadratic(*args, **kwargs)` on the device for the length of a `with` block: yields (obj, dev,
    free_bytes, wide_slab_bytes) — the quadratic, its device problem, the device memory free after the panel and the 16-column
    product's slab on it — and releases the panel on exit, also when the body raises."""
    obj = KernelQuadratic(*args, **kwargs)
    try:
        dev = obj.device_problem()
        yield obj, dev, device_free_bytes(), _lib.load().bq_problem_wide_slab_bytes(dev.handle)
    finally:
        obj.release()


def smo_column_bytes(n, task, weighted=False):
    """Device state of one batched-SMO column on n rows (`bq_msmo_create`): labels or targets, multipliers (two vectors for
    regression), error cache, the support list's coefficients (8 n each) and its indices (4 n); `weighted`
    (`bq_msmo_create_weighted`): its boxes too (8 n)."""
    return ((36 if task == _lib.SVC else 44) + (8 if weighted else 0)) * int(n)


def smo_column_cap(n, task, free_bytes, weighted=False):
    """Columns one batched SMO solve may take with `free_bytes` of device memory free after the panel: MEMORY_SHARE of it over
    `smo_column_bytes`; at most MAX_COLUMNS, at least 1.  Larger sets run in several solves; columns are independent, so the
    split changes no bits."""
    return int(max(1, min(MAX_COLUMNS, int(free_bytes * MEMORY_SHARE) // smo_column_bytes(n, task, weighted))))


def smo_heldout_column_cap(n, task, free_bytes, wide_slab_bytes, calibrators=False):
    """`smo_column_cap` for columns that are scored where they stand (`bq_msmo_svr_heldout` / `bq_msmo_svc_heldout`).  The budget —
    MEMORY_SHARE of `free_bytes` — holds per column the walker's state (`smo_column_bytes`) and the scoring's scratch, the product's
    input and output: two n-vectors, each padded by a tile; with `calibrators` (a calibrator per column) also the two n-vectors of
    its sample; and once the 16-column product's slab (`wide_slab_bytes`) and the two vectors of the last chunk's 15 padding
    columns.  At most MAX_COLUMNS, at least 1.  The split changes no column's bits."""
    vec = 8 * (int(n) + 256)
    per_column = smo_column_bytes(n, task) + (4 if calibrators else 2) * vec
    budget = int(free_bytes * MEMORY_SHARE) - int(wide_slab_bytes) - 2 * 15 * vec
    return int(max(1, min(MAX_COLUMNS, budget // per_column)))


def smo_failed_error():
    """what the single fit raises for a walker that met the reference's 'unexpected status': bq_smo_run's error"""
    return _lib.BcqpError(_lib.ERR_NONFINITE, 'SMO reached an unexpected status (no threshold index)')


# The smallest number of columns that takes the batched SMO path when nothing forces either one (`batch_smo` of the estimators and
# of the search).  A batched walker has no helper workgroups, so one column is slower than the single solver (n = 20 000: 0.242 s
# against 0.167 s); two columns already are not (0.234 s against 2 x 0.167 s), and the batch's time stays flat up to one column per
# CU (profiles/smo_batched/).  The measured break-even is 2; the constant is 4 so that the fits of two and three columns, which
# earlier commits (and tests/test_gpu_multioutput.py, on three targets) know as per-column fits, stay that — same bits either way.
SMO_MIN_COLUMNS = 4


def takes_batched_smo(k, force=None):
    """The dispatch between the batched SMO solve and one single solver per column for k columns of a configuration the batched
    path covers: `force` (True / False) where given, else k >= SMO_MIN_COLUMNS.  Both give the same bits."""
    return bool(force) if force is not None else int(k) >= SMO_MIN_COLUMNS


class _DeviceSMOSolver:
    """`bq_msmo_create`: k SMO columns on one kernel problem, one walker workgroup each.  task: `_lib.SVC` (Y: k x n labels +-1) or
    `_lib.SVR` (Y: k x n targets); C: k; epsilon: k or None (0); rows: None (every column trains on all rows) or k ascending
    arrays of panel rows; boxes: None, or k x n boxes per column and row (`bq_msmo_create_weighted`; C is not read then, and the
    entries on rows outside a column's list are not either)."""

    def __init__(self, problem, task, Y, C_, epsilon, tol, rows=None, boxes=None):
        self._lib = _lib.load()
        Y = np.ascontiguousarray(np.atleast_2d(Y), dtype=float)
        self.k, self.n = Y.shape
        self.task = task
        self._h = C.c_void_p()
        C_ = _lib.as_f64(np.broadcast_to(np.asarray(C_, dtype=float), (self.k,)), self.k, 'C')
        eps = None if epsilon is None else _lib.as_f64(np.broadcast_to(np.asarray(epsilon, dtype=float), (self.k,)), self.k,
                                                       'epsilon')
        row_ptr = flat = None
        if rows is not None:
            if len(rows) != self.k:
                raise ValueError('%d row lists for %d columns' % (len(rows), self.k))
            row_ptr = np.zeros(self.k + 1, dtype=np.int64)
            row_ptr[1:] = np.cumsum([len(r) for r in rows])
            flat = _lib.as_i32(np.concatenate([np.asarray(r, dtype=np.int64) for r in rows]))
        lists = (None if row_ptr is None else row_ptr.ctypes.data_as(C.POINTER(C.c_int64)),
                 None if flat is None else flat.ctypes.data_as(C.POINTER(C.c_int32)))
        if boxes is None:
            _lib.check(self._lib.bq_msmo_create(problem.handle, task, self.k, _lib.ptr(Y), _lib.ptr(C_), _lib.ptr(eps), float(tol),
                                                *lists, C.byref(self._h)))
        else:
            boxes = _lib.as_f64(boxes, self.k * self.n, 'boxes')
            _lib.check(self._lib.bq_msmo_create_weighted(problem.handle, task, self.k, _lib.ptr(Y), _lib.ptr(boxes), _lib.ptr(eps),
                                                         float(tol), *lists, C.byref(self._h)))

    def run(self, max_outer):
        """at most max_outer launches; (outer, finished, failed), k entries each"""
        outer = np.zeros(self.k, dtype=np.int64)
        fin, failed = np.zeros(self.k, dtype=np.int32), np.zeros(self.k, dtype=np.int32)
        _lib.check(self._lib.bq_msmo_run(self._h, int(max_outer), outer.ctypes.data_as(C.POINTER(C.c_int64)), _lib.iptr(fin),
                                         _lib.iptr(failed)))
        return outer, fin.astype(bool), failed.astype(bool)

    def get(self, c, what):
        size = {_lib.SMO_ALPHAS: self.n * (2 if self.task == _lib.SVR else 1), _lib.SMO_ERRORS: self.n, _lib.SMO_SCALARS: 6}
        out = np.empty(size.get(what, 0))
        _lib.check(self._lib.bq_msmo_get(self._h, int(c), what, _lib.ptr(out)))
        return out

    def vote_heldout(self, ncls, code, group_of, pair_of, held, predictions=False):
        """The (candidate, fold) groups of the pair columns of a classification solver as they stand, finished or not
        (`bq_msmo_vote_heldout`): code, the class code of every row; group_of / pair_of, the group of every column and the number
        of its pair in `ovo_pairs` order, each group holding every pair once; held, groups x n, 1 on the rows a group scores (rows
        in no row list of the group).  Returns (intercept, n_sv, n_held, n_correct[, pred]): per column the solver's intercept and
        the count of multipliers above 1e-6, per group the held rows and those whose one-vs-one vote is their class (-1 for a group
        with a failed column) and, with `predictions`, groups x n predicted classes (-1 on the rows a group does not score)."""
        code = _lib.as_i32(code, self.n, 'code')
        group_of = _lib.as_i32(group_of, self.k, 'group_of')
        pair_of = _lib.as_i32(pair_of, self.k, 'pair_of')
        held = np.ascontiguousarray(np.atleast_2d(held), dtype=np.uint8)
        groups = held.shape[0]
        if held.shape != (groups, self.n):
            raise ValueError('held must be groups x %d' % self.n)
        b, n_sv = np.empty(self.k), np.empty(self.k, dtype=np.int64)
        n_held, n_correct = np.empty(groups, dtype=np.int64), np.empty(groups, dtype=np.int64)
        pred = np.empty((groups, self.n), dtype=np.int32) if predictions else None
        i64, u8 = C.POINTER(C.c_int64), C.POINTER(C.c_ubyte)
        _lib.check(self._lib.bq_msmo_vote_heldout(self._h, int(ncls), _lib.iptr(code), groups, _lib.iptr(group_of),
                                                  _lib.iptr(pair_of), held.ctypes.data_as(u8), _lib.ptr(b), n_sv.ctypes.data_as(i64),
                                                  n_held.ctypes.data_as(i64), n_correct.ctypes.data_as(i64), _lib.iptr(pred)))
        return (b, n_sv, n_held, n_correct, pred) if predictions else (b, n_sv, n_held, n_correct)

    def _sets(self, set_of, held):
        """set_of (k ints) and held (sets x n bytes) as the held-out scorers take them"""
        set_of = _lib.as_i32(set_of, self.k, 'set_of')
        held = np.ascontiguousarray(np.atleast_2d(held), dtype=np.uint8)
        if held.shape[1] != self.n:
            raise ValueError('held must be sets x %d' % self.n)
        return set_of, held

    def svr_heldout(self, set_of, held):
        """(intercept, n_sv, sse, n_held), k entries each, of the columns of a regression solver as they stand, finished or not
        (`bq_msmo_svr_heldout`): held, sets x n, 1 on the rows a set scores; set_of, the set of every column (-1: it scores no
        row; else the column carries a row list that holds none of the set's rows).  Per column the solver's intercept, the count
        of rows with a multiplier above 1e-6, and the squared error and the count of its set's rows.  A column whose walker failed
        has intercept = sse = NaN."""
        set_of, held = self._sets(set_of, held)
        b, sse = np.empty(self.k), np.empty(self.k)
        n_sv, n_held = np.empty(self.k, dtype=np.int64), np.empty(self.k, dtype=np.int64)
        i64 = C.POINTER(C.c_int64)
        _lib.check(self._lib.bq_msmo_svr_heldout(self._h, held.shape[0], _lib.iptr(set_of), held.ctypes.data_as(C.POINTER(C.c_ubyte)),
                                                 _lib.ptr(b), n_sv.ctypes.data_as(i64), _lib.ptr(sse), n_held.ctypes.data_as(i64)))
        return b, n_sv, sse, n_held

    def svc_heldout(self, set_of, held, cal_of, ncal, decisions=False):
        """`_DeviceMultiSolver.heldout_svc` for the columns of a classification solver as they stand (`bq_msmo_svc_heldout`):
        set_of / held as `svr_heldout` takes them, cal_of the calibrator of every column (-1: none).  Returns (intercept, n_sv,
        fit): the solver's intercepts (NaN for a failed walker), the support counts and `platt_fit`'s dict, with `decisions` also
        'dec', the ncal x n decision values (0 on the rows no column of the calibrator scores)."""
        set_of, held = self._sets(set_of, held)
        cal_of = _lib.as_i32(cal_of, self.k, 'cal_of')
        b, n_sv = np.empty(self.k), np.empty(self.k, dtype=np.int64)
        fit, args = _platt_outputs(ncal)
        dec = np.empty((ncal, self.n)) if decisions else None
        _lib.check(self._lib.bq_msmo_svc_heldout(self._h, held.shape[0], _lib.iptr(set_of), held.ctypes.data_as(C.POINTER(C.c_ubyte)),
                                                 int(ncal), _lib.iptr(cal_of), _lib.ptr(b), n_sv.ctypes.data_as(C.POINTER(C.c_int64)),
                                                 *args, _lib.ptr(dec)))
        if decisions:
            fit['dec'] = dec
        return b, n_sv, fit

    def close(self):
        if self._h:
            self._lib.bq_msmo_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def run_batched_smo(solver, chunk=64):
    """Run a `_DeviceSMOSolver`'s columns to the end, `chunk` launches per call: (outer, failed), k entries each — the outer
    iterations done and whether the walker met the reference's 'unexpected status'.  Nothing is raised for a failed column and the
    solver stays open: a search scores its columns on it (`vote_heldout`) before closing it."""
    fin = np.zeros(solver.k, dtype=bool)
    while not fin.all():
        outer, fin, failed = solver.run(chunk)
    return outer, failed


def smo_column_result(solver, c, outer):
    """Column c of a `_DeviceSMOSolver` after `outer` outer iterations as the dict `solve_batched_smo` returns for it, downloaded
    from the walker's state."""
    n = solver.n
    a, sc = solver.get(c, _lib.SMO_ALPHAS), solver.get(c, _lib.SMO_SCALARS)
    r = dict(b_up=sc[0], b_low=sc[1], b_up_idx=int(sc[2]), b_low_idx=int(sc[3]), steps=int(sc[4]), b=sc[5], iter=int(outer),
             errors=solver.get(c, _lib.SMO_ERRORS))
    if solver.task == _lib.SVC:
        r['alphas'] = a
    else:
        r['alphas_p'], r['alphas_n'] = a[:n].copy(), a[n:].copy()
    return r


def solve_batched_smo(problem, task, Y, C_, epsilon, tol, rows=None, cap=None, chunk=64, boxes=None):
    """Run k SMO columns to the end, `cap` columns per solve at most (default: `smo_column_cap` of the memory free now): per column a
    dict of what `SMO.minimize` leaves — alphas (classification) or alphas_p / alphas_n (regression), b, errors, b_up, b_low,
    b_up_idx, b_low_idx, iter, steps.  A column that fails raises what the single fit raises.  boxes: None, or k x n boxes per
    column and row instead of C_ (`_DeviceSMOSolver`)."""
    Y = np.ascontiguousarray(np.atleast_2d(Y), dtype=float)
    k, n = Y.shape
    C_ = np.broadcast_to(np.asarray(C_, dtype=float), (k,))
    epsilon = None if epsilon is None else np.broadcast_to(np.asarray(epsilon, dtype=float), (k,))
    cap = smo_column_cap(n, task, device_free_bytes(), boxes is not None) if cap is None else int(cap)
    out = []
    for c0 in range(0, k, cap):
        sl = slice(c0, min(k, c0 + cap))
        solver = _DeviceSMOSolver(problem, task, Y[sl], C_[sl], None if epsilon is None else epsilon[sl], tol,
                                  None if rows is None else rows[sl], None if boxes is None else boxes[sl])
        try:
            outer, failed = run_batched_smo(solver, chunk)
            if failed.any():   # bq_smo_run's error for that column
                raise smo_failed_error()
            out.extend(smo_column_result(solver, c, outer[c]) for c in range(solver.k))
        finally:
            solver.close()
    return out


def smo_optimizer(quad, X, y, kernel, C_, tol, r, epsilon=None, verbose=False, box=None):
    """The `SMOClassifier` (epsilon None) / `SMORegression` that `minimize()` on `quad` leaves, from its column's result `r` of
    `solve_batched_smo` — constructed, not run.  box: the column's boxes on the rows of X, or None."""
    opt = SMOClassifier(quad, X, y, None, kernel, C_, tol, verbose, box) if epsilon is None else \
        SMORegression(quad, X, y, None, kernel, C_, epsilon, tol, verbose, box)
    for name, value in r.items():
        setattr(opt, name, value)
    opt.helper_stats = {'helpers': 0, 'delivered': 0, 'rejected_list_hash': 0, 'rejected_checksum': 0}
    if isinstance(kernel, LinearKernel):
        opt.w = opt._coefficients() @ opt.X
    return opt


def fitted_smo_svc(est, quad, r, X, y, box=None):
    """Make `est`, a fresh SVC of the configuration, the SVC that SVC.fit's SMO branch on (X, y: +-1) leaves, intercept included,
    from its column's result `r` of `solve_batched_smo`; quad: the class's view of the shared panel; box: the boxes `est`'s
    `class_weight` gives the rows of X, or None.  Returns the support mask."""
    est.obj = quad
    est.optimizer = smo_optimizer(quad, X, y, est.kernel, est.C, est.tol, r, verbose=est.verbose, box=box)
    sv = _svc_attributes(est, X, y, est.optimizer.alphas)
    if isinstance(est.kernel, LinearKernel):
        est.coef_ = est.optimizer.w
    est.intercept_ = est.optimizer.b
    return sv


def fitted_smo_svr(est, quad, r, X, y):
    """`fitted_smo_svc` for an SVR on the targets y; quad: the target's view of the shared panel."""
    est.obj = quad
    est.optimizer = smo_optimizer(quad, X, y, est.kernel, est.C, est.tol, r, epsilon=est.epsilon, verbose=est.verbose)
    sv = _svr_attributes(est, X, y, np.concatenate((est.optimizer.alphas_p, est.optimizer.alphas_n)))
    if isinstance(est.kernel, LinearKernel):
        est.coef_ = est.optimizer.w
    est.intercept_ = est.optimizer.b
    return sv


def uses_batched_smo(est, loss, world, weighted=False):
    """What `uses_batched_smo_path` (multiclass.py) and `uses_batched_smo_svr_path` (multioutput.py) share: `est`'s configuration
    takes the SMO branch of its `fit` (dual, optimizer 'smo' or `SMO`, the loss `loss`, an unregularised intercept) on a resident
    panel ('f64' / 'f32') in a single-rank context (`world` ranks).  An estimator with a `class_weight` only where the caller
    hands its columns their boxes (`weighted`)."""
    if has_class_weight(est) and not weighted:
        return False
    return bool(est._is_smo() and est.loss == loss and not est.reg_intercept and est.storage in ('f64', 'f32') and int(world) == 1)


def solver_kind(optimizer):
    return _lib.PG if issubclass(optimizer, ProjectedGradient) else _lib.FW


def _pair_array(pairs):
    return _lib.as_i32(np.asarray(pairs, dtype=np.int32).reshape(-1))


def _data_row(data_row, n):
    """the uint8 row mask of a class-sorted panel of n rows (1 a data row, 0 a ghost row)"""
    data_row = np.ascontiguousarray(data_row, dtype=np.uint8)
    if data_row.shape != (n,):
        raise ValueError('data_row must have %d entries' % n)
    return data_row


class _DeviceMultiSolver:
    """k columns on one panel.  `n` is the length of a column's vectors, the dual dimension: Y's row length — the panel's n for
    the SVC solvers, 2n for `_DeviceSVRSolver`, whose rows are the linear terms."""

    def __init__(self, problem, kind, Y, ub, eps, max_iter, t=0.0, x0=None):
        self._lib = _lib.load()
        self.k, self.n = Y.shape
        self._h = C.c_void_p()
        Y = _lib.as_f64(Y, self.k * self.n, 'Y')
        _lib.check(self._create(problem.handle, kind, Y, ub, x0, float(eps), int(max_iter), float(t)))

    def _x0(self, x0):
        return None if x0 is None else _lib.as_f64(x0, self.k * self.n, 'x0')

    def _create(self, handle, kind, Y, ub, x0, eps, max_iter, t):
        """The create call, the one part a subclass replaces; it converts ub, then x0 (`_x0`)."""
        boxes = np.ndim(ub) == 2   # one box per column (k x n): bq_msolver_create_boxes and the 16-column product
        ub = _lib.as_f64(ub, self.k * self.n if boxes else self.n, 'ub')
        x0 = self._x0(x0)
        create = self._lib.bq_msolver_create_boxes if boxes else self._lib.bq_msolver_create
        return create(handle, kind, self.k, _lib.ptr(Y), _lib.ptr(ub), _lib.ptr(x0), eps, max_iter, t, C.byref(self._h))

    def run(self, max_steps):
        stats = np.zeros((self.k, max_steps), dtype=_lib.STAT_DTYPE)
        n = np.zeros(self.k, dtype=np.int64)
        status = np.zeros(self.k, dtype=np.int32)
        _lib.check(self._lib.bq_msolver_run(self._h, max_steps, stats.ctypes.data_as(C.POINTER(_lib.IterStat)), max_steps,
                                            n.ctypes.data_as(C.POINTER(C.c_int64)), status.ctypes.data_as(C.POINTER(C.c_int))))
        if (status < 0).any():
            raise ValueError('array must not contain infs or NaNs')
        return [stats[c, :n[c]] for c in range(self.k)], [_lib.STATUS[int(s)] for s in status]

    def state(self, c):
        it, st, f = C.c_int64(0), C.c_int(0), C.c_double(0)
        _lib.check(self._lib.bq_msolver_state(self._h, c, C.byref(it), C.byref(st), C.byref(f)))
        return it.value, _lib.STATUS.get(st.value, 'unknown'), f.value

    def get(self, c, what):
        out = np.empty(self.n)
        _lib.check(self._lib.bq_msolver_get(self._h, c, what, _lib.ptr(out)))
        return out

    def _heldout(self, call, cal_of, ncal, decisions, *data_row):
        """`heldout_svc` and, with a data_row, `heldout_pairs`"""
        cal_of = _lib.as_i32(cal_of, self.k, 'cal_of')
        rows = [_data_row(d, self.n).ctypes.data_as(C.POINTER(C.c_ubyte)) for d in data_row]
        b, n_sv = np.empty(self.k), np.empty(self.k, dtype=np.int64)
        fit, args = _platt_outputs(ncal)
        dec = np.empty((ncal, self.n)) if decisions else None
        _lib.check(call(self._h, *rows, int(ncal), _lib.iptr(cal_of), _lib.ptr(b), n_sv.ctypes.data_as(C.POINTER(C.c_int64)), *args,
                        _lib.ptr(dec)))
        if decisions:
            fit['dec'] = dec
        return b, n_sv, fit

    def heldout_svc(self, cal_of, ncal, decisions=False):
        """The columns of a one-box-per-column SVC solver as they stand (`bq_msolver_svc_heldout`): per column SVC.fit's
        intercept and support count (NaN without a support vector), and per calibrator the Platt fit (`platt_fit`'s dict) on the
        held-out decision values of the columns c with cal_of[c] == that calibrator (-1: the column feeds none); with
        `decisions`, the dict also holds 'dec', the ncal x n decision values (0 on the rows no column of the calibrator holds
        out).  Returns (intercept, n_sv, fit)."""
        return self._heldout(self._lib.bq_msolver_svc_heldout, cal_of, ncal, decisions)

    def heldout_pairs(self, data_row, cal_of, ncal, decisions=False):
        """`heldout_svc` for the columns of a pair solver (`_DevicePairSolver`, `bq_msolver_pairs_heldout`): a column's held-out
        rows are the data rows (data_row: n entries, 1 a data row, 0 a ghost row) of its pair's two classes whose box is 0.
        Returns (intercept, n_sv, fit)."""
        return self._heldout(self._lib.bq_msolver_pairs_heldout, cal_of, ncal, decisions, data_row)

    def vote_heldout_pairs(self, data_row, group_of, held, predictions=False):
        """The (candidate, fold) groups of a pair solver's columns as they stand (`_DevicePairSolver`,
        `bq_msolver_pairs_vote_heldout`): group_of, the group of every column, each group holding every class pair once; held,
        groups x n, 1 on the rows a group scores (data rows none of its columns trained on).  Returns (intercept, n_sv, n_held,
        n_correct[, pred]): per column SVC.fit's intercept and support count (NaN without a support vector), per group the held rows
        and those whose one-vs-one vote is their class (-1 for a group with a NaN intercept) and, with `predictions`, groups x n
        predicted classes (-1 on the rows a group does not score)."""
        group_of = _lib.as_i32(group_of, self.k, 'group_of')
        data_row = _data_row(data_row, self.n)
        held = np.ascontiguousarray(np.atleast_2d(held), dtype=np.uint8)
        groups = held.shape[0]
        if held.shape != (groups, self.n):
            raise ValueError('held must be groups x %d' % self.n)
        b, n_sv = np.empty(self.k), np.empty(self.k, dtype=np.int64)
        n_held, n_correct = np.empty(groups, dtype=np.int64), np.empty(groups, dtype=np.int64)
        pred = np.empty((groups, self.n), dtype=np.int32) if predictions else None
        i64, u8 = C.POINTER(C.c_int64), C.POINTER(C.c_ubyte)
        _lib.check(self._lib.bq_msolver_pairs_vote_heldout(self._h, data_row.ctypes.data_as(u8), groups, _lib.iptr(group_of),
                                                           held.ctypes.data_as(u8), _lib.ptr(b), n_sv.ctypes.data_as(i64),
                                                           n_held.ctypes.data_as(i64), n_correct.ctypes.data_as(i64),
                                                           _lib.iptr(pred)))
        return (b, n_sv, n_held, n_correct, pred) if predictions else (b, n_sv, n_held, n_correct)

    def close(self):
        if self._h:
            self._lib.bq_msolver_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _platt_outputs(ncal):
    """The per-calibrator result arrays of `bq_platt_fit` / `bq_msolver_svc_heldout` and their pointers in the C argument order"""
    fit = dict(A=np.empty(ncal), B=np.empty(ncal), iters=np.empty(ncal, dtype=np.int32), loss=np.empty(ncal),
               n_pos=np.empty(ncal, dtype=np.int64), n_neg=np.empty(ncal, dtype=np.int64), flags=np.empty(ncal, dtype=np.int32))
    i64 = C.POINTER(C.c_int64)
    args = (_lib.ptr(fit['A']), _lib.ptr(fit['B']), _lib.iptr(fit['iters']), _lib.ptr(fit['loss']),
            fit['n_pos'].ctypes.data_as(i64), fit['n_neg'].ctypes.data_as(i64), _lib.iptr(fit['flags']))
    return fit, args


def platt_fit(D, L):
    """Platt's sigmoid p = 1 / (1 + exp(A f + B)) of every row of D (ncal x n decision values) with the labels L (ncal x n: +1, -1,
    or 0 for a row outside the calibrator's sample), all on the device in one launch (`bq_platt_fit`): a dict of the arrays A, B,
    iters, loss, n_pos, n_neg and flags (`_lib.PLATT_*`), ncal entries each."""
    D = np.ascontiguousarray(np.atleast_2d(D), dtype=float)
    L = np.ascontiguousarray(np.atleast_2d(L), dtype=float)
    if D.shape != L.shape:
        raise ValueError('decision values (%d x %d) and labels (%d x %d) do not match' % (D.shape + L.shape))
    ncal, n = D.shape
    fit, args = _platt_outputs(ncal)
    _lib.check(_lib.load().bq_platt_fit(get_context().handle, ncal, n, _lib.ptr(D), _lib.ptr(L), *args))
    return fit


class _DeviceSVRSolver(_DeviceMultiSolver):
    """`bq_msolver_create_svr`: one column per target on a 'svr' problem.  QL: k x 2n linear terms ([-y_c; y_c] + epsilon), ub: 2n,
    or k x 2n for one box per column (`bq_msolver_create_svr_boxes` and the 16-column product: the columns of a search, which
    `heldout` scores), x0: k x 2n or None; every vector the solver hands out has 2n entries."""

    def _create(self, handle, kind, QL, ub, x0, eps, max_iter, t):
        boxes = np.ndim(ub) == 2
        ub = _lib.as_f64(ub, self.k * self.n if boxes else self.n, 'ub')
        x0 = self._x0(x0)
        create = self._lib.bq_msolver_create_svr_boxes if boxes else self._lib.bq_msolver_create_svr
        return create(handle, kind, self.k, _lib.ptr(QL), _lib.ptr(ub), _lib.ptr(x0), eps, max_iter, t, C.byref(self._h))

    def heldout(self, y, epsilons):
        """(intercept, n_sv, sse, n_held), k entries each, of the columns as they stand (`bq_msolver_svr_heldout`): SVR.fit's
        intercept and support count, and the squared error and count of the rows whose box is 0 on both halves.  y: n targets,
        epsilons: k.  A column without support vectors has intercept = sse = NaN."""
        y = _lib.as_f64(y, self.n // 2, 'y')
        eps = _lib.as_f64(epsilons, self.k, 'epsilons')
        b, sse = np.empty(self.k), np.empty(self.k)
        n_sv, n_held = np.empty(self.k, dtype=np.int64), np.empty(self.k, dtype=np.int64)
        i64 = C.POINTER(C.c_int64)
        _lib.check(self._lib.bq_msolver_svr_heldout(self._h, _lib.ptr(y), _lib.ptr(eps), _lib.ptr(b), n_sv.ctypes.data_as(i64),
                                                    _lib.ptr(sse), n_held.ctypes.data_as(i64)))
        return b, n_sv, sse, n_held


class _DeviceSimplexSolver(_DeviceMultiSolver):
    """`bq_msolver_create_simplex`: k nu-one-class duals min 1/2 x'Kx over {0 <= x <= UB[c], sum x = mass[c]} on one 'plain'
    problem.  UB: k x n boxes (a zero-width entry: a row the column does not train on), mass: k, x0: k x n or None (the projection
    of 0); tol: the bound on libsvm's maximal-violating-pair measure.  The records' r1, r2, r3 are that measure, the step length
    and the spectral step."""

    def __init__(self, problem, UB, mass, tol, max_iter, x0=None):
        UB = np.ascontiguousarray(np.atleast_2d(UB), dtype=float)
        self._mass = _lib.as_f64(mass, UB.shape[0], 'mass')
        _DeviceMultiSolver.__init__(self, problem, None, UB, None, tol, max_iter, x0=x0)

    def _create(self, handle, kind, UB, ub, x0, eps, max_iter, t):
        x0 = self._x0(x0)
        return self._lib.bq_msolver_create_simplex(handle, self.k, _lib.ptr(UB), _lib.ptr(self._mass), _lib.ptr(x0), eps, max_iter,
                                                   C.byref(self._h))

    def offsets(self):
        """(rho, n_sv, n_free), k entries each, of the columns as they stand (`bq_msolver_simplex_offsets`): libsvm's
        calculate_rho, the rows with x > 0 and the rows strictly inside their box."""
        rho = np.empty(self.k)
        n_sv, n_free = np.empty(self.k, dtype=np.int64), np.empty(self.k, dtype=np.int64)
        i64 = C.POINTER(C.c_int64)
        _lib.check(self._lib.bq_msolver_simplex_offsets(self._h, _lib.ptr(rho), n_sv.ctypes.data_as(i64), n_free.ctypes.data_as(i64)))
        return rho, n_sv, n_free


class _DeviceSimplex2Solver(_DeviceMultiSolver):
    """`bq_msolver_create_simplex2`: k two-group columns (the nu-SVC / nu-SVR duals) on one 'plain' problem of n rows.  S: k x n
    labels +-1 (the LABELS layout, m = n variables, group 0 the rows with +1) or None (PAIRED, m = 2n, group 0 the first n); UB:
    k x m boxes; mass: k x 2, one per group; q: k x m linear terms or None (0); x0: k x m or None (the projection of 0 per group).
    Every vector the solver hands out has m entries; the records are `_DeviceSimplexSolver`'s."""

    def __init__(self, problem, S, UB, mass, q, tol, max_iter, x0=None):
        UB = np.ascontiguousarray(np.atleast_2d(UB), dtype=float)
        k, m = UB.shape
        n = problem.dims()[1]
        if m != (2 * n if S is None else n):   # (the library reads k x m entries of UB, q and x0)
            raise ValueError('UB has %d columns, expected %d' % (m, 2 * n if S is None else n))
        self._rows = n
        self._layout = _lib.SX_PAIRED if S is None else _lib.SX_LABELS
        self._S = None if S is None else _lib.as_f64(S, k * m, 'S')
        self._mass = _lib.as_f64(mass, 2 * k, 'mass')
        self._q = None if q is None else _lib.as_f64(q, k * m, 'q')
        _DeviceMultiSolver.__init__(self, problem, None, UB, None, tol, max_iter, x0=x0)

    def _create(self, handle, kind, UB, ub, x0, eps, max_iter, t):
        x0 = self._x0(x0)
        return self._lib.bq_msolver_create_simplex2(handle, self.k, self._layout, _lib.ptr(self._S), _lib.ptr(UB),
                                                    _lib.ptr(self._mass), _lib.ptr(self._q), _lib.ptr(x0), eps, max_iter,
                                                    C.byref(self._h))

    def offsets(self):
        """(r1, r2, n_sv, n_free) of the columns as they stand (`bq_msolver_simplex2_offsets`): libsvm's Solver_NU::calculate_rho
        per group (k entries each), and per (column, group) the rows with x > 0 and the rows strictly inside their box (k x 2)."""
        r1, r2 = np.empty(self.k), np.empty(self.k)
        n_sv, n_free = np.empty((self.k, 2), dtype=np.int64), np.empty((self.k, 2), dtype=np.int64)
        i64 = C.POINTER(C.c_int64)
        _lib.check(self._lib.bq_msolver_simplex2_offsets(self._h, _lib.ptr(r1), _lib.ptr(r2), n_sv.ctypes.data_as(i64),
                                                         n_free.ctypes.data_as(i64)))
        return r1, r2, n_sv, n_free

    def heldout(self, y):
        """(r1, r2, n_sv, n_free, n_held, n_correct, sse) of the columns as they stand (`bq_msolver_simplex2_heldout`): `offsets()`'s
        four, and per column (k entries each) the rows whose box is 0 (on both halves), how many of them the column's NuSVC predicts
        as y says (LABELS; y: the n labels +-1) and the squared error of its NuSVR's predictions on them (PAIRED; y: the n
        targets).  The count is 0 for PAIRED, the squared error 0 for LABELS.  The solver must have run; a
        `_DeviceSimplexPairSolver` is refused."""
        y = _lib.as_f64(y, self._rows, 'y')
        r1, r2, sse = np.empty(self.k), np.empty(self.k), np.empty(self.k)
        n_sv, n_free = np.empty((self.k, 2), dtype=np.int64), np.empty((self.k, 2), dtype=np.int64)
        n_held, n_correct = np.empty(self.k, dtype=np.int64), np.empty(self.k, dtype=np.int64)
        i64 = C.POINTER(C.c_int64)
        _lib.check(self._lib.bq_msolver_simplex2_heldout(self._h, _lib.ptr(y), _lib.ptr(r1), _lib.ptr(r2), n_sv.ctypes.data_as(i64),
                                                         n_free.ctypes.data_as(i64), n_held.ctypes.data_as(i64),
                                                         n_correct.ctypes.data_as(i64), _lib.ptr(sse)))
        return r1, r2, n_sv, n_free, n_held, n_correct, sse


class _DeviceSimplexPairSolver(_DeviceSimplex2Solver):
    """`bq_msolver_create_simplex2_pairs`: k two-group columns on a class-sorted 'plain' problem of n rows with the pair-routed
    product.  cls_tiles: the classes' tile rows (`sort_plan`); pairs: k class pairs (a, b), a < b, one per column (a pair may
    repeat); UB: k x n boxes, 0 outside the pair's rows; mass: k x 2, group 0 class b (+1), group 1 class a (-1); x0: k x n or
    None.  Every vector the solver hands out has n entries, in panel order; `offsets()` as `_DeviceSimplex2Solver`'s."""

    def __init__(self, problem, cls_tiles, pairs, UB, mass, tol, max_iter, x0=None):
        UB = np.ascontiguousarray(np.atleast_2d(UB), dtype=float)
        k, m = UB.shape
        n = problem.dims()[1]
        if m != n:   # (the library reads k x n entries of UB and x0)
            raise ValueError('UB has %d columns, expected %d' % (m, n))
        self._rows = n
        self._ct, self._pr = _lib.as_i32(cls_tiles), _pair_array(pairs)
        if self._pr.size != 2 * k:
            raise ValueError('%d pairs for %d columns' % (self._pr.size // 2, k))
        self._mass = _lib.as_f64(mass, 2 * k, 'mass')
        _DeviceMultiSolver.__init__(self, problem, None, UB, None, tol, max_iter, x0=x0)

    def _create(self, handle, kind, UB, ub, x0, eps, max_iter, t):
        x0 = self._x0(x0)
        return self._lib.bq_msolver_create_simplex2_pairs(handle, len(self._ct) - 1, _lib.iptr(self._ct), self.k,
                                                          _lib.iptr(self._pr), _lib.ptr(UB), _lib.ptr(self._mass), _lib.ptr(x0),
                                                          eps, max_iter, C.byref(self._h))


def simplex_project(V, UB, mass):
    """The Euclidean projection of every row of V (k x n) onto {0 <= p <= UB[c], sum p = mass[c]} by the simplex solver's projection
    kernel (`bq_simplex_project`), one workgroup per row."""
    V = np.ascontiguousarray(np.atleast_2d(V), dtype=float)
    k, n = V.shape
    UB = _lib.as_f64(UB, k * n, 'UB')
    mass = _lib.as_f64(mass, k, 'mass')
    P = np.empty_like(V)
    _lib.check(_lib.load().bq_simplex_project(get_context().handle, k, n, _lib.ptr(V), _lib.ptr(UB), _lib.ptr(mass), _lib.ptr(P)))
    return P


class _DeviceALSolver(_DeviceMultiSolver):
    """`bq_msolver_create_al`: k augmented-Lagrangian columns on one 'svc' or 'svr' problem.  prm: the rule's `_lib.AlParams`
    (`StochasticOptimizer._params`); x0: k x N, required; Y: k x n labels +-1 ('svc') or QL: k x 2n linear terms ('svr'); a: the
    equality row, None, N entries (one row for every column) or k x N (one per column); lb, ub: N each or None, shared; dual0:
    k x n_dual or None (zeros).  `get(c, _lib.GET_DUAL)` has `n_dual` entries, every other vector N."""

    def __init__(self, problem, prm, x0, Y=None, QL=None, a=None, lb=None, ub=None, dual0=None):
        self._lib = _lib.load()
        x0 = np.ascontiguousarray(x0, dtype=float)
        self.k, self.n = x0.shape
        self._h = C.c_void_p()
        k, N = self.k, self.n
        vec = lambda v, size, name: None if v is None else _lib.as_f64(v, size, name)   # noqa: E731
        per_column = a is not None and np.ndim(a) == 2
        Y = vec(Y, k * problem.dims()[1], 'Y')
        QL, a = vec(QL, k * N, 'QL'), vec(a, k * N if per_column else N, 'A')
        lb, ub = vec(lb, N, 'lb'), vec(ub, N, 'ub')
        self.n_dual = (a is not None) + N * ((lb is not None) + (ub is not None))
        dual0 = None if dual0 is None or self.n_dual == 0 else _lib.as_f64(dual0, k * self.n_dual, 'dual_x')
        _lib.check(self._lib.bq_msolver_create_al(problem.handle, C.byref(prm), k, _lib.ptr(Y), _lib.ptr(QL), _lib.ptr(a),
                                                  N if per_column else 0, _lib.ptr(lb), _lib.ptr(ub), _lib.ptr(x0),
                                                  _lib.ptr(dual0), C.byref(self._h)))

    def get(self, c, what):
        out = np.empty(self.n_dual if what == _lib.GET_DUAL else self.n)
        if out.size:
            _lib.check(self._lib.bq_msolver_get(self._h, c, what, _lib.ptr(out)))
        return out


def solve_batched_al(solver, chunk=256):
    """Run a `_DeviceALSolver` to the end and close it: per column a dict as a single `StochasticOptimizer.minimize` ends (rows:
    the iteration records, status, iter, f_x; x: the current point, past_x: the point of the last record, g, step, dual)."""
    try:
        rows = [[] for _ in range(solver.k)]
        status = ['unknown'] * solver.k
        while 'unknown' in status:
            recs, status = solver.run(chunk)
            for c in range(solver.k):
                rows[c].append(recs[c])
        out = []
        for c in range(solver.k):
            it, st, f = solver.state(c)
            out.append(dict(rows=np.concatenate(rows[c]), status=st, iter=it, f_x=f, x=solver.get(c, _lib.GET_X_NOW),
                            past_x=solver.get(c, _lib.GET_X), g=solver.get(c, _lib.GET_G), step=solver.get(c, _lib.GET_D),
                            dual=solver.get(c, _lib.GET_DUAL)))
        return out
    finally:
        solver.close()


def uses_batched_lagrangian(est, losses, world, ndim=None):
    """What `uses_batched_lagrangian_path` (multiclass.py) and `uses_batched_lagrangian_svr_path` (multioutput.py) share: `est`'s
    configuration takes the augmented-Lagrangian branch of its `fit` (dual, a `StochasticOptimizer`, a loss of `losses`) in the form
    `bq_msolver_create_al` batches: momentum 'none' or 'polyak' and constant (Nesterov momentum and schedules run one fit per
    column), a resident panel ('f64' / 'f32'), a single-rank context (`world` ranks) and, where the dual's size `ndim` is given,
    more than 3 variables (with <= 3 the optimizer keeps per-iteration x histories and runs step by step).  An estimator with a
    `class_weight` fits per column: the batched solver shares one box among its columns."""
    opt = est.optimizer
    if not (est.dual and isinstance(opt, type) and issubclass(opt, StochasticOptimizer)):
        return False
    if issubclass(opt, StochasticMomentumOptimizer) and isinstance(est.momentum, Iterable):
        return False
    return bool(est.momentum_type in ('none', 'polyak') and est.loss in losses and est.storage in ('f64', 'f32') and
                int(world) == 1 and (ndim is None or int(ndim) > 3) and not has_class_weight(est))


def solve_batched(problem, kind, Y, ub, eps=1e-6, max_iter=1000, t=0.0, x0=None, chunk=256, solver=None, before_close=None,
                  vectors=True):
    """Run the batched solver (`problem`: a device problem of KernelQuadratic 'svc'; Y: k x n labels +-1; ub: n, or k x n for one box
    per column (bq_msolver_create_boxes); x0: k x n or None)
    to the end: per class a dict (rows: the iteration records, status, iter, f_x, x, g) as a single-class optimizer ends them.
    solver: an already created solver of these columns instead of bq_msolver_create(_boxes); only Y's row count is read then, and
    x, g have the solver's column length (2n for a `_DeviceSVRSolver`).
    before_close: called as before_close(solver, out) on the live solver after the last run, before it is closed (a search scores
    its columns there, `_DeviceSVRSolver.heldout`); vectors=False leaves x and g on the device (no such keys)."""
    solver = _DeviceMultiSolver(problem, kind, Y, ub, eps, max_iter, t, x0) if solver is None else solver
    k = Y.shape[0]
    try:
        rows = [[] for _ in range(k)]
        status = ['unknown'] * k
        while 'unknown' in status:
            recs, status = solver.run(chunk)
            for c in range(k):
                rows[c].append(recs[c])
        out = []
        for c in range(k):
            it, st, f = solver.state(c)
            out.append(dict(rows=np.concatenate(rows[c]), status=st, iter=it, f_x=f))
            if vectors:
                out[c].update(x=solver.get(c, _lib.GET_X_NOW), g=solver.get(c, _lib.GET_G_NOW))
        if before_close is not None:
            before_close(solver, out)
        return out
    finally:
        solver.close()


def _gram_matmat(problem, W, wide=False):
    """OUT[c] = K W[c] for the rows of W, one multi-column product (bq_problem_gram_matmat; wide: the 16-column
    bq_problem_gram_matmat_wide)."""
    W = np.ascontiguousarray(W, dtype=float)
    out = np.empty_like(W)
    fn = _lib.load().bq_problem_gram_matmat_wide if wide else _lib.load().bq_problem_gram_matmat
    _lib.check(fn(problem.handle, W.shape[0], _lib.ptr(W), _lib.ptr(out)))
    return out


def gram_matmat_pairs(problem, cls_tiles, pairs, W):
    """OUT[p] = K W[p] on the rows of pair p's classes and 0 elsewhere, one routed product (bq_problem_gram_matmat_pairs)."""
    W = np.ascontiguousarray(W, dtype=float)
    out = np.empty_like(W)
    ct, pr = _lib.as_i32(cls_tiles), _pair_array(pairs)
    _lib.check(_lib.load().bq_problem_gram_matmat_pairs(problem.handle, len(ct) - 1, _lib.iptr(ct), W.shape[0], _lib.iptr(pr),
                                                        _lib.ptr(W), _lib.ptr(out)))
    return out


def uses_batched_decision(kernel, k, world, batched):
    """True when the k estimators of a batched fit predict through one fused pass (`batched_decision`) instead of one
    `decision_function` call each: the fit ran on the batched path (`batched`), k >= 2, a single-rank context (`world` ranks) and a
    Gaussian, polynomial or sigmoid kernel whose gamma is not 'scale'.  'scale' resolves against each estimator's own support
    vectors at prediction (`SVM.decision_function`), so the estimators have different kernels and share no kernel value; the
    linear kernel predicts from `coef_` on the host; the Laplacian kernel has no GEMM form.  The fallback fits promise the bits of
    the per-estimator calls and keep them."""
    return bool(batched and int(k) >= 2 and int(world) == 1 and isinstance(kernel, (GaussianKernel, PolyKernel, SigmoidKernel)) and
                getattr(kernel, 'gamma', None) != 'scale')


def batched_decision(spec, SV, W, b, X):
    """t x k decision values of k coefficient rows on shared support vectors in one pass over the kernel values
    (`bq_decision_function_multi`): kernel(X, SV) W' + b.  spec: the kernel's `device_spec` (gamma resolved); SV: m x d; W: k x m;
    b: k intercepts; X: t x d."""
    kind, gamma, coef0, degree = spec
    SV = np.ascontiguousarray(SV, dtype=float)
    X = np.ascontiguousarray(X, dtype=float)
    W = np.ascontiguousarray(W, dtype=float)
    k, m = W.shape
    if SV.shape[0] != m or X.shape[1] != SV.shape[1]:
        raise ValueError('shapes of SV (%d x %d), W (%d x %d) and X (%d x %d) do not match' % (SV.shape + W.shape + X.shape))
    b = _lib.as_f64(b, k, 'b')
    out = np.empty((k, X.shape[0]))
    _lib.check(_lib.load().bq_decision_function_multi(get_context().handle, kind, gamma, coef0, degree, m, SV.shape[1],
                                                      _lib.ptr(SV), k, _lib.ptr(W), _lib.ptr(b), X.shape[0], _lib.ptr(X),
                                                      _lib.ptr(out)))
    return np.ascontiguousarray(out.T)


class DecisionBatch:
    """What a batched fit keeps for `batched_decision`: the kernel spec, the union of the estimators' support vectors (the rows
    with a nonzero coefficient in any column), the k x m coefficients on that union and the k intercepts — the estimators as `fit`
    left them; later changes to `estimators_` are not seen.  coefs: k x n on the rows of X; `keep` masks rows that may enter
    (OneVsOneSVC's ghost rows may not)."""

    def __init__(self, kernel, X, coefs, intercepts, keep=None):
        coefs = np.asarray(coefs, dtype=float)
        rows = (coefs != 0).any(axis=0)
        if keep is not None:
            rows &= keep
        self.spec = kernel.device_spec(X)   # gamma is numeric or 'auto' here: it does not depend on the rows
        self.rows = np.flatnonzero(rows)
        self.SV = np.ascontiguousarray(X[self.rows])
        self.W = np.ascontiguousarray(coefs[:, self.rows])
        self.b = np.array(intercepts, dtype=float)

    def __call__(self, X):
        return batched_decision(self.spec, self.SV, self.W, self.b, X)


def fitted_svc(est, quad, r, X, y, pos=None):
    """Make `est`, a fresh SVC of the configuration, the SVC that SVC.fit on (X, y: +-1) leaves, from its column's result `r` of
    `solve_batched` on `quad`'s panel (pos: the panel rows of X's rows, in their order, where the panel holds other rows too).
    Returns the support mask; the intercept needs a product and is left to the caller (`intercept`)."""
    n = len(y)
    x, g = (r['x'], r['g']) if pos is None else (r['x'][pos], r['g'][pos])
    # the optimizer as SVC.fit leaves it (constrained/_base.py: minimize) — constructed, not run
    opt = est.optimizer(quad=quad, ub=np.ones(n) * est.C, tol=est.tol, max_iter=est.max_iter, verbose=est.verbose)
    if len(r['rows']):
        opt.iter = int(r['rows'][-1]['iter'])
        opt._after_row(r['rows'][-1])
    opt.status, opt.f_x, opt.x, opt.g_x = r['status'], r['f_x'], x, g
    est.train_loss_history = [float(f) for f in r['rows']['f']]
    est.optimizer = opt
    return _svc_attributes(est, X, y)


def _svc_attributes(est, X, y, alphas=None):
    """What SVC.fit derives from `est.optimizer.x` (y: +-1; alphas: the multipliers of an optimizer that keeps them elsewhere) but
    the intercept; returns the support mask."""
    est.classes_ = np.array([0, 1])   # OneVsRestClassifier and OneVsOneClassifier fit each SVC on 0 / 1 labels
    est.alphas_ = est.optimizer.x if alphas is None else alphas
    sv = est.alphas_ > 1e-6
    est.support_ = np.arange(len(y))[sv]
    est.support_vectors_ = X[sv]
    est.dual_coef_ = est.alphas_[sv] * y[sv]
    if isinstance(est.kernel, LinearKernel):
        est.coef_ = np.dot(est.dual_coef_, est.support_vectors_)
    return sv


def intercept(y, u, sv):
    """SVC.fit's intercept of the regularised-intercept dual from u = K (alpha y) on the support vectors `sv`, statement for
    statement."""
    b = 0.
    b += float(np.sum(y[sv] - u[sv]))
    b /= int(sv.sum())
    return b


class TargetQuadratic(KernelQuadratic):
    """One target's dual on the panel of a shared 'svr' `KernelQuadratic`: the same X, kernel and device problem, its own linear
    term q.  `function` / `jacobian` are 1/2 x'Qx + q'x and Qx + q with Qx from the shared panel (`bq_problem_matvec`, which does
    not read the device problem's q); `release` is left to the shared object, and `x_star`, which the device takes from the
    problem's own q, is not offered."""

    def __init__(self, shared, q):
        self.__dict__.update(shared.__dict__)
        self._shared = shared
        self._dev = None
        self.q = np.array(q, dtype=float)
        if self.q.size != self.ndim:
            raise ValueError('q size does not match with Q')

    def device_problem(self, ctx=None):
        return self._shared.device_problem(ctx)

    def release(self):
        pass

    def x_star(self):
        raise NotImplementedError('a target\'s view of a shared panel has no x_star: build KernelQuadratic(X, q, \'svr\', kernel)')

    def function_jacobian(self, x):
        x = np.asarray(x, dtype=float)
        Qx = self.device_problem().matvec(x)
        return 0.5 * float(x @ Qx) + float(self.q @ x), Qx + self.q

    def function(self, x):
        return self.function_jacobian(x)[0]

    def jacobian(self, x):
        return self.function_jacobian(x)[1]


def fitted_svr(est, quad, r, X, y):
    """Make `est`, a fresh SVR of the configuration, the SVR that SVR.fit on (X, y) leaves, from its column's result `r` (x, g: 2n)
    of `solve_batched` on `quad`'s panel.  Its optimizer's function is the target's own dual (`TargetQuadratic`: the shared panel
    with q = [-y; y] + epsilon).  Returns the support mask; the intercept needs a product and is left to the caller
    (`svr_intercept`)."""
    n = len(y)
    quad = TargetQuadratic(quad, np.hstack((-y, y)) + est.epsilon)
    # the optimizer as SVR.fit leaves it (constrained/_base.py: minimize) — constructed, not run
    opt = est.optimizer(quad=quad, ub=np.ones(2 * n) * est.C, tol=est.tol, max_iter=est.max_iter, verbose=est.verbose)
    if len(r['rows']):
        opt.iter = int(r['rows'][-1]['iter'])
        opt._after_row(r['rows'][-1])
    opt.status, opt.f_x, opt.x, opt.g_x = r['status'], r['f_x'], r['x'], r['g']
    est.train_loss_history = [float(f) for f in r['rows']['f']]
    est.optimizer = opt
    est.obj = quad
    return _svr_attributes(est, X, y)


def _svr_attributes(est, X, y, alphas=None):
    """What SVR.fit derives from `est.optimizer.x` (2n; alphas: the multipliers of an optimizer that keeps them elsewhere) but
    the intercept; returns the support mask."""
    est.alphas_ = est.optimizer.x if alphas is None else alphas
    alphas_p, alphas_n = np.split(est.alphas_, 2)
    sv = np.logical_or(alphas_p > 1e-6, alphas_n > 1e-6)
    est.support_ = np.arange(len(y))[sv]
    est.support_vectors_ = X[sv]
    est.dual_coef_ = alphas_p[sv] - alphas_n[sv]
    if isinstance(est.kernel, LinearKernel):
        est.coef_ = np.dot(est.dual_coef_, est.support_vectors_)
    return sv


class ClassQuadratic(TargetQuadratic):
    """One class's dual on the panel of a shared 'svc' `KernelQuadratic`: the same X, kernel, q and device problem, its own labels
    y_c, so Q_c = diag(y_c) P diag(y_c) (+ diag I).  The device problem applies the shared labels y_0: with s = y_c o y_0,
    Q_c x = s o (Q_0 (s o x)) — the diagonal term passes through, s o s = 1.  `Q` and `gram` read `self.y`, the class's."""

    def __init__(self, shared, y):
        TargetQuadratic.__init__(self, shared, shared.q)
        self.y = np.ascontiguousarray(y, dtype=float)
        if self.y.shape != shared.y.shape:
            raise ValueError('labels size does not match with Q')
        self._flip = self.y * shared.y

    def function_jacobian(self, x):
        x = np.asarray(x, dtype=float)
        Qx = self._flip * self.device_problem().matvec(self._flip * x)
        return 0.5 * float(x @ Qx) + float(self.q @ x), Qx + self.q


def lagrangian_columns(ests, views, a, ub):
    """Per column the objective and the optimizer of `SVM._lagrangian` on its view of the shared panel, constructed in column order
    (a loop of single fits draws its start points in that order), and the batched solver's x0 (k x N) and multipliers (k x n_dual).
    a: one equality row per column, or None."""
    pairs = [est._lagrangian(view, None if a is None else a[c], ub) for c, (est, view) in enumerate(zip(ests, views))]
    x0 = np.stack([opt.x for _, opt in pairs])
    dual0 = np.stack([obj.dual_x for obj, _ in pairs])
    return pairs, x0, dual0


def fitted_lagrangian(est, obj, opt, r):
    """Make `est.obj` / `est.optimizer` / `est.train_loss_history` / `est.alphas_` what `SVM._run_lagrangian` leaves, from the
    column's objective and optimizer (`lagrangian_columns`) and its result `r` of `solve_batched_al`; warns as it does."""
    rows = r['rows']
    if len(rows):
        opt.iter = int(rows[-1]['iter'])
        opt.epoch = opt.iter + 1   # full batch: one epoch per evaluation
        opt.f_x, opt.primal_f_x = float(rows[-1]['f']), float(rows[-1]['r1'])
        opt.dgap = abs((opt.primal_f_x - opt.f_x) / max(abs(opt.primal_f_x), 1))
    opt.status = r['status']
    opt.x, opt.g_x, opt.step, opt.past_x = r['x'], r['g'], r['step'], r['past_x']
    obj.past_dual_x = obj.dual_x.copy()
    obj.dual_x = r['dual']
    est.train_loss_history = [float(f) for f in rows['r1']]   # the primal values, as `_store_train_info` keeps them
    est.obj, est.optimizer = obj, opt
    if opt.status == 'stopped':
        warnings.warn('max_iter reached but the optimization has not converged yet', ConvergenceWarning)
    est.alphas_ = opt.x


def svr_intercept(y, u, sv, epsilon):
    """SVR.fit's intercept of the regularised-intercept dual from u = K (alpha+ - alpha-) on the support vectors `sv`, statement
    for statement."""
    b = 0.
    b += float(np.sum(y[sv] - u[sv]))
    b -= epsilon
    b /= int(sv.sum())
    return b


class _MultiClassSVC(ClassifierMixin, BaseEstimator):
    """Constructor and prototype of the multi-class estimators: SVC's arguments, SVC's checks."""

    def __init__(self, loss=squared_hinge, kernel=gaussian, C=1, rho=1, mu=1, fit_intercept=True, intercept_scaling=1,
                 reg_intercept=False, dual=False, optimizer=ProjectedGradient, master_solver='clarabel', learning_rate='auto',
                 momentum_type='none', momentum=0.9, max_iter=1000, max_f_eval=15000, tol=1e-4, batch_size=None, shuffle=True,
                 random_state=None, early_stopping=False, validation_split=0., patience=5, verbose=False, master_verbose=False,
                 storage='f64', class_weight=None):
        self._kw = dict(loss=loss, kernel=kernel, C=C, rho=rho, mu=mu, fit_intercept=fit_intercept,
                        intercept_scaling=intercept_scaling, reg_intercept=reg_intercept, dual=dual, optimizer=optimizer,
                        master_solver=master_solver, learning_rate=learning_rate, momentum_type=momentum_type,
                        momentum=momentum, max_iter=max_iter, max_f_eval=max_f_eval, tol=tol, batch_size=batch_size,
                        shuffle=shuffle, random_state=random_state, early_stopping=early_stopping,
                        validation_split=validation_split, patience=patience, verbose=verbose,
                        master_verbose=master_verbose, storage=storage, class_weight=class_weight)
        SVC(**self._kw)   # SVC's checks, SVC's exceptions
        for name, value in self._kw.items():
            setattr(self, name, value)

    def _prototype(self):
        return SVC(**{name: getattr(self, name) for name in self._kw})   # set_params may have changed them


class _MultiTargetSVR(RegressorMixin, BaseEstimator):
    """Constructor and prototype of the multi-output regressor: SVR's arguments, SVR's checks."""

    def __init__(self, loss=squared_epsilon_insensitive, epsilon=0.1, kernel=gaussian, C=1, rho=1, mu=1, fit_intercept=True,
                 intercept_scaling=1, reg_intercept=False, dual=False, optimizer=ProjectedGradient, master_solver='clarabel',
                 learning_rate='auto', momentum_type='none', momentum=0.9, max_iter=1000, max_f_eval=15000, tol=1e-4,
                 batch_size=None, shuffle=True, random_state=None, early_stopping=False, validation_split=0., patience=5,
                 verbose=False, master_verbose=False, storage='f64'):
        self._kw = dict(loss=loss, epsilon=epsilon, kernel=kernel, C=C, rho=rho, mu=mu, fit_intercept=fit_intercept,
                        intercept_scaling=intercept_scaling, reg_intercept=reg_intercept, dual=dual, optimizer=optimizer,
                        master_solver=master_solver, learning_rate=learning_rate, momentum_type=momentum_type,
                        momentum=momentum, max_iter=max_iter, max_f_eval=max_f_eval, tol=tol, batch_size=batch_size,
                        shuffle=shuffle, random_state=random_state, early_stopping=early_stopping,
                        validation_split=validation_split, patience=patience, verbose=verbose,
                        master_verbose=master_verbose, storage=storage)
        SVR(**self._kw)   # SVR's checks, SVR's exceptions
        for name, value in self._kw.items():
            setattr(self, name, value)

    def _prototype(self):
        return SVR(**{name: getattr(self, name) for name in self._kw})   # set_params may have changed them
