"""One-vs-one multi-class SVC: the result of sklearn's `OneVsOneClassifier(SVC(**kw))`, with the k(k-1)/2 pair duals solved
together on ONE class-sorted Gram panel.

Sorted by class, stable within a class, and with every class padded by ghost rows to whole 256-row tiles, the panel's tiles are of
two kinds: an off-diagonal class block (rows of b, columns of a < b) serves only pair (a, b), and a class's diagonal block serves the
pairs that contain the class.  Pair (a, b) is one column of the batched solver with ub = C on the rows of a and b and 0 on every
other row, ghost rows included, which is exactly the pair's own dual (those entries start at 0 and never move); its labels are +1 on
b, the larger label, as `OneVsOneClassifier` hands `SVC.fit` 0 / 1 labels.  Every iteration takes the pair-routed product
(`bq_msolver_create_pairs`, bq_symmp.hip), which streams the panel once for all live pairs; the intercepts come from one routed
product (`bq_problem_gram_matmat_pairs`).  Each pair follows the iteration of `SVC.fit` on its rows with the same optimizer, and its
iterates have the same bits whatever the other pairs do.

The batched path needs `OneVsRestSVC`'s batched configuration (`uses_batched_path`) and a kernel whose parameters do not depend on
X: a numeric gamma, gamma='auto', or the linear kernel.  gamma='scale' is 1 / (d X.var()) of each pair's own rows, so one panel
cannot serve every pair; that configuration and every other one fit one `SVC` per pair on the pair's rows — exactly the calls of
`OneVsOneClassifier(SVC)`, with bit-identical results.
"""
import ctypes as C

import numpy as np

from ... import _lib
from ...device import get_context
from ...opti import KernelQuadratic
from ...opti.constrained import ProjectedGradient
from ._base import SVC, ClassifierMixin, BaseEstimator
from .kernels import LinearKernel, gaussian
from .losses import squared_hinge
from .multiclass import _DeviceMultiSolver, solve_batched, uses_batched_path

__all__ = ['OneVsOneSVC', 'uses_batched_ovo', 'sort_plan', 'ovo_pairs', 'pair_problem', 'ovo_decision']

TILE = 256
MEMORY_SHARE = 0.5   # share of the free device memory (after the panel) that one solve's columns and slab may take


def uses_batched_ovo(svc, world):
    """True when `OneVsOneSVC` solves the pairs of `svc`'s configuration together on one panel: `uses_batched_path` holds and the
    kernel's parameters do not depend on the rows (numeric gamma, gamma='auto' or a linear kernel)."""
    if not uses_batched_path(svc, world):
        return False
    return isinstance(svc.kernel, LinearKernel) or getattr(svc.kernel, 'gamma', None) != 'scale'


def ovo_pairs(ncls):
    """The class-index pairs (i, j), i < j, in `OneVsOneClassifier`'s order."""
    return [(i, j) for i in range(ncls) for j in range(i + 1, ncls)]


def sort_plan(codes, ncls):
    """The class-sorted, tile-padded row layout of the panel for class codes 0..ncls-1.

    Returns (index, cls_tiles, n_pad): row r of the data sits at panel row index[r]; class c holds panel rows [256 cls_tiles[c],
    256 cls_tiles[c + 1]), its rows in their original order first and ghost rows after them; n_pad = 256 cls_tiles[ncls]."""
    codes = np.asarray(codes)
    counts = np.bincount(codes, minlength=ncls)
    if len(counts) != ncls or (counts == 0).any():
        raise ValueError('every class must have at least one row')
    tiles = (counts + TILE - 1) // TILE
    cls_tiles = np.concatenate(([0], np.cumsum(tiles))).astype(np.int32)
    order = np.argsort(codes, kind='stable')
    starts = np.concatenate(([0], np.cumsum(counts)[:-1]))
    rank = np.empty(len(codes), dtype=np.int64)
    rank[order] = np.arange(len(codes)) - np.repeat(starts, counts)   # position within the class
    index = cls_tiles[codes].astype(np.int64) * TILE + rank
    return index, cls_tiles, int(cls_tiles[-1]) * TILE


def pair_problem(codes, i, j):
    """(rows, y): the rows OneVsOneClassifier fits pair (i, j) on, in their original order, and SVC.fit's labels for them
    (class j, the larger 0 / 1 label, is +1)."""
    codes = np.asarray(codes)
    rows = np.flatnonzero((codes == i) | (codes == j))
    return rows, np.where(codes[rows] == j, 1., -1.)


def ovo_decision(predictions, confidences, ncls):
    """sklearn's `_ovr_decision_function`: votes plus the confidences' sums mapped monotonically into (-1/3, 1/3)."""
    n = predictions.shape[0]
    votes = np.zeros((n, ncls))
    conf = np.zeros((n, ncls))
    k = 0
    for i in range(ncls):
        for j in range(i + 1, ncls):
            conf[:, i] -= confidences[:, k]
            conf[:, j] += confidences[:, k]
            votes[predictions[:, k] == 0, i] += 1
            votes[predictions[:, k] == 1, j] += 1
            k += 1
    return votes + conf / (3 * (np.abs(conf) + 1))


def _pair_array(pairs):
    return _lib.as_i32(np.asarray(pairs, dtype=np.int32).reshape(-1))


class _DevicePairSolver(_DeviceMultiSolver):
    """`bq_msolver_create_pairs`: one column per pair on a class-sorted panel."""

    def __init__(self, problem, kind, cls_tiles, pairs, Y, UB, eps, max_iter, t=0.0, x0=None):
        self._lib = _lib.load()
        self.k, self.n = Y.shape
        self._h = C.c_void_p()
        Y = _lib.as_f64(Y, self.k * self.n, 'Y')
        UB = _lib.as_f64(UB, self.k * self.n, 'UB')
        x0 = None if x0 is None else _lib.as_f64(x0, self.k * self.n, 'x0')
        ct, pr = _lib.as_i32(cls_tiles), _pair_array(pairs)
        _lib.check(self._lib.bq_msolver_create_pairs(problem.handle, kind, len(ct) - 1, _lib.iptr(ct), self.k, _lib.iptr(pr),
                                                     _lib.ptr(Y), _lib.ptr(UB), _lib.ptr(x0), float(eps), int(max_iter), float(t),
                                                     C.byref(self._h)))


def gram_matmat_pairs(problem, cls_tiles, pairs, W):
    """OUT[p] = K W[p] on the rows of pair p's classes and 0 elsewhere, one routed product (bq_problem_gram_matmat_pairs)."""
    W = np.ascontiguousarray(W, dtype=float)
    out = np.empty_like(W)
    ct, pr = _lib.as_i32(cls_tiles), _pair_array(pairs)
    _lib.check(_lib.load().bq_problem_gram_matmat_pairs(problem.handle, len(ct) - 1, _lib.iptr(ct), W.shape[0], _lib.iptr(pr),
                                                        _lib.ptr(W), _lib.ptr(out)))
    return out


def pairs_slab_bytes(cls_tiles, pairs):
    ct, pr = _lib.as_i32(cls_tiles), _pair_array(pairs)
    out = C.c_int64(0)
    _lib.check(_lib.load().bq_pairs_slab_bytes(int(ct[-1]), len(ct) - 1, _lib.iptr(ct), len(pairs), _lib.iptr(pr), C.byref(out)))
    return out.value


def pair_chunks(pairs, cls_tiles, n_pad, free_bytes):
    """The pairs split into solves that fit MEMORY_SHARE of `free_bytes`: per pair about 16 device n-vectors (the solver's x, g,
    d, Qd, bounds, labels, product input and output) plus its slab region.  The split does not change any pair's bits."""
    per = [16 * 8 * (n_pad + TILE) + pairs_slab_bytes(cls_tiles, [p]) for p in pairs]
    budget = int(free_bytes * MEMORY_SHARE)
    chunks, cur, used = [], [], 0
    for p, b in zip(pairs, per):
        if cur and used + b > budget:
            chunks.append(cur)
            cur, used = [], 0
        cur.append(p)
        used += b
    chunks.append(cur)
    return chunks


class OneVsOneSVC(ClassifierMixin, BaseEstimator):
    """One-vs-one multi-class SVC; constructor arguments and their checks are SVC's.

    After `fit`: `classes_`, `n_classes_`, `estimators_` (one fitted SVC per class pair (i, j), i < j, in OneVsOneClassifier's
    order, fitted on the rows of classes i and j with j as the positive class), `batched_` (which path ran), and
    `decision_function` (votes plus normalised confidences, m x k; 1-D with two classes), `predict`, `score` as sklearn's
    OneVsOneClassifier(SVC(**kw)).  gamma='scale' resolves on each pair's rows and runs one SVC per pair (see the module).
    """

    def __init__(self, loss=squared_hinge, kernel=gaussian, C=1, rho=1, mu=1, fit_intercept=True, intercept_scaling=1,
                 reg_intercept=False, dual=False, optimizer=ProjectedGradient, master_solver='clarabel', learning_rate='auto',
                 momentum_type='none', momentum=0.9, max_iter=1000, max_f_eval=15000, tol=1e-4, batch_size=None, shuffle=True,
                 random_state=None, early_stopping=False, validation_split=0., patience=5, verbose=False, master_verbose=False,
                 storage='f64'):
        self._kw = dict(loss=loss, kernel=kernel, C=C, rho=rho, mu=mu, fit_intercept=fit_intercept,
                        intercept_scaling=intercept_scaling, reg_intercept=reg_intercept, dual=dual, optimizer=optimizer,
                        master_solver=master_solver, learning_rate=learning_rate, momentum_type=momentum_type,
                        momentum=momentum, max_iter=max_iter, max_f_eval=max_f_eval, tol=tol, batch_size=batch_size,
                        shuffle=shuffle, random_state=random_state, early_stopping=early_stopping,
                        validation_split=validation_split, patience=patience, verbose=verbose,
                        master_verbose=master_verbose, storage=storage)
        SVC(**self._kw)   # SVC's checks, SVC's exceptions
        for name, value in self._kw.items():
            setattr(self, name, value)

    def _prototype(self):
        return SVC(**{name: getattr(self, name) for name in self._kw})   # set_params may have changed them

    @property
    def n_classes_(self):
        return len(self.classes_)

    def fit(self, X, y):
        X = np.ascontiguousarray(X, dtype=float)
        y = np.asarray(y)
        self.classes_ = np.unique(y)
        if len(self.classes_) == 1:
            raise ValueError('OneVsOneSVC can not be fit when only one class is present.')
        codes = np.searchsorted(self.classes_, y)
        proto = self._prototype()
        self.batched_ = uses_batched_ovo(proto, get_context().world)
        if not self.batched_:
            self.estimators_ = []
            for i, j in ovo_pairs(len(self.classes_)):
                rows, yp = pair_problem(codes, i, j)
                self.estimators_.append(self._prototype().fit(X[rows], (yp > 0).astype(int)))
            return self
        self.estimators_ = self._fit_batched(proto, X, codes)
        return self

    def _fit_batched(self, proto, X, codes):
        ncls = len(self.classes_)
        pairs = ovo_pairs(ncls)
        index, cls_tiles, n_pad = sort_plan(codes, ncls)
        Xp = np.zeros((n_pad, X.shape[1]))
        Xp[index] = X
        ghost = np.ones(n_pad, dtype=bool)
        ghost[index] = False
        pcode = np.repeat(np.arange(ncls), np.diff(cls_tiles) * TILE)   # class of every panel row, ghost rows included
        obj = KernelQuadratic(Xp, -np.ones(n_pad), 'svc', proto.kernel, y=np.ones(n_pad), storage=proto.storage,
                              tune_placement=proto._streams_panel(), expected_products=proto.max_iter)
        dev = obj.device_problem()
        kind = _lib.PG if issubclass(proto.optimizer, ProjectedGradient) else _lib.FW
        free, total = C.c_int64(0), C.c_int64(0)
        _lib.check(_lib.load().bq_ctx_mem_info(get_context().handle, C.byref(free), C.byref(total)))
        ests = []
        for chunk in pair_chunks(pairs, cls_tiles, n_pad, free.value):
            Y = np.stack([np.where(pcode == j, 1., -1.) for _, j in chunk])
            UB = np.stack([np.where(((pcode == i) | (pcode == j)) & ~ghost, float(proto.C), 0.) for i, j in chunk])
            solver = _DevicePairSolver(dev, kind, cls_tiles, chunk, Y, UB, 1e-6, proto.max_iter)
            res = solve_batched(dev, kind, Y, UB, max_iter=proto.max_iter, solver=solver)
            W = np.zeros((len(chunk), n_pad))
            fits = []
            for p, (i, j) in enumerate(chunk):
                rows, yp = pair_problem(codes, i, j)
                pos = index[rows]
                est, sv = self._estimator(proto, obj, res[p], X[rows], yp, pos)
                W[p][pos[sv]] = est.dual_coef_
                fits.append((est, yp, pos, sv))
            U = gram_matmat_pairs(dev, cls_tiles, chunk, W)
            for p, (est, yp, pos, sv) in enumerate(fits):
                est.intercept_ = 0.
                est.intercept_ += float(np.sum(yp[sv] - U[p][pos][sv]))
                est.intercept_ /= int(sv.sum())
                ests.append(est)
        del dev, obj
        return ests

    def _estimator(self, proto, obj, r, Xpair, yp, pos):
        """The SVC that SVC.fit on the pair's rows leaves, from the pair's column (its panel rows `pos`, in the rows' order)."""
        est = self._prototype()
        ub = np.ones(len(pos)) * proto.C
        # the optimizer as SVC.fit leaves it (constrained/_base.py: minimize) — constructed, not run
        opt = proto.optimizer(quad=obj, ub=ub, tol=proto.tol, max_iter=proto.max_iter, verbose=proto.verbose)
        if len(r['rows']):
            opt.iter = int(r['rows'][-1]['iter'])
            opt._after_row(r['rows'][-1])
        opt.status, opt.f_x, opt.x, opt.g_x = r['status'], r['f_x'], r['x'][pos], r['g'][pos]
        est.train_loss_history = [float(f) for f in r['rows']['f']]
        est.optimizer = opt
        est.classes_ = np.array([0, 1])   # OneVsOneClassifier fits each SVC on 0 / 1 labels
        est.alphas_ = opt.x
        sv = est.alphas_ > 1e-6
        est.support_ = np.arange(len(pos))[sv]
        est.support_vectors_ = Xpair[sv]
        est.dual_coef_ = est.alphas_[sv] * yp[sv]
        if isinstance(est.kernel, LinearKernel):
            est.coef_ = np.dot(est.dual_coef_, est.support_vectors_)
        return est, sv

    def decision_function(self, X):
        X = np.ascontiguousarray(X, dtype=float)
        conf = np.stack([np.ravel(e.decision_function(X)) for e in self.estimators_], axis=1)
        Y = ovo_decision((conf > 0).astype(int), conf, len(self.classes_))
        return Y[:, 1] if len(self.classes_) == 2 else Y

    def predict(self, X):
        Y = self.decision_function(X)
        if len(self.classes_) == 2:
            return self.classes_[(Y > 0).astype(int)]
        return self.classes_[Y.argmax(axis=1)]
