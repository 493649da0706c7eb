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

SMO (`optimizer='smo'`, `uses_batched_ovo_smo`) has a batched form of its own: every pair is one walker column of the batched SMO
solver (`bq_msmo_*`) on ONE panel of all n rows that is NOT class-sorted and has no ghost rows.  SMO is a sequential sweep, so its
result depends on the row order, and `OneVsOneClassifier` hands `SVC.fit` a pair's rows in their original order: pair (i, j) is the
column whose ascending row list is `pair_problem(codes, i, j)[0]`, the sweep order of the per-pair fit, with +1 on class j.  A
column follows that fit step for step on the shared panel's own entries (tests/test_gpu_ovo_smo.py holds it to the oracle).  Whether
it also has the per-pair fit's bits hangs on one fact: is the Gram matrix `KernelQuadratic(X[rows], ...)` builds for a pair equal,
bit for bit, to the shared panel's entries `K[rows][:, rows]`?  Measured on an MI355X: at n = 240 (4 classes, RBF), where the shared
panel is one 256-row tile row, it IS bit-equal for every pair, and every pair estimator equals the per-pair `SVC.fit` field for field
(tests/test_gpu_ovo_smo.py::test_pair_estimators_equal_the_per_pair_fits_field_for_field).  It is NOT in general: at n = 360 (5
classes, two tile rows) no pair's own build is bit-equal, and at n = 20 000 (10 classes, 45 pairs of about 4 000 rows) the two fits'
multipliers differ and the pairs take 11 to 19 outer iterations as columns against 11 to 18 per pair — other walks through the same
tol-optimal sets, with every training row predicted alike (profiles/ovo_smo/).  So `batch_smo` chooses between two fits that agree
as two SMO runs to `tol` agree, not bit for bit; the default, None, takes the columns from four pairs on because they are faster
(0.153 s against 1.999 s at that size), and two or three classes stay one `SVC.fit` per pair.
"""
import ctypes as C

import numpy as np

from ... import _lib
from ...device import get_context
from ...opti import KernelQuadratic
from ._batched import (MEMORY_SHARE, DecisionBatch, _DeviceMultiSolver, _MultiClassSVC, _pair_array, column_bytes,
                       device_free_bytes, fitted_smo_svc, fitted_svc, gram_matmat_pairs, intercept, solve_batched,
                       solve_batched_smo, solver_kind, takes_batched_smo, uses_batched_decision)
from ._base import has_class_weight, row_boxes
from .kernels import LinearKernel
from .multiclass import uses_batched_path, uses_batched_smo_path

__all__ = ['OneVsOneSVC', 'uses_batched_ovo', 'uses_batched_ovo_smo', 'sort_plan', 'ovo_pairs', 'pair_problem', 'ovo_decision']

TILE = 256


def uses_batched_ovo(svc, world):
    """True when `OneVsOneSVC` solves the pairs of `svc`'s configuration together on one panel: `uses_batched_path` holds and the
    kernel's parameters do not depend on the rows (numeric gamma, gamma='auto' or a linear kernel)."""
    if not uses_batched_path(svc, world):
        return False
    return isinstance(svc.kernel, LinearKernel) or getattr(svc.kernel, 'gamma', None) != 'scale'


def uses_batched_ovo_smo(svc, world):
    """True when `OneVsOneSVC` can solve the pairs of `svc`'s configuration as row-list columns of the batched SMO solver on one
    unsorted panel: `uses_batched_smo_path` holds and the kernel's parameters do not depend on the rows (numeric gamma,
    gamma='auto' or a linear kernel).  Whether a fit then does is `takes_batched_smo`'s answer (`OneVsOneSVC.batch_smo`).  A
    `class_weight` stays on this path: every pair's column gets the boxes of the pair's own fit."""
    if not uses_batched_smo_path(svc, world):
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


class _DevicePairSolver(_DeviceMultiSolver):
    """`bq_msolver_create_pairs`: one column per pair on a class-sorted panel."""

    def __init__(self, problem, kind, cls_tiles, pairs, Y, UB, eps, max_iter, t=0.0, x0=None):
        self._ct, self._pr = _lib.as_i32(cls_tiles), _pair_array(pairs)
        super().__init__(problem, kind, Y, UB, eps, max_iter, t, x0)

    def _create(self, handle, kind, Y, UB, x0, eps, max_iter, t):
        UB = _lib.as_f64(UB, self.k * self.n, 'UB')
        x0 = self._x0(x0)
        return self._lib.bq_msolver_create_pairs(handle, kind, len(self._ct) - 1, _lib.iptr(self._ct), self.k, _lib.iptr(self._pr),
                                                 _lib.ptr(Y), _lib.ptr(UB), _lib.ptr(x0), eps, max_iter, t, C.byref(self._h))


def pairs_slab_bytes(cls_tiles, pairs):
    ct, pr = _lib.as_i32(cls_tiles), _pair_array(pairs)
    out = C.c_int64(0)
    _lib.check(_lib.load().bq_pairs_slab_bytes(int(ct[-1]), len(ct) - 1, _lib.iptr(ct), len(pairs), _lib.iptr(pr), C.byref(out)))
    return out.value


def pair_chunks(pairs, cls_tiles, n_pad, free_bytes):
    """The pairs split into solves that fit MEMORY_SHARE of `free_bytes`: per pair about 16 device n-vectors (the solver's x, g,
    d, Qd, bounds, labels, product input and output) plus its slab region.  The split does not change any pair's bits."""
    per = [column_bytes(n_pad) + pairs_slab_bytes(cls_tiles, [p]) for p in pairs]
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


class OneVsOneSVC(_MultiClassSVC):
    """One-vs-one multi-class SVC; constructor arguments and their checks are SVC's.

    After `fit`: `classes_`, `n_classes_`, `estimators_` (one fitted SVC per class pair (i, j), i < j, in OneVsOneClassifier's
    order, fitted on the rows of classes i and j with j as the positive class), `batched_` (which path ran), and
    `decision_function` (votes plus normalised confidences, m x k; 1-D with two classes), `predict`, `score` as sklearn's
    OneVsOneClassifier(SVC(**kw)).  gamma='scale' resolves on each pair's rows and runs one SVC per pair (see the module).

    `batched_decision_`: True when `decision_function` and `predict` take every pair's confidences from one fused pass over the
    kernel values of the union of the support vectors (`uses_batched_decision`; a training row is in up to k - 1 pairs and in the
    union once) instead of one call per estimator.  The stored batch (`decision_batch_`) describes the estimators as `fit` left
    them.

    `smo_`: the pairs were solved together as row-list columns of the batched SMO solver (`uses_batched_ovo_smo`); `batched_` is
    True when either batched path ran.  `batch_smo` (None, True, False) forces that choice where the configuration allows it; None
    leaves it to the number of pairs (`takes_batched_smo`: two and three classes stay one `SVC.fit` per pair).
    """
    batch_smo = None

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
        if isinstance(proto.class_weight, dict):
            for label in proto.class_weight:
                if not (self.classes_ == label).any():
                    raise ValueError('class_weight names the label %r, which is not among the classes %r' % (label, list(self.classes_)))
        ncls = len(self.classes_)
        P = ncls * (ncls - 1) // 2
        self.smo_ = uses_batched_ovo_smo(proto, get_context().world) and takes_batched_smo(P, self.batch_smo)
        self.batched_ = self.smo_ or uses_batched_ovo(proto, get_context().world)
        self.batched_decision_ = uses_batched_decision(proto.kernel, P, get_context().world, self.batched_)
        self.decision_batch_ = None
        if not self.batched_:
            self.estimators_ = []
            for i, j in ovo_pairs(len(self.classes_)):
                rows, yp = pair_problem(codes, i, j)
                self.estimators_.append(self._pair_prototype(i, j).fit(X[rows], (yp > 0).astype(int)))
            return self
        self.estimators_ = (self._fit_smo if self.smo_ else self._fit_batched)(proto, X, codes)
        return self

    def _pair_prototype(self, i, j):
        """The SVC of pair (i, j), fitted on the labels 0 (class i) / 1 (class j): a `class_weight` dict, whose keys are the data's
        labels, is handed over as the two weights under those labels; 'balanced' resolves on the pair's rows in `SVC.fit`."""
        est = self._prototype()
        if isinstance(est.class_weight, dict):
            est.class_weight = {0: est.class_weight.get(self.classes_[i], 1.), 1: est.class_weight.get(self.classes_[j], 1.)}
        return est

    def _fit_smo(self, proto, X, codes):
        """SVC.fit's SMO branch for every pair on one panel of all rows, built as `OneVsRestSVC._fit_smo` builds it (rank_one=False,
        compact=False; unsorted, no ghost rows): pair (i, j) is the column with the pair's rows as its ascending row list and +1 on
        class j; the intercepts are the solver's."""
        n = len(codes)
        pairs = ovo_pairs(len(self.classes_))
        problems = [pair_problem(codes, i, j) for i, j in pairs]
        Y = np.stack([np.where(codes == j, 1., -1.) for _, j in pairs])
        obj = KernelQuadratic(X, -np.ones(n), 'svc', proto.kernel, y=Y[0], storage=proto.storage, rank_one=False, compact=False)
        dev = obj.device_problem()
        # (in solves of `smo_column_cap` columns of the memory free after the panel)
        # class_weight: column p's boxes on its rows are those the pair's own SVC.fit computes from its 0 / 1 labels
        boxes = None
        if has_class_weight(proto):
            boxes = np.zeros((len(pairs), n))
            for p, ((i, j), (rows, yp)) in enumerate(zip(pairs, problems)):
                boxes[p, rows] = row_boxes(proto.C, (yp > 0).astype(int), np.arange(2), self._pair_prototype(i, j).class_weight)
        res = solve_batched_smo(dev, _lib.SVC, Y, proto.C, None, proto.tol, rows=[rows for rows, _ in problems], boxes=boxes)
        ests, coefs = [], []
        for p, (rows, yp) in enumerate(problems):
            r = dict(res[p])
            # the column's n-long state on the pair's rows; the threshold rows as positions among them
            r['alphas'], r['errors'] = r['alphas'][rows], r['errors'][rows]
            r['b_up_idx'], r['b_low_idx'] = (int(np.searchsorted(rows, r[name])) for name in ('b_up_idx', 'b_low_idx'))
            est = self._pair_prototype(*pairs[p])
            sv = fitted_smo_svc(est, obj, r, X[rows], yp, None if boxes is None else boxes[p, rows])
            w = np.zeros(n)
            w[rows[sv]] = est.dual_coef_
            coefs.append(w)
            ests.append(est)
            if self.verbose:
                print('pair (%r, %r): %d outer iterations, %d pair steps' % (self.classes_[pairs[p][0]], self.classes_[pairs[p][1]],
                                                                           est.optimizer.iter, est.optimizer.steps))
        if self.batched_decision_:
            self.decision_batch_ = DecisionBatch(proto.kernel, X, coefs, [est.intercept_ for est in ests])
        return ests

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
        kind = solver_kind(proto.optimizer)
        ests, coefs = [], []
        for chunk in pair_chunks(pairs, cls_tiles, n_pad, device_free_bytes()):
            Y = np.stack([np.where(pcode == j, 1., -1.) for _, j in chunk])
            UB = np.stack([np.where(((pcode == i) | (pcode == j)) & ~ghost, float(proto.C), 0.) for i, j in chunk])
            solver = _DevicePairSolver(dev, kind, cls_tiles, chunk, Y, UB, 1e-6, proto.max_iter)
            res = solve_batched(dev, kind, Y, UB, max_iter=proto.max_iter, solver=solver)
            W = np.zeros((len(chunk), n_pad))
            fits = []
            for p, (i, j) in enumerate(chunk):
                rows, yp = pair_problem(codes, i, j)
                pos = index[rows]
                est = self._prototype()
                sv = fitted_svc(est, obj, res[p], X[rows], yp, pos)
                W[p][pos[sv]] = est.dual_coef_
                fits.append((est, yp, pos, sv))
            U = gram_matmat_pairs(dev, cls_tiles, chunk, W)
            for p, (est, yp, pos, sv) in enumerate(fits):
                est.intercept_ = intercept(yp, U[p][pos], sv)
                ests.append(est)
            if self.batched_decision_:
                coefs.append(W)
        del dev, obj
        if self.batched_decision_:
            self.decision_batch_ = DecisionBatch(proto.kernel, Xp, np.vstack(coefs), [est.intercept_ for est in ests],
                                                 keep=~ghost)
        return ests

    def decision_function(self, X):
        X = np.ascontiguousarray(X, dtype=float)
        if self.batched_decision_:
            conf = self.decision_batch_(X)
        else:
            conf = np.stack([np.ravel(e.decision_function(X)) for e in self.estimators_], axis=1)
        Y = ovo_decision((conf > 0).astype(int), conf, len(self.classes_))
        return Y[:, 1] if len(self.classes_) == 2 else Y

    def predict(self, X):
        Y = self.decision_function(X)
        if len(self.classes_) == 2:
            return self.classes_[(Y > 0).astype(int)]
        return self.classes_[Y.argmax(axis=1)]
