"""One-vs-one multi-class nu-SVC: the result of sklearn's `OneVsOneClassifier(NuSVC(**kw))`, with the k(k-1)/2 pair duals solved
together on ONE class-sorted Gram panel.

The panel is `OneVsOneSVC`'s (`sort_plan`: sorted by class, stable within a class, every class padded by ghost rows to whole
256-row tiles).  Pair (i, j), i < j, is one column of the two-group simplex solver (`bq_msolver_create_simplex2_pairs`,
csrc/bq_simplex.hip's BLOCKS layout): group 0 is class j's row range with sign +1, as `OneVsOneClassifier` hands `NuSVC.fit` 0 / 1
labels with the larger class positive, group 1 class i's with sign -1; the box is 1 on the pair's data rows and 0 on its ghost
rows, and each group's mass is nu (n_i + n_j) / 2.  Every iteration takes the pair-routed product (bq_symmp.hip), which streams
the panel at most once for all live columns, and a column's own kernels walk its two classes' rows only.  Each pair follows the
iteration of `NuSVC.fit` on its rows, and its iterates have the same bits whatever the other columns do.

Several nu on the same data (`ovo_nu_svc_path`) are more columns of the same solve: column (nu, pair), the same pair once per nu.

The batched path needs a kernel whose parameters do not depend on the rows: a numeric gamma, gamma='auto', or the linear kernel.
gamma='scale' is 1 / (d X.var()) of each pair's own rows, so one panel cannot serve every pair; that configuration fits one
`NuSVC` per pair on the pair's rows — exactly the calls of `OneVsOneClassifier(NuSVC)`, with bit-identical results.
"""
import numpy as np

from ...device import get_context
from ...opti import KernelQuadratic
from ._base import ClassifierMixin, has_class_weight
from ._batched import (MEMORY_SHARE, DecisionBatch, _DeviceSimplexPairSolver, device_free_bytes, solve_batched,
                       uses_batched_decision)
from .kernels import BaseEstimator, LinearKernel, gaussian
from .nu import NuSVC, _check, _clones
from .oneclass import _resolved
from .onevsone import TILE, ovo_decision, ovo_pairs, pair_problem, pairs_slab_bytes, sort_plan

__all__ = ['OneVsOneNuSVC', 'ovo_nu_svc_path', 'uses_batched_ovo_nu', 'ovo_nu_columns', 'ovo_nu_boxes']


def uses_batched_ovo_nu(est, world):
    """True when `OneVsOneNuSVC` solves the pairs of `est`'s configuration together on one panel: a resident panel on a single-rank
    context (anything else is refused by `fit`) and a kernel whose parameters do not depend on the rows (numeric gamma,
    gamma='auto' or a linear kernel)."""
    if has_class_weight(est) or est.storage not in ('f64', 'f32') or int(world) != 1:
        return False
    return isinstance(est.kernel, LinearKernel) or getattr(est.kernel, 'gamma', None) != 'scale'


def _check_pairs_feasible(codes, ncls, nus):
    """libsvm's check of nu-SVC (svm_check_parameter) on every pair's rows: each class must be able to hold the mass
    nu (n_i + n_j) / 2."""
    counts = np.bincount(codes, minlength=ncls)
    for nu in nus:
        for i, j in ovo_pairs(ncls):
            if nu * int(counts[i] + counts[j]) / 2 > min(int(counts[i]), int(counts[j])):
                raise ValueError('specified nu is infeasible')


def ovo_nu_columns(codes, ncls, nus):
    """The columns of one solve over every nu of `nus` and every class pair, in (nu, pair) order with the pairs in
    `OneVsOneClassifier`'s order: a list of (index of nu, (i, j), each group's mass nu (n_i + n_j) / 2)."""
    counts = np.bincount(codes, minlength=ncls)
    return [(t, (i, j), float(nu) * int(counts[i] + counts[j]) / 2) for t, nu in enumerate(nus) for i, j in ovo_pairs(ncls)]


def ovo_nu_boxes(cols, pcode, ghost):
    """UB (k x n_pad: 1 on the data rows of the column's two classes, 0 on their ghost rows and on every other row) and mass (k x 2)
    of the columns `cols` (`ovo_nu_columns`) on a panel whose row r has class pcode[r] and is a ghost row where ghost[r]."""
    UB = np.stack([np.where(((pcode == i) | (pcode == j)) & ~ghost, 1., 0.) for _, (i, j), _ in cols])
    mass = np.array([[ms, ms] for _, _, ms in cols], dtype=float)
    return UB, mass


def column_chunks(cols, cls_tiles, n_pad, free_bytes):
    """The columns split into solves that fit MEMORY_SHARE of `free_bytes`: per column the six device n-vectors of this flavour (the
    column's x, g, d, box, its product input and output, each padded by a tile) plus its pair's slab region.  The split does not
    change any column's bits."""
    slab = {}
    budget = int(free_bytes * MEMORY_SHARE)
    chunks, cur, used = [], [], 0
    for col in cols:
        pair = col[1]
        if pair not in slab:
            slab[pair] = pairs_slab_bytes(cls_tiles, [pair])
        b = 6 * 8 * (n_pad + TILE) + slab[pair]
        if cur and used + b > budget:
            chunks.append(cur)
            cur, used = [], 0
        cur.append(col)
        used += b
    chunks.append(cur)
    return chunks


def _solve_columns(proto, X, codes, ncls, nus):
    """Every (nu, pair) column on one class-sorted panel of X: (kernel_, Xp, ghost, index, [(column, result, r1, r2), ...]), the
    results in `ovo_nu_columns`'s order with x and g in panel order."""
    cols = ovo_nu_columns(codes, ncls, nus)
    index, cls_tiles, n_pad = sort_plan(codes, ncls)
    Xp = np.zeros((n_pad, X.shape[1]))
    Xp[index] = X
    ghost = np.ones(n_pad, dtype=bool)
    ghost[index] = False
    pcode = np.repeat(np.arange(ncls), np.diff(cls_tiles) * TILE)   # class of every panel row, ghost rows included
    kernel = _resolved(proto.kernel, X)   # ('auto': 1 / d, the same on any rows)
    obj = KernelQuadratic(Xp, np.zeros(n_pad), 'plain', kernel, storage=proto.storage, tune_placement=bool(proto.tune_placement),
                          expected_products=proto.max_iter)
    try:
        dev = obj.device_problem()
        out = []
        for chunk in column_chunks(cols, cls_tiles, n_pad, device_free_bytes()):
            UB, mass = ovo_nu_boxes(chunk, pcode, ghost)
            held = {}

            def offsets(solver, _):
                held['r1'], held['r2'], _, _ = solver.offsets()

            solver = _DeviceSimplexPairSolver(dev, cls_tiles, [pair for _, pair, _ in chunk], UB, mass, proto.tol, proto.max_iter)
            res = solve_batched(dev, None, UB, None, solver=solver, before_close=offsets)
            out.extend((col, r, float(held['r1'][c]), float(held['r2'][c])) for c, (col, r) in enumerate(zip(chunk, res)))
        return kernel, Xp, ghost, index, out
    finally:
        obj.release()


class OneVsOneNuSVC(ClassifierMixin, BaseEstimator):
    """One-vs-one multi-class nu-SVC; constructor arguments and their checks are `NuSVC`'s.

    After `fit`: `classes_`, `n_classes_`, `estimators_` (one fitted `NuSVC` per class pair (i, j), i < j, in
    OneVsOneClassifier's order, fitted on the rows of classes i and j in their original order with j as the positive class),
    `batched_` (which path ran), and `decision_function` (votes plus normalised confidences, m x k; 1-D with two classes),
    `predict`, `score` as sklearn's OneVsOneClassifier(NuSVC(**kw)).  libsvm's feasibility check runs on every pair before any
    device work: nu (n_i + n_j) / 2 above the smaller class of a pair raises ValueError('specified nu is infeasible').
    storage='stream' and multi-rank contexts raise NotImplementedError, as `NuSVC` does; gamma='scale' resolves on each pair's
    rows and runs one `NuSVC` per pair (see the module).

    `batched_decision_`: True when `decision_function` and `predict` take every pair's confidences from one fused pass over the
    kernel values of the union of the support vectors (`uses_batched_decision`) instead of one call per estimator.  The stored
    batch (`decision_batch_`) describes the estimators as `fit` left them."""

    tune_placement = True   # as NuSVC.tune_placement

    def __init__(self, kernel=gaussian, nu=0.5, tol=1e-3, max_iter=1000, storage='f64'):
        _check(kernel, nu, tol, max_iter, storage)
        self.kernel = kernel
        self.nu = nu
        self.tol = tol
        self.max_iter = max_iter
        self.storage = storage

    @property
    def n_classes_(self):
        return len(self.classes_)

    def _binary(self, nu=None):
        return NuSVC(kernel=self.kernel, nu=self.nu if nu is None else nu, tol=self.tol, max_iter=self.max_iter,
                     storage=self.storage)

    def _codes(self, y, nus):
        """classes_ and the class codes of y; the one-class, feasibility, storage and context refusals, before any device work"""
        y = np.asarray(y)
        self.classes_ = np.unique(y)
        if len(self.classes_) == 1:
            raise ValueError('OneVsOneNuSVC can not be fit when only one class is present.')
        codes = np.searchsorted(self.classes_, y)
        _check_pairs_feasible(codes, len(self.classes_), nus)
        if self.storage == 'stream':
            raise NotImplementedError('OneVsOneNuSVC needs a resident panel: storage \'f64\' or \'f32\'')
        if get_context().world != 1:
            raise NotImplementedError('OneVsOneNuSVC runs on a single-rank context')
        return codes

    def _fitted(self, X, codes, kernel, Xp, ghost, index, results):
        """`estimators_` and the decision batch from the pairs' columns (`_solve_columns`'s results of this estimator's nu)"""
        ncls = len(self.classes_)
        self.batched_ = True
        self.batched_decision_ = uses_batched_decision(self.kernel, len(results), get_context().world, True)
        self.decision_batch_ = None
        self.estimators_ = []
        coefs = np.zeros((len(results), Xp.shape[0])) if self.batched_decision_ else None
        for p, ((_, (i, j), _), r, r1, r2) in enumerate(results):
            rows, yp = pair_problem(codes, i, j)
            pos = index[rows]
            est = self._binary()
            est.classes_ = np.array([0, 1])   # OneVsOneClassifier fits each NuSVC on 0 / 1 labels
            est._fitted(X[rows], yp, kernel, dict(r, x=r['x'][pos], g=r['g'][pos]), r1, r2)
            if coefs is not None:
                coefs[p][pos[est.support_]] = est.dual_coef_
            self.estimators_.append(est)
        assert len(self.estimators_) == ncls * (ncls - 1) // 2
        if coefs is not None:
            self.decision_batch_ = DecisionBatch(kernel, Xp, coefs, [est.intercept_ for est in self.estimators_], keep=~ghost)
        return self

    def fit(self, X, y):
        _check(self.kernel, self.nu, self.tol, self.max_iter, self.storage)   # set_params may have changed them
        X = np.ascontiguousarray(X, dtype=float)
        codes = self._codes(y, [self.nu])
        if not uses_batched_ovo_nu(self, get_context().world):
            self.batched_ = self.batched_decision_ = False
            self.decision_batch_ = None
            self.estimators_ = []
            for i, j in ovo_pairs(len(self.classes_)):
                rows, yp = pair_problem(codes, i, j)
                self.estimators_.append(self._binary().fit(X[rows], (yp > 0).astype(int)))
            return self
        kernel, Xp, ghost, index, results = _solve_columns(self, X, codes, len(self.classes_), [self.nu])
        return self._fitted(X, codes, kernel, Xp, ghost, index, results)

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


def ovo_nu_svc_path(estimator, X, y, nus):
    """A list of fitted clones of the `OneVsOneNuSVC` `estimator`, one per nu of `nus`, every (nu, pair) a column of one batched
    solve on one class-sorted Gram panel of X (in several solves where the device memory does not hold all columns at once).  Each
    clone equals its own `OneVsOneNuSVC(nu=nu, ...).fit(X, y)` bit for bit; a configuration whose `fit` runs one `NuSVC` per pair
    (gamma='scale') is fitted clone by clone."""
    nus = [float(nu) for nu in nus]
    ests = _clones(estimator, [dict(nu=nu) for nu in nus])
    X = np.ascontiguousarray(X, dtype=float)
    if not ests:
        return ests
    for est in ests:
        _check(est.kernel, est.nu, est.tol, est.max_iter, est.storage)
    codes = ests[0]._codes(y, nus)
    if not uses_batched_ovo_nu(estimator, get_context().world):
        return [est.fit(X, y) for est in ests]
    ncls = len(ests[0].classes_)
    kernel, Xp, ghost, index, results = _solve_columns(estimator, X, codes, ncls, nus)
    npairs = ncls * (ncls - 1) // 2
    for t, est in enumerate(ests):
        est.classes_ = ests[0].classes_.copy()
        est._fitted(X, codes, kernel, Xp, ghost, index, results[t * npairs:(t + 1) * npairs])
    return ests
