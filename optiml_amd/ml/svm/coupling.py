"""Multi-class probabilities of `OneVsOneSVC` by pairwise coupling: the model of `sklearn.svm.SVC(probability=True)`, that is
libsvm's — one Platt sigmoid per class pair, fitted on cross-validated decision values, and at prediction the pairwise
probabilities coupled by Wu, Lin & Weng's second method (`multiclass_probability` in libsvm's svm.cpp) — with every (pair, fold)
fit solved on ONE class-sorted Gram panel.

`OneVsOneSVC`'s panel carries over (onevsone.py: rows sorted by class, every class padded by ghost rows to whole tiles, one column
per pair with ub = C on the data rows of its two classes), and so does the searches' observation that a training fold's dual is the
full dual with ub = 0 on the held-out rows: column (pair, fold) has ub = C on the pair's data rows in the fold's training part and 0
everywhere else, column (pair, all) is `OneVsOneSVC`'s own.  With k classes and F folds the k (k - 1) / 2 * (F + 1) columns run on
the pair-routed solver (`bq_msolver_create_pairs`), which reads an off-diagonal class block once per column that uses it.  The columns
are scored where the solver's state lives (`bq_msolver_pairs_heldout`): per column an intercept and a support count, the held-out
decision values into one buffer row per pair, and on those rows the sigmoid fits (`platt_fit_kernel`).  At prediction the fused
decision pass and the coupling kernel (bq_couple.hip, one wavefront per test point) run back to back on the device
(`bq_decision_coupled`).

The batched path applies when `OneVsOneSVC`'s does (`uses_batched_ovo`), the panel is 'f64' and the kernel's gamma is not a string.
Every other configuration runs the loop: per pair and fold `SVC.fit` on the pair's training rows and `decision_function` on its
held-out rows, the sigmoids through the same kernel (`bq_platt_fit`), and the coupling through `bq_pairwise_coupling`.

Signs.  A pair's decision value f is positive towards its LARGER label b, and its sigmoid is P(b | a or b) = 1 / (1 + exp(A f + B)).
libsvm's decision value of the pair is -f (its positive class is the smaller label) and its sigmoid gives P(a | a or b), so `probA_`
is libsvm's probA_ and `probB_` is the negative of libsvm's probB_.
"""
import warnings

import numpy as np

from ... import _lib
from ...device import get_context
from ...opti import KernelQuadratic
from ._base import ClassifierMixin, ConvergenceWarning, has_class_weight
from ._batched import DecisionBatch, device_free_bytes, fitted_svc, platt_fit, solve_batched, solver_kind, uses_batched_decision
from .kernels import BaseEstimator
from .model_selection import _base_params, _make, check_cv_splits
from .onevsone import TILE, OneVsOneSVC, _DevicePairSolver, ovo_pairs, pair_chunks, pair_problem, sort_plan, uses_batched_ovo

__all__ = ['PairwiseCoupledSVC', 'pairwise_coupling', 'coupled_decision', 'uses_batched_coupling', 'coupling_columns', 'MAX_CLASSES']

MAX_CLASSES = 64   # one wavefront lane per class (bq_couple.hip)


def uses_batched_coupling(estimator, world):
    """True when `PairwiseCoupledSVC` solves every (pair, fold) on one panel and calibrates on the device: the estimator is an
    `OneVsOneSVC` on its batched path (`uses_batched_ovo`), its panel is 'f64' and its kernel's gamma is not a string — the fp64
    panel of a numeric gamma holds the decision kernel's values."""
    if not isinstance(estimator, OneVsOneSVC):
        return False
    proto = estimator._prototype()
    return bool(not has_class_weight(proto) and uses_batched_ovo(proto, world) and proto.storage == 'f64' and
                not isinstance(getattr(proto.kernel, 'gamma', None), str))


def pairwise_coupling(F, A, B, ncls):
    """(prob, iters, R) of t test points from their pair decision values F (t x P, `ovo_pairs` order, positive towards the larger
    label) and the pairs' sigmoids A, B (`bq_pairwise_coupling`): prob t x ncls, iters the sweeps each point took, R the clipped
    pair probabilities the sweeps started from."""
    ncls = int(ncls)
    if not 2 <= ncls <= MAX_CLASSES:
        raise ValueError('pairwise coupling takes 2 to %d classes' % MAX_CLASSES)
    P = ncls * (ncls - 1) // 2
    F = np.ascontiguousarray(F, dtype=float)
    if F.ndim == 1 and P == 1:
        F = F.reshape(-1, 1)
    if F.ndim != 2 or F.shape[1] != P:
        raise ValueError('F must be t x %d (one column per pair of %d classes), got shape %s' % (P, ncls, F.shape))
    t = len(F)
    A, B = _lib.as_f64(A, P, 'A'), _lib.as_f64(B, P, 'B')
    prob, iters, R = np.empty((t, ncls)), np.empty(t, dtype=np.int32), np.empty((t, P))
    if t == 0:
        return prob, iters, R
    _lib.check(_lib.load().bq_pairwise_coupling(get_context().handle, ncls, t, _lib.ptr(F), _lib.ptr(A), _lib.ptr(B),
                                                _lib.ptr(prob), _lib.iptr(iters), _lib.ptr(R)))
    return prob, iters, R


def coupled_decision(batch, X, A, B, ncls, details=False):
    """The class probabilities (t x ncls) of the pair estimators of a `DecisionBatch` under the sigmoids A, B, in one device call
    (`bq_decision_coupled`: the fused decision pass, then the coupling of each chunk of test points where its decision values lie).
    details: (prob, iters, R, dec) instead, dec being the t x pairs decision values."""
    X = np.ascontiguousarray(X, dtype=float)
    kind, gamma, coef0, degree = batch.spec
    k, m = batch.W.shape
    if X.ndim != 2 or X.shape[1] != batch.SV.shape[1]:
        raise ValueError('X must be t x %d, got shape %s' % (batch.SV.shape[1], X.shape))
    A, B = _lib.as_f64(A, k, 'A'), _lib.as_f64(B, k, 'B')
    t = len(X)
    prob = np.empty((t, ncls))
    iters, R, dec = (np.empty(t, dtype=np.int32), np.empty((t, k)), np.empty((k, t))) if details else (None, None, None)
    if t:
        _lib.check(_lib.load().bq_decision_coupled(get_context().handle, kind, gamma, coef0, degree, m, batch.SV.shape[1],
                                                   _lib.ptr(batch.SV), k, _lib.ptr(batch.W), _lib.ptr(batch.b), t, _lib.ptr(X), ncls,
                                                   _lib.ptr(A), _lib.ptr(B), _lib.ptr(prob), _lib.iptr(iters), _lib.ptr(R),
                                                   _lib.ptr(dec)))
    return (prob, iters, R, np.ascontiguousarray(dec.T)) if details else prob


def coupling_columns(codes, ncls, splits, C):
    """The batched path's panel and columns as plain arrays, for class codes 0..ncls-1 and (train, test) splits.  A dict of
    index, cls_tiles, n_pad (`sort_plan`); data_row (n_pad, 1 a data row, 0 a ghost row); pcode (the class of every panel row);
    pairs (`ovo_pairs`); cols, the columns in pair-major order as (pair number, fold number or None for the fit on all the data);
    Y, UB (columns x n_pad): the labels (+1 on the rows of the pair's larger class) and the boxes — C on the pair's data rows in the
    fold's training part, 0 on the fold's held-out rows, on ghost rows and on the rows of every other class."""
    codes = np.asarray(codes)
    index, cls_tiles, n_pad = sort_plan(codes, ncls)
    data_row = np.zeros(n_pad, dtype=np.uint8)
    data_row[index] = 1
    pcode = np.repeat(np.arange(ncls), np.diff(cls_tiles) * TILE)
    pairs = ovo_pairs(ncls)
    train = [np.ones(n_pad, dtype=bool)]   # last entry, reached as fold -1: all the data
    for tr, _ in splits:
        mask = np.zeros(n_pad, dtype=bool)
        mask[index[tr]] = True
        train.insert(len(train) - 1, mask)
    cols = [(p, f) for p in range(len(pairs)) for f in list(range(len(splits))) + [None]]
    Y = np.stack([np.where(pcode == pairs[p][1], 1., -1.) for p, _ in cols])
    UB = np.stack([np.where(((pcode == pairs[p][0]) | (pcode == pairs[p][1])) & (data_row > 0) & train[-1 if f is None else f],
                            float(C), 0.) for p, f in cols])
    return dict(index=index, cls_tiles=cls_tiles, n_pad=n_pad, data_row=data_row, pcode=pcode, pairs=pairs, cols=cols, Y=Y, UB=UB)


def chunk_calibrators(chunk_cols):
    """(cal_of, pair numbers): a solve's columns -> its calibrators.  A fold column feeds its pair's calibrator, numbered in order
    of appearance within the solve; the column of the fit on all the data feeds none (-1)."""
    local, cal_of = {}, []
    for p, f in chunk_cols:
        cal_of.append(-1 if f is None else local.setdefault(p, len(local)))
    return np.array(cal_of, dtype=np.int32), list(local)


class PairwiseCoupledSVC(ClassifierMixin, BaseEstimator):
    """Class probabilities of an `OneVsOneSVC` as `sklearn.svm.SVC(probability=True)` forms them: per class pair a Platt sigmoid
    fitted on the out-of-fold decision values of the pair's rows, and libsvm's pairwise coupling at prediction.  An int `cv` is
    StratifiedKFold(cv) without shuffling on all rows; every row must be held out exactly once and every fold's training rows must
    hold every class (else ValueError).  At most 64 classes.

    After `fit`: `classes_`; `estimator_`, the `OneVsOneSVC` fitted on all the data (on the batched path its pairs' iterates have
    the bits of `OneVsOneSVC(**kw).fit(X, y)`); `probA_`, `probB_` (one entry per pair in `ovo_pairs` order, positive class the
    larger label: see the module on libsvm's signs); `calibrators_`, a dict of the arrays A, B, iters, loss, flags, n_pos and n_neg
    of the sigmoids; `oof_decision_` (n x pairs, 0 where the row is in neither class of the pair); `n_iter_` / `status_` of shape
    (pairs, folds + 1), the last column the fit on all the data; `batched_`, which path ran, and `batched_decision_`:
    `predict_proba` takes the decision values and the coupling from one device call (`bq_decision_coupled`).  A sigmoid fit that
    ended on a failed line search or the iteration cap warns (`ConvergenceWarning`) and keeps the values reached.

    `predict_proba(X)` is t x classes; `predict` is libsvm's, the argmax of the probabilities (not the vote of
    `estimator_.predict`); `decision_function` is `estimator_`'s.
    """

    def __init__(self, estimator, cv=5):
        self.estimator = estimator
        self.cv = cv

    def fit(self, X, y):
        if not isinstance(self.estimator, OneVsOneSVC):
            raise TypeError('estimator must be a OneVsOneSVC')
        X = np.ascontiguousarray(X, dtype=float)
        y = np.asarray(y)
        self.classes_ = np.unique(y)
        ncls = len(self.classes_)
        if ncls < 2:
            raise ValueError('the training data must hold at least two classes')
        if ncls > MAX_CLASSES:
            raise ValueError('pairwise coupling takes at most %d classes (%d given)' % (MAX_CLASSES, ncls))
        codes = np.searchsorted(self.classes_, y)
        splits = check_cv_splits(self.cv, X, y)
        counts = np.zeros(len(y), dtype=np.int64)
        for _, te in splits:
            np.add.at(counts, te, 1)
        if not np.all(counts == 1):
            raise ValueError('the test folds must partition the rows: every row held out exactly once')
        for f, (tr, _) in enumerate(splits):
            if not np.array_equal(np.unique(y[tr]), self.classes_):
                raise ValueError('the training rows of fold %d miss a class' % f)
        world = get_context().world
        self.batched_ = uses_batched_coupling(self.estimator, world)
        fit = self._fit_batched if self.batched_ else self._fit_loop
        cal = fit(X, y, codes, splits)
        self.calibrators_ = {key: np.asarray(cal[key]) for key in ('A', 'B', 'iters', 'loss', 'flags', 'n_pos', 'n_neg')}
        self.probA_, self.probB_ = self.calibrators_['A'].copy(), self.calibrators_['B'].copy()
        bad = np.flatnonzero(self.calibrators_['flags'] & (_lib.PLATT_LINE_SEARCH | _lib.PLATT_MAX_ITER))
        if len(bad):
            warnings.warn('the sigmoid fit of %d pair(s) ended on a failed line search or the iteration cap (first: pair %d)'
                          % (len(bad), int(bad[0])), ConvergenceWarning)
        self.batched_decision_ = bool(self.estimator_.batched_decision_)
        return self

    def _new(self):
        """A fresh, unfitted `OneVsOneSVC` of the configuration"""
        return _make(OneVsOneSVC, _base_params(self.estimator), {})

    def _fit_loop(self, X, y, codes, splits):
        """Per pair and fold `SVC.fit` on the pair's training rows and `decision_function` on its held-out rows; the sigmoids through
        `bq_platt_fit`; `estimator_` by `OneVsOneSVC.fit`."""
        n, pairs = len(y), ovo_pairs(len(self.classes_))
        D, L = np.zeros((len(pairs), n)), np.zeros((len(pairs), n))
        self.n_iter_ = np.full((len(pairs), len(splits) + 1), -1, dtype=np.int64)
        self.status_ = np.full((len(pairs), len(splits) + 1), '', dtype=object)

        def record(p, f, est):
            opt = getattr(est, 'optimizer', None)
            self.n_iter_[p, f] = getattr(opt, 'iter', -1)
            self.status_[p, f] = getattr(opt, 'status', '')

        for p, (i, j) in enumerate(pairs):
            rows, yp = pair_problem(codes, i, j)
            L[p, rows] = yp
            inpair = np.zeros(n, dtype=bool)
            inpair[rows] = True
            for f, (tr, te) in enumerate(splits):
                tr, te = tr[inpair[tr]], te[inpair[te]]
                est = self.estimator._prototype().fit(X[tr], (codes[tr] == j).astype(int))
                D[p, te] = np.ravel(est.decision_function(X[te]))
                record(p, f, est)
        self.estimator_ = self._new().fit(X, y)
        for p, est in enumerate(self.estimator_.estimators_):
            record(p, len(splits), est)
        self.oof_decision_ = D.T.copy()
        return platt_fit(D, L)

    def _fit_batched(self, X, y, codes, splits):
        """One class-sorted panel; the columns (pair, fold) and (pair, all) in solves of `pair_chunks`' sizes on the pair-routed
        solver; intercepts, held-out decision values and sigmoids from the device (`heldout_pairs`)."""
        proto = self.estimator._prototype()
        ncls, ns = len(self.classes_), len(splits)
        plan = coupling_columns(codes, ncls, splits, proto.C)
        index, cls_tiles, n_pad, pairs, cols = plan['index'], plan['cls_tiles'], plan['n_pad'], plan['pairs'], plan['cols']
        P = len(pairs)
        Xp = np.zeros((n_pad, X.shape[1]))
        Xp[index] = X
        obj = KernelQuadratic(Xp, -np.ones(n_pad), 'svc', proto.kernel, y=np.ones(n_pad), storage=proto.storage,
                              tune_placement=proto._streams_panel(), expected_products=proto.max_iter)
        dev = obj.device_problem()
        kind = solver_kind(proto.optimizer)
        self.n_iter_ = np.zeros((P, ns + 1), dtype=np.int64)
        self.status_ = np.full((P, ns + 1), '', dtype=object)
        oof = np.zeros((P, n_pad))
        ests, W, fits = [None] * P, np.zeros((P, n_pad)), []
        c0 = 0
        for chunk in pair_chunks([pairs[p] for p, _ in cols], cls_tiles, n_pad, device_free_bytes()):
            sel = slice(c0, c0 + len(chunk))
            c0 += len(chunk)
            ccols = cols[sel]
            cal_of, cal_pairs = chunk_calibrators(ccols)
            kept = [j for j, (_, f) in enumerate(ccols) if f is None]   # the columns that become estimators
            held = {}

            def score(solver, out):
                if cal_pairs:
                    held['b'], held['n_sv'], held['fit'] = solver.heldout_pairs(plan['data_row'], cal_of, len(cal_pairs),
                                                                                decisions=True)
                else:   # only fits on all the data: one calibrator that nothing feeds
                    held['b'], held['n_sv'], _ = solver.heldout_pairs(plan['data_row'], cal_of, 1)
                for j in kept:
                    out[j].update(x=solver.get(j, _lib.GET_X_NOW), g=solver.get(j, _lib.GET_G_NOW))

            Y, UB = plan['Y'][sel], plan['UB'][sel]
            solver = _DevicePairSolver(dev, kind, cls_tiles, chunk, Y, UB, 1e-6, proto.max_iter)
            res = solve_batched(dev, kind, Y, UB, max_iter=proto.max_iter, solver=solver, before_close=score, vectors=False)
            if not held['n_sv'].all():
                raise ZeroDivisionError('a fit ended without support vectors')   # as SVC.fit's intercept
            if cal_pairs:
                fits.append((cal_pairs, held['fit']))
                oof[cal_pairs] += held['fit']['dec']   # the solves' rows of a pair are disjoint and 0 elsewhere
            for j, (p, f) in enumerate(ccols):
                self.n_iter_[p, ns if f is None else f] = res[j]['iter']
                self.status_[p, ns if f is None else f] = res[j]['status']
            for j in kept:
                p = ccols[j][0]
                rows, yp = pair_problem(codes, *pairs[p])
                pos = index[rows]
                est = self.estimator._prototype()
                sv = fitted_svc(est, obj, res[j], X[rows], yp, pos)
                W[p][pos[sv]] = est.dual_coef_
                est.intercept_ = float(held['b'][j])
                ests[p] = est
        del dev, obj
        if sum(len(cp) for cp, _ in fits) == P:   # every pair's folds in one solve: the sigmoids came from the device's own buffers
            cal = {key: np.empty(P, dtype=fits[0][1][key].dtype) for key in fits[0][1] if key != 'dec'}
            for cp, fit in fits:
                for key in cal:
                    cal[key][cp] = fit[key]
        else:   # a pair's folds were spread over several solves: the same kernel on the gathered rows
            L = np.stack([np.where(plan['pcode'] == j, 1., np.where(plan['pcode'] == i, -1., 0.)) * plan['data_row']
                          for i, j in pairs])
            cal = platt_fit(oof, L)
        self.oof_decision_ = oof[:, index].T.copy()
        ovo = self._new()
        ovo.classes_, ovo.estimators_, ovo.batched_ = self.classes_, ests, True
        ovo.batched_decision_ = uses_batched_decision(proto.kernel, P, get_context().world, True)
        ovo.decision_batch_ = None
        if ovo.batched_decision_:
            ovo.decision_batch_ = DecisionBatch(proto.kernel, Xp, W, [est.intercept_ for est in ests], keep=plan['data_row'] > 0)
        self.estimator_ = ovo
        return cal

    def pair_decisions(self, X):
        """t x pairs decision values of `estimator_`'s pairs, positive towards the larger label"""
        X = np.ascontiguousarray(X, dtype=float)
        if self.estimator_.batched_decision_:
            return self.estimator_.decision_batch_(X)
        return np.stack([np.ravel(e.decision_function(X)) for e in self.estimator_.estimators_], axis=1)

    def predict_proba(self, X):
        X = np.ascontiguousarray(X, dtype=float)
        ncls = len(self.classes_)
        if len(X) == 0:
            return np.empty((0, ncls))
        if not self.batched_decision_:
            return pairwise_coupling(self.pair_decisions(X), self.probA_, self.probB_, ncls)[0]
        return coupled_decision(self.estimator_.decision_batch_, X, self.probA_, self.probB_, ncls)

    def predict(self, X):
        return self.classes_[np.argmax(self.predict_proba(X), axis=1)]

    def decision_function(self, X):
        return self.estimator_.decision_function(X)
