"""One-vs-rest multi-class SVC: the result of sklearn's `OneVsRestClassifier(SVC(**kw))`, with the k binary duals solved
together on ONE Gram panel.

The panel does not depend on the labels: for the 'svc' structure class c's Hessian is Q_c = diag(y_c) (K + 1) diag(y_c), so every
first-order iteration of every class is a product with the same K + 1.  The batched path (`bq_msolver_*`) streams the panel once
per iteration for every 4 classes still running (bq_symm.hip) instead of once per class, and takes the intercepts' k masked
products in one multi-column product (`bq_problem_gram_matmat`).  Each class follows the iteration of `SVC.fit` with the same
optimizer — same formulas, thresholds, stop tests and records — and its iterates have the same bits whatever the other classes do.

Configurations the batched path does not cover (see `uses_batched_path`) fit the k binary problems one after another with `SVC`:
exactly what `OneVsRestClassifier(SVC)` does.
"""
import ctypes as C

import numpy as np

from ... import _lib
from ...device import get_context
from ...opti import KernelQuadratic
from ...opti.constrained import FrankWolfe, ProjectedGradient
from ._base import SVC, ClassifierMixin, BaseEstimator
from .kernels import LinearKernel, gaussian
from .losses import Hinge, squared_hinge

__all__ = ['OneVsRestSVC', 'uses_batched_path', 'binarize']


def uses_batched_path(svc, world):
    """True when `OneVsRestSVC` solves the classes of `svc`'s configuration together on one panel: the hinge dual with a regularised
    intercept by ProjectedGradient or FrankWolfe, a resident panel ('f64' / 'f32') and a single-rank context (`world` ranks).
    Every other configuration fits one `SVC` per class."""
    opt = svc.optimizer
    return bool(svc.dual and svc.reg_intercept and svc.loss == Hinge and isinstance(opt, type) and
                issubclass(opt, (ProjectedGradient, FrankWolfe)) and svc.storage in ('f64', 'f32') and int(world) == 1)


def binarize(y):
    """(classes_, Y): classes_ = np.unique(y) and Y[c] = +1 where y == classes_[c], -1 elsewhere (the labels OneVsRestClassifier
    hands SVC.fit after its LabelBinarizer, mapped as SVC maps them); with two classes the single row of classes_[1]."""
    y = np.asarray(y)
    classes = np.unique(y)
    if len(classes) < 2:
        raise ValueError('the training data must hold at least two classes')
    rows = classes[1:] if len(classes) == 2 else classes
    Y = np.stack([np.where(y == c, 1., -1.) for c in rows])
    return classes, Y


class _DeviceMultiSolver:
    def __init__(self, problem, kind, Y, ub, eps, max_iter, t=0.0, x0=None):
        self._lib = _lib.load()
        self.k, self.n = Y.shape
        self._h = C.c_void_p()
        Y = _lib.as_f64(Y, self.k * self.n, 'Y')
        boxes = np.ndim(ub) == 2   # one box per column (k x n): bq_msolver_create_boxes and the 16-column product
        ub = _lib.as_f64(ub, self.k * self.n if boxes else self.n, 'ub')
        x0 = None if x0 is None else _lib.as_f64(x0, self.k * self.n, 'x0')
        create = self._lib.bq_msolver_create_boxes if boxes else self._lib.bq_msolver_create
        _lib.check(create(problem.handle, kind, self.k, _lib.ptr(Y), _lib.ptr(ub), _lib.ptr(x0), float(eps), int(max_iter), float(t),
                          C.byref(self._h)))

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

    def close(self):
        if self._h:
            self._lib.bq_msolver_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def solve_batched(problem, kind, Y, ub, eps=1e-6, max_iter=1000, t=0.0, x0=None, chunk=256, solver=None):
    """Run the batched solver (`problem`: a device problem of KernelQuadratic 'svc'; Y: k x n labels +-1; ub: n, or k x n for one box
    per column (bq_msolver_create_boxes); x0: k x n or None)
    to the end: per class a dict (rows: the iteration records, status, iter, f_x, x, g) as a single-class optimizer ends them.
    solver: an already created solver of these columns (the one-vs-one pair solver) instead of bq_msolver_create(_boxes)."""
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
            out.append(dict(rows=np.concatenate(rows[c]), status=st, iter=it, f_x=f, x=solver.get(c, _lib.GET_X_NOW),
                            g=solver.get(c, _lib.GET_G_NOW)))
        return out
    finally:
        solver.close()


class OneVsRestSVC(ClassifierMixin, BaseEstimator):
    """One-vs-rest multi-class SVC; constructor arguments and their checks are SVC's.

    After `fit`: `classes_`, `estimators_` (one fitted SVC per class — per binary problem with two classes), and
    `decision_function` (m x k; 1-D with two classes), `predict`, `score` as sklearn's OneVsRestClassifier(SVC(**kw)).
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

    def fit(self, X, y):
        X = np.ascontiguousarray(X, dtype=float)
        self.classes_, Y = binarize(y)
        proto = self._prototype()
        self.batched_ = uses_batched_path(proto, get_context().world)
        if not self.batched_:
            self.estimators_ = [self._prototype().fit(X, (Yc > 0).astype(int)) for Yc in Y]
            return self
        self.estimators_ = self._fit_batched(proto, X, Y)
        return self

    def _fit_batched(self, proto, X, Y):
        k, n = Y.shape
        ub = np.ones(n) * proto.C
        # one panel for every class: the 'svc' structure's own labels are never used by the batched solver
        obj = KernelQuadratic(X, -np.ones(n), 'svc', proto.kernel, y=Y[0], storage=proto.storage,
                              tune_placement=proto._streams_panel(), expected_products=proto.max_iter * ((k + 3) // 4))
        opt_type = proto.optimizer
        dev = obj.device_problem()
        kind = _lib.PG if issubclass(opt_type, ProjectedGradient) else _lib.FW
        res = solve_batched(dev, kind, Y, ub, eps=1e-6, max_iter=proto.max_iter)
        ests, masks, coefs = [], [], []
        for c in range(k):
            est = self._prototype()
            r = res[c]
            # the optimizer as SVC.fit leaves it (constrained/_base.py: minimize) — constructed, not run
            opt = opt_type(quad=obj, ub=ub, tol=proto.tol, max_iter=proto.max_iter, verbose=proto.verbose)
            if len(r['rows']):
                opt.iter = int(r['rows'][-1]['iter'])
                opt._after_row(r['rows'][-1])
            opt.status, opt.f_x, opt.x, opt.g_x = r['status'], r['f_x'], r['x'], r['g']
            est.train_loss_history = [float(f) for f in r['rows']['f']]
            est.optimizer = opt
            est.classes_ = np.array([0, 1])   # OneVsRestClassifier fits each SVC on the 0 / 1 column of its LabelBinarizer
            est.alphas_ = opt.x
            sv = est.alphas_ > 1e-6
            est.support_ = np.arange(n)[sv]
            est.support_vectors_ = X[sv]
            est.dual_coef_ = est.alphas_[sv] * Y[c][sv]
            if isinstance(est.kernel, LinearKernel):
                est.coef_ = np.dot(est.dual_coef_, est.support_vectors_)
            w = np.zeros(n)
            w[sv] = est.dual_coef_
            ests.append(est)
            masks.append(sv)
            coefs.append(w)
            if self.verbose:
                print('class %r: %s after %d iterations, f = %1.6e' % (self.classes_[c if len(self.classes_) > 2 else 1],
                                                                         opt.status, opt.iter, opt.f_x))
        U = _gram_matmat(dev, np.stack(coefs))
        for c, est in enumerate(ests):
            sv = masks[c]
            est.intercept_ = 0.
            est.intercept_ += float(np.sum(Y[c][sv] - U[c][sv]))
            est.intercept_ /= int(sv.sum())
        return ests

    def decision_function(self, X):
        scores = np.stack([e.decision_function(X) for e in self.estimators_], axis=1)
        return scores[:, 0] if len(self.classes_) == 2 else scores

    def predict(self, X):
        scores = self.decision_function(X)
        if len(self.classes_) == 2:
            return self.classes_[(scores > 0).astype(int)]
        return self.classes_[np.argmax(scores, axis=1)]


def _gram_matmat(problem, W, wide=False):
    """OUT[c] = K W[c] for the rows of W, one multi-column product (bq_problem_gram_matmat; wide: the 16-column
    bq_problem_gram_matmat_wide)."""
    W = np.ascontiguousarray(W, dtype=float)
    out = np.empty_like(W)
    fn = _lib.load().bq_problem_gram_matmat_wide if wide else _lib.load().bq_problem_gram_matmat
    _lib.check(fn(problem.handle, W.shape[0], _lib.ptr(W), _lib.ptr(out)))
    return out
