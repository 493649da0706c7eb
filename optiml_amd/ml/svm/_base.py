"""sklearn-compatible SVC / SVR restricted to the box-constrained dual path, device-resident.

Constructor arguments, validation and fitted attributes follow optiml/ml/svm/_base.py (SVM :187-282,
SVC :366-419, SVR :907-963).  Two dual branches are implemented:

    dual=True, reg_intercept=True, optimizer in {ProjectedGradient, FrankWolfe, ActiveSet, InteriorPoint}
        (SVC.fit :547-559, :619-636, :725, :867-880; SVR.fit :1091-1104, :1169-1186, :1277, :1423-1437)
    dual=True, optimizer in {StochasticGradientDescent, Adam, AMSGrad, AdaMax, AdaGrad, AdaDelta, RMSProp}
        on the augmented Lagrangian of the dual, reg_intercept True or False, all four losses
        (SVC.fit :638-723, :776-860; SVR.fit :1188-1270, :1330-1415) — SURVEY 8(f).3
    dual=True, reg_intercept=False, optimizer='smo' (or SMO): SMOClassifier / SMORegression on the resident panel
        (SVC.fit :560-573, SVR.fit :1106-1120) — SURVEY 8(f).4; with storage='stream' RowSMOClassifier / RowSMORegression
        (smo_rows.py): libsvm's WSS2 decomposition on kernel rows made on demand, no panel, `tol` libsvm's (sklearn's)

In both the Gram panel is built and kept in HBM, the Wolfe dual never exists as an n x n host matrix
(`self.obj` is a lazy `KernelQuadratic`), and the support-vector / intercept post-processing uses one masked
panel product instead of the reference's Python loop.  Every other configuration raises NotImplementedError
(as the reference does for reg_intercept=False and for the squared losses with these optimizers).
"""
from abc import ABC

import numpy as np

from ... import _lib
from ...device import get_context
from ...opti import Optimizer, KernelQuadratic
from ...opti.constrained import BoxConstrainedQuadraticOptimizer, ProjectedGradient, AugmentedLagrangianQuadratic
from ...opti.unconstrained.stochastic import StochasticOptimizer, StochasticMomentumOptimizer
from .kernels import Kernel, LinearKernel, gaussian, BaseEstimator
from .smo import SMO, SMOClassifier, SMORegression
from .smo_rows import RowSMOClassifier, RowSMORegression
from .losses import (Hinge, SquaredHinge, EpsilonInsensitive, SquaredEpsilonInsensitive,
                     squared_hinge, squared_epsilon_insensitive)

try:
    from sklearn.base import ClassifierMixin, RegressorMixin
except ImportError:  # pragma: no cover
    class ClassifierMixin:
        def score(self, X, y):
            return float(np.mean(self.predict(X) == np.asarray(y)))

    class RegressorMixin:
        def score(self, X, y):
            y = np.asarray(y, dtype=float)
            r = y - self.predict(X)
            return 1.0 - float(r @ r) / float(((y - y.mean()) ** 2).sum())

__all__ = ['SVM', 'SVC', 'SVR', 'row_boxes', 'has_class_weight']


def has_class_weight(est):
    """True when `est` carries a `class_weight`: every batched path that was not taught about per-row boxes answers False to such an
    estimator, so that the per-column / per-fold calls of `SVC.fit` apply the weights."""
    return getattr(est, 'class_weight', None) is not None


def row_boxes(C, y=None, classes=None, class_weight=None, sample_weight=None):
    """The box of every row, C_i = C * sample_weight_i * class_weight[y_i] (libsvm's and sklearn.svm's weighting), or None when
    neither weight is given.  class_weight: None, a dict {label: weight} (a missing label weighs 1, a key outside `classes` is a
    ValueError, weights finite and > 0) or 'balanced' = n / (n_classes * bincount(y)) over the rows given, which is
    sklearn.utils.class_weight.compute_class_weight's formula.  sample_weight: n finite entries >= 0, not all zero.  A row whose box
    is 0 is one `fit` drops."""
    if class_weight is None and sample_weight is None:
        return None
    if sample_weight is not None:
        sample_weight = np.asarray(sample_weight, dtype=float)
        if sample_weight.ndim != 1 or (y is not None and len(sample_weight) != len(y)):
            raise ValueError('sample_weight must hold one weight per row')
        if not np.isfinite(sample_weight).all() or (sample_weight < 0).any():
            raise ValueError('sample_weight must be finite and >= 0')
        if not (sample_weight > 0).any():
            raise ValueError('sample_weight must not be zero on every row')
    if class_weight is None:
        return C * sample_weight
    y = np.asarray(y)
    classes = np.asarray(classes)
    codes = np.searchsorted(classes, y)
    if isinstance(class_weight, str):
        if class_weight != 'balanced':
            raise ValueError("class_weight must be None, a dict or 'balanced'")
        w = len(y) / (len(classes) * np.bincount(codes, minlength=len(classes)).astype(np.float64))
    elif isinstance(class_weight, dict):
        w = np.ones(len(classes))
        for label, value in class_weight.items():
            at = np.flatnonzero(classes == label)
            if len(at) != 1:
                raise ValueError('class_weight names the label %r, which is not among the classes %r' % (label, list(classes)))
            if not (np.isfinite(value) and value > 0):
                raise ValueError('class weights must be finite and > 0')
            w[at[0]] = value
    else:
        raise ValueError("class_weight must be None, a dict or 'balanced'")
    return C * w[codes] if sample_weight is None else C * sample_weight * w[codes]


def _kept_rows(box, y, n_groups):
    """the rows a weighted fit keeps (box > 0), or None when it keeps every row; y: the labels (None: regression)"""
    if box is None or (box > 0).all():
        return None
    keep = np.flatnonzero(box > 0)
    if y is not None and len(np.unique(y[keep])) < n_groups:
        raise ValueError('the weights leave a class without rows')
    return keep


def _scattered(values, keep, n):
    out = np.zeros(n)
    out[keep] = values
    return out

_OUT_OF_SCOPE = ('only dual=True with a box-constrained optimizer (ProjectedGradient, FrankWolfe, ActiveSet, '
                 'InteriorPoint) or a stochastic optimizer on the augmented-Lagrangian dual is implemented by '
                 'optiml_amd')

try:
    from sklearn.exceptions import ConvergenceWarning
except ImportError:  # pragma: no cover
    class ConvergenceWarning(UserWarning):
        pass


class SVM(BaseEstimator, ABC):

    def __init__(self, loss=None, kernel=gaussian, C=1, rho=1, mu=1, fit_intercept=True, intercept_scaling=1,
                 reg_intercept=False, dual=False, optimizer=ProjectedGradient, master_solver='clarabel',
                 learning_rate='auto', momentum_type='none', momentum=0.9, max_iter=1000, max_f_eval=15000,
                 tol=1e-4, batch_size=None, shuffle=True, random_state=None, early_stopping=False,
                 validation_split=0., patience=5, verbose=False, master_verbose=False, storage='f64'):
        self.loss = loss
        if not isinstance(kernel, Kernel):
            raise TypeError(f'{kernel} is not an allowed kernel function')
        self.kernel = kernel
        if not C > 0:
            raise ValueError('C must be > 0')
        self.C = C
        if not rho > 0:
            raise ValueError('rho must be > 0')
        self.rho = rho
        if not mu > 0:
            raise ValueError('mu must be > 0')
        self.mu = mu
        if not isinstance(fit_intercept, bool):
            raise ValueError('fit_intercept mu be a boolean value')
        self.fit_intercept = fit_intercept
        self.intercept_scaling = intercept_scaling
        if not isinstance(reg_intercept, bool):
            raise ValueError('reg_intercept mu be a boolean value')
        self.reg_intercept = reg_intercept
        if not isinstance(dual, bool):
            raise ValueError('dual must be a boolean value')
        self.dual = dual
        if not (isinstance(optimizer, str) or (isinstance(optimizer, type) and
                                               (issubclass(optimizer, Optimizer) or issubclass(optimizer, SMO)))):
            raise TypeError(f'{optimizer} is not an allowed optimization method')
        self.optimizer = optimizer
        self.master_solver = master_solver
        self.learning_rate = learning_rate
        self.max_iter = max_iter
        self.max_f_eval = max_f_eval
        self.momentum_type = momentum_type
        self.momentum = momentum
        if not tol > 0:
            raise ValueError('tol must be > 0')
        self.tol = tol
        self.batch_size = batch_size
        self.shuffle = shuffle
        self.random_state = random_state
        self.early_stopping = early_stopping
        self.validation_split = validation_split
        self.patience = patience
        self.verbose = verbose
        self.master_verbose = master_verbose
        self.storage = storage
        if not self.dual or isinstance(self.kernel, LinearKernel):
            self.coef_ = np.zeros(0)
        self.intercept_ = 0.
        self.support_ = np.zeros(0)
        self.support_vectors_ = np.zeros(0)
        if self.dual:
            self.alphas_ = np.zeros(0)
            self.dual_coef_ = np.zeros(0)
        if not isinstance(optimizer, str):
            self.train_loss_history = []

    def fit(self, X, y):
        raise NotImplementedError

    def decision_function(self, X):
        X = np.ascontiguousarray(X, dtype=float)
        if self.dual and not isinstance(self.kernel, LinearKernel):
            # gamma='scale' resolves against the support vectors here, as in the reference (kernels.py:127 with
            # kernel(self.support_vectors_, X), svm/_base.py:286) — not against the training set
            sv = np.ascontiguousarray(self.support_vectors_, dtype=float)
            kind, gamma, coef0, degree = self.kernel.device_spec(sv)
            lib = _lib.load()
            out = np.empty(X.shape[0])
            coef = _lib.as_f64(self.dual_coef_, sv.shape[0], 'dual_coef_')
            _lib.check(lib.bq_decision_function(get_context().handle, kind, gamma, coef0, degree, sv.shape[0],
                                                sv.shape[1], _lib.ptr(sv), _lib.ptr(coef), float(self.intercept_),
                                                X.shape[0], _lib.ptr(X), _lib.ptr(out)))
            return out
        return np.dot(X, self.coef_) + self.intercept_

    def _store_train_info(self, opt):
        if opt.is_lagrangian_dual():
            self.train_loss_history.append(opt.primal_f_x)
        else:
            self.train_loss_history.append(opt.f_x)

    _store_train_info._bq_needs_state = False  # reads opt.f_x only: replayed from the device iteration records

    def _is_smo(self):
        return self.dual and (self.optimizer == 'smo' or self.optimizer is SMO)

    def _smo_solver(self, resident, rows, obj, *args):
        """The SMO branch of `fit`: the walker on the resident panel (`resident`), or, with storage='stream', libsvm's decomposition
        on kernel rows made on demand (`rows`; single-rank contexts).  The two read `tol` differently: the walker compares every
        example with its thresholds b_up / b_low under 2 tol (smo.py), the row-based solver stops when libsvm's Gmax + Gmax2 < tol,
        which is sklearn.svm's tol.  A run that ends at libsvm's iteration cap warns like the augmented-Lagrangian branch."""
        if self.storage != 'stream':
            return resident(obj, *args).minimize()
        if get_context().world != 1:
            raise NotImplementedError("optimizer='smo' with storage='stream' runs on a single-rank context")
        opt = rows(obj, *args).minimize()
        if opt.status == 'stopped':
            import warnings
            warnings.warn('max_iter reached but the optimization has not converged yet', ConvergenceWarning)
        return opt

    def _is_stochastic(self):
        return self.dual and isinstance(self.optimizer, type) and issubclass(self.optimizer, StochasticOptimizer)

    # Choose the panel's placement (`KernelQuadratic(tune_placement=True)`, BQ_PLACE_PANEL) for the optimizers whose every
    # iteration is one panel product: the launch time of the product is a stable property of where the allocation landed (6.04 ...
    # 6.50 ms at n = 100 000) and nothing on the allocation side changes it, so the library times the product on the
    # fresh panel and, if it streams slowly, on as many further allocations as fit a 0.2 s budget (BQ_PLACE_BUDGET_MS), and keeps
    # the fastest.  On by default since round 4 — the path bench.py measures is the path `fit` runs; `SVC.tune_placement = False`
    # (class or instance) takes the first allocation.
    tune_placement = True

    def _streams_panel(self):
        from ...opti.constrained import ActiveSetCG, FrankWolfe, ProjectedGradient
        return bool(self.tune_placement) and isinstance(self.optimizer, type) and (
            issubclass(self.optimizer, (ProjectedGradient, FrankWolfe, ActiveSetCG)) or
            issubclass(self.optimizer, StochasticOptimizer))

    def _check_bcqp(self):
        if not self.dual or isinstance(self.optimizer, str) or not (
                isinstance(self.optimizer, type) and issubclass(self.optimizer, BoxConstrainedQuadraticOptimizer)):
            raise NotImplementedError(_OUT_OF_SCOPE)
        if not self.reg_intercept:
            # constrained optimizer with A x = 0 and 0 <= x <= ub is not available (svm/_base.py:621-624)
            raise NotImplementedError('box-constrained optimizers need reg_intercept=True')

    def _run(self, obj, ub):
        hook = self._store_train_info
        self.obj = obj
        self.optimizer = self.optimizer(quad=obj, ub=ub, tol=self.tol, max_iter=self.max_iter,
                                        callback=hook, verbose=self.verbose).minimize()
        self.alphas_ = self.optimizer.x

    def _lagrangian(self, primal, a, ub):
        """The objective and the optimizer of the augmented-Lagrangian branch as `_run_lagrangian` constructs them, not run: the
        batched fits take every column's start point and multipliers from here."""
        if isinstance(self.learning_rate, str) or not self.learning_rate > 0:
            raise ValueError('the dual needs a numeric learning_rate > 0')
        n = primal.ndim
        obj = AugmentedLagrangianQuadratic(primal=primal, A=a, b=None if a is None else np.zeros(1),
                                           lb=np.zeros(n), ub=ub, rho=self.rho)
        kw = dict(f=obj, tol=self.tol, step_size=self.learning_rate, epochs=self.max_iter,
                  random_state=self.random_state, callback=self._store_train_info, verbose=self.verbose)
        if issubclass(self.optimizer, StochasticMomentumOptimizer):
            kw.update(momentum_type=self.momentum_type, momentum=self.momentum)
        return obj, self.optimizer(**kw)

    def _run_lagrangian(self, primal, a, ub):
        """svm/_base.py:674-723 (SVC) / :1188-1270 (SVR): augmented Lagrangian of the dual + a stochastic optimizer."""
        import warnings
        self.obj, opt = self._lagrangian(primal, a, ub)
        self.optimizer = opt.minimize()
        if self.optimizer.status == 'stopped':
            warnings.warn('max_iter reached but the optimization has not converged yet', ConvergenceWarning)
        self.alphas_ = self.optimizer.x

    def _intercept_sum(self, obj, sv, dual_coef, sv_y):
        """sum_n ( y_n - sum_m dual_coef_m K[support_n, support_m] ) over the support set: one masked panel product."""
        w = np.zeros(len(sv))
        w[sv] = dual_coef
        u = obj.device_problem().gram_matvec(w)
        return float(np.sum(sv_y - u[sv]))


class SVC(ClassifierMixin, SVM):

    def __init__(self, loss=squared_hinge, kernel=gaussian, C=1, rho=1, mu=1, fit_intercept=True,
                 intercept_scaling=1, reg_intercept=False, dual=False, optimizer=ProjectedGradient,
                 master_solver='clarabel', learning_rate='auto', momentum_type='none', momentum=0.9, max_iter=1000,
                 max_f_eval=15000, tol=1e-4, batch_size=None, shuffle=True, random_state=None, early_stopping=False,
                 validation_split=0., patience=5, verbose=False, master_verbose=False, storage='f64', class_weight=None):
        super(SVC, self).__init__(loss=loss, kernel=kernel, C=C, rho=rho, mu=mu, fit_intercept=fit_intercept,
                                  intercept_scaling=intercept_scaling, reg_intercept=reg_intercept, dual=dual,
                                  optimizer=optimizer, master_solver=master_solver, learning_rate=learning_rate,
                                  momentum_type=momentum_type, momentum=momentum, max_iter=max_iter,
                                  max_f_eval=max_f_eval, tol=tol, batch_size=batch_size, shuffle=shuffle,
                                  random_state=random_state, early_stopping=early_stopping,
                                  validation_split=validation_split, patience=patience, verbose=verbose,
                                  master_verbose=master_verbose, storage=storage)
        if not getattr(loss, '_loss_type', None) == 'classifier':
            raise TypeError(f'{loss} is not an allowed SVC loss function')
        if not (class_weight is None or isinstance(class_weight, dict) or class_weight == 'balanced'):
            raise ValueError("class_weight must be None, a dict or 'balanced'")
        self.class_weight = class_weight

    def fit(self, X, y, sample_weight=None):
        """sample_weight / `class_weight`: row i's box is C_i = C * sample_weight_i * class_weight[y_i] (`row_boxes`) in the SMO
        branch, the box-constrained branch and the augmented-Lagrangian branch of the hinge dual; rows with C_i = 0 are dropped
        before the panel is built (`alphas_` holds 0 for them, `support_` indexes the rows given).  The squared hinge carries
        1 / (2C) as one scalar diagonal and refuses weights."""
        y = np.asarray(y)
        self.classes_ = np.unique(y)
        if len(self.classes_) > 2:
            raise ValueError('use OneVsOneClassifier or OneVsRestClassifier from sklearn.multiclass '
                             'to train a model over more than two labels')
        box = row_boxes(self.C, y, self.classes_, self.class_weight, sample_weight)
        # LabelBinarizer(neg_label=-1): the larger class label maps to +1 (svm/_base.py:419, 436-440)
        y = np.where(y == self.classes_[-1], 1., -1.)
        X = np.ascontiguousarray(X, dtype=float)
        keep = _kept_rows(box, y, len(self.classes_))
        if keep is not None:
            X_all, y_all = X, y
            X, y, box = np.ascontiguousarray(X[keep]), y[keep], box[keep]
        if box is not None and self.dual and self.loss == SquaredHinge:
            raise NotImplementedError('class_weight / sample_weight are not implemented for the squared hinge: its dual carries '
                                      '1 / (2C) as one scalar diagonal, not a box per row')
        n = len(y)
        if self._is_smo():
            if self.loss != Hinge or self.reg_intercept:
                raise NotImplementedError('SMO solves the hinge dual with an unregularised intercept')   # :571-573
            obj = KernelQuadratic(X, -np.ones(n), 'svc', self.kernel, y=y, storage=self.storage, rank_one=False, compact=False)
            self.obj = obj
            self.optimizer = self._smo_solver(SMOClassifier, RowSMOClassifier, obj, X, y, None, self.kernel, self.C, self.tol,
                                              self.verbose, box)
            self.alphas_ = self.optimizer.alphas
        elif self._is_stochastic():
            if self.loss not in (Hinge, SquaredHinge):
                raise TypeError(f'{self.loss} is not an allowed loss')
            sq = self.loss == SquaredHinge   # Q += I/(2C), no upper bound (svm/_base.py:727-730, :778-794)
            obj = KernelQuadratic(X, -np.ones(n), 'svc', self.kernel, y=y, storage=self.storage,
                                  diag=1. / (2 * self.C) if sq else 0., rank_one=self.reg_intercept,
                                  tune_placement=self._streams_panel(), expected_products=self.max_iter)
            self._run_lagrangian(obj, None if self.reg_intercept else y,
                                 None if sq else np.ones(n) * self.C if box is None else box)
        else:
            self._check_bcqp()
            if self.loss == SquaredHinge:
                # bcqp optimizer with 0 <= x <= +inf is not available (svm/_base.py:771-774)
                raise NotImplementedError('squared hinge is not available with box-constrained optimizers')
            if self.loss != Hinge:
                raise TypeError(f'{self.loss} is not an allowed loss')
            obj = KernelQuadratic(X, -np.ones(n), 'svc', self.kernel, y=y, storage=self.storage,
                                  tune_placement=self._streams_panel(), expected_products=self.max_iter)
            self._run(obj, np.ones(n) * self.C if box is None else box)

        if keep is not None:   # back to the rows given: the dropped ones hold 0
            self.alphas_ = _scattered(self.alphas_, keep, len(y_all))
            X, y = X_all, y_all
        sv = self.alphas_ > 1e-6
        self.support_ = np.arange(len(self.alphas_))[sv]
        self.support_vectors_, sv_y, alphas = X[sv], y[sv], self.alphas_[sv]
        self.dual_coef_ = alphas * sv_y
        if isinstance(self.optimizer, (SMOClassifier, RowSMOClassifier)):   # svm/_base.py:569-571, :872
            if isinstance(self.kernel, LinearKernel):
                self.coef_ = self.optimizer.w
            self.intercept_ = self.optimizer.b
            return self
        if isinstance(self.kernel, LinearKernel):
            self.coef_ = np.dot(self.dual_coef_, self.support_vectors_)
        self.intercept_ += self._intercept_sum(obj, sv if keep is None else sv[keep], self.dual_coef_, sv_y)
        self.intercept_ /= len(alphas)
        return self

    def predict(self, X):
        return np.where(self.decision_function(X) > 0, self.classes_[-1], self.classes_[0])


class SVR(RegressorMixin, SVM):

    def __init__(self, loss=squared_epsilon_insensitive, epsilon=0.1, kernel=gaussian, C=1, rho=1, mu=1,
                 fit_intercept=True, intercept_scaling=1, reg_intercept=False, dual=False,
                 optimizer=ProjectedGradient, master_solver='clarabel', learning_rate='auto', momentum_type='none',
                 momentum=0.9, max_iter=1000, max_f_eval=15000, tol=1e-4, batch_size=None, shuffle=True,
                 random_state=None, early_stopping=False, validation_split=0., patience=5, verbose=False,
                 master_verbose=False, storage='f64'):
        super(SVR, self).__init__(loss=loss, kernel=kernel, C=C, rho=rho, mu=mu, fit_intercept=fit_intercept,
                                  intercept_scaling=intercept_scaling, reg_intercept=reg_intercept, dual=dual,
                                  optimizer=optimizer, master_solver=master_solver, learning_rate=learning_rate,
                                  momentum_type=momentum_type, momentum=momentum, max_iter=max_iter,
                                  max_f_eval=max_f_eval, tol=tol, batch_size=batch_size, shuffle=shuffle,
                                  random_state=random_state, early_stopping=early_stopping,
                                  validation_split=validation_split, patience=patience, verbose=verbose,
                                  master_verbose=master_verbose, storage=storage)
        if not getattr(loss, '_loss_type', None) == 'regressor':
            raise TypeError(f'{loss} is not an allowed SVR loss function')
        if not epsilon >= 0:
            raise ValueError('epsilon must be >= 0')
        self.epsilon = epsilon

    def fit(self, X, y, sample_weight=None):
        """sample_weight: row i's box is C_i = C * sample_weight_i on both of its multipliers (`row_boxes`), as `SVC.fit` applies it;
        the squared epsilon-insensitive loss refuses weights."""
        y = np.asarray(y, dtype=float)
        targets = y.shape[1] if y.ndim > 1 else 1
        if targets > 1:
            raise ValueError('use sklearn.multioutput.MultiOutputRegressor '
                             'to train a model over more than one target')
        X = np.ascontiguousarray(X, dtype=float)
        box = row_boxes(self.C, y, sample_weight=sample_weight)
        keep = _kept_rows(box, None, 0)
        if keep is not None:
            X_all, y_all = X, y
            X, y, box = np.ascontiguousarray(X[keep]), y[keep], box[keep]
        if box is not None and self.dual and self.loss == SquaredEpsilonInsensitive:
            raise NotImplementedError('sample_weight is not implemented for the squared epsilon-insensitive loss: its dual carries '
                                      '1 / (2C) as one scalar diagonal, not a box per row')
        n = len(y)
        q = np.hstack((-y, y)) + self.epsilon
        if self._is_smo():
            if self.loss != EpsilonInsensitive or self.reg_intercept:
                raise NotImplementedError('SMO solves the epsilon-insensitive dual with an unregularised intercept')
            obj = KernelQuadratic(X, q, 'svr', self.kernel, storage=self.storage, rank_one=False, compact=False)
            self.obj = obj
            self.optimizer = self._smo_solver(SMORegression, RowSMORegression, obj, X, y, None, self.kernel, self.C, self.epsilon,
                                              self.tol, self.verbose, box)
            self.alphas_ = np.concatenate((self.optimizer.alphas_p, self.optimizer.alphas_n))
        elif self._is_stochastic():
            if self.loss not in (EpsilonInsensitive, SquaredEpsilonInsensitive):
                raise TypeError(f'{self.loss} is not an allowed loss')
            sq = self.loss == SquaredEpsilonInsensitive   # Q += I/(2C), no upper bound (svm/_base.py:1279-1283, :1332-1348)
            obj = KernelQuadratic(X, q, 'svr', self.kernel, storage=self.storage,
                                  diag=1. / (2 * self.C) if sq else 0., rank_one=self.reg_intercept,
                                  tune_placement=self._streams_panel(), expected_products=self.max_iter)
            e = np.hstack((np.ones(n), -np.ones(n)))   # equality row
            self._run_lagrangian(obj, None if self.reg_intercept else e,
                                 None if sq else np.ones(2 * n) * self.C if box is None else np.hstack((box, box)))
        else:
            self._check_bcqp()
            if self.loss == SquaredEpsilonInsensitive:
                # bcqp optimizer with 0 <= x <= +inf is not available (svm/_base.py:1325-1328)
                raise NotImplementedError('squared epsilon-insensitive is not available with box-constrained '
                                          'optimizers')
            if self.loss != EpsilonInsensitive:
                raise TypeError(f'{self.loss} is not an allowed loss')
            obj = KernelQuadratic(X, q, 'svr', self.kernel, storage=self.storage, tune_placement=self._streams_panel(), expected_products=self.max_iter)
            self._run(obj, np.ones(2 * n) * self.C if box is None else np.hstack((box, box)))

        if keep is not None:   # back to the rows given: the dropped ones hold 0
            self.alphas_ = np.concatenate([_scattered(half, keep, len(y_all)) for half in np.split(self.alphas_, 2)])
            X, y = X_all, y_all
        alphas_p, alphas_n = np.split(self.alphas_, 2)
        sv = np.logical_or(alphas_p > 1e-6, alphas_n > 1e-6)
        self.support_ = np.arange(len(alphas_p))[sv]
        self.support_vectors_, sv_y, alphas_p, alphas_n = X[sv], y[sv], alphas_p[sv], alphas_n[sv]
        self.dual_coef_ = alphas_p - alphas_n
        if isinstance(self.optimizer, (SMORegression, RowSMORegression)):   # svm/_base.py:1116-1118, :1428
            if isinstance(self.kernel, LinearKernel):
                self.coef_ = self.optimizer.w
            self.intercept_ = self.optimizer.b
            return self
        if isinstance(self.kernel, LinearKernel):
            self.coef_ = np.dot(self.dual_coef_, self.support_vectors_)
        self.intercept_ += self._intercept_sum(obj, sv if keep is None else sv[keep], self.dual_coef_, sv_y)
        self.intercept_ -= self.epsilon   # subtracted once before the division, as svm/_base.py:1436-1437
        self.intercept_ /= len(alphas_p)
        return self

    def predict(self, X):
        return self.decision_function(X)
