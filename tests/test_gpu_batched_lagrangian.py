"""The batched augmented-Lagrangian solver on the device (bq_msolver.hip: bq_msolver_create_al — mal_prep / mal_finish / mal_update /
mal_flush kernels on the 4-column panel product) and the two estimators that use it, `OneVsRestSVC` and `MultiOutputSVR` with a
stochastic optimizer: against the CPU oracle (oracle/al_oracle.py on svm_oracle.gram), against itself alone / in a batch / in a
permuted batch / cut into runs, and against the loop of single fits.

Tolerances are test_gpu_lagrangian.py's (`_cmp`): iteration counts and statuses equal, value and primal-value histories rtol 1e-9 /
atol 1e-10, iterates and multipliers rtol 1e-6 / atol 1e-9, gradients atol 1e-8.  The common data is n = 300 (a ragged second tile
row) with k = 5 classes (a full chunk of 4 columns and a ragged second panel stream)."""
import functools
import warnings

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

C_ = 1.0
N, D, K = 300, 8, 5

# name -> (squared loss, regularised intercept, oracle rule, optimizer class, rule keywords).  The step sizes keep the oracle's
# iterates bounded on this data for 100 epochs (max |x| < 1.6; SGD at 0.01 overflows); every class ends 'stopped' at iteration 99.
CONFIGS = {
    'adagrad_nob': (False, False, 'adagrad', 'AdaGrad', dict(step_size=1.)),                     # equality row + both bounds
    'adam_sq_b': (True, True, 'adam', 'Adam', dict(step_size=0.01, momentum_type='polyak', momentum=0.5)),   # diag, lb only, K + 1
    'rmsprop_b': (False, True, 'rmsprop', 'RMSProp', dict(step_size=0.01)),
    'sgd_nob': (False, False, 'sgd', 'StochasticGradientDescent', dict(step_size=0.001, momentum_type='polyak', momentum=0.5)),
    'amsgrad_nob': (False, False, 'amsgrad', 'AMSGrad', dict(step_size=0.01)),
    'adamax_nob': (False, False, 'adamax', 'AdaMax', dict(step_size=0.01)),
    'adadelta_nob': (False, False, 'adadelta', 'AdaDelta', dict(step_size=1.)),
}
LEAVERS = [37, 30, 32, 32, 36]   # the oracle on 'adagrad_nob' with tol = 1.0: every class 'optimal', at these iterations


@pytest.fixture(scope='module')
def amd():
    from optiml_amd import _lib
    from optiml_amd.device import get_context
    _lib.load()
    get_context()


@functools.lru_cache(maxsize=None)
def _data():
    """(X, y, Y, K, x0): the blobs, their one-vs-rest labels (k x n, +-1), the oracle's Gram matrix and the start point; computed
    once and shared by the tests, which leave them unchanged."""
    from oracle import svm_oracle as so
    from optiml_amd.datasets import make_multiclass_blobs
    from optiml_amd.ml.svm.multiclass import binarize
    X, y = make_multiclass_blobs(N, D, K, seed=1)
    _, Y = binarize(y)
    return X, y, Y, so.gram('rbf', X), np.random.RandomState(1).uniform(size=N)


def _parts(name):
    """(a, lb, ub) selectors of a configuration: equality rows per class or None, lower bound, upper bound or None"""
    sq, reg = CONFIGS[name][:2]
    _, _, Y, _, _ = _data()
    return (None if reg else Y), np.zeros(N), (None if sq else np.ones(N) * C_)


@functools.lru_cache(maxsize=None)
def _oracle(name, epochs, tol):
    """The oracle's run of every class of a configuration (a tuple of its result dicts)."""
    from oracle import al_oracle as ao
    sq, reg, rule, _, kw = CONFIGS[name]
    _, _, Y, Kmat, x0 = _data()
    a, lb, ub = _parts(name)
    out = []
    for c in range(K):
        yy = np.outer(Y[c], Y[c])
        Q = Kmat * yy + (yy if reg else 0.) + (np.eye(N) / (2 * C_) if sq else 0.)
        al = ao.AugLag(Q, -np.ones(N), a=None if a is None else a[c], lb=lb, ub=ub, rho=1.)
        out.append(ao.minimize(al, x0, rule, epochs=epochs, tol=tol, **kw))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def _quad(name):
    """The shared panel of a configuration as `OneVsRestSVC` builds it (kept for the module: several solves run on it)."""
    from optiml_amd.opti import KernelQuadratic
    from optiml_amd.ml.svm.kernels import gaussian
    sq, reg = CONFIGS[name][:2]
    X, _, Y, _, _ = _data()
    return KernelQuadratic(X, -np.ones(N), 'svc', gaussian, y=Y[0], diag=1. / (2 * C_) if sq else 0., rank_one=reg)


def _prm(name, epochs, tol):
    from optiml_amd.opti.constrained import AugmentedLagrangianQuadratic
    from optiml_amd.opti.unconstrained import stochastic as st
    quad = _quad(name)
    al = AugmentedLagrangianQuadratic(primal=quad, lb=np.zeros(N), rho=1.)
    return getattr(st, CONFIGS[name][3])(f=al, x=np.zeros(N), epochs=epochs, tol=tol, **CONFIGS[name][4])._params()


def _solve(name, cols, epochs, tol, chunk=256):
    """The batched solve of the classes `cols` (in that order) of a configuration: solve_batched_al's per-column dicts."""
    from optiml_amd.ml.svm._batched import _DeviceALSolver, solve_batched_al
    _, _, Y, _, x0 = _data()
    a, lb, ub = _parts(name)
    cols = list(cols)
    solver = _DeviceALSolver(_quad(name).device_problem(), _prm(name, epochs, tol), np.tile(x0, (len(cols), 1)), Y=Y[cols],
                             a=None if a is None else a[cols], lb=lb, ub=ub)
    return solve_batched_al(solver, chunk=chunk)


def _same(a, b):
    """two column results of the batched solver with the same bits"""
    assert a['status'] == b['status'] and a['iter'] == b['iter']
    assert a['rows'].dtype == b['rows'].dtype and len(a['rows']) == len(b['rows'])
    for field in a['rows'].dtype.names:
        assert np.array_equal(a['rows'][field], b['rows'][field]), field
    for v in ('x', 'past_x', 'g', 'step', 'dual'):
        assert np.array_equal(a[v], b[v]), v


@pytest.mark.parametrize('name', sorted(CONFIGS))
def test_trajectories_against_the_oracle(amd, name):
    """100 epochs of every class in the batch of 5 against the oracle's run of that class."""
    res, ref = _solve(name, range(K), 100, 1e-4), _oracle(name, 100, 1e-4)
    for c in range(K):
        r, o = res[c], ref[c]
        print(name, c, r['status'], r['iter'], 'f', np.max(np.abs(r['rows']['f'] / o['f_hist'] - 1)),
              'pf', np.max(np.abs(r['rows']['r1'] / o['pf_hist'] - 1)), 'x', np.max(np.abs(r['x'] - o['x'])),
              'dual', np.max(np.abs(r['dual'] - o['dual_x'])), 'g', np.max(np.abs(r['g'] - o['g_x'])))
        assert r['status'] == o['status'] == 'stopped' and r['iter'] == o['iter'] == 99
        np.testing.assert_allclose(r['rows']['f'], o['f_hist'], rtol=1e-9, atol=1e-10)
        np.testing.assert_allclose(r['rows']['r1'], o['pf_hist'], rtol=1e-9, atol=1e-10)
        np.testing.assert_allclose(r['x'], o['x'], rtol=1e-6, atol=1e-9)
        np.testing.assert_allclose(r['dual'], o['dual_x'], rtol=1e-6, atol=1e-9)
        np.testing.assert_allclose(r['g'], o['g_x'], rtol=1e-6, atol=1e-8)


def test_leavers_and_batch_invariance(amd):
    """tol = 1.0: the classes stop at different iterations and leave the product one by one.  Every class has the oracle's count, and
    the same bits alone (k = 1), in the batch of 5 and in a permuted batch (other slots, another chunk of the panel stream)."""
    name = 'adagrad_nob'
    ref = _oracle(name, 200, 1.0)
    assert [o['iter'] for o in ref] == LEAVERS and all(o['status'] == 'optimal' for o in ref)
    batch = _solve(name, range(K), 200, 1.0)
    assert [r['iter'] for r in batch] == LEAVERS and all(r['status'] == 'optimal' for r in batch)
    for c in range(K):
        np.testing.assert_allclose(batch[c]['rows']['f'], ref[c]['f_hist'], rtol=1e-9, atol=1e-10)
        np.testing.assert_allclose(batch[c]['x'], ref[c]['x'], rtol=1e-6, atol=1e-9)
        np.testing.assert_allclose(batch[c]['dual'], ref[c]['dual_x'], rtol=1e-6, atol=1e-9)
        _same(_solve(name, [c], 200, 1.0)[0], batch[c])
    perm = [3, 0, 4, 2, 1]
    for slot, r in enumerate(_solve(name, perm, 200, 1.0)):
        _same(r, batch[perm[slot]])


@pytest.mark.parametrize('chunk', [1, 7])
def test_run_cutting(amd, chunk):
    """The same solve driven in runs of 1 and of 7 steps against runs of 256: every run ends in the batched flush, which closes the
    last iteration (and may stop a column, whose slot the next run's start-up prep hands on); records and final vectors identical."""
    name = 'adagrad_nob'
    whole, cut = _solve(name, range(K), 200, 1.0, chunk=256), _solve(name, range(K), 200, 1.0, chunk=chunk)
    assert [r['iter'] for r in cut] == LEAVERS
    for c in range(K):
        _same(cut[c], whole[c])


def _svc_kw(name, **over):
    from optiml_amd.ml.svm.kernels import gaussian
    from optiml_amd.ml.svm.losses import hinge, squared_hinge
    from optiml_amd.opti.unconstrained import stochastic as st
    sq, reg, _, cls, kw = CONFIGS[name]
    out = dict(loss=squared_hinge if sq else hinge, kernel=gaussian, C=C_, reg_intercept=reg, dual=True, optimizer=getattr(st, cls),
               learning_rate=kw['step_size'], max_iter=100, random_state=1)
    out.update({k: v for k, v in kw.items() if k != 'step_size'})
    out.update(over)
    return out


def _fit_counting(fit):
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter('always')
        out = fit()
    return out, sum('max_iter reached' in str(x.message) for x in w)


def _cmp_estimator(est, one, halves):
    """A batched fit's estimator against the single fit's, attribute by attribute."""
    a = one.alphas_ if halves == 1 else np.maximum(*np.split(one.alphas_, 2))
    assert np.min(np.abs(a - 1e-6)) > 1e-8   # no alpha of the single fit on the support threshold: the supports must be identical
    eo, oo = est.optimizer, one.optimizer
    print(type(oo).__name__, oo.status, oo.iter, 'loss', np.max(np.abs(np.array(est.train_loss_history) / one.train_loss_history - 1)),
          'x', np.max(np.abs(eo.x - oo.x)), 'dual', np.max(np.abs(est.obj.dual_x - one.obj.dual_x)), 'g', np.max(np.abs(eo.g_x - oo.g_x)),
          'b', abs(est.intercept_ - one.intercept_))
    assert (eo.status, eo.iter, eo.epoch) == (oo.status, oo.iter, oo.epoch)
    np.testing.assert_allclose(est.train_loss_history, one.train_loss_history, rtol=1e-9, atol=1e-10)
    np.testing.assert_allclose(eo.f_x, oo.f_x, rtol=1e-9, atol=1e-10)
    np.testing.assert_allclose(eo.primal_f_x, oo.primal_f_x, rtol=1e-9, atol=1e-10)
    assert eo.primal_f_x == est.train_loss_history[-1]
    for v in ('x', 'past_x', 'step'):
        np.testing.assert_allclose(getattr(eo, v), getattr(oo, v), rtol=1e-6, atol=1e-9, err_msg=v)
    np.testing.assert_allclose(eo.g_x, oo.g_x, rtol=1e-6, atol=1e-8)
    assert type(est.obj) is type(one.obj) and est.obj is eo.f
    np.testing.assert_allclose(est.obj.dual_x, one.obj.dual_x, rtol=1e-6, atol=1e-9)
    np.testing.assert_allclose(est.obj.past_dual_x, one.obj.past_dual_x, rtol=1e-6, atol=1e-9)
    # the per-column view of the shared panel is the column's own dual: its value and gradient at the final point
    f_own, g_own = est.obj.primal.function_jacobian(eo.x)
    f_one, g_one = one.obj.primal.function_jacobian(eo.x)
    np.testing.assert_allclose(f_own, f_one, rtol=1e-9, atol=1e-10)
    np.testing.assert_allclose(g_own, g_one, rtol=1e-6, atol=1e-8)
    assert est.alphas_ is eo.x
    np.testing.assert_allclose(est.alphas_, one.alphas_, rtol=1e-6, atol=1e-9)
    assert np.array_equal(est.support_, one.support_)
    assert np.array_equal(est.support_vectors_, one.support_vectors_)
    np.testing.assert_allclose(est.dual_coef_, one.dual_coef_, rtol=1e-6, atol=1e-9)
    np.testing.assert_allclose(est.intercept_, one.intercept_, rtol=1e-6, atol=1e-9)
    if hasattr(one, 'coef_'):   # the linear kernel
        np.testing.assert_allclose(est.coef_, one.coef_, rtol=1e-6, atol=1e-9)


@pytest.mark.parametrize('name,storage', [(name, 'f64') for name in sorted(CONFIGS)] + [('adagrad_nob', 'f32')])
def test_one_vs_rest_against_the_loop_of_single_fits(amd, name, storage):
    """OneVsRestSVC on the batched augmented-Lagrangian path against SVC.fit on every class's 0 / 1 labels.  'f32': both sides read the
    same fp32 panel, the tolerances are the same."""
    from optiml_amd.ml.svm import SVC, OneVsRestSVC
    X, y, Y, _, _ = _data()
    Xte = X[::7] + 0.05
    kw = _svc_kw(name, storage=storage)
    ovr, n_warn = _fit_counting(lambda: OneVsRestSVC(**kw).fit(X, y))
    assert ovr.batched_ and ovr.lagrangian_
    loop, n_warn_loop = _fit_counting(lambda: [SVC(**kw).fit(X, (Yc > 0).astype(int)) for Yc in Y])
    assert n_warn == n_warn_loop == K
    for est, one in zip(ovr.estimators_, loop):
        _cmp_estimator(est, one, 1)
    scores = np.stack([one.decision_function(Xte) for one in loop], axis=1)
    np.testing.assert_allclose(ovr.decision_function(Xte), scores, rtol=1e-6, atol=1e-8)
    assert np.array_equal(ovr.predict(Xte), ovr.classes_[np.argmax(scores, axis=1)])


def test_one_vs_rest_linear_kernel_sets_coef(amd):
    from optiml_amd.ml.svm import SVC, OneVsRestSVC
    from optiml_amd.ml.svm.kernels import linear
    X, y, Y, _, _ = _data()
    kw = _svc_kw('adagrad_nob', kernel=linear)
    ovr, _ = _fit_counting(lambda: OneVsRestSVC(**kw).fit(X, y))
    assert ovr.batched_ and ovr.lagrangian_
    loop, _ = _fit_counting(lambda: [SVC(**kw).fit(X, (Yc > 0).astype(int)) for Yc in Y])
    for est, one in zip(ovr.estimators_, loop):
        assert est.coef_.shape == one.coef_.shape == (D,)
        _cmp_estimator(est, one, 1)


@functools.lru_cache(maxsize=None)
def _targets():
    """X of datasets.make_regression and 5 smooth targets of it with noise (test_gpu_multioutput.py's recipe)"""
    from optiml_amd.datasets import make_regression
    X, _ = make_regression(N, D, seed=1)
    rs = np.random.RandomState(7)
    return X, np.tanh(X @ rs.standard_normal((D, K)) / np.sqrt(D) / 4) + 0.1 * rs.standard_normal((N, K))


@pytest.mark.parametrize('squared,reg', [(False, False), (True, True)])
def test_multi_output_against_the_loop_of_single_fits(amd, squared, reg):
    """MultiOutputSVR on the batched path (vectors of 2n; the product input x+ - x- by the prep kernel of every iteration) against
    SVR.fit on every target: epsilon-insensitive with the equality row [1; -1], squared epsilon-insensitive with K + 1."""
    from optiml_amd.ml.svm import SVR, MultiOutputSVR
    from optiml_amd.ml.svm.kernels import gaussian
    from optiml_amd.ml.svm.losses import epsilon_insensitive, squared_epsilon_insensitive
    from optiml_amd.opti.unconstrained.stochastic import AdaGrad
    X, T = _targets()
    Xte = X[::7] + 0.05
    kw = dict(loss=squared_epsilon_insensitive if squared else epsilon_insensitive, epsilon=0.1, kernel=gaussian, C=C_,
              reg_intercept=reg, dual=True, optimizer=AdaGrad, learning_rate=1., max_iter=100, random_state=1)
    mo, n_warn = _fit_counting(lambda: MultiOutputSVR(**kw).fit(X, T))
    assert mo.batched_ and mo.lagrangian_
    loop, n_warn_loop = _fit_counting(lambda: [SVR(**kw).fit(X, T[:, c]) for c in range(K)])
    assert n_warn == n_warn_loop
    for est, one in zip(mo.estimators_, loop):
        assert est.alphas_.shape == (2 * N,)
        _cmp_estimator(est, one, 2)
    np.testing.assert_allclose(mo.predict(Xte), np.stack([one.predict(Xte) for one in loop], axis=1), rtol=1e-6, atol=1e-8)


def test_nesterov_falls_back_to_the_loop(amd):
    """Nesterov momentum is not batched: the estimator runs the loop of single fits, bit for bit."""
    from optiml_amd.ml.svm import SVC, OneVsRestSVC
    X, y, Y, _, _ = _data()
    kw = _svc_kw('adam_sq_b', momentum_type='nesterov')
    ovr, _ = _fit_counting(lambda: OneVsRestSVC(**kw).fit(X, y))
    assert ovr.batched_ is False and ovr.lagrangian_ is False
    loop, _ = _fit_counting(lambda: [SVC(**kw).fit(X, (Yc > 0).astype(int)) for Yc in Y])
    for est, one in zip(ovr.estimators_, loop):
        assert np.array_equal(est.alphas_, one.alphas_) and est.intercept_ == one.intercept_
        assert np.array_equal(est.train_loss_history, one.train_loss_history)
        assert np.array_equal(est.obj.dual_x, one.obj.dual_x)


def test_size_case(amd):
    """n = 20 000 (79 tile rows, the last ragged), d = 32, k = 6 (a full and a half chunk), AdaGrad, 20 iterations: every class's
    primal-value history against SVC.fit on that class."""
    from optiml_amd.datasets import make_multiclass_blobs
    from optiml_amd.ml.svm import SVC, OneVsRestSVC
    from optiml_amd.ml.svm.multiclass import binarize
    X, y = make_multiclass_blobs(20000, 32, 6, seed=3)
    _, Y = binarize(y)
    kw = _svc_kw('adagrad_nob', max_iter=20)
    ovr, _ = _fit_counting(lambda: OneVsRestSVC(**kw).fit(X, y))
    assert ovr.batched_ and ovr.lagrangian_
    for est, Yc in zip(ovr.estimators_, Y):
        one, _ = _fit_counting(lambda: SVC(**kw).fit(X, (Yc > 0).astype(int)))
        assert len(est.train_loss_history) == len(one.train_loss_history) == 20
        print('n=20000', np.max(np.abs(np.array(est.train_loss_history) / one.train_loss_history - 1)))
        np.testing.assert_allclose(est.train_loss_history, one.train_loss_history, rtol=1e-9)
        one.obj.release()
