"""MultiOutputSVR on the device: the batched SVR start-up and update kernels (bq_msolver.hip: bq_msolver_create_svr), the batched
ProjectedGradient / FrankWolfe iteration on vectors of 2n and the estimator, against the CPU oracle, the single-target path and
sklearn's MultiOutputRegressor(SVR)."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

C_, EPS = 1.0, 0.1


@pytest.fixture(scope='module')
def amd():
    from optiml_amd import _lib
    from optiml_amd.device import get_context
    _lib.load()
    get_context()


@functools.lru_cache(maxsize=None)
def _data(n, k):
    """X of datasets.make_regression and k smooth targets of it with noise; computed once and shared by the tests, which leave it
    unchanged."""
    from optiml_amd.datasets import make_regression
    X, _ = make_regression(n, 8, seed=1)
    rs = np.random.RandomState(7)
    Y = np.tanh(X @ rs.standard_normal((8, k)) / np.sqrt(8) / 4) + 0.1 * rs.standard_normal((n, k))
    return X, Y


def _quad(X, storage='f64'):
    from optiml_amd.opti import KernelQuadratic
    from optiml_amd.ml.svm.kernels import gaussian
    return KernelQuadratic(X, np.zeros(2 * X.shape[0]), 'svr', gaussian, storage=storage)


def _linear_terms(Y):
    """k x 2n: row c is SVR.fit's q of target c"""
    return np.hstack((-Y.T, Y.T)) + EPS


def _solve(dev, kind, QL, max_iter, t=0.0, x0=None):
    from optiml_amd.ml.svm._batched import _DeviceSVRSolver, solve_batched
    ub = np.ones(QL.shape[1]) * C_
    return solve_batched(dev, kind, QL, ub, solver=_DeviceSVRSolver(dev, kind, QL, ub, 1e-6, max_iter, t, x0))


@pytest.mark.parametrize('storage', ['f64', 'f32'])
def test_start_product_both_halves(amd, storage):
    """g_c = Q x0_c + q_c after the start-up of a batched solve, Q = [[K, -K], [-K, K]] + ee': 5 targets (a ragged second chunk of
    4) with their own start points, n = 1037 (5 tile rows, ragged last tile)."""
    from optiml_amd import _lib
    from optiml_amd.ml.svm._batched import _DeviceSVRSolver
    from oracle import svm_oracle as so
    n, k = 1037, 5
    X, Y = _data(n, k)
    quad = _quad(X, storage)
    K = so.gram('rbf', X)
    if storage == 'f32':
        K = quad.gram()   # the stored panel: fp32-rounded on the device
        np.testing.assert_allclose(K, so.gram('rbf', X), rtol=0, atol=1e-6)
    QL = _linear_terms(Y)
    x0 = np.random.RandomState(6).uniform(size=(k, 2 * n)) * C_
    s = _DeviceSVRSolver(quad.device_problem(), _lib.PG, QL, np.ones(2 * n) * C_, 1e-6, 10, 0.0, x0)
    s.run(1)
    for c in range(k):
        Q, q, _ = so.svr_dual(K, Y[:, c], C_, EPS)
        assert np.array_equal(q, QL[c])
        g = s.get(c, _lib.GET_G_NOW)
        assert g.shape == (2 * n,)
        np.testing.assert_allclose(g, Q @ x0[c] + q, rtol=1e-12, atol=1e-12 * 2 * n)
    s.close()
    quad.release()


@pytest.mark.parametrize('kind,t', [('pg', 0.0), ('fw', 0.0), ('fw', 0.1)])
def test_batched_trajectories_against_oracle(amd, kind, t):
    """n = 600, 3 targets, RBF: the first 100 iterations of every target against the oracle's solver on svr_dual(K, y_c, C, eps)."""
    from optiml_amd import _lib
    from oracle import svm_oracle as so, bcqp_oracle as bo
    X, Y = _data(600, 3)
    quad = _quad(X)
    K = so.gram('rbf', X)
    res = _solve(quad.device_problem(), _lib.PG if kind == 'pg' else _lib.FW, _linear_terms(Y), 100, t)
    for c in range(3):
        Q, q, ub = so.svr_dual(K, Y[:, c], C_, EPS)
        ref = bo.projected_gradient(Q, q, ub, max_iter=100) if kind == 'pg' else bo.frank_wolfe(Q, q, ub, max_iter=100, t=t)
        assert res[c]['status'] == ref['status'] and res[c]['iter'] == ref['iter']
        np.testing.assert_allclose(res[c]['rows']['f'], ref['f_hist'], rtol=1e-9)
    quad.release()


@functools.lru_cache(maxsize=None)
def _leaver_start():
    """(K, the oracle's interior-point solution of target 0) for n = 300, k = 4"""
    from oracle import svm_oracle as so, bcqp_oracle as bo
    X, Y = _data(300, 4)
    K = so.gram('rbf', X)
    Q, q, ub = so.svr_dual(K, Y[:, 0], C_, EPS)
    ip = bo.interior_point(Q, q, ub)
    assert ip['status'] == 'optimal'
    return K, ip['x']


@pytest.mark.parametrize('kind', ['pg', 'fw'])
def test_batched_solve_is_batch_invariant_with_a_leaver(amd, kind):
    """Target 0 starts at the interior-point solution of its dual, stops ('optimal') long before the others reach max_iter and
    leaves the batch; every target still has the same bits (records, x, g) alone, in the batch and in the reversed batch.
    The precondition is held on the oracle first: started there, its PG stops 'optimal' after 4 iterations and its FW after 0
    (measured on the CPU at n = 300; at most 4 is asserted), and the other targets run to max_iter."""
    from optiml_amd import _lib
    from oracle import svm_oracle as so, bcqp_oracle as bo
    n, k = 300, 4
    X, Y = _data(n, k)
    K, xip = _leaver_start()
    solve = bo.projected_gradient if kind == 'pg' else bo.frank_wolfe
    Q, q, ub = so.svr_dual(K, Y[:, 0], C_, EPS)
    ref = solve(Q, q, ub, x0=xip, max_iter=150)
    assert ref['status'] == 'optimal' and ref['iter'] <= 4
    for c in (1, 2, 3):
        Q, q, ub = so.svr_dual(K, Y[:, c], C_, EPS)
        assert solve(Q, q, ub, max_iter=150)['status'] == 'stopped'
    quad = _quad(X)
    dev = quad.device_problem()
    dk = _lib.PG if kind == 'pg' else _lib.FW
    QL = _linear_terms(Y)
    x0 = np.full((k, 2 * n), C_ / 2)
    x0[0] = xip
    batch = _solve(dev, dk, QL, 150, x0=x0)
    assert batch[0]['status'] == 'optimal' and batch[0]['iter'] < 50
    assert all(batch[c]['status'] == 'stopped' and batch[c]['iter'] == 150 for c in (1, 2, 3))
    rev = _solve(dev, dk, QL[::-1].copy(), 150, x0=x0[::-1].copy())   # other slots, other chunk positions
    for c in range(k):
        alone = _solve(dev, dk, QL[c:c + 1], 150, x0=x0[c:c + 1])[0]
        for other in (alone, rev[k - 1 - c]):
            assert other['status'] == batch[c]['status'] and other['iter'] == batch[c]['iter']
            for f in batch[c]['rows'].dtype.names:   # (the records hold NaN where a solver has no such figure)
                assert np.array_equal(other['rows'][f], batch[c]['rows'][f], equal_nan=True), f
            assert np.array_equal(other['x'], batch[c]['x']) and np.array_equal(other['g'], batch[c]['g'])
    quad.release()


def _kernels():
    from optiml_amd.ml.svm.kernels import gaussian, linear, poly
    return {'gaussian': gaussian, 'poly': poly, 'linear': linear}


def _kw(kernel='gaussian', opt='pg', **more):
    from optiml_amd.ml.svm.losses import epsilon_insensitive
    from optiml_amd.opti.constrained import FrankWolfe, ProjectedGradient
    kw = dict(loss=epsilon_insensitive, epsilon=EPS, kernel=_kernels()[kernel], C=C_, reg_intercept=True, dual=True, max_iter=100,
              optimizer=ProjectedGradient if opt == 'pg' else FrankWolfe)
    kw.update(more)
    return kw


def _compare(ours, ref, Xte):
    """the tolerances of test_gpu_multiclass._compare"""
    assert len(ours.estimators_) == len(ref.estimators_)
    for a, b in zip(ours.estimators_, ref.estimators_):
        # support_ equality is a condition on the inputs: no alpha of the reference within a decade of the 1e-6 threshold
        assert not ((b.alphas_ > 1e-7) & (b.alphas_ < 1e-5)).any()
        np.testing.assert_allclose(a.alphas_, b.alphas_, rtol=1e-9, atol=1e-12 * C_)
        assert np.array_equal(a.support_, b.support_)
        assert np.array_equal(a.support_vectors_, b.support_vectors_)
        np.testing.assert_allclose(a.dual_coef_, b.dual_coef_, rtol=1e-9, atol=1e-12 * C_)
        np.testing.assert_allclose(a.intercept_, b.intercept_, rtol=1e-9, atol=1e-12)
        np.testing.assert_allclose(a.train_loss_history, b.train_loss_history, rtol=1e-9)
        assert a.optimizer.iter == b.optimizer.iter and a.optimizer.status == b.optimizer.status
        np.testing.assert_allclose(a.optimizer.f_x, b.optimizer.f_x, rtol=1e-9)
        # the optimizer's function is the target's own dual, as after SVR.fit: its value and gradient at the result are the solver's
        np.testing.assert_allclose(a.optimizer.f.function(a.alphas_), a.optimizer.f_x, rtol=1e-9)
        np.testing.assert_allclose(a.optimizer.f.jacobian(a.alphas_), a.optimizer.g_x, rtol=1e-9, atol=1e-9)
        np.testing.assert_allclose(b.optimizer.f.function(b.alphas_), b.optimizer.f_x, rtol=1e-9)
        np.testing.assert_allclose(a.predict(Xte), b.predict(Xte), rtol=1e-9, atol=1e-9)
        if hasattr(b, 'coef_') and np.size(b.coef_):
            np.testing.assert_allclose(a.coef_, b.coef_, rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(ours.predict(Xte), ref.predict(Xte), rtol=1e-9, atol=1e-9)


@pytest.mark.parametrize('kernel', ['gaussian', 'poly', 'linear'])
@pytest.mark.parametrize('opt', ['pg', 'fw'])
def test_estimator_equals_multi_output_wrapper(amd, kernel, opt):
    pytest.importorskip('sklearn')
    from sklearn.multioutput import MultiOutputRegressor
    from optiml_amd.ml.svm import SVR, MultiOutputSVR
    X, Y = _data(400, 3)
    Xtr, Xte, Ytr, Yte = X[:300], X[300:], Y[:300], Y[300:]
    kw = _kw(kernel, opt)
    ours = MultiOutputSVR(**kw).fit(Xtr, Ytr)
    assert ours.batched_ is True
    ref = MultiOutputRegressor(SVR(**kw)).fit(Xtr, Ytr)
    _compare(ours, ref, Xte)
    assert ours.predict(Xte).shape == (100, 3)
    np.testing.assert_allclose(ours.score(Xte, Yte), ref.score(Xte, Yte), rtol=1e-9, atol=1e-9)


def test_one_target(amd):
    pytest.importorskip('sklearn')
    from sklearn.multioutput import MultiOutputRegressor
    from optiml_amd.ml.svm import SVR, MultiOutputSVR
    X, Y = _data(400, 3)
    Xtr, Xte, Ytr = X[:300], X[300:], Y[:300, :1]
    kw = _kw()
    ours = MultiOutputSVR(**kw).fit(Xtr, Ytr)
    ref = MultiOutputRegressor(SVR(**kw)).fit(Xtr, Ytr)
    assert ours.batched_ is True and len(ours.estimators_) == 1 and ours.predict(Xte).shape == (100, 1)
    _compare(ours, ref, Xte)


@pytest.mark.parametrize('opt', ['as', 'ip', 'smo'])
def test_fallback_optimizers_equal_the_wrapper(amd, opt):
    pytest.importorskip('sklearn')
    from sklearn.multioutput import MultiOutputRegressor
    from optiml_amd.ml.svm import SVR, MultiOutputSVR
    from optiml_amd.opti.constrained import ActiveSet, InteriorPoint
    X, Y = _data(400, 3)
    Xtr, Xte, Ytr = X[:300], X[300:], Y[:300]
    kw = _kw(optimizer='smo', reg_intercept=False) if opt == 'smo' else _kw(optimizer=ActiveSet if opt == 'as' else InteriorPoint)
    ours = MultiOutputSVR(**kw).fit(Xtr, Ytr)
    assert ours.batched_ is False
    ref = MultiOutputRegressor(SVR(**kw)).fit(Xtr, Ytr)
    assert len(ours.estimators_) == len(ref.estimators_) == 3
    for a, b in zip(ours.estimators_, ref.estimators_):
        assert np.array_equal(a.alphas_, b.alphas_) and a.intercept_ == b.intercept_
    assert np.array_equal(ours.predict(Xte), ref.predict(Xte))


def test_size_case_against_single_target_svr(amd):
    """n = 5000 (20 tile rows, several strips), k = 5, 20 PG iterations: every target's objective history against SVR on that
    target alone."""
    from optiml_amd.ml.svm import SVR, MultiOutputSVR
    X, Y = _data(5000, 5)
    kw = _kw(max_iter=20)
    est = MultiOutputSVR(**kw).fit(X, Y)
    assert est.batched_ is True
    for c in range(5):
        one = SVR(**kw).fit(X, Y[:, c])
        ours, ref = np.array(est.estimators_[c].train_loss_history), np.array(one.train_loss_history)
        print('target %d: largest relative deviation %.3e' % (c, np.max(np.abs(ours / ref - 1))))
        np.testing.assert_allclose(est.estimators_[c].train_loss_history, one.train_loss_history, rtol=1e-12)
        assert est.estimators_[c].optimizer.status == one.optimizer.status == 'stopped'
