"""SVRGridSearchCV on the device: the batched SVR solver with one box per column (bq_msolver.hip: bq_msolver_create_svr_boxes), the
held-out scoring on the solver's state (bq_msolver_svr_heldout: msvr_coef_kernel, msvr_score_kernel) and the search, against the CPU
oracle, the host scoring path, the single-fold SVR and sklearn's GridSearchCV(SVR)."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U53 = 2.0 ** -53


@pytest.fixture(scope='module')
def amd():
    from optiml_amd import _lib
    from optiml_amd.device import get_context
    _lib.load()
    get_context()


@functools.lru_cache(maxsize=None)
def _data(n):
    """X of datasets.make_regression and a smooth target of it with noise (test_gpu_multioutput's); computed once and shared by the
    tests, which leave it unchanged."""
    from optiml_amd.datasets import make_regression
    X, _ = make_regression(n, 8, seed=1)
    rs = np.random.RandomState(7)
    y = np.tanh(X @ rs.standard_normal(8) / np.sqrt(8) / 4) + 0.1 * rs.standard_normal(n)
    return X, y


def _quad(X, storage='f64', kernel=None):
    from optiml_amd.opti import KernelQuadratic
    from optiml_amd.ml.svm.kernels import gaussian
    return KernelQuadratic(X, np.zeros(2 * X.shape[0]), 'svr', kernel or gaussian, storage=storage)


def _column(y, held, C, eps):
    """(q, ub) of one search column: ub = C on both halves of the training rows, 0 on both halves of the rows `held`"""
    n = len(y)
    ub = np.full(2 * n, float(C))
    ub[held] = 0.
    ub[n + held] = 0.
    return np.hstack((-y, y)) + eps, ub


def _solve(dev, kind, QL, UB, max_iter, t=0.0, x0=None, y=None, epsilons=None):
    """the columns' results; with y and epsilons every result also carries its `heldout` figures (b, n_sv, sse, n_held)"""
    from optiml_amd.ml.svm._batched import _DeviceSVRSolver, solve_batched
    held = []
    res = solve_batched(dev, kind, QL, UB, solver=_DeviceSVRSolver(dev, kind, QL, UB, 1e-6, max_iter, t, x0),
                        before_close=None if y is None else lambda s, _: held.extend(s.heldout(y, epsilons)))
    if held:
        for c, r in enumerate(res):
            r.update(b=held[0][c], n_sv=held[1][c], sse=held[2][c], n_held=held[3][c])
    return res


@pytest.mark.parametrize('kind,t', [('pg', 0.0), ('fw', 0.0), ('fw', 0.1)])
def test_held_out_box_is_the_training_fold_dual(amd, kind, t):
    """n = 600 (3 tile rows, a ragged last tile), ub = 0 on both halves of rows 200-399: 100 iterations against the oracle on
    svr_dual(K[tr][:, tr], y[tr], C, eps); both halves of the held-out rows stay exactly 0."""
    from optiml_amd import _lib
    from oracle import svm_oracle as so, bcqp_oracle as bo
    n, C_, eps = 600, 1.0, 0.1
    X, y = _data(n)
    held = np.arange(200, 400)
    tr = np.setdiff1d(np.arange(n), held)
    quad = _quad(X)
    q, ub = _column(y, held, C_, eps)
    res = _solve(quad.device_problem(), _lib.PG if kind == 'pg' else _lib.FW, q[None, :], ub[None, :], 100, t)[0]
    K = so.gram('rbf', X)
    Q, qt, ubt = so.svr_dual(K[np.ix_(tr, tr)], y[tr], C_, eps)
    ref = bo.projected_gradient(Q, qt, ubt, max_iter=100) if kind == 'pg' else bo.frank_wolfe(Q, qt, ubt, max_iter=100, t=t)
    assert res['status'] == ref['status'] and res['iter'] == ref['iter']
    np.testing.assert_allclose(res['rows']['f'], ref['f_hist'], rtol=1e-9)
    assert np.all(res['x'][held] == 0.) and np.all(res['x'][n + held] == 0.)
    assert np.any(res['x'][tr] != 0.) or np.any(res['x'][n + tr] != 0.)
    quad.release()


NO_SV = 5   # the column of _columns17 that ends without a support vector


@functools.lru_cache(maxsize=None)
def _columns17(n):
    """17 columns (two chunks of 16) on n rows: 3 interleaved folds x mixed (C, epsilon), with start points inside their boxes.
    Column NO_SV has an epsilon far above max |y| and starts at 0: its linear term is positive everywhere, 0 is its optimum and it
    has no support vector."""
    X, y = _data(n)
    rs = np.random.RandomState(11)
    idx = np.arange(n)
    cols = [(c % 3, (0.5, 1.0, 2.0)[(c // 3) % 3], (0.05, 0.1, 0.2)[c % 3 if c < 9 else (c + 1) % 3]) for c in range(17)]
    QL, UB, eps = [], [], []
    for c, (f, C_, e) in enumerate(cols):
        if c == NO_SV:
            e = 100.0 * float(np.abs(y).max())
        q, ub = _column(y, idx[idx % 3 == f], C_, e)
        QL.append(q)
        UB.append(ub)
        eps.append(e)
    QL, UB, eps = np.stack(QL), np.stack(UB), np.array(eps)
    x0 = UB * rs.uniform(size=UB.shape)
    x0[NO_SV] = 0.
    return X, y, QL, UB, eps, x0


@pytest.mark.parametrize('kind', ['pg', 'fw'])
def test_boxes_solve_is_batch_invariant(amd, kind):
    """Every column has the same bits (every record field, x, g) alone, in the batch of 17 and in the reversed batch."""
    from optiml_amd import _lib
    n, k = 600, 17
    X, y, QL, UB, eps, x0 = _columns17(n)
    quad = _quad(X)
    dev = quad.device_problem()
    dk = _lib.PG if kind == 'pg' else _lib.FW
    batch = _solve(dev, dk, QL, UB, 40, x0=x0)
    rev = _solve(dev, dk, QL[::-1].copy(), UB[::-1].copy(), 40, x0=x0[::-1].copy())
    assert any(r['iter'] == 40 for r in batch)
    for c in range(k):
        alone = _solve(dev, dk, QL[c:c + 1], UB[c:c + 1], 40, x0=x0[c:c + 1])[0]
        for other in (alone, rev[k - 1 - c]):
            assert other['status'] == batch[c]['status'] and other['iter'] == batch[c]['iter']
            for f in batch[c]['rows'].dtype.names:   # (the records hold NaN where a solver has no such figure)
                assert np.array_equal(other['rows'][f], batch[c]['rows'][f], equal_nan=True), f
            assert np.array_equal(other['x'], batch[c]['x']) and np.array_equal(other['g'], batch[c]['g'])
    quad.release()


def _check_against_host(dev, y, UB, eps, res):
    """bq_msolver_svr_heldout's figures of every column against the host path on the downloaded x: W as fitted_svr forms it, one
    wide product, svr_intercept, NumPy sums.  Both sides sum the same terms (the same u bits) in different orders: a sum of m <= n
    terms t_i in any order is within (m - 1) 2^-53 sum |t_i| of the exact one, so two orders differ by less than
    2 n 2^-53 sum |t_i|; twice that covers the few further roundings (the subtraction of epsilon, the division, the squares)."""
    from optiml_amd.ml.svm._batched import _gram_matmat, svr_intercept
    n = len(y)
    k = len(res)
    W = np.zeros((k, n))
    svs = []
    for j, r in enumerate(res):
        xp, xn = np.split(r['x'], 2)
        sv = np.logical_or(xp > 1e-6, xn > 1e-6)
        W[j][sv] = xp[sv] - xn[sv]
        svs.append(sv)
    U = _gram_matmat(dev, W, wide=True)
    for j, r in enumerate(res):
        sv = svs[j]
        te = (UB[j][:n] == 0) & (UB[j][n:] == 0)
        assert r['n_sv'] == sv.sum() and r['n_held'] == te.sum() and te.sum() > 0
        if not sv.any():
            assert np.isnan(r['b']) and np.isnan(r['sse'])
            continue
        b = svr_intercept(y, U[j], sv, eps[j])
        bound_b = 4 * n * U53 * np.abs(y[sv] - U[j][sv]).sum() / sv.sum()
        print('column %d: |b_dev - b_host| = %.3e (bound %.3e)' % (j, abs(r['b'] - b), bound_b))
        assert abs(r['b'] - b) <= bound_b
        res_te = y[te] - (U[j][te] + b)
        sse = float((res_te ** 2).sum())
        bound_sse = 4 * n * U53 * sse + 2 * abs(r['b'] - b) * np.abs(res_te).sum()
        print('column %d: |sse_dev - sse_host| = %.3e (bound %.3e)' % (j, abs(r['sse'] - sse), bound_sse))
        assert abs(r['sse'] - sse) <= bound_sse


@pytest.mark.parametrize('kind', ['pg', 'fw'])
def test_device_scoring_against_the_host_path(amd, kind):
    """The 17 columns at n = 600: intercepts, support counts, held-out squared errors and counts against the host path; the same
    figures, bit for bit, for every column solved and scored alone; the column without a support vector scores NaN and leaves the
    others as they are."""
    from optiml_amd import _lib
    n, k = 600, 17
    X, y, QL, UB, eps, x0 = _columns17(n)
    quad = _quad(X)
    dev = quad.device_problem()
    dk = _lib.PG if kind == 'pg' else _lib.FW
    batch = _solve(dev, dk, QL, UB, 40, x0=x0, y=y, epsilons=eps)
    _check_against_host(dev, y, UB, eps, batch)
    assert batch[NO_SV]['n_sv'] == 0 and np.isnan(batch[NO_SV]['b']) and np.isnan(batch[NO_SV]['sse'])
    assert batch[NO_SV]['n_held'] == 200
    assert sum(r['n_sv'] > 0 and np.isfinite(r['b']) and np.isfinite(r['sse']) for r in batch) == k - 1
    for c in range(k):
        alone = _solve(dev, dk, QL[c:c + 1], UB[c:c + 1], 40, x0=x0[c:c + 1], y=y, epsilons=eps[c:c + 1])[0]
        for key in ('b', 'n_sv', 'sse', 'n_held'):
            assert np.array_equal(alone[key], batch[c][key], equal_nan=True), (c, key)
    quad.release()


@pytest.mark.parametrize('n', [256, 257])
def test_device_scoring_one_column_at_the_tile_edge(amd, n):
    """One column on exactly one tile and on one row more (a second tile row of one row), a third of the rows held out."""
    from optiml_amd import _lib
    X, y = _data(n)
    quad = _quad(X)
    dev = quad.device_problem()
    idx = np.arange(n)
    q, ub = _column(y, idx[idx % 3 == 1], 1.0, 0.1)
    res = _solve(dev, _lib.PG, q[None, :], ub[None, :], 40, y=y, epsilons=np.array([0.1]))
    assert res[0]['n_sv'] > 0
    _check_against_host(dev, y, ub[None, :], np.array([0.1]), res)
    quad.release()


def test_argument_checks(amd):
    from optiml_amd import _lib
    from optiml_amd.ml.svm._batched import _DeviceSVRSolver
    n = 300
    X, y = _data(n)
    quad = _quad(X)
    dev = quad.device_problem()
    q, ub = _column(y, np.arange(100), 1.0, 0.1)
    bad = ub.copy()
    bad[n + 150] = 0.   # one half of a training row
    with pytest.raises(_lib.BcqpError) as e:
        _DeviceSVRSolver(dev, _lib.PG, q[None, :], bad[None, :], 1e-6, 10)
    assert e.value.code == _lib.ERR_BADARG
    bad = ub.copy()
    bad[7] = 1.   # one half of a held-out row
    with pytest.raises(_lib.BcqpError) as e:
        _DeviceSVRSolver(dev, _lib.PG, q[None, :], bad[None, :], 1e-6, 10)
    assert e.value.code == _lib.ERR_BADARG
    shared = _DeviceSVRSolver(dev, _lib.PG, q[None, :], np.ones(2 * n), 1e-6, 10)   # bq_msolver_create_svr: one box for all
    shared.run(5)
    with pytest.raises(_lib.BcqpError) as e:
        shared.heldout(y, [0.1])
    assert e.value.code == _lib.ERR_BADARG
    shared.close()
    quad.release()


def _search_case(case):
    from optiml_amd.ml.svm.kernels import GaussianKernel, LinearKernel
    from optiml_amd.ml.svm.losses import epsilon_insensitive
    from optiml_amd.opti.constrained import FrankWolfe, ProjectedGradient
    kw = dict(loss=epsilon_insensitive, dual=True, reg_intercept=True, optimizer=ProjectedGradient, max_iter=100)
    grid = {'C': [0.5, 2], 'epsilon': [0.05, 0.2]}
    return {
        'gauss-num-pg': (dict(kw, kernel=GaussianKernel(gamma=0.1)), grid),
        'gauss-num-pg-f32': (dict(kw, kernel=GaussianKernel(gamma=0.1), storage='f32'), grid),
        'gauss-scale-fw': (dict(kw, kernel=GaussianKernel(gamma='scale'), optimizer=FrankWolfe), grid),
        'kernels-pg': (kw, dict(grid, kernel=[GaussianKernel(gamma=0.1), LinearKernel()])),
    }[case]


def _compare_results(ours, ref, n_splits):
    for i in range(n_splits):
        key = 'split%d_test_score' % i
        print(key, np.max(np.abs(ours.cv_results_[key] - ref.cv_results_[key])))
        np.testing.assert_allclose(ours.cv_results_[key], ref.cv_results_[key], rtol=1e-9, atol=1e-9)
    for key in ('mean_test_score', 'std_test_score'):
        np.testing.assert_allclose(ours.cv_results_[key], ref.cv_results_[key], rtol=1e-9, atol=1e-9)
    top = np.sort(ref.cv_results_['mean_test_score'])[::-1]
    if top[0] - top[1] > 1e-6:
        np.testing.assert_array_equal(ours.cv_results_['rank_test_score'], ref.cv_results_['rank_test_score'])
        assert ours.best_index_ == ref.best_index_ and ours.best_params_ == ref.best_params_
        np.testing.assert_allclose(ours.best_score_, ref.best_score_, rtol=1e-9, atol=1e-9)


@pytest.mark.parametrize('case', ['gauss-num-pg', 'gauss-num-pg-f32', 'gauss-scale-fw', 'kernels-pg'])
def test_search_equals_grid_search_cv(amd, case):
    pytest.importorskip('sklearn')
    from sklearn.model_selection import GridSearchCV, KFold
    from optiml_amd.ml.svm import SVR, SVRGridSearchCV
    kw, grid = _search_case(case)
    X, y = _data(400)
    ours = SVRGridSearchCV(SVR(**kw), grid, cv=3).fit(X, y)   # an int: KFold(3)
    assert ours.batched_ is True and ours.n_splits_ == 3
    ref = GridSearchCV(SVR(**kw), grid, cv=KFold(3)).fit(X, y)
    _compare_results(ours, ref, 3)
    nc = len(ours.cv_results_['params'])
    assert ours.cv_results_['params'] == ref.cv_results_['params']
    assert ours.n_iter_.shape == ours.status_.shape == (nc, 3)
    assert (ours.n_iter_ > 0).all() and set(ours.status_.ravel()) <= {'optimal', 'stopped'}
    Xte = _data(600)[0][400:]
    np.testing.assert_allclose(ours.best_estimator_.predict(Xte), ref.best_estimator_.predict(Xte), rtol=1e-9)
    np.testing.assert_allclose(ours.predict(Xte), ours.best_estimator_.predict(Xte), rtol=0)
    assert ours.score(X, y) == ours.best_estimator_.score(X, y)


@pytest.mark.parametrize('which', ['active-set', 'other-key'])
def test_fallback_equals_grid_search_cv(amd, which):
    pytest.importorskip('sklearn')
    from sklearn.model_selection import GridSearchCV, KFold
    from optiml_amd.ml.svm import SVR, SVRGridSearchCV
    from optiml_amd.ml.svm.kernels import GaussianKernel
    from optiml_amd.ml.svm.losses import epsilon_insensitive
    from optiml_amd.opti.constrained import ActiveSet, ProjectedGradient
    kw = dict(loss=epsilon_insensitive, dual=True, reg_intercept=True, optimizer=ProjectedGradient, max_iter=60,
              kernel=GaussianKernel(gamma=0.1))
    grid = {'C': [0.5, 2.0], 'epsilon': [0.05, 0.2]}
    if which == 'active-set':
        kw['optimizer'] = ActiveSet
    else:
        grid = {'C': [0.5, 2.0], 'max_iter': [20, 40]}
    X, y = _data(150)
    ours = SVRGridSearchCV(SVR(**kw), grid, cv=KFold(3)).fit(X, y)
    assert ours.batched_ is False
    ref = GridSearchCV(SVR(**kw), grid, cv=KFold(3)).fit(X, y)
    for i in range(3):
        assert np.array_equal(ours.cv_results_['split%d_test_score' % i], ref.cv_results_['split%d_test_score' % i])
    assert ours.best_params_ == ref.best_params_ and ours.n_iter_.shape == (4, 3)


def test_size_case_column_follows_svr_fit(amd):
    """n = 5000 (20 tile rows, several strips), 5 folds x 2 C x 2 epsilon, 20 PG iterations: the (fold 0, first candidate) column's
    objective history against SVR.fit on the fold's training rows, and its device R^2 against that estimator's score."""
    from optiml_amd import _lib
    from optiml_amd.ml.svm import SVR
    from optiml_amd.ml.svm.kernels import GaussianKernel
    from optiml_amd.ml.svm.losses import epsilon_insensitive
    from optiml_amd.ml.svm.model_selection import parameter_grid, plan_svr_columns, r2_from_sse
    n = 5000
    X, y = _data(n)
    idx = np.arange(n)
    splits = [(idx[idx % 5 != f], idx[idx % 5 == f]) for f in range(5)]
    kernel = GaussianKernel(gamma=0.1)
    cands = parameter_grid({'C': [1.0, 4.0], 'epsilon': [0.1, 0.3]})
    g, = plan_svr_columns(X, y, splits, cands, 1.0, 0.1, kernel)
    assert len(g['cols']) == 20
    quad = _quad(X, 'f64', g['kernel'])
    res = _solve(quad.device_problem(), _lib.PG, g['QL'], g['UB'], 20, y=y, epsilons=[c[3] for c in g['cols']])
    quad.release()
    j = g['cols'].index((0, 0, 1.0, 0.1))
    tr, te = splits[0]
    svr = SVR(loss=epsilon_insensitive, dual=True, reg_intercept=True, kernel=kernel, C=1.0, epsilon=0.1, max_iter=20).fit(X[tr], y[tr])
    np.testing.assert_allclose(res[j]['rows']['f'], svr.train_loss_history, rtol=1e-10)
    assert res[j]['iter'] == svr.optimizer.iter and res[j]['status'] == svr.optimizer.status
    assert res[j]['n_held'] == len(te)
    np.testing.assert_allclose(r2_from_sse(res[j]['sse'], y[te]), svr.score(X[te], y[te]), rtol=1e-9)


def test_a_failed_solve_releases_the_panel(amd, monkeypatch):
    """A batched solve that raises leaves no panel behind: `fit` raises the solve's error, and the one panel built so far was
    released once on the way out (n = 120, two candidates, two folds; the error is a Python exception before any launch)."""
    from optiml_amd.ml.svm import SVR, SVRGridSearchCV, model_selection
    from optiml_amd.opti import KernelQuadratic
    kw, _ = _search_case('gauss-num-pg')
    X, y = _data(120)
    calls, released = [], []

    def failing_solve(*args, **kwargs):
        calls.append(1)
        raise RuntimeError('the solve failed')

    release = KernelQuadratic.release
    monkeypatch.setattr(model_selection, 'solve_batched', failing_solve)
    monkeypatch.setattr(KernelQuadratic, 'release', lambda self: (released.append(self), release(self))[1])
    search = SVRGridSearchCV(SVR(**kw), {'C': [0.5, 2.0]}, cv=2)
    with pytest.raises(RuntimeError, match='the solve failed'):
        search.fit(X, y)
    assert len(calls) == 1 and len(released) == 1
