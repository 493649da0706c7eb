"""SVCGridSearchCV on the device: the 16-column MFMA panel product (bq_symmw.hip), the batched solver with one box per column
(bq_msolver_create_boxes) and the search, against NumPy, the 4-column product, the CPU oracle and sklearn's GridSearchCV(SVC)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def amd():
    from optiml_amd import _lib
    from optiml_amd.device import get_context
    _lib.load()
    get_context()


def _quad(X, storage='f64', kernel=None):
    from optiml_amd.opti import KernelQuadratic
    from optiml_amd.ml.svm.kernels import gaussian
    n = X.shape[0]
    return KernelQuadratic(X, -np.ones(n), 'svc', kernel or gaussian, y=np.ones(n), storage=storage)


def _wide(quad, W):
    from optiml_amd.ml.svm.multiclass import _gram_matmat
    return _gram_matmat(quad.device_problem(), W, wide=True)


def _blobs(n, k, d=8, seed=1):
    from optiml_amd.datasets import make_multiclass_blobs
    return make_multiclass_blobs(n, d, k, seed=seed)


@pytest.mark.parametrize('storage', ['f64', 'f32'])
@pytest.mark.parametrize('n', [2, 255, 256, 257, 1000, 4099])   # n = 1: KernelQuadratic rejects it ('Q is too small')
def test_wide_product_against_numpy(amd, n, storage):
    """K W for k in {1, 15, 16, 17, 40} (a ragged second and third chunk of 16) against NumPy on the stored panel."""
    X = np.random.RandomState(n).standard_normal((n, 5))
    quad = _quad(X, storage)
    K = quad.gram()
    rs = np.random.RandomState(n + 1)
    for k in (1, 15, 16, 17, 40):
        W = rs.standard_normal((k, n))
        np.testing.assert_allclose(_wide(quad, W), W @ K, rtol=1e-12, atol=1e-13 * np.abs(W).sum(axis=1).max())
    quad.release()


@pytest.mark.parametrize('n', [300, 777])
def test_wide_product_exact_on_small_integers(amd, n):
    """Linear kernel on small-integer data and small-integer W: every product and sum is exact, so the result equals the integer
    product bit for bit — any wrong lane map of the MFMA's A, B or C/D fragments (rows, k or slots swapped) shows here."""
    from optiml_amd.ml.svm.kernels import linear
    rs = np.random.RandomState(n)
    Xi = rs.randint(-3, 4, size=(n, 3))
    Wi = rs.randint(-4, 5, size=(40, n))
    quad = _quad(Xi.astype(float), 'f64', linear)
    want = (Wi @ (Xi @ Xi.T)).astype(float)
    assert np.array_equal(_wide(quad, Wi.astype(float)), want)
    quad.release()


def test_wide_product_against_four_column_product(amd):
    from optiml_amd.ml.svm.multiclass import _gram_matmat
    X, _ = _blobs(20000, 3, d=16)
    quad = _quad(X)
    W = np.random.RandomState(2).standard_normal((17, 20000))
    ref = _gram_matmat(quad.device_problem(), W)
    np.testing.assert_allclose(_wide(quad, W), ref, rtol=1e-12, atol=1e-12 * np.abs(W).sum(axis=1).max())
    quad.release()


def test_wide_product_batch_invariance(amd):
    """Column c has the same bits alone, in batches of 16, 17 and 40, at other positions, and on a second run."""
    X, _ = _blobs(1037, 3)
    quad = _quad(X)
    W = np.random.RandomState(4).standard_normal((40, 1037))
    full = _wide(quad, W)
    assert np.array_equal(_wide(quad, W), full)
    perm = np.random.RandomState(5).permutation(40)
    permuted = _wide(quad, W[perm])
    for c in (0, 7, 16, 33, 39):
        assert np.array_equal(_wide(quad, W[c:c + 1])[0], full[c])
        assert np.array_equal(permuted[np.where(perm == c)[0][0]], full[c])
        for width in (16, 17):
            lo = min(c, 40 - width)
            assert np.array_equal(_wide(quad, W[lo:lo + width])[c - lo], full[c])
    quad.release()


def _oracle_pg_optimum(Q, q, ub):
    from oracle import bcqp_oracle as bo
    r = bo.projected_gradient(Q, q, ub, max_iter=5000)
    assert r['status'] == 'optimal'
    return r['x']


def test_boxes_solve_is_batch_invariant(amd):
    """20 columns with their own boxes; one starts at its optimum and stops early (compaction).  Every column has the same bits
    alone, in the batch, in a reversed batch and on a second run."""
    from optiml_amd import _lib
    from optiml_amd.ml.svm.multiclass import solve_batched
    from oracle import svm_oracle as so
    n = 600
    X, y = _blobs(n, 4)
    quad = _quad(X)
    dev = quad.device_problem()
    K = quad.gram()
    rs = np.random.RandomState(8)
    Y = np.stack([np.where(y == c % 4, 1., -1.) for c in range(20)])
    UB = np.stack([np.where(rs.uniform(size=n) < 0.8, 0.5 + c / 4, 0.) for c in range(20)])
    x0 = UB / 2
    tr = UB[3] > 0
    Q, q, _ = so.svc_dual(K, Y[3], 1.0)
    x0[3] = 0.
    x0[3][tr] = _oracle_pg_optimum(Q[np.ix_(tr, tr)], q[tr], UB[3][tr])
    batch = solve_batched(dev, _lib.PG, Y, UB, max_iter=120, x0=x0)
    assert batch[3]['status'] == 'optimal' and batch[3]['iter'] < 50
    again = solve_batched(dev, _lib.PG, Y, UB, max_iter=120, x0=x0)
    rev = solve_batched(dev, _lib.PG, Y[::-1].copy(), UB[::-1].copy(), max_iter=120, x0=x0[::-1].copy())
    for c in (0, 3, 9, 19):
        alone = solve_batched(dev, _lib.PG, Y[c:c + 1], UB[c:c + 1], max_iter=120, x0=x0[c:c + 1])[0]
        for other in (alone, again[c], rev[19 - c]):
            assert other['status'] == batch[c]['status'] and other['iter'] == batch[c]['iter']
            assert np.array_equal(other['rows']['f'], batch[c]['rows']['f'])
            assert np.array_equal(other['x'], batch[c]['x']) and np.array_equal(other['g'], batch[c]['g'])
    quad.release()


@pytest.mark.parametrize('kind,t', [('pg', 0.0), ('fw', 0.0), ('fw', 0.1)])
def test_held_out_box_is_the_training_fold_dual(amd, kind, t):
    """ub = 0 on a held-out fifth: 100 iterations against the oracle on Q[tr][:, tr]; the held-out alphas stay exactly 0."""
    from optiml_amd import _lib
    from optiml_amd.ml.svm.multiclass import solve_batched
    from oracle import svm_oracle as so, bcqp_oracle as bo
    n = 600
    X, y = _blobs(n, 2)
    quad = _quad(X)
    K = so.gram('rbf', X)
    Y = np.where(y == 1, 1., -1.)[None, :]
    te = np.arange(n) % 5 == 2
    tr = ~te
    UB = np.where(tr, 2.0, 0.)[None, :]
    res = solve_batched(quad.device_problem(), _lib.PG if kind == 'pg' else _lib.FW, Y, UB, max_iter=100, t=t)[0]
    Q, q, _ = so.svc_dual(K[np.ix_(tr, tr)], Y[0][tr], 2.0)
    ub = np.full(tr.sum(), 2.0)
    ref = bo.projected_gradient(Q, q, ub, max_iter=100) if kind == 'pg' else bo.frank_wolfe(Q, q, ub, max_iter=100, t=t)
    assert res['status'] == ref['status'] and res['iter'] == ref['iter']
    np.testing.assert_allclose(res['rows']['f'], ref['f_hist'], rtol=1e-9)
    assert np.all(res['x'][te] == 0.)
    quad.release()


def _search_case(case):
    from optiml_amd.ml.svm.kernels import GaussianKernel, LinearKernel, PolyKernel
    from optiml_amd.ml.svm.losses import hinge
    from optiml_amd.opti.constrained import FrankWolfe, ProjectedGradient
    # C <= 1: the column (n-row panel, 16-column product) and SVC.fit on the fold's rows start 1 ulp apart (another summation
    # order) and PG amplifies that difference at a rate that grows with C.  tools/cv_drift_probe.py measures it on this data
    # (profiles/cv/drift_n240_pg.json): over 100 iterations max |alpha_column - alpha_fold| stays <= 2e-14 at C = 0.1 and 1, while
    # at C = 10 it grows about 10x every 10 iterations until the free sets part (iterations 52-87); both solves are bitwise
    # repeatable in and across processes.
    kw = dict(loss=hinge, dual=True, reg_intercept=True, optimizer=ProjectedGradient, max_iter=100)
    return {
        'binary-gauss-num-pg': (2, dict(kw, kernel=GaussianKernel(gamma=0.2)), {'C': [0.1, 0.3, 1.0]}),
        'binary-gauss-num-pg-f32': (2, dict(kw, kernel=GaussianKernel(gamma=0.2), storage='f32'), {'C': [0.1, 1.0]}),
        'binary-gauss-scale-fw': (2, dict(kw, kernel=GaussianKernel(gamma='scale'), optimizer=FrankWolfe),
                                  {'C': [0.5, 4.0]}),
        'binary-kernels-pg': (2, kw, {'C': [0.25, 1.0], 'kernel': [LinearKernel(), PolyKernel(degree=2, gamma=0.3),
                                                                   GaussianKernel(gamma='scale')]}),
        'multi-gauss-num-pg': (3, dict(kw, kernel=GaussianKernel(gamma=0.2)), {'C': [0.3, 1.0]}),
        'multi-linear-fw': (3, dict(kw, kernel=LinearKernel(), optimizer=FrankWolfe), {'C': [0.2, 2.0]}),
    }[case]


@pytest.mark.parametrize('case', ['binary-gauss-num-pg', 'binary-gauss-num-pg-f32', 'binary-gauss-scale-fw', 'binary-kernels-pg',
                                  'multi-gauss-num-pg', 'multi-linear-fw'])
def test_search_equals_grid_search_cv(amd, case):
    pytest.importorskip('sklearn')
    from sklearn.model_selection import GridSearchCV, StratifiedKFold
    from optiml_amd.ml.svm import SVC, OneVsRestSVC, SVCGridSearchCV
    k, kw, grid = _search_case(case)
    X, y = _blobs(240, k, d=4, seed=3)
    est = SVC if k == 2 else OneVsRestSVC
    ours = SVCGridSearchCV(est(**kw), grid, cv=StratifiedKFold(5)).fit(X, y)
    assert ours.batched_
    ref = GridSearchCV(est(**kw), grid, cv=StratifiedKFold(5)).fit(X, y)
    for i in range(5):
        assert np.array_equal(ours.cv_results_['split%d_test_score' % i], ref.cv_results_['split%d_test_score' % i])
    for key in ('mean_test_score', 'std_test_score', 'rank_test_score'):
        np.testing.assert_array_equal(ours.cv_results_[key], ref.cv_results_[key])
    assert ours.best_index_ == ref.best_index_ and ours.best_params_ == ref.best_params_
    assert ours.best_score_ == ref.best_score_ and ours.n_splits_ == 5
    assert ours.n_iter_.shape[:2] == (len(ours.cv_results_['params']), 5)
    assert (ours.n_iter_ > 0).all() and set(ours.status_.ravel()) <= {'optimal', 'stopped'}
    # held-out decision values against each fold's own estimator
    splits = list(StratifiedKFold(5).split(X, y))
    for ci, p in enumerate(ours.cv_results_['params']):
        for f in (0, 3):
            tr, te = splits[f]
            fold = est(**kw).set_params(**p).fit(X[tr], y[tr])
            want = fold.decision_function(X[te])
            got = ours._cv_decisions[ci][f]
            got = got[0] if k == 2 else np.stack(got, axis=1)
            np.testing.assert_allclose(got, want, rtol=1e-9, atol=1e-12)
    plain = est(**kw).set_params(**ours.best_params_).fit(X, y)
    assert np.array_equal(ours.decision_function(X), plain.decision_function(X))
    assert np.array_equal(ours.predict(X), plain.predict(X)) and ours.score(X, y) == plain.score(X, y)


@pytest.mark.parametrize('which', ['active-set', 'interior-point', 'other-key'])
def test_fallback_equals_grid_search_cv(amd, which):
    pytest.importorskip('sklearn')
    from sklearn.model_selection import GridSearchCV, StratifiedKFold
    from optiml_amd.ml.svm import SVC, SVCGridSearchCV
    from optiml_amd.ml.svm.kernels import GaussianKernel
    from optiml_amd.ml.svm.losses import hinge
    from optiml_amd.opti.constrained import ActiveSet, InteriorPoint, ProjectedGradient
    kw = dict(loss=hinge, dual=True, reg_intercept=True, optimizer=ProjectedGradient, max_iter=60,
              kernel=GaussianKernel(gamma=0.2))
    grid = {'C': [0.5, 2.0]}
    if which == 'active-set':
        kw['optimizer'] = ActiveSet
    elif which == 'interior-point':
        kw['optimizer'] = InteriorPoint
    else:
        grid = {'C': [0.5, 2.0], 'max_iter': [20, 40]}
    X, y = _blobs(150, 2, d=4, seed=5)
    ours = SVCGridSearchCV(SVC(**kw), grid, cv=StratifiedKFold(3)).fit(X, y)
    assert not ours.batched_
    ref = GridSearchCV(SVC(**kw), grid, cv=StratifiedKFold(3)).fit(X, y)
    for i in range(3):
        assert np.array_equal(ours.cv_results_['split%d_test_score' % i], ref.cv_results_['split%d_test_score' % i])
    assert ours.best_params_ == ref.best_params_


def test_size_case_column_follows_svc_fit(amd):
    """n = 20 000: the (fold 0, C = 1) column of a 5-fold x 2-C solve on the full panel against SVC.fit on the fold's training
    rows, f history over 20 iterations at rtol 1e-10."""
    from optiml_amd import _lib
    from optiml_amd.ml.svm import SVC
    from optiml_amd.ml.svm.kernels import GaussianKernel
    from optiml_amd.ml.svm.losses import hinge
    from optiml_amd.ml.svm.model_selection import plan_columns
    from optiml_amd.ml.svm.multiclass import solve_batched
    n = 20000
    X, y = _blobs(n, 2, d=16, seed=7)
    idx = np.arange(n)
    splits = [(idx[idx % 5 != f], idx[idx % 5 == f]) for f in range(5)]
    kernel = GaussianKernel(gamma=0.05)
    groups, _ = plan_columns(X, y, splits, [{'C': 1.0}, {'C': 4.0}], 1.0, kernel, multiclass=False)
    g = groups[0]
    quad = _quad(X, 'f64', g['kernel'])
    res = solve_batched(quad.device_problem(), _lib.PG, g['Y'], g['UB'], max_iter=20)
    quad.release()
    j = g['cols'].index((0, 0, 0, 1.0))
    tr = splits[0][0]
    svc = SVC(loss=hinge, dual=True, reg_intercept=True, kernel=kernel, C=1.0, max_iter=20).fit(X[tr], y[tr])
    np.testing.assert_allclose(res[j]['rows']['f'], svc.train_loss_history, rtol=1e-10)
    assert res[j]['iter'] == svc.optimizer.iter and res[j]['status'] == svc.optimizer.status


def test_a_failed_solve_releases_the_panel(amd, monkeypatch):
    """A batched solve that raises leaves no panel behind: `fit` raises the solve's error, and the one panel built so far was
    released once on the way out (n = 120, two candidates, two folds; the error is a Python exception before any launch)."""
    from optiml_amd.ml.svm import SVC, SVCGridSearchCV, model_selection
    from optiml_amd.opti import KernelQuadratic
    _, kw, _ = _search_case('binary-gauss-num-pg')
    X, y = _blobs(120, 2)
    calls, released = [], []

    def failing_solve(*args, **kwargs):
        calls.append(1)
        raise RuntimeError('the solve failed')

    release = KernelQuadratic.release
    monkeypatch.setattr(model_selection, 'solve_batched', failing_solve)
    monkeypatch.setattr(KernelQuadratic, 'release', lambda self: (released.append(self), release(self))[1])
    search = SVCGridSearchCV(SVC(**kw), {'C': [0.1, 1.0]}, cv=2)
    with pytest.raises(RuntimeError, match='the solve failed'):
        search.fit(X, y)
    assert len(calls) == 1 and len(released) == 1
