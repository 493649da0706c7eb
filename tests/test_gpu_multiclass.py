"""OneVsRestSVC on the device: the multi-column panel product (bq_symm.hip), the batched ProjectedGradient / FrankWolfe iteration
(bq_msolver.hip) and the estimator, against the CPU oracle, the single-class path and sklearn's OneVsRestClassifier(SVC)."""
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


def _matmat(quad, W):
    from optiml_amd.ml.svm.multiclass import _gram_matmat
    return _gram_matmat(quad.device_problem(), W)


def _blobs(n, k, d=8, seed=1):
    from optiml_amd.datasets import make_multiclass_blobs
    return make_multiclass_blobs(n, d, k, seed=seed)


@pytest.mark.parametrize('storage', ['f64', 'f32'])
@pytest.mark.parametrize('n', [300, 1037])
def test_gram_matmat_against_oracle(amd, n, storage):
    """K W for k in {1, 3, 16, 17} (17: a second pass over the chunks of 4 is ragged): against the oracle's Gram (fp64) or the
    fp32-rounded panel (fp32), ragged last tile, tile rows of several strips."""
    from oracle import svm_oracle as so
    X, _ = _blobs(n, 3)
    quad = _quad(X, storage)
    K = so.gram('rbf', X)
    if storage == 'f32':
        K = quad.gram()   # the stored panel: fp32-rounded on the device
        np.testing.assert_allclose(K, so.gram('rbf', X), rtol=0, atol=1e-6)
    rs = np.random.RandomState(n)
    for k in (1, 3, 16, 17):
        W = rs.standard_normal((k, n))
        out = _matmat(quad, W)
        ref = W @ K
        np.testing.assert_allclose(out, ref, rtol=1e-12, atol=1e-12 * np.abs(W).sum(axis=1).max())
    quad.release()


def test_gram_matmat_large_against_single_column(amd):
    """n = 20 000 (79 tile rows, 40 strips on the last one): every column of a 17-column product against the one-column
    product of the same panel, to rounding."""
    X, _ = _blobs(20000, 3, d=16)
    quad = _quad(X)
    dev = quad.device_problem()
    W = np.random.RandomState(2).standard_normal((17, 20000))
    out = _matmat(quad, W)
    for c in (0, 5, 16):
        ref = dev.gram_matvec(W[c])
        np.testing.assert_allclose(out[c], ref, rtol=1e-12, atol=1e-11 * np.abs(W[c]).sum())
    quad.release()


def test_matmat_batch_invariance(amd):
    """Column c has the same bits alone, in a batch of 3, in a batch of 17 and at another position of a permuted batch."""
    X, _ = _blobs(1037, 3)
    quad = _quad(X)
    W = np.random.RandomState(4).standard_normal((17, 1037))
    full = _matmat(quad, W)
    perm = np.random.RandomState(5).permutation(17)
    permuted = _matmat(quad, W[perm])
    for c in (0, 2, 7, 16):
        alone = _matmat(quad, W[c:c + 1])[0]
        assert np.array_equal(alone, full[c])
        assert np.array_equal(permuted[np.where(perm == c)[0][0]], full[c])
        lo = min(c, 14)
        assert np.array_equal(_matmat(quad, W[lo:lo + 3])[c - lo], full[c])
    quad.release()


@pytest.mark.parametrize('storage', ['f64', 'f32'])
def test_start_product_with_rank_one_term(amd, storage):
    """The product with K + 1 (the regularised intercept's Hessian): g_c = y_c o ((K + 1)(y_c o x0_c)) - 1 after the start-up
    of a batched solve, for 5 classes with their own labels and start points."""
    from optiml_amd import _lib
    from optiml_amd.ml.svm.multiclass import _DeviceMultiSolver
    from oracle import svm_oracle as so
    X, y = _blobs(1037, 5)
    quad = _quad(X, storage)
    K = quad.gram()
    Y = np.stack([np.where(y == c, 1., -1.) for c in range(5)])
    x0 = np.random.RandomState(6).uniform(size=Y.shape)
    s = _DeviceMultiSolver(quad.device_problem(), _lib.PG, Y, np.ones(1037), 1e-6, 10, 0.0, x0)
    s.run(1)
    for c in range(5):
        Q, q, _ = so.svc_dual(K, Y[c], 1.0)
        np.testing.assert_allclose(s.get(c, _lib.GET_G_NOW), Q @ x0[c] + q, rtol=1e-12, atol=1e-12 * 1037)
    s.close()
    quad.release()


def _oracle_pg_optimum(K, yc):
    from oracle import svm_oracle as so, bcqp_oracle as bo
    Q, q, ub = so.svc_dual(K, yc, 1.0)
    r = bo.projected_gradient(Q, q, ub, max_iter=5000)
    assert r['status'] == 'optimal'
    return r['x']


def test_batched_solve_is_batch_invariant(amd):
    """A class started at its optimum stops ('optimal') long before the others reach max_iter and leaves the batch; every class
    still has the same bits (records, x, g) as when it is solved alone through the batched path."""
    from optiml_amd import _lib
    from optiml_amd.ml.svm.multiclass import solve_batched
    from oracle import svm_oracle as so
    X, y = _blobs(600, 4)
    quad = _quad(X)
    dev = quad.device_problem()
    K = so.gram('rbf', X)
    Y = np.stack([np.where(y == c, 1., -1.) for c in range(4)])
    x0 = np.full(Y.shape, 0.5)
    x0[0] = _oracle_pg_optimum(K, Y[0])
    ub = np.ones(600)
    batch = solve_batched(dev, _lib.PG, Y, ub, max_iter=150, x0=x0)
    assert batch[0]['status'] == 'optimal' and batch[0]['iter'] < 50
    assert all(batch[c]['status'] == 'stopped' and batch[c]['iter'] == 150 for c in (1, 2, 3))
    for c in range(4):
        alone = solve_batched(dev, _lib.PG, Y[c:c + 1], ub, max_iter=150, x0=x0[c:c + 1])[0]
        assert alone['status'] == batch[c]['status'] and alone['iter'] == batch[c]['iter']
        assert np.array_equal(alone['rows']['f'], batch[c]['rows']['f'])
        assert np.array_equal(alone['x'], batch[c]['x']) and np.array_equal(alone['g'], batch[c]['g'])
    # reversed batch: other slots, other chunk positions
    rev = solve_batched(dev, _lib.PG, Y[::-1].copy(), ub, max_iter=150, x0=x0[::-1].copy())
    for c in range(4):
        assert np.array_equal(rev[3 - c]['x'], batch[c]['x'])
    quad.release()


@pytest.mark.parametrize('kind,t', [('pg', 0.0), ('fw', 0.0), ('fw', 0.1)])
def test_batched_trajectories_against_oracle(amd, kind, t):
    """4-class blobs, n = 600, RBF: the first 100 iterations of every class against the oracle's solver on svc_dual(K, y_c, C)."""
    from optiml_amd import _lib
    from optiml_amd.ml.svm.multiclass import solve_batched
    from oracle import svm_oracle as so, bcqp_oracle as bo
    X, y = _blobs(600, 4)
    quad = _quad(X)
    K = so.gram('rbf', X)
    Y = np.stack([np.where(y == c, 1., -1.) for c in range(4)])
    res = solve_batched(quad.device_problem(), _lib.PG if kind == 'pg' else _lib.FW, Y, np.ones(600), max_iter=100, t=t)
    for c in range(4):
        Q, q, ub = so.svc_dual(K, Y[c], 1.0)
        ref = bo.projected_gradient(Q, q, ub, max_iter=100) if kind == 'pg' else bo.frank_wolfe(Q, q, ub, max_iter=100, t=t)
        assert res[c]['status'] == ref['status'] and res[c]['iter'] == ref['iter']
        np.testing.assert_allclose(res[c]['rows']['f'], ref['f_hist'], rtol=1e-9)
    quad.release()


def _iris():
    from sklearn.datasets import load_iris
    from sklearn.model_selection import train_test_split
    from sklearn.preprocessing import MinMaxScaler
    X, y = load_iris(return_X_y=True)
    X = MinMaxScaler().fit_transform(X)
    return train_test_split(X, y, train_size=0.75, random_state=123456)


def _kernels():
    from optiml_amd.ml.svm.kernels import gaussian, linear, poly
    return {'gaussian': gaussian, 'poly': poly, 'linear': linear}


def _compare(ours, ref, C, Xte):
    assert len(ours.estimators_) == len(ref.estimators_)
    for a, b in zip(ours.estimators_, ref.estimators_):
        np.testing.assert_allclose(a.alphas_, b.alphas_, rtol=1e-9, atol=1e-12 * C)
        assert np.array_equal(a.support_, b.support_)
        np.testing.assert_allclose(a.dual_coef_, b.dual_coef_, rtol=1e-9, atol=1e-12 * C)
        np.testing.assert_allclose(a.intercept_, b.intercept_, rtol=1e-9, atol=1e-12)
        np.testing.assert_allclose(a.train_loss_history, b.train_loss_history, rtol=1e-9)
        assert a.optimizer.iter == b.optimizer.iter and a.optimizer.status == b.optimizer.status
        np.testing.assert_allclose(a.decision_function(Xte), b.decision_function(Xte), rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(ours.decision_function(Xte), ref.decision_function(Xte), rtol=1e-9, atol=1e-9)
    assert np.array_equal(ours.predict(Xte), ref.predict(Xte))


@pytest.mark.parametrize('data', ['iris', 'blobs5'])
@pytest.mark.parametrize('kernel', ['gaussian', 'poly', 'linear'])
@pytest.mark.parametrize('opt', ['pg', 'fw'])
def test_estimator_equals_one_vs_rest_wrapper(amd, data, kernel, opt):
    pytest.importorskip('sklearn')
    from sklearn.multiclass import OneVsRestClassifier
    from optiml_amd.ml.svm import SVC, OneVsRestSVC
    from optiml_amd.ml.svm.losses import hinge
    from optiml_amd.opti.constrained import FrankWolfe, ProjectedGradient
    if data == 'iris':
        Xtr, Xte, ytr, _ = _iris()
    else:
        X, y = _blobs(400, 5)
        Xtr, Xte, ytr = X[:300], X[300:], y[:300]
    kw = dict(loss=hinge, kernel=_kernels()[kernel], C=1.0, reg_intercept=True, dual=True, max_iter=100,
              optimizer=ProjectedGradient if opt == 'pg' else FrankWolfe)
    ours = OneVsRestSVC(**kw).fit(Xtr, ytr)
    assert ours.batched_
    ref = OneVsRestClassifier(SVC(**kw)).fit(Xtr, ytr)
    _compare(ours, ref, 1.0, Xte)
    assert ours.decision_function(Xte).shape == (len(Xte), len(np.unique(ytr)))


def test_two_classes(amd):
    pytest.importorskip('sklearn')
    from sklearn.multiclass import OneVsRestClassifier
    from optiml_amd.ml.svm import SVC, OneVsRestSVC
    from optiml_amd.ml.svm.losses import hinge
    X, y = _blobs(300, 3)
    keep = y != 1
    X, y = X[keep], np.where(y[keep] == 0, 'a', 'c')
    kw = dict(loss=hinge, reg_intercept=True, dual=True, max_iter=60)
    ours = OneVsRestSVC(**kw).fit(X, y)
    ref = OneVsRestClassifier(SVC(**kw)).fit(X, y)
    assert len(ours.estimators_) == 1 and ours.decision_function(X).ndim == 1
    _compare(ours, ref, 1.0, X)


@pytest.mark.parametrize('opt', ['as', 'ip'])
def test_fallback_optimizers_equal_the_wrapper(amd, opt):
    pytest.importorskip('sklearn')
    from sklearn.multiclass import OneVsRestClassifier
    from optiml_amd.ml.svm import SVC, OneVsRestSVC
    from optiml_amd.ml.svm.kernels import gaussian
    from optiml_amd.ml.svm.losses import hinge
    from optiml_amd.opti.constrained import ActiveSet, InteriorPoint
    Xtr, Xte, ytr, _ = _iris()
    kw = dict(loss=hinge, kernel=gaussian, reg_intercept=True, dual=True, optimizer=ActiveSet if opt == 'as' else InteriorPoint)
    ours = OneVsRestSVC(**kw).fit(Xtr, ytr)
    assert not ours.batched_
    ref = OneVsRestClassifier(SVC(**kw)).fit(Xtr, ytr)
    for a, b in zip(ours.estimators_, ref.estimators_):
        assert np.array_equal(a.alphas_, b.alphas_) and a.intercept_ == b.intercept_
    assert np.array_equal(ours.decision_function(Xte), ref.decision_function(Xte))


@pytest.mark.parametrize('opt', ['pg', 'fw'])
def test_iris_accuracy(amd, opt):
    """The reference's integration test (optiml/ml/tests/test_svc.py:96-115) with OneVsRestSVC: test accuracy >= 0.97."""
    pytest.importorskip('sklearn')
    from optiml_amd.ml.svm import OneVsRestSVC
    from optiml_amd.ml.svm.kernels import gaussian
    from optiml_amd.ml.svm.losses import hinge
    from optiml_amd.opti.constrained import FrankWolfe, ProjectedGradient
    Xtr, Xte, ytr, yte = _iris()
    est = OneVsRestSVC(loss=hinge, kernel=gaussian, reg_intercept=True, dual=True,
                       optimizer=ProjectedGradient if opt == 'pg' else FrankWolfe).fit(Xtr, ytr)
    assert est.batched_ and est.score(Xte, yte) >= 0.97


def test_size_case_against_single_class_svc(amd):
    """n = 20 000, k = 10, 20 PG iterations: every class's objective history against SVC on that class alone."""
    from optiml_amd.ml.svm import SVC, OneVsRestSVC
    from optiml_amd.ml.svm.losses import hinge
    from optiml_amd.opti.constrained import ProjectedGradient
    X, y = _blobs(20000, 10, d=32)
    kw = dict(loss=hinge, reg_intercept=True, dual=True, optimizer=ProjectedGradient, max_iter=20)
    est = OneVsRestSVC(**kw).fit(X, y)
    for c in range(10):
        one = SVC(**kw).fit(X, (y == c).astype(int))
        np.testing.assert_allclose(est.estimators_[c].train_loss_history, one.train_loss_history, rtol=1e-12)
        assert est.estimators_[c].optimizer.status == one.optimizer.status == 'stopped'
