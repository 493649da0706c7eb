"""OneVsOneSVC on the device: the pair-routed panel product (bq_symmp.hip), the pair solver (bq_msolver_create_pairs) and the
estimator, against NumPy, the wide product, SVC.fit on each pair's rows and sklearn's OneVsOneClassifier(SVC)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def amd():
    from optiml_amd import _lib
    from optiml_amd.device import get_context
    _lib.load()
    get_context()


def _layout(sizes, d=5, seed=0, integer=False):
    """Class-sorted, tile-padded rows for classes of `sizes` rows: (Xp, cls_tiles, pcode: class of every panel row)."""
    from optiml_amd.ml.svm.onevsone import sort_plan
    rs = np.random.RandomState(seed)
    codes = np.concatenate([np.full(s, c) for c, s in enumerate(sizes)])
    rs.shuffle(codes)
    X = rs.randint(-3, 4, size=(len(codes), d)).astype(float) if integer else rs.standard_normal((len(codes), d)) + codes[:, None]
    index, ct, n_pad = sort_plan(codes, len(sizes))
    Xp = np.zeros((n_pad, d))
    Xp[index] = X
    return Xp, ct, np.repeat(np.arange(len(sizes)), np.diff(ct) * 256)


def _quad(Xp, storage='f64', kernel=None):
    from optiml_amd.opti import KernelQuadratic
    from optiml_amd.ml.svm.kernels import GaussianKernel
    n = Xp.shape[0]
    return KernelQuadratic(Xp, -np.ones(n), 'svc', kernel or GaussianKernel(gamma=0.2), y=np.ones(n), storage=storage)


def _routed(quad, ct, pairs, W):
    from optiml_amd.ml.svm.onevsone import gram_matmat_pairs
    return gram_matmat_pairs(quad.device_problem(), ct, pairs, W)


LAYOUTS = {
    'k2': [300, 40],
    'k3': [1, 257, 600],
    'k10': [1, 255, 256, 257, 700, 30, 90, 512, 3, 400],
    'k20': [10 + 13 * c for c in range(20)],   # 19 pairs per class: two 16-slot chunks per diagonal block
}


@pytest.mark.parametrize('storage', ['f64', 'f32'])
@pytest.mark.parametrize('layout', sorted(LAYOUTS))
def test_routed_product_against_numpy(amd, layout, storage):
    """Every pair's column against NumPy's K W on the pair's rows; exact 0 on every other row.  W is NaN outside the pair's rows:
    those entries must never be read."""
    from optiml_amd.ml.svm.onevsone import ovo_pairs
    sizes = LAYOUTS[layout]
    Xp, ct, pcode = _layout(sizes, seed=len(sizes))
    quad = _quad(Xp, storage)
    K = quad.gram()
    pairs = ovo_pairs(len(sizes))
    rs = np.random.RandomState(3)
    W = rs.standard_normal((len(pairs), len(pcode)))
    masks = [(pcode == i) | (pcode == j) for i, j in pairs]
    for p, m in enumerate(masks):
        W[p][~m] = np.nan
    out = _routed(quad, ct, pairs, W)
    for p, m in enumerate(masks):
        want = K[np.ix_(m, m)] @ W[p][m]
        np.testing.assert_allclose(out[p][m], want, rtol=1e-12, atol=1e-13 * np.abs(W[p][m]).sum())
        assert np.all(out[p][~m] == 0.)
    quad.release()


@pytest.mark.parametrize('sizes', [[300, 777], [5, 260, 100, 513]])
def test_routed_product_exact_on_small_integers(amd, sizes):
    """Linear kernel, small-integer X and W: every product and sum is exact, so any wrong lane, slot, tile or slab entry shows."""
    from optiml_amd.ml.svm.kernels import linear
    from optiml_amd.ml.svm.onevsone import ovo_pairs
    Xp, ct, pcode = _layout(sizes, d=3, seed=7, integer=True)
    quad = _quad(Xp, 'f64', linear)
    pairs = ovo_pairs(len(sizes))
    Wi = np.random.RandomState(8).randint(-4, 5, size=(len(pairs), len(pcode))).astype(float)
    out = _routed(quad, ct, pairs, Wi)
    K = Xp @ Xp.T
    for p, (i, j) in enumerate(pairs):
        m = (pcode == i) | (pcode == j)
        want = np.zeros(len(pcode))
        want[m] = K[np.ix_(m, m)] @ Wi[p][m]
        assert np.array_equal(out[p], want)
    quad.release()


def test_routed_product_against_wide_product(amd):
    from optiml_amd.ml.svm.multiclass import _gram_matmat
    from optiml_amd.ml.svm.onevsone import ovo_pairs
    Xp, ct, pcode = _layout([500, 300, 20, 900], seed=2)
    quad = _quad(Xp)
    pairs = ovo_pairs(4)
    W = np.random.RandomState(4).standard_normal((len(pairs), len(pcode)))
    for p, (i, j) in enumerate(pairs):
        W[p][(pcode != i) & (pcode != j)] = 0.
    out = _routed(quad, ct, pairs, W)
    wide = _gram_matmat(quad.device_problem(), W, wide=True)
    for p, (i, j) in enumerate(pairs):
        m = (pcode == i) | (pcode == j)
        np.testing.assert_allclose(out[p][m], wide[p][m], rtol=1e-12, atol=1e-13 * np.abs(W[p]).sum())
    quad.release()


def test_routed_product_batch_invariance(amd):
    """A pair's column has the same bits alone, in the full set, at another slot and on a second run."""
    from optiml_amd.ml.svm.onevsone import ovo_pairs
    sizes = LAYOUTS['k20']
    Xp, ct, pcode = _layout(sizes, seed=5)
    quad = _quad(Xp)
    pairs = ovo_pairs(len(sizes))
    W = np.random.RandomState(6).standard_normal((len(pairs), len(pcode)))
    full = _routed(quad, ct, pairs, W)
    assert np.array_equal(_routed(quad, ct, pairs, W), full)
    perm = np.random.RandomState(7).permutation(len(pairs))
    permuted = _routed(quad, ct, [pairs[q] for q in perm], W[perm])
    for p in (0, 18, 19, 77, len(pairs) - 1):
        assert np.array_equal(_routed(quad, ct, [pairs[p]], W[p:p + 1])[0], full[p])
        assert np.array_equal(permuted[np.where(perm == p)[0][0]], full[p])
    quad.release()


def _pair_columns(pcode, pairs, C, ghost):
    Y = np.stack([np.where(pcode == j, 1., -1.) for _, j in pairs])
    UB = np.stack([np.where(((pcode == i) | (pcode == j)) & ~ghost, C, 0.) for i, j in pairs])
    return Y, UB


def _solve(dev, kind, ct, pairs, Y, UB, max_iter, x0=None, t=0.0):
    from optiml_amd.ml.svm.multiclass import solve_batched
    from optiml_amd.ml.svm.onevsone import _DevicePairSolver
    solver = _DevicePairSolver(dev, kind, ct, pairs, Y, UB, 1e-6, max_iter, t=t, x0=x0)
    return solve_batched(dev, kind, Y, UB, max_iter=max_iter, solver=solver)


def _blob_panel(sizes, d=6, seed=1):
    from optiml_amd.datasets import make_multiclass_blobs
    from optiml_amd.ml.svm.onevsone import sort_plan
    X, y = make_multiclass_blobs(sum(sizes) * 3, d, len(sizes), seed=seed)
    keep = np.concatenate([np.flatnonzero(y == c)[:s] for c, s in enumerate(sizes)])
    keep.sort()
    X, y = X[keep], y[keep]
    index, ct, n_pad = sort_plan(y, len(sizes))
    Xp = np.zeros((n_pad, d))
    Xp[index] = X
    ghost = np.ones(n_pad, dtype=bool)
    ghost[index] = False
    return X, y, Xp, ct, np.repeat(np.arange(len(sizes)), np.diff(ct) * 256), ghost, index


@pytest.mark.parametrize('kind,t', [('pg', 0.0), ('fw', 0.0)])
def test_pair_solve_is_batch_invariant(amd, kind, t):
    """One pair starts at its optimum and stops early, the others run 100 iterations: every pair has the same bits (records, x, g)
    alone, in the full solve and in a reversed solve."""
    from optiml_amd import _lib
    from optiml_amd.ml.svm.onevsone import ovo_pairs, pair_problem
    from oracle import svm_oracle as so, bcqp_oracle as bo
    X, y, Xp, ct, pcode, ghost, index = _blob_panel([150, 300, 90, 200])
    quad = _quad(Xp)
    dev = quad.device_problem()
    pairs = ovo_pairs(4)
    Y, UB = _pair_columns(pcode, pairs, 0.5, ghost)
    x0 = UB / 2
    rows, yp = pair_problem(y, 0, 1)
    Q, q, _ = so.svc_dual(so.gram('rbf', X[rows], gamma=0.2), yp, 0.5)
    r = bo.projected_gradient(Q, q, np.full(len(rows), 0.5), max_iter=5000)
    assert r['status'] == 'optimal'
    x0[0] = 0.
    x0[0][index[rows]] = r['x']
    k = _lib.PG if kind == 'pg' else _lib.FW
    batch = _solve(dev, k, ct, pairs, Y, UB, 100, x0=x0, t=t)
    if kind == 'pg':
        assert batch[0]['status'] == 'optimal' and batch[0]['iter'] < 50
    rev = _solve(dev, k, ct, pairs[::-1], Y[::-1].copy(), UB[::-1].copy(), 100, x0=x0[::-1].copy(), t=t)
    for p in range(len(pairs)):
        alone = _solve(dev, k, ct, pairs[p:p + 1], Y[p:p + 1], UB[p:p + 1], 100, x0=x0[p:p + 1], t=t)[0]
        for other in (alone, rev[len(pairs) - 1 - p]):
            assert other['status'] == batch[p]['status'] and other['iter'] == batch[p]['iter']
            assert np.array_equal(other['rows']['f'], batch[p]['rows']['f'])
            assert np.array_equal(other['x'], batch[p]['x']) and np.array_equal(other['g'], batch[p]['g'])
        assert np.all(batch[p]['x'][UB[p] == 0.] == 0.)
    quad.release()


@pytest.mark.parametrize('kind', ['pg', 'fw'])
@pytest.mark.parametrize('C', [0.1, 1.0])
def test_pair_column_follows_svc_fit(amd, kind, C):
    """100 iterations at C <= 1 (the rank-one panel term, ADD_ONE, is on): each pair column against SVC.fit on the pair's rows —
    alpha to rounding (test_gpu_cv.py's tolerances), the objective history at rtol 1e-12."""
    from optiml_amd import _lib
    from optiml_amd.ml.svm import SVC
    from optiml_amd.ml.svm.kernels import GaussianKernel
    from optiml_amd.ml.svm.losses import hinge
    from optiml_amd.ml.svm.onevsone import ovo_pairs, pair_problem
    from optiml_amd.opti.constrained import FrankWolfe, ProjectedGradient
    X, y, Xp, ct, pcode, ghost, index = _blob_panel([120, 260, 75])
    quad = _quad(Xp)
    pairs = ovo_pairs(3)
    Y, UB = _pair_columns(pcode, pairs, C, ghost)
    res = _solve(quad.device_problem(), _lib.PG if kind == 'pg' else _lib.FW, ct, pairs, Y, UB, 100)
    for p, (i, j) in enumerate(pairs):
        rows, yp = pair_problem(y, i, j)
        svc = SVC(loss=hinge, kernel=GaussianKernel(gamma=0.2), C=C, reg_intercept=True, dual=True, max_iter=100,
                  optimizer=ProjectedGradient if kind == 'pg' else FrankWolfe).fit(X[rows], (yp > 0).astype(int))
        np.testing.assert_allclose(res[p]['x'][index[rows]], svc.alphas_, rtol=1e-9, atol=1e-12 * C)
        # rtol 1e-12 of the history's scale: where f passes near 0 its own relative error is not that of the iterates
        f = np.asarray(svc.train_loss_history)
        np.testing.assert_allclose(res[p]['rows']['f'], f, rtol=1e-12, atol=1e-12 * np.abs(f).max() * 1e-2)
        assert res[p]['iter'] == svc.optimizer.iter and res[p]['status'] == svc.optimizer.status
    quad.release()


def _iris():
    from sklearn.datasets import load_iris
    from sklearn.model_selection import train_test_split
    from sklearn.preprocessing import MinMaxScaler
    X, y = load_iris(return_X_y=True)
    X = MinMaxScaler().fit_transform(X)
    return train_test_split(X, y, train_size=0.75, random_state=123456)


def _kernels():
    from optiml_amd.ml.svm.kernels import GaussianKernel, PolyKernel, linear
    return {'gaussian': GaussianKernel(gamma=0.7), 'poly': PolyKernel(degree=3, gamma='auto', coef0=1.), 'linear': linear}


def _compare(ours, ref, C, Xte):
    """Alphas and gradients to the rounding the solver accumulates from its 1-ulp start difference (1e-10 absolute at C = 1),
    decision values at rtol 1e-9, predictions equal."""
    assert len(ours.estimators_) == len(ref.estimators_)
    for a, b in zip(ours.estimators_, ref.estimators_):
        np.testing.assert_allclose(a.alphas_, b.alphas_, rtol=1e-9, atol=1e-10 * C)
        assert np.array_equal(a.support_, b.support_)
        np.testing.assert_allclose(a.dual_coef_, b.dual_coef_, rtol=1e-9, atol=1e-10 * C)
        np.testing.assert_allclose(a.intercept_, b.intercept_, rtol=1e-9, atol=1e-12)
        np.testing.assert_allclose(a.train_loss_history, b.train_loss_history, rtol=1e-9)
        assert a.optimizer.iter == b.optimizer.iter and a.optimizer.status == b.optimizer.status
        np.testing.assert_allclose(a.optimizer.g_x, b.optimizer.g_x, rtol=1e-9, atol=1e-10 * len(a.alphas_))   # Q x: n terms
    np.testing.assert_allclose(ours.decision_function(Xte), ref.decision_function(Xte), rtol=1e-9, atol=1e-9)
    assert np.array_equal(ours.predict(Xte), ref.predict(Xte))
    assert ours.score(Xte, ours.predict(Xte)) == 1.0


@pytest.mark.parametrize('data', ['iris', 'blobs5'])
@pytest.mark.parametrize('kernel', ['gaussian', 'poly', 'linear'])
@pytest.mark.parametrize('opt', ['pg', 'fw'])
def test_estimator_equals_one_vs_one_wrapper(amd, data, kernel, opt):
    from sklearn.multiclass import OneVsOneClassifier
    from optiml_amd.datasets import make_multiclass_blobs
    from optiml_amd.ml.svm import SVC, OneVsOneSVC
    from optiml_amd.ml.svm.losses import hinge
    from optiml_amd.opti.constrained import FrankWolfe, ProjectedGradient
    if data == 'iris':
        Xtr, Xte, ytr, _ = _iris()
    else:
        X, y = make_multiclass_blobs(400, 8, 5, seed=1)
        Xtr, Xte, ytr = X[:300], X[300:], y[:300]
    # The pair's column and SVC.fit on the pair's rows sum their products in different orders and start 1 ulp apart; PG amplifies
    # that difference (about 10x per 10 iterations at C = 1 on these data, as test_gpu_cv.py notes for folds), so its comparison
    # stops at 20 iterations, where decision values still agree to 1e-9; FW's runs 100.
    kw = dict(loss=hinge, kernel=_kernels()[kernel], C=1.0, reg_intercept=True, dual=True, max_iter=20 if opt == 'pg' else 100,
              optimizer=ProjectedGradient if opt == 'pg' else FrankWolfe)
    ours = OneVsOneSVC(**kw).fit(Xtr, ytr)
    assert ours.batched_ and ours.n_classes_ == len(np.unique(ytr))
    ref = OneVsOneClassifier(SVC(**kw)).fit(Xtr, ytr)
    _compare(ours, ref, 1.0, Xte)
    assert ours.decision_function(Xte).shape == (len(Xte), len(np.unique(ytr)))


def test_two_classes(amd):
    from sklearn.multiclass import OneVsOneClassifier
    from optiml_amd.datasets import make_multiclass_blobs
    from optiml_amd.ml.svm import SVC, OneVsOneSVC
    from optiml_amd.ml.svm.kernels import GaussianKernel
    from optiml_amd.ml.svm.losses import hinge
    X, y = make_multiclass_blobs(300, 8, 3, seed=1)
    keep = y != 1
    X, y = X[keep], np.where(y[keep] == 0, 'a', 'c')
    kw = dict(loss=hinge, kernel=GaussianKernel(gamma='auto'), reg_intercept=True, dual=True, max_iter=60)
    ours = OneVsOneSVC(**kw).fit(X, y)
    ref = OneVsOneClassifier(SVC(**kw)).fit(X, y)
    assert ours.batched_ and len(ours.estimators_) == 1 and ours.decision_function(X).ndim == 1
    _compare(ours, ref, 1.0, X)


@pytest.mark.parametrize('which', ['scale', 'as', 'ip'])
def test_fallback_equals_the_wrapper(amd, which):
    from sklearn.multiclass import OneVsOneClassifier
    from optiml_amd.ml.svm import SVC, OneVsOneSVC
    from optiml_amd.ml.svm.kernels import GaussianKernel
    from optiml_amd.ml.svm.losses import hinge
    from optiml_amd.opti.constrained import ActiveSet, InteriorPoint, ProjectedGradient
    Xtr, Xte, ytr, _ = _iris()
    opt = {'scale': ProjectedGradient, 'as': ActiveSet, 'ip': InteriorPoint}[which]
    kw = dict(loss=hinge, kernel=GaussianKernel(gamma='scale' if which == 'scale' else 0.7), reg_intercept=True, dual=True,
              optimizer=opt, max_iter=100)
    ours = OneVsOneSVC(**kw).fit(Xtr, ytr)
    assert not ours.batched_
    ref = OneVsOneClassifier(SVC(**kw)).fit(Xtr, ytr)
    for a, b in zip(ours.estimators_, ref.estimators_):
        assert np.array_equal(a.alphas_, b.alphas_) and a.intercept_ == b.intercept_
    assert np.array_equal(ours.decision_function(Xte), ref.decision_function(Xte))
    assert np.array_equal(ours.predict(Xte), ref.predict(Xte))


@pytest.mark.parametrize('opt', ['pg', 'fw'])
def test_iris_accuracy(amd, opt):
    """The reference's Iris integration test (optiml/ml/tests/test_svc.py:96-115) with OneVsOneSVC, gamma='auto': >= 0.97."""
    from optiml_amd.ml.svm import OneVsOneSVC
    from optiml_amd.ml.svm.kernels import GaussianKernel
    from optiml_amd.ml.svm.losses import hinge
    from optiml_amd.opti.constrained import FrankWolfe, ProjectedGradient
    Xtr, Xte, ytr, yte = _iris()
    est = OneVsOneSVC(loss=hinge, kernel=GaussianKernel(gamma='auto'), reg_intercept=True, dual=True,
                      optimizer=ProjectedGradient if opt == 'pg' else FrankWolfe).fit(Xtr, ytr)
    assert est.batched_ and est.score(Xte, yte) >= 0.97


def test_grid_search_over_one_vs_one(amd):
    """SVCGridSearchCV takes a OneVsOneSVC through its per-fold path: each fold's fit is one batched one-vs-one solve."""
    from sklearn.model_selection import GridSearchCV
    from sklearn.multiclass import OneVsOneClassifier
    from optiml_amd.ml.svm import SVC, OneVsOneSVC, SVCGridSearchCV
    from optiml_amd.ml.svm.kernels import GaussianKernel
    from optiml_amd.ml.svm.losses import hinge
    Xtr, _, ytr, _ = _iris()
    kw = dict(loss=hinge, kernel=GaussianKernel(gamma=0.7), reg_intercept=True, dual=True, max_iter=60)
    ours = SVCGridSearchCV(OneVsOneSVC(**kw), {'C': [0.5, 1.0]}, cv=3).fit(Xtr, ytr)
    assert not ours.batched_ and ours.best_estimator_.batched_
    assert ours.n_iter_.shape == (2, 3, 3)
    ref = GridSearchCV(OneVsOneClassifier(SVC(**kw)), {'estimator__C': [0.5, 1.0]}, cv=3).fit(Xtr, ytr)
    np.testing.assert_allclose(ours.cv_results_['mean_test_score'], ref.cv_results_['mean_test_score'])


def test_size_case_against_single_pair_svc(amd):
    """n = 20 000, k = 10, 20 PG iterations: every pair's objective history against SVC on that pair's rows alone."""
    from optiml_amd.datasets import make_multiclass_blobs
    from optiml_amd.ml.svm import SVC, OneVsOneSVC
    from optiml_amd.ml.svm.kernels import GaussianKernel
    from optiml_amd.ml.svm.losses import hinge
    from optiml_amd.ml.svm.onevsone import ovo_pairs, pair_problem
    from optiml_amd.opti.constrained import ProjectedGradient
    X, y = make_multiclass_blobs(20000, 32, 10, seed=1)
    kw = dict(loss=hinge, kernel=GaussianKernel(gamma=1. / 32), reg_intercept=True, dual=True, optimizer=ProjectedGradient,
              max_iter=20)
    est = OneVsOneSVC(**kw).fit(X, y)
    assert est.batched_
    for p, (i, j) in enumerate(ovo_pairs(10)):
        rows, yp = pair_problem(y, i, j)
        one = SVC(**kw).fit(X[rows], (yp > 0).astype(int))
        np.testing.assert_allclose(est.estimators_[p].train_loss_history, one.train_loss_history, rtol=1e-12)
