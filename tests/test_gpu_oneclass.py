"""OneClassSVM on the device: the capped-simplex projection kernel alone (bq_simplex_project), the batched nu-one-class solver
(bq_msolver_create_simplex: sx_top / sx_dir / sx_close around the 16-column panel product) against the NumPy reference
(tests/oneclass_reference.py), the estimator against sklearn, one box per column, and the nu path."""
import functools

import numpy as np
import pytest

import oneclass_reference as ocr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def amd():
    from optiml_amd import _lib
    from optiml_amd.device import get_context
    _lib.load()
    get_context()


def _quad(X, kernel, storage='f64'):
    from optiml_amd.opti import KernelQuadratic
    return KernelQuadratic(X, np.zeros(X.shape[0]), 'plain', kernel, storage=storage)


def _solve(dev, UB, mass, tol, max_iter, x0=None):
    """the columns' results (rows, status, iter, f_x, x, g) with rho, n_sv, n_free from the device"""
    from optiml_amd.ml.svm._batched import _DeviceSimplexSolver, solve_batched
    UB = np.atleast_2d(UB)
    held = []
    res = solve_batched(dev, None, UB, None, solver=_DeviceSimplexSolver(dev, UB, mass, tol, max_iter, x0),
                        before_close=lambda s, _: held.extend(s.offsets()))
    for c, r in enumerate(res):
        r.update(rho=held[0][c], n_sv=int(held[1][c]), n_free=int(held[2][c]))
    return res


def _same_bits(a, b):
    return (np.array_equal(a['x'], b['x']) and np.array_equal(a['g'], b['g']) and len(a['rows']) == len(b['rows']) and
            a['rows'].tobytes() == b['rows'].tobytes() and a['rho'] == b['rho'] and a['status'] == b['status'])


# ---- 1. the projection kernel alone -------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _projection_columns(n):
    """17 columns (V, UB, mass) on n entries: two seeds x the three scales x the three masses of the host test, less one"""
    cols = []
    for seed in (0, 1):
        for scale in (1.0, 1e4, 1e-4):
            v, u, masses = ocr.projection_inputs(n, scale, seed)
            cols.extend((v, u, r) for r in masses)
    cols = cols[:17]
    return np.stack([c[0] for c in cols]), np.stack([c[1] for c in cols]), np.array([c[2] for c in cols])


@pytest.mark.parametrize('n', [1, 256, 257, 600, 1100])
def test_projection_against_the_reference(amd, n):
    """n = 1; 256 exactly and 257 (one entry over a quarter of the workgroup's stride); 600; 1100 (the 1024-thread strided loop takes
    a second, ragged trip).  17 columns of different (u, r) in one launch: the box holds bitwise, zero-width rows stay 0, r = sum u
    gives u itself, and the two error figures stay within the host test's bounds (8 x the reference's own, floor 2^-50 max(1,
    |v|_inf)).  Three of the columns again alone: the same bits."""
    from optiml_amd.ml.svm._batched import simplex_project
    V, UB, mass = _projection_columns(n)
    P = simplex_project(V, UB, mass)
    assert P.shape == V.shape
    for c in range(len(mass)):
        v, u, r = V[c], UB[c], mass[c]
        assert np.all(P[c] >= 0) and np.all(P[c] <= u)
        assert np.all(P[c][u == 0] == 0)
        if r == u.sum():
            assert np.array_equal(P[c], u)
        fs, fi = ocr.projection_figures(P[c], v, u, r)
        bs, bi = ocr.projection_bounds(v, u, r)
        print('n=%d column %d: |sum P - r| = %.2e (bound %.2e), |P - P_ext| = %.2e (bound %.2e)' % (n, c, fs, bs, fi, bi))
        assert fs <= bs and fi <= bi
    for c in (0, 9, 16):
        alone = simplex_project(V[c:c + 1], UB[c:c + 1], mass[c:c + 1])
        assert np.array_equal(alone[0], P[c])


def test_projection_refuses_bad_columns(amd):
    from optiml_amd import _lib
    from optiml_amd.ml.svm._batched import simplex_project
    v, u = np.zeros(5), np.ones(5)
    for UB, mass in ((-u, 1.0), (u, 0.0), (u, 5.1), (u * np.inf, 1.0)):
        with pytest.raises(_lib.BcqpError):
            simplex_project(v, UB, [mass])


# ---- 2. trajectory parity -------------------------------------------------------------------------------------------------------------
TRAJ_NUS = (0.0517, 0.2517, 0.8017)
TRAJ_GAMMA = 3.0   # d = 3: none of the six cases is near its optimum after 30 iterations (the reference's violation there: 1e-2 ... 0.2)


@functools.lru_cache(maxsize=None)
def _trajectory_reference(n):
    """The reference's 30 iterations for the three nu, and per nu the largest spread of its final x over three seeded draws of K
    perturbed by one ulp per entry.  Measured: n = 600: 2.2e-14, 1.4e-13, 5.4e-13; n = 1100: 1.1e-13, 1.5e-13, 1.3e-13 (the f
    histories of such runs moved by < 3e-13 relative); the device's x was 1.1e-14 ... 5.1e-13 from the reference's."""
    from oracle import svm_oracle as so
    X = ocr.one_class_data(n, 3)
    K = so.gram('rbf', X, gamma=TRAJ_GAMMA)
    u = np.ones(n)
    out = []
    for nu in TRAJ_NUS:
        base = ocr.solve(K, u, nu * n, tol=0.0, max_iter=30)
        spread = 0.0
        for seed in range(3):
            up = np.random.RandomState(seed).rand(n, n) < 0.5
            r = ocr.solve(np.nextafter(K, np.where(up, np.inf, -np.inf)), u, nu * n, tol=0.0, max_iter=30)
            assert r['iter'] == base['iter']
            spread = max(spread, float(np.abs(r['x'] - base['x']).max()))
        out.append((base, spread))
    return X, out


@pytest.mark.parametrize('n', [600, 1100])
def test_trajectory_parity(amd, n):
    """n = 600: 3 tile rows and a ragged last tile; n = 1100: 5.  tol = 0, max_iter = 30: statuses and iteration counts are the
    reference's, the f history agrees to rtol 1e-9, and x after the last iteration lies within 10 x the spread that one ulp per entry
    of K gives the reference's own x."""
    from optiml_amd.ml.svm.kernels import GaussianKernel
    X, ref = _trajectory_reference(n)
    quad = _quad(X, GaussianKernel(gamma=TRAJ_GAMMA))
    res = _solve(quad.device_problem(), np.ones((3, n)), [nu * n for nu in TRAJ_NUS], 0.0, 30)
    for r, (base, spread) in zip(res, ref):
        assert r['status'] == base['status'] and r['iter'] == base['iter']
        assert np.array_equal(r['rows']['iter'], base['rows'][:, 0].astype(np.int64))
        np.testing.assert_allclose(r['rows']['f'], base['rows'][:, 1], rtol=1e-9)
        np.testing.assert_allclose(r['rows']['r1'], base['rows'][:, 2], rtol=1e-6, atol=1e-9)
        err = float(np.abs(r['x'] - base['x']).max())
        print('n=%d: |x - x_ref| = %.2e, 10 x spread = %.2e' % (n, err, 10 * spread))
        assert err <= 10 * spread
        assert np.all(r['x'] >= 0) and np.all(r['x'] <= 1)
    quad.release()


# ---- 3. convergence, and the estimator against sklearn --------------------------------------------------------------------------
EST_NUS = (0.0517, 0.2517, 0.5017, 0.8017)
FLAT_CASE = (1.0 / 8, 0.0517)   # (gamma, nu): see test_estimator_against_sklearn


@functools.lru_cache(maxsize=None)
def _sklearn_fits(gamma):
    svm = pytest.importorskip('sklearn.svm')
    X = ocr.one_class_data(600, 8)
    Xnew = np.random.RandomState(50).standard_normal((50, 8)) * 1.5
    return X, Xnew, [svm.OneClassSVM(kernel='rbf', gamma=gamma, nu=nu, tol=1e-12).fit(X) for nu in EST_NUS]


@pytest.mark.parametrize('tol', [1e-3, 1e-6])
@pytest.mark.parametrize('gamma', [1.0 / 8, 0.02])
def test_estimator_against_sklearn(amd, gamma, tol):
    """The host grid at n = 600: 'optimal'; the violation recomputed in NumPy from alphas_ is within tol; sum alpha = nu n; the
    decision values on X and on 50 fresh points lie within 10 tol of sklearn's (tol 1e-12); predict equals sklearn's wherever
    sklearn's |decision| exceeds 10 tol, which leaves out at most 15 % of the training rows in every (gamma, nu, tol) case but
    FLAT_CASE; score_samples - offset_ is decision_function bit for bit; at tol 1e-6 the support set is sklearn's.

    FLAT_CASE, gamma = 1 / d with nu = 0.0517: sklearn's own solution has 103 free support vectors (0 < dual_coef < 1), 17.2 % of
    the 600 rows, and a free support vector's decision value is 0 by the optimality conditions, so no comparison of predictions
    can keep them.  There the rows left out are bounded by those free support vectors plus 1 % of the rows, and the measured
    counts are asserted: 109 rows (18.2 %) at tol 1e-3, 103 rows (17.2 %) at tol 1e-6."""
    from optiml_amd.ml.svm import OneClassSVM
    from optiml_amd.ml.svm.kernels import GaussianKernel
    from oracle import svm_oracle as so
    X, Xnew, refs = _sklearn_fits(gamma)
    n = X.shape[0]
    K = so.gram('rbf', X, gamma=gamma)
    left_out = []
    for nu, ref in zip(EST_NUS, refs):
        est = OneClassSVM(kernel=GaussianKernel(gamma=gamma), nu=nu, tol=tol).fit(X)
        assert est.status_ == 'optimal' and est.n_iter_ <= 1000
        a = est.alphas_
        assert a.shape == (n,) and a.min() >= 0 and a.max() <= 1
        viol = ocr.violation(a, K @ a, np.ones(n))
        print('gamma=%g nu=%g tol=%g: %d iterations, violation %.3e (device: %.3e)' % (gamma, nu, tol, est.n_iter_, viol,
                                                                                          est.kkt_violation_))
        assert viol <= tol + 1e-9 and est.kkt_violation_ <= tol
        assert abs(a.sum() - nu * n) <= 1e-10 * nu * n
        assert np.array_equal(est.support_, np.flatnonzero(a > 0)) and np.array_equal(est.dual_coef_, a[a > 0])
        assert est.intercept_ == -est.offset_ and len(est.train_loss_history) == est.n_iter_ + 1
        for Z in (X, Xnew):
            dec, theirs = est.decision_function(Z), ref.decision_function(Z)
            assert np.abs(dec - theirs).max() <= 10 * tol
            assert np.array_equal(est.score_samples(Z) - est.offset_, dec)
            clear = np.abs(theirs) > 10 * tol
            assert np.array_equal(est.predict(Z)[clear], ref.predict(Z)[clear])
            if Z is X:
                left = int((~clear).sum())
                left_out.append(left / n)
                if (gamma, nu) == FLAT_CASE:
                    coef = ref.dual_coef_[0]
                    free = int(((coef > 0) & (coef < 1)).sum())
                    assert free == 103 and free <= left <= free + 0.01 * n
                    assert left == {1e-3: 109, 1e-6: 103}[tol]
                else:
                    assert left <= 0.15 * n
        assert set(np.unique(est.predict(X))) <= {-1, 1}
        if tol == 1e-6:
            assert np.array_equal(est.support_, ref.support_)
    print('left out of the predict comparison per nu:', ['%.3f' % v for v in left_out])


def test_string_gamma_is_resolved_on_the_training_rows(amd):
    from optiml_amd.ml.svm import OneClassSVM
    from optiml_amd.ml.svm.kernels import GaussianKernel
    X = ocr.one_class_data(257, 3)
    a = OneClassSVM(kernel=GaussianKernel(gamma='scale'), nu=0.2517).fit(X)
    g = 1.0 / (3 * X.var())
    b = OneClassSVM(kernel=GaussianKernel(gamma=g), nu=0.2517).fit(X)
    assert a.kernel_.gamma == g and a.kernel.gamma == 'scale'
    assert np.array_equal(a.alphas_, b.alphas_) and a.offset_ == b.offset_
    assert np.array_equal(a.decision_function(X[:40]), b.decision_function(X[:40]))


def test_stopped_fit_warns(amd):
    from optiml_amd.ml.svm import OneClassSVM
    from optiml_amd.ml.svm._base import ConvergenceWarning
    from optiml_amd.ml.svm.kernels import GaussianKernel
    X = ocr.one_class_data(257, 3)
    with pytest.warns(ConvergenceWarning):
        est = OneClassSVM(kernel=GaussianKernel(gamma=1.0), nu=0.2517, tol=0.0, max_iter=5).fit(X)
    assert est.status_ == 'stopped' and est.n_iter_ == 5 and len(est.train_loss_history) == 6


# ---- 4. one box per column ------------------------------------------------------------------------------------------------------------
FULL, SMALL = 7, 11   # the column whose mass is its whole box, and the one whose mass is below its smallest non-zero box


@functools.lru_cache(maxsize=None)
def _columns17():
    """17 columns (two chunks of 16) on n = 600 rows with five duplicated rows: column c holds out fold c % 3 of three interleaved
    folds (u = 0 there), has nu from a mixed list, and every fourth column has half boxes on every 5th row."""
    n = 600
    X = ocr.one_class_data(n, 3).copy()
    X[300:305] = X[10:15]
    nus = [0.0517, 0.2517, 0.5017, 0.8017, 0.1017, 0.3517]
    UB = np.ones((17, n))
    mass = np.empty(17)
    for c in range(17):
        UB[c, np.arange(n) % 3 == c % 3] = 0.
        if c % 4 == 1:
            UB[c, ::5] *= 0.5
        mass[c] = nus[c % len(nus)] * UB[c].sum()
    mass[FULL] = UB[FULL].sum()
    mass[SMALL] = 0.5 * UB[SMALL][UB[SMALL] > 0].min()
    return X, UB, mass


def test_one_box_per_column(amd):
    """gamma = 1 / 3, tol = 1e-3, max_iter = 60: the columns stop at different iterations, some at the cap.  Held-out rows stay exactly
    0; every column follows the reference on its training rows' sub-matrix (status, iterations, f history to rtol 1e-9); and every
    column's x, g, records and rho have the same bits solved alone and in the reversed batch."""
    from optiml_amd.ml.svm.kernels import GaussianKernel
    from oracle import svm_oracle as so
    X, UB, mass = _columns17()
    n = X.shape[0]
    K = so.gram('rbf', X, gamma=1.0 / 3)
    quad = _quad(X, GaussianKernel(gamma=1.0 / 3))
    dev = quad.device_problem()
    res = _solve(dev, UB, mass, 1e-3, 60)
    assert len({r['iter'] for r in res}) >= 4
    for c, r in enumerate(res):
        tr = UB[c] > 0
        assert np.all(r['x'][~tr] == 0.)
        assert np.all(r['x'] >= 0) and np.all(r['x'] <= UB[c])
        ref = ocr.solve(K[np.ix_(tr, tr)], UB[c][tr], mass[c], tol=1e-3, max_iter=60)
        assert r['status'] == ref['status'] and r['iter'] == ref['iter'], (c, r['status'], r['iter'], ref['status'], ref['iter'])
        np.testing.assert_allclose(r['rows']['f'], ref['rows'][:, 1], rtol=1e-9)
        np.testing.assert_allclose(r['x'][tr], ref['x'], rtol=0, atol=1e-9)
        rho, n_sv, n_free = ocr.rho(r['x'][tr], r['g'][tr], UB[c][tr])   # the reference's statements on the device's state
        assert (r['n_sv'], r['n_free']) == (n_sv, n_free)
        assert r['rho'] == rho   # the same statements in the same order (inf for a column without a row at 0)
    assert res[FULL]['status'] == 'optimal' and res[FULL]['iter'] == 0 and np.array_equal(res[FULL]['x'], UB[FULL])
    assert res[SMALL]['x'].max() < UB[SMALL][UB[SMALL] > 0].min() and abs(res[SMALL]['x'].sum() - mass[SMALL]) <= 1e-12
    order = np.arange(17)[::-1]
    rev = _solve(dev, UB[order], mass[order], 1e-3, 60)
    for j, c in enumerate(order):
        assert _same_bits(rev[j], res[c]), c
    for c in range(17):
        alone = _solve(dev, UB[c], mass[c:c + 1], 1e-3, 60)[0]
        assert _same_bits(alone, res[c]), c
    quad.release()


def test_start_point_and_bad_columns(amd):
    """A start point inside its set is taken as given (the solution: no step is left); one outside it, a mass above its box and a
    problem of another structure are refused."""
    from optiml_amd import _lib
    from optiml_amd.opti import KernelQuadratic
    from optiml_amd.ml.svm._batched import _DeviceSimplexSolver
    from optiml_amd.ml.svm.kernels import GaussianKernel
    X = ocr.one_class_data(257, 3)
    n = 257
    quad = _quad(X, GaussianKernel(gamma=1.0))
    dev = quad.device_problem()
    u = np.ones((1, n))
    a = _solve(dev, u, [0.2517 * n], 1e-6, 1000)[0]
    assert a['status'] == 'optimal'
    # (tol 1e-5: g is formed afresh from x0, and the violation there may differ from the stopped run's in its last digits)
    b = _solve(dev, u, [a['x'].sum()], 1e-5, 1000, x0=a['x'][None, :])[0]
    assert b['status'] == 'optimal' and b['iter'] == 0 and np.array_equal(b['x'], a['x'])
    for UB, mass, x0 in ((u, [n + 1.0], None), (u, [0.0], None), (-u, [1.0], None), (u, [10.0], 2 * u), (u, [10.0], u * 0.5)):
        with pytest.raises(_lib.BcqpError):
            _DeviceSimplexSolver(dev, UB, mass, 1e-3, 10, x0)
    # the start point is the solver's x before any run; after one the direction is served and other vectors are refused
    x0 = np.stack([a['x'], np.full(n, 0.3)])
    s = _DeviceSimplexSolver(dev, np.ones((2, n)), [a['x'].sum(), 0.3 * n], 1e-6, 50, x0)
    for c in range(2):
        assert np.array_equal(s.get(c, _lib.GET_X_NOW), x0[c])
    s.run(5)
    for c in range(2):
        d = s.get(c, _lib.GET_D)
        assert d.shape == (n,) and np.isfinite(d).all()
        with pytest.raises(_lib.BcqpError, match='vector not available'):
            s.get(c, _lib.GET_LP)
    s.close()
    quad.release()
    svc = KernelQuadratic(X, -np.ones(n), 'svc', GaussianKernel(gamma=1.0), y=np.where(np.arange(n) % 2, 1., -1.))
    with pytest.raises(_lib.BcqpError):
        _DeviceSimplexSolver(svc.device_problem(), u, [10.0], 1e-3, 10)
    svc.release()


# ---- 5. the nu path, fp32 panels, the indefinite kernels ----------------------------------------------------------------------------
def test_nu_path_equals_the_single_fits(amd):
    from optiml_amd.ml.svm import OneClassSVM, one_class_nu_path
    from optiml_amd.ml.svm.kernels import GaussianKernel
    X = ocr.one_class_data(600, 8)
    nus = [0.0517, 0.2517, 0.5017, 0.8017, 0.1017]
    proto = OneClassSVM(kernel=GaussianKernel(gamma=0.125), tol=1e-4, max_iter=500)
    path = one_class_nu_path(proto, X, nus)

    class Mine(OneClassSVM):
        pass
    sub = one_class_nu_path(Mine(kernel=GaussianKernel(gamma=0.125), tol=1e-4, max_iter=500), X, nus[:2])
    assert all(type(e) is Mine for e in sub) and np.array_equal(sub[1].alphas_, path[1].alphas_)
    assert [e.nu for e in path] == nus and proto.nu == 0.5 and not hasattr(proto, 'alphas_')
    for est in path:
        one = OneClassSVM(kernel=GaussianKernel(gamma=0.125), nu=est.nu, tol=1e-4, max_iter=500).fit(X)
        assert est.status_ == 'optimal'
        assert np.array_equal(est.alphas_, one.alphas_) and est.offset_ == one.offset_
        assert est.n_iter_ == one.n_iter_ and est.train_loss_history == one.train_loss_history
        assert np.array_equal(est.decision_function(X[:64]), one.decision_function(X[:64]))


def test_fp32_panel(amd):
    """The fp32 panel holds K rounded to fp32 (entries within 1e-6 of the fp64 Gram matrix, the existing batched tests' figure): the
    solve follows the reference on the stored panel.  Against the f64 fit, both at tol 1e-7 so that the panel's rounding is what
    remains: the decision values agree to rtol 1e-4, atol 1e-5, the tolerance of the existing fp32-against-fp64 comparisons (the
    reference on K rounded to fp32 against itself on K: 5.8e-8 at most)."""
    from optiml_amd.ml.svm import OneClassSVM
    from optiml_amd.ml.svm.kernels import GaussianKernel
    from oracle import svm_oracle as so
    n, nu = 600, 0.2517
    X = ocr.one_class_data(n, 8)
    quad = _quad(X, GaussianKernel(gamma=0.125), 'f32')
    K = quad.gram()
    np.testing.assert_allclose(K, so.gram('rbf', X, gamma=0.125), rtol=0, atol=1e-6)
    r = _solve(quad.device_problem(), np.ones((1, n)), [nu * n], 0.0, 15)[0]
    ref = ocr.solve(K, np.ones(n), nu * n, tol=0.0, max_iter=15)
    assert r['status'] == ref['status'] and r['iter'] == ref['iter']
    np.testing.assert_allclose(r['rows']['f'], ref['rows'][:, 1], rtol=1e-9)
    quad.release()
    a = OneClassSVM(kernel=GaussianKernel(gamma=0.125), nu=nu, tol=1e-7, storage='f32').fit(X)
    b = OneClassSVM(kernel=GaussianKernel(gamma=0.125), nu=nu, tol=1e-7).fit(X)
    assert a.status_ == 'optimal' and b.status_ == 'optimal'
    da, db = a.decision_function(X), b.decision_function(X)
    print('fp32 panel against fp64: |decision difference| = %.2e' % np.abs(da - db).max())
    np.testing.assert_allclose(da, db, rtol=1e-4, atol=1e-5)


@pytest.mark.parametrize('kind', ['poly', 'sigmoid'])
def test_indefinite_kernels(amd, kind):
    """A polynomial kernel, and a sigmoid kernel whose Gram matrix is indefinite (smallest eigenvalue about -50): directions of
    non-positive curvature take the branch d'Kd <= 0 (s = 1e10; asserted on the reference's records).  There v = x - 1e10 g is of the
    order 1e12, and a projection that rounded tau into one number would carry ulp(1e12) = 1e-4 into P: both the kernel and the
    reference keep tau as a breakpoint plus an offset."""
    from optiml_amd.ml.svm.kernels import PolyKernel, SigmoidKernel
    from oracle import svm_oracle as so
    n, nu = 600, 0.2517
    X = ocr.one_class_data(n, 3)
    if kind == 'poly':
        kernel, K = PolyKernel(degree=3, gamma=0.5, coef0=1.0), so.gram('poly', X, gamma=0.5, coef0=1.0, degree=3)
    else:
        kernel, K = SigmoidKernel(gamma=1.0, coef0=0.0), so.gram('sigmoid', X, gamma=1.0, coef0=0.0)
    ref = ocr.solve(K, np.ones(n), nu * n, tol=0.0, max_iter=20)
    if kind == 'sigmoid':
        assert (ref['rows'][:, 4] == 1e10).sum() >= 1
    quad = _quad(X, kernel)
    r = _solve(quad.device_problem(), np.ones((1, n)), [nu * n], 0.0, 20)[0]
    assert r['status'] == ref['status'] and r['iter'] == ref['iter']
    np.testing.assert_allclose(r['rows']['f'], ref['rows'][:, 1], rtol=1e-9)
    np.testing.assert_allclose(r['rows']['r3'], ref['rows'][:, 4], rtol=1e-6)
    np.testing.assert_allclose(r['x'], ref['x'], rtol=0, atol=1e-9)
    quad.release()
