"""NuSVCGridSearchCV and NuSVRGridSearchCV on the device: the held-out scoring of the two-group simplex solver's columns
(bq_msolver_simplex2_heldout: msx_fold_kernel, the 16-column product, msx_score_kernel) against the host on the same state, at the
tile edge and its refusals; the searches against sklearn's GridSearchCV over the project's own estimators, with failed fits and on
the fallback path."""
import ctypes as C
import warnings

import numpy as np
import pytest

import test_gpu_nu as tgn
from test_gpu_svr_cv import _compare_results

pytestmark = pytest.mark.gpu

U53 = 2.0 ** -53
KEYS = ('r1', 'r2', 'n_sv', 'n_free', 'n_held', 'n_correct', 'sse')


@pytest.fixture(scope='module')
def amd():
    from optiml_amd import _lib
    from optiml_amd.device import get_context
    _lib.load()
    get_context()


def _solver(dev, S, UB, mass, Q, tol, max_iter):
    from optiml_amd.ml.svm._batched import _DeviceSimplex2Solver
    return _DeviceSimplex2Solver(dev, S, np.atleast_2d(UB), mass, Q, tol, max_iter)


def _finish(solver):
    """run to the end: the records of every column, concatenated over the runs"""
    rows = [[] for _ in range(solver.k)]
    status = ['unknown']
    while 'unknown' in status:
        recs, status = solver.run(256)
        for c in range(solver.k):
            rows[c].append(recs[c])
    return [np.concatenate(r) for r in rows]


def _scored(dev, S, UB, mass, Q, y, tol, max_iter):
    """the columns solved to the end, then offsets(), heldout(y) and the state: per column a dict of KEYS, `off` (offsets()'s four)
    and x"""
    from optiml_amd import _lib
    solver = _solver(dev, S, UB, mass, Q, tol, max_iter)
    try:
        _finish(solver)
        off = solver.offsets()
        held = solver.heldout(y)
        again = solver.offsets()   # the scoring leaves the state as it was
        out = []
        for c in range(solver.k):
            r = {key: held[i][c] for i, key in enumerate(KEYS)}
            r['off'] = tuple(o[c] for o in off)
            r['x'] = solver.get(c, _lib.GET_X_NOW)
            assert all(np.array_equal(a[c], b[c]) for a, b in zip(off, again))
            out.append(r)
        return out
    finally:
        solver.close()


def _same_scores(a, b):
    return all(np.array_equal(a[key], b[key]) for key in KEYS)


def _check_against_host(dev, S, UB, y, res):
    """bq_msolver_simplex2_heldout's figures of every column against the host on the downloaded x.  r1, r2 and the counts are
    offsets()'s, compared with ==.  The product of the folded x through bq_problem_gram_matmat_wide has the device's bits (the same
    16-column product, batch-invariant), and (u - rho) / r rounds identically in NumPy, so n_held and n_correct are compared with ==.
    The squared error sums the same terms in another order: a sum of m <= n non-negative terms in any order is within
    (m - 1) 2^-53 of the exact one relatively, so two orders differ by less than 2 n 2^-53 sse; twice that covers the square's and
    a fused multiply-add's roundings."""
    from optiml_amd.ml.svm._batched import _gram_matmat
    k, n = len(res), len(y)
    paired = S is None
    if paired:
        B = np.stack([r['x'][:n] - r['x'][n:] for r in res])
    else:
        B = np.stack([np.where(UB[c] > 0, S[c], 1.) * r['x'] for c, r in enumerate(res)])   # (the device's labels are +1 where ub = 0)
    U = _gram_matmat(dev, B, wide=True)
    for c, r in enumerate(res):
        r1, r2, n_sv, n_free = r['off']
        assert r['r1'] == r1 and r['r2'] == r2 and np.array_equal(r['n_sv'], n_sv) and np.array_equal(r['n_free'], n_free)
        te = (UB[c][:n] == 0) & (UB[c][n:] == 0) if paired else UB[c] == 0
        assert te.sum() > 0 and r['n_held'] == te.sum()
        rho, scale = (r1 - r2) / 2, (r1 + r2) / 2
        if paired:
            sse = float(((y[te] - (U[c][te] - rho)) ** 2).sum())
            print('column %d: |sse_dev - sse_host| = %.3e (bound %.3e)' % (c, abs(r['sse'] - sse), 4 * n * U53 * sse))
            assert abs(r['sse'] - sse) <= 4 * n * U53 * sse and sse > 0
            assert r['n_correct'] == 0
        else:
            pred = np.where((U[c] - rho) / scale > 0, 1., -1.)
            assert r['n_correct'] == int((pred[te] == y[te]).sum()) and 0 < r['n_correct'] <= r['n_held']
            assert r['sse'] == 0.


# ---- 1. device scoring against the host on the same state ---------------------------------------------------------------------------
@pytest.mark.parametrize('paired', [False, True], ids=['labels', 'paired'])
def test_device_scoring_against_the_host(amd, paired):
    """The 17 columns of test_gpu_nu._columns17 (n = 600, three interleaved folds, mixed parameters, 60 iterations): the figures
    against the host; every column scored alone and in the reversed batch has the same bits; and a run after the call continues to
    the records, x and g of a solver that was never scored."""
    from optiml_amd import _lib
    from optiml_amd.ml.svm.kernels import GaussianKernel
    X, S, UB, mass, Q = tgn._columns17(paired)
    _, yc, t = tgn._data(600, 17)
    y = t if paired else yc
    tol = 0.1 if paired else 1e-3
    quad = tgn._quad(X, GaussianKernel(gamma=1.0 / 3))
    dev = quad.device_problem()
    sub = lambda A, rows: None if A is None else A[rows]   # noqa: E731
    res = _scored(dev, S, UB, mass, Q, y, tol, 60)
    _check_against_host(dev, S, UB, y, res)
    assert all(r['n_held'] == 200 for r in res)
    order = np.arange(17)[::-1]
    rev = _scored(dev, sub(S, order), UB[order], mass[order], sub(Q, order), y, tol, 60)
    for j, c in enumerate(order):
        assert _same_scores(rev[j], res[c]), c
    for c in range(17):
        one = slice(c, c + 1)
        alone = _scored(dev, sub(S, one), UB[one], mass[one], sub(Q, one), y, tol, 60)[0]
        assert _same_scores(alone, res[c]), c
    # 20 iterations, the scoring of one of two solvers, then both to the end
    a, b = (_solver(dev, S, UB, mass, Q, tol, 60) for _ in range(2))
    first = [s.run(20)[0] for s in (a, b)]
    mid = a.heldout(y)
    assert any(m != f for m, f in zip(mid[0], [r['r1'] for r in res]))   # (scored mid-way: another state than the end's)
    rest = [_finish(s) for s in (a, b)]
    assert sum(len(r) for r in rest[0]) > 0
    for c in range(17):
        assert first[0][c].tobytes() == first[1][c].tobytes() and rest[0][c].tobytes() == rest[1][c].tobytes()
        for what in (_lib.GET_X_NOW, _lib.GET_G_NOW):
            assert np.array_equal(a.get(c, what), b.get(c, what))
        assert a.state(c) == b.state(c)
    end = a.heldout(y)
    for c in range(17):
        assert all(np.array_equal(end[i][c], res[c][key]) for i, key in enumerate(KEYS))
    a.close()
    b.close()
    quad.release()


# ---- 2. the tile edge ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('paired', [False, True], ids=['labels', 'paired'])
@pytest.mark.parametrize('n', [256, 257])
def test_device_scoring_one_column_at_the_tile_edge(amd, n, paired):
    """One column on exactly one tile and on one row more (a second tile row of one row), a third of the rows held out."""
    from optiml_amd.ml.svm.kernels import GaussianKernel
    X, yc, t = tgn._data(n, 3)
    mask = np.ones((1, n))
    mask[0, np.arange(n) % 3 == 1] = 0.
    quad = tgn._quad(X, GaussianKernel(gamma=1.0 / 3))
    dev = quad.device_problem()
    if paired:
        UB, mass, Q = tgn._paired_columns(t, [(1.0, 0.5017)], mask)
        S, y = None, t
    else:
        S, UB, mass = tgn._labels_columns(yc, [0.5017], mask)
        Q, y = None, yc
    res = _scored(dev, S, UB, mass, Q, y, 1e-3, 60)
    assert res[0]['n_held'] == np.count_nonzero(mask == 0)
    _check_against_host(dev, S, UB, y, res)
    quad.release()


# ---- 3. refusals --------------------------------------------------------------------------------------------------------------------
def _raw_heldout(solver, n):
    """bq_msolver_simplex2_heldout on any solver's handle, with valid arrays: the return code"""
    from optiml_amd import _lib
    k = solver.k
    y = np.ones(n)
    d = [np.empty(k) for _ in range(3)]
    i = [np.empty(2 * k, dtype=np.int64) for _ in range(4)]
    p64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int64))   # noqa: E731
    return _lib.load().bq_msolver_simplex2_heldout(solver._h, _lib.ptr(y), _lib.ptr(d[0]), _lib.ptr(d[1]), p64(i[0]), p64(i[1]),
                                                   p64(i[2]), p64(i[3]), _lib.ptr(d[2]))


def test_refusals(amd):
    from optiml_amd import _lib
    from optiml_amd.ml.svm._batched import _DeviceMultiSolver, _DeviceSimplexPairSolver, _DeviceSimplexSolver
    from optiml_amd.ml.svm.kernels import GaussianKernel
    from optiml_amd.ml.svm.onevsone import sort_plan
    from optiml_amd.opti import KernelQuadratic
    n = 257
    X, yc, t = tgn._data(n, 3)
    quad = tgn._quad(X, GaussianKernel(gamma=1.0 / 3))
    dev = quad.device_problem()

    def refused(call):
        with pytest.raises(_lib.BcqpError) as e:
            call()
        assert e.value.code == _lib.ERR_BADARG

    one = _DeviceSimplexSolver(dev, np.ones((1, n)), [0.5 * n], 1e-3, 10)   # the ONE layout
    one.run(5)
    assert _raw_heldout(one, n) == _lib.ERR_BADARG
    one.close()
    S, UB, mass = tgn._labels_columns(yc, [0.5017])
    labels = _solver(dev, S, UB, mass, None, 1e-3, 10)
    refused(lambda: labels.heldout(yc))   # before its first run
    labels.run(5)
    assert labels.heldout(yc)[4][0] == 0   # (no row is held out)
    bad = yc.copy()
    bad[100] = 0.
    refused(lambda: labels.heldout(bad))
    labels.close()
    UB2, mass2, Q = tgn._paired_columns(t, [(1.0, 0.5017)])
    paired = _solver(dev, None, UB2, mass2, Q, 1e-3, 10)
    paired.run(5)
    assert paired.heldout(t)[4][0] == 0
    bad = t.copy()
    bad[100] = np.nan
    refused(lambda: paired.heldout(bad))
    paired.close()
    quad.release()
    # a pair-routed simplex solver on a class-sorted panel
    codes = (yc > 0).astype(int)
    index, ct, n_pad = sort_plan(codes, 2)
    Xp = np.zeros((n_pad, X.shape[1]))
    Xp[index] = X
    box = np.zeros((1, n_pad))
    box[0, index] = 1.
    pq = KernelQuadratic(Xp, np.zeros(n_pad), 'plain', GaussianKernel(gamma=1.0 / 3))
    pairs = _DeviceSimplexPairSolver(pq.device_problem(), ct, [(0, 1)], box, [[30.0, 30.0]], 1e-3, 10)
    pairs.run(5)
    refused(lambda: pairs.heldout(np.ones(n_pad)))
    pairs.close()
    pq.release()
    # a one-box-per-column ProjectedGradient solver
    svc = KernelQuadratic(X, -np.ones(n), 'svc', GaussianKernel(gamma=1.0 / 3), y=yc)
    boxes = _DeviceMultiSolver(svc.device_problem(), _lib.PG, yc[None, :], np.ones((1, n)), 1e-6, 10)
    boxes.run(5)
    assert _raw_heldout(boxes, n) == _lib.ERR_BADARG
    boxes.close()
    svc.release()


# ---- 4. the searches against GridSearchCV over the project's own estimators ----------------------------------------------------------
SVC_NUS = [0.3517, 0.5017, 0.7017, 0.9517]
SVR_GRID = {'C': [0.5, 1], 'nu': [0.2517, 0.8017]}
KW = dict(tol=1e-3, max_iter=60)


def _case(case, grid):
    from optiml_amd.ml.svm.kernels import GaussianKernel
    third = GaussianKernel(gamma=1.0 / 3)
    return {
        'gauss-num': (dict(KW, kernel=third), grid),
        'gauss-scale': (dict(KW, kernel=GaussianKernel(gamma='scale')), grid),
        'gauss-num-f32': (dict(KW, kernel=third, storage='f32'), grid),
        # the second kernel is test_gpu_nu's TRAJ_GAMMA: of gamma = 0.1, 1, 3 and the linear kernel it is the one at which the NumPy
        # reference's own held-out R^2 after 60 iterations moves least under one ulp per entry of K (at most 2.8e-13 over the 12 NuSVR
        # fits; 1.2e-9 at gamma = 1, 1.1e-9 at 0.1, 5.8e-7 for the linear kernel), and its smallest NuSVC held-out |u - rho| is 2.0e-3
        'kernels': (KW, dict(grid, kernel=[third, GaussianKernel(gamma=3.0)])),
    }[case]


CASES = ['gauss-num', 'gauss-scale', 'gauss-num-f32', 'kernels']


def _reference_search(est, grid, cv, X, y):
    """GridSearchCV over the project's estimator; its warnings (a stopped fit's, a failed fit's) are its own"""
    from sklearn.model_selection import GridSearchCV
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        return GridSearchCV(est, grid, cv=cv).fit(X, y)


def _fit_search(search, X, y):
    from optiml_amd.ml.svm._base import ConvergenceWarning
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter('always')
        search.fit(X, y)
    stopped = [w for w in caught if issubclass(w.category, ConvergenceWarning)]
    # one for the search if any fit ends 'stopped', and the refit's own
    assert len(stopped) == int((search.status_ == 'stopped').any()) + int(search.best_estimator_.status_ == 'stopped')
    return search, caught


def _shape_checks(ours, ref, ns):
    nc = len(ours.cv_results_['params'])
    assert ours.cv_results_['params'] == ref.cv_results_['params'] and ours.n_splits_ == ns
    assert ours.n_iter_.shape == ours.status_.shape == (nc, ns)
    return nc


@pytest.mark.parametrize('case', CASES)
def test_nu_svc_search_equals_grid_search_cv(amd, case):
    """_data(400, 7), StratifiedKFold(3), tol 1e-3, max_iter 60, nu in SVC_NUS: split scores, means, stds, ranks, best_* and the
    best estimator's predictions at rtol 1e-9 / atol 1e-9.  The accuracies are quotients of small integers and must be EQUAL when no
    held-out decision value is within rounding of 0: on the reference fits (GridSearchCV's per-fold NuSVC, every one of them) every
    held-out |decision_function| margin_scale_ is asserted to be >= 1e-6, where the two paths' u differ by about the 1e-9 of x."""
    pytest.importorskip('sklearn')
    from sklearn.model_selection import StratifiedKFold
    from optiml_amd.ml.svm import NuSVC, NuSVCGridSearchCV
    from optiml_amd.ml.svm.model_selection import parameter_grid
    kw, grid = _case(case, {'nu': SVC_NUS})
    X, y, _ = tgn._data(400, 7)
    ours, _ = _fit_search(NuSVCGridSearchCV(NuSVC(**kw), grid, cv=3), X, y)   # an int: StratifiedKFold(3)
    assert ours.batched_ is True
    cv = StratifiedKFold(3)
    ref = _reference_search(NuSVC(**kw), grid, cv, X, y)
    nc = _shape_checks(ours, ref, 3)
    assert (ours.n_iter_ > 0).all() and set(ours.status_.ravel()) <= {'optimal', 'stopped'}
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        for ci, p in enumerate(parameter_grid(grid)):
            for f, (tr, te) in enumerate(cv.split(X, y)):
                fold = NuSVC(**kw).set_params(**p).fit(X[tr], y[tr])
                margin = float(np.abs(fold.decision_function(X[te])).min() * fold.margin_scale_)
                assert margin >= 1e-6, (ci, f, margin)
    for i in range(3):
        key = 'split%d_test_score' % i
        assert np.array_equal(ours.cv_results_[key], ref.cv_results_[key]), key
    _compare_results(ours, ref, 3)
    assert nc == len(SVC_NUS) * (2 if case == 'kernels' else 1)
    Xte = tgn._data(600, 7)[0][400:]
    assert np.array_equal(ours.best_estimator_.predict(Xte), ref.best_estimator_.predict(Xte))
    assert np.array_equal(ours.predict(Xte), ours.best_estimator_.predict(Xte))
    assert np.array_equal(ours.decision_function(Xte), ours.best_estimator_.decision_function(Xte))
    assert ours.score(X, y) == ours.best_estimator_.score(X, y)


@pytest.mark.parametrize('case', CASES)
def test_nu_svr_search_equals_grid_search_cv(amd, case):
    """The same data's targets, KFold(3), (C, nu) in {0.5, 1} x {0.2517, 0.8017}: the comparison of test_gpu_svr_cv._compare_results at
    rtol 1e-9 / atol 1e-9, and the best estimator's predictions to rtol 1e-9.

    'gauss-scale' has one panel per fold, and the search puts the fold's training rows first on it: its columns then follow the
    fold's own fit (scores equal to 1.2e-16 on an MI355X).  That matters: fold 0 of (C = 1, nu = 0.8017) is 'stopped' at an iterate
    far from the optimum (R^2 0.53, its neighbours 0.90) that the arithmetic does not determine to 1e-9 -- the NumPy reference's own
    R^2 of it moves by 5.9e-9 under one ulp per entry of K, and on a panel in the data's row order it came out 1.48e-8 away.  On a
    panel shared by the folds (the other cases) the two paths differ by the summation order of their products: at most 1.7e-10
    here."""
    pytest.importorskip('sklearn')
    from sklearn.model_selection import KFold
    from optiml_amd.ml.svm import NuSVR, NuSVRGridSearchCV
    kw, grid = _case(case, SVR_GRID)
    X, _, t = tgn._data(400, 7)
    ours, _ = _fit_search(NuSVRGridSearchCV(NuSVR(**kw), grid, cv=3), X, t)   # an int: KFold(3)
    assert ours.batched_ is True
    ref = _reference_search(NuSVR(**kw), grid, KFold(3), X, t)
    nc = _shape_checks(ours, ref, 3)
    assert nc == 4 * (2 if case == 'kernels' else 1)
    assert (ours.n_iter_ > 0).all() and set(ours.status_.ravel()) <= {'optimal', 'stopped'}
    _compare_results(ours, ref, 3)
    Xte = tgn._data(600, 7)[0][400:]
    np.testing.assert_allclose(ours.best_estimator_.predict(Xte), ref.best_estimator_.predict(Xte), rtol=1e-9)
    np.testing.assert_allclose(ours.predict(Xte), ours.best_estimator_.predict(Xte), rtol=0)
    assert ours.score(X, t) == ours.best_estimator_.score(X, t)


# ---- 5. failed fits -----------------------------------------------------------------------------------------------------------------
def test_failed_fits_score_nan_and_rank_last(amd):
    """_data(257, 3) has 144 / 113 labels: nu = 0.9517 is infeasible on every stratified fold's training labels.  Its scores are NaN,
    it ranks last, one RuntimeWarning names the failed fits, and the result is GridSearchCV's; nu = 0.9517 alone raises ValueError."""
    pytest.importorskip('sklearn')
    from sklearn.model_selection import StratifiedKFold
    from optiml_amd.ml.svm import NuSVC, NuSVCGridSearchCV
    from optiml_amd.ml.svm.kernels import GaussianKernel
    kw = dict(KW, kernel=GaussianKernel(gamma=1.0 / 3))
    X, y, _ = tgn._data(257, 3)
    assert sorted(np.unique(y, return_counts=True)[1]) == [113, 144]
    grid = {'nu': [0.5017, 0.9517]}
    ours, caught = _fit_search(NuSVCGridSearchCV(NuSVC(**kw), grid, cv=3), X, y)
    failed = [w for w in caught if issubclass(w.category, RuntimeWarning)]
    assert len(failed) == 1 and '3 fits failed' in str(failed[0].message)
    assert ours.batched_ is True
    ref = _reference_search(NuSVC(**kw), grid, StratifiedKFold(3), X, y)
    _shape_checks(ours, ref, 3)
    for i in range(3):
        key = 'split%d_test_score' % i
        assert np.isnan(ours.cv_results_[key][1]) and np.isnan(ref.cv_results_[key][1])
        assert ours.cv_results_[key][0] == ref.cv_results_[key][0]
    assert np.isnan(ours.cv_results_['mean_test_score'][1]) and np.isnan(ours.cv_results_['std_test_score'][1])
    assert list(ours.cv_results_['rank_test_score']) == list(ref.cv_results_['rank_test_score']) == [1, 2]
    assert list(ours.n_iter_[1]) == [-1] * 3 and list(ours.status_[1]) == ['failed'] * 3 and (ours.n_iter_[0] > 0).all()
    assert ours.best_index_ == ref.best_index_ == 0 and ours.best_params_ == ref.best_params_ == {'nu': 0.5017}
    assert ours.best_score_ == ref.best_score_
    _compare_results(ours, ref, 3)
    with pytest.raises(ValueError, match='fits failed'):
        NuSVCGridSearchCV(NuSVC(**kw), {'nu': [0.9517]}, cv=3).fit(X, y)


# ---- 6. the fallback ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('which', ['svc', 'svr'])
def test_fallback_equals_grid_search_cv(amd, which):
    pytest.importorskip('sklearn')
    from sklearn.model_selection import KFold, StratifiedKFold
    from optiml_amd.ml.svm import NuSVC, NuSVCGridSearchCV, NuSVR, NuSVRGridSearchCV
    from optiml_amd.ml.svm.kernels import GaussianKernel
    kw = dict(kernel=GaussianKernel(gamma=1.0 / 3), max_iter=60)
    X, y, t = tgn._data(150, 5)
    grid = {'nu': [0.3517, 0.5017], 'tol': [1e-2, 1e-3]}
    if which == 'svc':
        ours, _ = _fit_search(NuSVCGridSearchCV(NuSVC(**kw), grid, cv=3), X, y)
        ref = _reference_search(NuSVC(**kw), grid, StratifiedKFold(3), X, y)
    else:
        ours, _ = _fit_search(NuSVRGridSearchCV(NuSVR(**kw), grid, cv=3), X, t)
        ref = _reference_search(NuSVR(**kw), grid, KFold(3), X, t)
    assert ours.batched_ is False
    for i in range(3):
        assert np.array_equal(ours.cv_results_['split%d_test_score' % i], ref.cv_results_['split%d_test_score' % i])
    assert ours.best_params_ == ref.best_params_ and ours.n_iter_.shape == (4, 3) and (ours.n_iter_ > 0).all()
