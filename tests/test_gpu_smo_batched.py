"""GPU tests of the batched SMO (`bq_msmo_*`, csrc/bq_smo.hip: one walker workgroup per column on one Gram panel) through
`_DeviceSMOSolver` / `solve_batched_smo` and the estimators that take it.

A column IS the single solver's walker on that column's data (one copy of the walker, no helper workgroups; the helpers do
not change the single solver's bits, tests/test_gpu_smo.py), so against a single fit on the same panel the bar is equality
of bits (`np.array_equal`).  A column with a row list is the single solver of the sub-problem on those rows; the device has
no such single solver, so those columns are held step for step to the CPU oracle with the kernel's tie rule and summation
order on the device's own Gram entries (rtol 1e-12, test_gpu_smo.py's bar (1)).
"""
import ctypes as C

import numpy as np
import pytest

from conftest import load_golden

pytestmark = pytest.mark.gpu

SMO_CAP = 4096   # csrc/bq_smo.hip: entries of the support list mirrored in LDS
SVC_FIELDS = ('alphas', 'errors', 'b', 'b_up', 'b_low', 'b_up_idx', 'b_low_idx', 'iter', 'steps')
SVR_FIELDS = ('alphas_p', 'alphas_n') + SVC_FIELDS[1:]


@pytest.fixture(scope='module')
def amd():
    import optiml_amd
    from optiml_amd import _lib
    from optiml_amd.device import get_context
    _lib.load()
    get_context()
    return optiml_amd


def _kernel(kname):
    from optiml_amd.ml.svm.kernels import gaussian, linear
    return {'rbf': gaussian, 'linear': linear}[kname]


def _svc_data(n):
    g = load_golden('smo.npz')
    X, y = g[f'svc{n}_X'], g[f'svc{n}_y']
    return X, np.where(y == np.unique(y)[-1], 1., -1.)


def _svr_data(n):
    g = load_golden('smo.npz')
    return g[f'svr{n}_X'], g[f'svr{n}_y']


def _svc_quad(X, yb, kname, **kw):
    from optiml_amd.opti import KernelQuadratic
    return KernelQuadratic(X, -np.ones(len(yb)), 'svc', _kernel(kname), y=yb, rank_one=False, **kw)


def _svr_quad(X, y, kname, **kw):
    from optiml_amd.opti import KernelQuadratic
    return KernelQuadratic(X, np.hstack((-y, y)) + 0.1, 'svr', _kernel(kname), rank_one=False, **kw)


def _same(r, opt, fields, what):
    for f in fields:
        assert np.array_equal(r[f], getattr(opt, f)), (what, f)


def _folds(n):
    idx = np.arange(n)
    return [(np.setdiff1d(idx, idx[f::3]), idx[f::3]) for f in range(3)]


@pytest.fixture(scope='module')
def svc600_oracle(amd):
    """svc600 RBF: the device's Gram matrix and, per (fold, C), the oracle's fit on the fold's training rows — computed once,
    shared by the row-list test and the search test, which leave it unchanged."""
    from oracle import smo_oracle as smo
    X, yb = _svc_data(600)
    quad = _svc_quad(X, yb, 'rbf')
    Kdev = quad.gram()
    quad.release()
    fits = {}
    for f, (tr, _) in enumerate(_folds(600)):
        for Cv in (0.1, 1., 10.):
            fits[f, Cv] = smo.smo_svc(Kdev[tr][:, tr], yb[tr], C=Cv, tol=1e-3, tie='index', dot='tree')
    return X, yb, Kdev, fits


# ---- 1. a column is the single fit, bit for bit -----------------------------------------------------------------------------------
@pytest.mark.parametrize('full', [False, True], ids=['packed', 'square'])
@pytest.mark.parametrize('kname', ['rbf', 'linear'])
@pytest.mark.parametrize('n', [200, 600])
def test_svc_columns_equal_single_fits(amd, n, kname, full):
    from optiml_amd import _lib
    from optiml_amd.ml.svm._batched import solve_batched_smo
    from optiml_amd.ml.svm.smo import SMOClassifier
    X, yb = _svc_data(n)
    quad = _svc_quad(X, yb, kname, full_panel=full)
    Cs = [0.1, 0.3, 1., 3., 10., 1.]
    Y = np.stack([yb] * 5 + [-yb])   # the last column: the labels flipped
    res = solve_batched_smo(quad.device_problem(), _lib.SVC, Y, Cs, None, 1e-3)
    assert len({r['iter'] for r in res}) > 1   # the columns are different problems
    for c, r in enumerate(res):
        one = SMOClassifier(quad, X, Y[c], None, _kernel(kname), Cs[c], 1e-3).minimize()
        _same(r, one, SVC_FIELDS, c)


@pytest.mark.parametrize('full', [False, True], ids=['packed', 'square'])
@pytest.mark.parametrize('kname', ['rbf', 'linear'])
@pytest.mark.parametrize('n', [150, 400])
def test_svr_columns_equal_single_fits(amd, n, kname, full):
    from optiml_amd import _lib
    from optiml_amd.ml.svm._batched import solve_batched_smo
    from optiml_amd.ml.svm.smo import SMORegression
    X, y = _svr_data(n)
    quad = _svr_quad(X, y, kname, full_panel=full)
    Cs, eps = [0.1, 1., 0.3, 1., 3.], [0.05, 0.1, 0.2, 0., 0.3]
    Y = np.stack([y, y, y, y, -2. * y])
    res = solve_batched_smo(quad.device_problem(), _lib.SVR, Y, Cs, eps, 1e-3)
    for c, r in enumerate(res):
        one = SMORegression(quad, X, Y[c], None, _kernel(kname), Cs[c], eps[c], 1e-3).minimize()
        _same(r, one, SVR_FIELDS, c)


def test_fp32_panel_columns_equal_single_fits(amd):
    from optiml_amd import _lib
    from optiml_amd.ml.svm._batched import solve_batched_smo
    from optiml_amd.ml.svm.smo import SMOClassifier
    X, yb = _svc_data(200)
    quad = _svc_quad(X, yb, 'rbf', storage='f32')
    Cs = [0.1, 1., 10.]
    res = solve_batched_smo(quad.device_problem(), _lib.SVC, np.stack([yb] * 3), Cs, None, 1e-3)
    for c, r in enumerate(res):
        _same(r, SMOClassifier(quad, X, yb, None, _kernel('rbf'), Cs[c], 1e-3).minimize(), SVC_FIELDS, c)


# ---- 2. outer-iteration lockstep --------------------------------------------------------------------------------------------------
def _single_outer_states(quad, task, y, Cv, eps, tol, pull):
    """the single solver one outer iteration at a time: [(alphas, b_up, b_low)] after every call, to its end"""
    from optiml_amd import _lib
    lib = _lib.load()
    h = C.c_void_p()
    _lib.check(lib.bq_smo_create(quad.device_problem().handle, task, _lib.ptr(np.ascontiguousarray(y)), float(Cv), float(eps),
                                 float(tol), C.byref(h)))
    states = []
    outer, fin = C.c_int64(0), C.c_int(0)
    try:
        while not fin.value:
            _lib.check(lib.bq_smo_run(h, 1, C.byref(outer), C.byref(fin)))
            a, sc = np.empty(pull), np.empty(6)
            _lib.check(lib.bq_smo_get(h, _lib.SMO_ALPHAS, _lib.ptr(a)))
            _lib.check(lib.bq_smo_get(h, _lib.SMO_SCALARS, _lib.ptr(sc)))
            states.append((a, sc[0], sc[1]))
    finally:
        lib.bq_smo_destroy(h)
    return states


@pytest.mark.parametrize('task', ['svc', 'svr'])
def test_outer_iterations_in_lockstep(amd, task):
    from optiml_amd import _lib
    from optiml_amd.ml.svm._batched import _DeviceSMOSolver
    Cs = [0.1, 1., 10.]
    if task == 'svc':
        X, y = _svc_data(200)
        quad, code, eps, pull = _svc_quad(X, y, 'rbf'), _lib.SVC, [0., 0., 0.], 200
    else:
        X, y = _svr_data(150)
        quad, code, eps, pull = _svr_quad(X, y, 'rbf'), _lib.SVR, [0.05, 0.1, 0.2], 300
    ref = [_single_outer_states(quad, code, y, Cs[c], eps[c], 1e-3, pull) for c in range(3)]
    assert len({len(r) for r in ref}) > 1   # the columns finish at different counts
    solver = _DeviceSMOSolver(quad.device_problem(), code, np.stack([y] * 3), Cs, eps, 1e-3)
    try:
        for call in range(1, max(len(r) for r in ref) + 1):
            outer, fin, failed = solver.run(1)
            assert not failed.any()
            for c in range(3):
                done = min(call, len(ref[c]))   # a finished column no longer moves
                a, up, low = ref[c][done - 1]
                sc = solver.get(c, _lib.SMO_SCALARS)
                assert outer[c] == done and bool(fin[c]) == (call >= len(ref[c])), (call, c)
                assert np.array_equal(solver.get(c, _lib.SMO_ALPHAS), a) and sc[0] == up and sc[1] == low, (call, c)
        assert fin.all()
    finally:
        solver.close()


# ---- 3. row lists against the oracle, step for step --------------------------------------------------------------------------------
def test_svc_row_lists_follow_the_oracle(amd, svc600_oracle):
    from optiml_amd import _lib
    from optiml_amd.ml.svm._batched import solve_batched_smo
    X, yb, Kdev, fits = svc600_oracle
    quad = _svc_quad(X, yb, 'rbf')
    cols = [(f, Cv) for f in range(3) for Cv in (0.1, 1., 10.)]
    folds = _folds(600)
    rows = [folds[f][0] for f, _ in cols] + [np.arange(600)]   # the last column: the identity list
    Cs = [Cv for _, Cv in cols] + [1.]
    res = solve_batched_smo(quad.device_problem(), _lib.SVC, np.stack([yb] * 10), Cs, None, 1e-3, rows=rows)
    for (f, Cv), r in zip(cols, res):
        tr, te = folds[f]
        ref = fits[f, Cv]
        assert r['iter'] == ref['iter'] and r['steps'] == ref['steps'], (f, Cv)
        np.testing.assert_allclose(r['alphas'][tr], ref['alphas'], rtol=1e-12, atol=1e-15)
        np.testing.assert_allclose([r['b'], r['b_up'], r['b_low']], [ref['b'], ref['b_up'], ref['b_low']], rtol=1e-12, atol=1e-15)
        assert not r['alphas'][te].any()   # an unlisted row is never examined
    # the identity list takes the null list's path: same bits as a column without a list
    null = solve_batched_smo(quad.device_problem(), _lib.SVC, yb[None], [1.], None, 1e-3)[0]
    for f in SVC_FIELDS:
        assert np.array_equal(res[9][f], null[f]), f


def test_identity_list_and_null_list_in_one_solve(amd):
    """rows=None is every column on all rows; a solve with lists whose columns all carry the identity equals it bit for bit"""
    from optiml_amd import _lib
    from optiml_amd.ml.svm._batched import solve_batched_smo
    X, yb = _svc_data(200)
    quad = _svc_quad(X, yb, 'rbf')
    a = solve_batched_smo(quad.device_problem(), _lib.SVC, np.stack([yb, -yb]), [1., 3.], None, 1e-3)
    b = solve_batched_smo(quad.device_problem(), _lib.SVC, np.stack([yb, -yb]), [1., 3.], None, 1e-3, rows=[np.arange(200)] * 2)
    for ra, rb in zip(a, b):
        for f in SVC_FIELDS:
            assert np.array_equal(ra[f], rb[f]), f


def test_svr_row_lists_follow_the_oracle(amd):
    from oracle import smo_oracle as smo
    from optiml_amd import _lib
    from optiml_amd.ml.svm._batched import solve_batched_smo
    X, y = _svr_data(400)
    quad = _svr_quad(X, y, 'rbf')
    Kdev = quad.gram()
    idx = np.arange(400)
    folds = [(np.setdiff1d(idx, idx[f::2]), idx[f::2]) for f in range(2)]
    res = solve_batched_smo(quad.device_problem(), _lib.SVR, np.stack([y] * 2), [1., 1.], [0.1, 0.1], 1e-3,
                            rows=[tr for tr, _ in folds])
    for (tr, te), r in zip(folds, res):
        ref = smo.smo_svr(Kdev[tr][:, tr], y[tr], C=1., epsilon=0.1, tol=1e-3, tie='index', dot='tree')
        assert r['iter'] == ref['iter'] and r['steps'] == ref['steps']
        np.testing.assert_allclose(r['alphas_p'][tr], ref['alphas_p'], rtol=1e-12, atol=1e-15)
        np.testing.assert_allclose(r['alphas_n'][tr], ref['alphas_n'], rtol=1e-12, atol=1e-15)
        np.testing.assert_allclose([r['b'], r['b_up'], r['b_low']], [ref['b'], ref['b_up'], ref['b_low']], rtol=1e-12, atol=1e-15)
        assert not r['alphas_p'][te].any() and not r['alphas_n'][te].any()


# ---- 4. more columns than CUs -----------------------------------------------------------------------------------------------------
def test_more_columns_than_compute_units(amd):
    from optiml_amd import _lib
    from optiml_amd.ml.svm._batched import solve_batched_smo
    from optiml_amd.ml.svm.smo import SMOClassifier
    X, yb = _svc_data(200)
    quad = _svc_quad(X, yb, 'rbf')
    Cs = np.logspace(-1, 1, 300)
    res = solve_batched_smo(quad.device_problem(), _lib.SVC, np.stack([yb] * 300), Cs, None, 1e-3)
    assert len(res) == 300 and all(r['iter'] >= 2 for r in res)   # every column ran to its end
    for c in (0, 255, 256, 299):
        _same(res[c], SMOClassifier(quad, X, yb, None, _kernel('rbf'), Cs[c], 1e-3).minimize(), SVC_FIELDS, c)
    # the split into several solves changes no bits
    part = solve_batched_smo(quad.device_problem(), _lib.SVC, np.stack([yb] * 300)[250:], Cs[250:], None, 1e-3, cap=7)
    for c in (5, 6, 49):
        for f in SVC_FIELDS:
            assert np.array_equal(part[c][f], res[250 + c][f]), (c, f)


# ---- 5. a support list past the LDS mirror, in a column other than 0 ----------------------------------------------------------------
def test_support_list_past_the_lds_mirror_in_column_one(amd):
    from optiml_amd import _lib
    from optiml_amd.ml.svm._batched import solve_batched_smo
    from optiml_amd.ml.svm.smo import SMOClassifier
    rs = np.random.RandomState(11)
    X = rs.standard_normal((4800, 10))
    Y = np.stack([np.where(X[:, 0] > 0, 1., -1.), np.where(rs.uniform(size=4800) < 0.5, 1., -1.)])
    quad = _svc_quad(X, Y[1], 'rbf')
    res = solve_batched_smo(quad.device_problem(), _lib.SVC, Y, [0.1, 0.1], None, 1e-2)
    nnz = [int(np.count_nonzero(r['alphas'])) for r in res]
    print('nonzero multipliers per column:', nnz, 'outer iterations:', [r['iter'] for r in res])
    assert nnz[1] > SMO_CAP
    _same(res[1], SMOClassifier(quad, X, Y[1], None, _kernel('rbf'), 0.1, 1e-2).minimize(), SVC_FIELDS, 1)


# ---- 6. estimators ------------------------------------------------------------------------------------------------------------------
def test_one_vs_rest_equals_one_svc_per_class(amd):
    from optiml_amd.datasets import make_multiclass_blobs
    from optiml_amd.ml.svm import SVC, OneVsRestSVC
    from optiml_amd.ml.svm.kernels import GaussianKernel
    from optiml_amd.ml.svm.losses import hinge, squared_hinge
    X, y = make_multiclass_blobs(600, 6, 4, seed=5)
    kw = dict(loss=hinge, kernel=GaussianKernel(gamma=0.2), C=1., dual=True, optimizer='smo', tol=1e-3)
    est = OneVsRestSVC(**kw)
    est.batch_smo = True
    est.fit(X, y)
    assert est.batched_ is True and est.smo_ is True and len(est.estimators_) == 4
    for c, e in enumerate(est.estimators_):
        one = SVC(**kw).fit(X, (y == est.classes_[c]).astype(int))
        assert np.array_equal(e.alphas_, one.alphas_) and e.intercept_ == one.intercept_
        assert np.array_equal(e.support_, one.support_) and e.optimizer.iter == one.optimizer.iter
        assert np.array_equal(e.dual_coef_, one.dual_coef_) and e.optimizer.steps == one.optimizer.steps
        assert e.optimizer.helper_stats == dict(helpers=0, delivered=0, rejected_list_hash=0, rejected_checksum=0)
    Xt = X[::7] + 0.01
    per = np.stack([e.decision_function(Xt) for e in est.estimators_], axis=1)
    assert est.batched_decision_ is True
    np.testing.assert_allclose(est.decision_function(Xt), per, rtol=0, atol=1e-10)
    # the per-class path on the same commit: the same estimators
    loop = OneVsRestSVC(**kw)
    loop.batch_smo = False
    loop.fit(X, y)
    assert loop.batched_ is False and loop.smo_ is False
    for a, b in zip(est.estimators_, loop.estimators_):
        assert np.array_equal(a.alphas_, b.alphas_) and a.intercept_ == b.intercept_
    for bad in (dict(reg_intercept=True), dict(loss=squared_hinge)):
        forced = OneVsRestSVC(**dict(kw, **bad))
        forced.batch_smo = True
        with pytest.raises(NotImplementedError):
            forced.fit(X, y)


def test_one_vs_rest_linear_kernel(amd):
    from optiml_amd.datasets import make_multiclass_blobs
    from optiml_amd.ml.svm import SVC, OneVsRestSVC
    from optiml_amd.ml.svm.losses import hinge
    X, y = make_multiclass_blobs(300, 5, 3, seed=2)
    kw = dict(loss=hinge, kernel=_kernel('linear'), C=1., dual=True, optimizer='smo', tol=1e-3)
    est = OneVsRestSVC(**kw)
    est.batch_smo = True
    est.fit(X, y)
    assert est.smo_ is True
    for c, e in enumerate(est.estimators_):
        one = SVC(**kw).fit(X, (y == est.classes_[c]).astype(int))
        assert np.array_equal(e.alphas_, one.alphas_) and e.intercept_ == one.intercept_ and np.array_equal(e.coef_, one.coef_)


def test_multi_output_equals_one_svr_per_target(amd):
    from optiml_amd.datasets import make_regression
    from optiml_amd.ml.svm import SVR, MultiOutputSVR
    from optiml_amd.ml.svm.kernels import GaussianKernel
    from optiml_amd.ml.svm.losses import epsilon_insensitive, squared_epsilon_insensitive
    X, y0 = make_regression(400, 6, seed=7)
    Y = np.stack([y0, np.sin(y0), y0 ** 2 - 1.], axis=1)
    kw = dict(loss=epsilon_insensitive, epsilon=0.1, kernel=GaussianKernel(gamma=0.2), C=1., dual=True, optimizer='smo', tol=1e-3)
    est = MultiOutputSVR(**kw)
    est.batch_smo = True
    est.fit(X, Y)
    assert est.batched_ is True and est.smo_ is True and len(est.estimators_) == 3
    for c, e in enumerate(est.estimators_):
        one = SVR(**kw).fit(X, Y[:, c])
        assert np.array_equal(e.alphas_, one.alphas_) and e.intercept_ == one.intercept_
        assert np.array_equal(e.support_, one.support_) and e.optimizer.iter == one.optimizer.iter
    Xt = X[::5] + 0.01
    per = np.stack([e.predict(Xt) for e in est.estimators_], axis=1)
    assert est.batched_decision_ is True
    np.testing.assert_allclose(est.predict(Xt), per, rtol=0, atol=1e-10)
    for bad in (dict(reg_intercept=True), dict(loss=squared_epsilon_insensitive)):
        forced = MultiOutputSVR(**dict(kw, **bad))
        forced.batch_smo = True
        with pytest.raises(NotImplementedError):
            forced.fit(X, Y)


def test_create_refuses_bad_columns(amd):
    from optiml_amd import _lib
    from optiml_amd.ml.svm._batched import _DeviceSMOSolver
    X, yb = _svc_data(200)
    dev = _svc_quad(X, yb, 'rbf').device_problem()
    Y = np.stack([yb, yb])
    ok = [np.arange(200), np.arange(0, 200, 2)]
    one_class = np.flatnonzero(yb > 0)
    bad = [dict(rows=[ok[0], np.array([3, 3, 5])]), dict(rows=[ok[0], np.array([5, 3])]), dict(rows=[ok[0], np.array([0, 200])]),
           dict(rows=[ok[0], np.array([-1, 4])]), dict(rows=[ok[0], np.array([7])]), dict(rows=[ok[0], one_class]),
           dict(C_=[1., 0.]), dict(epsilon=[0., -0.1]), dict(tol=0.)]
    for kw in bad:
        args = dict(C_=[1., 1.], epsilon=None, tol=1e-3, rows=ok)
        args.update(kw)
        with pytest.raises(_lib.BcqpError) as err:
            _DeviceSMOSolver(dev, _lib.SVC, Y, args['C_'], args['epsilon'], args['tol'], args['rows'])
        assert err.value.code == _lib.ERR_BADARG, kw
    s = _DeviceSMOSolver(dev, _lib.SVC, Y, [1., 1.], None, 1e-3, ok)
    with pytest.raises(_lib.BcqpError):
        s.get(2, _lib.SMO_ALPHAS)
    with pytest.raises(_lib.BcqpError):
        s.get(0, _lib.SMO_STATS)
    s.close()


# ---- 7. search ----------------------------------------------------------------------------------------------------------------------
def test_search_columns_are_the_folds_fits(amd, svc600_oracle):
    from optiml_amd.ml.svm import SVC, SVCGridSearchCV
    from optiml_amd.ml.svm.kernels import GaussianKernel
    from optiml_amd.ml.svm.losses import hinge
    X, yb, _, _ = svc600_oracle
    y = (yb > 0).astype(int)
    folds = _folds(600)
    # the oracle's fits are on the device's Gram matrix of THIS kernel: gamma as the golden fixture's 'scale' resolves on all rows
    gamma = _kernel('rbf').device_spec(X)[1]
    from optiml_amd.opti import KernelQuadratic
    quad = KernelQuadratic(X, -np.ones(600), 'svc', GaussianKernel(gamma=gamma), y=yb, rank_one=False)
    Kdev = quad.gram()
    quad.release()
    assert np.array_equal(Kdev, svc600_oracle[2])
    fits = svc600_oracle[3]
    Cs = [0.1, 1., 10.]
    tol = 1e-3
    est = SVC(loss=hinge, kernel=GaussianKernel(gamma=gamma), dual=True, optimizer='smo', tol=tol)
    search = SVCGridSearchCV(est, {'C': Cs}, cv=folds, refit=False)
    search.batch_smo = True
    search.fit(X, y)
    assert search.batched_ is True and search.smo_ is True
    want = np.empty((3, 3))
    for ci, Cv in enumerate(Cs):
        for f, (tr, te) in enumerate(folds):
            ref = fits[f, Cv]
            d = Kdev[te][:, tr] @ (ref['alphas'] * yb[tr]) + ref['b']
            np.testing.assert_allclose(search._cv_decisions[ci][f][0], d, rtol=0, atol=1e-10)
            want[ci, f] = np.mean((d > 0).astype(int) == y[te])
            assert search.n_iter_[ci, f, 0] == ref['iter'] and search.status_[ci, f, 0] == ''
            assert search.cv_results_['split%d_test_score' % f][ci] == want[ci, f]
    # the per-fold calls on the same commit: a fit on X[tr] is another Gram build and another walk through the same tol-optimal
    # set, so predictions are compared where the fallback's decision is clear of 12 tol (test_gpu_smo.py's bar (d)) — every row
    loop = SVCGridSearchCV(est, {'C': Cs}, cv=folds, refit=False)
    loop.batch_smo = False
    loop.fit(X, y)
    assert loop.batched_ is False and loop.smo_ is False
    for ci, Cv in enumerate(Cs):
        for f, (tr, te) in enumerate(folds):
            one = SVC(loss=hinge, kernel=GaussianKernel(gamma=gamma), C=Cv, dual=True, optimizer='smo', tol=tol).fit(X[tr], y[tr])
            d = one.decision_function(X[te])
            print('C = %g, fold %d: smallest |decision| of the per-fold fit %.4f' % (Cv, f, np.abs(d).min()))
            assert np.abs(d).min() > 12 * tol
            assert np.array_equal(d > 0, search._cv_decisions[ci][f][0] > 0)
            assert loop.cv_results_['split%d_test_score' % f][ci] == search.cv_results_['split%d_test_score' % f][ci]
            assert loop.n_iter_[ci, f, 0] == one.optimizer.iter


def test_search_falls_back_when_a_fold_misses_a_class(amd):
    from optiml_amd.ml.svm import SVC, SVCGridSearchCV
    from optiml_amd.ml.svm.kernels import GaussianKernel
    from optiml_amd.ml.svm.losses import hinge
    from optiml_amd.datasets import make_multiclass_blobs
    from optiml_amd.ml.svm import OneVsRestSVC
    X, y = make_multiclass_blobs(300, 5, 3, seed=4)
    idx = np.arange(300)
    miss = np.flatnonzero(y != 2)   # a training fold without class 2
    folds = [(miss, np.setdiff1d(idx, miss)), (np.setdiff1d(idx, idx[::2]), idx[::2])]
    est = OneVsRestSVC(loss=hinge, kernel=GaussianKernel(gamma=0.2), dual=True, optimizer='smo', tol=1e-3)
    search = SVCGridSearchCV(est, {'C': [0.5, 2.]}, cv=folds, refit=False)
    search.batch_smo = True
    search.fit(X, y)
    assert search.batched_ is False and search.smo_ is False
    loop = SVCGridSearchCV(est, {'C': [0.5, 2.]}, cv=folds, refit=False)
    loop.batch_smo = False
    loop.fit(X, y)
    for f in range(2):
        assert np.array_equal(search.cv_results_['split%d_test_score' % f], loop.cv_results_['split%d_test_score' % f])
    # the same estimator on folds that hold every class: batched, multi-class columns
    ok = [(np.setdiff1d(idx, idx[f::2]), idx[f::2]) for f in range(2)]
    both = SVCGridSearchCV(est, {'C': [0.5, 2.]}, cv=ok, refit=False)
    both.batch_smo = True
    both.fit(X, y)
    assert both.batched_ is True and both.smo_ is True and both.n_iter_.shape == (2, 2, 3) and (both.n_iter_ > 0).all()


# ---- 9. the batched walkers no other test launches: the compact 7-byte panel, and regression on the fp32 panel ---------------------
COVER_C, COVER_EPS = [0.3, 1., 3.], [0.05, 0.1, 0.2]
COVER_CASES = [('svc', 'compact', False), ('svr', 'compact', False), ('svr', 'f32', False), ('svr', 'f32', True)]


def _cover_draw(task):
    """300 x 6 standard normal rows (two 256-row tiles, the second ragged) and three label / target rows along random directions"""
    rs = np.random.RandomState(0)
    X = rs.standard_normal((300, 6))
    W = rs.standard_normal((6, 3))
    if task == 'svc':
        return X, np.where(X @ W + 0.5 * rs.standard_normal((300, 3)) > 0, 1., -1.).T.copy()
    return X, (np.sin(X @ W) + 0.3 * rs.standard_normal((300, 3))).T.copy()


@pytest.mark.parametrize('task,panel,boxes', COVER_CASES, ids=['%s-%s%s' % (t, p, '-rowboxes' if b else '') for t, p, b in COVER_CASES])
def test_batched_walkers_on_compact_and_fp32_panels_follow_the_oracle(amd, task, panel, boxes):
    """`smo_batch_kernel` for (classification, 7-byte panel), (regression, 7-byte panel), (regression, fp32 panel) and (regression,
    fp32 panel, per-row boxes — a constant vector per column, which walks the scalar box's path): three columns with C = 0.3, 1, 3
    (epsilon = 0.05, 0.1, 0.2), each held bit for bit to oracle/smo_oracle.py (tie='index', dot='tree') on the device's own Gram
    entries: multipliers, error cache, thresholds, outer iterations, pair steps.

    The oracle alone, on the CPU's Gram matrix of the draw (rounded to fp32 for the fp32 cases), takes per column
    (outer iterations, pair steps, support vectors):
      svc compact   (19, 489, 171)  (26, 855, 132)   (34, 1337, 101)
      svr compact   (23, 644, 288)  (37, 1354, 272)  (69, 4388, 210)
      svr fp32      (23, 765, 286)  (31, 1796, 271)  (82, 7973, 197)
    so both sweep kinds occur and every column moves.  On the device's Gram entries, which differ from NumPy's in the last bits, the
    oracle's compact runs took (17, 492, 171) (29, 888, 132) (25, 1085, 101) and (20, 619, 288) (33, 1293, 271) (76, 4970, 209),
    its fp32 runs the figures above; the test re-checks the floor (3 outer iterations, 20 steps, 5 support vectors) on the run it
    compares with and prints the figures."""
    from types import SimpleNamespace
    import smo_list_reference as lr
    from oracle import smo_oracle as smo
    from optiml_amd import _lib
    from optiml_amd.ml.svm._batched import solve_batched_smo
    from optiml_amd.ml.svm.kernels import GaussianKernel
    from optiml_amd.opti import KernelQuadratic
    X, Y = _cover_draw(task)
    n = 300
    kw, esz, gamma = (dict(compact=True), 7, lr.compact_gamma(X)) if panel == 'compact' else (dict(storage='f32'), 4, lr.rbf_gamma(X))
    kern = GaussianKernel(gamma=gamma)
    if task == 'svc':
        quad = KernelQuadratic(X, -np.ones(n), 'svc', kern, y=Y[0], rank_one=False, **kw)
    else:
        quad = KernelQuadratic(X, np.hstack((-Y[0], Y[0])) + 0.1, 'svr', kern, rank_one=False, **kw)
    # two tile rows of 256: three 256 x 256 tiles of 7 (the panel is in fact compact) or 4 bytes per element
    assert quad.device_problem().layout()['panel_bytes'] == 3 * 65536 * esz
    Kdev = quad.gram()
    eps = None if task == 'svc' else COVER_EPS
    res = solve_batched_smo(quad.device_problem(), _lib.SVC if task == 'svc' else _lib.SVR, Y, COVER_C, eps, 1e-3,
                            boxes=np.asarray(COVER_C)[:, None] * np.ones((3, n)) if boxes else None)
    quad.release()
    for c, r in enumerate(res):
        if task == 'svc':
            ref = smo.smo_svc(Kdev, Y[c], C=COVER_C[c], tol=1e-3, tie='index', dot='tree')
            n_sv, fields = np.count_nonzero(ref['alphas']), ('alphas',)
        else:
            ref = smo.smo_svr(Kdev, Y[c], C=COVER_C[c], epsilon=COVER_EPS[c], tol=1e-3, tie='index', dot='tree')
            n_sv, fields = np.count_nonzero(ref['alphas_p'] + ref['alphas_n']), ('alphas_p', 'alphas_n')
        print('%s %s column %d: oracle (outer, steps, support vectors) = (%d, %d, %d)' % (task, panel, c, ref['iter'], ref['steps'], n_sv))
        assert ref['finished'] and ref['iter'] >= 3 and ref['steps'] >= 20 and n_sv >= 5, (c, ref['iter'], ref['steps'], n_sv)
        _same(r, SimpleNamespace(**ref), fields + ('errors', 'b', 'b_up', 'b_low', 'iter', 'steps'), (task, panel, c))
