"""CPU checks of OneClassSVM: the NumPy reference of the solver (tests/oneclass_reference.py) against sklearn, the reference
projection's own properties, and the surface that needs no device."""
import ctypes as C

import numpy as np
import pytest

import oneclass_reference as ocr
from oracle import svm_oracle as so

NUS = (0.0517, 0.2517, 0.5017, 0.8017)   # nu n is never an integer: a free support vector exists and rho is unique


@pytest.fixture(scope='module')
def sk():
    return pytest.importorskip('sklearn.svm')


@pytest.mark.parametrize('n,d', [(257, 3), (600, 8)])
@pytest.mark.parametrize('gamma', ['1/d', 0.02])
def test_reference_against_sklearn(sk, n, d, gamma):
    """libsvm solves the same dual by SMO to tol 1e-12; the reference stops on the same measure at tol, so its decision values lie
    within a small multiple of tol of libsvm's (measured on this grid: at most 1.4 tol at 1e-3 and 1.6 tol at 1e-6; 10 tol, the
    issue's bound, allows for another BLAS), and at 1e-6 the support sets agree."""
    gamma = 1.0 / d if gamma == '1/d' else gamma
    X = ocr.one_class_data(n, d)
    K = so.gram('rbf', X, gamma=gamma)
    for nu in NUS:
        assert abs(nu * n - round(nu * n)) > 1e-3
        ref = sk.OneClassSVM(kernel='rbf', gamma=gamma, nu=nu, tol=1e-12).fit(X)
        dec = ref.decision_function(X)
        for tol in (1e-3, 1e-6):
            r = ocr.fit(K, nu, tol=tol, max_iter=1000)
            assert r['status'] == 'optimal' and r['iter'] <= 1000, (nu, tol, r['status'], r['iter'])
            mine = K @ r['x'] - r['rho']
            err = float(np.abs(mine - dec).max())
            print('n=%d gamma=%g nu=%g tol=%g: %d iterations, |dec - sklearn| = %.2f tol' % (n, gamma, nu, tol, r['iter'], err / tol))
            assert err <= 10 * tol
            assert abs(r['x'].sum() - nu * n) <= 1e-10 * nu * n
            assert r['x'].min() >= 0 and r['x'].max() <= 1
            if tol == 1e-6:
                assert np.array_equal(np.flatnonzero(r['x'] > 0), ref.support_)
                np.testing.assert_allclose(r['x'][ref.support_], ref.dual_coef_[0], atol=100 * tol)


def test_reference_records_and_stops():
    X = ocr.one_class_data(257, 3)
    K = so.gram('rbf', X, gamma=1.0)
    r = ocr.solve(K, np.ones(257), 0.25 * 257, tol=0.0, max_iter=12)
    assert r['status'] == 'stopped' and r['iter'] == 12 and len(r['rows']) == 13
    assert np.array_equal(r['rows'][:, 0], np.arange(13))
    assert r['rows'][0, 3] == 0.0 and r['rows'][0, 4] == 1.0   # no step yet, s = 1
    f = r['rows'][:, 1]   # nonmonotone: a value may rise, never above the largest of the ten before it
    assert all(f[i] <= f[max(0, i - 10):i].max() for i in range(1, 13)) and f[-1] < f[0]
    # the whole box is a single point: optimal at once, without a step
    r = ocr.solve(K, np.ones(257), 257.0, tol=1e-3)
    assert r['status'] == 'optimal' and r['iter'] == 0 and np.array_equal(r['x'], np.ones(257)) and r['rows'][0, 2] == -np.inf
    # a warm start at the solution stops at once
    a = ocr.solve(K, np.ones(257), 0.25 * 257, tol=1e-6)
    b = ocr.solve(K, np.ones(257), 0.25 * 257, tol=1e-6, x0=a['x'])
    assert b['iter'] == 0 and b['status'] == 'optimal'


def test_rho_without_a_free_row():
    u = np.array([1., 1., 0., 1.])
    x = np.array([1., 0., 0., 1.])
    g = np.array([0.2, 0.9, -5., 0.4])
    rho, n_sv, n_free = ocr.rho(x, g, u)
    assert (rho, n_sv, n_free) == ((0.9 + 0.4) / 2, 2, 0)
    x = np.array([1., 0.5, 0., 0.25])
    assert ocr.rho(x, g, u) == ((0.9 + 0.4) / 2, 3, 2)


@pytest.mark.parametrize('n', [257, 600, 1100])
@pytest.mark.parametrize('scale', [1.0, 1e4, 1e-4])
def test_projection_reference(n, scale):
    """The box holds bitwise, a zero-width row stays 0, and both error figures, taken in np.longdouble against the projection run
    in np.longdouble, stay within n 2^-52 max(1, |v|_inf): tau is the quotient of sums of at most n terms of that size by the number
    of free rows, every free P_i inherits tau's error plus one rounding of its own, and sum P collects at most n of those."""
    v, u, masses = ocr.projection_inputs(n, scale)
    for r in masses:
        P = ocr.project(v, u, r)
        assert P.dtype == np.float64
        assert np.all(P >= 0) and np.all(P <= u)
        assert np.all(P[u == 0] == 0)
        if r == u.sum():
            assert np.array_equal(P, u)
        fs, fi = ocr.projection_figures(P, v, u, r)
        bound = n * 2.0 ** -52 * max(1.0, float(np.abs(v).max()))
        print('n=%d scale=%g r=%g: |sum P - r| = %.2e, |P - P_ext| = %.2e, bound %.2e' % (n, scale, r, fs, fi, bound))
        assert fs <= bound and fi <= bound
        bs, bi = ocr.projection_bounds(v, u, r)
        assert bs >= 2.0 ** -50 and bi >= 2.0 ** -50
        # the defining property: no feasible point is closer to v (checked against random feasible points)
        rs = np.random.RandomState(n)
        for _ in range(3):
            z = ocr.project(v + rs.standard_normal(n) * scale, u, r)
            assert np.sum((P - v) ** 2) <= np.sum((z - v) ** 2) * (1 + 1e-12)


def test_projection_of_one_entry():
    assert ocr.project(np.array([3.0]), np.array([1.0]), 0.25)[0] == 0.25
    assert ocr.project(np.array([-3.0]), np.array([0.5]), 0.5)[0] == 0.5


# ---- the surface ------------------------------------------------------------------------------------------------------------------
def test_exports_and_parameters():
    import optiml_amd.ml.svm as svm
    from optiml_amd.ml.svm import OneClassSVM, one_class_nu_path
    from optiml_amd.ml.svm.kernels import gaussian, GaussianKernel
    assert 'OneClassSVM' in svm.__all__ and 'one_class_nu_path' in svm.__all__
    assert callable(one_class_nu_path)
    est = OneClassSVM()
    assert est.get_params(deep=False) == dict(kernel=gaussian, nu=0.5, tol=1e-3, max_iter=1000, storage='f64')
    for bad in (dict(nu=0), dict(nu=1.0001), dict(nu=-0.1), dict(tol=-1e-9), dict(max_iter=0), dict(storage='f16')):
        with pytest.raises(ValueError):
            OneClassSVM(**bad)
    with pytest.raises(TypeError):
        OneClassSVM(kernel='rbf')
    OneClassSVM(nu=1.0, tol=0.0, max_iter=1)
    base = pytest.importorskip('sklearn.base')
    est = OneClassSVM(kernel=GaussianKernel(gamma=0.1), nu=0.2, tol=1e-5, max_iter=77, storage='f32')
    twin = base.clone(est)
    assert twin is not est and twin.get_params(deep=False).keys() == est.get_params(deep=False).keys()
    assert (twin.nu, twin.tol, twin.max_iter, twin.storage, twin.kernel.gamma) == (0.2, 1e-5, 77, 'f32', 0.1)
    assert est.set_params(nu=0.9).nu == 0.9
    with pytest.raises(ValueError):   # set_params is checked at fit
        est.set_params(nu=2).fit(np.zeros((4, 2)))


def test_not_implemented_cases(monkeypatch):
    from optiml_amd.ml.svm import OneClassSVM, one_class_nu_path
    from optiml_amd.ml.svm import oneclass
    X = ocr.one_class_data(40, 2)
    with pytest.raises(NotImplementedError):
        OneClassSVM(storage='stream').fit(X)
    with pytest.raises(NotImplementedError):
        one_class_nu_path(OneClassSVM(storage='stream'), X, [0.1, 0.2])

    class TwoRanks:
        world = 2
    monkeypatch.setattr(oneclass, 'get_context', lambda: TwoRanks())
    with pytest.raises(NotImplementedError):
        OneClassSVM().fit(X)


def test_bad_arguments_without_a_device():
    from optiml_amd import build, _lib
    build.build()
    lib = _lib.load()
    h = C.c_void_p()
    one = np.ones(4)
    p = _lib.ptr(one)
    fake = C.c_void_p(1)   # never dereferenced: the NULL and k checks come first
    assert lib.bq_msolver_create_simplex(None, 1, p, p, None, 1e-3, 10, C.byref(h)) == _lib.ERR_BADARG
    assert lib.bq_msolver_create_simplex(fake, 1, None, p, None, 1e-3, 10, C.byref(h)) == _lib.ERR_BADARG
    assert lib.bq_msolver_create_simplex(fake, 1, p, None, None, 1e-3, 10, C.byref(h)) == _lib.ERR_BADARG
    assert lib.bq_msolver_create_simplex(fake, 1, p, p, None, 1e-3, 10, None) == _lib.ERR_BADARG
    assert b'NULL' in lib.bq_last_error()
    assert lib.bq_msolver_create_simplex(fake, 0, p, p, None, 1e-3, 10, C.byref(h)) == _lib.ERR_BADARG
    assert b'k must be' in lib.bq_last_error()
    assert not h
    i64 = C.POINTER(C.c_int64)
    n_sv = np.zeros(1, dtype=np.int64)
    assert lib.bq_msolver_simplex_offsets(None, p, n_sv.ctypes.data_as(i64), n_sv.ctypes.data_as(i64)) == _lib.ERR_BADARG
    assert lib.bq_msolver_simplex_offsets(fake, None, n_sv.ctypes.data_as(i64), n_sv.ctypes.data_as(i64)) == _lib.ERR_BADARG
    assert lib.bq_msolver_simplex_offsets(fake, p, None, n_sv.ctypes.data_as(i64)) == _lib.ERR_BADARG
    assert lib.bq_msolver_simplex_offsets(fake, p, n_sv.ctypes.data_as(i64), None) == _lib.ERR_BADARG
    # bq_simplex_project checks its host arrays before it touches the context
    mass = np.array([2.0])
    out = np.empty(4)
    args = lambda **kw: [kw.get('ctx', fake), kw.get('k', 1), kw.get('n', 4), _lib.ptr(kw.get('V', one)), _lib.ptr(kw.get('UB', one)),
                         _lib.ptr(kw.get('mass', mass)), _lib.ptr(kw.get('P', out))]   # noqa: E731
    assert lib.bq_simplex_project(*args(ctx=None)) == _lib.ERR_BADARG
    for name in ('V', 'UB', 'mass', 'P'):
        assert lib.bq_simplex_project(*args(**{name: None})) == _lib.ERR_BADARG
    assert lib.bq_simplex_project(*args(k=0)) == _lib.ERR_BADARG
    assert lib.bq_simplex_project(*args(n=0)) == _lib.ERR_BADARG
    assert lib.bq_simplex_project(*args(UB=np.array([1., -1., 1., 1.]))) == _lib.ERR_BADARG and b'boxes' in lib.bq_last_error()
    assert lib.bq_simplex_project(*args(UB=np.array([1., np.inf, 1., 1.]))) == _lib.ERR_BADARG
    assert lib.bq_simplex_project(*args(UB=np.array([1., np.nan, 1., 1.]))) == _lib.ERR_BADARG
    assert lib.bq_simplex_project(*args(mass=np.array([0.0]))) == _lib.ERR_BADARG and b'mass' in lib.bq_last_error()
    assert lib.bq_simplex_project(*args(mass=np.array([-1.0]))) == _lib.ERR_BADARG
    assert lib.bq_simplex_project(*args(mass=np.array([4.5]))) == _lib.ERR_BADARG and b'sum' in lib.bq_last_error()
    assert lib.bq_simplex_project(*args(V=np.array([1., np.nan, 1., 1.]))) == _lib.ERR_BADARG
