"""The NumPy statement of the two-group simplex solver (tests/nu_reference.py) against sklearn's NuSVC and NuSVR (libsvm), on the
host: what the device tests (test_gpu_nu.py) then hold the kernels to."""
import functools

import numpy as np
import pytest

import nu_reference as nur
import oneclass_reference as ocr


def _rbf(A, B, gamma):
    d2 = (A * A).sum(1)[:, None] + (B * B).sum(1)[None, :] - 2.0 * A @ B.T
    return np.exp(-gamma * np.maximum(d2, 0.0))


@functools.lru_cache(maxsize=None)
def _grams(gamma):
    X, Xnew, _, _ = nur.nu_data()
    return _rbf(X, X, gamma), _rbf(Xnew, X, gamma)


@functools.lru_cache(maxsize=None)
def _sk_svc(gamma, nu):
    svm = pytest.importorskip('sklearn.svm')
    X, _, yc, _ = nur.nu_data()
    return svm.NuSVC(kernel='rbf', gamma=gamma, nu=nu, tol=1e-12).fit(X, yc)


@functools.lru_cache(maxsize=None)
def _sk_svr(gamma, C, nu):
    svm = pytest.importorskip('sklearn.svm')
    X, _, _, yr = nur.nu_data()
    return svm.NuSVR(kernel='rbf', gamma=gamma, C=C, nu=nu, tol=1e-12).fit(X, yr)


def test_data_is_the_issue_s():
    X, Xnew, yc, yr = nur.nu_data()
    assert X.shape == (600, 8) and Xnew.shape == (50, 8) and yr.shape == (600,)
    assert ((yc == 1).sum(), (yc == -1).sum()) == (314, 286)


@pytest.mark.parametrize('tol', nur.TOLS)
@pytest.mark.parametrize('gamma,nu', nur.SVC_GRID)
def test_nu_svc_reference_against_sklearn(gamma, nu, tol):
    """'optimal' within the default 1000 iterations; each class's alpha sums to nu n / 2; the decision values on X and on 50 fresh
    points lie within 10 tol / r of sklearn's (tol 1e-12): tol bounds the violation of the unscaled dual, and the decision function
    is that dual's divided by r; predict agrees wherever sklearn's |decision| exceeds that, which leaves out at most 5 % of the
    training rows; at tol 1e-6 the support set is sklearn's (which orders support_ by class: compared sorted)."""
    X, Xnew, yc, _ = nur.nu_data()
    K, Knew = _grams(gamma)
    ref = _sk_svc(gamma, nu)
    y = yc.astype(float)
    out = nur.fit_nu_svc(K, y, nu, tol=tol, max_iter=1000)
    n = len(y)
    assert out['status'] == 'optimal'
    a, r = out['x'], out['r']
    assert a.min() >= 0 and a.max() <= 1 and r > 0
    for cls in (1, -1):
        assert abs(a[yc == cls].sum() - nu * n / 2) <= 1e-10 * nu * n / 2
    bound = 10 * tol / r
    for Kz, Z in ((K, X), (Knew, Xnew)):
        dec, theirs = Kz @ out['coef'] + out['intercept'], ref.decision_function(Z)
        print('gamma=%g nu=%g tol=%g: %d iterations, r = %.3e, r |decision difference| / tol = %.2f'
              % (gamma, nu, tol, out['iter'], r, r * np.abs(dec - theirs).max() / tol))
        assert np.abs(dec - theirs).max() <= bound
        clear = np.abs(theirs) > bound
        assert np.array_equal(np.where(dec > 0, 1, -1)[clear], ref.predict(Z)[clear])
        if Z is X:
            assert (~clear).sum() <= 0.05 * n
    if tol == 1e-6:
        assert np.array_equal(np.flatnonzero(a > 0), np.sort(ref.support_))


@pytest.mark.parametrize('tol', nur.TOLS)
@pytest.mark.parametrize('gamma,C,nu', nur.SVR_GRID)
def test_nu_svr_reference_against_sklearn(gamma, C, nu, tol):
    """'optimal' within 3000 iterations; each half sums to C nu n / 2; no row has alpha and alpha* both positive; the predictions on X
    and on 50 fresh points lie within 10 tol of sklearn's."""
    X, Xnew, _, yr = nur.nu_data()
    K, Knew = _grams(gamma)
    ref = _sk_svr(gamma, C, nu)
    out = nur.fit_nu_svr(K, yr, C, nu, tol=tol, max_iter=3000)
    n = len(yr)
    assert out['status'] == 'optimal'
    x = out['x']
    assert x.min() >= 0 and x.max() <= C
    for half in (x[:n], x[n:]):
        assert abs(half.sum() - C * nu * n / 2) <= 1e-10 * C * nu * n / 2
    assert not ((x[:n] > 0) & (x[n:] > 0)).any()
    for Kz, Z in ((K, X), (Knew, Xnew)):
        pred, theirs = Kz @ out['coef'] + out['intercept'], ref.predict(Z)
        print('gamma=%g C=%g nu=%g tol=%g: %d iterations, |prediction difference| / tol = %.2f'
              % (gamma, C, nu, tol, out['iter'], np.abs(pred - theirs).max() / tol))
        assert np.abs(pred - theirs).max() <= 10 * tol


def test_infeasible_nu():
    """libsvm's check: nu n / 2 may not exceed the smaller class."""
    from optiml_amd.ml.svm.nu import _check_feasible
    y = np.array([1.] * 10 + [-1.] * 30)
    _check_feasible(y, 0.5)
    with pytest.raises(ValueError, match='specified nu is infeasible'):
        _check_feasible(y, 0.5017)


@pytest.mark.parametrize('paired', [False, True])
def test_projection_per_group(paired):
    """The projection onto the product of the two simplices is the two `project` calls: each group of the result is the projection of
    that group's entries alone (bitwise), the groups' sums are the masses, and no feasible point is nearer to v."""
    n = 257
    rs = np.random.RandomState(3)
    m = 2 * n if paired else n
    v = rs.standard_normal(m) * 2
    u = rs.choice([0., 0.5, 1.], m)
    sgn = None if paired else np.where(rs.rand(n) < 0.3, 1., -1.)
    lay = nur.Layout(n, sgn)
    mass = [0.37 * u[idx].sum() for idx in lay.groups]
    P = nur.project2(v, u, mass, lay)
    assert np.all(P >= 0) and np.all(P <= u)
    assert len(np.intersect1d(*lay.groups)) == 0 and len(lay.groups[0]) + len(lay.groups[1]) == m
    for idx, r in zip(lay.groups, mass):
        assert np.array_equal(P[idx], ocr.project(v[idx], u[idx], r))
        assert abs(P[idx].sum() - r) <= 1e-12 * r
    best = float(((P - v) ** 2).sum())
    for _ in range(20):   # feasible points: projections of perturbed v
        Z = nur.project2(v + 0.3 * rs.standard_normal(m), u, mass, lay)
        assert float(((Z - v) ** 2).sum()) >= best - 1e-12


def test_reference_layouts_agree_on_a_signed_problem():
    """A PAIRED column and the LABELS column on the doubled Gram matrix [[K, K], [K, K]] with labels (+1, -1) are the same problem:
    the same f history to rounding."""
    X, _, _, yr = nur.nu_data()
    n = 120
    K = _rbf(X[:n], X[:n], 0.125)
    q = np.concatenate((-yr[:n], yr[:n]))
    u = np.full(2 * n, 1.0)
    mass = (0.4 * n / 2, 0.4 * n / 2)
    a = nur.solve(K, u, mass, q=q, tol=0.0, max_iter=20)
    b = nur.solve(np.block([[K, K], [K, K]]), u, mass, sgn=np.concatenate((np.ones(n), -np.ones(n))), q=q, tol=0.0, max_iter=20)
    assert a['iter'] == b['iter'] == 20
    np.testing.assert_allclose(a['rows'][:, 1], b['rows'][:, 1], rtol=1e-9)
