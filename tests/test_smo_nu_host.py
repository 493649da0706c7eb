"""The NumPy restatement of the row-based SMO's general entry (tests/smo_nu_reference.py: libsvm's Solver from a nonzero start for
the one-class dual, Solver_NU for nu-SVC and nu-SVR) held to libsvm itself through sklearn.svm.OneClassSVM / NuSVC / NuSVR
(kernel='precomputed', shrinking=False, tol=1e-6) on seeded data: smo_rows_reference's svc / svr problems, and for one-class
default_rng(0) standard normal X with every 9th row scaled by 3.  The restatement starts from libsvm's own start gradient (the
sum of alpha_i Q_i in ascending i).

Measured on the CPU (steps of the restatement, sklearn's n_iter_ in brackets, largest difference of the decision values):
    one-class n = 300  d = 5 gamma 0.5 nu 0.2     725 (725)        2.0e-8
    one-class n = 1500 d = 8 gamma 0.2 nu 0.1     1364 (1364)      6.5e-8
    nu-SVC svc300  nu 0.3                         2048 (1817)      8.7e-6 raw, r = 0.148:  1.3e-6 of r x decision
    nu-SVC svc1500 nu 0.2                         22756 (23038)    3.4e-5 raw, r = 0.0305: 1.0e-6 of r x decision
    nu-SVR svr300  C 1 nu 0.5                     5350 (5358)      6.5e-7
    nu-SVR svr1500 C 1 nu 0.2                     15223 (15290)    6.4e-7
The bound is 1e-5, that of test_smo_rows_host.py and for its reason: both solvers stop at a violation of tol, so their decision
values agree to a few tol.  For nu-SVC the compared quantity is r x decision, the unscaled dual's: tol bounds that one, and the raw
values move by tol / r.  Step counts are not asserted (libsvm keeps its kernel rows in float; near-ties fall differently).
(svr1500 with C = 10, nu = 0.3 is not a case: epsilon collapses to 0 there and the restatement takes 600 000 steps.)"""
import functools

import numpy as np
import pytest

import smo_nu_reference as nu
import smo_rows_reference as ref

sklearn_svm = pytest.importorskip('sklearn.svm')

TOL = 1e-6
NAMES = ['oc300', 'oc1500', 'nusvc300', 'nusvc1500', 'nusvr300', 'nusvr1500']


@functools.lru_cache(maxsize=None)
def _solved(name):
    X, y, gamma, (signs, p, C, alpha0, rule) = nu.case_problem(name)
    K = ref.rbf(X, gamma)
    K.setflags(write=False)
    G0 = nu.libsvm_start_gradient(K, signs, p, alpha0)
    return K, y, (signs, p, C, alpha0), nu.solve(rule, K, signs, p, C, TOL, alpha0, G0)


@pytest.mark.parametrize('name', NAMES)
def test_reference_follows_libsvm(name):
    kind, n, d, gamma, nu_, Cval = nu.CASES[name]
    K, y, _, got = _solved(name)
    assert got.status == 'optimal'
    if kind == 'oc':
        model = sklearn_svm.OneClassSVM(kernel='precomputed', nu=nu_, tol=TOL, shrinking=False).fit(K)
        want = model.decision_function(K)
        dec, scale = K @ got.alpha - got.rho, 1.0
    elif kind == 'nusvc':
        model = sklearn_svm.NuSVC(kernel='precomputed', nu=nu_, tol=TOL, shrinking=False).fit(K, y)
        scale = got.r
        want = scale * model.decision_function(K)          # r x decision: the unscaled dual's
        dec = K @ (got.alpha * y) - got.rho
    else:
        model = sklearn_svm.NuSVR(kernel='precomputed', nu=nu_, C=Cval, tol=TOL, shrinking=False).fit(K, y)
        want = model.predict(K)
        dec, scale = K @ (got.alpha[:n] - got.alpha[n:]) - got.rho, 1.0
    err = float(np.abs(dec - want).max())
    print(f'{name}: sklearn n_iter_ {np.ravel(model.n_iter_)[0]}, reference {got.steps} steps, max decision difference {err:.3e}'
          + (f' (r = {scale:.4g}, raw {err / scale:.3e})' if kind == 'nusvc' else ''))
    assert err <= 1e-5


@pytest.mark.parametrize('name', ['oc300', 'nusvc300', 'nusvr300'])
def test_reference_invariants(name):
    K, y, (signs, p, C, alpha0), got = _solved(name)
    assert (got.alpha >= 0).all() and (got.alpha <= C).all()
    groups = (signs > 0, signs < 0) if name != 'oc300' else (signs > 0,)
    for g in groups:   # the mass of each group stays what the start gave it
        assert abs(float(got.alpha[g].sum() - alpha0[g].sum())) <= 1e-12 * float(alpha0[g].sum())
    rep = len(signs) // len(K)
    Q = (signs[:, None] * signs[None, :]) * np.tile(K, (rep, rep))
    np.testing.assert_allclose(got.G, Q @ got.alpha + p, rtol=0, atol=1e-10)
    assert len(set(got.pairs)) > 1 and all(i != j for i, j in got.pairs)
    if name == 'oc300':
        assert got.gmax + got.gmax2 < TOL
    else:
        assert max(got.gap_p, got.gap_n) < TOL
        assert all(signs[i] == signs[j] for i, j in got.pairs)   # a Solver_NU pair never crosses the signs


def test_starts_are_libsvm_s():
    a = nu.one_class_start(300, 0.2)
    assert a.sum() == 60.0 and (a[:60] == 1).all() and (a[60:] == 0).all()
    a = nu.one_class_start(10, 0.25)
    assert list(a[:4]) == [1.0, 1.0, 0.5, 0.0]
    y = np.array([1, -1, 1, 1, -1, -1, 1.0, -1])
    a = nu.nu_svc_start(y, 0.4)   # 1.6 per class, in index order
    np.testing.assert_allclose(a, [1, 1, 0.6, 0, 0.6, 0, 0, 0], rtol=0, atol=1e-15)
    a = nu.nu_svr_start(4, 2.0, 0.75)   # 3 per half
    np.testing.assert_allclose(a, [2, 1, 0, 0, 2, 1, 0, 0], rtol=0, atol=0)


def test_the_two_start_gradients_differ_in_rounding_only():
    for name in ('oc300', 'nusvc300', 'nusvr300'):
        X, y, gamma, (signs, p, C, alpha0, rule) = nu.case_problem(name)
        K = ref.rbf(X, gamma)
        a, b = nu.libsvm_start_gradient(K, signs, p, alpha0), nu.product_start_gradient(K, signs, p, alpha0)
        rep = len(signs) // len(K)
        terms = np.tile(np.abs(K), (1, rep)) @ np.abs(alpha0) + np.abs(p[:len(K)])   # the sum of the magnitudes libsvm adds up
        bound = np.tile(2 * (len(signs) + 16) * 2.0 ** -53 * terms, rep)             # any two orders of N + 1 terms
        assert (np.abs(a - b) <= bound).all()
        if name == 'nusvr300':   # alpha and alpha* start equal: b = 0, G0 = p with p's bits
            assert b.tobytes() == p.tobytes()


def test_cap_and_cut():
    X, y, gamma, (signs, p, C, alpha0, rule) = nu.case_problem('nusvr300')
    K = ref.rbf(X, gamma)
    whole = nu.solve_nu(K, signs, p, C, 1e-3, alpha0, p)
    capped = nu.solve_nu(K, signs, p, C, 1e-3, alpha0, p, max_steps=25)
    cut = nu.solve_nu(K, signs, p, C, 1e-3, alpha0, p, steps_only=25)
    assert capped.status == 'stopped' and cut.status == 'running' and capped.steps == cut.steps == 25
    assert capped.pairs == whole.pairs[:25] and capped.alpha.tobytes() == cut.alpha.tobytes()


def test_estimator_starts_and_argument_checks():
    """the estimators' vectorised starts have the bits of libsvm's loops (the restatement's), and a cache too small for the rule is
    a ValueError at construction and at fit, before anything is built"""
    from optiml_amd.ml.svm import RowNuSVC, RowNuSVR, RowOneClassSVM, nu_rows
    rng = np.random.default_rng(1)
    for n in (1, 2, 3, 50, 301, 1000):
        y = np.where(rng.standard_normal(n) > 0, 1.0, -1.0)
        for v in (0.01, 0.2, 0.37, 0.5, 0.999, 1.0):
            assert nu.one_class_start(n, v).tobytes() == nu_rows.one_class_start(n, v).tobytes()
            assert nu.nu_svc_start(y, v).tobytes() == nu_rows.nu_svc_start(y, v).tobytes(), (n, v)
            for Cval in (1.0, 2.5, 0.3, 10.0, 1 / 3):
                assert nu.nu_svr_start(n, Cval, v).tobytes() == nu_rows.nu_svr_start(n, Cval, v).tobytes(), (n, Cval, v)
    for cls in (RowNuSVC, RowNuSVR):
        with pytest.raises(ValueError, match='cache_rows'):
            cls(cache_rows=2)
        with pytest.raises(ValueError, match='cache_rows'):
            cls().set_params(cache_rows=2).fit(np.zeros((4, 2)), np.array([1.0, -1.0, 1.0, -1.0]))
    assert RowOneClassSVM(cache_rows=2).cache_rows == 2   # a Solver step holds two rows
    with pytest.raises(ValueError, match='cache_rows'):
        RowOneClassSVM(cache_rows=1)
