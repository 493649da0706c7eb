"""The NumPy restatement of libsvm's Solver without shrinking (tests/smo_rows_reference.py) — the reference of the row-based SMO
(bq_rsmo_*) — held to libsvm itself through sklearn.svm.SVC / SVR(kernel='precomputed', shrinking=False) on seeded data
(default_rng(0), X standard normal; SVC labels sign(x0 x1 + 0.3 noise) with gamma = 0.5, n = 300, d = 5, C = 1 and gamma = 0.2,
n = 1500, d = 8, C = 10; SVR targets sin x0 + 0.1 noise, epsilon = 0.1; the n = 300 SVC problem again with class weights
{+1: 5, -1: 1}).

The step counts differ (libsvm keeps its kernel rows in float, so ties and near-ties fall differently); measured on the CPU, as
sklearn n_iter_ / this reference at tol 1e-3 and 1e-6:
    SVC n = 300    312 / 286      563 / 516          weighted   501 / 542     1041 / 1184
    SVC n = 1500   5795 / 5950    12695 / 12839
    SVR n = 300    676 / 676      1731 / 1776
    SVR n = 1500   9927 / 10112   29623 / 29476
Both solvers stop at a violation of tol, so at tol = 1e-6 their decision values agree to a few tol: measured 1.1e-6 / 3.9e-6 (SVC),
1.8e-6 (weighted), 8.7e-7 / 1.3e-6 (SVR); the test asserts <= 1e-5 (2.5x the worst case).  The dual objectives agree to a relative
1e-10 (measured <= 6.3e-12)."""
import functools

import numpy as np
import pytest

import smo_rows_reference as ref

sklearn_svm = pytest.importorskip('sklearn.svm')

TOL = 1e-6
CASES = [('svc300', False), ('svc300', True), ('svc1500', False), ('svr300', False), ('svr1500', False)]


@functools.lru_cache(maxsize=None)
def _solved(name, weighted):
    X, y, gamma, signs, p, C = ref.case_problem(name, weighted)
    K = ref.rbf(X, gamma)
    K.setflags(write=False)
    return K, y, ref.solve(K, signs, p, C, TOL)


@pytest.mark.parametrize('name,weighted', CASES)
def test_reference_follows_libsvm(name, weighted):
    task, n, d, gamma, Cval = ref.CASES[name]
    K, y, got = _solved(name, weighted)
    assert got.status == 'optimal'
    if task == 'svc':
        model = sklearn_svm.SVC(kernel='precomputed', C=Cval, tol=TOL, shrinking=False,
                                class_weight=ref.CLASS_WEIGHT if weighted else None).fit(K, y)
        want_dec = model.decision_function(K)
        coef = np.zeros(n)
        coef[model.support_] = model.dual_coef_[0]          # y alpha
        want_obj = 0.5 * coef @ K @ coef - np.abs(coef).sum()
        dec = K @ (got.alpha * y) - got.rho
    else:
        model = sklearn_svm.SVR(kernel='precomputed', C=Cval, tol=TOL, epsilon=ref.EPSILON, shrinking=False).fit(K, y)
        want_dec = model.predict(K)
        coef = np.zeros(n)
        coef[model.support_] = model.dual_coef_[0]          # alpha - alpha*
        want_obj = 0.5 * coef @ K @ coef + ref.EPSILON * np.abs(coef).sum() - y @ coef
        dec = K @ (got.alpha[:n] - got.alpha[n:]) - got.rho
    err = float(np.abs(dec - want_dec).max())
    rel = abs(got.objective - want_obj) / abs(want_obj)
    print(f'{name} weighted={weighted}: sklearn n_iter_ {np.ravel(model.n_iter_)[0]}, reference {got.steps} steps, '
          f'max decision difference {err:.3e}, relative objective difference {rel:.3e}')
    assert err <= 1e-5
    assert rel <= 1e-10
    assert abs(-got.rho - float(np.ravel(model.intercept_)[0])) <= 1e-5


def test_reference_invariants():
    K, y, got = _solved('svc300', True)
    X, y, gamma, signs, p, C = ref.case_problem('svc300', True)
    assert (got.alpha >= 0).all() and (got.alpha <= C).all()
    assert abs(float(signs @ got.alpha)) <= 1e-12 * float(np.abs(got.alpha).sum())
    # G is the gradient of the dual at alpha, up to the rounding of `steps` updates
    Q = (signs[:, None] * signs[None, :]) * K
    np.testing.assert_allclose(got.G, Q @ got.alpha + p, rtol=0, atol=1e-10)
    assert got.gmax + got.gmax2 < TOL
    assert len(set(got.pairs)) > 1 and all(i != j for i, j in got.pairs)


def test_reference_cap_and_cut():
    X, y, gamma, signs, p, C = ref.case_problem('svr300')
    K = ref.rbf(X, gamma)
    whole = ref.solve(K, signs, p, C, 1e-3)
    capped = ref.solve(K, signs, p, C, 1e-3, max_steps=25)
    cut = ref.solve(K, signs, p, C, 1e-3, steps_only=25)
    assert capped.status == 'stopped' and cut.status == 'running' and capped.steps == cut.steps == 25
    assert capped.pairs == whole.pairs[:25] and capped.alpha.tobytes() == cut.alpha.tobytes()
