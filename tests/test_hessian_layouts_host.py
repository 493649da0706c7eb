"""Conditions on the INPUTS of test_gpu_hessian_layouts.py, checked on the CPU: the cases must be able to tell the triangles apart.

The GPU tests hold the device to the oracle reading the UPPER triangle of a dense Q in row blocks (scipy's default, what the
reference's `cho_factor` calls do).  That says something only if reading the other triangle would have failed them: here the
oracle runs with both and the two answers must lie at least 100 tolerances apart, for every quantity the GPU tests compare.
"""
import numpy as np
import pytest

import hessian_layout_reference as hl
from oracle import bcqp_oracle as bo

FACTOR = 100.0   # fixed: a case that does not reach it gets another seed, not a smaller factor


def _margins(other, ref):
    """{quantity: tolerances between the two runs}"""
    return {
        'as f history': hl.margin(other['as']['f_hist'], ref['as']['f_hist'], **hl.F_TOL),
        'as x': hl.margin(other['as']['x'], ref['as']['x'], **hl.X_TOL),
        'ip f history': hl.margin(other['ip']['f_hist'], ref['ip']['f_hist'], **hl.F_TOL),
        'ip x': hl.margin(other['ip']['x'], ref['ip']['x'], **hl.X_TOL),
        'x_star': hl.margin(other['x_star'], ref['x_star'], **hl.xstar_tol(ref['x_star'])),
    }


@pytest.mark.parametrize('storage', ['f64', 'f32'])
@pytest.mark.parametrize('n', hl.NONSYM_SIZES)
def test_nonsymmetric_case_is_a_stable_reference_that_tells_the_triangles_apart(n, storage):
    Q, q, ub, lb = hl.nonsymmetric_case(n)
    Q = hl.rounded(Q, storage)
    assert not np.array_equal(Q, Q.T)
    ref = hl.solve_all(Q, q, ub, lb, 'upper', n)
    # ActiveSet converges, and never through the minres branch (np.inner(QAA, QAA) of a non-symmetric block: out of scope)
    assert ref['as']['status'] == 'optimal' and ref['as']['iter'] <= hl.as_iters(n)
    assert all(not ev['used_minres'] for ev in ref['as']['trace'])
    assert any(ev['kind'] == 'step' for ev in ref['as']['trace'])   # ratio steps exist: their f is what the product-free chain forms
    assert ref['ip']['iter'] == hl.IP_ITERS and len(ref['ip']['f_hist']) == hl.IP_ITERS + 1
    assert ref['x_star_method'] == 'cholesky'
    # the patched oracle with scipy's default triangle IS the oracle
    plain = bo.active_set(Q, q, ub, lb=lb, max_iter=hl.as_iters(n))
    assert np.array_equal(plain['f_hist'], ref['as']['f_hist']) and np.array_equal(plain['x'], ref['as']['x'])
    low = hl.solve_all(Q, q, ub, lb, 'lower', n)
    m = _margins(low, ref)
    print(f'n={n} {storage} margins (tolerances): ' + ', '.join(f'{k} {v:.3g}' for k, v in m.items()))
    for k, v in m.items():
        assert v >= FACTOR, (k, v)


@pytest.mark.parametrize('n', hl.OTHER_SIZES)
def test_lower_only_case_garbage_is_visible(n):
    """symmetric=True reads the lower triangle only: the oracle on the matrix as given (garbage above the diagonal) must not be
    mistaken for the oracle on the mirrored one.  Where the garbage makes a factorisation raise, nothing is left to mistake."""
    Q, mirrored, q, ub, lb = hl.lower_only_case(n)
    assert np.array_equal(mirrored, mirrored.T) and np.array_equal(np.tril(Q), np.tril(mirrored))
    ref = hl.solve_all(mirrored, q, ub, lb, 'upper', n)
    assert ref['as']['status'] == 'optimal' and all(not ev['used_minres'] for ev in ref['as']['trace'])
    assert ref['x_star_method'] == 'cholesky'
    given = {}
    for name, run in (('as', lambda: bo.active_set(Q, q, ub, lb=lb, max_iter=hl.as_iters(n))),
                      ('ip', lambda: bo.interior_point(Q, q, ub, lb=lb, max_iter=hl.IP_ITERS)),
                      ('x_star', lambda: bo.x_star(Q, q)[0])):
        try:
            given[name] = run()
        except np.linalg.LinAlgError:
            given[name] = None
    for name, pairs in (('as', (('f_hist', hl.F_TOL), ('x', hl.X_TOL))), ('ip', (('f_hist', hl.F_TOL), ('x', hl.X_TOL)))):
        for key, tol in pairs:
            if given[name] is not None:
                assert hl.margin(given[name][key], ref[name][key], **tol) >= FACTOR, (name, key)
    if given['x_star'] is not None:
        assert hl.margin(given['x_star'], ref['x_star'], **hl.xstar_tol(ref['x_star'])) >= FACTOR


@pytest.mark.parametrize('n', hl.OTHER_SIZES)
def test_rounding_case_has_one_answer(n):
    """An exactly symmetric Q: either triangle gives the same bits, so the layout alone is under test there."""
    Q, q, ub, lb = hl.rounding_case(n)
    up, low = hl.solve_all(Q, q, ub, lb, 'upper', n), hl.solve_all(Q, q, ub, lb, 'lower', n)
    assert up['as']['status'] == 'optimal' and all(not ev['used_minres'] for ev in up['as']['trace'])
    assert up['x_star_method'] == 'cholesky'
    for k, v in _margins(low, up).items():
        assert v <= 1.0, (k, v)


# ---- kernel problems: the device builds K itself, so the reference must not hang on the last bits of K ----------------------------
def _gram(n):
    from oracle import svm_oracle as so
    return so.gram('rbf', hl.kernel_data(n)[0], gamma=hl.GAMMA)


@pytest.mark.parametrize('n', hl.SVC_SIZES)
def test_svc_case_is_a_stable_reference(n):
    """x_star takes the Cholesky branch; ActiveSet never takes minres; a Gram matrix 4 ulps away leaves every compared quantity
    within a tenth of its tolerance."""
    K = _gram(n)
    X, y, Q, q, ub = hl.svc_case(n)
    xs, method = bo.x_star(Q, q)
    assert method == 'cholesky' and np.linalg.cond(Q) < 1e5
    a = bo.active_set(Q, q, ub, max_iter=hl.as_iters(n), trace=True)
    assert a['status'] == 'optimal' and all(not ev['used_minres'] for ev in a['trace'])
    ip = bo.interior_point(Q, q, ub, max_iter=200)
    assert ip['status'] == 'optimal'
    if n == max(hl.SVC_SIZES):   # released variables border the kept factor: two of them meet in bq_as_schur.hip's V block
        assert sum(ev['kind'] == 'release' for ev in a['trace']) >= 2
    Qp = hl.svc_case(n, hl.perturbed(K, 4.0))[2]
    ap, ipp = bo.active_set(Qp, q, ub, max_iter=hl.as_iters(n)), bo.interior_point(Qp, q, ub, max_iter=200)
    m = {'x_star': hl.margin(bo.x_star(Qp, q)[0], xs, **hl.xstar_tol(xs)),
         'as f': hl.margin(ap['f_hist'], a['f_hist'], **hl.F_TOL), 'as x': hl.margin(ap['x'], a['x'], **hl.X_TOL),
         'ip f': hl.margin(ipp['f_hist'], ip['f_hist'], **hl.F_TOL), 'ip x': hl.margin(ipp['x'], ip['x'], **hl.X_TOL)}
    print(f'svc n={n}: cond(Q) {np.linalg.cond(Q):.3g}, 4 ulps of K move (tolerances) ' + ', '.join(f'{k} {v:.2g}' for k, v in m.items()))
    for k, v in m.items():
        assert v <= 0.1, (k, v)


@pytest.mark.parametrize('n', hl.SVR_SIZES)
def test_svr_case_interior_point_is_stable_and_active_set_only_in_its_end_point(n):
    """The 2n x 2n SVR Hessian [[P, -P], [-P, P]] is singular, and ActiveSet starts with every index free: its first iterations
    take the reference's minres branch, whose candidate carries rounding noise along the null directions (a+ + a-).  With K moved
    by one ulp the oracle's own f history moves by far more than any tolerance (5.4e5 tolerances at n = 40, 680 at n = 129; most
    iterations go through minres), so for SVR + ActiveSet only status, end point and final objective are a reference.
    InteriorPoint is stable."""
    K = _gram(n)
    X, Q, q, ub = hl.svr_case(n)
    Qp = hl.svr_case(n, hl.perturbed(K, 1.0))[1]
    ip, ipp = bo.interior_point(Q, q, ub, max_iter=200), bo.interior_point(Qp, q, ub, max_iter=200)
    assert ip['status'] == 'optimal'
    assert hl.margin(ipp['f_hist'], ip['f_hist'], **hl.F_TOL) <= 0.1 and hl.margin(ipp['x'], ip['x'], **hl.X_TOL) <= 0.1
    a = bo.active_set(Q, q, ub, max_iter=hl.as_iters(2 * n), trace=True)
    ap = bo.active_set(Qp, q, ub, max_iter=hl.as_iters(2 * n))
    assert a['status'] == 'optimal' and ap['status'] == 'optimal'
    assert a['trace'][0]['used_minres']
    hist = hl.margin(ap['f_hist'], a['f_hist'], **hl.F_TOL)
    print(f'svr n={n}: ActiveSet {a["iter"]} / {ap["iter"]} iterations, {sum(ev["used_minres"] for ev in a["trace"])} through minres; '
          f'one ulp of K moves the f history by {hist:.3g} tolerances, the end point by {hl.margin(ap["x"], a["x"], **hl.X_TOL):.2g}')
    assert hl.margin(ap['x'], a['x'], **hl.X_TOL) <= 0.1
    assert hl.margin(ap['f_x'], a['f_x'], **hl.F_TOL) <= 0.1


def test_plain_and_squared_hinge_cases_are_stable_references():
    n = 129
    X, Q, q, ub, diag = hl.plain_case(n)
    assert bo.x_star(Q, q)[1] == 'cholesky'
    a = bo.active_set(Q, q, ub, max_iter=hl.as_iters(n), trace=True)
    assert a['status'] == 'optimal' and all(not ev['used_minres'] for ev in a['trace'])
    assert any(ev['kind'] == 'release' for ev in a['trace']) and any(ev['kind'] == 'step' for ev in a['trace'])
    X, y, Q, q, ub, x0, diag = hl.sqhinge_case(n)
    a = bo.active_set(Q, q, ub, x0=x0, max_iter=hl.as_iters(n), trace=True)
    assert a['status'] == 'optimal' and all(not ev['used_minres'] for ev in a['trace'])
    assert sum(ev['kind'] == 'step' for ev in a['trace']) >= 10   # not solved by its first candidate


@pytest.mark.parametrize('n', hl.OTHER_SIZES)
def test_asymmetry_cases_sit_on_their_side_of_64_ulps(n):
    """The device keeps ActiveSet's shortcuts on row blocks while max |Q_ij - Q_ji| <= 64 ulps of max |Q|: the cases measure 1, 32
    and 128 (within one ulp), and the oracle does not tell the triangles of any of them apart."""
    Q, q, ub, lb = hl.rounding_case(n)
    for ulps in (1, 32, 128):
        Qa = hl.with_asymmetry(Q, ulps)
        assert not np.array_equal(Qa, Qa.T) and abs(hl.asymmetry_ulps(Qa) - ulps) <= 1.0
        up = hl.oracle_with_triangle(bo.active_set, 'upper', Qa, q, ub, lb=lb, max_iter=hl.as_iters(n))
        low = hl.oracle_with_triangle(bo.active_set, 'lower', Qa, q, ub, lb=lb, max_iter=hl.as_iters(n))
        assert hl.margin(low['f_hist'], up['f_hist'], **hl.F_TOL) <= 0.01 and hl.margin(low['x'], up['x'], **hl.X_TOL) <= 0.01
    for m in hl.NONSYM_SIZES:
        assert hl.asymmetry_ulps(hl.nonsymmetric_case(m)[0]) > 1e9


def test_oracle_with_triangle_restores_the_oracle():
    saved = bo.cho_factor
    with pytest.raises(ZeroDivisionError):
        hl.oracle_with_triangle(lambda: 1 / 0, 'lower')
    assert bo.cho_factor is saved
    with pytest.raises(ValueError):
        hl.oracle_with_triangle(lambda: None, 'both')
