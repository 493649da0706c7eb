"""tests/scoring_reference.py on the CPU: the restated scoring kernels against the project's own host path on random inputs,
against answers written out by hand at every threshold, and the preconditions of the pinned inputs that
tests/test_gpu_scoring_edges.py runs on the device, checked with the CPU oracle for the same iteration count."""
import functools
import math

import numpy as np
import pytest

import scoring_reference as sr

LO, HI = sr.LO, sr.HI


# ---- 1. the reference against the host path -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('seed', range(4))
def test_svr_scores_against_svr_intercept(seed):
    """b against svr_intercept (NumPy's pairwise sum: another order of the same terms) and sse against the NumPy sum, at the bounds
    the device is held to; the counts exactly"""
    from optiml_amd.ml.svm._batched import svr_intercept
    rs = np.random.RandomState(seed)
    n = (5, 37, 300, 1100)[seed]
    x = np.where(rs.rand(2 * n) < 0.5, 0., rs.rand(2 * n))
    u, y = rs.standard_normal(n), rs.standard_normal(n)
    ub = np.where(rs.rand(n) < 0.3, 0., 1.)
    ub = np.hstack((ub, ub))
    b, n_sv, sse, n_held = sr.svr_scores(x, u, y, ub, 0.1)
    sv = (x[:n] > 1e-6) | (x[n:] > 1e-6)
    te = ub[:n] == 0
    assert n_sv == sv.sum() > 0 and n_held == te.sum() > 0
    sr.check_intercept('svr %d' % n, svr_intercept(y, u, sv, 0.1), b, y[sv] - u[sv], 0.1, n_sv)
    sr.check_sse('svr %d' % n, float(((y[te] - (u[te] + b)) ** 2).sum()), sse, n_held)
    assert sr.svr_scores(x, u, y, ub, 0.1, b_used=b)[2] == sse and sr.svr_scores(x, u, y, ub, 0.1, b_used=b + 1.0)[2] != sse


@pytest.mark.parametrize('seed', range(4))
def test_svc_scores_against_intercept(seed):
    from optiml_amd.ml.svm._batched import intercept
    rs = np.random.RandomState(10 + seed)
    n = (5, 37, 300, 1100)[seed]
    x = np.where(rs.rand(n) < 0.5, 0., rs.rand(n))
    u, sgn = rs.standard_normal(n), np.where(rs.rand(n) < 0.5, 1., -1.)
    ub = np.where(rs.rand(n) < 0.3, 0., 1.)
    b, n_sv, dec, lab = sr.svc_scores(x, u, sgn, ub)
    sv, te = x > 1e-6, ub == 0
    assert n_sv == sv.sum() > 0 and te.sum() > 0
    sr.check_intercept('svc %d' % n, intercept(sgn, u, sv), b, sgn[sv] - u[sv], 0., n_sv)
    assert np.array_equal(dec[te], u[te] + b) and np.array_equal(lab[te], sgn[te]) and not dec[~te].any() and not lab[~te].any()
    assert np.array_equal(sr.svc_scores(x, u, sgn, ub, b_used=0.25)[2][te], u[te] + 0.25)


@pytest.mark.parametrize('paired', [False, True], ids=['labels', 'paired'])
@pytest.mark.parametrize('seed', range(3))
def test_nu_scores_against_the_numpy_expressions(seed, paired):
    """the expressions of test_gpu_nu_cv._check_against_host, written out"""
    rs = np.random.RandomState(20 + seed)
    n = (5, 300, 1100)[seed]
    u = rs.standard_normal(n)
    r1, r2 = 0.7 + rs.rand(), 0.2 + rs.rand()
    rho, scale = (r1 - r2) / 2, (r1 + r2) / 2
    mask = np.where(rs.rand(n) < 0.3, 0., 1.)
    if paired:
        ub, y = np.hstack((mask, mask)), rs.standard_normal(n)
        te = (ub[:n] == 0) & (ub[n:] == 0)
        n_held, n_correct, sse = sr.nu_scores(None, u, y, ub, r1, r2, True)
        assert n_held == te.sum() > 0 and n_correct == 0
        sr.check_sse('nu %d' % n, float(((y[te] - (u[te] - rho)) ** 2).sum()), sse, n_held)
    else:
        y = np.where(rs.rand(n) < 0.5, 1., -1.)
        te = mask == 0
        pred = np.where((u - rho) / scale > 0, 1., -1.)
        assert sr.nu_scores(None, u, y, mask, r1, r2, False) == (te.sum(), int((pred[te] == y[te]).sum()), 0.)


# ---- 2. five rows per threshold, the answers by hand --------------------------------------------------------------------------------
def test_svr_support_threshold_by_hand():
    """x+ = 1e-6 is no support vector, one ulp above is one; the same on x-; either half is enough.  The support rows are 1, 3, 4:
    y - u = 2, 8, 16, so b = (26 - 0.5) / 3 = 8.5"""
    xp = np.array([LO, HI, 0., 0., 0.5])
    xn = np.array([0., 0., LO, HI, 0.])
    y, u = np.array([1., 2., 4., 8., 16.]), np.zeros(5)
    b, n_sv, _, _ = sr.svr_scores(np.hstack((xp, xn)), u, y, np.ones(10), 0.5)
    assert (b, n_sv) == (8.5, 3)
    none = sr.svr_scores(np.full(10, LO), u, y, np.zeros(10), 0.5)   # no support vector: NaN, and the held count stays exact
    assert math.isnan(none[0]) and math.isnan(none[2]) and none[1] == 0 and none[3] == 5


def test_svr_held_threshold_by_hand():
    """Held: ub = 0 on BOTH halves, and -0.0 is 0.  The rows 0 (0, 0) and 1 (-0.0, 0) are held, the rows 2 (0, 1), 3 (1, 0) and
    4 (1, 1) are not.  With b_used = 0.5 the residuals of rows 0, 1 are 3 - (1 + 0.5) = 1.5 and 1 - (2 + 0.5) = -1.5: sse = 4.5"""
    ub = np.array([0., -0.0, 0., 1., 1.] + [0., 0., 1., 0., 1.])
    y, u = np.array([3., 1., 100., 100., 100.]), np.array([1., 2., 0., 0., 0.])
    _, n_sv, sse, n_held = sr.svr_scores(np.ones(10), u, y, ub, 0., b_used=0.5)
    assert (n_sv, sse, n_held) == (5, 4.5, 2)


def test_svc_thresholds_by_hand():
    """Support rows: x > 1e-6, the rows 1 and 4 — sgn - u = 1 - 3 and -1 - 0, so b = -3 / 2.  Held: ub == 0, the rows 0 and 2
    (-0.0): dec = u + b = 0.5 and -0.5 there, 0 elsewhere, and lab = sgn there"""
    x = np.array([0., HI, LO, 0.5e-6, 1.])
    u, sgn = np.array([2., 3., 1., 7., 0.]), np.array([1., 1., -1., 1., -1.])
    ub = np.array([0., 1., -0.0, 1e-300, 1.])
    b, n_sv, dec, lab = sr.svc_scores(x, u, sgn, ub)
    assert (b, n_sv) == (-1.5, 2)
    assert dec.tolist() == [0.5, 0., -0.5, 0., 0.] and lab.tolist() == [1., 0., -1., 0., 0.]


def test_svc_pair_rows_by_hand():
    """Classes of one tile row each, n = 768 = 3 x 256, pair (0, 2).  Of the rows 0 (class 0, data, held), 1 (class 0, ghost, ub 0),
    300 (class 1, ub 0), 600 (class 2, data, held) and 601 (class 2, data, trained, the support vector) only 0 and 600 are written"""
    n = 768
    x, u, sgn, ub, data = np.zeros(n), np.zeros(n), -np.ones(n), np.zeros(n), np.zeros(n, dtype=np.uint8)
    data[[0, 300, 600, 601]] = 1
    ub[601], x[601], sgn[600:] = 1., 1., 1.
    u[[0, 1, 300, 600, 601]] = [1., 2., 3., 4., 0.5]
    b, n_sv, dec, lab = sr.svc_scores(x, u, sgn, ub, pair=(0, 2), ct=[0, 1, 2, 3], data_row=data)
    assert (b, n_sv) == (0.5, 1)
    assert np.flatnonzero(dec).tolist() == [0, 600] and dec[0] == 1.5 and dec[600] == 4.5
    assert np.flatnonzero(lab).tolist() == [0, 600] and lab[0] == -1. and lab[600] == 1.


def test_nu_labels_decision_threshold_by_hand():
    """r1 = 3, r2 = 1: rho = 1, scale = 2.  u - rho = 0, -0.0 (u = 1), one ulp above 0, -1, 2 give -1, -1, +1, -1, +1; row 4 is not
    held.  Against y = +1 everywhere one held row is right, against -1 three, and the two add up to the four held rows"""
    u = np.array([1., 1., float(np.nextafter(1., 2.)), 0., 3.])
    ub = np.array([0., -0.0, 0., 0., 1.])
    assert sr.nu_scores(None, u, np.ones(5), ub, 3., 1., False) == (4, 1, 0.)
    assert sr.nu_scores(None, u, -np.ones(5), ub, 3., 1., False) == (4, 3, 0.)
    assert sr.nu_scores(None, u, np.array([-1., -1., 1., -1., 1.]), ub, 3., 1., False) == (4, 4, 0.)


def test_nu_paired_held_threshold_by_hand():
    """Held: ub = 0 on both halves — the rows 0 and 1 (0, -0.0); ub = 0 on the first half alone (row 2) or on the second alone (row 3)
    is a trained row.  r1 = r2 = 1: rho = 0; the residuals of the held rows are 2 - 0.5 and -1 - 0.5: sse = 4.5"""
    ub = np.array([0., 0., 0., 1., 1.] + [0., -0.0, 1., 0., 1.])
    y, u = np.array([2., -1., 1e8, 1e8, 1e8]), np.full(5, 0.5)
    assert sr.nu_scores(None, u, y, ub, 1., 1., True) == (2, 0, 4.5)


def test_the_bounds_by_hand():
    assert sr.intercept_bound(np.array([1., -2., 3.]), -0.5, 3) == 6 * 2.0 ** -53 * 6.5 / 3
    assert sr.sse_bound(2.0, 5) == 14 * 2.0 ** -53 * 2.0


# ---- 3. the preconditions of the GPU inputs, with the oracle -------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _oracle_run(kind, n):
    """projected_gradient for the GPU tests' iteration count on the Q, q, ub, x0 of every column of the case, with its trace"""
    from oracle import bcqp_oracle as bo, svm_oracle as so
    case = sr.svr_case(n) if kind == 'svr' else sr.svc_case(n)
    K = so.gram('rbf', case['X'], gamma=sr.SVR_GAMMA if kind == 'svr' else sr.SVC_GAMMA)
    out = []
    for c in range(len(case['UB'])):
        if kind == 'svr':
            Q, q, _ = so.svr_dual(K, case['y'], 1.0, case['eps'][c])
            assert np.array_equal(q, case['QL'][c])
        else:
            Q, _, _ = so.svc_dual(K, case['Y'][c], 1.0)
            q = case['q']
        out.append(bo.projected_gradient(Q, q, case['UB'][c], x0=case['x0'][c], max_iter=sr.BOX_ITERS, trace=True))
    return case, K, out


def _pinned_coordinates(kind, n, pins):
    if kind == 'svr':
        return [(r if half == '+' else n + r, n + r if half == '+' else r, cap) for r, half, cap in pins]
    return [(r, None, cap) for r, cap in pins]


@pytest.mark.parametrize('kind,n', [('svc', 1024), ('svc', 1025), ('svc', 2049), ('svr', 1024), ('svr', 1025), ('svr', 2049)])
def test_pinned_inputs_with_the_oracle(kind, n):
    """(a) every pinned coordinate ends bit-equal to its cap (and the other half of an SVR pin at 0); its gradient points outward by a
    margin in every iteration, and its kernel values to every other row are 0.  (b) every column except the empty one has a support
    vector below row 1024 and, where it trains rows past 1024 (the block fold holds them all out), one at or past 1024.  (c) no other
    x lies in [0.5e-6, 2e-6], so the support set cannot flip between the oracle and the device through rounding.  The held rows stay
    at 0, the -0.0 boxes included."""
    case, K, runs = _oracle_run(kind, n)
    rows = sorted({p[0] for pins in case['pins'] for p in pins})
    assert len(rows) == (8 if kind == 'svr' else 4)
    assert sum(r >= 1024 for r in rows) == (0 if n == 1024 else 1 if n == 1025 else len(rows) // 2)
    off = K[rows].copy()
    off[np.arange(len(rows)), rows] = 0.
    assert not off.any() and np.all(K[rows, rows] == 1.)
    for c, (res, pins, held) in enumerate(zip(runs, case['pins'], case['held'])):
        x = res['x']
        assert res['iter'] == sr.BOX_ITERS or c == case['empty']
        pinned = np.zeros(len(x), dtype=bool)
        for at, other, cap in _pinned_coordinates(kind, n, pins):
            assert x[at] == cap, (c, at, x[at])
            out = max(t['g'][at] for t in res['trace'])
            assert out < -0.1, (c, at, out)
            pinned[at] = True
            if other is not None:
                assert x[other] == 0. and min(t['g'][other] for t in res['trace']) > 0.1
                pinned[other] = True
        every = np.concatenate((held, n + held)) if kind == 'svr' else held
        assert not x[every].any()
        if c == case['empty']:
            assert not x.any() and res['iter'] == 0
            continue
        assert len(pins) > 0 and {cap for _, _, cap in _pinned_coordinates(kind, n, pins)} == {LO, HI}
        sv = (x[:n] > 1e-6) | (x[n:] > 1e-6) if kind == 'svr' else x > 1e-6
        assert sv[:1024].any()
        trains_past = np.setdiff1d(np.arange(1024, n), held).size > 0
        assert sv[1024:].any() == trains_past
        free = x[~pinned]
        assert not ((free >= 0.5e-6) & (free <= 2e-6)).any(), (c, free[(free >= 0.5e-6) & (free <= 2e-6)])
        print('%s n = %d column %d: %d support rows, %d past 1024, %d pins' % (kind, n, c, sv.sum(), sv[1024:].sum(), len(pins)))


@pytest.mark.parametrize('n', sr.SIZES)
def test_case_layout(n):
    """What the GPU tests rely on: the block fold holds out exactly [1024, n); the -0.0 boxes sit on held rows; the one-half-zero rows
    of the PAIRED column are trained rows of its fold"""
    svr, svc = sr.svr_case(n), sr.svc_case(n)
    if n > 1024:
        for case in (svr, svc):
            assert np.array_equal(case['held'][2], np.arange(1024, n))
        assert np.array_equal(np.flatnonzero((svr['UB'][2][:n] == 0) & (svr['UB'][2][n:] == 0)), np.arange(1024, n))
        assert np.array_equal(np.flatnonzero(svc['UB'][2] == 0), np.arange(1024, n))
    assert len(svr['UB']) == len(svc['UB']) == (4 if n > 1024 else 3)
    assert np.signbit(svr['UB'][0][[3, n + 3, n + 6]]).all() and not np.signbit(svr['UB'][0][6]) and svr['UB'][0][6] == 0.
    assert np.signbit(svc['UB'][0][3]) and svc['UB'][0][3] == 0.
    first, second = sr.half_zero_rows(n)
    assert all(r % 3 == 1 and r < n for r in first + second) and len(set(first + second)) == 4
    assert sum(r >= 1024 for r in first) == sum(r >= 1024 for r in second) == (1 if n >= 2049 else 0) or n == 1025
    for ub in svr['UB']:   # what bq_msolver_create_svr_boxes requires
        assert np.array_equal(ub[:n] == 0, ub[n:] == 0) and (ub >= 0).all()
