"""The held-out scoring kernels of bq_mscore.hip (msvr_score_kernel, mscore_intercept / mheldout_kernel, msx_score_kernel<PAIRED>,
mvote_kernel / mvote_count_kernel) on pinned states and past 1024 rows, against tests/scoring_reference.py: the same statements in
NumPy with exactly rounded sums.

Every scoring kernel is one workgroup of 1024 threads per column that walks i = tid, tid + 1024, ...; the sizes here are 1024 (one
trip), 1025 (one row into the second trip) and 2049 (one row into the third), and the folds are two interleaved ones (i % 3) and a
block fold whose held rows are exactly [1024, n).  The thresholds (x > 1e-6 is a support vector, ub == 0 is a held row, on both
halves for SVR and PAIRED) are met exactly: rows pinned through their box to 1e-6 and to one ulp above it (scoring_reference.svr_case
/ svc_case, whose preconditions tests/test_scoring_edges_host.py checks with the CPU oracle), -0.0 boxes on held rows, and PAIRED rows
with a zero box on one half only.

u is obtained as the neighbouring files obtain it: the coefficients formed on the host from the downloaded x, then the same
batch-invariant product the device takes (bq_problem_gram_matmat_wide, bq_problem_gram_matmat_pairs), so u has the device's bits and
the counts, predictions, labels and decision values are compared with ==.  The intercepts and squared errors are held to
scoring_reference.intercept_bound / sse_bound, which follow from the arithmetic.

Not reachable at test size, and not faked: mvote_count_kernel's own stride takes more than 1024 blocks of 64 rows, n > 65536; a
non-positive or NaN scale in msx_score_kernel stays covered by the failed-fit tests of test_gpu_nu_cv.py.
"""
import numpy as np
import pytest

import scoring_reference as sr
import test_gpu_nu as tgn
import test_gpu_nu_cv as tgnc
import test_gpu_ovo as tgo
import test_gpu_ovo_search as tgos
import test_gpu_svr_cv as tgs

pytestmark = pytest.mark.gpu

PAIR_SIZES = [1030, 6, 260]   # class 0: five tile rows, 1280 panel rows with the ghosts 1030 ... 1279; a tiny class between two large ones


@pytest.fixture(scope='module')
def amd():
    from optiml_amd import _lib
    from optiml_amd.device import get_context
    _lib.load()
    get_context()


def _assert_pinned(n, x, ub, pins, svr):
    """the state the test wants, on the downloaded x: if this fails the input is wrong, not the kernel"""
    for pin in pins:
        if svr:
            r, half, cap = pin
            at, other = (r, n + r) if half == '+' else (n + r, r)
            assert x[at] == cap and x[other] == 0., (pin, x[at], x[other])
        else:
            r, cap = pin
            assert x[r] == cap, (pin, x[r])
    assert not x[ub == 0].any()


# ---- 1. bq_msolver_svr_heldout ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', sr.SIZES)
def test_svr_heldout_on_pinned_states(amd, n):
    """Two rows pinned at 1e-6 and two one ulp above it on each half (half of them past row 1024 where n allows, row 2048 among
    them), the other half at 0; a -0.0 box pair and a (+0.0, -0.0) pair on held rows; the last column without a support vector.
    n_sv and n_held with ==, b and sse to the bounds (sse with the device's b in the residuals)."""
    from optiml_amd import _lib
    from optiml_amd.ml.svm._batched import _gram_matmat
    from optiml_amd.ml.svm.kernels import GaussianKernel
    case = sr.svr_case(n)
    y, UB, eps = case['y'], case['UB'], case['eps']
    quad = tgs._quad(case['X'], 'f64', GaussianKernel(gamma=sr.SVR_GAMMA))
    dev = quad.device_problem()
    res = tgs._solve(dev, _lib.PG, case['QL'], UB, sr.BOX_ITERS, x0=case['x0'], y=y, epsilons=eps)
    k = len(res)
    W = np.zeros((k, n))
    for j, r in enumerate(res):
        _assert_pinned(n, r['x'], UB[j], case['pins'][j], True)
        xp, xn = r['x'][:n], r['x'][n:]
        sv = (xp > 1e-6) | (xn > 1e-6)
        W[j][sv] = xp[sv] - xn[sv]
    U = _gram_matmat(dev, W, wide=True)
    quad.release()
    for j, r in enumerate(res):
        b, n_sv, sse, n_held = sr.svr_scores(r['x'], U[j], y, UB[j], eps[j], b_used=r['b'])
        assert r['n_held'] == n_held == len(case['held'][j]) > 0, j
        assert r['n_sv'] == n_sv, (j, r['n_sv'], n_sv)
        if j == case['empty']:
            assert n_sv == 0 and np.isnan(r['b']) and np.isnan(r['sse']) and r['iter'] == 0
            continue
        assert r['iter'] == sr.BOX_ITERS
        sv = (r['x'][:n] > 1e-6) | (r['x'][n:] > 1e-6)
        hi = sum(cap == sr.HI for _, _, cap in case['pins'][j])
        assert hi > 0 and sum(sv[p[0]] for p in case['pins'][j]) == hi   # the pins one ulp above 1e-6 count, those at 1e-6 do not
        sr.check_intercept('svr n = %d column %d' % (n, j), r['b'], b, y[sv] - U[j][sv], eps[j], n_sv)
        sr.check_sse('svr n = %d column %d' % (n, j), r['sse'], sse, n_held)
    if n > 1024:
        assert res[2]['n_held'] == n - 1024   # the block fold: 1 row at n = 1025, 1025 rows at n = 2049
    assert res[0]['n_held'] == (n + 2) // 3 and res[case['empty']]['n_held'] == n // 3


# ---- 2. bq_msolver_svc_heldout ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', sr.SIZES)
def test_svc_heldout_on_pinned_states(amd, n):
    """Two rows pinned at 1e-6 and two one ulp above it, a -0.0 box on a held row, a column that feeds no calibrator.  n_sv with ==, b
    to the bound; dec is u + b_dev bit for bit on the held rows and exactly 0 on every other row, the rows past 1024 that are not held
    included; the Platt fit of the returned sample, called again, gives the returned figures bit for bit."""
    from optiml_amd import _lib
    from optiml_amd.ml.svm._batched import _gram_matmat, platt_fit, solve_batched
    from optiml_amd.ml.svm.kernels import GaussianKernel
    from optiml_amd.opti import KernelQuadratic
    case = sr.svc_case(n)
    Y, UB, cal_of, ncal = case['Y'], case['UB'], case['cal_of'], case['ncal']
    quad = KernelQuadratic(case['X'], case['q'], 'svc', GaussianKernel(gamma=sr.SVC_GAMMA), y=np.ones(n))
    dev = quad.device_problem()
    got = {}

    def score(solver, _):
        got['b'], got['n_sv'], got['fit'] = solver.heldout_svc(cal_of, ncal, decisions=True)

    res = solve_batched(dev, _lib.PG, Y, UB, eps=1e-6, max_iter=sr.BOX_ITERS, x0=case['x0'], before_close=score)
    k = len(res)
    W = np.zeros((k, n))
    for j, r in enumerate(res):
        assert r['iter'] == sr.BOX_ITERS
        _assert_pinned(n, r['x'], UB[j], case['pins'][j], False)
        sv = r['x'] > 1e-6
        W[j][sv] = r['x'][sv] * Y[j][sv]
    U = _gram_matmat(dev, W, wide=True)
    quad.release()
    dec, lab = np.zeros((ncal, n)), np.zeros((ncal, n))
    for j, r in enumerate(res):
        b, n_sv, d, l = sr.svc_scores(r['x'], U[j], Y[j], UB[j], b_used=got['b'][j])
        sv = r['x'] > 1e-6
        assert got['n_sv'][j] == n_sv > 0, (j, got['n_sv'][j], n_sv)
        assert [bool(sv[row]) for row, _ in case['pins'][j]] == [cap == sr.HI for _, cap in case['pins'][j]]
        sr.check_intercept('svc n = %d column %d' % (n, j), got['b'][j], b, Y[j][sv] - U[j][sv], 0., n_sv)
        if cal_of[j] >= 0:
            assert np.count_nonzero(l) == len(case['held'][j]) > 0 and not lab[cal_of[j]][l != 0].any()
            dec[cal_of[j]] += d
            lab[cal_of[j]] += l
    fit = got['fit']
    assert np.array_equal(fit['dec'], dec) and np.array_equal(fit['dec'] != 0, lab != 0)
    if n > 1024:
        assert np.count_nonzero(fit['dec'][1]) == n - 1024 and not fit['dec'][1][:1024].any()   # the block fold's calibrator
        assert np.count_nonzero(fit['dec'][0][1024:]) == np.count_nonzero(np.arange(1024, n) % 3 != 2)
    again = platt_fit(fit['dec'], lab)
    for key in again:
        assert np.array_equal(again[key], fit[key], equal_nan=again[key].dtype.kind == 'f'), key
    assert np.array_equal(fit['n_pos'], (lab > 0).sum(axis=1)) and np.array_equal(fit['n_neg'], (lab < 0).sum(axis=1))


# ---- 3. bq_msolver_simplex2_heldout -------------------------------------------------------------------------------------------------
def _simplex_run(dev, S, UB, mass, Q, tol, ys):
    """the columns run to the end (60 iterations at most), offsets(), heldout(y) for every y of ys, and the columns' x"""
    from optiml_amd import _lib
    solver = tgnc._solver(dev, S, UB, mass, Q, tol, sr.SIMPLEX_ITERS)
    try:
        tgnc._finish(solver)
        off = solver.offsets()
        held = [solver.heldout(y) for y in ys]
        x = [solver.get(c, _lib.GET_X_NOW) for c in range(solver.k)]
        return off, held, x
    finally:
        solver.close()


def _same_offsets(held, off):
    return all(np.array_equal(h, o) for h, o in zip(held[:4], off))


@pytest.mark.parametrize('n', sr.SIZES)
def test_simplex2_heldout_labels_past_1024_rows(amd, n):
    """LABELS: the same state scored with y = the labels, y = +1 everywhere and y = -1 everywhere.  Each matches the reference; the
    rows right against +1 and against -1 add up to the held rows exactly; and both signs occur among a column's held rows."""
    from optiml_amd.ml.svm._batched import _gram_matmat
    from optiml_amd.ml.svm.kernels import GaussianKernel
    X, yc, _ = tgn._data(n, 31)
    helds = sr.folds(n)
    k = len(helds)
    mask = np.ones((k, n))
    for c, held in enumerate(helds):
        mask[c, held] = 0.
    S, UB, mass = tgn._labels_columns(yc, [0.3517, 0.5017, 0.4017][:k], mask)
    quad = tgn._quad(X, GaussianKernel(gamma=1.0 / 3))
    dev = quad.device_problem()
    ys = [yc, np.ones(n), -np.ones(n)]
    off, scored, x = _simplex_run(dev, S, UB, mass, None, 1e-3, ys)
    U = _gram_matmat(dev, np.stack([np.where(UB[c] > 0, S[c], 1.) * x[c] for c in range(k)]), wide=True)
    quad.release()
    both = 0
    for c in range(k):
        right = []
        for y, held in zip(ys, scored):
            assert _same_offsets([h[c] for h in held], [o[c] for o in off])
            want = sr.nu_scores(x[c], U[c], y, UB[c], held[0][c], held[1][c], False)
            assert (held[4][c], held[5][c], held[6][c]) == want, (c, held[4][c], held[5][c], want)
            assert held[4][c] == len(helds[c])
            right.append(int(held[5][c]))
        print('labels n = %d column %d: held %d, right %d, right against +1 %d, against -1 %d' % (n, c, len(helds[c]), *right))
        assert right[1] + right[2] == len(helds[c])
        both += 0 < right[1] < len(helds[c])
    assert both > 0


@pytest.mark.parametrize('n', sr.SIZES)
def test_simplex2_heldout_paired_past_1024_rows(amd, n):
    """PAIRED: column 0 has two rows with ub = 0 on the first half only and two with ub = 0 on the second half only
    (scoring_reference.half_zero_rows); none of them is counted or enters the squared error.  Scored with the targets and with a y
    whose entries span 1e-8 ... 1e8 in magnitude: the bound is relative to the reference's sum and holds for both."""
    from optiml_amd.ml.svm._batched import _gram_matmat
    from optiml_amd.ml.svm.kernels import GaussianKernel
    X, _, t = tgn._data(n, 31)
    helds = sr.folds(n)
    k = len(helds)
    mask = np.ones((k, n))
    for c, held in enumerate(helds):
        mask[c, held] = 0.
    UB, mass, Q = tgn._paired_columns(t, [(1.0, 0.5017), (0.5, 0.4017), (1.0, 0.3017)][:k], mask)
    first, second = sr.half_zero_rows(n)
    UB[0][first] = 0.
    UB[0][[n + r for r in second]] = 0.
    wide = (10.0 ** (np.arange(n) % 17 - 8.0)) * np.where(np.arange(n) % 2 == 0, 1., -1.)
    quad = tgn._quad(X, GaussianKernel(gamma=1.0 / 3))
    dev = quad.device_problem()
    ys = [t, wide]
    off, scored, x = _simplex_run(dev, None, UB, mass, Q, 0.1, ys)
    U = _gram_matmat(dev, np.stack([x[c][:n] - x[c][n:] for c in range(k)]), wide=True)
    quad.release()
    for c in range(k):
        assert x[c][:n][UB[c][:n] == 0].sum() == 0. and x[c][n:][UB[c][n:] == 0].sum() == 0.
        for name, y, held in zip(('targets', '1e-8 ... 1e8'), ys, scored):
            assert _same_offsets([h[c] for h in held], [o[c] for o in off])
            n_held, n_correct, sse = sr.nu_scores(x[c], U[c], y, UB[c], held[0][c], held[1][c], True)
            assert held[4][c] == n_held == len(helds[c]), (c, held[4][c], n_held, len(helds[c]))
            assert held[5][c] == n_correct == 0 and sse > 0
            sr.check_sse('paired n = %d column %d, %s' % (n, c, name), held[6][c], sse, n_held)
        mags = np.abs(wide[helds[c]])
        assert len(helds[c]) == 1 or (mags.min() == 1e-8 and mags.max() == 1e8)
    assert not np.isin(first + second, helds[0]).any()


# ---- 4. bq_msolver_pairs_heldout ----------------------------------------------------------------------------------------------------
def test_pairs_heldout_with_a_class_past_1024_rows(amd):
    """Class sizes 1030, 6, 260 on one pair solver, built as test_gpu_coupling.heldout_run builds it (3 folds i % 3 over the data
    rows, the (pair, fold) and (pair, all) columns, ProjectedGradient): class 0 spans 1280 panel rows, so mheldout_kernel's per-class
    loop takes its second trip, over the data rows 1024 ... 1029 and the ghosts after them.  n_sv with ==, b to the bound; dec is
    u + b_dev bit for bit on exactly the held data rows of the pair's two classes and 0 on ghost rows, on the rows of the third class
    and on trained rows; the Platt refit of the returned sample is bit-equal."""
    from optiml_amd import _lib
    from optiml_amd.ml.svm._batched import gram_matmat_pairs, platt_fit, solve_batched
    from optiml_amd.ml.svm.coupling import chunk_calibrators, coupling_columns
    from optiml_amd.ml.svm.onevsone import _DevicePairSolver
    _, y, Xp, ct, pcode, ghost, index = tgo._blob_panel(PAIR_SIZES)
    rows = np.arange(len(y))
    plan = coupling_columns(y, 3, [(rows[rows % 3 != f], rows[rows % 3 == f]) for f in range(3)], 1.0)
    n_pad = plan['n_pad']
    assert np.array_equal(plan['index'], index) and list(plan['cls_tiles']) == list(ct) == [0, 5, 6, 8]
    # sort_plan pads every class to whole tile rows, so the panel does not end ragged: ct[cls + 1] * 256 <= n for every class and the
    # kernel's clip by n binds for none
    assert n_pad == 256 * ct[-1] == len(pcode) == 2048
    assert np.array_equal(np.flatnonzero(ghost & (pcode == 0)), np.arange(1030, 1280))
    Y, UB, data = plan['Y'], plan['UB'], plan['data_row'] > 0
    pairs = [plan['pairs'][p] for p, _ in plan['cols']]
    cal_of, _ = chunk_calibrators(plan['cols'])
    quad = tgo._quad(Xp)
    dev = quad.device_problem()
    got = {}

    def score(solver, _):
        got['b'], got['n_sv'], got['fit'] = solver.heldout_pairs(plan['data_row'], cal_of, 3, decisions=True)

    solver = _DevicePairSolver(dev, _lib.PG, plan['cls_tiles'], pairs, Y, UB, 1e-6, sr.BOX_ITERS)
    res = solve_batched(dev, _lib.PG, Y, UB, max_iter=sr.BOX_ITERS, solver=solver, before_close=score)
    assert len(res) == 12
    W = np.zeros((12, n_pad))
    for j, r in enumerate(res):
        sv = r['x'] > 1e-6
        W[j][sv] = r['x'][sv] * Y[j][sv]
        assert not r['x'][UB[j] == 0].any()
    U = gram_matmat_pairs(dev, plan['cls_tiles'], pairs, W)
    quad.release()
    dec, lab = np.zeros((3, n_pad)), np.zeros((3, n_pad))
    for j, (r, (p, f)) in enumerate(zip(res, plan['cols'])):
        b, n_sv, d, l = sr.svc_scores(r['x'], U[j], Y[j], UB[j], b_used=got['b'][j], pair=pairs[j], ct=ct, data_row=plan['data_row'])
        sv = r['x'] > 1e-6
        assert got['n_sv'][j] == n_sv > 0, (j, got['n_sv'][j], n_sv)
        sr.check_intercept('pairs column %d' % j, got['b'][j], b, Y[j][sv] - U[j][sv], 0., n_sv)
        if f is not None:
            assert cal_of[j] == p and np.count_nonzero(l) > 0 and not lab[p][l != 0].any()
            dec[p] += d
            lab[p] += l
    fit = got['fit']
    assert np.array_equal(fit['dec'], dec) and np.array_equal(fit['dec'] != 0, lab != 0)
    for p, (a, b) in enumerate(plan['pairs']):
        mine = ((pcode == a) | (pcode == b)) & data
        assert np.array_equal(fit['dec'][p] != 0, mine)   # every data row of the pair is held out by exactly one fold; nothing else
        assert fit['n_pos'][p] == PAIR_SIZES[b] and fit['n_neg'][p] == PAIR_SIZES[a]
    assert fit['dec'][0][1024:1030].all() and fit['dec'][1][1024:1030].all() and not fit['dec'][:, 1030:1280].any()
    again = platt_fit(fit['dec'], lab)
    for key in again:
        assert np.array_equal(again[key], fit[key], equal_nan=again[key].dtype.kind == 'f'), key


# ---- 5. bq_msolver_pairs_vote_heldout -----------------------------------------------------------------------------------------------
def test_vote_heldout_with_a_class_past_1024_rows(amd):
    """The same class sizes through test_gpu_ovo_search._Layout, 3 groups (the folds 0 ... 2, one C): mvote_kernel's class lookup
    walks a class of five tile rows and then a tiny one.  test_gpu_ovo_search._check_against_host as it is, and: pred is -1 on every
    ghost row; the rows 1024 ... 1029 of class 0, the part of it past the first 1024 rows, are voted on and counted; n_correct of a
    group is the sum over the classes of (pred == class) on its held rows."""
    lay = tgos._Layout(PAIR_SIZES, [(f, 1.0) for f in range(3)])
    assert list(lay.ct) == [0, 5, 6, 8] and lay.n_pad == 2048
    quad = tgo._quad(lay.Xp)
    dev = quad.device_problem()
    groups = [0, 1, 2]
    out, x = tgos._scored(lay, dev, groups, max_iter=sr.BOX_ITERS)
    tgos._check_against_host(lay, dev, groups, out, x)
    quad.release()
    _, _, n_held, n_correct, pred = out
    ghost = lay.data_row == 0
    assert np.array_equal(np.flatnonzero(ghost & (lay.pcode == 0)), np.arange(1030, 1280))
    assert (pred[:, ghost] == -1).all()
    past = np.arange(1024, 1030)
    assert lay.held[:, past].sum() == 6 and lay.held[:, past].sum(axis=0).max() == 1   # each is held by exactly one group
    for g in groups:
        h = lay.held[g] > 0
        assert np.array_equal(pred[g] >= 0, h) and (pred[g][h] < 3).all()
        assert n_held[g] == h.sum() and h[past].any()
        assert n_correct[g] == sum(int(((pred[g] == cls) & (lay.pcode == cls) & h).sum()) for cls in range(3))
    assert n_held.sum() == sum(PAIR_SIZES)
