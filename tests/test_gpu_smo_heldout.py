"""GPU tests of the held-out scorers of the batched SMO walkers (`bq_msmo_svr_heldout`, `bq_msmo_svc_heldout`: msmo_coef_kernel<SVR>,
the 16-column product, msmo_svr_score_kernel / msmo_svc_score_kernel, the Platt kernel) and of the two estimators on them:
`SVRGridSearchCV` and `CalibratedSVC` over SMO estimators.

The scorer is held to the state it read: every column's multipliers and scalars are downloaded (`bq_msmo_get`), the coefficients are
formed in NumPy and multiplied by the same product (`_gram_matmat(dev, W, wide=True)`, whose columns have the same bits in any slot),
so counts, intercepts and decision values are compared with ==, and a squared error at `scoring_reference.sse_bound` against an
exactly rounded sum over the device's own intercept.  The sigmoids are compared bit for bit with `bq_platt_fit` on the downloaded
sample (the same kernel on the same bits) and, where `platt_reference`'s own preconditions hold for the sample (no stop test and no
line-search test decided by a hair: test_gpu_calibration.py's statement), with that reference at `PLATT_RTOL`, A and B relative to
the larger of the two (they solve 2 x 2 systems together); the counts always.  The Platt kernel itself is test_gpu_calibration.py's
subject; here it runs on the scorer's buffers.

Sizes: n = 240 (one tile row, fewer rows than the 1024 threads), 1025 (the second 1024-stride trip holds one row; the last 64 rows
span two tile rows) and 2049 (a third trip of one row); 1, 17 and 36 columns (one product chunk, a second chunk of one column,
three chunks with the last partial).  Past n = 240 the run is cut after 3 outer iterations: the scorer is specified for any state.
Folds are idx[f::3], so row 0 and the last row are held by some fold.

The estimators are held to the CPU oracle with the kernel's tie rule and summation order on the device's own Gram entries
(test_gpu_smo_batched.py's bar, rtol 1e-12 on the multipliers) and to the per-fold calls of the same commit where the fold's own
Gram build has the shared panel's bits (asserted at n = 240, one tile row).
"""
import ctypes as C
import math

import numpy as np
import pytest

import platt_reference as pr
import scoring_reference as sr
from test_gpu_svr_cv import _data

pytestmark = pytest.mark.gpu

GAMMA, TOL = 0.1, 1e-3
SIZES, COUNTS = (240, 1025, 2049), (1, 17, 36)
SVR_CS, SVR_EPS = (0.5, 2., 8., 1.), (0.05, 0.1, 0.2)
SVC_CS = (0.5, 4., 1., 2.)
BIG_EPS = 10.   # above the targets' range (|y| < 2): such a column's walker ends without a step


@pytest.fixture(scope='module')
def amd():
    import optiml_amd
    from optiml_amd import _lib
    from optiml_amd.device import get_context
    _lib.load()
    get_context()
    return optiml_amd


def _kernel():
    from optiml_amd.ml.svm.kernels import GaussianKernel
    return GaussianKernel(gamma=GAMMA)


def _folds(n):
    idx = np.arange(n)
    return [(np.setdiff1d(idx, idx[f::3]), idx[f::3]) for f in range(3)]


def _held(n):
    held = np.zeros((3, n), dtype=np.uint8)
    for f, (_, te) in enumerate(_folds(n)):
        held[f, te] = 1
    return held


def _svr_quad(X, y):
    """the panel as `MultiOutputSVR._fit_smo` and the search build it"""
    from optiml_amd.opti import KernelQuadratic
    return KernelQuadratic(X, np.hstack((-y, y)) + 0.1, 'svr', _kernel(), rank_one=False, compact=False)


def _svc_quad(X, yb):
    """the panel as `SVCGridSearchCV._fit_batched_smo` builds it"""
    from optiml_amd.opti import KernelQuadratic
    return KernelQuadratic(X, -np.ones(len(X)), 'svc', _kernel(), y=yb, rank_one=False, compact=False)


def svr_columns(n, k):
    """k regression columns on the folds of n rows: column j trains on fold j % 3's training rows and scores its test rows; C and
    epsilon walk their lists; with more than one column, column 4 has an epsilon above the targets' range and column 7 scores
    nothing.  Returns (C, epsilon, set_of, rows)."""
    folds = _folds(n)
    Cs = [SVR_CS[(j // 3) % 4] for j in range(k)]
    eps = [SVR_EPS[(j // 12) % 3] for j in range(k)]
    set_of = [j % 3 for j in range(k)]
    if k > 1:
        eps[4] = BIG_EPS
        set_of[7] = -1
    return Cs, eps, set_of, [folds[j % 3][0] for j in range(k)]


def svc_columns(codes, k):
    """k classification columns (3 classes) on the folds: column j is class (j // 3) % 3 against the rest on fold j % 3 with C
    SVC_CS[j // 9]; its calibrator is (C, class), fed by that pair's fold columns, whose test rows are disjoint; with more than
    one column, column 5 feeds no calibrator and column 7 scores nothing.  Returns (Y, C, set_of, cal_of, ncal, rows)."""
    folds = _folds(len(codes))
    Y = np.stack([np.where(codes == (j // 3) % 3, 1., -1.) for j in range(k)])
    Cs = [SVC_CS[(j // 9) % 4] for j in range(k)]
    set_of = [j % 3 for j in range(k)]
    cal_of = [3 * (j // 9) + (j // 3) % 3 for j in range(k)]
    ncal = max(cal_of) + 1
    if k > 1:
        cal_of[5] = -1
        set_of[7] = -1
    return Y, Cs, set_of, cal_of, ncal, [folds[j % 3][0] for j in range(k)]


@pytest.fixture(scope='module')
def data(amd):
    """Per size the regression input (test_gpu_svr_cv._data) and the classification input (make_multiclass_blobs, 3 classes);
    computed once and shared by the tests, which leave it unchanged."""
    from optiml_amd.datasets import make_multiclass_blobs
    out = {}
    for n in SIZES:
        X, y = _data(n)
        Xc, codes = make_multiclass_blobs(n, 5, 3, seed=3)
        out[n] = dict(X=X, y=y, Xc=Xc, codes=codes)
    assert all(np.abs(d['y']).max() < 2. for d in out.values())
    return out


def _svr_solver(dev, y, cols):
    from optiml_amd import _lib
    from optiml_amd.ml.svm._batched import _DeviceSMOSolver
    Cs, eps, _, rows = cols
    return _DeviceSMOSolver(dev, _lib.SVR, np.stack([y] * len(Cs)), Cs, eps, TOL, rows)


def _svc_solver(dev, cols):
    from optiml_amd import _lib
    from optiml_amd.ml.svm._batched import _DeviceSMOSolver
    Y, Cs, _, _, _, rows = cols
    return _DeviceSMOSolver(dev, _lib.SVC, Y, Cs, None, TOL, rows)


def _advance(solver, n):
    """to the end at n = 240, else 3 outer iterations: an unfinished state"""
    from optiml_amd.ml.svm._batched import run_batched_smo
    if n == 240:
        _, failed = run_batched_smo(solver)
    else:
        _, _, failed = solver.run(3)
    assert not failed.any()


def _svr_state(solver, dev):
    """(coef rows, u rows, scalars) of a regression solver's columns from its downloaded state and the same product"""
    from optiml_amd import _lib
    from optiml_amd.ml.svm._batched import _gram_matmat
    n = solver.n
    W, scal = np.zeros((solver.k, n)), []
    for c in range(solver.k):
        a = solver.get(c, _lib.SMO_ALPHAS)
        sv = (a[:n] > 1e-6) | (a[n:] > 1e-6)
        W[c][sv] = a[:n][sv] - a[n:][sv]
        scal.append(solver.get(c, _lib.SMO_SCALARS))
    return W, _gram_matmat(dev, W, wide=True), scal


def _svc_state(solver, dev, Y):
    from optiml_amd import _lib
    from optiml_amd.ml.svm._batched import _gram_matmat
    W, scal = np.zeros((solver.k, solver.n)), []
    for c in range(solver.k):
        a = solver.get(c, _lib.SMO_ALPHAS)
        sv = a > 1e-6
        W[c][sv] = a[sv] * Y[c][sv]
        scal.append(solver.get(c, _lib.SMO_SCALARS))
    return W, _gram_matmat(dev, W, wide=True), scal


def _check_svr(solver, dev, y, set_of, held, what):
    """the scorer's figures against the state it read; returns them"""
    b, n_sv, sse, n_held = solver.svr_heldout(set_of, held)
    W, U, scal = _svr_state(solver, dev)
    assert list(n_sv) == _n_sv_svr(solver), what
    for c in range(solver.k):
        assert b[c] == scal[c][5], (what, c)
        te = np.flatnonzero(held[set_of[c]]) if set_of[c] >= 0 else np.zeros(0, dtype=np.intp)
        assert n_held[c] == len(te), (what, c)
        ref = math.fsum(float(t) for t in (y[te] - (U[c][te] + b[c])) ** 2)
        assert np.isfinite(sse[c])
        sr.check_sse('%s column %d' % (what, c), float(sse[c]), ref, max(1, len(te)))
    return b, n_sv, sse, n_held


def _n_sv_svr(solver):
    from optiml_amd import _lib
    n = solver.n
    out = []
    for c in range(solver.k):
        a = solver.get(c, _lib.SMO_ALPHAS)
        out.append(int(((a[:n] > 1e-6) | (a[n:] > 1e-6)).sum()))
    return out


# ---- 1. the scorer against the state it read ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('k', COUNTS)
@pytest.mark.parametrize('n', SIZES)
def test_svr_scorer_against_the_state_it_read(amd, data, n, k):
    d = data[n]
    cols = svr_columns(n, k)
    held = _held(n)
    quad = _svr_quad(d['X'], d['y'])
    dev = quad.device_problem()
    solver = _svr_solver(dev, d['y'], cols)
    try:
        _advance(solver, n)
        b, n_sv, sse, n_held = _check_svr(solver, dev, d['y'], cols[2], held, 'n = %d, k = %d' % (n, k))
        assert list(n_sv) == _n_sv_svr(solver)
        if k > 1:
            # epsilon above the targets' range: no step, no support vector, a constant prediction
            assert n_sv[4] == 0 and np.isfinite(b[4]) and np.isfinite(sse[4]) and n_held[4] == len(_folds(n)[4 % 3][1])
            assert n_held[7] == 0 and sse[7] == 0. and n_sv[7] > 0
        assert (np.delete(n_sv, 4) > 0).all() if k > 1 else n_sv[0] > 0
    finally:
        solver.close()
        quad.release()


def _check_svc(solver, dev, cols, held, what):
    Y, _, set_of, cal_of, ncal, _ = cols
    from optiml_amd.ml.svm._batched import platt_fit
    n = solver.n
    b, n_sv, fit = solver.svc_heldout(set_of, held, cal_of, ncal, decisions=True)
    W, U, scal = _svc_state(solver, dev, Y)
    dec, lab = np.zeros((ncal, n)), np.zeros((ncal, n))
    for c in range(solver.k):
        assert n_sv[c] == np.count_nonzero(W[c]) and b[c] == scal[c][5], (what, c)
        if set_of[c] >= 0 and cal_of[c] >= 0:
            te = np.flatnonzero(held[set_of[c]])
            assert not lab[cal_of[c]][te].any()
            dec[cal_of[c]][te] = U[c][te] + b[c]
            lab[cal_of[c]][te] = Y[c][te]
    assert np.array_equal(fit['dec'], dec), what   # u + b on the scored rows, 0 elsewhere
    again = platt_fit(dec, lab)   # the same kernel on the same bits
    for key in again:
        assert np.array_equal(again[key], fit[key]), (what, key)
    compared = 0
    for cal in range(ncal):
        ref = pr.platt_reference(dec[cal], lab[cal])
        assert int(fit['n_pos'][cal]) == ref['n_pos'] and int(fit['n_neg'][cal]) == ref['n_neg'], (what, cal)
        if not (ref['stop_ratio'] < 1 / 1.1 and ref['search_margin'] > pr.SEARCH_MARGIN):
            continue   # the reference says its own iteration count hangs on a hair for this sample
        compared += 1
        assert int(fit['iters'][cal]) == ref['iters'] and int(fit['flags'][cal]) == ref['flags'], (what, cal)
        # (A, B) solves 2 x 2 Newton systems: its error is normwise, relative to the larger of the two — a B near 0 beside an A of
        # order 1 has no relative accuracy of its own
        scale = {'A': max(abs(ref['A']), abs(ref['B'])), 'B': max(abs(ref['A']), abs(ref['B'])), 'loss': abs(ref['loss'])}
        for key in ('A', 'B', 'loss'):
            got, want = float(fit[key][cal]), ref[key]
            assert got == want or abs(got - want) <= pr.PLATT_RTOL * scale[key], (what, cal, key, got, want)
    print('%s: %d of %d calibrators compared with platt_reference' % (what, compared, ncal))
    return b, n_sv, fit


@pytest.mark.parametrize('k', COUNTS)
@pytest.mark.parametrize('n', SIZES)
def test_svc_scorer_against_the_state_it_read(amd, data, n, k):
    d = data[n]
    cols = svc_columns(d['codes'], k)
    held = _held(n)
    quad = _svc_quad(d['Xc'], cols[0][0])
    dev = quad.device_problem()
    solver = _svc_solver(dev, cols)
    try:
        _advance(solver, n)
        b, n_sv, fit = _check_svc(solver, dev, cols, held, 'n = %d, k = %d' % (n, k))
        assert (n_sv > 0).all() and np.isfinite(b).all()
        if k == 36:   # calibrators 0 and 2 .. 11 are fed by three folds: every row once; calibrator 1 misses column 5's fold
            full = fit['n_pos'] + fit['n_neg']
            assert (np.delete(full, [1, 2]) == n).all() and full[1] == n - len(_folds(n)[2][1]) and full[2] == n - len(_folds(n)[1][1])
    finally:
        solver.close()
        quad.release()


# ---- 2. column independence ---------------------------------------------------------------------------------------------------------
def test_a_column_has_the_same_bits_alone_first_last_and_cut(amd, data):
    """SVR column 5 and SVC column 4 of the 17-column sets at n = 1025 after 3 outer iterations: alone, first, last, and in a
    solve of the first 9 columns only (what a column cap leaves)"""
    n = 1025
    d = data[n]
    held = _held(n)

    def pick(cols, order):
        return tuple([v[j] for j in order] if isinstance(v, list) else (v[order] if isinstance(v, np.ndarray) else v) for v in cols)

    quad = _svr_quad(d['X'], d['y'])
    dev = quad.device_problem()
    base_cols = svr_columns(n, 17)
    got = {}
    for name, order in (('base', list(range(17))), ('alone', [5]), ('first', [5] + [j for j in range(17) if j != 5]),
                        ('last', [j for j in range(17) if j != 5] + [5]), ('cut', list(range(9)))):
        solver = _svr_solver(dev, d['y'], pick(base_cols, order))
        try:
            _advance(solver, n)
            res = solver.svr_heldout([base_cols[2][j] for j in order], held)
            got[name] = [v[order.index(5)] for v in res]
        finally:
            solver.close()
    quad.release()
    for name in ('alone', 'first', 'last', 'cut'):
        assert all(np.array_equal(a, b) for a, b in zip(got[name], got['base'])), name

    cols = svc_columns(d['codes'], 17)
    quad = _svc_quad(d['Xc'], cols[0][0])
    dev = quad.device_problem()
    got = {}
    for name, order in (('base', list(range(17))), ('alone', [4]), ('first', [4] + [j for j in range(17) if j != 4]),
                        ('last', [j for j in range(17) if j != 4] + [4]), ('cut', list(range(9)))):
        Y, Cs, set_of, cal_of, ncal, rows = cols
        # a calibrator of its own for column 4, so that its row of the decision buffer is the column's alone
        mine = [(-1 if j != 4 else 0) for j in order]
        sub = (Y[order], [Cs[j] for j in order], [set_of[j] for j in order], mine, 1, [rows[j] for j in order])
        solver = _svc_solver(dev, sub)
        try:
            _advance(solver, n)
            b, n_sv, fit = solver.svc_heldout(sub[2], held, mine, 1, decisions=True)
            at = order.index(4)
            got[name] = [b[at], n_sv[at]] + [fit[key] for key in sorted(fit)]
        finally:
            solver.close()
    quad.release()
    for name in ('alone', 'first', 'last', 'cut'):
        assert all(np.array_equal(a, b) for a, b in zip(got[name], got['base'])), name


# ---- 3. the state is untouched --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('task', ['svr', 'svc'])
def test_scoring_leaves_the_state_and_the_run_untouched(amd, data, task):
    from optiml_amd import _lib
    from optiml_amd.ml.svm._batched import run_batched_smo
    n = 240
    d = data[n]
    held = _held(n)
    if task == 'svr':
        cols = svr_columns(n, 17)
        quad = _svr_quad(d['X'], d['y'])
        make = lambda: _svr_solver(quad.device_problem(), d['y'], cols)   # noqa: E731
    else:
        cols = svc_columns(d['codes'], 17)
        quad = _svc_quad(d['Xc'], cols[0][0])
        make = lambda: _svc_solver(quad.device_problem(), cols)   # noqa: E731
    scored, plain = make(), make()
    try:
        for s in (scored, plain):
            _, _, failed = s.run(3)
            assert not failed.any()
        if task == 'svr':
            scored.svr_heldout(cols[2], held)
        else:
            scored.svc_heldout(cols[2], held, cols[3], cols[4], decisions=True)
        for c in range(scored.k):   # the call itself changed nothing
            for what in (_lib.SMO_ALPHAS, _lib.SMO_ERRORS, _lib.SMO_SCALARS):
                assert np.array_equal(scored.get(c, what), plain.get(c, what)), (c, what)
        outer_a, failed_a = run_batched_smo(scored)
        outer_b, failed_b = run_batched_smo(plain)
        assert np.array_equal(outer_a, outer_b) and (outer_a > 3).any() and not failed_a.any() and not failed_b.any()
        for c in range(scored.k):
            for what in (_lib.SMO_ALPHAS, _lib.SMO_ERRORS, _lib.SMO_SCALARS):
                assert np.array_equal(scored.get(c, what), plain.get(c, what)), (c, what)
    finally:
        scored.close()
        plain.close()
        quad.release()


# ---- 4. refusals ----------------------------------------------------------------------------------------------------------------------
def test_scorers_refuse_bad_arguments_and_the_solver_stays_usable(amd, data):
    from optiml_amd import _lib
    from optiml_amd.ml.svm._batched import _DeviceSMOSolver, run_batched_smo
    n, k = 240, 6
    d = data[n]
    held = _held(n)
    lib = _lib.load()
    u8, i64 = C.POINTER(C.c_ubyte), C.POINTER(C.c_int64)
    folds = _folds(n)
    rows = [folds[j % 3][0] for j in range(k)]
    set_of = np.array([j % 3 for j in range(k)], dtype=np.int32)
    cal_of = np.array([j // 3 for j in range(k)], dtype=np.int32)   # two calibrators, three disjoint folds each
    Ycls = np.stack([np.where(d['codes'] == j // 3, 1., -1.) for j in range(k)])

    def svr_rc(solver, null=(), nsets=3, set_of=set_of, held=held):
        b, sse = np.empty(k), np.empty(k)
        n_sv, n_held = np.empty(k, dtype=np.int64), np.empty(k, dtype=np.int64)
        args = dict(set_of=_lib.iptr(np.ascontiguousarray(set_of, dtype=np.int32)), held=held.ctypes.data_as(u8), b=_lib.ptr(b),
                    n_sv=n_sv.ctypes.data_as(i64), sse=_lib.ptr(sse), n_held=n_held.ctypes.data_as(i64))
        for name in null:
            args[name] = None
        return lib.bq_msmo_svr_heldout(solver._h if solver is not None else None, nsets, args['set_of'], args['held'], args['b'],
                                       args['n_sv'], args['sse'], args['n_held'])

    def svc_rc(solver, null=(), nsets=3, set_of=set_of, held=held, ncal=2, cal_of=cal_of):
        b, n_sv = np.empty(k), np.empty(k, dtype=np.int64)
        m = max(1, ncal)
        v = [np.empty(m) for _ in range(3)]
        cnt = [np.empty(m, dtype=np.int64) for _ in range(2)]
        ints = [np.empty(m, dtype=np.int32) for _ in range(2)]
        args = dict(set_of=_lib.iptr(np.ascontiguousarray(set_of, dtype=np.int32)), held=held.ctypes.data_as(u8),
                    cal_of=_lib.iptr(np.ascontiguousarray(cal_of, dtype=np.int32)), b=_lib.ptr(b), n_sv=n_sv.ctypes.data_as(i64),
                    A=_lib.ptr(v[0]), B=_lib.ptr(v[1]), iters=_lib.iptr(ints[0]), loss=_lib.ptr(v[2]), n_pos=cnt[0].ctypes.data_as(i64),
                    n_neg=cnt[1].ctypes.data_as(i64), flags=_lib.iptr(ints[1]))
        for name in null:
            args[name] = None
        return lib.bq_msmo_svc_heldout(solver._h if solver is not None else None, nsets, args['set_of'], args['held'], ncal,
                                       args['cal_of'], args['b'], args['n_sv'], args['A'], args['B'], args['iters'], args['loss'],
                                       args['n_pos'], args['n_neg'], args['flags'], None)

    own = held.copy()
    own[1, int(rows[1][0])] = 1   # a training row of column 1 (fold 1) said to be scored by set 1
    shared = np.zeros(k, dtype=np.int32)   # every column on calibrator 0: columns 0 and 3 both score fold 0's rows
    quad_r = _svr_quad(d['X'], d['y'])
    quad_c = _svc_quad(d['Xc'], Ycls[0])
    dev_r, dev_c = quad_r.device_problem(), quad_c.device_problem()
    svr = _DeviceSMOSolver(dev_r, _lib.SVR, np.stack([d['y']] * k), 1., 0.1, TOL, rows)
    svr_all = _DeviceSMOSolver(dev_r, _lib.SVR, np.stack([d['y']] * k), 1., 0.1, TOL)
    svc = _DeviceSMOSolver(dev_c, _lib.SVC, Ycls, 1., None, TOL, rows)
    svc_all = _DeviceSMOSolver(dev_c, _lib.SVC, Ycls, 1., None, TOL)
    try:
        for rc, mine, other, no_list, names in (
                (svr_rc, svr, svc, svr_all, ('set_of', 'held', 'b', 'n_sv', 'sse', 'n_held')),
                (svc_rc, svc, svr, svc_all, ('set_of', 'held', 'cal_of', 'b', 'n_sv', 'A', 'B', 'iters', 'loss', 'n_pos', 'n_neg',
                                             'flags'))):
            assert rc(None) == _lib.ERR_BADARG
            for name in names:
                assert rc(mine, null=(name,)) == _lib.ERR_BADARG, name
            assert rc(other) == _lib.ERR_BADARG                     # a solver of the other task
            assert rc(mine, nsets=0) == _lib.ERR_BADARG
            for at, value in ((2, 3), (2, -2)):                     # an entry out of range
                bad = set_of.copy()
                bad[at] = value
                assert rc(mine, set_of=bad) == _lib.ERR_BADARG, value
            assert rc(mine, held=own) == _lib.ERR_BADARG            # a scored row in the column's own list
            assert rc(no_list) == _lib.ERR_BADARG                   # a scoring column that trains on every row
            assert b'bad argument' in lib.bq_last_error()
            assert rc(no_list, set_of=np.full(k, -1, dtype=np.int32)) == _lib.OK   # ... unless it scores nothing
        for ncal, cals in ((0, cal_of), (2, np.array([0, 0, 0, 1, 1, 2])), (2, np.array([0, 0, 0, 1, 1, -2]))):
            assert svc_rc(svc, ncal=ncal, cal_of=cals) == _lib.ERR_BADARG, (ncal, cals)
        assert svc_rc(svc, ncal=1, cal_of=shared) == _lib.ERR_BADARG and b'disjoint' in lib.bq_last_error()
        # nothing above touched the solvers: they score the fresh state, run to their end and score again
        assert svr_rc(svr) == _lib.OK and svc_rc(svc) == _lib.OK
        for s in (svr, svc):
            _, failed = run_batched_smo(s)
            assert not failed.any()
        _check_svr(svr, dev_r, d['y'], list(set_of), held, 'after the refusals')
        _check_svc(svc, dev_c, (Ycls, None, list(set_of), list(cal_of), 2, rows), held, 'after the refusals')
    finally:
        for s in (svr, svr_all, svc, svc_all):
            s.close()
        quad_r.release()
        quad_c.release()


# ---- 5. the search against the oracle -------------------------------------------------------------------------------------------------
GRID = {'C': [0.5, 4.], 'epsilon': [0.05, 0.2]}


def _svr(**over):
    from optiml_amd.ml.svm import SVR
    from optiml_amd.ml.svm.losses import epsilon_insensitive
    return SVR(**dict(dict(loss=epsilon_insensitive, kernel=_kernel(), C=1., epsilon=0.1, dual=True, optimizer='smo', tol=TOL,
                           reg_intercept=False), **over))


def _search(d, force, refit=False):
    from optiml_amd.ml.svm import SVRGridSearchCV
    search = SVRGridSearchCV(_svr(), GRID, cv=_folds(240), refit=refit)
    search.batch_smo = force
    return search.fit(d['X'], d['y'])


@pytest.fixture(scope='module')
def svr_oracle(amd, data):
    """the device's Gram matrix of the shared panel at n = 240 and, per (candidate, fold), the oracle's fit on the fold's training
    rows of it; computed once"""
    from oracle import smo_oracle as smo
    from optiml_amd.ml.svm.model_selection import parameter_grid
    d = data[240]
    quad = _svr_quad(d['X'], d['y'])
    K = quad.gram()
    quad.release()
    cands = parameter_grid(GRID)
    fits = {(ci, f): smo.smo_svr(K[tr][:, tr], d['y'][tr], C=p['C'], epsilon=p['epsilon'], tol=TOL, tie='index', dot='tree')
            for ci, p in enumerate(cands) for f, (tr, _) in enumerate(_folds(240))}
    return dict(K=K, cands=cands, fits=fits)


def test_search_scores_are_the_oracle_s_fold_fits(amd, data, svr_oracle, monkeypatch):
    from optiml_amd import _lib
    from optiml_amd.ml.svm import model_selection as ms
    from optiml_amd.ml.svm._batched import _gram_matmat, solve_batched_smo
    d = data[240]
    X, y = d['X'], d['y']
    folds = _folds(240)
    cands, fits = svr_oracle['cands'], svr_oracle['fits']
    assert cands == [{'C': 0.5, 'epsilon': 0.05}, {'C': 0.5, 'epsilon': 0.2}, {'C': 4., 'epsilon': 0.05}, {'C': 4., 'epsilon': 0.2}]
    # the columns' multipliers are the oracle's
    quad = _svr_quad(X, y)
    dev = quad.device_problem()
    assert np.array_equal(quad.gram(), svr_oracle['K'])
    order = [(ci, f) for ci in range(4) for f in range(3)]
    res = solve_batched_smo(dev, _lib.SVR, np.stack([y] * 12), [cands[ci]['C'] for ci, _ in order],
                            [cands[ci]['epsilon'] for ci, _ in order], TOL, rows=[folds[f][0] for _, f in order])
    W = np.zeros((12, 240))
    for j, (ci, f) in enumerate(order):
        tr, te = folds[f]
        ref, r = fits[ci, f], res[j]
        assert r['iter'] == ref['iter'] and r['steps'] == ref['steps'], (ci, f)
        np.testing.assert_allclose(r['alphas_p'][tr], ref['alphas_p'], rtol=1e-12, atol=1e-15)
        np.testing.assert_allclose(r['alphas_n'][tr], ref['alphas_n'], rtol=1e-12, atol=1e-15)
        np.testing.assert_allclose([r['b'], r['b_up'], r['b_low']], [ref['b'], ref['b_up'], ref['b_low']], rtol=1e-12, atol=1e-15)
        assert not r['alphas_p'][te].any() and not r['alphas_n'][te].any()
        sv = (ref['alphas_p'] > 1e-6) | (ref['alphas_n'] > 1e-6)
        W[j][tr[sv]] = ref['alphas_p'][sv] - ref['alphas_n'][sv]
    U = _gram_matmat(dev, W, wide=True)   # the oracle's coefficients through the same product
    quad.release()
    search = _search(d, True)
    assert search.smo_ is True and search.batched_ is True
    assert search.n_iter_.shape == (4, 3) and (search.status_ == '').all()
    want = np.empty((4, 3))
    for j, (ci, f) in enumerate(order):
        te = folds[f][1]
        sse_ref = math.fsum(float(t) for t in (y[te] - (U[j][te] + fits[ci, f]['b'])) ** 2)
        want[ci, f] = ms.r2_from_sse(sse_ref, y[te])
        got = search.cv_results_['split%d_test_score' % f][ci]
        den = float(((y[te] - np.average(y[te])) ** 2).sum())
        # the squared error at its bound, over the denominator of R^2; the division and the subtraction from 1 round once each
        bound = sr.sse_bound(sse_ref, len(te)) / den + 2 * np.finfo(float).eps * max(1., sse_ref / den)
        print('candidate %d fold %d: R^2 %.17g, oracle %.17g, |diff| %.3e (bound %.3e)' % (ci, f, got, want[ci, f],
                                                                                       abs(got - want[ci, f]), bound))
        assert abs(got - want[ci, f]) <= bound, (ci, f)
        assert search.n_iter_[ci, f] == fits[ci, f]['iter']
    best = int(np.argmax(want.mean(axis=1)))
    assert search.best_index_ == best and search.best_params_ == cands[best]
    # more columns than one solve takes: the same bits
    monkeypatch.setattr(ms, 'smo_heldout_column_cap', lambda *args, **kw: 5)
    split = _search(d, True)
    assert split.smo_ is True and split.batched_ is True
    for f in range(3):
        assert np.array_equal(split.cv_results_['split%d_test_score' % f], search.cv_results_['split%d_test_score' % f])
    assert np.array_equal(split.n_iter_, search.n_iter_)


# ---- 6. the search against the per-fold calls -----------------------------------------------------------------------------------------
def _fold_gram_equal(X, quad_of, K, folds):
    """whether every fold's own Gram build has the bits of the shared panel's entries; prints the finding"""
    same = True
    for f, (tr, _) in enumerate(folds):
        quad = quad_of(tr)
        own = quad.gram()
        quad.release()
        diff = np.abs(own - K[tr][:, tr])
        print('fold %d, %d rows: entries of the fold\'s own Gram build that differ from the shared panel\'s: %d of %d, largest '
              'difference %.3e' % (f, len(tr), int((diff > 0).sum()), diff.size, diff.max()))
        same &= not diff.any()
    return same


def test_search_against_the_per_fold_calls(amd, data, svr_oracle):
    d = data[240]
    X, y = d['X'], d['y']
    folds = _folds(240)
    assert _fold_gram_equal(X, lambda tr: _svr_quad(X[tr], y[tr]), svr_oracle['K'], folds)   # one tile row: the same bits
    loop, search = _search(d, False), _search(d, True)
    assert loop.smo_ is False and loop.batched_ is False and search.smo_ is True and search.batched_ is True
    for f in range(3):
        np.testing.assert_allclose(search.cv_results_['split%d_test_score' % f], loop.cv_results_['split%d_test_score' % f],
                                   rtol=1e-9, atol=1e-9)
    assert search.best_index_ == loop.best_index_ and search.best_params_ == loop.best_params_
    assert np.array_equal(search.n_iter_, loop.n_iter_) and np.array_equal(search.status_, loop.status_)
    # 12 columns: the default dispatch takes the batched path too, with the same bits
    auto = _search(d, None, refit=True)
    assert auto.smo_ is True and auto.batched_ is True
    assert np.array_equal(auto.cv_results_['mean_test_score'], search.cv_results_['mean_test_score'])
    assert auto.best_estimator_.C == auto.best_params_['C'] and auto.best_estimator_.epsilon == auto.best_params_['epsilon']


# ---- 7. calibration -------------------------------------------------------------------------------------------------------------------
CAL_C = 2.


def _svc_kw():
    from optiml_amd.ml.svm.losses import hinge
    return dict(loss=hinge, kernel=_kernel(), C=CAL_C, dual=True, optimizer='smo', tol=TOL, reg_intercept=False)


def _labels(d, classes):
    """3 classes: the codes; 2: class 2 against the rest, on the same rows"""
    return d['codes'] if classes == 3 else (d['codes'] == 2).astype(int)


def _calibrated(d, classes, ensemble, force):
    from optiml_amd.ml.svm import SVC, CalibratedSVC, OneVsRestSVC
    est = CalibratedSVC((SVC if classes == 2 else OneVsRestSVC)(**_svc_kw()), cv=_folds(240), ensemble=ensemble)
    est.batch_smo = force
    return est.fit(d['Xc'], _labels(d, classes))


@pytest.fixture(scope='module')
def svc_oracle(amd, data):
    """the device's Gram matrix of the shared classification panel at n = 240 and, per class column (one-vs-rest of the 3 codes;
    class 2 is also the binary problem's positive class) and fold, the oracle's fit on the fold's training rows and its decision
    values on the held-out rows; computed once"""
    from oracle import smo_oracle as smo
    d = data[240]
    quad = _svc_quad(d['Xc'], np.where(d['codes'] == 0, 1., -1.))
    K = quad.gram()
    quad.release()
    dec, fits = np.zeros((3, 240)), {}
    for r in range(3):
        yb = np.where(d['codes'] == r, 1., -1.)
        for f, (tr, te) in enumerate(_folds(240)):
            ref = smo.smo_svc(K[tr][:, tr], yb[tr], C=CAL_C, tol=TOL, tie='index', dot='tree')
            sv = ref['alphas'] > 1e-6
            dec[r][te] = K[te][:, tr[sv]] @ (ref['alphas'][sv] * yb[tr][sv]) + ref['b']
            fits[r, f] = ref
    return dict(K=K, dec=dec, fits=fits)


@pytest.mark.parametrize('ensemble', [True, False])
@pytest.mark.parametrize('classes', [2, 3])
def test_calibrated_svc_over_smo(amd, data, svc_oracle, classes, ensemble):
    """The fold columns are the oracle's fits (multipliers at rtol 1e-12, test_gpu_smo_batched.py's bar); the held-out decision
    values against the oracle-derived ones at DECISION_RTOL of the largest; the sigmoids against `platt_reference` on the
    oracle-derived values and the probabilities against the per-fold calls of the same commit (`batch_smo=False`) at PLATT_RTOL +
    DECISION_RTOL, test_gpu_calibration.py's bound between two ways to the same decision values — A and B relative to the larger of
    the two.  The fold fits of the two paths are the same walks where a fold's own Gram build has the shared panel's bits, which
    is asserted first (n = 240: one tile row), so their multipliers are compared with ==."""
    d = data[240]
    X, y = d['Xc'], _labels(d, classes)
    folds = _folds(240)
    rows = [2] if classes == 2 else [0, 1, 2]   # the oracle's class columns behind the estimator's
    kc = len(rows)
    assert _fold_gram_equal(X, lambda tr: _svc_quad(X[tr], np.where(d['codes'][tr] == 0, 1., -1.)), svc_oracle['K'], folds)
    est, loop = _calibrated(d, classes, ensemble, True), _calibrated(d, classes, ensemble, False)
    assert est.smo_ is True and est.batched_ is True and loop.smo_ is False and loop.batched_ is False
    assert np.array_equal(est.classes_, loop.classes_)
    want = svc_oracle['dec'][rows]
    Ycls = np.stack([np.where(d['codes'] == r, 1., -1.) for r in rows])
    if ensemble:
        assert len(est.calibrated_classifiers_) == 3 and not hasattr(est, 'oof_decision_')
        got = np.zeros((kc, 240))
        for f, (tr, te) in enumerate(folds):
            mine, theirs = est.calibrated_classifiers_[f].estimator, loop.calibrated_classifiers_[f].estimator
            got[:, te] = np.asarray(mine.decision_function(X[te]), dtype=float).reshape(len(te), kc).T
            for j, (a, b) in enumerate(zip(mine.estimators_ if classes == 3 else [mine], theirs.estimators_ if classes == 3 else [theirs])):
                ref = svc_oracle['fits'][rows[j], f]
                np.testing.assert_allclose(a.alphas_, ref['alphas'], rtol=1e-12, atol=1e-15)
                np.testing.assert_allclose(a.intercept_, ref['b'], rtol=1e-12, atol=1e-15)
                assert a.optimizer.iter == ref['iter'] and a.optimizer.steps == ref['steps']
                assert np.array_equal(a.alphas_, b.alphas_) and a.intercept_ == b.intercept_, (f, j)
                assert np.array_equal(a.support_, b.support_) and np.array_equal(a.dual_coef_, b.dual_coef_), (f, j)
        cals = [pr.platt_reference(want[j][te], Ycls[j][te]) for _, te in folds for j in range(kc)]
        shape = (3, kc)
    else:
        assert len(est.calibrated_classifiers_) == 1
        assert est.oof_decision_.shape == ((240,) if kc == 1 else (240, kc)) and np.all(est.oof_decision_ != 0)   # every row once
        got = est.oof_decision_.reshape(240, kc).T
        cals = [pr.platt_reference(want[j], Ycls[j]) for j in range(kc)]
        shape = (kc,)
        mine, theirs = est.calibrated_classifiers_[0].estimator, loop.calibrated_classifiers_[0].estimator
        for a, b in zip(mine.estimators_ if classes == 3 else [mine], theirs.estimators_ if classes == 3 else [theirs]):
            assert np.array_equal(a.alphas_, b.alphas_) and a.intercept_ == b.intercept_
    dev = np.abs(got - want).max() / np.abs(want).max()
    print('classes %d, ensemble %s: held-out decision deviation from the oracle-derived values %.3e (bound %.3e)'
          % (classes, ensemble, dev, pr.DECISION_RTOL))
    assert dev <= pr.DECISION_RTOL
    rtol = pr.PLATT_RTOL + pr.DECISION_RTOL
    assert est.calibrators_['A'].shape == shape
    for i, c in enumerate(cals):
        # the precondition of equal iteration counts, as test_gpu_calibration.py states it for decision values that differ by
        # DECISION_RTOL: no stop test decided by less than 1 %, no line-search test by a hair
        assert c['flags'] == 0 and c['stop_ratio'] < 1 / 1.01 and c['search_margin'] > pr.SEARCH_MARGIN, (i, c)
        A, B = est.calibrators_['A'].reshape(-1)[i], est.calibrators_['B'].reshape(-1)[i]
        scale = max(abs(c['A']), abs(c['B']))
        print('calibrator %d: A %.17g / %.17g, B %.17g / %.17g, iters %d / %d, cond %.3g' % (
            i, A, c['A'], B, c['B'], est.calibrators_['iters'].reshape(-1)[i], c['iters'], c['cond']))
        assert est.calibrators_['iters'].reshape(-1)[i] == c['iters'] and est.calibrators_['flags'].reshape(-1)[i] == 0
        assert abs(A - c['A']) <= rtol * scale and abs(B - c['B']) <= rtol * scale, i
    Xnew = X[::5] + 0.01
    P, Q = est.predict_proba(Xnew), loop.predict_proba(Xnew)
    print('largest relative probability deviation between the paths: %.3e (bound %.3e)' % (np.abs(P / Q - 1).max(), rtol))
    np.testing.assert_allclose(P, Q, rtol=rtol, atol=0)
    np.testing.assert_allclose(P.sum(axis=1), 1., rtol=1e-14)
    assert P.shape == (len(Xnew), classes) and np.array_equal(est.predict(Xnew), loop.predict(Xnew))


def test_calibration_default_dispatch_and_split_solves(amd, data, monkeypatch):
    """3 folds x 3 classes: nine columns take the batched SMO path by default, the binary estimator's three do not; folds spread
    over several solves (a tiny column cap) give the same sigmoids as one solve, bit for bit with ensemble (a calibrator is one
    column's) and through `platt_fit` on the gathered rows without"""
    from optiml_amd.ml.svm import calibration
    d = data[240]
    assert _calibrated(d, 3, True, None).smo_ is True and _calibrated(d, 2, True, None).smo_ is False
    for ensemble in (True, False):
        one = _calibrated(d, 3, ensemble, True)
        monkeypatch.setattr(calibration, 'smo_heldout_column_cap', lambda *args, **kw: 4)
        cut = _calibrated(d, 3, ensemble, True)
        monkeypatch.undo()
        assert cut.smo_ is True
        for key in ('A', 'B', 'iters', 'loss', 'flags'):
            assert np.array_equal(cut.calibrators_[key], one.calibrators_[key]), (ensemble, key)
        if not ensemble:
            assert np.array_equal(cut.oof_decision_, one.oof_decision_)


def test_a_failed_calibration_solve_releases_the_panel(amd, data, monkeypatch):
    from optiml_amd import _lib
    from optiml_amd.ml.svm import _batched, calibration
    from optiml_amd.opti import KernelQuadratic
    released, closed = [], []
    release, close = KernelQuadratic.release, _batched._DeviceSMOSolver.close

    def failing(solver, chunk=64):
        outer, _, failed = solver.run(1)
        failed[-1] = True
        return outer, failed

    monkeypatch.setattr(KernelQuadratic, 'release', lambda self: (released.append(self), release(self))[1])
    monkeypatch.setattr(_batched._DeviceSMOSolver, 'close', lambda self: (closed.append(self), close(self))[1])
    monkeypatch.setattr(calibration, 'run_batched_smo', failing)
    with pytest.raises(_lib.BcqpError) as e:
        _calibrated(data[240], 3, True, True)
    assert e.value.code == _lib.ERR_NONFINITE and len(released) == 1 and len(closed) >= 1


# ---- 8. a failing solve releases the panel --------------------------------------------------------------------------------------------
def test_a_failed_solve_releases_the_panel_and_closes_the_solver(amd, data, monkeypatch):
    from optiml_amd import _lib
    from optiml_amd.ml.svm import _batched, model_selection as ms
    from optiml_amd.opti import KernelQuadratic
    d = data[240]
    released, closed = [], []
    release, close = KernelQuadratic.release, _batched._DeviceSMOSolver.close

    def spy_release(self):
        released.append(self)
        return release(self)

    def spy_close(self):
        closed.append(self)
        return close(self)

    def failing(solver, chunk=64):
        outer, _, failed = solver.run(1)
        failed[0] = True
        return outer, failed

    monkeypatch.setattr(KernelQuadratic, 'release', spy_release)
    monkeypatch.setattr(_batched._DeviceSMOSolver, 'close', spy_close)
    monkeypatch.setattr(ms, 'run_batched_smo', failing)
    with pytest.raises(_lib.BcqpError) as e:
        _search(d, True)
    assert e.value.code == _lib.ERR_NONFINITE and 'unexpected status' in str(e.value)
    assert len(released) == 1 and len(closed) >= 1
