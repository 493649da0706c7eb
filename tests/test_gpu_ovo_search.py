"""OneVsOneGridSearchCV on the device: the vote kernel (bq_ovo_vote) against ovo_decision and argmax bit for bit; the held-out vote of
the pair solver's columns (bq_msolver_pairs_vote_heldout: mcoef_kernel, the 16-column product, the intercepts, mvote_kernel,
mvote_count_kernel) against the host on the same state, its batch invariance and its refusals; the search against sklearn's
GridSearchCV over the project's own OneVsOneSVC, with failed fits and on the per-fold path."""
import ctypes as C
import functools
import warnings

import numpy as np
import pytest

import test_gpu_ovo as tgo
from test_gpu_svr_cv import _compare_results

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def amd():
    from optiml_amd import _lib
    from optiml_amd.device import get_context
    _lib.load()
    get_context()


# ---- 1. the vote kernel against NumPy -----------------------------------------------------------------------------------------------
def _vote_input(family, ncls, t):
    P = ncls * (ncls - 1) // 2
    rs = np.random.RandomState(1000 * ncls + t)
    if family == 'normal':
        return rs.standard_normal((t, P))
    if family == 'zeros':
        return np.zeros((t, P))
    if family == 'halves':   # every sum is exact, and many rows tie
        return rs.randint(-3, 4, size=(t, P)) * 0.5
    if family == 'negzero':
        return np.where(rs.rand(t, P) < 0.5, -0.0, rs.randint(-1, 2, size=(t, P)) * 0.5)
    D = rs.standard_normal((t, P))   # 'special': every row holds an infinity or a NaN, every third row two of them
    special = np.array([np.inf, -np.inf, np.nan])
    D[np.arange(t), rs.randint(0, P, size=t)] = special[np.arange(t) % 3]
    D[::3, rs.randint(0, P)] = special[(np.arange(t)[::3] // 3 + 1) % 3]
    return D


@pytest.mark.parametrize('family', ['normal', 'zeros', 'halves', 'negzero', 'special'])
@pytest.mark.parametrize('t', [1, 63, 64, 65, 257])
@pytest.mark.parametrize('ncls', [2, 3, 7, 64])
def test_vote_kernel_equals_ovo_decision_and_argmax(amd, ncls, t, family):
    """pred is ovo_decision(...).argmax(1) and Y is ovo_decision's, bit for bit (NaNs in the same places): the order of operations is
    the host's"""
    from optiml_amd.ml.svm.onevsone import ovo_decision
    from optiml_amd.ml.svm.ovo_search import ovo_vote
    D = _vote_input(family, ncls, t)
    with np.errstate(invalid='ignore'):
        want = ovo_decision((D > 0).astype(int), D, ncls)
    pred, Y = ovo_vote(D, ncls, details=True)
    assert np.array_equal(Y, want, equal_nan=True)
    assert np.array_equal(pred, want.argmax(axis=1))
    assert np.array_equal(ovo_vote(D, ncls), pred)
    if family == 'special':
        assert np.isnan(want).any(axis=1).all()
    if ncls == 2:   # OneVsOneSVC.predict with two classes
        assert np.array_equal(pred, (want[:, 1] > 0).astype(int))


def test_vote_kernel_refusals(amd):
    from optiml_amd import _lib
    from optiml_amd.device import get_context
    lib, ctx = _lib.load(), get_context().handle
    D, pred = np.zeros(2016 + 64), np.zeros(4, dtype=np.int32)
    for ncls, t in ((1, 1), (65, 1), (3, 0), (0, 1), (3, -1)):
        assert lib.bq_ovo_vote(ctx, ncls, t, _lib.ptr(D), _lib.iptr(pred), None) == _lib.ERR_BADARG
    assert lib.bq_ovo_vote(None, 3, 1, _lib.ptr(D), _lib.iptr(pred), None) == _lib.ERR_BADARG
    assert lib.bq_ovo_vote(ctx, 3, 1, None, _lib.iptr(pred), None) == _lib.ERR_BADARG
    assert lib.bq_ovo_vote(ctx, 3, 1, _lib.ptr(D), None, None) == _lib.ERR_BADARG
    assert lib.bq_ovo_vote(ctx, 3, 1, _lib.ptr(D), _lib.iptr(pred), None) == _lib.OK and pred[0] == 0


# ---- 2. the held-out vote against the host on the same state ------------------------------------------------------------------------
class _Layout:
    """A class-sorted blob panel (test_gpu_ovo._blob_panel) and the columns of `fits`, a list of (fold, C): the fold's held-out rows
    are the data rows r with r % 3 == fold; group-major columns, the pairs in ovo_pairs order"""

    def __init__(self, sizes, fits):
        from optiml_amd.ml.svm.onevsone import ovo_pairs
        self.X, self.y, self.Xp, self.ct, self.pcode, ghost, self.index = tgo._blob_panel(sizes)
        self.ncls, self.n_pad = len(sizes), len(self.pcode)
        self.data_row = (~ghost).astype(np.uint8)
        self.pairs = ovo_pairs(self.ncls)
        self.P = len(self.pairs)
        self.fits = list(fits)
        rows = np.arange(len(self.y))
        self.held = np.zeros((len(self.fits), self.n_pad), dtype=np.uint8)
        Y, UB = [], []
        for g, (fold, Cv) in enumerate(self.fits):
            self.held[g, self.index[rows % 3 == fold]] = 1
            train = (self.data_row > 0) & (self.held[g] == 0)
            for i, j in self.pairs:
                Y.append(np.where(self.pcode == j, 1., -1.))
                UB.append(np.where(((self.pcode == i) | (self.pcode == j)) & train, Cv, 0.))
        self.Y, self.UB = np.stack(Y), np.stack(UB)

    def columns(self, groups):
        return np.concatenate([np.arange(g * self.P, (g + 1) * self.P) for g in groups])

    def solver(self, dev, groups, max_iter, kind=None):
        from optiml_amd import _lib
        from optiml_amd.ml.svm.onevsone import _DevicePairSolver
        cols = self.columns(groups)
        return _DevicePairSolver(dev, _lib.PG if kind is None else kind, self.ct, self.pairs * len(groups), self.Y[cols],
                                 self.UB[cols], 1e-6, max_iter)

    def score(self, solver, groups):
        return solver.vote_heldout_pairs(self.data_row, np.repeat(np.arange(len(groups)), self.P), self.held[list(groups)],
                                         predictions=True)


def _finish(solver):
    rows = [[] for _ in range(solver.k)]
    status = ['unknown']
    while 'unknown' in status:
        recs, status = solver.run(256)
        for c in range(solver.k):
            rows[c].append(recs[c])
    return [np.concatenate(r) for r in rows]


def _scored(lay, dev, groups, max_iter=60):
    """the groups' columns solved to the end and scored: (b, n_sv, n_held, n_correct, pred) and the columns' x"""
    from optiml_amd import _lib
    solver = lay.solver(dev, groups, max_iter)
    try:
        _finish(solver)
        out = lay.score(solver, groups)
        x = np.stack([solver.get(c, _lib.GET_X_NOW) for c in range(solver.k)])
        return out, x
    finally:
        solver.close()


def _check_against_host(lay, dev, groups, out, x):
    """The host on the downloaded x: coef = x y on the rows above 1e-6, u through bq_problem_gram_matmat_wide — the same
    batch-invariant 16-column product, so the device's bits — the RETURNED intercept (itself within rtol 1e-12 of intercept(), whose
    sum takes another order), ovo_decision and argmax on u + b at the held rows.  The counts and pred are compared with ==."""
    from optiml_amd.ml.svm._batched import _gram_matmat, intercept
    from optiml_amd.ml.svm.onevsone import ovo_decision
    b, n_sv, n_held, n_correct, pred = out
    cols = lay.columns(groups)
    Y = lay.Y[cols]
    sv = x > 1e-6
    U = _gram_matmat(dev, np.where(sv, x * Y, 0.), wide=True)
    for c in range(len(cols)):
        assert n_sv[c] == sv[c].sum() > 0
        np.testing.assert_allclose(b[c], intercept(Y[c], U[c], sv[c]), rtol=1e-12, atol=0)
    for j, g in enumerate(groups):
        rows = np.flatnonzero(lay.held[g])
        D = (U[j * lay.P:(j + 1) * lay.P][:, rows] + b[j * lay.P:(j + 1) * lay.P, None]).T
        want = ovo_decision((D > 0).astype(int), D, lay.ncls).argmax(axis=1)
        assert n_held[j] == len(rows) > 0
        assert n_correct[j] == int((want == lay.pcode[rows]).sum())
        print('group %d: %d of %d held rows right' % (g, n_correct[j], n_held[j]))
        assert 0 < n_correct[j] <= n_held[j]
        full = np.full(lay.n_pad, -1)
        full[rows] = want
        assert np.array_equal(pred[j], full)


def _same(a, b, ja, jb, P):
    """group ja of result a and group jb of result b have the same bits"""
    return (a[0][ja * P:(ja + 1) * P].tobytes() == b[0][jb * P:(jb + 1) * P].tobytes() and
            np.array_equal(a[1][ja * P:(ja + 1) * P], b[1][jb * P:(jb + 1) * P]) and a[2][ja] == b[2][jb] and a[3][ja] == b[3][jb] and
            np.array_equal(a[4][ja], b[4][jb]))


def test_heldout_vote_against_the_host_four_classes(amd):
    """Class sizes 255, 256, 257, 40 (the tile edge from both sides and a small class), P = 6, 2 boxes x 3 interleaved folds: 36
    columns across three 16-column chunks, 60 ProjectedGradient iterations.  Against the host; every group alone and in the reversed
    batch has the same bits; and a solver scored after 20 iterations and then run to the end has the records, x and g of one that
    was never scored."""
    from optiml_amd import _lib
    lay = _Layout([255, 256, 257, 40], [(f, Cv) for Cv in (0.25, 1.0) for f in range(3)])
    quad = tgo._quad(lay.Xp)
    dev = quad.device_problem()
    groups = list(range(6))
    out, x = _scored(lay, dev, groups)
    assert len(x) == 36
    _check_against_host(lay, dev, groups, out, x)
    rev, _ = _scored(lay, dev, groups[::-1])
    for j, g in enumerate(groups[::-1]):
        assert _same(rev, out, j, g, lay.P), g
    for g in (0, 4):
        alone, _ = _scored(lay, dev, [g])
        assert _same(alone, out, 0, g, lay.P), g
    a, b = (lay.solver(dev, groups, 60) for _ in range(2))
    first = [s.run(20)[0] for s in (a, b)]
    mid = lay.score(a, groups)
    assert mid[0].tobytes() != out[0].tobytes()   # (scored mid-way: another state than the end's)
    rest = [_finish(s) for s in (a, b)]
    assert sum(len(r) for r in rest[0]) > 0
    for c in range(36):
        assert first[0][c].tobytes() == first[1][c].tobytes() and rest[0][c].tobytes() == rest[1][c].tobytes()
        for what in (_lib.GET_X_NOW, _lib.GET_G_NOW):
            assert np.array_equal(a.get(c, what), b.get(c, what))
        assert a.state(c) == b.state(c)
    end = lay.score(a, groups)
    for g in groups:
        assert _same(end, out, g, g, lay.P)
    a.close()
    b.close()
    quad.release()


def test_heldout_vote_against_the_host_seven_classes(amd):
    """Class sizes 30, 90, 257, 3, 256, 100, 64: P = 21, so a group spans a 16-column chunk edge; 2 groups (42 columns)."""
    lay = _Layout([30, 90, 257, 3, 256, 100, 64], [(0, 1.0), (1, 0.5)])
    quad = tgo._quad(lay.Xp)
    dev = quad.device_problem()
    out, x = _scored(lay, dev, [0, 1])
    _check_against_host(lay, dev, [0, 1], out, x)
    rev, _ = _scored(lay, dev, [1, 0])
    assert _same(rev, out, 0, 1, lay.P) and _same(rev, out, 1, 0, lay.P)
    quad.release()


def test_heldout_vote_against_the_host_two_classes(amd):
    """Two classes of 300 and 40 rows, 17 groups of one column (P = 1): a second chunk of one column."""
    lay = _Layout([300, 40], [(g % 3, 0.25 * (1 + g % 5)) for g in range(17)])
    quad = tgo._quad(lay.Xp)
    dev = quad.device_problem()
    groups = list(range(17))
    out, x = _scored(lay, dev, groups)
    _check_against_host(lay, dev, groups, out, x)
    rev, _ = _scored(lay, dev, groups[::-1])
    for j, g in enumerate(groups[::-1]):
        assert _same(rev, out, j, g, lay.P), g
    quad.release()


# ---- 3. refusals --------------------------------------------------------------------------------------------------------------------
def _raw(solver, n, ngroups=1, group_of=None, held=None, data_row=None, null=None):
    """bq_msolver_pairs_vote_heldout on any solver's handle, with valid arrays but what the arguments replace: the return code"""
    from optiml_amd import _lib
    k = solver.k
    u8, i64 = (lambda a: a.ctypes.data_as(C.POINTER(C.c_ubyte))), (lambda a: a.ctypes.data_as(C.POINTER(C.c_int64)))
    group_of = np.ascontiguousarray(np.zeros(k) if group_of is None else group_of, dtype=np.int32)
    held = np.ascontiguousarray(np.zeros((ngroups, n)) if held is None else held, dtype=np.uint8)
    data_row = np.ascontiguousarray(np.ones(n) if data_row is None else data_row, dtype=np.uint8)
    b = np.empty(k)
    cnt = [np.empty(max(k, ngroups), dtype=np.int64) for _ in range(3)]
    args = [solver._h, u8(data_row), ngroups, _lib.iptr(group_of), u8(held), _lib.ptr(b), i64(cnt[0]), i64(cnt[1]), i64(cnt[2]), None]
    if null is not None:
        args[null] = None
    return _lib.load().bq_msolver_pairs_vote_heldout(*args)


def test_heldout_vote_refusals(amd):
    from optiml_amd import _lib
    from optiml_amd.ml.svm._batched import _DeviceMultiSolver, _DeviceSimplexPairSolver, _DeviceSimplexSolver
    from optiml_amd.ml.svm.kernels import GaussianKernel
    from optiml_amd.ml.svm.onevsone import _DevicePairSolver
    from optiml_amd.opti import KernelQuadratic
    lay = _Layout([40, 257, 30], [(0, 1.0)])
    n = lay.n_pad
    bad = _lib.ERR_BADARG
    # the solvers that are not bq_msolver_create_pairs's
    plain = KernelQuadratic(lay.Xp, np.zeros(n), 'plain', GaussianKernel(gamma=0.2))
    one = _DeviceSimplexSolver(plain.device_problem(), np.ones((1, n)), [0.5 * n], 1e-3, 10)
    one.run(5)
    assert _raw(one, n) == bad
    one.close()
    box = (lay.UB[:1] > 0).astype(float)
    routed = _DeviceSimplexPairSolver(plain.device_problem(), lay.ct, [(0, 1)], box, [[10.0, 10.0]], 1e-3, 10)
    routed.run(5)
    assert _raw(routed, n) == bad
    routed.close()
    plain.release()
    quad = tgo._quad(lay.Xp)
    dev = quad.device_problem()
    boxes = _DeviceMultiSolver(dev, _lib.PG, lay.Y[:3], lay.UB[:3], 1e-6, 10)
    boxes.run(5)
    assert _raw(boxes, n, held=lay.held) == bad
    boxes.close()
    # a pair solver: the groups, the held rows, NULL arguments
    pairs = lay.solver(dev, [0], 30)
    pairs.run(10)
    assert _raw(pairs, n, held=lay.held, data_row=lay.data_row) == _lib.OK
    assert _raw(pairs, n, ngroups=2, group_of=[0, 1, 1], held=np.zeros((2, n))) == bad   # k != ngroups x P
    assert _raw(pairs, n, group_of=[0, 0, 1], held=lay.held) == bad                       # a group outside [0, ngroups)
    assert _raw(pairs, n, ngroups=0, held=lay.held) == bad
    ghost = lay.held.copy()
    ghost[0, np.flatnonzero(lay.data_row == 0)[0]] = 1
    assert _raw(pairs, n, held=ghost, data_row=lay.data_row) == bad                       # a held ghost row
    trained = lay.held.copy()
    trained[0, np.flatnonzero(lay.UB[0] > 0)[0]] = 1
    assert _raw(pairs, n, held=trained, data_row=lay.data_row) == bad                     # a held row with a positive box
    for null in (0, 1, 3, 4, 5, 6, 7, 8):
        assert _raw(pairs, n, held=lay.held, data_row=lay.data_row, null=null) == bad, null
    _finish(pairs)   # the solver is still usable
    out = lay.score(pairs, [0])
    x = np.stack([pairs.get(c, _lib.GET_X_NOW) for c in range(3)])
    _check_against_host(lay, dev, [0], out, x)
    pairs.close()
    twice = _DevicePairSolver(dev, _lib.PG, lay.ct, [(0, 1), (0, 1), (1, 2)], lay.Y[[0, 0, 2]], lay.UB[[0, 0, 2]], 1e-6, 10)
    twice.run(5)
    assert _raw(twice, n, held=lay.held, data_row=lay.data_row) == bad                    # a duplicated pair, a missing one
    twice.close()
    quad.release()


# ---- 4. the search against GridSearchCV over the project's own estimator ------------------------------------------------------------
# make_multiclass_blobs(n, 6, classes, seed): the first seed, counted from 1, at which the condition of _condition holds for every
# case below.  Seed 1 holds it for both: on an MI355X the smallest |pair decision| / top-two gap over the cases are 5.4e-5 / 1.2e-2
# with 3 classes and 4.2e-6 / 3.2e-4 with 7 (FrankWolfe, gamma 0.5)
SEARCH_DATA = {3: (600, 1), 7: (1050, 1)}
MARGIN = 1e-6


def _svc_kw(opt='pg', **kw):
    from optiml_amd.ml.svm.kernels import GaussianKernel
    from optiml_amd.ml.svm.losses import hinge
    from optiml_amd.opti.constrained import FrankWolfe, ProjectedGradient
    base = dict(loss=hinge, kernel=GaussianKernel(gamma=0.5), reg_intercept=True, dual=True, max_iter=60,
                optimizer=ProjectedGradient if opt == 'pg' else FrankWolfe)
    base.update(kw)
    return base


@functools.lru_cache(maxsize=None)
def _search_data(classes):
    from optiml_amd.datasets import make_multiclass_blobs
    n, seed = SEARCH_DATA[classes]
    X, y = make_multiclass_blobs(n, 6, classes, seed=seed)
    return X, y, make_multiclass_blobs(200, 6, classes, seed=seed + 100)[0]   # and fresh rows to predict


def _pair_decisions(est, X):
    if est.batched_decision_:
        return est.decision_batch_(X)
    return np.stack([np.ravel(e.decision_function(X)) for e in est.estimators_], axis=1)


def _condition(kw, candidates, X, y, splits):
    """(smallest |pair decision|, smallest gap between the top two entries of ovo_decision) over the held-out rows of the reference's
    own per-fold fits: the two paths' products differ by summation order (about 1e-9), so a vote can differ only where one of these
    is that small"""
    from optiml_amd.ml.svm import OneVsOneSVC
    from optiml_amd.ml.svm.onevsone import ovo_decision
    small, gap = np.inf, np.inf
    for p in candidates:
        for tr, te in splits:
            est = OneVsOneSVC(**dict(kw, **p)).fit(X[tr], y[tr])
            D = _pair_decisions(est, X[te])
            small = min(small, float(np.abs(D).min()))
            if len(est.classes_) > 2:
                top = np.sort(ovo_decision((D > 0).astype(int), D, len(est.classes_)), axis=1)
                gap = min(gap, float((top[:, -1] - top[:, -2]).min()))
    return small, gap


@pytest.mark.parametrize('case', ['pg', 'fw', 'kernels'])
@pytest.mark.parametrize('classes', [3, 7])
def test_search_equals_grid_search_cv(amd, classes, case):
    """Split scores EQUAL to GridSearchCV's over OneVsOneSVC, under the condition — asserted on the reference's own per-fold fits,
    no row excluded — that no held-out pair decision is within 1e-6 of zero and no held-out row's top two entries of ovo_decision
    are within 1e-6 of each other."""
    from sklearn.model_selection import GridSearchCV, StratifiedKFold
    from optiml_amd.ml.svm import OneVsOneGridSearchCV, OneVsOneSVC
    from optiml_amd.ml.svm.kernels import GaussianKernel
    from optiml_amd.ml.svm.model_selection import parameter_grid
    X, y, Xnew = _search_data(classes)
    kw = _svc_kw('fw' if case == 'fw' else 'pg')
    grid = {'C': [0.25, 1]}
    if case == 'kernels':
        grid['kernel'] = [GaussianKernel(gamma=0.5), GaussianKernel(gamma=1.0 / 6)]
    cv = StratifiedKFold(3)
    small, gap = _condition(kw, parameter_grid(grid), X, y, list(cv.split(X, y)))
    print('%d classes, %s: min |pair decision| %.3e, min top-two gap %.3e' % (classes, case, small, gap))
    assert small >= MARGIN and gap >= MARGIN
    ours = OneVsOneGridSearchCV(OneVsOneSVC(**kw), grid, cv=3).fit(X, y)   # an int: StratifiedKFold(3)
    assert ours.batched_ is True and ours.n_splits_ == 3
    ref = GridSearchCV(OneVsOneSVC(**kw), grid, cv=cv).fit(X, y)
    nc, P = len(ours.cv_results_['params']), classes * (classes - 1) // 2
    for i in range(3):
        key = 'split%d_test_score' % i
        print(key, ours.cv_results_[key], ref.cv_results_[key])
        assert np.array_equal(ours.cv_results_[key], ref.cv_results_[key])
    _compare_results(ours, ref, 3)
    assert len(np.unique(np.stack([ref.cv_results_['split%d_test_score' % i] for i in range(3)]))) > 1   # the scores discriminate
    assert ours.cv_results_['params'] == ref.cv_results_['params']
    assert ours.n_iter_.shape == ours.status_.shape == (nc, 3, P)
    assert (ours.n_iter_ > 0).all() and set(ours.status_.ravel()) <= {'optimal', 'stopped'}
    assert np.array_equal(ours.best_estimator_.predict(Xnew), ref.best_estimator_.predict(Xnew))
    assert np.array_equal(ours.predict(Xnew), ours.best_estimator_.predict(Xnew))
    assert ours.score(X, y) == ours.best_estimator_.score(X, y)


# ---- 5. failed fits -----------------------------------------------------------------------------------------------------------------
def test_failed_fits_score_nan_as_grid_search_cv(amd):
    """At C = 1e-7 no x exceeds the 1e-6 support threshold: every pair's intercept is 0 / 0 and OneVsOneSVC.fit raises, which
    GridSearchCV records as a failed fit scored NaN.  Ours: NaN scores, rank last, status_ 'failed', one RuntimeWarning."""
    from sklearn.model_selection import GridSearchCV, StratifiedKFold
    from optiml_amd.ml.svm import OneVsOneGridSearchCV, OneVsOneSVC
    X, y, _ = _search_data(3)
    kw = _svc_kw('pg')
    grid = {'C': [1e-7, 1]}
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter('always')
        ours = OneVsOneGridSearchCV(OneVsOneSVC(**kw), grid, cv=3).fit(X, y)
    runtime = [w for w in caught if issubclass(w.category, RuntimeWarning)]
    assert len(runtime) == 1 and '3 fits failed out of a total of 6' in str(runtime[0].message)
    assert ours.batched_ is True
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        ref = GridSearchCV(OneVsOneSVC(**kw), grid, cv=StratifiedKFold(3)).fit(X, y)
    for i in range(3):
        key = 'split%d_test_score' % i
        assert np.isnan(ref.cv_results_[key][0]) and np.isnan(ours.cv_results_[key][0])
        assert ours.cv_results_[key][1] == ref.cv_results_[key][1]
    for key in ('mean_test_score', 'std_test_score'):
        assert np.array_equal(ours.cv_results_[key], ref.cv_results_[key], equal_nan=True)
    assert list(ours.cv_results_['rank_test_score']) == list(ref.cv_results_['rank_test_score']) == [2, 1]
    assert ours.best_index_ == ref.best_index_ == 1
    assert (ours.status_[0] == 'failed').all() and (ours.n_iter_[0] == -1).all()
    assert set(ours.status_[1].ravel()) <= {'optimal', 'stopped'} and (ours.n_iter_[1] > 0).all()
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        with pytest.raises(ValueError, match='all the 3 fits failed'):
            OneVsOneGridSearchCV(OneVsOneSVC(**kw), {'C': [1e-7]}, cv=3).fit(X, y)


# ---- 6. fallbacks -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('which', ['scale', 'f32', 'tol', 'missing-class'])
def test_fallback_equals_grid_search_cv(amd, which):
    from sklearn.model_selection import GridSearchCV, StratifiedKFold
    from optiml_amd.ml.svm import OneVsOneGridSearchCV, OneVsOneSVC
    from optiml_amd.ml.svm.kernels import GaussianKernel
    X, y, _ = _search_data(3)
    X, y = X[:240], y[:240]
    kw = _svc_kw('pg', max_iter=30)
    grid = {'C': [0.25, 1]}
    cv = list(StratifiedKFold(3).split(X, y))
    if which == 'scale':
        kw['kernel'] = GaussianKernel(gamma='scale')
    elif which == 'f32':
        kw['storage'] = 'f32'
    elif which == 'tol':
        grid = {'C': [0.25, 1], 'tol': [1e-4, 1e-2]}
    else:   # the first fold trains without the largest class and is scored on it alone
        last = np.flatnonzero(y == y.max())
        cv[0] = (np.setdiff1d(np.arange(len(y)), last), last)
    ours = OneVsOneGridSearchCV(OneVsOneSVC(**kw), grid, cv=cv).fit(X, y)
    assert ours.batched_ is False
    ref = GridSearchCV(OneVsOneSVC(**kw), grid, cv=cv).fit(X, y)
    for i in range(3):
        assert np.array_equal(ours.cv_results_['split%d_test_score' % i], ref.cv_results_['split%d_test_score' % i])
    assert ours.best_params_ == ref.best_params_ and ours.n_iter_.shape[:2] == (len(ours.cv_results_['params']), 3)
