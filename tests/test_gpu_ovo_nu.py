"""OneVsOneNuSVC on the device: the two-group simplex solver on a class-sorted panel with the pair-routed product
(bq_msolver_create_simplex2_pairs: the BLOCKS instantiations of sx_tau / sx_dir / sx_start / sx_close around bq_symmp.hip) against
the per-pair NumPy reference (tests/ovo_nu_reference.py), its batch invariance, its edges, the rows a column does not own, the
refusals; the estimator against sklearn's OneVsOneClassifier(NuSVC), its fallback, decision routes, path and fp32 panels."""
import functools

import numpy as np
import pytest

import nu_reference as nur
import ovo_nu_reference as onr
from test_gpu_nu import _follows, _same_bits

pytestmark = pytest.mark.gpu

TILE = 256


@pytest.fixture(scope='module')
def amd():
    from optiml_amd import _lib
    from optiml_amd.device import get_context
    _lib.load()
    get_context()


class _Panel:
    """the class-sorted, ghost-padded panel of (X, codes) as OneVsOneNuSVC builds it"""

    def __init__(self, X, codes, gamma, storage='f64', structure='plain'):
        from optiml_amd.ml.svm.kernels import GaussianKernel
        from optiml_amd.ml.svm.onevsone import sort_plan
        from optiml_amd.opti import KernelQuadratic
        self.X, self.codes, self.ncls = X, codes, int(codes.max()) + 1
        self.index, self.ct, self.n_pad = sort_plan(codes, self.ncls)
        Xp = np.zeros((self.n_pad, X.shape[1]))
        Xp[self.index] = X
        self.ghost = np.ones(self.n_pad, dtype=bool)
        self.ghost[self.index] = False
        self.pcode = np.repeat(np.arange(self.ncls), np.diff(self.ct) * TILE)
        if structure == 'plain':
            self.quad = KernelQuadratic(Xp, np.zeros(self.n_pad), 'plain', GaussianKernel(gamma=gamma), storage=storage)
        else:
            self.quad = KernelQuadratic(Xp, -np.ones(self.n_pad), 'svc', GaussianKernel(gamma=gamma), y=np.ones(self.n_pad))
        self.dev = self.quad.device_problem()

    def boxes(self, pairs):
        return np.stack([np.where(((self.pcode == i) | (self.pcode == j)) & ~self.ghost, 1., 0.) for i, j in pairs])

    def pos(self, pair):
        """the pair's data rows (original order), their labels and their panel rows"""
        rows, y = onr.pair_rows(self.codes, *pair)
        return rows, y, self.index[rows]

    def solve(self, pairs, UB, mass, tol, max_iter, x0=None, chunk=256):
        """the columns' results (rows, status, iter, f_x, x, g in panel order) with d, r1, r2, n_sv, n_free from the device"""
        from optiml_amd import _lib
        from optiml_amd.ml.svm._batched import _DeviceSimplexPairSolver, solve_batched
        held = {}

        def last(solver, _):
            held['off'] = solver.offsets()
            held['d'] = [solver.get(c, _lib.GET_D) for c in range(len(pairs))]

        solver = _DeviceSimplexPairSolver(self.dev, self.ct, pairs, UB, mass, tol, max_iter, x0)
        res = solve_batched(self.dev, None, np.atleast_2d(UB), None, solver=solver, before_close=last, chunk=chunk)
        r1, r2, n_sv, n_free = held['off']
        for c, r in enumerate(res):
            r.update(d=held['d'][c], r1=r1[c], r2=r2[c], n_sv=tuple(int(v) for v in n_sv[c]), n_free=tuple(int(v) for v in n_free[c]))
        return res

    def release(self):
        self.quad.release()


# ---- 1 and 4. trajectory parity; the rows a column does not own ----------------------------------------------------------------------
@pytest.fixture(scope='module')
def traj(amd):
    """counts (1100, 300, 130, 257): class 0 is 5 tile rows, ragged, with a second trip of the 1024-thread loop; class 2 one tile with
    126 ghost rows; class 3 two tiles with 255 ghost rows; class 0's diagonal block serves 6 of the 12 columns.  One solve, tol = 0,
    20 iterations."""
    X, codes, cols = onr.traj_columns()
    panel = _Panel(X, codes, onr.TRAJ_GAMMA)
    assert list(panel.ct) == [0, 5, 7, 8, 10]
    pairs = [pair for pair, _ in cols]
    UB = panel.boxes(pairs)
    mass = np.array([[ms, ms] for _, ms in cols])
    res = panel.solve(pairs, UB, mass, 0.0, onr.TRAJ_ITERS)
    yield panel, pairs, UB, mass, res
    panel.release()


def test_trajectory_parity(traj):
    """Every column against nu_reference.solve on its pair's own sub-Gram under test_gpu_nu.test_trajectory_parity's conditions:
    statuses, iteration counts and the records' iter are the reference's, the f history agrees to rtol 1e-9, the violation to rtol
    1e-6 / atol 1e-9, and x after the last iteration lies within 10 x the spread that one ulp per entry of K gives the reference's
    own x.  The boxes hold bitwise.  (The reference asserts that every column is far from its optimum at iteration 20.)"""
    panel, pairs, UB, mass, res = traj
    _, _, _, ref = onr.trajectory_reference()
    for c, (r, (rows, base, spread)) in enumerate(zip(res, ref)):
        pos = panel.index[rows]
        assert r['status'] == base['status'] and r['iter'] == base['iter']
        assert np.array_equal(r['rows']['iter'], base['rows'][:, 0].astype(np.int64))
        nur.assert_f_history(r['rows']['f'], base)
        np.testing.assert_allclose(r['rows']['r1'], base['rows'][:, 2], rtol=1e-6, atol=1e-9)
        err = float(np.abs(r['x'][pos] - base['x']).max())
        print('column %d, pair %s: |x - x_ref| = %.2e, 10 x spread = %.2e' % (c, pairs[c], err, 10 * spread))
        assert err <= 10 * spread
        assert np.all(r['x'] >= 0) and np.all(r['x'] <= UB[c])


def test_rows_the_column_does_not_own(traj):
    """x and d are exactly 0 on ghost rows and on every row outside the pair's classes, g is exactly 0 outside the pair's classes,
    and each group sums to its mass within 1e-10 relative."""
    panel, pairs, UB, mass, res = traj
    for c, ((i, j), r) in enumerate(zip(pairs, res)):
        mine = (panel.pcode == i) | (panel.pcode == j)
        assert r['x'].shape == r['g'].shape == r['d'].shape == (panel.n_pad,)
        for v in (r['x'], r['d']):
            assert not v[~mine].any() and not v[panel.ghost].any()
        assert not r['g'][~mine].any()
        assert np.abs(r['d'][mine & ~panel.ghost]).max() > 0 and np.abs(r['g'][mine]).max() > 0
        for t, cls in enumerate((j, i)):   # group 0: the larger class
            assert abs(r['x'][panel.pcode == cls].sum() - mass[c, t]) <= 1e-10 * mass[c, t]


# ---- 2. batch invariance -------------------------------------------------------------------------------------------------------------
def test_batch_invariance_bit_for_bit(traj):
    """tol = 2e-2, at most 60 iterations: the 12 columns stop at four or more different iterations, so pairs leave the routed
    product one after another.  Every column's x, g, records, r1, r2 and status have the same bits in the batch, alone, in the
    reversed batch and with the run cut into bq_msolver_run calls of 7 iterations."""
    panel, pairs, UB, mass, _ = traj
    tol, cap = 2e-2, 60
    res = panel.solve(pairs, UB, mass, tol, cap)
    iters = [r['iter'] for r in res]
    print('iterations:', iters)
    assert len(set(iters)) >= 4 and min(iters) < cap
    order = np.arange(len(pairs))[::-1]
    rev = panel.solve([pairs[c] for c in order], UB[order], mass[order], tol, cap)
    for j, c in enumerate(order):
        assert _same_bits(rev[j], res[c]), c
    cut = panel.solve(pairs, UB, mass, tol, cap, chunk=7)
    for c in range(len(pairs)):
        assert _same_bits(cut[c], res[c]), c
        alone = panel.solve([pairs[c]], UB[c:c + 1], mass[c:c + 1], tol, cap)[0]
        assert _same_bits(alone, res[c]), c


# ---- 3. edges ------------------------------------------------------------------------------------------------------------------------
EDGE_COUNTS, EDGE_GAMMA = (256, 1, 40), 1.0


@pytest.fixture(scope='module')
def edge(amd):
    X, _, codes = onr.ovo_nu_data(EDGE_COUNTS, 3)
    panel = _Panel(X, codes, EDGE_GAMMA)
    assert list(panel.ct) == [0, 1, 2, 3] and not panel.ghost[:256].any() and panel.ghost[256:512].sum() == 255
    yield panel
    panel.release()


def test_edges(edge):
    """A class that fills its tile (no ghost row) and a one-row group: pair (1, 2) at mass 0.5; the same pair with the one-row
    group's mass its whole box (x = 1 there from the start to the end); pair (0, 2) with every third data row of its classes held
    out (UB = 0 there: the reference runs on the trained rows' sub-Gram).  Each follows the reference: status, iterations, f
    history to rtol 1e-9, x to 1e-9."""
    panel = edge
    pairs = [(1, 2), (1, 2), (0, 2)]
    UB = panel.boxes(pairs)
    rows02, _, pos02 = panel.pos((0, 2))
    held = np.arange(len(rows02)) % 3 == 1
    UB[2][pos02[held]] = 0.
    mass = np.array([[0.5, 0.5], [12.5, 1.0], [10.0, 10.0]])   # (class b, class a)
    res = panel.solve(pairs, UB, mass, 1e-6, 25)
    for c, pair in enumerate(pairs):
        rows, y, pos = panel.pos(pair)
        u = UB[c][pos]
        tr = u > 0
        ref = onr.solve_column(panel.X[rows[tr]], panel.codes[rows[tr]], pair, tuple(mass[c]), EDGE_GAMMA, 1e-6, 25)[3]
        assert ref['iter'] >= 3, (c, ref['iter'])
        got = dict(res[c], x=res[c]['x'][pos[tr]])
        _follows(got, ref)
        assert not res[c]['x'][pos[~tr]].any()
        for t, cls in enumerate((1., -1.)):
            assert abs(got['x'][y[tr] == cls].sum() - mass[c, t]) <= 1e-10 * mass[c, t]
    assert res[1]['x'][panel.index[np.flatnonzero(panel.codes == 1)]] == 1.0


def test_a_feasible_start_point(edge):
    """A start point inside the set of pair (0, 2) that is not the projection of 0: the reference from the same start."""
    panel = edge
    pair, mass = (0, 2), (8.0, 20.0)
    rows, y, pos = panel.pos(pair)
    UB = panel.boxes([pair])
    w = 0.5 + np.random.RandomState(5).rand(len(y))   # not the uniform point, which is P(0)
    x0p = np.where(y > 0, mass[0] * w / w[y > 0].sum(), mass[1] * w / w[y < 0].sum())
    x0 = np.zeros((1, panel.n_pad))
    x0[0, pos] = x0p
    r = panel.solve([pair], UB, [mass], 1e-6, 25, x0=x0)[0]
    ref = onr.solve_column(panel.X, panel.codes, pair, mass, EDGE_GAMMA, 1e-6, 25, x0=x0p)[3]
    assert ref['iter'] >= 3 and x0p.max() <= 1 and np.ptp(x0p[y > 0]) > 0
    _follows(dict(r, x=r['x'][pos]), ref)


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals(edge):
    from optiml_amd import _lib
    from optiml_amd.ml.svm._batched import _DeviceSimplexPairSolver
    from optiml_amd.opti import KernelQuadratic
    from optiml_amd.ml.svm.kernels import GaussianKernel
    panel = edge
    pair = (0, 2)
    UB = panel.boxes([pair])
    ok = dict(cls_tiles=panel.ct, pairs=[pair], UB=UB, mass=[[10.0, 10.0]], x0=None)
    assert panel.solve(ok['pairs'], UB, ok['mass'], 1e-3, 5)[0]['iter'] >= 1

    def refused(dev=None, **kw):
        a = dict(ok, **kw)
        with pytest.raises(_lib.BcqpError):
            _DeviceSimplexPairSolver(dev or panel.dev, a['cls_tiles'], a['pairs'], a['UB'], a['mass'], 1e-3, 10, a['x0'])

    outside = UB.copy()
    outside[0, 256] = 1.   # class 1's data row
    refused(UB=outside)
    ghost = UB.copy()
    ghost[0, 300] = 1.     # a ghost row of class 1: outside the pair too
    refused(UB=ghost)
    empty = UB.copy()
    empty[0, :256] = 0.    # class 0 (group 1) has no box
    refused(UB=empty)
    refused(UB=-UB)
    refused(mass=[[40.5, 10.0]])    # above class 2's 40 rows
    refused(mass=[[10.0, 0.0]])
    refused(pairs=[(2, 0)])
    refused(pairs=[(0, 3)])
    refused(cls_tiles=np.array([0, 1, 1, 3]))     # not increasing
    refused(cls_tiles=np.array([0, 1, 2, 4]))     # not the panel's tile rows
    refused(x0=2 * UB)
    with pytest.raises(ValueError):
        _DeviceSimplexPairSolver(panel.dev, panel.ct, [pair], UB[:, :700], ok['mass'], 1e-3, 10)
    with pytest.raises(ValueError):
        _DeviceSimplexPairSolver(panel.dev, panel.ct, [pair, pair], UB, ok['mass'], 1e-3, 10)
    svc = _Panel(panel.X, panel.codes, EDGE_GAMMA, structure='svc')
    refused(dev=svc.dev)
    svc.release()
    Xp = np.zeros((panel.n_pad, panel.X.shape[1]))
    Xp[panel.index] = panel.X
    streamed = KernelQuadratic(Xp, np.zeros(panel.n_pad), 'plain', GaussianKernel(gamma=EDGE_GAMMA), storage='stream')
    refused(dev=streamed.device_problem())
    streamed.release()


# ---- 6. the estimator against sklearn ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _fit(gamma, nu, tol, storage='f64'):
    from optiml_amd.ml.svm import OneVsOneNuSVC
    from optiml_amd.ml.svm.kernels import GaussianKernel
    X, _, _, y = onr.est_data()
    return OneVsOneNuSVC(kernel=GaussianKernel(gamma=gamma), nu=nu, tol=tol, storage=storage).fit(X, y)


@pytest.mark.parametrize('tol', onr.TOLS)
@pytest.mark.parametrize('gamma,nu', onr.EST_GRID)
def test_against_sklearn(amd, gamma, nu, tol):
    """ovo_nu_reference.check_against_sklearn's conditions (the host test holds the NumPy reference to the same) with the default
    max_iter, and: every estimator is a NuSVC fitted on the pair's rows in their original order with the larger class positive."""
    pytest.importorskip('sklearn')
    from optiml_amd.ml.svm import NuSVC
    X, _, codes, y = onr.est_data()
    est = _fit(gamma, nu, tol)
    assert est.batched_ and est.batched_decision_ and est.n_classes_ == 3 and np.array_equal(est.classes_, onr.EST_LABELS)
    onr.check_against_sklearn(est, onr.sk_ovo(gamma, nu), gamma, nu, tol)
    for e, (i, j) in zip(est.estimators_, onr.pairs_of(3)):
        rows, yp = onr.pair_rows(codes, i, j)
        a = e.alphas_
        assert type(e) is NuSVC and e.nu == nu and np.array_equal(e.classes_, [0, 1]) and e.kernel_ is est.kernel
        assert np.array_equal(e.support_, np.flatnonzero(a > 0)) and np.array_equal(e.support_vectors_, X[rows][a > 0])
        assert np.array_equal(e.dual_coef_, (yp * a)[a > 0] / e.margin_scale_)
        assert len(e.train_loss_history) == e.n_iter_ + 1
    assert 0.5 <= est.score(X, y) <= 1.0


# ---- 7. gamma = 'scale' --------------------------------------------------------------------------------------------------------------
def test_gamma_scale_takes_the_per_pair_route(amd):
    from optiml_amd.ml.svm import NuSVC, OneVsOneNuSVC
    from optiml_amd.ml.svm.kernels import GaussianKernel
    X, Xnew, codes, y = onr.est_data()
    kw = dict(kernel=GaussianKernel(gamma='scale'), nu=0.5017, tol=1e-3)
    est = OneVsOneNuSVC(**kw).fit(X, y)
    assert est.batched_ is False and est.batched_decision_ is False and est.decision_batch_ is None
    conf = []
    for e, (i, j) in zip(est.estimators_, onr.pairs_of(3)):
        rows, yp = onr.pair_rows(codes, i, j)
        one = NuSVC(**kw).fit(X[rows], (yp > 0).astype(int))
        assert np.array_equal(e.alphas_, one.alphas_) and e.intercept_ == one.intercept_ and e.n_iter_ == one.n_iter_
        assert e.train_loss_history == one.train_loss_history and e.kernel_.gamma == one.kernel_.gamma
        assert np.array_equal(e.decision_function(Xnew), one.decision_function(Xnew))
        conf.append(one.decision_function(Xnew))
    assert np.array_equal(est.decision_function(Xnew), onr.ovo_decision(np.stack(conf, axis=1), 3))


# ---- 8. decision routes --------------------------------------------------------------------------------------------------------------
def test_decision_routes(amd):
    """decision_function through the DecisionBatch against the per-estimator loop (rtol = atol = 1e-9, the tolerance of the
    estimator-level comparisons of test_gpu_decision_batch.py); two classes give a 1-D decision and predictions from its sign."""
    from optiml_amd.ml.svm import OneVsOneNuSVC
    from optiml_amd.ml.svm.kernels import GaussianKernel
    from optiml_amd.ml.svm.onevsone import ovo_decision
    X, Xnew, codes, y = onr.est_data()
    est = _fit(0.5, 0.5017, 1e-3)
    assert est.batched_decision_ and est.decision_batch_ is not None
    for Z in (X, Xnew):
        conf = np.stack([e.decision_function(Z) for e in est.estimators_], axis=1)
        np.testing.assert_allclose(est.decision_batch_(Z), conf, rtol=1e-9, atol=1e-9)
        loop = ovo_decision((conf > 0).astype(int), conf, 3)
        np.testing.assert_allclose(est.decision_function(Z), loop, rtol=1e-9, atol=1e-9)
    two = codes != 1
    est2 = OneVsOneNuSVC(kernel=GaussianKernel(gamma=0.5), nu=0.5017).fit(X[two], y[two])
    assert est2.batched_ and not est2.batched_decision_ and len(est2.estimators_) == 1
    dec = est2.decision_function(Xnew)
    assert dec.shape == (50,)
    conf = est2.estimators_[0].decision_function(Xnew)
    assert np.array_equal(est2.predict(Xnew), np.where(conf > 0, 11, 3))
    assert np.array_equal(dec > 0, conf > 0)


# ---- 9. the path ---------------------------------------------------------------------------------------------------------------------
def test_path_equals_the_single_fits(amd):
    from optiml_amd.ml.svm import OneVsOneNuSVC, ovo_nu_svc_path
    from optiml_amd.ml.svm.kernels import GaussianKernel
    X, Xnew, _, y = onr.est_data()
    nus = [0.5017, 0.3517, 0.4517]

    class Mine(OneVsOneNuSVC):
        pass
    kw = dict(kernel=GaussianKernel(gamma=0.5), tol=1e-4)
    proto = Mine(**kw)
    path = ovo_nu_svc_path(proto, X, y, nus)
    assert [e.nu for e in path] == nus and all(type(e) is Mine for e in path)
    assert proto.nu == 0.5 and not hasattr(proto, 'estimators_') and not hasattr(proto, 'classes_')
    for est in path:
        one = Mine(nu=est.nu, **kw).fit(X, y)
        assert est.batched_ and np.array_equal(est.classes_, one.classes_) and len(est.estimators_) == 3
        for a, b in zip(est.estimators_, one.estimators_):
            assert a.status_ == 'optimal' and a.nu == est.nu
            assert np.array_equal(a.alphas_, b.alphas_) and a.intercept_ == b.intercept_ and a.n_iter_ == b.n_iter_
            assert a.train_loss_history == b.train_loss_history and a.margin_scale_ == b.margin_scale_
            assert np.array_equal(a.dual_coef_, b.dual_coef_) and np.array_equal(a.support_, b.support_)
        assert np.array_equal(est.decision_function(Xnew), one.decision_function(Xnew))


# ---- 10. fp32 panels -----------------------------------------------------------------------------------------------------------------
def test_fp32_panel(amd):
    """storage='f32' fits, is 'optimal' at tol 1e-3, and predicts as the f64 fit on the rows that test 6's conditions call clear:
    every pair's sklearn |decision| above 10 tol / r and sklearn's top two values more than twice sum_p bound_p / 3 apart."""
    pytest.importorskip('sklearn')
    X, _, _, y = onr.est_data()
    gamma, nu, tol = 0.5, 0.5017, 1e-3
    a, b = _fit(gamma, nu, tol, 'f32'), _fit(gamma, nu, tol)
    assert a.batched_ and all(e.status_ == 'optimal' for e in a.estimators_)
    bounds = [10 * tol / e.margin_scale_ for e in b.estimators_]
    _, sure = onr.clear_rows(onr.sk_ovo(gamma, nu), bounds, X)
    print('fp32 panel: %d of %d rows clear' % (sure.sum(), len(X)))
    assert sure.sum() >= 0.95 * len(X)
    assert np.array_equal(a.predict(X)[sure], b.predict(X)[sure])
