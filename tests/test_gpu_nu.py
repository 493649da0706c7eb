"""NuSVC and NuSVR on the device: the two-group simplex solver (bq_msolver_create_simplex2: sx_top / sx_tau / sx_dir / sx_close
around the 16-column panel product) against the NumPy reference (tests/nu_reference.py), the group handling at its edges, one box
per column, the estimators against sklearn, the paths, the refusals and fp32 panels."""
import functools

import numpy as np
import pytest

import nu_reference as nur

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def amd():
    from optiml_amd import _lib
    from optiml_amd.device import get_context
    _lib.load()
    get_context()


def _quad(X, kernel, storage='f64'):
    from optiml_amd.opti import KernelQuadratic
    return KernelQuadratic(X, np.zeros(X.shape[0]), 'plain', kernel, storage=storage)


def _solve(dev, S, UB, mass, q, tol, max_iter, x0=None):
    """the columns' results (rows, status, iter, f_x, x, g) with r1, r2, n_sv, n_free from the device"""
    from optiml_amd.ml.svm._batched import _DeviceSimplex2Solver, solve_batched
    UB = np.atleast_2d(UB)
    held = []
    res = solve_batched(dev, None, UB, None, solver=_DeviceSimplex2Solver(dev, S, UB, mass, q, tol, max_iter, x0),
                        before_close=lambda s, _: held.extend(s.offsets()))
    for c, r in enumerate(res):
        r.update(r1=held[0][c], r2=held[1][c], n_sv=tuple(int(v) for v in held[2][c]), n_free=tuple(int(v) for v in held[3][c]))
    return res


def _same_bits(a, b):
    return (np.array_equal(a['x'], b['x']) and np.array_equal(a['g'], b['g']) and len(a['rows']) == len(b['rows']) and
            a['rows'].tobytes() == b['rows'].tobytes() and a['r1'] == b['r1'] and a['r2'] == b['r2'] and a['status'] == b['status'])


def _follows(r, ref, x_atol=1e-9):
    """status, iterations, the f history to rtol 1e-9 (nu_reference.assert_f_history: a PAIRED column's f starts at an exact 0, which
    is held to the rounding bound of that sum instead) and x"""
    assert r['status'] == ref['status'] and r['iter'] == ref['iter'], (r['status'], r['iter'], ref['status'], ref['iter'])
    nur.assert_f_history(r['rows']['f'], ref)
    np.testing.assert_allclose(r['x'], ref['x'], rtol=0, atol=x_atol)


def _data(n, seed):
    """n rows of 3 features with the issue's noisy labels and targets (drawn as nu_reference.nu_data draws them)"""
    rs = np.random.RandomState(seed)
    X = rs.standard_normal((n, 3))
    y = np.where(X[:, 0] + 0.5 * X[:, 1] ** 2 + 0.6 * rs.standard_normal(n) > 0.4, 1., -1.)
    t = np.sin(X[:, 0]) + 0.5 * X[:, 1] + 0.2 * rs.standard_normal(n)
    return X, y, t


def _labels_columns(y, nus, UB=None):
    """S, UB, mass of NuSVC columns with these nu (mass: nu x the trained rows / 2 per class)"""
    k, n = len(nus), len(y)
    UB = np.ones((k, n)) if UB is None else UB
    mass = np.array([[nu * np.count_nonzero(UB[c]) / 2] * 2 for c, nu in enumerate(nus)])
    return np.tile(y, (k, 1)), UB, mass


def _paired_columns(t, params, UB1=None):
    """UB, mass, q of NuSVR columns (C, nu); UB1: k x n 0/1 masks of the trained rows"""
    k, n = len(params), len(t)
    UB1 = np.ones((k, n)) if UB1 is None else UB1
    UB = np.stack([np.concatenate((C * UB1[c], C * UB1[c])) for c, (C, _) in enumerate(params)])
    mass = np.array([[C * nu * np.count_nonzero(UB1[c]) / 2] * 2 for c, (C, nu) in enumerate(params)])
    return UB, mass, np.tile(np.concatenate((-t, t)), (k, 1))


# ---- 1. trajectory parity -------------------------------------------------------------------------------------------------------------
TRAJ_GAMMA = 3.0   # d = 3: no column of either layout is near its optimum after 30 iterations (asserted on the reference)
TRAJ_NUS = (0.2517, 0.5017, 0.8017)
TRAJ_SVR = ((1.0, 0.2517), (1.0, 0.5017), (0.5, 0.8017))


@functools.lru_cache(maxsize=None)
def _trajectory_reference(n, paired):
    """The reference's 30 iterations of the three columns, and per column the largest spread of its final x over three seeded draws of
    K perturbed by one ulp per entry (test_gpu_oneclass._trajectory_reference's figure)."""
    from oracle import svm_oracle as so
    X, y, t = _data(n, n)
    K = so.gram('rbf', X, gamma=TRAJ_GAMMA)
    if paired:
        UB, mass, Q = _paired_columns(t, TRAJ_SVR)
        cols = [dict(u=UB[c], mass=tuple(mass[c]), q=Q[c]) for c in range(3)]
    else:
        S, UB, mass = _labels_columns(y, TRAJ_NUS)
        cols = [dict(u=UB[c], mass=tuple(mass[c]), sgn=y) for c in range(3)]
    out = []
    for kw in cols:
        base = nur.solve(K, tol=0.0, max_iter=30, **kw)
        assert base['status'] == 'stopped' and base['iter'] == 30 and base['rows'][-1, 2] > 1e-3   # far from its optimum
        spread = 0.0
        for seed in range(3):
            up = np.random.RandomState(seed).rand(n, n) < 0.5
            r = nur.solve(np.nextafter(K, np.where(up, np.inf, -np.inf)), tol=0.0, max_iter=30, **kw)
            assert r['iter'] == base['iter']
            spread = max(spread, float(np.abs(r['x'] - base['x']).max()))
        out.append((base, spread))
    return X, y, t, out


@pytest.mark.parametrize('paired', [False, True], ids=['labels', 'paired'])
@pytest.mark.parametrize('n', [600, 1100])
def test_trajectory_parity(amd, n, paired):
    """n = 600: 3 tile rows and a ragged last tile; n = 1100: 5, and a second, ragged trip of the 1024-thread loop.  tol = 0,
    max_iter = 30, three columns in one solve: statuses, iteration counts and the records' iter are the reference's, the f history
    agrees to rtol 1e-9, the violation to rtol 1e-6 / atol 1e-9, and x after the last iteration lies within 10 x the spread that one
    ulp per entry of K gives the reference's own x.  The boxes hold bitwise."""
    from optiml_amd.ml.svm.kernels import GaussianKernel
    X, y, t, ref = _trajectory_reference(n, paired)
    quad = _quad(X, GaussianKernel(gamma=TRAJ_GAMMA))
    if paired:
        UB, mass, Q = _paired_columns(t, TRAJ_SVR)
        res = _solve(quad.device_problem(), None, UB, mass, Q, 0.0, 30)
    else:
        S, UB, mass = _labels_columns(y, TRAJ_NUS)
        res = _solve(quad.device_problem(), S, UB, mass, None, 0.0, 30)
    for c, (r, (base, spread)) in enumerate(zip(res, ref)):
        assert r['status'] == base['status'] and r['iter'] == base['iter']
        assert np.array_equal(r['rows']['iter'], base['rows'][:, 0].astype(np.int64))
        nur.assert_f_history(r['rows']['f'], base)
        np.testing.assert_allclose(r['rows']['r1'], base['rows'][:, 2], rtol=1e-6, atol=1e-9)
        err = float(np.abs(r['x'] - base['x']).max())
        print('n=%d %s column %d: |x - x_ref| = %.2e, 10 x spread = %.2e' % (n, 'paired' if paired else 'labels', c, err, 10 * spread))
        assert err <= 10 * spread
        assert np.all(r['x'] >= 0) and np.all(r['x'] <= UB[c])
    quad.release()


# ---- 2. the group handling at its edges ------------------------------------------------------------------------------------------------
def _edge(n, n_pos, seed):
    """n rows whose first n_pos (by a seeded shuffle) carry +1"""
    X, _, t = _data(n, seed)
    y = -np.ones(n)
    y[np.random.RandomState(seed + 1).permutation(n)[:n_pos]] = 1.
    return X, y, t


@pytest.mark.parametrize('n,n_pos,mass', [(257, 1, (0.5, 20.0)), (1100, 40, (12.5, 12.5))], ids=['one-row-group', '40-and-1060'])
def test_label_groups_of_unequal_sizes(amd, n, n_pos, mass):
    """n = 257 with a positive group of exactly one row (its projection is a one-row search); n = 1100 with groups of 40 and 1060 rows
    spread over the index range: one group fits a single pass of the 1024-thread loop, the other takes the ragged second trip.  Both
    follow the reference: status, iterations, f history to rtol 1e-9, x to 1e-9."""
    from optiml_amd.ml.svm.kernels import GaussianKernel
    from oracle import svm_oracle as so
    X, y, _ = _edge(n, n_pos, 7)
    K = so.gram('rbf', X, gamma=1.0)
    quad = _quad(X, GaussianKernel(gamma=1.0))
    r = _solve(quad.device_problem(), y[None, :], np.ones((1, n)), [mass], None, 1e-6, 25)[0]
    ref = nur.solve(K, np.ones(n), mass, sgn=y, tol=1e-6, max_iter=25)
    assert ref['iter'] >= 5
    _follows(r, ref)
    for cls, ms in zip((1., -1.), mass):
        assert abs(r['x'][y == cls].sum() - ms) <= 1e-10 * ms
    quad.release()


def test_interleaved_and_sorted_labels(amd):
    """The same rows with the labels interleaved and sorted by class (the data permuted with them): the same problem, so the same f
    history to rtol 1e-9 and the same x through the permutation to 1e-9."""
    from optiml_amd.ml.svm.kernels import GaussianKernel
    n = 600
    X, y, _ = _data(n, 11)
    order = np.argsort(-y, kind='stable')   # the +1 rows first
    mass = [[0.4 * n / 2] * 2]
    out = []
    for Xp, yp in ((X, y), (X[order], y[order])):
        quad = _quad(Xp, GaussianKernel(gamma=1.0))
        out.append(_solve(quad.device_problem(), yp[None, :], np.ones((1, n)), mass, None, 0.0, 20)[0])
        quad.release()
    a, b = out
    assert a['iter'] == b['iter'] == 20
    np.testing.assert_allclose(a['rows']['f'], b['rows']['f'], rtol=1e-9)
    np.testing.assert_allclose(a['x'][order], b['x'], rtol=0, atol=1e-9)


def test_a_group_whose_mass_is_its_whole_box(amd):
    """nu = 2 min(n+, n-) / n: the smaller class's mass is its whole box, so its x equals UB exactly from the start to the end, and the
    other class still iterates (against the reference)."""
    from optiml_amd.ml.svm.kernels import GaussianKernel
    from oracle import svm_oracle as so
    n = 600
    X, y, _ = _edge(n, 200, 5)
    K = so.gram('rbf', X, gamma=1.0)
    mass = (200.0, 200.0)   # nu n / 2 with nu = 2 * 200 / 600
    quad = _quad(X, GaussianKernel(gamma=1.0))
    r = _solve(quad.device_problem(), y[None, :], np.ones((1, n)), [mass], None, 1e-6, 25)[0]
    ref = nur.solve(K, np.ones(n), mass, sgn=y, tol=1e-6, max_iter=25)
    assert ref['iter'] >= 5
    _follows(r, ref)
    assert np.array_equal(r['x'][y > 0], np.ones(200))
    assert abs(r['x'][y < 0].sum() - 200.0) <= 1e-10 * 200.0
    quad.release()


def test_paired_at_600(amd):
    """PAIRED at n = 600: m = 1200 variables, the second half straddling the 1024-thread stride; a column with a linear term, to
    tol 1e-4: the reference's status, iterations, f history and x."""
    from optiml_amd.ml.svm.kernels import GaussianKernel
    from oracle import svm_oracle as so
    n = 600
    X, _, t = _data(n, 13)
    K = so.gram('rbf', X, gamma=0.5)
    UB, mass, Q = _paired_columns(t, [(1.0, 0.4017)])
    quad = _quad(X, GaussianKernel(gamma=0.5))
    r = _solve(quad.device_problem(), None, UB, mass, Q, 1e-4, 40)[0]
    ref = nur.solve(K, UB[0], tuple(mass[0]), q=Q[0], tol=1e-4, max_iter=40)
    assert ref['iter'] >= 5
    _follows(r, ref)
    assert r['x'].shape == (2 * n,) and r['g'].shape == (2 * n,)
    for half in (r['x'][:n], r['x'][n:]):
        assert abs(half.sum() - mass[0, 0]) <= 1e-10 * mass[0, 0]
    quad.release()


# ---- 3. one box per column ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _columns17(paired):
    """17 columns (two chunks of 16) on n = 600 rows: column c holds out fold c % 3 of three interleaved folds (u = 0 there) and has
    its parameters from a mixed list"""
    n = 600
    X, y, t = _data(n, 17)
    masks = np.ones((17, n))
    for c in range(17):
        masks[c, np.arange(n) % 3 == c % 3] = 0.
    nus = [0.3517, 0.5017, 0.7017, 0.8017, 0.2517, 0.6017]
    if paired:
        UB, mass, Q = _paired_columns(t, [((1.0, 0.5)[c % 2], nus[c % 6]) for c in range(17)], masks)
        return X, None, UB, mass, Q
    S, UB, mass = _labels_columns(y, [nus[c % 6] for c in range(17)], masks)
    return X, S, UB, mass, None


@pytest.mark.parametrize('paired', [False, True], ids=['labels', 'paired'])
def test_one_box_per_column(amd, paired):
    """gamma = 1 / 3, max_iter = 60, tol = 1e-3 (LABELS: the columns stop at four or more different iterations) or 0.1 (PAIRED, whose
    columns converge more slowly: three stop at iteration 41 and leave the product, the others run to the cap).  Held-out rows stay exactly 0; every column follows the reference on its training
    rows' sub-matrix (status, iterations, f history to rtol 1e-9, x to 1e-9); r1, r2 and the counts are the reference's offsets
    evaluated on the device's own (x, g), compared with ==; and every column's x, g, records, r1 and r2 have the same bits solved
    alone, in the batch and in the reversed batch."""
    from optiml_amd.ml.svm.kernels import GaussianKernel
    from oracle import svm_oracle as so
    X, S, UB, mass, Q = _columns17(paired)
    n = X.shape[0]
    K = so.gram('rbf', X, gamma=1.0 / 3)
    quad = _quad(X, GaussianKernel(gamma=1.0 / 3))
    dev = quad.device_problem()
    sub = lambda A, rows: None if A is None else A[rows]   # noqa: E731
    tol = 0.1 if paired else 1e-3
    res = _solve(dev, S, UB, mass, Q, tol, 60)
    assert len({r['iter'] for r in res}) >= (2 if paired else 4)
    for c, r in enumerate(res):
        tr1 = UB[c][:n] > 0
        tr = np.concatenate((tr1, tr1)) if paired else tr1
        assert np.all(r['x'][~tr] == 0.)
        assert np.all(r['x'] >= 0) and np.all(r['x'] <= UB[c])
        sgn = None if paired else S[c][tr]
        ref = nur.solve(K[np.ix_(tr1, tr1)], UB[c][tr], tuple(mass[c]), sgn=sgn, q=None if Q is None else Q[c][tr], tol=tol,
                        max_iter=60)
        assert r['status'] == ref['status'] and r['iter'] == ref['iter'], (c, r['status'], r['iter'], ref['status'], ref['iter'])
        nur.assert_f_history(r['rows']['f'], ref)
        np.testing.assert_allclose(r['x'][tr], ref['x'], rtol=0, atol=1e-9)
        r1, r2, n_sv, n_free = nur.offsets(r['x'][tr], r['g'][tr], UB[c][tr], sgn)   # the reference's statements on the device's state
        assert (r['n_sv'], r['n_free']) == (n_sv, n_free)
        assert r['r1'] == r1 and r['r2'] == r2
    order = np.arange(17)[::-1]
    rev = _solve(dev, sub(S, order), UB[order], mass[order], sub(Q, order), tol, 60)
    for j, c in enumerate(order):
        assert _same_bits(rev[j], res[c]), c
    for c in range(17):
        one = slice(c, c + 1)
        alone = _solve(dev, sub(S, one), UB[one], mass[one], sub(Q, one), tol, 60)[0]
        assert _same_bits(alone, res[c]), c
    quad.release()


# ---- 4. the estimators against sklearn -------------------------------------------------------------------------------------------------
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


@pytest.mark.parametrize('tol', nur.TOLS)
@pytest.mark.parametrize('gamma', nur.GAMMAS)
def test_nu_svc_against_sklearn(amd, gamma, tol):
    """The host test's grid and conditions (test_nu_host.py) with the default max_iter, and: kkt_violation_ <= tol; the violation
    recomputed in NumPy from alphas_ is within tol + 1e-9; the history has n_iter_ + 1 entries."""
    from optiml_amd.ml.svm import NuSVC
    from optiml_amd.ml.svm.kernels import GaussianKernel
    from oracle import svm_oracle as so
    X, Xnew, yc, _ = nur.nu_data()
    n = len(yc)
    y = yc.astype(float)
    K = so.gram('rbf', X, gamma=gamma)
    lay = nur.Layout(n, y)
    for g, nu in nur.SVC_GRID:
        if g != gamma:
            continue
        ref = _sk_svc(gamma, nu)
        est = NuSVC(kernel=GaussianKernel(gamma=gamma), nu=nu, tol=tol).fit(X, yc)
        assert est.status_ == 'optimal' and est.n_iter_ <= 1000
        a, r = est.alphas_, est.margin_scale_
        assert a.shape == (n,) and a.min() >= 0 and a.max() <= 1 and r > 0
        for cls in (1, -1):
            assert abs(a[yc == cls].sum() - nu * n / 2) <= 1e-10 * nu * n / 2
        viol = nur.violation2(a, y * (K @ (y * a)), np.ones(n), lay)
        print('gamma=%g nu=%g tol=%g: %d iterations, r = %.3e, violation %.3e (device: %.3e)' % (gamma, nu, tol, est.n_iter_, r, viol,
                                                                                                  est.kkt_violation_))
        assert viol <= tol + 1e-9 and est.kkt_violation_ <= tol
        assert len(est.train_loss_history) == est.n_iter_ + 1
        assert np.array_equal(est.support_, np.flatnonzero(a > 0))
        assert np.array_equal(est.dual_coef_, (y * a)[a > 0] / r) and np.array_equal(est.classes_, [-1, 1])
        bound = 10 * tol / r
        for Z in (X, Xnew):
            dec, theirs = est.decision_function(Z), ref.decision_function(Z)
            print('    r |decision difference| / tol = %.2f' % (r * np.abs(dec - theirs).max() / tol))
            assert np.abs(dec - theirs).max() <= bound
            clear = np.abs(theirs) > bound
            assert np.array_equal(est.predict(Z)[clear], ref.predict(Z)[clear])
            if Z is X:
                assert (~clear).sum() <= 0.05 * n
        assert 0.5 <= est.score(X, yc) <= 1.0
        if tol == 1e-6:
            assert np.array_equal(est.support_, np.sort(ref.support_))


@pytest.mark.parametrize('tol', nur.TOLS)
@pytest.mark.parametrize('gamma', nur.GAMMAS)
def test_nu_svr_against_sklearn(amd, gamma, tol):
    """The host test's grid and conditions with max_iter = 3000 (the reference needs 1419), and the same three checks of the
    violation and the history."""
    from optiml_amd.ml.svm import NuSVR
    from optiml_amd.ml.svm.kernels import GaussianKernel
    from oracle import svm_oracle as so
    X, Xnew, _, yr = nur.nu_data()
    n = len(yr)
    K = so.gram('rbf', X, gamma=gamma)
    lay = nur.Layout(n)
    q = np.concatenate((-yr, yr))
    for g, C, nu in nur.SVR_GRID:
        if g != gamma:
            continue
        ref = _sk_svr(gamma, C, nu)
        est = NuSVR(kernel=GaussianKernel(gamma=gamma), C=C, nu=nu, tol=tol, max_iter=3000).fit(X, yr)
        assert est.status_ == 'optimal'
        x = est.alphas_
        assert x.shape == (2 * n,) and x.min() >= 0 and x.max() <= C
        for half in (x[:n], x[n:]):
            assert abs(half.sum() - C * nu * n / 2) <= 1e-10 * C * nu * n / 2
        assert not ((x[:n] > 0) & (x[n:] > 0)).any()
        viol = nur.violation2(x, q + lay.s * (K @ lay.fold(x))[lay.row], np.full(2 * n, C), lay)
        print('gamma=%g C=%g nu=%g tol=%g: %d iterations, violation %.3e (device: %.3e), epsilon %.4f' %
              (gamma, C, nu, tol, est.n_iter_, viol, est.kkt_violation_, est.epsilon_))
        assert viol <= tol + 1e-9 and est.kkt_violation_ <= tol
        assert len(est.train_loss_history) == est.n_iter_ + 1
        coef = x[:n] - x[n:]
        assert np.array_equal(est.support_, np.flatnonzero(coef != 0)) and np.array_equal(est.dual_coef_, coef[coef != 0])
        for Z in (X, Xnew):
            pred, theirs = est.predict(Z), ref.predict(Z)
            print('    |prediction difference| / tol = %.2f' % (np.abs(pred - theirs).max() / tol))
            assert np.abs(pred - theirs).max() <= 10 * tol
        assert est.epsilon_ > 0 and abs(est.score(X, yr) - ref.score(X, yr)) <= 1e-2


def test_string_gamma_and_stopped_fit(amd):
    from optiml_amd.ml.svm import NuSVC, NuSVR
    from optiml_amd.ml.svm._base import ConvergenceWarning
    from optiml_amd.ml.svm.kernels import GaussianKernel
    X, y, t = _data(257, 3)
    a = NuSVC(kernel=GaussianKernel(gamma='scale'), nu=0.5017).fit(X, y)
    g = 1.0 / (3 * X.var())
    b = NuSVC(kernel=GaussianKernel(gamma=g), nu=0.5017).fit(X, y)
    assert a.kernel_.gamma == g and a.kernel.gamma == 'scale'
    assert np.array_equal(a.alphas_, b.alphas_) and a.intercept_ == b.intercept_
    assert np.array_equal(a.decision_function(X[:40]), b.decision_function(X[:40]))
    with pytest.warns(ConvergenceWarning):
        est = NuSVR(kernel=GaussianKernel(gamma=1.0), nu=0.5017, tol=0.0, max_iter=5).fit(X, t)
    assert est.status_ == 'stopped' and est.n_iter_ == 5 and len(est.train_loss_history) == 6


# ---- 5. the paths ----------------------------------------------------------------------------------------------------------------------
def _same_fit(a, b):
    return (np.array_equal(a.alphas_, b.alphas_) and a.intercept_ == b.intercept_ and a.n_iter_ == b.n_iter_ and
            a.train_loss_history == b.train_loss_history and np.array_equal(a.dual_coef_, b.dual_coef_))


def test_nu_svc_path_equals_the_single_fits(amd):
    from optiml_amd.ml.svm import NuSVC, nu_svc_path
    from optiml_amd.ml.svm.kernels import GaussianKernel
    X, _, yc, _ = nur.nu_data()
    nus = [0.5017, 0.7017, 0.9017, 0.3517, 0.6017]
    kw = dict(kernel=GaussianKernel(gamma=0.125), tol=1e-4, max_iter=500)
    proto = NuSVC(**kw)
    path = nu_svc_path(proto, X, yc, nus)

    class Mine(NuSVC):
        pass
    sub = nu_svc_path(Mine(**kw), X, yc, nus[:2])
    assert all(type(e) is Mine for e in sub) and np.array_equal(sub[1].alphas_, path[1].alphas_)
    assert [e.nu for e in path] == nus and proto.nu == 0.5 and not hasattr(proto, 'alphas_')
    for est in path:
        one = NuSVC(nu=est.nu, **kw).fit(X, yc)
        assert est.status_ == 'optimal' and _same_fit(est, one) and est.margin_scale_ == one.margin_scale_
        assert np.array_equal(est.decision_function(X[:64]), one.decision_function(X[:64]))


def test_nu_svr_path_equals_the_single_fits(amd):
    from optiml_amd.ml.svm import NuSVR, nu_svr_path
    from optiml_amd.ml.svm.kernels import GaussianKernel
    X, _, _, yr = nur.nu_data()
    params = [(1.0, 0.2517), (1.0, 0.5017), (0.5, 0.8017), (0.5, 0.4017)]
    kw = dict(kernel=GaussianKernel(gamma=0.125), tol=1e-3, max_iter=1000)
    proto = NuSVR(**kw)
    path = nu_svr_path(proto, X, yr, params)

    class Mine(NuSVR):
        pass
    sub = nu_svr_path(Mine(**kw), X, yr, params[:2])
    assert all(type(e) is Mine for e in sub) and np.array_equal(sub[1].alphas_, path[1].alphas_)
    assert [(e.C, e.nu) for e in path] == params and (proto.C, proto.nu) == (1.0, 0.5) and not hasattr(proto, 'alphas_')
    for est in path:
        one = NuSVR(C=est.C, nu=est.nu, **kw).fit(X, yr)
        assert est.status_ == 'optimal' and _same_fit(est, one) and est.epsilon_ == one.epsilon_
        assert np.array_equal(est.predict(X[:64]), one.predict(X[:64]))


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals(amd):
    from optiml_amd import _lib
    from optiml_amd.opti import KernelQuadratic
    from optiml_amd.ml.svm import NuSVC, NuSVR
    from optiml_amd.ml.svm._batched import _DeviceSimplex2Solver
    from optiml_amd.ml.svm.kernels import GaussianKernel
    n = 257
    X, _, t = _data(n, 3)
    y = np.where(np.arange(n) % 2, 1., -1.)   # 128 rows of +1, 129 of -1
    u = np.ones((1, n))
    quad = _quad(X, GaussianKernel(gamma=1.0))
    dev = quad.device_problem()
    ok = _solve(dev, y[None, :], u, [[30.0, 30.0]], None, 1e-3, 5)[0]
    assert ok['iter'] >= 1
    half = np.where(y > 0, 30.0 / 128, 30.0 / 129)[None, :]   # inside its set
    assert _solve(dev, y[None, :], u, [[30.0, 30.0]], None, 1e-3, 5, x0=half)[0]['iter'] >= 1
    bad_s = y.copy()
    bad_s[5] = 0.5
    masked = u.copy()
    masked[0, y > 0] = 0.   # no row of positive box in the +1 group
    for S, UB, mass, x0 in ((bad_s[None, :], u, [[30.0, 30.0]], None),      # S not +-1
                            (y[None, :], u, [[128.5, 30.0]], None),         # a mass above its group's box
                            (y[None, :], u, [[0.0, 30.0]], None),
                            (y[None, :], masked, [[30.0, 30.0]], None),     # an empty group
                            (y[None, :], u, [[30.0, 30.0]], 2 * u),         # x0 outside its box
                            (y[None, :], u, [[30.0, 30.0]], half * 1.01),   # x0 off its masses
                            (y[None, :], -u, [[30.0, 30.0]], None)):
        with pytest.raises(_lib.BcqpError):
            _DeviceSimplex2Solver(dev, S, UB, mass, None, 1e-3, 10, x0)
    with pytest.raises(ValueError):   # PAIRED: UB must be k x 2n
        _DeviceSimplex2Solver(dev, None, u, [[30.0, 30.0]], None, 1e-3, 10)
    quad.release()
    svc = KernelQuadratic(X, -np.ones(n), 'svc', GaussianKernel(gamma=1.0), y=y)
    with pytest.raises(_lib.BcqpError):
        _DeviceSimplex2Solver(svc.device_problem(), y[None, :], u, [[30.0, 30.0]], None, 1e-3, 10)
    svc.release()
    with pytest.raises(ValueError, match='more than two labels'):
        NuSVC().fit(X, np.arange(n) % 3)
    with pytest.raises(ValueError, match='specified nu is infeasible'):
        NuSVC(nu=0.9).fit(X, np.where(np.arange(n) < 60, 1, -1))
    with pytest.raises(NotImplementedError):
        NuSVC(storage='stream').fit(X, y)
    with pytest.raises(NotImplementedError):
        NuSVR(storage='stream').fit(X, t)


# ---- 7. fp32 panels --------------------------------------------------------------------------------------------------------------------
def test_fp32_panel(amd):
    """The fp32 panel holds K rounded to fp32: one NuSVC and one NuSVR column follow the reference on the stored panel for 15
    iterations (f history to rtol 1e-9).  Against the f64 fit, both at tol 1e-7 so that the panel's rounding is what remains, the
    decision values agree to rtol 1e-4, atol 1e-5, the tolerance of the existing fp32-against-fp64 comparisons."""
    from optiml_amd.ml.svm import NuSVC, NuSVR
    from optiml_amd.ml.svm.kernels import GaussianKernel
    X, _, yc, yr = nur.nu_data()
    n = len(yc)
    y = yc.astype(float)
    quad = _quad(X, GaussianKernel(gamma=0.125), 'f32')
    K = quad.gram()
    dev = quad.device_problem()
    S, UB, mass = _labels_columns(y, [0.5017])
    r = _solve(dev, S, UB, mass, None, 0.0, 15)[0]
    ref = nur.solve(K, UB[0], tuple(mass[0]), sgn=y, tol=0.0, max_iter=15)
    assert r['status'] == ref['status'] and r['iter'] == ref['iter']
    nur.assert_f_history(r['rows']['f'], ref)
    UB, mass, Q = _paired_columns(yr, [(1.0, 0.5017)])
    r = _solve(dev, None, UB, mass, Q, 0.0, 15)[0]
    ref = nur.solve(K, UB[0], tuple(mass[0]), q=Q[0], tol=0.0, max_iter=15)
    assert r['status'] == ref['status'] and r['iter'] == ref['iter']
    nur.assert_f_history(r['rows']['f'], ref)
    quad.release()
    # (NuSVR at nu = 0.2517: the reference reaches tol 1e-7 in about 540 iterations there, and in over 3000 at nu = 0.5017)
    for make, target, nu in ((NuSVC, yc, 0.5017), (NuSVR, yr, 0.2517)):
        kw = dict(kernel=GaussianKernel(gamma=0.125), nu=nu, tol=1e-7, max_iter=3000)
        a = make(storage='f32', **kw).fit(X, target)
        b = make(**kw).fit(X, target)
        assert a.status_ == 'optimal' and b.status_ == 'optimal'
        da, db = a.decision_function(X), b.decision_function(X)
        print('%s fp32 panel against fp64: |decision difference| = %.2e' % (make.__name__, np.abs(da - db).max()))
        np.testing.assert_allclose(da, db, rtol=1e-4, atol=1e-5)
