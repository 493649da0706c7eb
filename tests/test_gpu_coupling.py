"""PairwiseCoupledSVC on the device: the coupling kernel (bq_couple.hip: couple_kernel) against the NumPy restatement of the same
statements (tests/coupling_reference.py), the held-out scoring of a pair solver (bq_msolver.hip: bq_msolver_pairs_heldout,
mpairs_heldout_kernel) against the host path, and the estimator against its own loop path and against `OneVsOneSVC`.

The bounds.  The coupling is specified by its order of operations (no fused multiply-add, sequential sums, IEEE division), so the
device's probabilities and sweep counts are compared with the restatement BIT FOR BIT, on the clipped pair probabilities the device
itself returns (R): no tolerance.  R differs from NumPy's sigmoid by the two exps; the estimator's batched path differs from its
loop path by the decision values (another product kernel, DECISION_RTOL) and what the sigmoid fits and the coupling make of that.
Those deviations were measured on an MI355X (profiles/coupling/parity.json) and the bounds are 16 times the figures
(coupling_reference.SIGMOID_RTOL, AB_RTOL, PROBA_RTOL).
"""
import functools

import numpy as np
import pytest

import coupling_reference as cr
import platt_reference as pr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def amd():
    from optiml_amd import _lib
    from optiml_amd.device import get_context
    _lib.load()
    get_context()


def rel_dev(got, want):
    got, want = np.asarray(got, dtype=float), np.asarray(want, dtype=float)
    return float(np.max(np.abs(got - want) / np.abs(want)))


# ---- the coupling kernel -----------------------------------------------------------------------------------------------------------
def couple(S, k):
    """the device's (prob, iters, R) for target pair probabilities S, through A = -1, B = 0 and F = log(s / (1 - s))"""
    from optiml_amd.ml.svm.coupling import pairwise_coupling
    P = k * (k - 1) // 2
    return pairwise_coupling(cr.decision_values(S), -np.ones(P), np.zeros(P), k)


def coupling_case(family, k, t):
    """One (family, k, t) case: the exact assertions, and the deviation of R from NumPy's sigmoid"""
    S = cr.target_probabilities(family, k, t)
    prob, iters, R = couple(S, k)
    assert prob.shape == (t, k) and iters.shape == (t,) and R.shape == S.shape
    assert R.min() >= cr.CLIP and R.max() <= 1. - cr.CLIP
    want, want_iters, margin = cr.couple_rows(R, k)
    diff = np.flatnonzero((prob != want).any(axis=1) | (iters != want_iters))
    print('%s k=%d t=%d: sweeps %d to %d, points that differ %d, smallest stop margin %.3g' % (
        family, k, t, iters.min(), iters.max(), len(diff), margin.min()))
    assert np.array_equal(iters, want_iters), (family, k, t, diff[:5])
    assert np.array_equal(prob, want), (family, k, t, diff[:5], rel_dev(prob, want))
    assert iters.max() < max(100, k)
    np.testing.assert_allclose(prob.sum(axis=1), 1., rtol=0, atol=1e-14)
    if family == 'half':
        assert np.array_equal(R, S) and not iters.any() and np.array_equal(prob, np.full((t, k), 1. / k))
    if family == 'clipped':
        assert np.array_equal(R, S)
    if family == 'dominant':
        assert (prob.max(axis=1) > 1.5 / k).all()
    return rel_dev(R, cr.sigmoid(cr.decision_values(S), -1., 0.))


@pytest.mark.parametrize('family', cr.FAMILIES)
@pytest.mark.parametrize('k', cr.CLASSES)
def test_coupling_equals_the_restatement_bit_for_bit(amd, k, family):
    """t = 1, 63, 64, 65, 257 points of every family and class count: `prob` and `iters` equal `couple_rows(R)`; R against NumPy's
    sigmoid at 16 times the measured deviation."""
    dev = max(coupling_case(family, k, t) for t in cr.POINTS)
    print('%s k=%d: sigmoid deviation %.3e (bound %.3e)' % (family, k, dev, cr.SIGMOID_RTOL))
    assert dev <= cr.SIGMOID_RTOL


@pytest.mark.parametrize('k', [3, 33, 64])
def test_coupling_is_batch_invariant(amd, k):
    """A point alone, first, in the middle and last of a batch of other points: identical bits."""
    S = cr.target_probabilities('uniform', k, 65, seed=1)
    other = cr.target_probabilities('dominant', k, 65, seed=2)
    prob, iters, R = couple(S, k)
    for i in (0, 31, 64):
        alone = couple(S[i:i + 1], k)
        assert np.array_equal(alone[0][0], prob[i]) and alone[1][0] == iters[i] and np.array_equal(alone[2][0], R[i])
        for pos in (0, 40, 64):
            mixed = other.copy()
            mixed[pos] = S[i]
            got = couple(mixed, k)
            assert np.array_equal(got[0][pos], prob[i]) and got[1][pos] == iters[i] and np.array_equal(got[2][pos], R[i])


def test_the_sigmoid_takes_a_and_b(amd):
    """R is the clipped 1 / (1 + exp(f A + B)) of column q's own A and B, on both branches and at both clips"""
    from optiml_amd.ml.svm.coupling import pairwise_coupling
    rng = np.random.default_rng(5)
    F = rng.standard_normal((40, 6)) * 3
    F[0], F[1] = 500., -500.
    A, B = np.array([-2., -1., -0.5, 0.7, -3., -1.5]), np.array([0.3, -0.2, 0., 1., -1., 0.1])
    prob, _, R = pairwise_coupling(F, A, B, 4)
    want = cr.sigmoid(F, A, B)
    dev = rel_dev(R, want)
    print('sigmoid deviation %.3e (bound %.3e)' % (dev, cr.SIGMOID_RTOL))
    assert dev <= cr.SIGMOID_RTOL
    assert set(np.unique(R[:2])) == {cr.CLIP, 1. - cr.CLIP}
    assert np.array_equal(prob, cr.couple_rows(R, 4)[0])


# ---- bq_msolver_pairs_heldout ------------------------------------------------------------------------------------------------------
SIZES, GAMMA = (300, 257, 40), 0.1


PAIR_SEED = 21


@functools.lru_cache(maxsize=None)
def _pair_data(seed=PAIR_SEED):
    """Class sizes (300, 257, 40): tiles 2, 2, 1 with ghost rows in every class; 5 features, overlapping classes; 3 folds.
    Computed once and shared by the tests, which leave it unchanged.  (The seed: test_pairs_heldout_against_the_host_path.)"""
    from optiml_amd.ml.svm.coupling import coupling_columns
    from optiml_amd.ml.svm.model_selection import check_cv_splits
    rng = np.random.default_rng(seed)
    codes = rng.permutation(np.repeat(np.arange(3), SIZES))
    X = rng.standard_normal((len(codes), 5)) + 0.9 * rng.standard_normal((3, 5))[codes]
    splits = check_cv_splits(3, X, codes)
    plan = coupling_columns(codes, 3, splits, 1.0)
    Xp = np.zeros((plan['n_pad'], 5))
    Xp[plan['index']] = X
    return X, codes, splits, plan, Xp


def _quad(Xp):
    from optiml_amd.opti import KernelQuadratic
    from optiml_amd.ml.svm.kernels import GaussianKernel
    return KernelQuadratic(Xp, -np.ones(len(Xp)), 'svc', GaussianKernel(gamma=GAMMA), y=np.ones(len(Xp)))


def _solve_pairs(dev, kind, plan, sel, cal_of, ncal, max_iter=100):
    """the columns `sel` of the plan on one pair solver: (results, [heldout_pairs twice])"""
    from optiml_amd import _lib
    from optiml_amd.ml.svm._batched import solve_batched
    from optiml_amd.ml.svm.onevsone import _DevicePairSolver
    kind = _lib.PG if kind == 'pg' else _lib.FW
    Y, UB = plan['Y'][sel], plan['UB'][sel]
    chunk = [plan['pairs'][plan['cols'][c][0]] for c in sel]
    held = []

    def score(solver, _):
        for _ in range(2):
            held.append(solver.heldout_pairs(plan['data_row'], cal_of, ncal, decisions=True))

    solver = _DevicePairSolver(dev, kind, plan['cls_tiles'], chunk, Y, UB, 1e-6, max_iter)
    res = solve_batched(dev, kind, Y, UB, max_iter=max_iter, solver=solver, before_close=score)
    return res, held


@functools.lru_cache(maxsize=None)
def heldout_run(kind, seed=None):
    """The 12 columns (pair, fold) and (pair, all) of three classes on one pair solver, scored twice; the host path's product of
    the same (repeated) pairs; column 5 solved alone.  Run once per optimizer and shared."""
    from optiml_amd.ml.svm._batched import gram_matmat_pairs
    from optiml_amd.ml.svm.coupling import chunk_calibrators
    X, codes, splits, plan, Xp = _pair_data() if seed is None else _pair_data(seed)
    quad = _quad(Xp)
    dev = quad.device_problem()
    cal_of, _ = chunk_calibrators(plan['cols'])
    res, (first, second) = _solve_pairs(dev, kind, plan, list(range(12)), cal_of, 3)
    W, svs = np.zeros((12, plan['n_pad'])), []
    for j, r in enumerate(res):
        sv = r['x'] > 1e-6
        W[j][sv] = r['x'][sv] * plan['Y'][j][sv]
        svs.append(sv)
    U = gram_matmat_pairs(dev, plan['cls_tiles'], [plan['pairs'][p] for p, _ in plan['cols']], W)
    # column 5 = (pair (0, 2), fold 1), whose pair the batch names four times, solved alone
    alone, (held, _) = _solve_pairs(dev, kind, plan, [5], np.array([0]), 1)
    quad.release()
    return dict(plan=plan, res=res, first=first, second=second, svs=svs, U=U, alone=alone[0], alone_held=held)


def heldout_labels(plan):
    """3 x n_pad: +-1 on the data rows of each pair's two classes (every one is held out by exactly one fold column), 0 elsewhere"""
    pcode, data = plan['pcode'], plan['data_row'] > 0
    return np.stack([np.where(pcode == b, 1., np.where(pcode == a, -1., 0.)) * data for a, b in plan['pairs']])


def heldout_platt_deviation(kind, seed=None):
    """The device's sigmoids of the held-out buffers against the NumPy reference on the same buffers: per pair (reference record,
    device iters, relative deviation of A, of B)"""
    run = heldout_run(kind, seed)
    fit, labels = run['first'][2], heldout_labels(run['plan'])
    out = []
    for p in range(3):
        ref = pr.platt_reference(fit['dec'][p], labels[p])
        out.append((ref, int(fit['iters'][p]), rel_dev(fit['A'][p], ref['A']), rel_dev(fit['B'][p], ref['B'])))
    return out


@pytest.mark.parametrize('kind', ['pg', 'fw'])
def test_pairs_heldout_against_the_host_path(amd, kind):
    """Per column the support count exactly and the intercept against `intercept(Y, U, sv)` on the downloaded x and one routed
    product, at rtol 1e-12; the decision buffer against U + b on the held-out rows at the same rtol and an atol of 1e-12 |b|
    (test_gpu_calibration.py's tolerances and their reasons), and exactly 0 on ghost rows, rows of other classes and training rows;
    the label buffer through the calibrators' counts, which are those of the held-out rows exactly; the sigmoids against
    bq_platt_fit on the downloaded buffer bit for bit (the same kernel on the same bits) and against the NumPy reference at
    PLATT_RTOL; a second call gives the same bits, and a column solved alone the bits it has in the batch.

    The reference comparison has test_gpu_calibration.py's preconditions (no stop test decided by less than a factor 1.1, no
    line-search test by a hair) and one more: no pair's B is a cancellation residue (|B| >= 0.1; its start value is
    log((N- + 1) / (N+ + 1)), 0.15 to 2 here).  PLATT_RTOL is a relative bound, and a B that the iteration drives to nearly 0 keeps
    the absolute rounding of its terms: on an earlier draw of the features pair (0, 1) ended at B = -0.0146 and deviated by 1.0e-16
    absolute, 7.0e-15 of itself, against PLATT_RTOL = 5.5e-15.  The features' seed is the first of 20, 21, ... at which both
    optimizers meet the preconditions, which are properties of the reference alone (of 20 to 35 the seeds 21, 22 and 26 do; 11 of the
    others fail on |B|, two on a stop ratio)."""
    from optiml_amd.ml.svm._batched import intercept, platt_fit
    run = heldout_run(kind)
    plan, res, first, second, svs, U = (run[key] for key in ('plan', 'res', 'first', 'second', 'svs', 'U'))
    n_pad, data, pcode = plan['n_pad'], plan['data_row'] > 0, plan['pcode']
    assert all(0 < r['iter'] <= 100 for r in res)
    for a, b in zip(first[:2], second[:2]):
        assert np.array_equal(a, b)
    for key in first[2]:
        assert np.array_equal(first[2][key], second[2][key]), key
    b_dev, n_sv, fit = first
    Y, UB = plan['Y'], plan['UB']
    got, labels = fit['dec'], np.zeros((3, n_pad))
    for j, (p, f) in enumerate(plan['cols']):
        assert np.all(res[j]['x'][UB[j] == 0] == 0.)
        assert n_sv[j] == svs[j].sum() > 0
        b = intercept(Y[j], U[j], svs[j])
        np.testing.assert_allclose(b_dev[j], b, rtol=1e-12)
        if f is None:
            continue
        a_cls, b_cls = plan['pairs'][p]
        te = ((pcode == a_cls) | (pcode == b_cls)) & data & (UB[j] == 0)
        assert te.sum() > 0 and not labels[p][te].any()
        np.testing.assert_allclose(got[p][te], U[j][te] + b, rtol=1e-12, atol=1e-12 * abs(b))
        labels[p][te] = Y[j][te]
    assert np.array_equal(labels, heldout_labels(plan))
    assert np.array_equal(got != 0, labels != 0)   # 0 on ghost rows, on the rows of the third class and nowhere else
    for p, (a_cls, b_cls) in enumerate(plan['pairs']):
        assert not got[p][~data].any() and not got[p][(pcode != a_cls) & (pcode != b_cls)].any()
        assert fit['n_pos'][p] == (labels[p] > 0).sum() == SIZES[b_cls] and fit['n_neg'][p] == (labels[p] < 0).sum() == SIZES[a_cls]
    again = platt_fit(got, labels)
    for key in again:
        assert np.array_equal(again[key], fit[key]), key
    assert not fit['flags'].any() and (fit['iters'] > 0).all()
    for p, (ref, iters, dev_a, dev_b) in enumerate(heldout_platt_deviation(kind)):
        print('pair %d: iters %d / %d, A %.17g (deviation %.3e), B %.17g (deviation %.3e), stop ratio %.3g, search margin %.3g' % (
            p, iters, ref['iters'], ref['A'], dev_a, ref['B'], dev_b, ref['stop_ratio'], ref['search_margin']))
        assert ref['flags'] == 0 and ref['stop_ratio'] < 1 / 1.1 and ref['search_margin'] > pr.SEARCH_MARGIN
        assert abs(ref['B']) >= 0.1
        assert iters == ref['iters']
        assert dev_a <= pr.PLATT_RTOL and dev_b <= pr.PLATT_RTOL
    alone, held = run['alone'], run['alone_held']
    assert np.array_equal(alone['x'], res[5]['x']) and alone['iter'] == res[5]['iter']
    assert held[0][0] == b_dev[5] and held[1][0] == n_sv[5]
    te = labels[1] * (UB[5] == 0) != 0
    assert np.array_equal(held[2]['dec'][0][te], got[1][te]) and not held[2]['dec'][0][~te].any()


def test_pairs_heldout_argument_checks(amd):
    from optiml_amd import _lib
    from optiml_amd.ml.svm._batched import _DeviceMultiSolver
    from optiml_amd.ml.svm.onevsone import _DevicePairSolver
    X, codes, splits, plan, Xp = _pair_data()
    quad = _quad(Xp)
    dev = quad.device_problem()
    Y, UB = plan['Y'][:4], plan['UB'][:4]
    boxes = _DeviceMultiSolver(dev, _lib.PG, Y, UB, 1e-6, 10)   # bq_msolver_create_boxes: a solver of another kind
    boxes.run(3)
    with pytest.raises(_lib.BcqpError) as e:
        boxes.heldout_pairs(plan['data_row'], np.array([0, 0, 0, -1]), 1)
    assert e.value.code == _lib.ERR_BADARG and 'create_pairs' in str(e.value)
    boxes.close()
    pairs = _DevicePairSolver(dev, _lib.PG, plan['cls_tiles'], [(0, 1)] * 4, Y, UB, 1e-6, 10)
    pairs.run(3)
    pairs.heldout_pairs(plan['data_row'], np.array([0, 0, 0, -1]), 1)
    with pytest.raises(_lib.BcqpError) as e:
        pairs.heldout_svc(np.array([0, 0, 0, -1]), 1)   # and the boxes' entry refuses a pair solver
    assert e.value.code == _lib.ERR_BADARG
    for cal_of, ncal in ((np.array([0, 0, 0, 1]), 1), (np.array([0, 0, -2, -1]), 1), (np.array([0, 0, 0, -1]), 0)):
        with pytest.raises(_lib.BcqpError) as e:
            pairs.heldout_pairs(plan['data_row'], cal_of, ncal)
        assert e.value.code == _lib.ERR_BADARG
    pairs.close()
    UB2 = UB.copy()
    UB2[1][np.flatnonzero((UB[0] == 0) & (plan['data_row'] > 0) & (plan['pcode'] < 2))[:3]] = 0.   # columns 0 and 1 now share 3 held-out rows
    pairs = _DevicePairSolver(dev, _lib.PG, plan['cls_tiles'], [(0, 1)] * 4, Y, UB2, 1e-6, 10)
    pairs.run(3)
    with pytest.raises(_lib.BcqpError) as e:
        pairs.heldout_pairs(plan['data_row'], np.array([0, 0, 0, -1]), 1)
    assert e.value.code == _lib.ERR_BADARG and 'disjoint' in str(e.value)
    pairs.heldout_pairs(plan['data_row'], np.array([0, 1, 2, -1]), 3)   # a calibrator each: fine (every column has ub = 0 on the ghost rows)
    pairs.close()
    quad.release()


def test_pairs_heldout_leaves_the_solver_running(amd):
    """A scoring call between two runs: the product it takes has every pair live, and the run after it continues with the bits of an
    uninterrupted run (columns 0 to 7: two pairs, a pair named four times)."""
    from optiml_amd import _lib
    from optiml_amd.ml.svm.onevsone import _DevicePairSolver
    X, codes, splits, plan, Xp = _pair_data()
    quad = _quad(Xp)
    dev = quad.device_problem()
    Y, UB = plan['Y'][:8], plan['UB'][:8]
    chunk = [plan['pairs'][p] for p, _ in plan['cols'][:8]]
    cal_of = np.array([0, 0, 0, -1, 1, 1, 1, -1])
    xs = []
    for cut in (None, 15):
        solver = _DevicePairSolver(dev, _lib.PG, plan['cls_tiles'], chunk, Y, UB, 1e-6, 40)
        if cut:
            solver.heldout_pairs(plan['data_row'], cal_of, 2)   # before the first run: x = 0, no support vector, NaN intercepts
            solver.run(cut)
            b, n_sv, _ = solver.heldout_pairs(plan['data_row'], cal_of, 2)
            assert (n_sv > 0).all() and np.isfinite(b).all()
            solver.run(40 - cut)
        else:
            solver.run(40)
        xs.append([solver.get(c, _lib.GET_X_NOW) for c in range(8)])
        assert all(solver.state(c)[0] == 40 for c in range(8))
        solver.close()
    for a, b in zip(*xs):
        assert np.array_equal(a, b) and a.any()
    quad.release()


# ---- PairwiseCoupledSVC end to end -------------------------------------------------------------------------------------------------
def _svc_kw(kind, **kw):
    from optiml_amd.ml.svm.kernels import GaussianKernel
    from optiml_amd.ml.svm.losses import hinge
    from optiml_amd.opti.constrained import FrankWolfe, ProjectedGradient
    base = dict(loss=hinge, dual=True, reg_intercept=True, optimizer=ProjectedGradient if kind == 'pg' else FrankWolfe,
                kernel=GaussianKernel(gamma=GAMMA), C=1, max_iter=100)
    base.update(kw)
    return base


@functools.lru_cache(maxsize=None)
def _data(classes):
    """n about 500 rows of 5 features in `classes` overlapping classes with labels that are neither codes nor +-1, and 50 further
    rows to predict on.  Shared and left unchanged."""
    sizes = {2: (260, 240), 3: (200, 170, 130), 4: (150, 130, 120, 100)}[classes]
    rng = np.random.default_rng(31 + classes)
    codes = rng.permutation(np.repeat(np.arange(classes), sizes))
    centres = 1.1 * rng.standard_normal((classes, 5))
    X = rng.standard_normal((len(codes), 5)) + centres[codes]
    new = rng.integers(0, classes, 50)
    return X, 2 * codes + 3, rng.standard_normal((50, 5)) + centres[new]


@functools.lru_cache(maxsize=None)
def fitted(classes, kind):
    """(batched estimator, the loop path of the same class, OneVsOneSVC.fit), fitted once per configuration and shared"""
    from optiml_amd.ml.svm import OneVsOneSVC, PairwiseCoupledSVC
    from optiml_amd.ml.svm import coupling
    X, y, _ = _data(classes)
    est = PairwiseCoupledSVC(OneVsOneSVC(**_svc_kw(kind)), cv=3).fit(X, y)
    assert est.batched_ is True
    with pytest.MonkeyPatch.context() as mp:   # the way test_gpu_ovo.py reaches its fallback
        mp.setattr(coupling, 'uses_batched_coupling', lambda estimator, world: False)
        loop = PairwiseCoupledSVC(OneVsOneSVC(**_svc_kw(kind)), cv=3).fit(X, y)
    assert loop.batched_ is False
    return est, loop, OneVsOneSVC(**_svc_kw(kind)).fit(X, y)


def estimator_deviations(classes, kind):
    """(deviation of probA_ / probB_, deviation of predict_proba on the 50 fresh rows) of the batched path from the loop path"""
    est, loop, _ = fitted(classes, kind)
    Xnew = _data(classes)[2]
    ab = max(rel_dev(est.probA_, loop.probA_), rel_dev(est.probB_, loop.probB_))
    return ab, rel_dev(est.predict_proba(Xnew), loop.predict_proba(Xnew))


@pytest.mark.parametrize('kind', ['pg', 'fw'])
@pytest.mark.parametrize('classes', [3, 4])
def test_the_estimator_equals_one_vs_one_and_its_own_loop(amd, classes, kind):
    """The (pair, all) columns are `OneVsOneSVC.fit`'s: the same alphas bit for bit (the pair solver is batch-invariant and the
    columns are OneVsOneSVC's own).  The sigmoids and the probabilities of 50 fresh rows against the loop path of the same class
    (per pair and fold SVC.fit and decision_function, the sigmoids through bq_platt_fit, the coupling through
    bq_pairwise_coupling), at 16 times the deviations measured on an MI355X (profiles/coupling/parity.json).  The sigmoids' share of
    the probabilities' bound is PLATT_RTOL + DECISION_RTOL, as in test_gpu_calibration.py; the coupling divides by Q[t][t] and
    renormalises, which spreads a pair's deviation over the classes, so the probabilities' own figure is the one that is used."""
    est, loop, ovo = fitted(classes, kind)
    X, y, Xnew = _data(classes)
    P = classes * (classes - 1) // 2
    assert est.batched_decision_ is True and est.estimator_.batched_ is True and len(est.estimator_.estimators_) == P
    for mine, theirs in zip(est.estimator_.estimators_, ovo.estimators_):
        assert np.array_equal(mine.alphas_, theirs.alphas_)
        assert np.array_equal(mine.support_, theirs.support_)
        np.testing.assert_allclose(mine.intercept_, theirs.intercept_, rtol=1e-12)
    np.testing.assert_allclose(est.decision_function(Xnew), ovo.decision_function(Xnew), rtol=pr.DECISION_RTOL, atol=0)
    assert est.n_iter_.shape == est.status_.shape == loop.n_iter_.shape == (P, 4) and (est.n_iter_ > 0).all()
    assert list(est.n_iter_[:, 3]) == [e.optimizer.iter for e in ovo.estimators_]
    assert list(est.status_[:, 3]) == [e.optimizer.status for e in ovo.estimators_]
    assert est.oof_decision_.shape == (len(y), P)
    codes = np.searchsorted(est.classes_, y)
    for p, (a, b) in enumerate(cr.pairs(classes)):
        inpair = (codes == a) | (codes == b)
        assert np.array_equal(est.oof_decision_[:, p] != 0, inpair)
    dev_oof = np.abs(est.oof_decision_ - loop.oof_decision_).max() / np.abs(loop.oof_decision_).max()
    ab, proba = estimator_deviations(classes, kind)
    print('classes %d %s: oof decision deviation %.3e (bound %.3e), A / B deviation %.3e (bound %.3e), probability deviation %.3e '
          '(bound %.3e)' % (classes, kind, dev_oof, pr.DECISION_RTOL, ab, cr.AB_RTOL, proba, cr.PROBA_RTOL))
    assert dev_oof <= pr.DECISION_RTOL
    assert np.array_equal(est.calibrators_['iters'], loop.calibrators_['iters']) and not est.calibrators_['flags'].any()
    assert np.array_equal(est.calibrators_['n_pos'], loop.calibrators_['n_pos'])
    assert ab <= cr.AB_RTOL
    assert proba <= cr.PROBA_RTOL
    got = est.predict_proba(Xnew)
    assert got.shape == (50, classes) and np.array_equal(est.classes_, np.unique(y))
    np.testing.assert_allclose(got.sum(axis=1), 1., rtol=0, atol=1e-14)
    assert np.array_equal(est.predict(Xnew), est.classes_[np.argmax(got, axis=1)])


@pytest.mark.parametrize('classes', [3, 4])
def test_the_fused_pass_equals_coupling_the_pair_decisions(amd, classes):
    """predict_proba (bq_decision_coupled: the decision values coupled where they lie) against `pairwise_coupling` on
    `estimator_`'s own pair decisions brought to the host, on the points whose stop tests are decided clearly."""
    from optiml_amd.ml.svm.coupling import pairwise_coupling
    est, _, _ = fitted(classes, 'pg')
    Xnew = np.vstack([_data(classes)[2]] * 6)[:257]   # more than two test tiles
    F = est.pair_decisions(Xnew)
    want, iters, R = pairwise_coupling(F, est.probA_, est.probB_, classes)
    safe = cr.couple_rows(R, classes)[2] > cr.SAFE_MARGIN
    assert safe.mean() >= cr.SAFE_SHARE
    got = est.predict_proba(Xnew)
    print('classes %d: deviation %.3e, sweeps %d to %d' % (classes, rel_dev(got[safe], want[safe]), iters.min(), iters.max()))
    np.testing.assert_allclose(got[safe], want[safe], rtol=pr.DECISION_RTOL, atol=0)
    assert np.array_equal(got[:50], got[50:100])   # a point's bits do not depend on its place


def test_the_fused_call_s_optional_outputs_over_several_chunks(amd, monkeypatch):
    """bq_decision_coupled with iters, R and dec, on 257 test points cut into chunks of 128 (hook decision_multi_chunk_rows): dec has
    bq_decision_function_multi's bits, and prob, iters and R are those of bq_pairwise_coupling on dec, bit for bit — every chunk's
    points land at their own rows of the three outputs; the chunking changes no bit."""
    from conftest import set_hooks
    from optiml_amd.ml.svm.coupling import coupled_decision, pairwise_coupling
    est, _, _ = fitted(4, 'pg')
    batch = est.estimator_.decision_batch_
    rng = np.random.default_rng(9)
    Xnew = np.vstack([_data(4)[2]] * 6)[:257] + 0.05 * rng.standard_normal((257, 5))   # 257 different points
    set_hooks(monkeypatch, decision_multi_unit=None, decision_multi_chunk_rows=None)
    whole = coupled_decision(batch, Xnew, est.probA_, est.probB_, 4, details=True)
    F = batch(Xnew)
    set_hooks(monkeypatch, decision_multi_chunk_rows=128)
    prob, iters, R, dec = coupled_decision(batch, Xnew, est.probA_, est.probB_, 4, details=True)
    assert dec.shape == (257, 6) and np.array_equal(dec, F)
    want = pairwise_coupling(F, est.probA_, est.probB_, 4)
    for got, ref, one in zip((prob, iters, R), want, whole[:3]):
        assert np.array_equal(got, ref) and np.array_equal(got, one)
    assert np.array_equal(whole[3], F) and len(np.unique(prob[:, 0])) > 200
    assert np.array_equal(coupled_decision(batch, Xnew, est.probA_, est.probB_, 4), prob)   # and without them
    set_hooks(monkeypatch, decision_multi_chunk_rows=None)
    assert est.predict_proba(Xnew[:0]).shape == (0, 4)
    with pytest.raises(ValueError):
        pairwise_coupling(np.zeros((3, 12)), est.probA_, est.probB_, 4)   # t x 2P is not 2t points


@pytest.mark.parametrize('cut', [5, 3])
def test_a_pair_s_folds_spread_over_several_solves(amd, monkeypatch, cut):
    """`pair_chunks` forced to solves of `cut` columns, which cut inside a pair's four columns: the held-out rows of a pair are
    gathered from its solves and the sigmoids fitted by bq_platt_fit on them.  The solver and the Platt kernel are batch-invariant,
    so everything equals the single-solve fit bit for bit."""
    from optiml_amd.ml.svm import OneVsOneSVC, PairwiseCoupledSVC
    from optiml_amd.ml.svm import coupling
    one, _, _ = fitted(3, 'pg')
    X, y, Xnew = _data(3)
    solves = []

    def chunks(pairs, cls_tiles, n_pad, free_bytes):
        out = [pairs[i:i + cut] for i in range(0, len(pairs), cut)]
        solves.append(len(out))
        return out

    monkeypatch.setattr(coupling, 'pair_chunks', chunks)
    est = PairwiseCoupledSVC(OneVsOneSVC(**_svc_kw('pg')), cv=3).fit(X, y)
    assert est.batched_ is True and solves == [-(-12 // cut)]
    for key in ('A', 'B', 'iters', 'loss', 'flags', 'n_pos', 'n_neg'):
        assert np.array_equal(est.calibrators_[key], one.calibrators_[key]), key
    assert np.array_equal(est.oof_decision_, one.oof_decision_)
    assert np.array_equal(est.n_iter_, one.n_iter_) and np.array_equal(est.status_, one.status_)
    for mine, theirs in zip(est.estimator_.estimators_, one.estimator_.estimators_):
        assert np.array_equal(mine.alphas_, theirs.alphas_) and mine.intercept_ == theirs.intercept_
    assert np.array_equal(est.predict_proba(Xnew), one.predict_proba(Xnew))


def test_two_classes(amd):
    """One pair: no fused pass (it needs two columns); the coupling of one pair is that pair, p = (1 - s, s) within the sweeps' stop
    tolerance, and predict is the argmax."""
    from optiml_amd.ml.svm import OneVsOneSVC, PairwiseCoupledSVC
    X, y, Xnew = _data(2)
    est = PairwiseCoupledSVC(OneVsOneSVC(**_svc_kw('pg')), cv=3).fit(X, y)
    assert est.batched_ is True and est.batched_decision_ is False and est.probA_.shape == (1,) and est.n_iter_.shape == (1, 4)
    P = est.predict_proba(Xnew)
    s = cr.sigmoid(est.pair_decisions(Xnew)[:, 0], est.probA_[0], est.probB_[0])
    np.testing.assert_allclose(P[:, 1], s, rtol=0, atol=0.005 / 2)
    np.testing.assert_allclose(P.sum(axis=1), 1., rtol=0, atol=1e-14)
    assert np.array_equal(est.predict(Xnew), est.classes_[np.argmax(P, axis=1)])
    assert (est.predict(X) == y).mean() > 0.8


def test_a_laplacian_kernel_takes_the_per_estimator_decisions(amd):
    from optiml_amd.ml.svm import OneVsOneSVC, PairwiseCoupledSVC
    from optiml_amd.ml.svm.kernels import LaplacianKernel
    X, y, Xnew = _data(3)
    est = PairwiseCoupledSVC(OneVsOneSVC(**_svc_kw('pg', kernel=LaplacianKernel(gamma=GAMMA))), cv=3).fit(X, y)
    assert est.batched_ is True and est.batched_decision_ is False
    P = est.predict_proba(Xnew)
    assert P.shape == (50, 3) and (P > 0).all()
    np.testing.assert_allclose(P.sum(axis=1), 1., rtol=0, atol=1e-14)
    assert np.array_equal(est.predict(Xnew), est.classes_[np.argmax(P, axis=1)])
    assert (est.predict(X) == y).mean() > 0.6
