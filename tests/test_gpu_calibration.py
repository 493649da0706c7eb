"""CalibratedSVC on the device: the batched Platt fit (bq_platt.hip: platt_fit_kernel) against the NumPy reference of the same
iteration (tests/platt_reference.py), the held-out decision values and sigmoids taken from a one-box-per-column solver's state
(bq_msolver.hip: bq_msolver_svc_heldout, msvc_coef_kernel, msvc_heldout_kernel) against the host path, and the estimator against the
loop it replaces, written out with the project's own single fits.

The bounds.  Device and reference run the same iteration on the same inputs and differ in the order of their sums and in exp /
log1p, so they take the same number of Newton steps wherever no stop test and no line-search test is decided by a hair — which
the tests assert on the reference first — and A, B and the loss then differ by rounding times the conditioning of the 2 x 2
Hessians.  The largest relative deviation over every input of this file was measured on an MI355X
(profiles/calibration/platt_parity.json: `platt_max_rel_dev`); the bound is 16 times that figure (`platt_reference.PLATT_RTOL`),
the headroom being for another compiler's exp / log1p.

The line search: none of the issue's inputs halves a step; a search of 2000 seeds of a bimodal family with a few mislabelled
extremes (`platt_reference.backtracking_candidate`) finds 47 that do, and two of them, where the reference halves twice and every
test is decided clearly, are compared like the others (`BACKTRACK_SEEDS`).
"""
import ctypes as C
import functools

import numpy as np
import pytest

import platt_reference as pr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def amd():
    from optiml_amd import _lib
    from optiml_amd.device import get_context
    _lib.load()
    get_context()


def platt_inputs():
    """(name, f, labels) of every input the Platt kernel is compared on"""
    out = [('noisy-%d' % n,) + pr.noisy_input(n) for n in pr.NOISY_N]
    out += [(c,) + pr.edge_input(c) for c in pr.EDGE_CASES]
    out += [('masked',) + pr.masked_input()]
    out += [('backtrack-%d' % s,) + pr.backtracking_candidate(s) for s in pr.BACKTRACK_SEEDS]
    return out


def rel_dev(got, want):
    return 0. if got == want else abs(got - want) / abs(want)


def platt_deviation(name, f, y):
    """The device fit of one input against the reference: the exact figures are asserted, the largest relative deviation of A, B
    and the loss is returned."""
    from optiml_amd.ml.svm._batched import platt_fit
    ref = pr.platt_reference(f, y)
    # the precondition of equal iteration counts: no stop test decided by less than a factor 1.1, no line-search test by a hair
    assert ref['stop_ratio'] < 1 / 1.1, (name, ref['stop_ratio'])
    assert ref['search_margin'] > pr.SEARCH_MARGIN, (name, ref['search_margin'])
    fit = platt_fit(f, y)
    got = {key: fit[key][0] for key in fit}
    dev = max(rel_dev(float(got[key]), ref[key]) for key in ('A', 'B', 'loss'))
    print('%s: iters %d / %d, A %.17g / %.17g, B %.17g / %.17g, loss %.17g / %.17g, deviation %.3e, cond %.3g' % (
        name, got['iters'], ref['iters'], got['A'], ref['A'], got['B'], ref['B'], got['loss'], ref['loss'], dev, ref['cond']))
    for key in ('iters', 'n_pos', 'n_neg', 'flags'):
        assert int(got[key]) == ref[key], (name, key, got[key], ref[key])
    return dev


@pytest.mark.parametrize('case', range(13))
def test_platt_fit_against_the_reference(amd, case):
    name, f, y = platt_inputs()[case]
    if name.startswith('backtrack'):
        assert pr.platt_reference(f, y)['halvings'] >= 2
    elif name == 'masked':
        assert (y == 0).sum() == len(y) // 2
    assert platt_deviation(name, f, y) <= pr.PLATT_RTOL


def test_platt_fit_is_batch_invariant(amd):
    """The calibrator of n = 1025 alone, first and last of 21 (the others: other samples, masks, an empty one): identical bits."""
    from optiml_amd import _lib
    from optiml_amd.ml.svm._batched import platt_fit
    n = 1025
    f, y = pr.noisy_input(n)
    rng = np.random.default_rng(3)
    D = rng.standard_normal((21, n)) * rng.uniform(0.1, 5, (21, 1))
    L = np.where(rng.random((21, n)) < 0.5, 1., -1.) * (rng.random((21, n)) < 0.7)
    L[7] = 0.
    alone = platt_fit(f, y)
    for pos in (0, 20):
        Dp, Lp = D.copy(), L.copy()
        Dp[pos], Lp[pos] = f, y
        batch = platt_fit(Dp, Lp)
        for key in alone:
            assert alone[key][0] == batch[key][pos], (pos, key)
        assert batch['flags'][7] == _lib.PLATT_EMPTY and batch['A'][7] == 0. and batch['B'][7] == 0. and batch['iters'][7] == 0
        assert batch['n_pos'][7] == 0 and batch['n_neg'][7] == 0
        for j in range(21):
            if j not in (pos, 7):
                assert batch['n_pos'][j] == (Lp[j] > 0).sum() and batch['n_neg'][j] == (Lp[j] < 0).sum()
                assert np.isfinite([batch['A'][j], batch['B'][j], batch['loss'][j]]).all()


def test_platt_fit_argument_checks(amd):
    from optiml_amd import _lib
    from optiml_amd.device import get_context
    lib, ctx = _lib.load(), get_context().handle
    D, L = np.zeros(4), np.ones(4)
    out = [np.zeros(1), np.zeros(1), np.zeros(1, dtype=np.int32), np.zeros(1), np.zeros(1, dtype=np.int64),
           np.zeros(1, dtype=np.int64), np.zeros(1, dtype=np.int32)]
    i64 = C.POINTER(C.c_int64)
    ptrs = [_lib.ptr(out[0]), _lib.ptr(out[1]), _lib.iptr(out[2]), _lib.ptr(out[3]), out[4].ctypes.data_as(i64),
            out[5].ctypes.data_as(i64), _lib.iptr(out[6])]
    assert lib.bq_platt_fit(ctx, 1, 4, _lib.ptr(D), _lib.ptr(L), *ptrs) == _lib.OK
    assert lib.bq_platt_fit(ctx, 0, 4, _lib.ptr(D), _lib.ptr(L), *ptrs) == _lib.ERR_BADARG
    assert lib.bq_platt_fit(ctx, 1, 0, _lib.ptr(D), _lib.ptr(L), *ptrs) == _lib.ERR_BADARG
    assert lib.bq_platt_fit(ctx, 1, 4, None, _lib.ptr(L), *ptrs) == _lib.ERR_BADARG
    assert lib.bq_platt_fit(ctx, 1, 4, _lib.ptr(D), None, *ptrs) == _lib.ERR_BADARG
    for i in range(7):
        bad = list(ptrs)
        bad[i] = None
        assert lib.bq_platt_fit(ctx, 1, 4, _lib.ptr(D), _lib.ptr(L), *bad) == _lib.ERR_BADARG, i


# ---- bq_msolver_svc_heldout ---------------------------------------------------------------------------------------------------------
N, GAMMA = 600, 0.1


@functools.lru_cache(maxsize=None)
def _data(classes):
    """n = 600 (3 tile rows, a ragged last tile) rows of 8 features and labels of `classes` classes with overlap; 50 further rows
    to predict on.  Computed once and shared by the tests, which leave it unchanged."""
    rng = np.random.default_rng(17)
    X = rng.standard_normal((N + 50, 8))
    centres = rng.standard_normal((classes, 8))
    scores = X @ centres.T + 1.2 * rng.standard_normal((N + 50, classes))
    y = np.argmax(scores, axis=1) + 3   # labels 3, 4(, 5): not 0 / 1 and not +-1
    return X[:N], y[:N], X[N:]


def _folds(y, nfolds):
    from optiml_amd.ml.svm.model_selection import check_cv_splits
    return check_cv_splits(nfolds, np.zeros((len(y), 1)), y)


def _columns(classes, nfolds, full, shared):
    """(X, Y, UB, cal_of, ncal) of the (fold, class) columns, fold-major, and `full` columns on all rows that feed no calibrator;
    shared: one calibrator per class fed by every fold's column of it, else one per column"""
    X, y, _ = _data(classes)
    pos = np.unique(y)[1:] if classes == 2 else np.unique(y)
    Y, UB, cal_of = [], [], []
    for f, (tr, _) in enumerate(_folds(y, nfolds)):
        for r, p in enumerate(pos):
            ub = np.zeros(N)
            ub[tr] = 1.0
            Y.append(np.where(y == p, 1., -1.))
            UB.append(ub)
            cal_of.append(r if shared else len(cal_of))
    ncal = len(pos) if shared else len(cal_of)
    for r in range(full):
        Y.append(np.where(y == pos[r % len(pos)], 1., -1.))
        UB.append(np.ones(N))
        cal_of.append(-1)
    return X, np.stack(Y), np.stack(UB), np.array(cal_of, dtype=np.int32), ncal


def _quad(X):
    from optiml_amd.opti import KernelQuadratic
    from optiml_amd.ml.svm.kernels import GaussianKernel
    return KernelQuadratic(X, -np.ones(len(X)), 'svc', GaussianKernel(gamma=GAMMA), y=np.ones(len(X)))


def _solve(dev, kind, Y, UB, cal_of, ncal, max_iter=100):
    from optiml_amd import _lib
    from optiml_amd.ml.svm._batched import solve_batched
    held = {}

    def score(solver, _):
        held['b'], held['n_sv'], held['fit'] = solver.heldout_svc(cal_of, ncal, decisions=True)

    res = solve_batched(dev, _lib.PG if kind == 'pg' else _lib.FW, Y, UB, eps=1e-6, max_iter=max_iter, before_close=score)
    return res, held


CASES = {'two-classes': (2, 3, 1, False), 'three-classes': (3, 3, 3, False), 'three-classes-shared': (3, 3, 3, True),
         'seventeen-columns': (3, 5, 2, True)}


@pytest.mark.parametrize('kind', ['pg', 'fw'])
@pytest.mark.parametrize('case', list(CASES))
def test_heldout_against_the_host_path(amd, kind, case):
    """Per column the intercept and the support count against `intercept(Y, U, sv)` on the downloaded x and one wide product (the
    count exactly, the intercept at the per-kernel rtol 1e-12); the decision buffer against U + b with the host's b on the held-out
    rows, at the same rtol and an atol of 1e-12 |b| — the intercept's own tolerance, which an entry inherits: a decision value
    near 0 is a cancelling sum of u and b and has no relative accuracy beyond that of its terms — and 0 elsewhere; the sigmoids
    against bq_platt_fit on the downloaded buffer and labels, bit for bit — the same kernel on the same bits."""
    from optiml_amd.ml.svm._batched import _gram_matmat, intercept, platt_fit
    X, Y, UB, cal_of, ncal = _columns(*CASES[case])
    k = len(Y)
    assert k == {'two-classes': 4, 'three-classes': 12, 'three-classes-shared': 12, 'seventeen-columns': 17}[case]
    quad = _quad(X)
    dev = quad.device_problem()
    res, held = _solve(dev, kind, Y, UB, cal_of, ncal)
    assert all(0 < r['iter'] <= 100 for r in res)
    W = np.zeros((k, N))
    svs = []
    for j, r in enumerate(res):
        sv = r['x'] > 1e-6
        W[j][sv] = r['x'][sv] * Y[j][sv]
        svs.append(sv)
        assert np.all(r['x'][UB[j] == 0] == 0.)
    U = _gram_matmat(dev, W, wide=True)
    got, labels = held['fit']['dec'], np.zeros((ncal, N))
    for j in range(k):
        assert held['n_sv'][j] == svs[j].sum() > 0
        b = intercept(Y[j], U[j], svs[j])
        np.testing.assert_allclose(held['b'][j], b, rtol=1e-12)
        if cal_of[j] >= 0:
            te = UB[j] == 0
            assert te.sum() > 0 and not labels[cal_of[j]][te].any()
            np.testing.assert_allclose(got[cal_of[j]][te], U[j][te] + b, rtol=1e-12, atol=1e-12 * abs(b))
            labels[cal_of[j]][te] = Y[j][te]
    assert np.array_equal(got != 0, labels != 0)
    again = platt_fit(got, labels)
    for key in again:
        assert np.array_equal(again[key], held['fit'][key]), key
    assert not held['fit']['flags'].any() and (held['fit']['iters'] > 0).all()
    if CASES[case][3]:
        assert (held['fit']['n_pos'] + held['fit']['n_neg'] == N).all()   # every row held out once over the folds
    quad.release()


def test_heldout_argument_checks(amd):
    from optiml_amd import _lib
    from optiml_amd.ml.svm._batched import _DeviceMultiSolver
    X, Y, UB, cal_of, ncal = _columns(2, 3, 1, True)
    quad = _quad(X)
    dev = quad.device_problem()
    boxes = _DeviceMultiSolver(dev, _lib.PG, Y, UB, 1e-6, 10)
    boxes.run(5)
    boxes.heldout_svc(cal_of, ncal)
    bad = [(np.array([0, 0, 0, 0]), 1),     # the full column's held-out rows: none, so this one is fine
           (np.array([0, 0, 0, 1]), 1),     # a calibrator out of range
           (np.array([0, 0, -2, -1]), 1),
           (cal_of, 0)]
    boxes.heldout_svc(*bad[0])
    for c, m in bad[1:]:
        with pytest.raises(_lib.BcqpError) as e:
            boxes.heldout_svc(c, m)
        assert e.value.code == _lib.ERR_BADARG
    boxes.close()
    UB2 = UB.copy()
    UB2[1][np.flatnonzero(UB[0] == 0)[:3]] = 0.   # columns 0 and 1 share calibrator 0 and now three held-out rows
    overlap = _DeviceMultiSolver(dev, _lib.PG, Y, UB2, 1e-6, 10)
    overlap.run(5)
    with pytest.raises(_lib.BcqpError) as e:
        overlap.heldout_svc(cal_of, ncal)
    assert e.value.code == _lib.ERR_BADARG and 'disjoint' in str(e.value)
    overlap.heldout_svc(np.array([0, 1, 2, -1]), 3)   # a calibrator each: fine
    overlap.close()
    shared = _DeviceMultiSolver(dev, _lib.PG, Y, np.ones(N), 1e-6, 10)   # bq_msolver_create: one box for all
    shared.run(5)
    with pytest.raises(_lib.BcqpError) as e:
        shared.heldout_svc(cal_of, ncal)
    assert e.value.code == _lib.ERR_BADARG
    shared.close()
    quad.release()


# ---- CalibratedSVC end to end -------------------------------------------------------------------------------------------------------
def _svc_kw(**kw):
    from optiml_amd.ml.svm.kernels import GaussianKernel
    from optiml_amd.ml.svm.losses import hinge
    from optiml_amd.opti.constrained import ProjectedGradient
    base = dict(loss=hinge, dual=True, reg_intercept=True, optimizer=ProjectedGradient, kernel=GaussianKernel(gamma=GAMMA), C=1,
                max_iter=100)
    base.update(kw)
    return base


def _estimator(classes, **kw):
    from optiml_amd.ml.svm import SVC, OneVsRestSVC
    return (SVC if classes == 2 else OneVsRestSVC)(**_svc_kw(**kw))


@functools.lru_cache(maxsize=None)
def _loop(classes):
    """The loop CalibratedSVC replaces, with the project's own single fits (3 folds): per fold `fit` on X[tr] and
    `decision_function` on X[te] and on the 50 fresh rows, the fit on all the data, the NumPy Platt reference.  Computed once for
    both ensemble modes."""
    X, y, Xnew = _data(classes)
    kc = 1 if classes == 2 else classes
    pos = np.unique(y)[-kc:]
    Ycls = np.stack([np.where(y == p, 1., -1.) for p in pos])
    splits = _folds(y, 3)
    oof = np.zeros((kc, N))
    fold_new, fold_cal = [], []
    for tr, te in splits:
        est = _estimator(classes).fit(X[tr], y[tr])
        F = est.decision_function(X[te]).reshape(len(te), kc)
        oof[:, te] = F.T
        fold_new.append(est.decision_function(Xnew).reshape(len(Xnew), kc))
        fold_cal.append([pr.platt_reference(F[:, r], Ycls[r][te]) for r in range(kc)])
    full = _estimator(classes).fit(X, y)
    return dict(splits=splits, oof=oof, fold_new=fold_new, fold_cal=fold_cal, full_new=full.decision_function(Xnew).reshape(-1, kc),
                full_cal=[pr.platt_reference(oof[r], Ycls[r]) for r in range(kc)], classes=np.unique(y))


def _proba(F, cals):
    """the assembly rules, written out"""
    P = np.stack([1. / (1. + np.exp(c['A'] * F[:, r] + c['B'])) for r, c in enumerate(cals)], axis=1)
    if P.shape[1] == 1:
        return np.hstack((1. - P, P))
    total = P.sum(axis=1, keepdims=True)
    return np.where(total == 0, 1. / P.shape[1], P / np.where(total == 0, 1., total))


@functools.lru_cache(maxsize=None)
def decision_deviation(classes, ensemble):
    """Fitted once per configuration and shared: (fitted estimator, reference, the largest deviation of the batched columns'
    decision values from the single fits' — held-out and fresh rows — relative to the largest decision value)"""
    from optiml_amd.ml.svm import CalibratedSVC
    X, y, Xnew = _data(classes)
    ref = _loop(classes)
    est = CalibratedSVC(_estimator(classes), cv=3, ensemble=ensemble).fit(X, y)
    assert est.batched_ is True and est.batched_decision_ is True
    got = est._decisions(Xnew)
    want = np.hstack(ref['fold_new']) if ensemble else ref['full_new']
    assert got.shape == want.shape
    dev = np.abs(got - want).max() / np.abs(want).max()
    if not ensemble:
        oof = est.oof_decision_.reshape(N, -1).T
        dev = max(dev, np.abs(oof - ref['oof']).max() / np.abs(ref['oof']).max())
    return est, ref, float(dev)


def probability_deviation(classes, ensemble):
    """(estimator, reference, the loop's probabilities on the 50 fresh rows, the estimator's, the largest deviation of an entry
    relative to the loop's)"""
    est, ref, _ = decision_deviation(classes, ensemble)
    Xnew = _data(classes)[2]
    cals = ref['fold_cal'] if ensemble else [ref['full_cal']]
    news = ref['fold_new'] if ensemble else [ref['full_new']]
    want = np.mean([_proba(F, c) for F, c in zip(news, cals)], axis=0)
    got = est.predict_proba(Xnew)
    return est, ref, want, got, float((np.abs(got - want) / want).max())


@pytest.mark.parametrize('ensemble', [True, False])
@pytest.mark.parametrize('classes', [2, 3])
def test_calibrated_svc_equals_the_loop(amd, classes, ensemble):
    """predict_proba on 50 fresh rows against the loop's, entry by entry, at the bound of the Platt comparison widened by the
    decision-value deviation of the batched columns against single fits (PLATT_RTOL + DECISION_RTOL): both measured on an MI355X
    (profiles/calibration/platt_parity.json) and taken 16-fold.  The project's own figure for alphas over 100 PG iterations at
    C <= 1 is 2e-14.

    The headroom on the decision figure is needed, not spare: a probability deviates by more than its decision value does (8.1e-12
    against 2.9e-12 measured).  With z = A f + B and p = 1 / (1 + exp(z)), dp / p = -(1 - p) dz, and dz = A df carries the
    sigmoid's slope (|A| is 1.5 to 2.9 here) on a df that is relative to the LARGEST decision value; the calibrators themselves
    are also fitted on perturbed held-out values, which moves A and B by a few times as much.

    Three of the four configurations measure 2e-14 to 7e-14, the two-class `ensemble=False` one 2.9e-12, all of it on the fresh
    rows, which the column of the fit on all the data predicts (its out-of-fold values deviate by 2.2e-14).  That column's alphas
    agree with `SVC.fit`'s to 1.2e-13 (the folds': 7e-15 to 2e-14) — the two objective histories agree to 1e-13 for 90 iterations
    and part to 1e-12 in the last ten, the amplified rounding DESIGN notes for the search — and the intercept then multiplies it:
    b = sum (y - u) / n_sv runs over 553 support rows of u = K (alpha y), each carrying the deviations of 553 alphas, and this
    b is a cancelling sum (-0.026 from terms of order 1), so it deviates by 7.7e-12, 2.9e-10 of itself, and shifts every decision
    value by that amount: 2.9e-12 of the largest."""
    est, ref, dev = decision_deviation(classes, ensemble)
    Xnew = _data(classes)[2]
    print('classes %d, ensemble %s: decision deviation %.3e' % (classes, ensemble, dev))
    assert dev <= pr.DECISION_RTOL
    _, _, want, got, pdev = probability_deviation(classes, ensemble)
    flat = [c for group in (ref['fold_cal'] if ensemble else [ref['full_cal']]) for c in group]
    # The preconditions of equal iteration counts.  Here the device's calibrator and the reference's read decision values that
    # differ by DECISION_RTOL (5e-11 of the largest) at most, which moves a gradient entry by about as much of sum |f d1|, a few
    # units: a stop test decided by 1 % (gradient entries are compared with 1e-5) is 4 orders of magnitude beyond that.  (One of
    # these calibrators stops with its larger entry at 0.914e-5, so platt_deviation's factor 1.1 is not on offer on this data.)
    for c in flat:
        print('reference: iters %d, stop ratio %.3g, search margin %.3g, cond %.3g' % (c['iters'], c['stop_ratio'], c['search_margin'],
                                                                                     c['cond']))
        assert c['flags'] == 0 and c['stop_ratio'] < 1 / 1.01 and c['search_margin'] > pr.SEARCH_MARGIN
    print('probability deviation %.3e (bound %.3e)' % (pdev, pr.PLATT_RTOL + pr.DECISION_RTOL))
    np.testing.assert_allclose(got, want, rtol=pr.PLATT_RTOL + pr.DECISION_RTOL, atol=0)
    np.testing.assert_allclose(got.sum(axis=1), 1., rtol=1e-14)
    assert got.shape == (50, classes) and np.array_equal(est.classes_, ref['classes'])
    assert np.array_equal(est.predict(Xnew), ref['classes'][np.argmax(want, axis=1)])
    shape = (3, len(flat) // 3) if ensemble else (len(flat),)
    assert est.calibrators_['A'].shape == shape and len(est.calibrated_classifiers_) == (3 if ensemble else 1)
    iters = np.array([c['iters'] for c in flat]).reshape(shape)
    assert np.array_equal(est.calibrators_['iters'], iters) and not est.calibrators_['flags'].any()
    for rec in est.calibrated_classifiers_:   # the records predict on their own, as the loop's classifiers do
        assert np.asarray(rec.estimator.decision_function(Xnew)).shape == ((50,) if classes == 2 else (50, classes))


@pytest.mark.parametrize('classes', [2, 3])
def test_an_fp32_panel_takes_the_loop_path(amd, classes):
    """storage='f32': the loop of single fits (the fp32 panel does not hold the decision kernel's values), the sigmoids through
    bq_platt_fit; its decision values agree with the f64 estimator's at the project's fp32 tolerances."""
    from optiml_amd.ml.svm import CalibratedSVC
    X, y, Xnew = _data(classes)
    est64, _, _ = decision_deviation(classes, True)
    est32 = CalibratedSVC(_estimator(classes, storage='f32'), cv=3).fit(X, y)
    assert est32.batched_ is False and est32.batched_decision_ is False
    np.testing.assert_allclose(est32._decisions(Xnew), est64._decisions(Xnew), rtol=1e-4, atol=1e-5)
    P = est32.predict_proba(Xnew)
    np.testing.assert_allclose(P.sum(axis=1), 1., rtol=1e-14)
    assert P.shape == (50, classes) and not est32.calibrators_['flags'].any()
    off = CalibratedSVC(_estimator(classes, storage='f32'), cv=3, ensemble=False).fit(X, y)
    assert off.batched_ is False and off.oof_decision_.shape == ((N,) if classes == 2 else (N, classes))
    assert len(off.calibrated_classifiers_) == 1 and off.predict_proba(Xnew).shape == (50, classes)
