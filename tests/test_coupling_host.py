"""CPU checks of PairwiseCoupledSVC: the NumPy restatement of libsvm's pairwise coupling (tests/coupling_reference.py) against
sklearn's SVC(probability=True), the argument checks and the C ABI of the three new entry points, the batched path's column plan as
plain arrays, the class's own checks and its path selection (no GPU needed)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import coupling_reference as cr

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ['bq_msolver_pairs_heldout', 'bq_pairwise_coupling', 'bq_decision_coupled']


@pytest.fixture(scope='module')
def lib():
    from optiml_amd import build, _lib
    build.build()
    return _lib.load()


@pytest.mark.parametrize('k', [3, 5, 9])
def test_reference_against_sklearn(k):
    """sklearn.svm.SVC(probability=True) on blobs of n = 60 k: its probA_ / probB_ and its ovo decision values into the
    restatement give its predict_proba.  libsvm's positive class of a pair is the SMALLER label: its decision value is -f and its
    sigmoid 1 / (1 + exp(A' f' + B')) is P(a), so P(b) = 1 / (1 + exp(A' f - B')): A = A', B = -B' on f = -f'.  (k = 2 is left out:
    sklearn flips the binary sign.)  libsvm rounds P(a) and takes P(b) = 1 - P(a), the restatement the other way round, so a pair
    probability differs by an ulp of 1, which is a large relative change of a small one: overlapping blobs (no probability below
    1e-3) keep the comparison about the iteration."""
    svm = pytest.importorskip('sklearn.svm')
    from sklearn.datasets import make_blobs
    X, y = make_blobs(n_samples=60 * k, centers=k, n_features=4, cluster_std=6.0, random_state=k)
    model = svm.SVC(probability=True, decision_function_shape='ovo', kernel='rbf', gamma=0.1, random_state=0).fit(X, y)
    F = -model.decision_function(X)
    S = cr.sigmoid(F, model.probA_, -model.probB_)
    P, iters, _ = cr.couple_rows(S, k)
    want = model.predict_proba(X)
    print('k = %d: largest deviation %.3e relative, %.3e absolute; sweeps %d to %d' % (
        k, np.abs(P / want - 1).max(), np.abs(P - want).max(), iters.min(), iters.max()))
    np.testing.assert_allclose(P, want, rtol=1e-12, atol=0)
    np.testing.assert_allclose(P.sum(axis=1), 1., rtol=0, atol=1e-14)
    assert 1 <= iters.min() and iters.max() <= 8


def test_reference_on_hand_inputs():
    """All s = 0.5: the start point passes the stop test (sweep 0, p = 1 / k exactly).  Two classes: p = (1 - s, s) to rounding,
    the coupling of one pair being that pair."""
    for k in cr.CLASSES:
        p, it, margin = cr.coupling_reference([0.5] * (k * (k - 1) // 2), k)
        assert it == 0 and np.array_equal(p, np.full(k, 1. / k)) and margin > 0.99
    p, it, _ = cr.coupling_reference([0.8], 2)
    np.testing.assert_allclose(p, [0.2, 0.8], rtol=0, atol=0.005 / 2)
    assert it >= 1


def test_the_vectorised_restatement_has_the_scalar_one_s_bits():
    for k in (2, 3, 7, 33):
        for family in cr.FAMILIES:
            S = cr.sigmoid(cr.decision_values(cr.target_probabilities(family, k, 5)), -1., 0.)
            P, iters, margin = cr.couple_rows(S, k)
            for i, row in enumerate(S):
                p, it, m = cr.coupling_reference(row, k)
                assert np.array_equal(p, P[i]) and it == iters[i] and m == margin[i], (k, family, i)
    assert cr.couple_rows(np.full((2, 1), 1. - cr.CLIP), 2)[1].max() < 100


def test_the_bounds_are_sixteen_times_the_recorded_measurements():
    import json
    rec = json.load(open(os.path.join(REPO, 'profiles', 'coupling', 'parity.json')))
    assert rec['coupling_points_that_differ'] == 0   # the coupling is compared bit for bit: no bound
    for name in ('sigmoid', 'ab', 'proba'):
        measured = getattr(cr, name.upper() + '_MEASURED')
        assert measured == rec[name + '_max_rel_dev'] == max(rec[name].values()), name
        assert getattr(cr, name.upper() + '_RTOL') == 16 * measured
    assert rec['sigmoid_max_rel_dev'] < 1e-14 and rec['proba_max_rel_dev'] < 1e-8   # above that: a defect to explain, not a tolerance


@pytest.mark.parametrize('family', cr.FAMILIES)
def test_the_shared_inputs_stay_clear_of_the_cap_and_of_undecided_stop_tests(family):
    """What the device comparison presupposes, checked on the reference alone: the inputs take a handful of sweeps, never the cap,
    and at least 95 % of every case's points have every stop test decided by more than 1e-9 (relative)."""
    for k in cr.CLASSES:
        for t in cr.POINTS:
            S = cr.sigmoid(cr.decision_values(cr.target_probabilities(family, k, t)), -1., 0.)
            assert S.min() >= cr.CLIP and S.max() <= 1. - cr.CLIP
            if family == 'clipped':
                assert np.isin(S, [cr.CLIP, 1. - cr.CLIP]).all()
            P, iters, margin = cr.couple_rows(S, k)
            assert iters.max() <= 8 and (family != 'half' or iters.max() == 0), (k, iters.max())
            assert (margin > cr.SAFE_MARGIN).mean() >= cr.SAFE_SHARE, k
            np.testing.assert_allclose(P.sum(axis=1), 1., rtol=0, atol=1e-14)


def test_the_symbols_are_declared_exported_and_bound(lib):
    from optiml_amd import _lib
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(REPO, 'include', 'bcqp.h')).read(), flags=re.S)
    assert re.search(r'#define BQ_ABI_VERSION 3\b', text)
    for s in NEW_SYMBOLS:
        assert re.search(r'\bint\s+%s\s*\(' % s, text), s
        assert hasattr(lib, s), s
        assert s in _lib.PROTOTYPES, s
    assert _lib.ABI_VERSION == 3 and lib.bq_abi_version() == 3


def test_coupling_argument_checks_answer_before_any_device_call(lib):
    """k > 64, k < 2, a non-positive size, a NULL required pointer: ERR_BADARG with a message.  The context is a block of zeroed
    host memory: the checks must answer before the library reads it or calls the device."""
    from optiml_amd import _lib
    fake = C.cast(C.create_string_buffer(1 << 16), C.c_void_p)
    k, t = 3, 4
    F, A, B, prob = np.zeros((t, 3)), -np.ones(3), np.zeros(3), np.empty((t, k))
    p = lambda a: None if a is None else _lib.ptr(a)   # noqa: E731

    def call(ctx=fake, k=k, t=t, F=F, A=A, B=B, prob=prob):
        return lib.bq_pairwise_coupling(ctx, k, t, p(F), p(A), p(B), p(prob), None, None)

    for kw in (dict(ctx=None), dict(F=None), dict(A=None), dict(B=None), dict(prob=None)):
        assert call(**kw) == _lib.ERR_BADARG, kw
        assert b'NULL' in lib.bq_last_error()
    for kw, msg in ((dict(k=65), b'64'), (dict(k=1), b'ncls'), (dict(k=0), b'ncls'), (dict(k=-2), b'ncls'), (dict(t=0), b't must'),
                    (dict(t=-5), b't must')):
        assert call(**kw) == _lib.ERR_BADARG, kw
        assert msg in lib.bq_last_error(), (kw, lib.bq_last_error())

    m, d = 5, 2
    SV, W, b, Xt = np.ones((m, d)), np.ones((3, m)), np.zeros(3), np.ones((t, d))

    def fused(ctx=fake, kernel=_lib.KERNEL_RBF, m=m, d=d, SV=SV, cols=3, W=W, t=t, Xt=Xt, k=k, A=A, B=B, prob=prob):
        return lib.bq_decision_coupled(ctx, kernel, 0.5, 0.0, 3, m, d, p(SV), cols, p(W), p(b), t, p(Xt), k, p(A), p(B), p(prob),
                                       None, None, None)

    for kw in (dict(ctx=None), dict(SV=None), dict(W=None), dict(Xt=None), dict(A=None), dict(B=None), dict(prob=None)):
        assert fused(**kw) == _lib.ERR_BADARG, kw
        assert b'NULL' in lib.bq_last_error()
    for kw in (dict(k=65, cols=2080), dict(k=1, cols=0), dict(t=0), dict(m=0), dict(d=0), dict(cols=2), dict(cols=4)):
        assert fused(**kw) == _lib.ERR_BADARG, kw
        assert lib.bq_last_error()
    assert fused(kernel=_lib.KERNEL_LAPLACIAN) == _lib.ERR_BADARG
    assert b'Laplacian' in lib.bq_last_error()
    assert fused(kernel=17) == _lib.ERR_BADARG


def test_pairs_heldout_takes_a_solver(lib):
    from optiml_amd import _lib
    i64 = C.POINTER(C.c_int64)
    out = [np.zeros(1), np.zeros(1), np.zeros(1, dtype=np.int32), np.zeros(1), np.zeros(1, dtype=np.int64),
           np.zeros(1, dtype=np.int64), np.zeros(1, dtype=np.int32)]
    ptrs = [_lib.ptr(out[0]), _lib.ptr(out[1]), _lib.iptr(out[2]), _lib.ptr(out[3]), out[4].ctypes.data_as(i64),
            out[5].ctypes.data_as(i64), _lib.iptr(out[6])]
    cal_of, b, n_sv, rows = np.zeros(1, dtype=np.int32), np.zeros(1), np.zeros(1, dtype=np.int64), np.ones(4, dtype=np.uint8)
    assert lib.bq_msolver_pairs_heldout(None, rows.ctypes.data_as(C.POINTER(C.c_ubyte)), 1, _lib.iptr(cal_of), _lib.ptr(b),
                                        n_sv.ctypes.data_as(i64), *ptrs, None) == _lib.ERR_BADARG
    assert b'NULL' in lib.bq_last_error()


# ---- the column plan ---------------------------------------------------------------------------------------------------------------
def _plan(sizes=(300, 257, 40), nfolds=3, C=2.5, seed=0):
    from optiml_amd.ml.svm.coupling import coupling_columns
    from optiml_amd.ml.svm.model_selection import check_cv_splits
    rng = np.random.default_rng(seed)
    codes = rng.permutation(np.repeat(np.arange(len(sizes)), sizes))
    splits = check_cv_splits(nfolds, np.zeros((len(codes), 1)), codes)
    return codes, splits, coupling_columns(codes, len(sizes), splits, C)


def test_the_column_plan():
    """Class sizes (300, 257, 40): tiles 2, 2, 1, ghost rows in every class.  Column (pair, fold): C exactly on the pair's data
    rows of the fold's training part; 0 on its held-out rows, on ghost rows and on every row of another class.  The held-out rows
    of a pair's fold columns partition the pair's data rows.  Column (pair, all) is OneVsOneSVC's."""
    from optiml_amd.ml.svm.coupling import chunk_calibrators
    codes, splits, plan = _plan()
    n_pad, index, pcode, data = plan['n_pad'], plan['index'], plan['pcode'], plan['data_row'] > 0
    assert list(plan['cls_tiles']) == [0, 2, 4, 5] and n_pad == 1280 and data.sum() == 597
    assert [(~data & (pcode == c)).sum() for c in range(3)] == [212, 255, 216]
    assert np.array_equal(pcode[index], codes)
    assert plan['pairs'] == [(0, 1), (0, 2), (1, 2)]
    assert plan['cols'] == [(p, f) for p in range(3) for f in (0, 1, 2, None)]
    assert plan['Y'].shape == plan['UB'].shape == (12, n_pad)
    for c, (p, f) in enumerate(plan['cols']):
        a, b = plan['pairs'][p]
        ub, mine = plan['UB'][c], (pcode == a) | (pcode == b)
        assert set(np.unique(ub)) <= {0., 2.5}
        assert not ub[~data].any() and not ub[~mine].any()
        assert np.array_equal(plan['Y'][c], np.where(pcode == b, 1., -1.))
        if f is None:
            assert np.array_equal(ub > 0, mine & data)
            continue
        tr, te = splits[f]
        want = np.zeros(n_pad, dtype=bool)
        want[index[tr]] = True
        assert np.array_equal(ub > 0, want & mine)
        held = mine & data & (ub == 0)
        te_pair = te[(codes[te] == a) | (codes[te] == b)]
        assert np.array_equal(np.sort(index[te_pair]), np.flatnonzero(held)) and held.sum() > 0
    for p, (a, b) in enumerate(plan['pairs']):
        mine = ((pcode == a) | (pcode == b)) & data
        held = np.stack([mine & (plan['UB'][4 * p + f] == 0) for f in range(3)])
        assert np.array_equal(held.sum(axis=0), mine.astype(int))   # every row of the pair held out exactly once
    cal_of, cal_pairs = chunk_calibrators(plan['cols'])
    assert list(cal_of) == [0, 0, 0, -1, 1, 1, 1, -1, 2, 2, 2, -1] and cal_pairs == [0, 1, 2]
    cal_of, cal_pairs = chunk_calibrators(plan['cols'][5:11])   # a solve that starts inside pair 1
    assert list(cal_of) == [0, 0, -1, 1, 1, 1] and cal_pairs == [1, 2]
    cal_of, cal_pairs = chunk_calibrators([(2, None)])
    assert list(cal_of) == [-1] and cal_pairs == []


# ---- the class ---------------------------------------------------------------------------------------------------------------------
def _svc_kw(**kw):
    from optiml_amd.ml.svm.kernels import GaussianKernel
    from optiml_amd.ml.svm.losses import hinge
    from optiml_amd.opti.constrained import ProjectedGradient
    base = dict(loss=hinge, dual=True, reg_intercept=True, optimizer=ProjectedGradient, kernel=GaussianKernel(gamma=0.1))
    base.update(kw)
    return base


def _blobs(n, k, seed=0):
    rng = np.random.default_rng(seed)
    y = np.arange(n) % k
    return rng.standard_normal((n, 3)) + 2. * y[:, None], y


def test_exported_from_the_svm_package():
    from optiml_amd.ml import svm
    from optiml_amd.ml.svm.coupling import PairwiseCoupledSVC
    assert svm.PairwiseCoupledSVC is PairwiseCoupledSVC and 'PairwiseCoupledSVC' in svm.__all__


def test_only_one_vs_one_is_coupled():
    from optiml_amd.ml.svm import SVC, OneVsRestSVC, PairwiseCoupledSVC
    X, y = _blobs(30, 3)
    for est in (SVC(**_svc_kw()), OneVsRestSVC(**_svc_kw()), None):
        with pytest.raises(TypeError, match='OneVsOneSVC'):
            PairwiseCoupledSVC(est).fit(X, y)


@pytest.mark.parametrize('which', ['overlapping', 'incomplete'])
def test_every_row_is_held_out_exactly_once(which):
    from optiml_amd.ml.svm import OneVsOneSVC, PairwiseCoupledSVC
    X, y = _blobs(30, 3)
    idx = np.arange(30)
    te = [idx[:10], idx[10:20], idx[20:]]
    if which == 'overlapping':
        te[1] = idx[8:20]
    else:
        te[2] = idx[20:28]
    splits = [(np.setdiff1d(idx, t), t) for t in te]
    with pytest.raises(ValueError, match='held out exactly once'):
        PairwiseCoupledSVC(OneVsOneSVC(**_svc_kw()), cv=splits).fit(X, y)


def test_a_fold_that_misses_a_class_is_refused():
    from optiml_amd.ml.svm import OneVsOneSVC, PairwiseCoupledSVC
    X, y = _blobs(30, 3)
    y = np.sort(y)
    idx = np.arange(30)
    last = idx[y == 2]
    splits = [(np.setdiff1d(idx, last), last), (last, np.setdiff1d(idx, last))]
    with pytest.raises(ValueError, match='miss a class'):
        PairwiseCoupledSVC(OneVsOneSVC(**_svc_kw()), cv=splits).fit(X, y)


def test_more_than_64_classes_are_refused():
    from optiml_amd.ml.svm import OneVsOneSVC, PairwiseCoupledSVC
    from optiml_amd.ml.svm.coupling import pairwise_coupling
    X, y = _blobs(195, 65)
    with pytest.raises(ValueError, match='at most 64 classes'):
        PairwiseCoupledSVC(OneVsOneSVC(**_svc_kw()), cv=3).fit(X, y)
    with pytest.raises(ValueError, match='one class|two classes'):
        PairwiseCoupledSVC(OneVsOneSVC(**_svc_kw()), cv=3).fit(X, np.zeros(195))
    for k in (1, 65):
        with pytest.raises(ValueError, match='2 to 64 classes'):
            pairwise_coupling(np.zeros((1, 1)), [1.], [0.], k)
    for shape in ((3, 12), (3, 5), (6,), (2, 3, 6)):   # not t x 6: in particular t x 12 is not 2 t points
        with pytest.raises(ValueError, match='t x 6'):
            pairwise_coupling(np.zeros(shape), -np.ones(6), np.zeros(6), 4)
    prob, iters, R = pairwise_coupling(np.zeros((0, 6)), -np.ones(6), np.zeros(6), 4)   # no point: no device call
    assert prob.shape == (0, 4) and iters.shape == (0,) and R.shape == (0, 6)


def test_path_selection():
    """The batched path: OneVsOneSVC's own, an fp64 panel and a numeric gamma.  A string gamma, an fp32 panel and two ranks take
    the loop."""
    from optiml_amd.ml.svm import SVC, OneVsOneSVC, OneVsRestSVC
    from optiml_amd.ml.svm.coupling import uses_batched_coupling
    from optiml_amd.ml.svm.kernels import GaussianKernel, linear
    from optiml_amd.opti.constrained import FrankWolfe, InteriorPoint
    table = [
        (OneVsOneSVC(**_svc_kw()), 1, True),
        (OneVsOneSVC(**_svc_kw(optimizer=FrankWolfe)), 1, True),
        (OneVsOneSVC(**_svc_kw(kernel=linear)), 1, True),
        (OneVsOneSVC(**_svc_kw(kernel=GaussianKernel(gamma='auto'))), 1, False),
        (OneVsOneSVC(**_svc_kw(kernel=GaussianKernel(gamma='scale'))), 1, False),
        (OneVsOneSVC(**_svc_kw(storage='f32')), 1, False),
        (OneVsOneSVC(**_svc_kw(storage='stream')), 1, False),
        (OneVsOneSVC(**_svc_kw(optimizer=InteriorPoint)), 1, False),
        (OneVsOneSVC(**_svc_kw()), 2, False),
        (OneVsRestSVC(**_svc_kw()), 1, False),
        (SVC(**_svc_kw()), 1, False),
    ]
    for est, world, want in table:
        assert uses_batched_coupling(est, world) is want, (type(est).__name__, world)


def test_a_flagged_sigmoid_fit_warns_and_keeps_its_values(monkeypatch):
    from types import SimpleNamespace
    from optiml_amd import _lib
    from optiml_amd.ml.svm import OneVsOneSVC, PairwiseCoupledSVC
    from optiml_amd.ml.svm import coupling
    from optiml_amd.ml.svm._base import ConvergenceWarning
    X, y = _blobs(30, 3)
    flags = np.array([0, _lib.PLATT_MAX_ITER, 0], dtype=np.int32)
    cal = dict(A=np.array([-1., -2., -3.]), B=np.array([0.1, 0.2, 0.3]), iters=np.array([5, 100, 6], dtype=np.int32),
               loss=np.ones(3), flags=flags, n_pos=np.full(3, 10), n_neg=np.full(3, 10))

    def fit_loop(self, X, y, codes, splits):
        self.estimator_ = SimpleNamespace(batched_decision_=False)
        return cal

    monkeypatch.setattr(coupling, 'get_context', lambda: SimpleNamespace(world=1))
    monkeypatch.setattr(PairwiseCoupledSVC, '_fit_loop', fit_loop)
    est = PairwiseCoupledSVC(OneVsOneSVC(**_svc_kw(storage='f32')), cv=3)
    with pytest.warns(ConvergenceWarning, match=r'1 pair\(s\).*first: pair 1'):
        est.fit(X, y)
    assert est.batched_ is False and est.batched_decision_ is False
    assert list(est.probA_) == [-1., -2., -3.] and list(est.probB_) == [0.1, 0.2, 0.3]
    assert np.array_equal(est.calibrators_['flags'], flags)
    cal['flags'] = np.zeros(3, dtype=np.int32)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        est.fit(X, y)
