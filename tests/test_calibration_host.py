"""CPU checks of CalibratedSVC: the NumPy reference of the Platt iteration against sklearn's optimiser, the probability assembly
against hand-computed values, path selection, the argument checks and the C ABI of the two new entry points (no GPU needed)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import platt_reference as pr

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ['bq_platt_fit', 'bq_msolver_svc_heldout']


def _inputs():
    return [('noisy-%d' % n, pr.noisy_input(n)) for n in pr.NOISY_N] + [(c, pr.edge_input(c)) for c in pr.EDGE_CASES] + \
        [('masked', pr.masked_input())] + [('backtrack-%d' % s, pr.backtracking_candidate(s)) for s in pr.BACKTRACK_SEEDS]


SKLEARN_CASES = [i for i, c in enumerate(['noisy'] * 5 + list(pr.EDGE_CASES) + ['masked', 'backtrack', 'backtrack']) if c != 'one-class']


@pytest.mark.parametrize('case', SKLEARN_CASES)
def test_reference_against_sklearn(case):
    """sklearn minimises the same loss from the same targets by L-BFGS and stops on L-BFGS's own tolerance, so the two agree only
    as far as that tolerance goes: 1e-6 to 1e-8 on the well-conditioned inputs.  The margin here is loose on purpose, 1e-4 relative
    with 1e-5 absolute: it catches a wrong target, sign or loss, not rounding.  (The single-class input is left to the test below:
    the reference stops at its start point there.)"""
    cal = pytest.importorskip('sklearn.calibration')
    name, (f, y) = _inputs()[case]
    keep = y != 0
    ref = pr.platt_reference(f, y)
    a, b = cal._sigmoid_calibration(f[keep], (y[keep] > 0).astype(float))
    print(name, ref['A'], a, ref['B'], b)
    np.testing.assert_allclose([ref['A'], ref['B']], [a, b], rtol=1e-4, atol=1e-5)


def test_reference_on_the_issue_inputs_takes_few_steps_and_never_halves():
    for name, (f, y) in _inputs()[:11]:
        ref = pr.platt_reference(f, y)
        assert 0 <= ref['iters'] <= 8 and ref['halvings'] == 0 and ref['flags'] == 0, name
        assert ref['stop_ratio'] < 1 / 1.1 and ref['search_margin'] > pr.SEARCH_MARGIN, name
    one = pr.platt_reference(*pr.edge_input('one-class'))
    assert one['iters'] == 0 and one['A'] == 0. and one['B'] == np.log(301.) and one['n_pos'] == 0 and one['n_neg'] == 300
    for s in pr.BACKTRACK_SEEDS:
        ref = pr.platt_reference(*pr.backtracking_candidate(s))
        assert ref['halvings'] >= 1 and ref['flags'] == 0 and ref['stop_ratio'] < 1 / 1.1 and ref['search_margin'] > 1e-9 > pr.SEARCH_MARGIN


def test_reference_ignores_unlabelled_rows_and_handles_an_empty_sample():
    f, y = pr.masked_input()
    keep = y != 0
    assert keep.sum() == 500
    assert pr.platt_reference(f, y) == pr.platt_reference(f[keep], y[keep])
    empty = pr.platt_reference(f, np.zeros_like(y))
    assert empty['flags'] == pr.EMPTY and empty['A'] == 0. and empty['B'] == 0.


def test_two_class_probabilities():
    from optiml_amd.ml.svm.calibration import sigmoid_probabilities
    f = np.array([0., 1., -2.])
    P = sigmoid_probabilities(f, [-2.], [0.5])
    p = 1. / (1. + np.exp(-2. * f + 0.5))
    np.testing.assert_allclose(P, np.stack((1. - p, p), axis=1), rtol=1e-15)
    np.testing.assert_allclose(P[0], [1. - 1. / (1. + np.exp(0.5)), 1. / (1. + np.exp(0.5))], rtol=1e-15)
    assert np.array_equal(P, sigmoid_probabilities(f[:, None], [-2.], [0.5]))


def test_multiclass_probabilities_are_normalised_and_a_zero_row_is_uniform():
    from optiml_amd.ml.svm.calibration import sigmoid_probabilities
    F = np.array([[0., 0., 0.], [1., -1., 0.], [800., 800., 800.]])
    P = sigmoid_probabilities(F, [-1., -1., 1.], [0., 0., 0.])
    np.testing.assert_allclose(P[0], [1. / 3] * 3, rtol=1e-15)
    e = np.e
    raw = np.array([1. / (1. + 1. / e), 1. / (1. + e), 0.5])
    np.testing.assert_allclose(P[1], raw / raw.sum(), rtol=1e-15)
    np.testing.assert_allclose(P.sum(axis=1), 1., rtol=1e-15)
    # every sigmoid underflows to 0 (exp overflows to inf): the row sum is 0 and the row is 1 / k
    Z = sigmoid_probabilities(np.full((2, 4), 800.), [1.] * 4, [0.] * 4)
    assert np.array_equal(Z, np.full((2, 4), 0.25))


def test_the_ensemble_is_the_mean_over_folds():
    from optiml_amd.ml.svm.calibration import assemble_probabilities
    a = np.array([[0.2, 0.8], [0.5, 0.5]])
    b = np.array([[0.4, 0.6], [0.1, 0.9]])
    c = np.array([[0.6, 0.4], [0.3, 0.7]])
    np.testing.assert_allclose(assemble_probabilities([a, b, c]), [[0.4, 0.6], [0.3, 0.7]], rtol=1e-15)
    assert np.array_equal(assemble_probabilities([a]), a)


def _svc_kw(**kw):
    from optiml_amd.ml.svm.kernels import GaussianKernel
    from optiml_amd.ml.svm.losses import hinge
    from optiml_amd.opti.constrained import ProjectedGradient
    base = dict(loss=hinge, dual=True, reg_intercept=True, optimizer=ProjectedGradient, kernel=GaussianKernel(gamma=0.1))
    base.update(kw)
    return base


def _path_rows():
    from optiml_amd.ml.svm import SVC, OneVsOneSVC, OneVsRestSVC
    from optiml_amd.ml.svm.kernels import GaussianKernel, linear
    from optiml_amd.opti.constrained import FrankWolfe, InteriorPoint
    return [
        (SVC(**_svc_kw()), 1, True),
        (OneVsRestSVC(**_svc_kw()), 1, True),
        (OneVsRestSVC(**_svc_kw(optimizer=FrankWolfe)), 1, True),
        (SVC(**_svc_kw(kernel=linear)), 1, True),
        (SVC(**_svc_kw(kernel=GaussianKernel(gamma='auto'))), 1, False),
        (SVC(**_svc_kw(storage='f32')), 1, False),
        (OneVsRestSVC(**_svc_kw(storage='f32')), 1, False),
        (SVC(**_svc_kw(kernel=GaussianKernel(gamma='scale'))), 1, False),
        (OneVsRestSVC(**_svc_kw(optimizer=InteriorPoint)), 1, False),
        (SVC(**_svc_kw()), 2, False),
        (OneVsRestSVC(**_svc_kw()), 2, False),
        (SVC(**_svc_kw(storage='stream')), 1, False),
        (OneVsOneSVC(**_svc_kw()), 1, False),
    ]


@pytest.mark.parametrize('row', range(13))
def test_path_selection(row):
    from optiml_amd.ml.svm.calibration import uses_batched_calibration
    est, world, want = _path_rows()[row]
    assert uses_batched_calibration(est, world) is want


def _blobs(n, k, seed=0):
    rng = np.random.default_rng(seed)
    y = np.arange(n) % k
    return rng.standard_normal((n, 3)) + 2. * y[:, None], y


def test_only_svc_and_one_vs_rest_are_calibrated():
    from optiml_amd.ml.svm import SVR, CalibratedSVC, OneVsOneSVC
    X, y = _blobs(30, 2)
    with pytest.raises(TypeError):
        CalibratedSVC(OneVsOneSVC(**_svc_kw())).fit(X, y)
    with pytest.raises(TypeError):
        CalibratedSVC(SVR()).fit(X, y)
    with pytest.raises(TypeError):
        CalibratedSVC(estimator=None).fit(X, y)
    with pytest.raises(TypeError):
        CalibratedSVC(OneVsOneSVC(**_svc_kw()), 3, False, method='sigmoid')   # the method is always the sigmoid


@pytest.mark.parametrize('which', ['overlapping', 'incomplete'])
def test_ensemble_false_needs_every_row_held_out_once(which):
    from optiml_amd.ml.svm import SVC, CalibratedSVC
    X, y = _blobs(30, 2)
    idx = np.arange(30)
    te = [idx[:10], idx[10:20], idx[20:]]
    if which == 'overlapping':
        te[1] = idx[8:20]
    else:
        te[2] = idx[20:28]
    splits = [(np.setdiff1d(idx, t), t) for t in te]
    with pytest.raises(ValueError, match='held out exactly once'):
        CalibratedSVC(SVC(**_svc_kw()), cv=splits, ensemble=False).fit(X, y)


@pytest.mark.parametrize('multiclass', [False, True])
def test_a_fold_that_misses_a_class_is_refused(multiclass):
    from optiml_amd.ml.svm import SVC, CalibratedSVC, OneVsRestSVC
    k = 3 if multiclass else 2
    X, y = _blobs(30, k)
    y = np.sort(y)   # the last class in the last rows: the first fold's training rows miss it
    idx = np.arange(30)
    last = idx[y == k - 1]
    splits = [(np.setdiff1d(idx, last), last), (last, np.setdiff1d(idx, last))]
    est = OneVsRestSVC(**_svc_kw()) if multiclass else SVC(**_svc_kw())
    with pytest.raises(ValueError, match='miss a class'):
        CalibratedSVC(est, cv=splits).fit(X, y)


def test_an_svc_takes_two_classes():
    from optiml_amd.ml.svm import SVC, CalibratedSVC
    X, y = _blobs(30, 3)
    with pytest.raises(ValueError, match='more than two labels'):
        CalibratedSVC(SVC(**_svc_kw())).fit(X, y)


def test_exported_from_the_svm_package():
    from optiml_amd.ml import svm
    from optiml_amd.ml.svm.calibration import CalibratedSVC
    assert svm.CalibratedSVC is CalibratedSVC and 'CalibratedSVC' in svm.__all__


def test_calibration_abi_is_declared_exported_and_bound():
    from optiml_amd import build, _lib
    build.build()
    lib = _lib.load()
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(REPO, 'include', 'bcqp.h')).read(), flags=re.S)
    assert re.search(r'#define BQ_ABI_VERSION 3\b', text)
    for s in NEW_SYMBOLS:
        assert re.search(r'\b%s\s*\(' % s, text), s
        assert hasattr(lib, s), s
        assert s in _lib.PROTOTYPES, s
    assert _lib.ABI_VERSION == 3 and lib.bq_abi_version() == 3
    for name in ('LINE_SEARCH', 'MAX_ITER', 'EMPTY'):
        value = int(re.search(r'#define BQ_PLATT_%s (\d+)' % name, text).group(1))
        assert getattr(_lib, 'PLATT_' + name) == value == getattr(pr, name)


def _platt_args(ncal=1, n=4):
    from optiml_amd import _lib
    d = lambda: np.zeros(ncal * n)   # noqa: E731
    out = [np.zeros(ncal), np.zeros(ncal), np.zeros(ncal, dtype=np.int32), np.zeros(ncal), np.zeros(ncal, dtype=np.int64),
           np.zeros(ncal, dtype=np.int64), np.zeros(ncal, dtype=np.int32)]
    i64 = C.POINTER(C.c_int64)
    ptrs = [_lib.ptr(out[0]), _lib.ptr(out[1]), _lib.iptr(out[2]), _lib.ptr(out[3]), out[4].ctypes.data_as(i64),
            out[5].ctypes.data_as(i64), _lib.iptr(out[6])]
    return d(), d(), out, ptrs


def test_null_arguments_are_bad_arguments():
    """What is decidable without a device: a NULL context or solver.  The empty sizes and the NULL arrays behind a live context are
    in the GPU file."""
    from optiml_amd import build, _lib
    build.build()
    lib = _lib.load()
    D, L, keep, ptrs = _platt_args()
    assert lib.bq_platt_fit(None, 1, 4, _lib.ptr(D), _lib.ptr(L), *ptrs) == _lib.ERR_BADARG
    assert b'NULL' in lib.bq_last_error()
    cal_of = np.zeros(1, dtype=np.int32)
    b, n_sv = np.zeros(1), np.zeros(1, dtype=np.int64)
    assert lib.bq_msolver_svc_heldout(None, 1, _lib.iptr(cal_of), _lib.ptr(b), n_sv.ctypes.data_as(C.POINTER(C.c_int64)), *ptrs,
                                      None) == _lib.ERR_BADARG
    assert b'NULL' in lib.bq_last_error()


def test_the_bounds_are_sixteen_times_the_recorded_measurements():
    import json
    rec = json.load(open(os.path.join(REPO, 'profiles', 'calibration', 'platt_parity.json')))
    assert pr.PLATT_MEASURED == rec['platt_max_rel_dev'] == max(rec['platt'].values()) and pr.PLATT_RTOL == 16 * pr.PLATT_MEASURED
    assert pr.DECISION_MEASURED == rec['decision_max_rel_dev'] == max(rec['decision'].values())
    assert pr.DECISION_RTOL == 16 * pr.DECISION_MEASURED
    assert rec['platt_max_rel_dev'] < 1e-9   # above that the deviation would be a defect to explain, not a tolerance
    assert len(rec['platt']) == 13


@pytest.mark.parametrize('flag,where', [('LINE_SEARCH', (1, 0)), ('MAX_ITER', (2, 0))])
def test_a_flagged_sigmoid_fit_warns_and_keeps_its_values(monkeypatch, flag, where):
    """libsvm's two warnings: a calibrator whose fit ended on a failed line search or the iteration cap produces a
    ConvergenceWarning that counts the calibrators and names the first, and its A and B are kept."""
    from types import SimpleNamespace
    from optiml_amd import _lib
    from optiml_amd.ml.svm import SVC, CalibratedSVC
    from optiml_amd.ml.svm import calibration
    from optiml_amd.ml.svm._base import ConvergenceWarning
    X, y = _blobs(30, 2)
    flags = np.zeros(3, dtype=np.int32)
    flags[where[0]] = getattr(_lib, 'PLATT_' + flag)
    cal = dict(A=np.array([-1., -2., -3.]), B=np.array([0.1, 0.2, 0.3]), iters=np.array([5, 6, 100], dtype=np.int32),
               loss=np.ones(3), flags=flags)
    monkeypatch.setattr(calibration, 'get_context', lambda: SimpleNamespace(world=1))
    monkeypatch.setattr(CalibratedSVC, '_fit_loop', lambda self, X, y, splits, rows: (['c0', 'c1', 'c2'], cal, None))
    est = CalibratedSVC(SVC(**_svc_kw(storage='f32')), cv=3)
    with pytest.warns(ConvergenceWarning, match=r'1 calibrator\(s\).*first: \(%d, %d\)' % where):
        est.fit(X, y)
    assert est.batched_ is False and est.batched_decision_ is False
    assert np.array_equal(est.calibrators_['flags'].ravel(), flags) and est.calibrators_['A'].shape == (3, 1)
    assert [c.A[0] for c in est.calibrated_classifiers_] == [-1., -2., -3.]
    cal['flags'] = np.zeros(3, dtype=np.int32)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        est.fit(X, y)   # no flag, no warning
