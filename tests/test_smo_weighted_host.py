"""Host side of sample_weight / class_weight in SMO (no GPU): the test-side reference with one box per row
(tests/smo_weighted_reference.py) against the oracle on a constant box and against sklearn on weighted problems, the box helper
against sklearn's compute_class_weight, the batched-path predicates under a class_weight, and the C ABI of the two new entry points.
"""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import smo_weighted_reference as wr
from conftest import load_golden
from oracle import smo_oracle as smo
from oracle import svm_oracle as so

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-3
SVC_FIELDS = ('alphas', 'b', 'iter', 'b_up', 'b_low', 'errors', 'steps', 'finished')
SVR_FIELDS = ('alphas_p', 'alphas_n') + SVC_FIELDS[1:]


@pytest.fixture(scope='module')
def svc200():
    g = load_golden('smo.npz')
    X, y = g['svc200_X'], g['svc200_y']
    return so.gram('rbf', X), np.where(y == np.unique(y)[-1], 1., -1.)


@pytest.fixture(scope='module')
def svr150():
    g = load_golden('smo.npz')
    return so.gram('rbf', g['svr150_X']), g['svr150_y']


# ---- 1. a constant box is the oracle, bit for bit --------------------------------------------------------------------------------
@pytest.mark.parametrize('Cv', [0.1, 1., 10.])
@pytest.mark.parametrize('tie', ['set', 'index'])
def test_constant_box_is_the_oracle_bit_for_bit(svc200, svr150, tie, Cv):
    K, yb = svc200
    ref = smo.smo_svc(K, yb, C=Cv, tol=TOL, tie=tie)
    got = wr.smo_svc_weighted(K, yb, Cv * np.ones(len(yb)), tol=TOL, tie=tie)
    for f in SVC_FIELDS:
        assert np.array_equal(got[f], ref[f]), ('svc', f)
    K, y = svr150
    ref = smo.smo_svr(K, y, C=Cv, epsilon=0.1, tol=TOL, tie=tie)
    got = wr.smo_svr_weighted(K, y, Cv * np.ones(len(y)), epsilon=0.1, tol=TOL, tie=tie)
    for f in SVR_FIELDS:
        assert np.array_equal(got[f], ref[f]), ('svr', f)


# ---- 2. the reference on weighted problems ---------------------------------------------------------------------------------------
def svc_gap(K, yb, a, Cw):
    """b_low - b_up recomputed from the multipliers and K alone: F_i = sum_j a_j y_j K_ij - y_i, b_up its minimum over libsvm's up
    set {y = +1, a < C_i} u {y = -1, a > 0}, b_low its maximum over the low set {y = +1, a > 0} u {y = -1, a < C_i}"""
    F = K @ (a * yb) - yb
    up = ((yb == 1) & (a < Cw)) | ((yb == -1) & (a > 0))
    low = ((yb == 1) & (a > 0)) | ((yb == -1) & (a < Cw))
    return F[low].max() - F[up].min()


def svr_gap(K, y, ap, an, Cw, eps):
    """the same for regression (Shevade et al.): F_i = y_i - sum_j (a+_j - a-_j) K_ij.  The KKT conditions of the dual with the
    multiplier b of sum (a+ - a-) = 0: a+_i may grow (a+_i < C_i) only if F_i - eps <= b and a-_i may shrink (a-_i > 0) only if
    F_i + eps <= b — the candidates of b_low; a+_i may shrink (a+_i > 0) only if F_i - eps >= b and a-_i may grow (a-_i < C_i)
    only if F_i + eps >= b — the candidates of b_up"""
    F = y - K @ (ap - an)
    low = np.concatenate((F[ap < Cw] - eps, F[an > 0] + eps))
    up = np.concatenate((F[ap > 0] - eps, F[an < Cw] + eps))
    return low.max() - up.min()


def svc_objective(K, yb, a):
    c = a * yb
    return 0.5 * c @ K @ c - a.sum()


def svr_objective(K, y, ap, an, eps):
    beta = ap - an
    return 0.5 * beta @ K @ beta - y @ beta + eps * (ap + an).sum()


def test_weighted_svc_reference_is_tol_optimal_and_near_sklearn(svc200):
    from sklearn.svm import SVC as SkSVC
    K, yb = svc200
    # error-cache drift, measured on the unweighted oracle run of the same data: the reported b_low - b_up comes from cached
    # errors updated step by step, the recomputed one from a fresh product.  Measured here: 5.1e-16 (svc200, RBF, C = 1).
    plain = smo.smo_svc(K, yb, C=1., tol=TOL, tie='index')
    drift = abs(svc_gap(K, yb, plain['alphas'], np.ones(len(yb))) - (plain['b_low'] - plain['b_up']))
    print('svc200 error-cache drift', drift)
    Cw = np.where(yb == 1, 5., 1.)   # a two-valued class box, ratio 5
    for tie in ('set', 'index'):
        r = wr.smo_svc_weighted(K, yb, Cw, tol=TOL, tie=tie)
        a = r['alphas']
        assert r['finished'] and (a >= 0).all() and (a <= Cw).all() and abs(a @ yb) < 1e-9
        assert (a > 1.).any()   # the larger box is used
        gap = svc_gap(K, yb, a, Cw)
        print(tie, 'recomputed violation', gap, 'bound', 2 * TOL + 10 * drift)
        assert gap <= 2 * TOL + 10 * drift
        sk = SkSVC(kernel='precomputed', C=1., class_weight={1.: 5., -1.: 1.}, tol=1e-8).fit(K, yb)
        a_sk = np.zeros(len(yb))
        a_sk[sk.support_] = np.abs(sk.dual_coef_[0])
        f, f_sk = svc_objective(K, yb, a), svc_objective(K, yb, a_sk)
        print(tie, 'objective', f, 'sklearn', f_sk, 'slack', 2 * TOL * Cw.sum())
        # derived, not measured: for a point whose violation is <= 2 tol, f - f* <= grad f' (a - a*) <= 2 tol sum_i C_i
        assert f <= f_sk + 2 * TOL * Cw.sum()


def test_weighted_svr_reference_is_tol_optimal_and_near_sklearn(svr150):
    from sklearn.svm import SVR as SkSVR
    K, y = svr150
    n = len(y)
    # error-cache drift on the unweighted oracle run of the same data.  Measured here: 5.6e-17 (svr150, RBF, C = 1, epsilon = 0.1).
    plain = smo.smo_svr(K, y, C=1., epsilon=0.1, tol=TOL, tie='index')
    drift = abs(svr_gap(K, y, plain['alphas_p'], plain['alphas_n'], np.ones(n), 0.1) - (plain['b_low'] - plain['b_up']))
    print('svr150 error-cache drift', drift)
    sw = np.random.RandomState(3).uniform(0.05, 20., n)
    for tie in ('set', 'index'):
        r = wr.smo_svr_weighted(K, y, sw, epsilon=0.1, tol=TOL, tie=tie)
        ap, an = r['alphas_p'], r['alphas_n']
        assert r['finished'] and (ap >= 0).all() and (an >= 0).all() and (ap <= sw).all() and (an <= sw).all()
        assert abs((ap - an).sum()) < 1e-9 and (np.maximum(ap, an) > 1.).any()
        gap = svr_gap(K, y, ap, an, sw, 0.1)
        print(tie, 'recomputed violation', gap, 'bound', 2 * TOL + 10 * drift)
        assert gap <= 2 * TOL + 10 * drift
        sk = SkSVR(kernel='precomputed', C=1., epsilon=0.1, tol=1e-8).fit(K, y, sample_weight=sw)
        beta = np.zeros(n)
        beta[sk.support_] = sk.dual_coef_[0]
        f, f_sk = svr_objective(K, y, ap, an, 0.1), svr_objective(K, y, np.maximum(beta, 0), np.maximum(-beta, 0), 0.1)
        print(tie, 'objective', f, 'sklearn', f_sk, 'slack', 2 * TOL * sw.sum())
        assert f <= f_sk + 2 * TOL * sw.sum()


# ---- 3. the box helper ------------------------------------------------------------------------------------------------------------
def test_row_boxes_equal_sklearns_class_weights_times_sample_weight():
    from sklearn.utils.class_weight import compute_class_weight
    from optiml_amd.ml.svm._base import row_boxes
    rs = np.random.RandomState(0)
    y = rs.choice([2, 5, 9], size=60, p=[0.6, 0.3, 0.1])
    classes = np.unique(y)
    codes = np.searchsorted(classes, y)
    sw = rs.uniform(0., 3., 60)
    sw[::7] = 0.
    assert row_boxes(2.5, y, classes) is None
    for cw in ({5: 3.}, {2: 0.5, 9: 7.}, 'balanced'):
        w = compute_class_weight(cw, classes=classes, y=y)
        assert np.array_equal(row_boxes(2.5, y, classes, cw), 2.5 * w[codes]), cw
        assert np.array_equal(row_boxes(2.5, y, classes, cw, sw), 2.5 * sw * w[codes]), cw
    assert np.array_equal(row_boxes(2.5, y, classes, None, sw), 2.5 * sw)
    assert np.array_equal(row_boxes(2.5, sample_weight=sw), 2.5 * sw)
    for bad in ({4: 1.}, {5: -1.}, {5: float('nan')}, {5: 0.}, {5: float('inf')}, 'auto', 3.):
        with pytest.raises(ValueError):
            row_boxes(1., y, classes, bad)
    for bad in (-sw, np.where(sw > 1, np.nan, sw), np.zeros(60), sw[:-1], np.where(sw > 1, np.inf, sw)):
        with pytest.raises(ValueError):
            row_boxes(1., y, classes, None, bad)


def test_weights_that_empty_a_class_and_bad_arguments_raise_before_any_device_work():
    from optiml_amd.ml.svm import SVC, SVR, OneVsRestSVC, OneVsOneSVC
    from optiml_amd.ml.svm.losses import hinge, epsilon_insensitive
    rs = np.random.RandomState(1)
    X, y = rs.standard_normal((20, 3)), np.arange(20) % 2
    kw = dict(loss=hinge, dual=True, optimizer='smo')
    with pytest.raises(ValueError, match='without rows'):
        SVC(**kw).fit(X, y, sample_weight=(y == 0).astype(float))
    with pytest.raises(ValueError, match='not among the classes'):
        SVC(class_weight={7: 2.}, **kw).fit(X, y)
    with pytest.raises(ValueError):
        SVC(class_weight='auto', **kw)
    with pytest.raises(ValueError):
        SVC(**kw).fit(X, y, sample_weight=-np.ones(20))
    with pytest.raises(ValueError):
        SVR(loss=epsilon_insensitive, dual=True, optimizer='smo').fit(X, y.astype(float), sample_weight=np.zeros(20))
    est = SVC(class_weight='balanced', **kw)
    assert est.get_params()['class_weight'] == 'balanced' and list(inspect.signature(SVC).parameters)[-1] == 'class_weight'
    assert list(inspect.signature(OneVsRestSVC).parameters) == list(inspect.signature(SVC).parameters)
    assert OneVsRestSVC(class_weight='balanced', **kw)._prototype().class_weight == 'balanced'
    y3 = np.arange(20) % 3
    with pytest.raises(ValueError, match="None or 'balanced'"):
        OneVsRestSVC(class_weight={0: 2.}, **kw).fit(X, y3)
    with pytest.raises(ValueError, match='not among the classes'):
        OneVsOneSVC(class_weight={7: 2.}, **kw).fit(X, y3)
    pair = OneVsOneSVC(class_weight={2: 3.}, **kw)
    pair.classes_ = np.unique(y3)
    assert pair._pair_prototype(0, 2).class_weight == {0: 1., 1: 3.} and pair._pair_prototype(0, 1).class_weight == {0: 1., 1: 1.}


# ---- 4. the predicates --------------------------------------------------------------------------------------------------------------
def test_only_the_two_taught_paths_take_a_class_weight():
    from optiml_amd.ml.svm import (SVC, SVR, NuSVC, CalibratedSVC, OneVsOneNuSVC, OneVsOneSVC, OneVsRestSVC)   # noqa: F401
    from optiml_amd.ml.svm import _batched, calibration, coupling, model_selection, multiclass, multioutput, nu_ovo, nu_search
    from optiml_amd.ml.svm import onevsone, ovo_search
    from optiml_amd.ml.svm.kernels import GaussianKernel
    from optiml_amd.ml.svm.losses import hinge, epsilon_insensitive, Hinge, EpsilonInsensitive
    from optiml_amd.opti.constrained import ProjectedGradient
    from optiml_amd.opti.unconstrained.stochastic import Adam
    k = GaussianKernel(gamma=0.5)
    smo_kw = dict(loss=hinge, dual=True, optimizer='smo', kernel=k)
    pg_kw = dict(loss=hinge, dual=True, reg_intercept=True, optimizer=ProjectedGradient, kernel=k)
    al_kw = dict(loss=hinge, dual=True, optimizer=Adam, learning_rate=0.01, kernel=k)
    y = (np.arange(30) // 3) % 3   # every fold's training rows hold every class
    idx = np.arange(30)
    splits = [(np.setdiff1d(idx, idx[f::3]), idx[f::3]) for f in range(3)]
    grid = [{'C': 1.}]

    def svr(**kw):   # SVR takes no class_weight: the predicates read the attribute
        est = SVR(loss=epsilon_insensitive, dual=True, kernel=k, **{key: v for key, v in kw.items() if key != 'class_weight'})
        est.class_weight = kw.get('class_weight')
        return est

    def nu(cls, cw):
        est = cls(kernel=k)
        est.class_weight = cw
        return est

    others = [   # (predicate of an estimator with the given class_weight)
        lambda cw: multiclass.uses_batched_path(SVC(class_weight=cw, **pg_kw), 1),
        lambda cw: multiclass.uses_batched_lagrangian_path(SVC(class_weight=cw, **al_kw), 1, 100),
        lambda cw: onevsone.uses_batched_ovo(SVC(class_weight=cw, **pg_kw), 1),
        lambda cw: multioutput.uses_batched_svr_path(svr(class_weight=cw, reg_intercept=True, optimizer=ProjectedGradient), 1),
        lambda cw: multioutput.uses_batched_lagrangian_svr_path(svr(class_weight=cw, optimizer=Adam, learning_rate=0.01), 1, 100),
        lambda cw: multioutput.uses_batched_smo_svr_path(svr(class_weight=cw, optimizer='smo'), 1),
        lambda cw: model_selection.uses_batched_search(SVC(class_weight=cw, **pg_kw), grid, 1),
        lambda cw: model_selection.uses_batched_search(OneVsRestSVC(class_weight=cw, **pg_kw), grid, 1),
        lambda cw: model_selection.uses_batched_smo_search(SVC(class_weight=cw, **smo_kw), grid, 1),
        lambda cw: model_selection.uses_batched_smo_search(OneVsRestSVC(class_weight=cw, **smo_kw), grid, 1),
        lambda cw: model_selection.uses_batched_svr_search(svr(class_weight=cw, reg_intercept=True, optimizer=ProjectedGradient),
                                                           grid, 1),
        lambda cw: model_selection.uses_batched_smo_svr_search(svr(class_weight=cw, optimizer='smo'), grid, 1),
        lambda cw: ovo_search.uses_batched_ovo_search(OneVsOneSVC(class_weight=cw, **pg_kw), grid, splits, y, 1),
        lambda cw: ovo_search.uses_batched_ovo_smo_search(OneVsOneSVC(class_weight=cw, **smo_kw), grid, splits, y, 1),
        lambda cw: calibration.uses_batched_calibration(SVC(class_weight=cw, **pg_kw), 1),
        lambda cw: calibration.uses_batched_smo_calibration(OneVsRestSVC(class_weight=cw, **smo_kw), 1),
        lambda cw: coupling.uses_batched_coupling(OneVsOneSVC(class_weight=cw, **pg_kw), 1),
        lambda cw: nu_search.uses_batched_nu_search(nu(NuSVC, cw), [{'nu': 0.3}]),
        lambda cw: nu_ovo.uses_batched_ovo_nu(nu(OneVsOneNuSVC, cw), 1),
        lambda cw: _batched.uses_batched_smo(SVC(class_weight=cw, **smo_kw), Hinge, 1),
        lambda cw: _batched.uses_batched_smo(svr(class_weight=cw, optimizer='smo'), EpsilonInsensitive, 1),
        lambda cw: _batched.uses_batched_lagrangian(SVC(class_weight=cw, **al_kw), (Hinge,), 1, 100),
    ]
    for i, pred in enumerate(others):
        assert pred(None) is True, i            # the configuration is one the path takes ...
        assert pred('balanced') is False, i     # ... and a class_weight alone turns it away
    taught = [
        lambda cw: multiclass.uses_batched_smo_path(SVC(class_weight=cw, **smo_kw), 1),
        lambda cw: onevsone.uses_batched_ovo_smo(SVC(class_weight=cw, **smo_kw), 1),
    ]
    for pred in taught:
        assert pred(None) is True and pred('balanced') is True and pred({1: 2.}) is True
    # their existing conditions still hold
    assert multiclass.uses_batched_smo_path(SVC(class_weight='balanced', **smo_kw), 2) is False
    assert multiclass.uses_batched_smo_path(SVC(class_weight='balanced', **dict(smo_kw, reg_intercept=True)), 1) is False
    assert onevsone.uses_batched_ovo_smo(SVC(class_weight='balanced', **dict(smo_kw, kernel=GaussianKernel(gamma='scale'))), 1) is False


# ---- 5. the C ABI ------------------------------------------------------------------------------------------------------------------
def test_new_entry_points_are_declared_exported_and_bound():
    from optiml_amd import build, _lib
    build.build()
    lib = _lib.load()
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(REPO, 'include', 'bcqp.h')).read(), flags=re.S)
    assert re.search(r'#define BQ_ABI_VERSION 3\b', text) and lib.bq_abi_version() == 3

    def kinds(name):
        args = re.search(r'int\s+%s\s*\(([^)]*)\)' % name, text).group(1).split(',')
        return [re.sub(r'\s*\w+$', '', a.strip()).replace(' ', '') for a in args]
    assert kinds('bq_smo_create_weighted') == ['bq_problem*', 'int', 'constdouble*', 'constdouble*', 'double', 'double', 'bq_smo**']
    assert kinds('bq_msmo_create_weighted') == ['bq_problem*', 'int', 'int', 'constdouble*', 'constdouble*', 'constdouble*', 'double',
                                                'constint64_t*', 'constint32_t*', 'bq_msmo**']
    # the existing create calls keep their signatures
    assert kinds('bq_smo_create') == ['bq_problem*', 'int', 'constdouble*', 'double', 'double', 'double', 'bq_smo**']
    assert kinds('bq_msmo_create') == kinds('bq_msmo_create_weighted')
    _dp, _vp, _i64 = C.POINTER(C.c_double), C.c_void_p, C.c_int64
    assert _lib.PROTOTYPES['bq_smo_create_weighted'][1] == [_vp, C.c_int, _dp, _dp, C.c_double, C.c_double, C.POINTER(_vp)]
    assert _lib.PROTOTYPES['bq_msmo_create_weighted'][1] == _lib.PROTOTYPES['bq_msmo_create'][1]
    for s in ('bq_smo_create_weighted', 'bq_msmo_create_weighted'):
        assert hasattr(lib, s), s


def test_null_arguments_are_refused_before_any_device_call():
    """as tests/test_smo_batched_host.py does for bq_msmo_create: without a problem only the NULL checks can be reached on the
    host; the checks of the boxes themselves need a device problem and are in tests/test_gpu_smo_weighted.py"""
    from optiml_amd import build, _lib
    build.build()
    lib = _lib.load()
    y, cw = np.ones(4), np.ones(4)
    h = C.c_void_p()
    assert lib.bq_smo_create_weighted(None, _lib.SVC, _lib.ptr(y), _lib.ptr(cw), 0., 1e-3, C.byref(h)) == _lib.ERR_BADARG
    assert b'NULL' in lib.bq_last_error() and not h.value
    assert lib.bq_msmo_create_weighted(None, _lib.SVC, 1, _lib.ptr(y), _lib.ptr(cw), None, 1e-3, None, None,
                                       C.byref(h)) == _lib.ERR_BADARG
    assert b'NULL' in lib.bq_last_error() and not h.value
