"""CPU checks of the held-out scoring of batched SMO columns: which configurations `SVRGridSearchCV` and `CalibratedSVC` take onto it
(and that the PG / FW predicates still answer as before), the SVR planner's groups, row lists and sets, the column cap's
arithmetic, the C ABI of `bq_msmo_svr_heldout` / `bq_msmo_svc_heldout` — declared, exported, bound, and refusing NULL arguments
before any device call — and that the inputs of tests/test_gpu_smo_heldout.py meet the solver's conditions (no GPU needed)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ['bq_msmo_svr_heldout', 'bq_msmo_svc_heldout']


def _svr(**over):
    from optiml_amd.ml.svm import SVR
    from optiml_amd.ml.svm.kernels import GaussianKernel
    from optiml_amd.ml.svm.losses import epsilon_insensitive
    return SVR(**dict(dict(loss=epsilon_insensitive, dual=True, reg_intercept=False, optimizer='smo', kernel=GaussianKernel(gamma=0.5)),
                      **over))


def _svc_kw(**over):
    from optiml_amd.ml.svm.kernels import GaussianKernel
    from optiml_amd.ml.svm.losses import hinge
    return dict(dict(loss=hinge, dual=True, reg_intercept=False, optimizer='smo', kernel=GaussianKernel(gamma=0.5)), **over)


def _search_rows():
    from optiml_amd.ml.svm import SVC
    from optiml_amd.ml.svm.kernels import GaussianKernel, linear
    from optiml_amd.ml.svm.losses import squared_epsilon_insensitive
    from optiml_amd.ml.svm.smo import SMO
    from optiml_amd.opti.constrained import ProjectedGradient
    grid = [{'C': 1.0}]
    return [
        (_svr(), grid, 1, True),
        (_svr(optimizer=SMO), [{'C': 1.0, 'epsilon': 0.2}], 1, True),
        (_svr(), [{'kernel': GaussianKernel(gamma=2.)}, {'kernel': linear}], 1, True),
        (_svr(reg_intercept=True), grid, 1, False),
        (_svr(), grid, 2, False),                                            # world 2
        (_svr(storage='f32'), grid, 1, False),                               # an fp32 panel keeps the per-fold calls
        (_svr(storage='stream'), grid, 1, False),
        (_svr(kernel=GaussianKernel(gamma='scale')), grid, 1, False),        # a string gamma, on the base kernel ...
        (_svr(), [{'kernel': GaussianKernel(gamma='scale')}], 1, False),     # ... or on a candidate's
        (_svr(), [{'C': 1.0, 'tol': 1e-2}], 1, False),                       # a foreign grid key
        (_svr(loss=squared_epsilon_insensitive), grid, 1, False),
        (_svr(optimizer=ProjectedGradient, reg_intercept=True), grid, 1, False),   # a PG estimator: the other batched search
        (SVC(**_svc_kw()), grid, 1, False),
    ]


@pytest.mark.parametrize('row', range(13))
def test_which_searches_take_the_batched_smo_path(row):
    from optiml_amd.ml.svm.model_selection import uses_batched_smo_svr_search, uses_batched_svr_search
    est, grid, world, want = _search_rows()[row]
    assert uses_batched_smo_svr_search(est, grid, world) is want
    if want:
        assert uses_batched_svr_search(est, grid, world) is False   # the PG / FW search's predicate stays as it is


def test_the_pg_search_predicate_is_untouched():
    from optiml_amd.ml.svm.model_selection import uses_batched_smo_svr_search, uses_batched_svr_search
    from optiml_amd.opti.constrained import ProjectedGradient
    pg = _svr(optimizer=ProjectedGradient, reg_intercept=True)
    assert uses_batched_svr_search(pg, [{'C': 1.0}], 1) is True and uses_batched_smo_svr_search(pg, [{'C': 1.0}], 1) is False
    assert uses_batched_svr_search(_svr(), [{'C': 1.0}], 1) is False


def _calibration_rows():
    from optiml_amd.ml.svm import SVC, OneVsOneSVC, OneVsRestSVC
    from optiml_amd.ml.svm.kernels import GaussianKernel
    from optiml_amd.ml.svm.losses import squared_hinge
    from optiml_amd.opti.constrained import ProjectedGradient
    return [
        (SVC(**_svc_kw()), 1, True),
        (OneVsRestSVC(**_svc_kw()), 1, True),
        (SVC(**_svc_kw(reg_intercept=True)), 1, False),
        (OneVsRestSVC(**_svc_kw()), 2, False),
        (SVC(**_svc_kw(storage='f32')), 1, False),
        (OneVsRestSVC(**_svc_kw(kernel=GaussianKernel(gamma='scale'))), 1, False),
        (SVC(**_svc_kw(loss=squared_hinge)), 1, False),
        (SVC(**_svc_kw(optimizer=ProjectedGradient, reg_intercept=True)), 1, False),   # the PG estimator: the other batched path
        (OneVsOneSVC(**_svc_kw()), 1, False),
        (_svr(), 1, False),
    ]


@pytest.mark.parametrize('row', range(10))
def test_which_calibrations_take_the_batched_smo_path(row):
    from optiml_amd.ml.svm.calibration import uses_batched_calibration, uses_batched_smo_calibration
    est, world, want = _calibration_rows()[row]
    assert uses_batched_smo_calibration(est, world) is want
    if want:
        assert uses_batched_calibration(est, world) is False   # the PG / FW calibration's predicate stays as it is


def test_the_pg_calibration_predicate_is_untouched():
    from optiml_amd.ml.svm import SVC
    from optiml_amd.ml.svm.calibration import uses_batched_calibration, uses_batched_smo_calibration
    from optiml_amd.opti.constrained import ProjectedGradient
    pg = SVC(**_svc_kw(optimizer=ProjectedGradient, reg_intercept=True))
    assert uses_batched_calibration(pg, 1) is True and uses_batched_smo_calibration(pg, 1) is False


def test_the_estimators_carry_the_dispatch_switch_and_export_the_predicates():
    from optiml_amd.ml.svm import CalibratedSVC, SVRGridSearchCV, calibration, model_selection
    assert SVRGridSearchCV.batch_smo is None and CalibratedSVC.batch_smo is None
    assert 'uses_batched_smo_svr_search' in model_selection.__all__ and 'plan_smo_svr_columns' in model_selection.__all__
    assert 'uses_batched_smo_calibration' in calibration.__all__


def _splits(n, k):
    idx = np.arange(n)
    return [(np.setdiff1d(idx, idx[f::k]), idx[f::k]) for f in range(k)]


def test_plan_smo_svr_columns_groups_row_lists_and_sets():
    from optiml_amd.ml.svm.kernels import GaussianKernel, LinearKernel
    from optiml_amd.ml.svm.model_selection import parameter_grid, plan_smo_svr_columns
    n = 15
    rng = np.random.default_rng(0)
    X, y = rng.standard_normal((n, 3)), rng.standard_normal(n)
    splits = [(rng.permutation(tr), te) for tr, te in _splits(n, 3)]   # training rows in any order
    cands = parameter_grid({'epsilon': [0.05, 0.2], 'C': [0.5, 2.0]})
    groups = plan_smo_svr_columns(X, y, splits, cands, 1.0, 0.1, GaussianKernel(gamma=0.3))
    assert len(groups) == 1
    g = groups[0]
    assert g['Y'].shape == (12, n) and len(g['rows']) == 12
    assert [c[:2] for c in g['cols']] == [(ci, f) for ci in range(4) for f in range(3)]
    for (ci, f, C_, eps), Yc, rows in zip(g['cols'], g['Y'], g['rows']):
        assert C_ == cands[ci]['C'] and eps == cands[ci]['epsilon']
        assert np.array_equal(Yc, y)                                  # the held rows' targets are what the scorer compares with
        assert np.all(np.diff(rows) > 0) and np.array_equal(rows, np.sort(splits[f][0]))
        assert not np.intersect1d(rows, splits[f][1]).size            # the fold's set (its test rows) is off the list
    # base values, and one group per resolved kernel
    groups = plan_smo_svr_columns(X, y, splits, parameter_grid({'kernel': [GaussianKernel(gamma=0.3), LinearKernel()]}), 3.0, 0.25,
                                  GaussianKernel())
    assert len(groups) == 2 and all(len(g['cols']) == 3 for g in groups)
    assert all(c[2:] == (3.0, 0.25) for g in groups for c in g['cols'])
    # no plan for folds that are no row lists: a repeated training row, a repeated test row, a row both trained on and tested
    tr, te = splits[0]
    for bad in ((np.append(tr, tr[0]), te), (tr, np.append(te, te[0])), (np.append(tr, te[0]), te)):
        assert plan_smo_svr_columns(X, y, [bad] + splits[1:], cands, 1.0, 0.1, GaussianKernel(gamma=0.3)) is None


def test_the_column_cap_counts_the_scoring_scratch():
    from optiml_amd import _lib
    from optiml_amd.ml.svm._batched import MAX_COLUMNS, MEMORY_SHARE, smo_column_bytes, smo_column_cap, smo_heldout_column_cap
    n, free, slab = 100000, 10 ** 9, 16 * 391 * 391 * 256 * 8 // 1000
    vec = 8 * (n + 256)
    budget = int(free * MEMORY_SHARE) - slab - 2 * 15 * vec
    assert smo_heldout_column_cap(n, _lib.SVR, free, slab) == budget // (smo_column_bytes(n, _lib.SVR) + 2 * vec)
    assert smo_heldout_column_cap(n, _lib.SVC, free, slab) == budget // (smo_column_bytes(n, _lib.SVC) + 2 * vec)
    assert smo_heldout_column_cap(n, _lib.SVC, free, slab, calibrators=True) == budget // (smo_column_bytes(n, _lib.SVC) + 4 * vec)
    # two n-vectors of doubles per column on top of the walker's state: fewer columns than the solver alone would take
    assert smo_heldout_column_cap(n, _lib.SVR, free, slab) < smo_column_cap(n, _lib.SVR, free)
    assert 2 * vec >= 16 * n
    assert smo_heldout_column_cap(100, _lib.SVR, free, 0) == MAX_COLUMNS
    assert smo_heldout_column_cap(10 ** 7, _lib.SVR, 1000, slab) == 1   # never 0: a column too large fails in the library


def _prototype_of(text, name):
    m = re.search(r'int\s+%s\s*\(([^)]*)\)' % name, text)
    args = [a.strip() for a in m.group(1).split(',')]
    return [re.sub(r'\s*\w+$', '', a).replace(' ', '') for a in args]


def test_abi_is_declared_exported_and_bound():
    from optiml_amd import build, _lib
    build.build()
    lib = _lib.load()
    raw = open(os.path.join(REPO, 'include', 'bcqp.h')).read()
    assert '(still 3: bq_msmo_svr_heldout and bq_msmo_svc_heldout were added; nothing existing changed)' in raw
    text = re.sub(r'/\*.*?\*/', '', raw, flags=re.S)
    assert re.search(r'#define BQ_ABI_VERSION 3\b', text) and _lib.ABI_VERSION == 3 and lib.bq_abi_version() == 3
    for s in SYMBOLS:
        assert re.search(r'\b%s\s*\(' % s, text), s
        assert hasattr(lib, s), s
        assert s in _lib.PROTOTYPES, s
    assert _prototype_of(text, 'bq_msmo_svr_heldout') == ['bq_msmo*', 'int', 'constint*', 'constunsignedchar*', 'double*', 'int64_t*',
                                                          'double*', 'int64_t*']
    assert _prototype_of(text, 'bq_msmo_svc_heldout') == ['bq_msmo*', 'int', 'constint*', 'constunsignedchar*', 'int', 'constint*',
                                                          'double*', 'int64_t*', 'double*', 'double*', 'int*', 'double*', 'int64_t*',
                                                          'int64_t*', 'int*', 'double*']
    dp, ip, vp, i64p, u8p = C.POINTER(C.c_double), C.POINTER(C.c_int), C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_ubyte)
    assert _lib.PROTOTYPES['bq_msmo_svr_heldout'] == (C.c_int, [vp, C.c_int, ip, u8p, dp, i64p, dp, i64p])
    assert _lib.PROTOTYPES['bq_msmo_svc_heldout'] == (C.c_int, [vp, C.c_int, ip, u8p, C.c_int, ip, dp, i64p, dp, dp, ip, dp, i64p, i64p,
                                                                ip, dp])


def test_null_arguments_are_refused_before_any_device_call():
    from optiml_amd import build, _lib
    build.build()
    lib = _lib.load()
    v, i = np.ones(4), np.zeros(4, dtype=np.int32)
    i64 = np.zeros(4, dtype=np.int64).ctypes.data_as(C.POINTER(C.c_int64))
    u8 = np.zeros(4, dtype=np.uint8).ctypes.data_as(C.POINTER(C.c_ubyte))
    assert lib.bq_msmo_svr_heldout(None, 1, _lib.iptr(i), u8, _lib.ptr(v), i64, _lib.ptr(v), i64) == _lib.ERR_BADARG
    assert b'NULL' in lib.bq_last_error()
    assert lib.bq_msmo_svc_heldout(None, 1, _lib.iptr(i), u8, 1, _lib.iptr(i), _lib.ptr(v), i64, _lib.ptr(v), _lib.ptr(v), _lib.iptr(i),
                                   _lib.ptr(v), i64, i64, _lib.iptr(i), None) == _lib.ERR_BADARG
    assert b'NULL' in lib.bq_last_error()


def test_the_gpu_file_s_inputs_meet_the_solver_s_conditions():
    """every fold's training list has at least two rows; for the classification input every fold's training rows hold both labels
    of every class column; the targets lie inside the epsilon that is meant to be above their range; row 0 and the last row are
    held by some fold"""
    import test_gpu_smo_heldout as gpu
    from optiml_amd.datasets import make_multiclass_blobs
    for n in gpu.SIZES:
        folds = gpu._folds(n)
        held = gpu._held(n)
        assert held.sum(axis=0).tolist() == [1] * n and held[:, 0].any() and held[:, -1].any()
        _, y = gpu._data(n)
        assert np.ptp(y) < gpu.BIG_EPS and np.abs(y).max() < 2.
        _, codes = make_multiclass_blobs(n, 5, 3, seed=3)
        for tr, te in folds:
            assert len(tr) >= 2 and len(te) >= 1 and not np.intersect1d(tr, te).size and np.all(np.diff(tr) > 0)
            for cls in range(3):
                assert 0 < int((codes[tr] == cls).sum()) < len(tr)
        for k in gpu.COUNTS:
            Cs, eps, set_of, rows = gpu.svr_columns(n, k)
            assert len(Cs) == len(eps) == len(set_of) == len(rows) == k and min(Cs) > 0 and min(eps) >= 0
            Y, Cs, set_of, cal_of, ncal, rows = gpu.svc_columns(codes, k)
            assert Y.shape == (k, n) and set(np.unique(Y)) == {-1., 1.} and max(cal_of) == ncal - 1
            for cal in range(ncal):   # the columns of a calibrator score disjoint rows
                mine = [j for j in range(k) if cal_of[j] == cal and set_of[j] >= 0]
                assert len({set_of[j] for j in mine}) == len(mine)
    # the binary problem of the calibration test: class 2 against the rest
    _, codes = make_multiclass_blobs(240, 5, 3, seed=3)
    for tr, _ in gpu._folds(240):
        assert 0 < int((codes[tr] == 2).sum()) < len(tr)
