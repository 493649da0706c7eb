"""CPU checks of the batched SMO: which configurations take it, the dispatch by column count, the memory cap, and the C ABI of
`bq_msmo_*` — declared, exported, bound, and refusing NULL arguments before any device call (no GPU needed)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ['bq_msmo_create', 'bq_msmo_run', 'bq_msmo_get', 'bq_msmo_destroy']


def _svc_rows():
    from optiml_amd.ml.svm.losses import hinge, squared_hinge
    from optiml_amd.ml.svm.smo import SMO
    from optiml_amd.opti.constrained import ProjectedGradient
    base = dict(loss=hinge, dual=True, reg_intercept=False, optimizer='smo')
    return [
        (dict(base), 1, True),
        (dict(base, optimizer=SMO), 1, True),
        (dict(base, storage='f32'), 1, True),
        (dict(base, storage='stream'), 1, False),
        (dict(base), 2, False),
        (dict(base, reg_intercept=True), 1, False),
        (dict(base, loss=squared_hinge), 1, False),
        (dict(base, dual=False), 1, False),
        (dict(base, optimizer=ProjectedGradient, reg_intercept=True), 1, False),
    ]


@pytest.mark.parametrize('row', range(9))
def test_which_svc_configurations_batch(row):
    from optiml_amd.ml.svm import SVC
    from optiml_amd.ml.svm.multiclass import uses_batched_smo_path, uses_batched_path
    kw, world, want = _svc_rows()[row]
    assert uses_batched_smo_path(SVC(**kw), world) is want
    if want:
        assert uses_batched_path(SVC(**kw), world) is False   # the regularised-intercept path is another one


def _svr_rows():
    from optiml_amd.ml.svm.losses import epsilon_insensitive, squared_epsilon_insensitive
    from optiml_amd.ml.svm.smo import SMO
    base = dict(loss=epsilon_insensitive, dual=True, reg_intercept=False, optimizer='smo')
    return [
        (dict(base), 1, True),
        (dict(base, optimizer=SMO), 1, True),
        (dict(base, storage='f32'), 1, True),
        (dict(base, storage='stream'), 1, False),
        (dict(base), 2, False),
        (dict(base, reg_intercept=True), 1, False),
        (dict(base, loss=squared_epsilon_insensitive), 1, False),
    ]


@pytest.mark.parametrize('row', range(7))
def test_which_svr_configurations_batch(row):
    from optiml_amd.ml.svm import SVR
    from optiml_amd.ml.svm.multioutput import uses_batched_smo_svr_path
    kw, world, want = _svr_rows()[row]
    assert uses_batched_smo_svr_path(SVR(**kw), world) is want


def test_dispatch_by_column_count_and_by_force():
    from optiml_amd.ml.svm import _batched
    m = _batched.SMO_MIN_COLUMNS
    assert isinstance(m, int) and m >= 1
    assert _batched.takes_batched_smo(m) is True and _batched.takes_batched_smo(m - 1) is False
    assert _batched.takes_batched_smo(1, force=True) is True and _batched.takes_batched_smo(10 ** 6, force=False) is False


def test_memory_cap():
    from optiml_amd import _lib
    from optiml_amd.ml.svm._batched import MAX_COLUMNS, MEMORY_SHARE, smo_column_bytes, smo_column_cap
    assert smo_column_bytes(1000, _lib.SVC) == 36000 and smo_column_bytes(1000, _lib.SVR) == 44000
    free = 10 ** 9
    assert smo_column_cap(100000, _lib.SVC, free) == int(free * MEMORY_SHARE) // 3600000
    assert smo_column_cap(100000, _lib.SVR, free) == int(free * MEMORY_SHARE) // 4400000
    assert smo_column_cap(100, _lib.SVC, free) == MAX_COLUMNS
    assert smo_column_cap(10 ** 7, _lib.SVR, 1000) == 1   # never 0: a column too large fails in the library, with its message


def test_abi_is_declared_exported_and_bound():
    from optiml_amd import build, _lib
    build.build()
    lib = _lib.load()
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(REPO, 'include', 'bcqp.h')).read(), flags=re.S)
    for s in SYMBOLS:
        assert re.search(r'\b%s\s*\(' % s, text), s
        assert hasattr(lib, s), s
        assert s in _lib.PROTOTYPES, s
    m = re.search(r'int\s+bq_msmo_create\s*\(([^)]*)\)', text)
    args = [a.strip() for a in m.group(1).split(',')]
    assert [a.replace(' ', '').rstrip('abcdefghijklmnopqrstuvwxyzCY_') if '*' in a else a.split()[0] for a in args] == [
        'bq_problem*', 'int', 'int', 'constdouble*', 'constdouble*', 'constdouble*', 'double', 'constint64_t*', 'constint32_t*',
        'bq_msmo**']
    _dp, _vp, _i64 = C.POINTER(C.c_double), C.c_void_p, C.c_int64
    assert _lib.PROTOTYPES['bq_msmo_create'][1] == [_vp, C.c_int, C.c_int, _dp, _dp, _dp, C.c_double, C.POINTER(_i64),
                                                    C.POINTER(C.c_int32), C.POINTER(_vp)]
    assert _lib.PROTOTYPES['bq_msmo_run'][1] == [_vp, _i64, C.POINTER(_i64), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    assert _lib.PROTOTYPES['bq_msmo_get'][1] == [_vp, C.c_int, C.c_int, _dp]
    assert _lib.PROTOTYPES['bq_msmo_destroy'][1] == [_vp]


def test_null_arguments_are_refused_before_any_device_call():
    from optiml_amd import build, _lib
    build.build()
    lib = _lib.load()
    y, c = np.ones(4), np.ones(1)
    h = C.c_void_p()
    outer, flag = C.c_int64(0), C.c_int(0)
    assert lib.bq_msmo_create(None, _lib.SVC, 1, _lib.ptr(y), _lib.ptr(c), None, 1e-3, None, None, C.byref(h)) == _lib.ERR_BADARG
    assert b'NULL' in lib.bq_last_error() and not h.value
    assert lib.bq_msmo_run(None, 1, C.byref(outer), C.byref(flag), C.byref(flag)) == _lib.ERR_BADARG
    assert lib.bq_msmo_get(None, 0, _lib.SMO_ALPHAS, _lib.ptr(y)) == _lib.ERR_BADARG
    assert lib.bq_msmo_destroy(None) == _lib.OK


def test_search_predicate_and_planning():
    from optiml_amd.ml.svm import SVC, OneVsRestSVC, OneVsOneSVC
    from optiml_amd.ml.svm.kernels import GaussianKernel
    from optiml_amd.ml.svm.losses import hinge
    from optiml_amd.ml.svm.model_selection import plan_smo_columns, uses_batched_smo_search
    kw = dict(loss=hinge, dual=True, optimizer='smo', kernel=GaussianKernel(gamma=0.5))
    assert uses_batched_smo_search(SVC(**kw), [{'C': 1.}, {'kernel': GaussianKernel(gamma=1.)}], 1) is True
    assert uses_batched_smo_search(OneVsRestSVC(**kw), [{'C': 1.}], 1) is True
    assert uses_batched_smo_search(SVC(**kw), [{'C': 1.}], 2) is False
    assert uses_batched_smo_search(SVC(**kw), [{'tol': 1e-2}], 1) is False
    assert uses_batched_smo_search(OneVsOneSVC(**kw), [{'C': 1.}], 1) is False
    assert uses_batched_smo_search(SVC(**dict(kw, reg_intercept=True)), [{'C': 1.}], 1) is False
    rs = np.random.RandomState(0)
    X = rs.standard_normal((30, 3))
    y = (np.arange(30) // 2) % 3
    idx = np.arange(30)
    splits = [(rs.permutation(np.setdiff1d(idx, idx[f::3])), idx[f::3]) for f in range(3)]   # training rows in any order
    cands = [{'C': 0.1}, {'C': 10.}]
    groups, folds = plan_smo_columns(X, y, splits, cands, 1., GaussianKernel(gamma=0.5), True)
    assert len(groups) == 1 and len(groups[0]['cols']) == 2 * 3 * 3 and groups[0]['Y'].shape == (18, 30)
    for (ci, f, r, C_), Yc, rows in zip(groups[0]['cols'], groups[0]['Y'], groups[0]['rows']):
        assert C_ == cands[ci]['C']
        assert np.all(np.diff(rows) > 0) and np.array_equal(rows, np.sort(splits[f][0]))
        assert np.array_equal(Yc, np.where(y == folds[f][1][r], 1., -1.))
    # binary labels: one column per (candidate, fold); a string gamma: one panel per fold
    yb = (np.arange(30) // 3) % 2
    groups, _ = plan_smo_columns(X, yb, splits, cands, 1., GaussianKernel(gamma='scale'), False)
    assert len(groups) == 3 and all(len(g['cols']) == 2 for g in groups)
    # a fold whose training rows miss a class: no plan
    miss = [(np.flatnonzero(y != 2), np.flatnonzero(y == 2))] + splits[1:]
    assert plan_smo_columns(X, y, miss, cands, 1., GaussianKernel(gamma=0.5), True) is None
