"""CPU checks of SVRGridSearchCV: the C ABI of the per-column-box SVR solver and its held-out scoring, column planning, path
selection, the cv argument forms and the R^2 assembled from a held-out squared error (no GPU needed)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ['bq_msolver_create_svr_boxes', 'bq_msolver_svr_heldout']


def test_svr_cv_abi_is_declared_exported_and_bound():
    from optiml_amd import build, _lib
    build.build()
    lib = _lib.load()
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(REPO, 'include', 'bcqp.h')).read(), flags=re.S)
    assert re.search(r'#define BQ_ABI_VERSION 3\b', text)
    for s in NEW_SYMBOLS:
        assert re.search(r'\b%s\s*\(' % s, text), s
        assert hasattr(lib, s), s
        assert s in _lib.PROTOTYPES, s
    assert _lib.PROTOTYPES['bq_msolver_create_svr_boxes'] == _lib.PROTOTYPES['bq_msolver_create_svr']   # the same argument list
    assert _lib.ABI_VERSION == 3 and lib.bq_abi_version() == 3


def test_null_arguments_are_bad_arguments():
    from optiml_amd import build, _lib
    build.build()
    lib = _lib.load()
    v = np.ones(4)
    out = C.c_void_p()
    assert lib.bq_msolver_create_svr_boxes(None, _lib.PG, 1, _lib.ptr(v), _lib.ptr(v), None, 1e-6, 10, 0., C.byref(out)) == \
        _lib.ERR_BADARG
    assert b'NULL' in lib.bq_last_error() and not out.value
    i = np.zeros(1, dtype=np.int64).ctypes.data_as(C.POINTER(C.c_int64))
    assert lib.bq_msolver_svr_heldout(None, _lib.ptr(v), _lib.ptr(v), _lib.ptr(v), i, _lib.ptr(v), i) == _lib.ERR_BADARG
    assert b'NULL' in lib.bq_last_error()


def test_exported_from_the_svm_package():
    from optiml_amd.ml import svm
    from optiml_amd.ml.svm.model_selection import SVRGridSearchCV
    assert svm.SVRGridSearchCV is SVRGridSearchCV and 'SVRGridSearchCV' in svm.__all__


def _splits(n, k):
    idx = np.arange(n)
    return [(np.setdiff1d(idx, idx[f::k]), idx[f::k]) for f in range(k)]


def test_plan_svr_columns_boxes_linear_terms_and_order():
    from optiml_amd.ml.svm.kernels import GaussianKernel
    from optiml_amd.ml.svm.model_selection import parameter_grid, plan_svr_columns
    n = 12
    rng = np.random.default_rng(0)
    X, y = rng.standard_normal((n, 3)), rng.standard_normal(n)
    splits = _splits(n, 3)
    cands = parameter_grid({'epsilon': [0.05, 0.2], 'C': [0.5, 2.0]})
    assert cands == [{'C': 0.5, 'epsilon': 0.05}, {'C': 0.5, 'epsilon': 0.2}, {'C': 2.0, 'epsilon': 0.05}, {'C': 2.0, 'epsilon': 0.2}]
    groups = plan_svr_columns(X, y, splits, cands, 1.0, 0.1, GaussianKernel(gamma=0.3))
    assert len(groups) == 1
    g = groups[0]
    assert g['QL'].shape == g['UB'].shape == (4 * 3, 2 * n)
    assert [c[:2] for c in g['cols']] == [(ci, f) for ci in range(4) for f in range(3)]
    for j, (ci, f, C_, eps) in enumerate(g['cols']):
        assert C_ == cands[ci]['C'] and eps == cands[ci]['epsilon']
        tr, te = splits[f]
        for half in (0, n):
            assert np.all(g['UB'][j][half + tr] == C_) and np.all(g['UB'][j][half + te] == 0)
        assert np.array_equal(g['QL'][j], np.hstack((-y, y)) + eps)


def test_plan_svr_columns_base_values_and_kernel_groups():
    from optiml_amd.ml.svm.kernels import GaussianKernel, LinearKernel
    from optiml_amd.ml.svm.model_selection import parameter_grid, plan_svr_columns
    n = 12
    rng = np.random.default_rng(1)
    X, y = rng.standard_normal((n, 3)), rng.standard_normal(n)
    splits = _splits(n, 3)
    groups = plan_svr_columns(X, y, splits, parameter_grid({'kernel': [GaussianKernel(gamma=0.3), LinearKernel()]}), 3.0, 0.25,
                              GaussianKernel())
    assert len(groups) == 2 and all(len(g['cols']) == 3 for g in groups)
    assert all(c[2:] == (3.0, 0.25) for g in groups for c in g['cols'])
    groups = plan_svr_columns(X, y, splits, [{'C': 1.0}, {'C': 2.0}], 1.0, 0.1, GaussianKernel(gamma='scale'))
    assert len(groups) == 3   # a string gamma resolves on every fold's training rows
    for f, g in enumerate(groups):
        assert g['kernel'].gamma == 1. / (X.shape[1] * X[splits[f][0]].var()) and {c[1] for c in g['cols']} == {f}


def _path_rows():
    from optiml_amd.ml.svm import SVR
    from optiml_amd.ml.svm.kernels import linear
    from optiml_amd.ml.svm.losses import epsilon_insensitive, squared_epsilon_insensitive
    from optiml_amd.opti.constrained import ActiveSet, FrankWolfe, InteriorPoint, ProjectedGradient
    base = dict(loss=epsilon_insensitive, dual=True, reg_intercept=True, optimizer=ProjectedGradient)
    grid = [{'C': 1.0}]
    return [
        (SVR(**base), grid, 1, True),
        (SVR(**dict(base, optimizer=FrankWolfe)), grid, 1, True),
        (SVR(**base), [{'C': 1.0, 'epsilon': 0.2}], 1, True),
        (SVR(**dict(base, storage='f32')), [{'epsilon': 0.2}], 1, True),
        (SVR(**dict(base, optimizer=FrankWolfe, storage='f32')), [{'C': 1.0, 'epsilon': 0.2, 'kernel': linear}], 1, True),
        (SVR(**base), [{'kernel': linear}], 1, True),
        (SVR(**dict(base, storage='stream')), grid, 1, False),
        (SVR(**base), grid, 2, False),
        (SVR(**dict(base, optimizer=ActiveSet)), grid, 1, False),
        (SVR(**dict(base, optimizer=InteriorPoint)), grid, 1, False),
        (SVR(**dict(base, optimizer='smo', reg_intercept=False)), grid, 1, False),
        (SVR(**dict(base, reg_intercept=False)), grid, 1, False),
        (SVR(**dict(base, loss=squared_epsilon_insensitive)), grid, 1, False),
        (SVR(**base), [{'C': 1.0, 'max_iter': 10}], 1, False),
    ]


@pytest.mark.parametrize('row', range(14))
def test_path_selection(row):
    from optiml_amd.ml.svm.model_selection import uses_batched_svr_search
    est, grid, world, want = _path_rows()[row]
    assert uses_batched_svr_search(est, grid, world) is want


def test_an_svc_is_not_an_svr_search():
    from optiml_amd.ml.svm import SVC, SVRGridSearchCV
    from optiml_amd.ml.svm.model_selection import uses_batched_svr_search
    assert uses_batched_svr_search(SVC(), [{'C': 1.0}], 1) is False
    with pytest.raises(TypeError):
        SVRGridSearchCV(SVC(), {'C': [1]}).fit(np.zeros((6, 2)), np.arange(6.))
    from optiml_amd.ml.svm import SVR
    with pytest.raises(NotImplementedError):
        SVRGridSearchCV(SVR(), {'C': [1]}, scoring='neg_mean_squared_error').fit(np.zeros((6, 2)), np.arange(6.))


def test_int_cv_is_kfold_and_the_default_stays_stratified():
    ms = pytest.importorskip('sklearn.model_selection')
    from optiml_amd.ml.svm.model_selection import check_cv_splits
    rng = np.random.default_rng(2)
    X, y = rng.standard_normal((50, 3)), rng.standard_normal(50)
    want = list(ms.KFold(5).split(X, y))
    for cv in (5, np.int64(5), ms.KFold(5), want):
        got = check_cv_splits(cv, X, y, stratified=False)
        assert len(got) == 5
        for (a, b), (c, d) in zip(got, want):
            assert np.array_equal(a, c) and np.array_equal(b, d)
    labels = np.arange(50) % 3
    rng.shuffle(labels)
    strat = list(ms.StratifiedKFold(5).split(X, labels))
    assert any(not np.array_equal(b, d) for (_, b), (_, d) in zip(strat, want))   # the two differ on these labels
    for got in (check_cv_splits(5, X, labels), check_cv_splits(5, X, labels, stratified=True)):
        for (a, b), (c, d) in zip(got, strat):
            assert np.array_equal(a, c) and np.array_equal(b, d)


@pytest.mark.parametrize('seed', range(4))
def test_r2_from_sse_is_r2_score(seed):
    metrics = pytest.importorskip('sklearn.metrics')
    from optiml_amd.ml.svm.model_selection import r2_from_sse
    rng = np.random.default_rng(seed)
    y = rng.standard_normal(200) * (1 + seed) + seed
    te = np.sort(rng.choice(200, 67, replace=False))
    pred = y[te] + 0.3 * rng.standard_normal(67)
    sse = float(((y[te] - pred) ** 2).sum())
    np.testing.assert_allclose(r2_from_sse(sse, y[te]), metrics.r2_score(y[te], pred), rtol=1e-12)


def test_r2_from_sse_edge_cases():
    metrics = pytest.importorskip('sklearn.metrics')
    from optiml_amd.ml.svm.model_selection import r2_from_sse
    const = np.full(5, 2.0)
    assert r2_from_sse(0., const) == metrics.r2_score(const, const) == 1.0
    assert r2_from_sse(5., const) == metrics.r2_score(const, const + 1) == 0.0
    assert np.isnan(r2_from_sse(float('nan'), np.arange(5.)))


def test_svr_column_cap_follows_memory():
    from optiml_amd.ml.svm import model_selection as ms
    from optiml_amd.ml.svm._batched import column_bytes
    n = 100000
    slab = 16 * 391 * 391 * 256 * 8
    assert ms.svr_column_cap(100, 200 << 30, slab) == ms.MAX_COLUMNS
    cap = ms.svr_column_cap(n, 50 << 30, slab)
    assert 16 <= cap < ms.MAX_COLUMNS and cap * column_bytes(2 * n) + slab <= ms.MEMORY_SHARE * (50 << 30)
    assert cap < ms.column_cap(n, 50 << 30, slab)   # a column of 2n-vectors takes more than one of n-vectors
    assert ms.svr_column_cap(n, 1 << 30, slab) == 16
