"""CPU checks of NuSVCGridSearchCV and NuSVRGridSearchCV: the C ABI of the held-out scoring of the two-group simplex solver
(bq_msolver_simplex2_heldout), the column plans on hand-made splits (masses, boxes, labels, grouping by kernel, a failed fit left
out), path selection, cv_results_ with a NaN candidate and the type errors (no GPU needed)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOL = 'bq_msolver_simplex2_heldout'


def test_heldout_is_declared_exported_and_bound_with_nine_arguments():
    from optiml_amd import build, _lib
    build.build()
    lib = _lib.load()
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(REPO, 'include', 'bcqp.h')).read(), flags=re.S)
    assert re.search(r'#define BQ_ABI_VERSION 3\b', text)
    decl = re.search(r'\b%s\s*\(([^)]*)\)' % SYMBOL, text)
    assert decl and len(decl.group(1).split(',')) == 9
    assert hasattr(lib, SYMBOL) and SYMBOL in _lib.PROTOTYPES
    restype, args = _lib.PROTOTYPES[SYMBOL]
    assert restype is C.c_int and len(args) == 9
    off = _lib.PROTOTYPES['bq_msolver_simplex2_offsets'][1]
    assert args[0] == off[0] and args[2:6] == off[1:]   # the solver, then y, then the offsets' four results


def test_null_arguments_are_bad_arguments():
    from optiml_amd import build, _lib
    build.build()
    lib = _lib.load()
    v = np.ones(4)
    i = np.zeros(4, dtype=np.int64).ctypes.data_as(C.POINTER(C.c_int64))
    assert lib.bq_msolver_simplex2_heldout(None, _lib.ptr(v), _lib.ptr(v), _lib.ptr(v), i, i, i, i, _lib.ptr(v)) == _lib.ERR_BADARG
    assert b'NULL' in lib.bq_last_error()
    assert lib.bq_msolver_simplex2_heldout(None, None, None, None, None, None, None, None, None) == _lib.ERR_BADARG


def test_exported_from_the_svm_package():
    from optiml_amd.ml import svm
    from optiml_amd.ml.svm import nu_search
    for name in ('NuSVCGridSearchCV', 'NuSVRGridSearchCV'):
        assert getattr(svm, name) is getattr(nu_search, name) and name in svm.__all__
    assert {'plan_nu_svc_columns', 'plan_nu_svr_columns'} <= set(nu_search.__all__)


def _splits(n, k):
    idx = np.arange(n)
    return [(np.setdiff1d(idx, idx[f::k]), idx[f::k]) for f in range(k)]


def test_plan_nu_svc_columns_masses_boxes_and_labels():
    from optiml_amd.ml.svm.kernels import GaussianKernel
    from optiml_amd.ml.svm.model_selection import parameter_grid
    from optiml_amd.ml.svm.nu_search import plan_nu_svc_columns
    n = 12
    X = np.random.default_rng(0).standard_normal((n, 3))
    y = np.array([3, 3, 3, 7, 7, 7, 3, 3, 3, 7, 7, 7])   # every fold of _splits(12, 3) trains on 4 rows of each label
    splits = _splits(n, 3)
    cands = parameter_grid({'nu': [0.25, 0.75]})
    groups, classes, failed = plan_nu_svc_columns(X, y, splits, cands, 0.5, GaussianKernel(gamma=0.3))
    assert np.array_equal(classes, [3, 7]) and failed == [] and len(groups) == 1
    g = groups[0]
    assert g['S'].shape == g['UB'].shape == (6, n) and g['mass'].shape == (6, 2)
    assert g['cols'] == [(ci, f, cands[ci]['nu']) for ci in range(2) for f in range(3)]
    for j, (ci, f, nu) in enumerate(g['cols']):
        tr, te = splits[f]
        assert np.array_equal(g['S'][j], np.where(y == 7, 1., -1.))   # the larger label is +1
        assert np.all(g['UB'][j][tr] == 1.) and np.all(g['UB'][j][te] == 0.)
        assert np.array_equal(g['mass'][j], [nu * 8 / 2] * 2)
    base, _, _ = plan_nu_svc_columns(X, y, splits, [{}], 0.5, GaussianKernel(gamma=0.3))
    assert [c[2] for c in base[0]['cols']] == [0.5] * 3


def test_plan_nu_svc_columns_leaves_a_failed_fit_out():
    from optiml_amd.ml.svm.kernels import GaussianKernel
    from optiml_amd.ml.svm.nu_search import plan_nu_svc_columns
    n = 12
    X = np.random.default_rng(1).standard_normal((n, 3))
    y = np.array([1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0])
    # fold 0 trains on one row of label 1 and 8 of label 0: nu 9 / 2 <= 1 needs nu <= 2 / 9; fold 1 trains on label 0 alone;
    # fold 2 trains on all three rows of label 1 and 6 of label 0: nu <= 6 / 9
    splits = [(np.r_[0, 4:12], np.r_[1:4]), (np.r_[3:12], np.r_[0:3]), (np.r_[0:3, 6:12], np.r_[3:6])]
    assert all(len(np.intersect1d(tr, te)) == 0 and len(tr) + len(te) == n for tr, te in splits)
    cands = [{'nu': 0.2}, {'nu': 0.5}, {'nu': 0.9}]
    groups, classes, failed = plan_nu_svc_columns(X, y, splits, cands, 0.5, GaussianKernel(gamma=0.3))
    assert failed == [(0, 1), (1, 0), (1, 1), (2, 0), (2, 1), (2, 2)]
    assert [c[:2] for c in groups[0]['cols']] == [(0, 0), (0, 2), (1, 2)]
    assert np.array_equal(groups[0]['mass'], [[0.2 * 9 / 2] * 2, [0.2 * 9 / 2] * 2, [0.5 * 9 / 2] * 2])
    with pytest.raises(ValueError, match='more than two labels'):
        plan_nu_svc_columns(X, np.arange(n) % 3, splits, cands, 0.5, GaussianKernel(gamma=0.3))


def test_plan_nu_svr_columns_masses_boxes_and_linear_terms():
    from optiml_amd.ml.svm.kernels import GaussianKernel
    from optiml_amd.ml.svm.model_selection import parameter_grid
    from optiml_amd.ml.svm.nu_search import plan_nu_svr_columns
    n = 11   # folds of 4, 4 and 3 held-out rows: n_train differs
    rng = np.random.default_rng(2)
    X, y = rng.standard_normal((n, 3)), rng.standard_normal(n)
    splits = _splits(n, 3)
    cands = parameter_grid({'nu': [0.25, 0.75], 'C': [0.5, 2.0]})
    assert cands == [{'C': 0.5, 'nu': 0.25}, {'C': 0.5, 'nu': 0.75}, {'C': 2.0, 'nu': 0.25}, {'C': 2.0, 'nu': 0.75}]
    groups = plan_nu_svr_columns(X, y, splits, cands, 1.0, 0.5, GaussianKernel(gamma=0.3))
    assert len(groups) == 1
    g = groups[0]
    assert g['UB'].shape == g['q'].shape == (12, 2 * n) and g['mass'].shape == (12, 2)
    assert [c[:2] for c in g['cols']] == [(ci, f) for ci in range(4) for f in range(3)]
    for j, (ci, f, C_, nu) in enumerate(g['cols']):
        assert (C_, nu) == (cands[ci]['C'], cands[ci]['nu'])
        tr, te = splits[f]
        for half in (0, n):
            assert np.all(g['UB'][j][half + tr] == C_) and np.all(g['UB'][j][half + te] == 0)
        assert np.array_equal(g['mass'][j], [C_ * nu * len(tr) / 2] * 2)
        assert np.array_equal(g['q'][j], np.concatenate((-y, y)))


def test_plans_group_by_resolved_kernel():
    from optiml_amd.ml.svm.kernels import GaussianKernel, LinearKernel
    from optiml_amd.ml.svm.model_selection import parameter_grid
    from optiml_amd.ml.svm.nu_search import plan_nu_svc_columns, plan_nu_svr_columns
    n = 12
    rng = np.random.default_rng(3)
    X, t = rng.standard_normal((n, 3)), rng.standard_normal(n)
    y = np.arange(n) // 3 % 2
    splits = _splits(n, 3)
    two = parameter_grid({'kernel': [GaussianKernel(gamma=0.3), LinearKernel()]})
    groups, _, _ = plan_nu_svc_columns(X, y, splits, two, 0.25, GaussianKernel())
    assert len(groups) == 2 and all(len(g['cols']) == 3 for g in groups) and isinstance(groups[1]['kernel'], LinearKernel)
    groups = plan_nu_svr_columns(X, t, splits, two, 3.0, 0.25, GaussianKernel())
    assert len(groups) == 2 and all(c[2:] == (3.0, 0.25) for g in groups for c in g['cols'])
    # a string gamma resolves on every fold's training rows: one panel per fold, shared by the candidates
    for groups in (plan_nu_svc_columns(X, y, splits, [{'nu': 0.25}, {'nu': 0.5}], 0.25, GaussianKernel(gamma='scale'))[0],
                   plan_nu_svr_columns(X, t, splits, [{'nu': 0.25}, {'nu': 0.5}], 1.0, 0.25, GaussianKernel(gamma='scale'))):
        assert len(groups) == 3
        for f, g in enumerate(groups):
            assert g['kernel'].gamma == 1. / (X.shape[1] * X[splits[f][0]].var())
            assert [c[:2] for c in g['cols']] == [(0, f), (1, f)]


def _path_rows():
    from optiml_amd.ml.svm import NuSVC, NuSVR, SVC
    from optiml_amd.ml.svm.kernels import linear
    return [
        (NuSVC(), [{'nu': 0.3}], True),
        (NuSVC(), [{}], True),
        (NuSVC(storage='f32'), [{'nu': 0.3, 'kernel': linear}], True),
        (NuSVC(), [{'nu': 0.3}, {'kernel': linear}], True),
        (NuSVC(), [{'nu': 0.3, 'tol': 1e-4}], False),
        (NuSVC(), [{'max_iter': 10}], False),
        (NuSVC(), [{'storage': 'f32'}], False),
        (NuSVC(), [{'C': 1.0}], False),   # NuSVC has no C
        (NuSVR(), [{'C': 1.0, 'nu': 0.3}], True),
        (NuSVR(), [{'C': 1.0, 'nu': 0.3, 'kernel': linear}], True),
        (NuSVR(storage='f32'), [{'C': 2.0}], True),
        (NuSVR(), [{'C': 1.0, 'tol': 1e-4}], False),
        (NuSVR(), [{'nu': 0.3}, {'max_iter': 10}], False),
        (NuSVR(), [{'storage': 'f32'}], False),
        (SVC(), [{'C': 1.0}], False),
    ]


@pytest.mark.parametrize('row', range(15))
def test_path_selection(row):
    from optiml_amd.ml.svm.nu_search import uses_batched_nu_search
    est, grid, want = _path_rows()[row]
    assert uses_batched_nu_search(est, grid) is want


def test_aggregate_scores_with_a_nan_candidate():
    """A candidate with a failed fit has a NaN mean and std and ranks last, as GridSearchCV's error_score=nan leaves it."""
    from optiml_amd.ml.svm.model_selection import aggregate_scores
    cands = [{'nu': 0.3}, {'nu': 0.9}, {'nu': 0.5}]
    scores = np.array([[0.75, 0.5, 0.625], [np.nan, 0.9, 0.9], [0.875, 0.75, 0.625]])
    res = aggregate_scores(cands, scores)
    assert np.array_equal(res['split0_test_score'], scores[:, 0], equal_nan=True)
    assert res['mean_test_score'][0] == 0.625 and res['mean_test_score'][2] == 0.75 and np.isnan(res['mean_test_score'][1])
    assert np.isnan(res['std_test_score'][1]) and res['std_test_score'][0] == np.std(scores[0])
    assert list(res['rank_test_score']) == [2, 3, 1]
    assert list(res['param_nu']) == [0.3, 0.9, 0.5]
    assert list(aggregate_scores(cands, np.full((3, 2), np.nan))['rank_test_score']) == [1, 1, 1]


def test_type_errors_and_refusals_before_any_device_work():
    from optiml_amd.ml.svm import NuSVC, NuSVCGridSearchCV, NuSVR, NuSVRGridSearchCV, SVC, SVR
    X, y = np.zeros((6, 2)), np.arange(6) % 2
    for search, wrong in ((NuSVCGridSearchCV, NuSVR()), (NuSVCGridSearchCV, SVC()), (NuSVRGridSearchCV, NuSVC()),
                          (NuSVRGridSearchCV, SVR())):
        with pytest.raises(TypeError):
            search(wrong, {'nu': [0.5]}).fit(X, y)
    with pytest.raises(NotImplementedError):
        NuSVCGridSearchCV(NuSVC(), {'nu': [0.5]}, scoring='f1').fit(X, y)
    with pytest.raises(NotImplementedError):
        NuSVRGridSearchCV(NuSVR(), {'nu': [0.5]}, scoring='neg_mean_squared_error').fit(X, y.astype(float))
    with pytest.raises(ValueError, match='more than two labels'):
        NuSVCGridSearchCV(NuSVC(), {'nu': [0.5]}).fit(X, np.arange(6) % 3)
    with pytest.raises(ValueError, match='nu must be in'):   # the estimator's own checks on every candidate
        NuSVCGridSearchCV(NuSVC(), {'nu': [0.5, 1.5]}, cv=2).fit(X, y)
    with pytest.raises(ValueError, match='more than one target'):
        NuSVRGridSearchCV(NuSVR(), {'nu': [0.5]}).fit(X, np.zeros((6, 2)))
    search = NuSVCGridSearchCV(NuSVC(), {'nu': [0.5]}, cv=3, refit=False)
    assert search.get_params(deep=False)['cv'] == 3 and search.refit is False
