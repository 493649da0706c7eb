"""CPU checks of the one-vs-one layer over the batched SMO walkers: which configurations `OneVsOneSVC` and `OneVsOneGridSearchCV`
solve as pair columns (`uses_batched_ovo_smo`, `uses_batched_ovo_smo_search`; `uses_batched_ovo` keeps answering False for SMO),
the column plan on hand-made codes and folds, the memory budget of a solve, the dispatch by `batch_smo`, and the C ABI of
`bq_msmo_vote_heldout` — declared, exported, bound, and refusing NULL before any device call (no GPU needed)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _svc_rows():
    """(SVC keywords, world, uses_batched_ovo_smo, uses_batched_ovo)"""
    from optiml_amd.ml.svm.kernels import GaussianKernel, PolyKernel, linear
    from optiml_amd.ml.svm.losses import hinge, squared_hinge
    from optiml_amd.ml.svm.smo import SMO
    from optiml_amd.opti.constrained import ProjectedGradient
    base = dict(loss=hinge, dual=True, reg_intercept=False, optimizer='smo', kernel=GaussianKernel(gamma=0.5))
    return [
        (dict(base), 1, True, False),
        (dict(base, optimizer=SMO), 1, True, False),
        (dict(base, kernel=GaussianKernel(gamma='auto')), 1, True, False),
        (dict(base, kernel=PolyKernel(gamma='auto')), 1, True, False),
        (dict(base, kernel=linear), 1, True, False),
        (dict(base, storage='f32'), 1, True, False),
        (dict(base, kernel=GaussianKernel(gamma='scale')), 1, False, False),
        (dict(base, kernel=PolyKernel(gamma='scale')), 1, False, False),
        (dict(base, storage='stream'), 1, False, False),
        (dict(base), 2, False, False),
        (dict(base, reg_intercept=True), 1, False, False),
        (dict(base, loss=squared_hinge), 1, False, False),
        (dict(base, dual=False), 1, False, False),
        (dict(base, optimizer=ProjectedGradient, reg_intercept=True), 1, False, True),   # the class-sorted panel's path
    ]


@pytest.mark.parametrize('row', range(14))
def test_which_svc_configurations_take_pair_columns(row):
    from optiml_amd.ml.svm import SVC
    from optiml_amd.ml.svm.onevsone import uses_batched_ovo, uses_batched_ovo_smo
    kw, world, want, sorted_path = _svc_rows()[row]
    assert uses_batched_ovo_smo(SVC(**kw), world) is want
    assert uses_batched_ovo(SVC(**kw), world) is sorted_path


def _search_rows():
    from optiml_amd.ml.svm import OneVsOneSVC, OneVsRestSVC, SVC
    from optiml_amd.ml.svm.kernels import GaussianKernel, linear
    from optiml_amd.ml.svm.losses import hinge
    from optiml_amd.opti.constrained import ProjectedGradient
    base = dict(loss=hinge, dual=True, optimizer='smo', kernel=GaussianKernel(gamma=0.5))
    y = np.arange(30) % 3
    idx = np.arange(30)
    splits = [(idx[idx // 10 != f], idx[idx // 10 == f]) for f in range(3)]   # every fold trains on all three classes
    lacks = [(idx[y != 2], idx[y == 2])] + splits[1:]   # the first fold's training rows miss class 2
    grid = [{'C': 1.0}, {'C': 2.0}]
    ok = OneVsOneSVC(**base)
    return [
        (ok, grid, splits, y, 1, True),
        (ok, [{}], splits, y, 1, True),
        (ok, [{'C': 1.0, 'kernel': linear}], splits, y, 1, True),
        (OneVsOneSVC(**dict(base, kernel=GaussianKernel(gamma='auto'))), grid, splits, y, 1, True),
        (ok, grid, splits, np.arange(30) % 2, 1, True),
        (ok, grid, [(idx, idx)], idx, 1, True),   # 30 classes
        (OneVsOneSVC(**dict(base, storage='f32')), grid, splits, y, 1, False),
        (OneVsOneSVC(**dict(base, storage='stream')), grid, splits, y, 1, False),
        (OneVsOneSVC(**dict(base, kernel=GaussianKernel(gamma='scale'))), grid, splits, y, 1, False),
        (ok, [{'C': 1.0, 'kernel': GaussianKernel(gamma='scale')}], splits, y, 1, False),
        (ok, [{'C': 1.0}, {'tol': 1e-2}], splits, y, 1, False),
        (ok, grid, splits, y, 2, False),
        (ok, grid, lacks, y, 1, False),
        (OneVsOneSVC(**dict(base, reg_intercept=True, optimizer=ProjectedGradient)), grid, splits, y, 1, False),
        (SVC(**base), grid, splits, np.arange(30) % 2, 1, False),
        (OneVsRestSVC(**base), grid, splits, y, 1, False),
    ]


@pytest.mark.parametrize('row', range(16))
def test_which_searches_take_pair_columns(row):
    from optiml_amd.ml.svm.ovo_search import uses_batched_ovo_search, uses_batched_ovo_smo_search
    est, grid, splits, y, world, want = _search_rows()[row]
    assert uses_batched_ovo_smo_search(est, grid, splits, y, world) is want
    if want:
        assert uses_batched_ovo_search(est, grid, splits, y, world) is False   # the class-sorted panel is not SMO's
    if row == 13:
        assert uses_batched_ovo_search(est, grid, splits, y, world) is True


def test_more_than_64_classes_take_the_per_fold_path():
    from optiml_amd.ml.svm.ovo_search import uses_batched_ovo_smo_search
    est, grid = _search_rows()[0][:2]
    idx = np.arange(130)
    assert uses_batched_ovo_smo_search(est, grid, [(idx, idx)], idx % 65, 1) is False
    assert uses_batched_ovo_smo_search(est, grid, [(idx[:128], idx[:128])], np.arange(128) % 64, 1) is True


def _hand_made():
    """14 rows of 3 classes (sizes 6, 5, 3), two interleaved folds, two candidates on one kernel and one on another"""
    from optiml_amd.ml.svm.kernels import GaussianKernel
    codes = np.array([1, 0, 2, 0, 1, 1, 0, 2, 0, 1, 0, 2, 1, 0])
    idx = np.arange(len(codes))
    splits = [(idx[idx % 2 != f], idx[idx % 2 == f]) for f in range(2)]
    other = GaussianKernel(gamma=0.25)
    cands = [{'C': 0.5}, {'C': 2.0, 'kernel': other}, {'C': 4.0}]
    return codes, splits, cands, other


def test_plan_ovo_smo_columns_lists_labels_and_held_rows():
    from optiml_amd.ml.svm.kernels import GaussianKernel
    from optiml_amd.ml.svm.onevsone import ovo_pairs
    from optiml_amd.ml.svm.ovo_search import plan_ovo_smo_columns
    codes, splits, cands, other = _hand_made()
    base = GaussianKernel(gamma=0.5)
    groups = plan_ovo_smo_columns(codes, 3, splits, cands, 1.0, base)
    pairs = ovo_pairs(3)
    assert len(groups) == 2 and groups[0]['kernel'] is base and groups[1]['kernel'] is other
    assert groups[0]['fits'] == [(0, 0, 0.5), (0, 1, 0.5), (2, 0, 4.0), (2, 1, 4.0)]   # candidate-major
    assert groups[1]['fits'] == [(1, 0, 2.0), (1, 1, 2.0)]
    # written out: fold 0 trains on the odd rows 1 3 5 7 9 11 13 (classes 0 0 1 2 1 2 0)
    assert [list(r) for r in groups[0]['rows'][:3]] == [[1, 3, 5, 9, 13], [1, 3, 7, 11, 13], [5, 7, 9, 11]]
    assert list(groups[0]['Y'][2]) == [1. if c == 2 else -1. for c in codes]   # pair (1, 2): +1 on class 2
    assert list(groups[0]['held'][0]) == [1, 0] * 7
    for g in groups:
        nfits = len(g['fits'])
        assert g['cols'] == [(fit, q) for fit in range(nfits) for q in range(3)]   # group-major, pairs in ovo_pairs order
        assert g['Y'].shape == (3 * nfits, 14) and len(g['rows']) == 3 * nfits and g['C'].shape == (3 * nfits,)
        assert g['held'].shape == (nfits, 14) and g['held'].dtype == np.uint8
        for c, (fit, q) in enumerate(g['cols']):
            ci, f, Cv = g['fits'][fit]
            i, j = pairs[q]
            tr, te = splits[f]
            assert g['C'][c] == Cv == cands[ci]['C']
            assert np.array_equal(g['Y'][c], np.where(codes == j, 1., -1.))   # +1 on the larger class
            want = np.sort(tr[(codes[tr] == i) | (codes[tr] == j)])
            assert np.array_equal(g['rows'][c], want) and np.all(np.diff(g['rows'][c]) > 0)
            assert not g['held'][fit][g['rows'][c]].any()   # no held row in a list of its own group
        for fit, (ci, f, Cv) in enumerate(g['fits']):
            want = np.zeros(14, dtype=np.uint8)
            want[splits[f][1]] = 1
            assert np.array_equal(g['held'][fit], want)
    assert [fit[2] for fit in plan_ovo_smo_columns(codes, 3, splits, [{}], 1.5, base)[0]['fits']] == [1.5] * 2
    # training rows in any order give the same ascending lists; a repeated training row or a tested one: no plan
    shuffled = [(tr[::-1], te) for tr, te in splits]
    again = plan_ovo_smo_columns(codes, 3, shuffled, cands, 1.0, base)
    assert all(np.array_equal(a, b) for a, b in zip(again[0]['rows'], groups[0]['rows']))
    assert plan_ovo_smo_columns(codes, 3, [(np.append(splits[0][0], 1), splits[0][1])], cands, 1.0, base) is None
    assert plan_ovo_smo_columns(codes, 3, [(splits[0][0], np.append(splits[0][1], 1))], cands, 1.0, base) is None


def test_smo_groups_per_solve_counts_the_scoring_scratch():
    from optiml_amd import _lib
    from optiml_amd.ml.svm._batched import MAX_COLUMNS, MEMORY_SHARE, smo_column_bytes
    from optiml_amd.ml.svm.ovo_search import smo_groups_per_solve
    P, n = 6, 1000
    vec = 8 * (n + 256)
    assert smo_column_bytes(n, _lib.SVC) == 36000
    per = P * 36000 + 2 * P * vec
    wide = 16 * 4 * 4 * 256 * 8
    fixed = wide + 2 * 15 * vec
    for want in (0, 1, 5):
        free = (fixed + want * per + per // 2) / MEMORY_SHARE
        assert smo_groups_per_solve(P, n, free, wide) == want
    assert smo_groups_per_solve(P, n, 1 << 50, wide) == MAX_COLUMNS // P
    assert smo_groups_per_solve(P, n, 0, wide) == 0
    assert smo_groups_per_solve(1, n, 1 << 50, wide) == MAX_COLUMNS


def test_dispatch_by_batch_smo():
    """`batch_smo` is None on both classes; the search's dispatch follows it: True and False force, None goes by the number of
    columns; a configuration off the SMO path is not forced onto it"""
    from optiml_amd.ml.svm import OneVsOneGridSearchCV, OneVsOneSVC
    from optiml_amd.ml.svm._batched import SMO_MIN_COLUMNS, takes_batched_smo
    from optiml_amd.ml.svm.kernels import GaussianKernel
    from optiml_amd.ml.svm.losses import hinge
    from optiml_amd.ml.svm.ovo_search import takes_batched_ovo_smo_search as takes
    from optiml_amd.opti.constrained import ProjectedGradient
    assert OneVsOneSVC.batch_smo is None and OneVsOneGridSearchCV.batch_smo is None
    est, grid, splits, y = _search_rows()[0][:4]
    assert takes(est, grid, splits, y, 1, True) is True and takes(est, grid, splits, y, 1, False) is False
    assert takes(est, grid, splits, y, 1) is takes_batched_smo(2 * 3 * 3) is True
    assert 1 * 1 * 1 < SMO_MIN_COLUMNS   # one candidate, one fold, two classes: one column
    assert takes(est, [{'C': 1.0}], splits[:1], np.arange(30) % 2, 1) is False
    assert takes(est, [{'C': 1.0}], splits[:1], np.arange(30) % 2, 1, True) is True
    assert takes(est, grid, splits, y, 2, True) is False   # two ranks: not forced
    pg = OneVsOneSVC(loss=hinge, dual=True, reg_intercept=True, optimizer=ProjectedGradient, kernel=GaussianKernel(gamma=0.5))
    assert takes(pg, grid, splits, y, 1, True) is False   # the class-sorted panel's path is not forced onto SMO's
    assert takes_batched_smo(3, None) is False   # OneVsOneSVC on two or three classes (1 or 3 pairs) stays per pair
    assert takes_batched_smo(1, None) is False and takes_batched_smo(6, None) is True


def test_new_symbol_is_declared_exported_and_bound():
    from optiml_amd import build, _lib
    build.build()
    lib = _lib.load()
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(REPO, 'include', 'bcqp.h')).read(), flags=re.S)
    decl = re.search(r'int\s+bq_msmo_vote_heldout\s*\(([^)]*)\)', text)
    assert decl
    args = [' '.join(a.split()) for a in decl.group(1).split(',')]
    assert [a.rsplit(' ', 1)[0] if '*' not in a else a[:a.rindex('*') + 1] for a in args] == [
        'bq_msmo *', 'int', 'const int *', 'int', 'const int *', 'const int *', 'const unsigned char *', 'double *', 'int64_t *',
        'int64_t *', 'int64_t *', 'int *']
    assert hasattr(lib, 'bq_msmo_vote_heldout') and 'bq_msmo_vote_heldout' in _lib.PROTOTYPES
    _dp, _ip, _vp, _i64 = C.POINTER(C.c_double), C.POINTER(C.c_int), C.c_void_p, C.POINTER(C.c_int64)
    assert _lib.PROTOTYPES['bq_msmo_vote_heldout'] == (C.c_int, [_vp, C.c_int, _ip, C.c_int, _ip, _ip, C.POINTER(C.c_ubyte), _dp,
                                                                 _i64, _i64, _i64, _ip])
    assert '(still 3: bq_msmo_vote_heldout was added; nothing existing changed)' in open(os.path.join(REPO, 'include', 'bcqp.h')).read()


def test_null_arguments_are_refused_before_any_device_call():
    from optiml_amd import build, _lib
    build.build()
    lib = _lib.load()
    u8 = lambda a: a.ctypes.data_as(C.POINTER(C.c_ubyte))   # noqa: E731
    i64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int64))   # noqa: E731
    code, one, held = np.zeros(4, dtype=np.int32), np.zeros(1, dtype=np.int32), np.zeros(4, dtype=np.uint8)
    b, cnt = np.zeros(1), np.zeros(1, dtype=np.int64)
    assert lib.bq_msmo_vote_heldout(None, 2, _lib.iptr(code), 1, _lib.iptr(one), _lib.iptr(one), u8(held), _lib.ptr(b), i64(cnt),
                                    i64(cnt), i64(cnt), None) == _lib.ERR_BADARG
    assert b'NULL' in lib.bq_last_error()


def test_exported_from_the_modules():
    from optiml_amd.ml.svm import onevsone, ovo_search
    assert 'uses_batched_ovo_smo' in onevsone.__all__
    assert {'uses_batched_ovo_smo_search', 'plan_ovo_smo_columns', 'smo_groups_per_solve'} <= set(ovo_search.__all__)
