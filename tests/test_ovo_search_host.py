"""CPU checks of OneVsOneGridSearchCV: the C ABI of the vote kernel and of the held-out vote of the pair solver (bq_ovo_vote,
bq_msolver_pairs_vote_heldout) and their device-free refusals, the column plan on hand-made codes and splits, path selection, the
memory budget of a solve, and a plain restatement of the vote against ovo_decision (no GPU needed)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = {'bq_ovo_vote': 6, 'bq_msolver_pairs_vote_heldout': 10}


def test_new_symbols_are_declared_exported_and_bound():
    from optiml_amd import build, _lib
    build.build()
    lib = _lib.load()
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(REPO, 'include', 'bcqp.h')).read(), flags=re.S)
    assert re.search(r'#define BQ_ABI_VERSION 3\b', text)
    for name, nargs in NEW_SYMBOLS.items():
        decl = re.search(r'\b%s\s*\(([^)]*)\)' % name, text)
        assert decl and len(decl.group(1).split(',')) == nargs, name
        assert hasattr(lib, name) and name in _lib.PROTOTYPES, name
        restype, args = _lib.PROTOTYPES[name]
        assert restype is C.c_int and len(args) == nargs, name
    readme = open(os.path.join(REPO, 'README.md')).read()
    declared = set(re.findall(r'^\w[\w \*]*?\s*\*?(bq_\w+)\s*\(', text, flags=re.M))
    assert declared == set(_lib.PROTOTYPES)
    assert '(%d entry points' % len(declared) in readme   # the README's count is the header's


def test_device_free_refusals():
    from optiml_amd import build, _lib
    build.build()
    lib = _lib.load()
    D, pred = np.zeros(3), np.zeros(1, dtype=np.int32)
    assert lib.bq_ovo_vote(None, 3, 1, _lib.ptr(D), _lib.iptr(pred), None) == _lib.ERR_BADARG
    assert b'NULL' in lib.bq_last_error()
    assert lib.bq_ovo_vote(None, 3, 1, None, None, None) == _lib.ERR_BADARG
    u8 = lambda a: a.ctypes.data_as(C.POINTER(C.c_ubyte))   # noqa: E731
    i64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int64))   # noqa: E731
    rows, group_of, b, n = np.ones(4, dtype=np.uint8), np.zeros(1, dtype=np.int32), np.zeros(1), np.zeros(1, dtype=np.int64)
    assert lib.bq_msolver_pairs_vote_heldout(None, u8(rows), 1, _lib.iptr(group_of), u8(rows), _lib.ptr(b), i64(n), i64(n), i64(n),
                                             None) == _lib.ERR_BADARG
    assert b'NULL' in lib.bq_last_error()


def test_exported_from_the_svm_package():
    from optiml_amd.ml import svm
    from optiml_amd.ml.svm import ovo_search
    for name in ('OneVsOneGridSearchCV', 'ovo_vote'):
        assert getattr(svm, name) is getattr(ovo_search, name) and name in svm.__all__
    assert {'plan_ovo_columns', 'uses_batched_ovo_search'} <= set(ovo_search.__all__)


def _vote(D, ncls):
    """The vote of bq_vote.h in plain Python, row by row and pair by pair: (pred, Y)"""
    t = len(D)
    Y, pred = np.empty((t, ncls)), np.empty(t, dtype=np.int64)
    with np.errstate(invalid='ignore'):
        for r in range(t):
            conf, votes = [0.0] * ncls, [0] * ncls
            k = 0
            for i in range(ncls):
                for j in range(i + 1, ncls):
                    d = float(D[r, k])
                    conf[i] -= d
                    conf[j] += d
                    votes[j if d > 0 else i] += 1
                    k += 1
            Y[r] = [np.float64(votes[c]) + np.float64(conf[c]) / (3 * (abs(np.float64(conf[c])) + 1)) for c in range(ncls)]
            best = 0
            for c in range(1, ncls):
                if np.isnan(Y[r, best]):
                    break
                if np.isnan(Y[r, c]) or Y[r, c] > Y[r, best]:
                    best = c
            pred[r] = best
    return pred, Y


@pytest.mark.parametrize('ncls', [2, 3, 7])
def test_the_vote_restated_is_ovo_decision_and_argmax(ncls):
    from optiml_amd.ml.svm.onevsone import ovo_decision
    P = ncls * (ncls - 1) // 2
    rng = np.random.default_rng(ncls)
    D = np.vstack([rng.standard_normal((40, P)), np.zeros((2, P)), rng.integers(-4, 5, (40, P)) * 0.5, -np.zeros((1, P)),
                   rng.standard_normal((6, P))])
    D[-6:-3, 0] = [np.nan, np.inf, -np.inf]
    D[-3:, P - 1] = [np.nan, np.inf, -np.inf]
    pred, Y = _vote(D, ncls)
    with np.errstate(invalid='ignore'):
        want = ovo_decision((D > 0).astype(int), D, ncls)
    assert np.array_equal(Y, want, equal_nan=True)
    assert np.array_equal(pred, want.argmax(axis=1))
    if ncls == 2:   # OneVsOneSVC.predict with two classes: class 1 exactly when Y[:, 1] > 0
        assert np.array_equal(pred, (want[:, 1] > 0).astype(int))


def _hand_made():
    """17 rows of 3 classes (sizes 6, 7, 4), three interleaved folds, two candidates on one kernel and one on another"""
    from optiml_amd.ml.svm.kernels import GaussianKernel
    codes = np.array([0, 1, 2, 1, 0, 1, 0, 2, 1, 0, 1, 2, 0, 1, 0, 2, 1])
    idx = np.arange(len(codes))
    splits = [(idx[idx % 3 != f], idx[idx % 3 == f]) for f in range(3)]
    other = GaussianKernel(gamma=0.25)
    cands = [{'C': 0.5}, {'C': 2.0, 'kernel': other}, {'C': 4.0}]
    return codes, splits, cands, other


def test_plan_ovo_columns_order_boxes_and_held_rows():
    from optiml_amd.ml.svm.kernels import GaussianKernel
    from optiml_amd.ml.svm.onevsone import TILE, ovo_pairs
    from optiml_amd.ml.svm.ovo_search import plan_ovo_columns
    codes, splits, cands, other = _hand_made()
    base = GaussianKernel(gamma=0.5)
    plan = plan_ovo_columns(codes, 3, splits, cands, 1.0, base)
    n_pad, index, pcode, data_row = plan['n_pad'], plan['index'], plan['pcode'], plan['data_row']
    assert n_pad == 3 * TILE and list(plan['cls_tiles']) == [0, 1, 2, 3] and plan['pairs'] == ovo_pairs(3)
    assert data_row.sum() == len(codes) and np.array_equal(pcode[index], codes) and data_row[index].all()
    groups = plan['groups']
    assert len(groups) == 2 and groups[0]['kernel'] is base and groups[1]['kernel'] is other
    assert groups[0]['fits'] == [(0, f, 0.5) for f in range(3)] + [(2, f, 4.0) for f in range(3)]
    assert groups[1]['fits'] == [(1, f, 2.0) for f in range(3)]
    for g in groups:
        nfits = len(g['fits'])
        assert g['cols'] == [(fit, q) for fit in range(nfits) for q in range(3)]   # group-major, pairs in ovo_pairs order
        assert g['Y'].shape == g['UB'].shape == (3 * nfits, n_pad)
        assert g['held'].shape == (nfits, n_pad) and g['held'].dtype == np.uint8
        for c, (fit, q) in enumerate(g['cols']):
            ci, f, Cv = g['fits'][fit]
            i, j = plan['pairs'][q]
            tr, te = splits[f]
            assert np.array_equal(g['Y'][c], np.where(pcode == j, 1., -1.))   # +1 on the larger class
            box = np.zeros(n_pad)
            box[index[tr[(codes[tr] == i) | (codes[tr] == j)]]] = Cv
            assert np.array_equal(g['UB'][c], box)
            assert np.all(g['UB'][c][data_row == 0] == 0) and np.all(g['UB'][c][index[te]] == 0)   # ghost and held-out rows
            assert np.all(g['UB'][c][(pcode != i) & (pcode != j)] == 0)   # the rows of every other class
        for fit, (ci, f, Cv) in enumerate(g['fits']):
            want = np.zeros(n_pad, dtype=np.uint8)
            want[index[splits[f][1]]] = 1
            assert np.array_equal(g['held'][fit], want) and np.all(data_row[g['held'][fit] > 0] == 1)
    base_only = plan_ovo_columns(codes, 3, splits, [{}], 1.5, base)
    assert [fit[2] for fit in base_only['groups'][0]['fits']] == [1.5] * 3


def test_plan_ovo_columns_auto_gamma_is_its_own_panel():
    from optiml_amd.ml.svm.kernels import GaussianKernel
    from optiml_amd.ml.svm.ovo_search import plan_ovo_columns
    codes, splits, _, _ = _hand_made()
    cands = [{'kernel': GaussianKernel(gamma='auto')}, {'kernel': GaussianKernel(gamma=1.0)}, {'kernel': GaussianKernel(gamma='auto')}]
    groups = plan_ovo_columns(codes, 3, splits, cands, 1.0, GaussianKernel(gamma=0.5))['groups']
    assert [[fit[0] for fit in g['fits'][::3]] for g in groups] == [[0, 2], [1]]


def _path_rows():
    from optiml_amd.ml.svm import OneVsOneSVC, OneVsRestSVC, SVC
    from optiml_amd.ml.svm.kernels import GaussianKernel, linear
    from optiml_amd.ml.svm.losses import hinge
    from optiml_amd.opti.constrained import FrankWolfe, ProjectedGradient
    base = dict(loss=hinge, dual=True, reg_intercept=True, optimizer=ProjectedGradient, kernel=GaussianKernel(gamma=0.5))
    y = np.arange(30) % 3
    idx = np.arange(30)
    splits = [(idx[idx // 10 != f], idx[idx // 10 == f]) for f in range(3)]   # every fold trains on all three classes
    lacks = [(idx[y != 2], idx[y == 2])] + splits[1:]   # the first fold's training rows miss class 2
    grid = [{'C': 1.0}, {'C': 2.0}]
    ok = OneVsOneSVC(**base)
    return [
        (ok, grid, splits, y, 1, True),
        (ok, [{}], splits, y, 1, True),
        (OneVsOneSVC(**dict(base, optimizer=FrankWolfe)), [{'C': 1.0, 'kernel': linear}], splits, y, 1, True),
        (OneVsOneSVC(**dict(base, kernel=GaussianKernel(gamma='auto'))), grid, splits, y, 1, True),
        (ok, grid, splits, np.arange(30) % 2, 1, True),
        (OneVsOneSVC(**dict(base, storage='f32')), grid, splits, y, 1, False),
        (OneVsOneSVC(**dict(base, storage='stream')), grid, splits, y, 1, False),
        (OneVsOneSVC(**dict(base, kernel=GaussianKernel(gamma='scale'))), grid, splits, y, 1, False),
        (ok, [{'C': 1.0, 'kernel': GaussianKernel(gamma='scale')}], splits, y, 1, False),
        (ok, [{'C': 1.0}, {'tol': 1e-3}], splits, y, 1, False),
        (ok, grid, splits, y, 2, False),
        (ok, grid, lacks, y, 1, False),
        (ok, grid, [(idx, idx)], idx, 1, True),   # 30 classes
        (SVC(**base), grid, splits, np.arange(30) % 2, 1, False),
        (OneVsRestSVC(**base), grid, splits, y, 1, False),
    ]


@pytest.mark.parametrize('row', range(15))
def test_path_selection(row):
    from optiml_amd.ml.svm.ovo_search import uses_batched_ovo_search
    est, grid, splits, y, world, want = _path_rows()[row]
    assert uses_batched_ovo_search(est, grid, splits, y, world) is want


def test_more_than_64_classes_take_the_per_fold_path():
    from optiml_amd.ml.svm.ovo_search import uses_batched_ovo_search
    est, grid, _, _, _, _ = _path_rows()[0]
    y = np.arange(130) % 65
    idx = np.arange(130)
    assert uses_batched_ovo_search(est, grid, [(idx, idx)], y, 1) is False
    assert uses_batched_ovo_search(est, grid, [(idx[:128], idx[:128])], np.arange(128) % 64, 1) is True


def test_groups_per_solve_counts_the_scoring_scratch():
    """Whole (candidate, fold) groups inside `pair_chunks`' budget, the scoring's slab and two n-vectors per column included; none
    when one group's columns do not fit"""
    from optiml_amd import build
    from optiml_amd.ml.svm._batched import MEMORY_SHARE, column_bytes
    from optiml_amd.ml.svm.model_selection import MAX_COLUMNS
    from optiml_amd.ml.svm.onevsone import ovo_pairs, pairs_slab_bytes
    from optiml_amd.ml.svm.ovo_search import groups_per_solve
    build.build()
    cls_tiles = np.array([0, 1, 3, 4], dtype=np.int32)
    pairs, n_pad = ovo_pairs(3), 4 * 256
    vec = 8 * (n_pad + 256)
    per = sum(column_bytes(n_pad) + pairs_slab_bytes(cls_tiles, [p]) for p in pairs) + 2 * 3 * vec
    wide = 16 * 4 * 4 * 256 * 8
    fixed = wide + 2 * 15 * vec
    for want in (0, 1, 5):
        free = (fixed + want * per + per // 2) / MEMORY_SHARE
        assert groups_per_solve(pairs, cls_tiles, n_pad, free, wide) == want
    assert groups_per_solve(pairs, cls_tiles, n_pad, 1 << 50, wide) == MAX_COLUMNS // 3
    assert groups_per_solve(pairs, cls_tiles, n_pad, 0, wide) == 0


def test_type_errors_before_any_device_work():
    from optiml_amd.ml.svm import OneVsOneGridSearchCV, OneVsOneSVC, SVC
    X, y = np.zeros((6, 2)), np.arange(6) % 3
    with pytest.raises(TypeError):
        OneVsOneGridSearchCV(SVC(), {'C': [1.0]}).fit(X, y)
    with pytest.raises(NotImplementedError):
        OneVsOneGridSearchCV(OneVsOneSVC(), {'C': [1.0]}, scoring='f1_macro').fit(X, y)
    search = OneVsOneGridSearchCV(OneVsOneSVC(), {'C': [1.0]}, cv=3, refit=False)
    assert search.get_params(deep=False)['cv'] == 3 and search.refit is False
