"""CPU checks of OneVsOneSVC: the C ABI of the pair-routed product and pair solver, the class-sorted panel layout, the pair order and
labels, the routed product's work list against a brute-force enumeration of the stored tiles, the vote aggregation against
sklearn's, path selection and the argument checks of the new entry points (no GPU needed)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ['bq_msolver_create_pairs', 'bq_problem_gram_matmat_pairs', 'bq_pairs_slab_bytes', 'bq_pairs_work_list']


@pytest.fixture(scope='module')
def lib():
    from optiml_amd import build, _lib
    build.build()
    return _lib.load()


def test_ovo_abi_is_declared_exported_and_bound(lib):
    from optiml_amd import _lib
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(REPO, 'include', 'bcqp.h')).read(), flags=re.S)
    assert re.search(r'#define BQ_ABI_VERSION 3\b', text)
    for s in NEW_SYMBOLS:
        assert re.search(r'\b%s\s*\(' % s, text), s
        assert hasattr(lib, s), s
        assert s in _lib.PROTOTYPES, s
    assert lib.bq_abi_version() == 3


def test_exported_from_the_svm_package():
    from optiml_amd.ml import svm
    from optiml_amd.ml.svm.onevsone import OneVsOneSVC
    assert svm.OneVsOneSVC is OneVsOneSVC and 'OneVsOneSVC' in svm.__all__


@pytest.mark.parametrize('sizes', [[1, 255, 256, 257, 700], [700, 1], [256, 256], [3, 5, 2]])
def test_sort_plan(sizes):
    from optiml_amd.ml.svm.onevsone import sort_plan
    rs = np.random.RandomState(len(sizes))
    codes = np.concatenate([np.full(s, c) for c, s in enumerate(sizes)])
    rs.shuffle(codes)
    index, ct, n_pad = sort_plan(codes, len(sizes))
    tiles = [(s + 255) // 256 for s in sizes]
    assert list(ct) == list(np.concatenate(([0], np.cumsum(tiles)))) and n_pad == 256 * ct[-1]
    assert len(np.unique(index)) == len(codes) and index.max() < n_pad
    for c, s in enumerate(sizes):
        rows = np.flatnonzero(codes == c)
        # the class's rows first, in their original order; ghost rows fill the rest of its tiles
        assert np.array_equal(index[rows], 256 * ct[c] + np.arange(s))
    ghosts = n_pad - len(codes)
    assert ghosts == sum(256 * t - s for t, s in zip(tiles, sizes))


def test_sort_plan_rejects_an_empty_class():
    from optiml_amd.ml.svm.onevsone import sort_plan
    with pytest.raises(ValueError):
        sort_plan(np.array([0, 0, 2]), 3)


@pytest.mark.parametrize('k', [2, 3, 5])
def test_pair_order_and_labels_match_one_vs_one_classifier(k):
    """The pairs come in OneVsOneClassifier's order and each pair's rows and labels are what _fit_ovo_binary hands SVC.fit."""
    from sklearn.base import BaseEstimator, ClassifierMixin
    from sklearn.multiclass import OneVsOneClassifier
    from optiml_amd.ml.svm.onevsone import ovo_pairs, pair_problem

    class Record(ClassifierMixin, BaseEstimator):
        def fit(self, X, y):
            self.rows_, self.y_ = X[:, 0].astype(int), np.asarray(y)
            self.classes_ = np.unique(y)
            return self

        def decision_function(self, X):
            return np.zeros(len(X))

    rs = np.random.RandomState(k)
    labels = np.array([3, 7, 11, 20, 42])[:k]
    y = labels[rs.randint(0, k, size=60)]
    y[:k] = labels
    X = np.arange(60, dtype=float)[:, None]
    ovo = OneVsOneClassifier(Record()).fit(X, y)
    codes = np.searchsorted(np.unique(y), y)
    pairs = ovo_pairs(k)
    assert len(pairs) == len(ovo.estimators_) == k * (k - 1) // 2
    for (i, j), est in zip(pairs, ovo.estimators_):
        rows, yp = pair_problem(codes, i, j)
        assert np.array_equal(rows, est.rows_)
        assert np.array_equal(np.where(yp > 0, 1, 0), est.y_)   # class j, the larger label, is the positive one


def _work(lib, ct, pairs):
    from optiml_amd import _lib
    ct = np.asarray(ct, dtype=np.int32)
    pr = np.asarray(pairs, dtype=np.int32).reshape(-1)
    n = C.c_int64(0)
    _lib.check(lib.bq_pairs_work_list(int(ct[-1]), len(ct) - 1, _lib.iptr(ct), len(pairs), _lib.iptr(pr), None, 0, C.byref(n)))
    items = np.zeros((n.value, 5), dtype=np.int32)
    _lib.check(lib.bq_pairs_work_list(int(ct[-1]), len(ct) - 1, _lib.iptr(ct), len(pairs), _lib.iptr(pr), _lib.iptr(items),
                                      n.value, C.byref(n)))
    return items


@pytest.mark.parametrize('layout', [[1, 1], [3, 1, 2], [1, 9, 1, 4], [2] * 10, [1] * 20, [5, 17, 3]])
@pytest.mark.parametrize('subset', [False, True])
def test_work_list_covers_every_stored_tile_once(lib, layout, subset):
    """Against a brute-force walk of the lower triangle: every tile the pairs use is in exactly one strip (per 16-slot chunk the
    kernel runs it), strips are contiguous pieces of one class segment, and a strip serves exactly the pairs that read its tile:
    (a, b) for an off-diagonal block, every pair containing c for c's diagonal block.  No other tile is read."""
    from optiml_amd.ml.svm.onevsone import ovo_pairs
    k = len(layout)
    ct = np.concatenate(([0], np.cumsum(layout)))
    pairs = ovo_pairs(k)
    if subset:
        pairs = pairs[::3]
    cls = np.repeat(np.arange(k), layout)
    want = {}
    for I in range(ct[-1]):
        for J in range(I + 1):
            a, b = cls[J], cls[I]
            cols = {p for p, (i, j) in enumerate(pairs) if (i, j) == (a, b) or (a == b and a in (i, j))}
            if cols:
                want[(I, J)] = cols
    got = {}
    for kind, I, J0, nj, ident in _work(lib, ct, pairs):
        assert nj >= 1
        for J in range(J0, J0 + nj):
            assert (I, J) not in got, (I, J)
            if kind == 0:
                i, j = pairs[ident]
                assert cls[I] == j and cls[J] == i
                assert nj <= 8 and (J0 - ct[i]) % 8 == 0
                got[(I, J)] = {ident}
            else:
                assert cls[I] == cls[J] == ident and J <= I
                assert nj <= 4 and (J0 - ct[ident]) % 4 == 0
                got[(I, J)] = {p for p, pr in enumerate(pairs) if ident in pr}
    assert got == want


def test_slab_bytes_is_the_pairs_local_triangles(lib):
    from optiml_amd import _lib
    ct = np.array([0, 2, 5, 6], dtype=np.int32)
    pr = np.array([0, 1, 0, 2, 1, 2], dtype=np.int32)
    out = C.c_int64(0)
    _lib.check(lib.bq_pairs_slab_bytes(6, 3, _lib.iptr(ct), 3, _lib.iptr(pr), C.byref(out)))
    assert out.value == 8 * 256 * (5 ** 2 + 3 ** 2 + 4 ** 2)


@pytest.mark.parametrize('ct, pairs, nb', [
    ([0, 2, 2, 4], [(0, 1)], 4),      # an empty class
    ([1, 2, 4], [(0, 1)], 4),         # does not start at 0
    ([0, 2, 3], [(0, 1)], 4),         # does not cover the panel
    ([0, 3, 2, 4], [(0, 1)], 4),      # not monotone
    ([0, 2, 4], [(1, 0)], 4),         # a >= b
    ([0, 2, 4], [(0, 2)], 4),         # b out of range
    ([0, 2, 4], [(-1, 1)], 4),        # a out of range
    ([0, 4], [(0, 1)], 4),            # one class
])
def test_argument_errors(lib, ct, pairs, nb):
    from optiml_amd import _lib
    c = np.asarray(ct, dtype=np.int32)
    p = np.asarray(pairs, dtype=np.int32).reshape(-1)
    n = C.c_int64(0)
    assert lib.bq_pairs_work_list(nb, len(c) - 1, _lib.iptr(c), len(pairs), _lib.iptr(p), None, 0, C.byref(n)) == _lib.ERR_BADARG
    assert b'bad argument' in lib.bq_last_error()
    assert lib.bq_pairs_slab_bytes(nb, len(c) - 1, _lib.iptr(c), len(pairs), _lib.iptr(p), C.byref(n)) == _lib.ERR_BADARG


def test_null_arguments_and_short_capacity(lib):
    from optiml_amd import _lib
    c = np.array([0, 1, 2], dtype=np.int32)
    p = np.array([0, 1], dtype=np.int32)
    n = C.c_int64(0)
    assert lib.bq_pairs_work_list(2, 2, None, 1, _lib.iptr(p), None, 0, C.byref(n)) == _lib.ERR_BADARG
    assert lib.bq_pairs_work_list(2, 2, _lib.iptr(c), 1, _lib.iptr(p), None, 0, None) == _lib.ERR_BADARG
    items = np.zeros(5, dtype=np.int32)
    assert lib.bq_pairs_work_list(2, 2, _lib.iptr(c), 1, _lib.iptr(p), _lib.iptr(items), 1, C.byref(n)) == _lib.ERR_BADARG
    assert n.value == 3   # tile (1, 0), and the diagonal tiles of both classes
    assert lib.bq_problem_gram_matmat_pairs(None, 2, _lib.iptr(c), 1, _lib.iptr(p), None, None) == _lib.ERR_BADARG
    assert lib.bq_msolver_create_pairs(None, _lib.PG, 2, _lib.iptr(c), 1, _lib.iptr(p), None, None, None, 1e-6, 10, 0.,
                                       C.byref(C.c_void_p())) == _lib.ERR_BADARG


@pytest.mark.parametrize('k', [2, 3, 4, 7])
@pytest.mark.parametrize('seed', [0, 1])
def test_vote_aggregation_matches_sklearn(k, seed):
    from sklearn.utils.multiclass import _ovr_decision_function
    from optiml_amd.ml.svm.onevsone import ovo_decision
    rs = np.random.RandomState(seed)
    m = k * (k - 1) // 2
    conf = rs.standard_normal((50, m))
    conf[:10] = np.round(conf[:10])        # ties in the confidences and zero decision values
    conf[10:15] = 0.
    pred = (conf > 0).astype(int)
    assert np.array_equal(ovo_decision(pred, conf, k), _ovr_decision_function(pred, conf, k))


def _path_rows():
    from optiml_amd.ml.svm.kernels import GaussianKernel, PolyKernel, linear
    from optiml_amd.ml.svm.losses import hinge
    from optiml_amd.opti.constrained import ActiveSet, FrankWolfe, InteriorPoint, ProjectedGradient
    from optiml_amd.opti.unconstrained.stochastic import AdaGrad
    base = dict(loss=hinge, dual=True, reg_intercept=True, optimizer=ProjectedGradient, kernel=GaussianKernel(gamma=0.5))
    return [
        (dict(base), 1, True),
        (dict(base, kernel=GaussianKernel(gamma='auto')), 1, True),
        (dict(base, kernel=PolyKernel(gamma='auto')), 1, True),
        (dict(base, kernel=linear), 1, True),
        (dict(base, optimizer=FrankWolfe), 1, True),
        (dict(base, storage='f32'), 1, True),
        (dict(base, kernel=GaussianKernel(gamma='scale')), 1, False),
        (dict(base, kernel=PolyKernel(gamma='scale')), 1, False),
        (dict(base, storage='stream'), 1, False),
        (dict(base), 2, False),
        (dict(base, optimizer=ActiveSet), 1, False),
        (dict(base, optimizer=InteriorPoint), 1, False),
        (dict(base, optimizer='smo', reg_intercept=False), 1, False),
        (dict(base, optimizer=AdaGrad, learning_rate=1.), 1, False),
    ]


@pytest.mark.parametrize('row', range(14))
def test_path_selection(row):
    from optiml_amd.ml.svm import SVC
    from optiml_amd.ml.svm.onevsone import uses_batched_ovo
    kw, world, want = _path_rows()[row]
    assert uses_batched_ovo(SVC(**kw), world) is want


def test_constructor_checks_are_svc_s():
    from optiml_amd.ml.svm import OneVsOneSVC
    with pytest.raises(ValueError):
        OneVsOneSVC(C=0)
    with pytest.raises(TypeError):
        OneVsOneSVC(kernel='rbf')
    est = OneVsOneSVC(C=3.)
    assert est.get_params()['C'] == 3.
    assert est.set_params(C=5.)._prototype().C == 5.


def test_grid_search_takes_it_on_the_per_fold_path():
    from optiml_amd.ml.svm import OneVsOneSVC
    from optiml_amd.ml.svm.losses import hinge
    from optiml_amd.ml.svm.model_selection import uses_batched_search
    est = OneVsOneSVC(loss=hinge, dual=True, reg_intercept=True)
    assert uses_batched_search(est, [{'C': 1.}], 1) is False


def test_pair_chunks_follow_memory():
    from optiml_amd.ml.svm import onevsone as ovo
    ct = np.array([0, 4, 8, 12, 16], dtype=np.int32)
    pairs = ovo.ovo_pairs(4)
    per = 16 * 8 * (16 * 256 + 256) + 8 * 256 * 64
    chunks = ovo.pair_chunks(pairs, ct, 16 * 256, free_bytes=2 * 3 * per + 1)
    assert [len(c) for c in chunks] == [3, 3] and sum(chunks, []) == pairs
    assert ovo.pair_chunks(pairs, ct, 16 * 256, free_bytes=1) == [[p] for p in pairs]
