"""The row-list form of the batched row-based SMO (bq_mrsmo_create_lists, the ml_* kernels of csrc/bq_mrsmo.hip): every list column
step for step against the NumPy restatement (smo_rows_reference.py) on the device's own rows K[rows][:, rows], at the slice edges,
alone or in any batch, any cache, any cut; OneVsOneSVC(batch_smo='rows') against sklearn; the refusals."""
import ctypes as C
import functools
from contextlib import closing

import numpy as np
import pytest

import smo_rows_reference as ref
from test_gpu_smo_rows import _points, amd  # noqa: F401 (the fixture: library loaded, long double checked)
from test_gpu_smo_rows_batched import Batch, _same_end

pytestmark = pytest.mark.gpu

MR_SLICE = 2048   # RSMO_T * ML_PER of csrc/bq_mrsmo.hip: positions per workgroup of ml_select_kernel / ml_update_kernel


class ListBatch(Batch):   # bq_mrsmo_create_lists; columns: (rows, signs, lin, boxes)
    def __init__(self, X, kernel, columns, tol=1e-3, cache_rows=0, storage='stream', k=None, offsets=None):
        from optiml_amd import _lib
        from optiml_amd.opti import KernelQuadratic
        self._lib, self.lib, self.n, self.k, self.h = _lib, _lib.load(), len(X), len(columns) if k is None else k, C.c_void_p()
        self.m = [len(col[0]) for col in columns]
        rows, signs, lin, boxes = (np.concatenate(part) for part in zip(*columns))
        offsets = np.ascontiguousarray(np.concatenate(([0], np.cumsum(self.m))) if offsets is None else offsets, dtype=np.int64)
        rows, signs, lin, boxes = _lib.as_i32(rows), _lib.as_f64(signs), _lib.as_f64(lin), _lib.as_f64(boxes)
        self.quad = KernelQuadratic(X, np.zeros(self.n), 'plain', kernel, storage=storage)
        rc = self.lib.bq_mrsmo_create_lists(self.quad.device_problem().handle, self.k, offsets.ctypes.data_as(C.POINTER(C.c_int64)),
                                            _lib.iptr(rows), _lib.ptr(signs), _lib.ptr(lin), _lib.ptr(boxes), float(tol), 0,
                                            int(cache_rows), C.byref(self.h))
        if rc:
            self.quad.release()
        _lib.check(rc)

    def vectors(self, c):
        return self.get(self._lib.RSMO_ALPHAS, c, self.m[c]).tobytes(), self.get(self._lib.RSMO_GRADIENT, c, self.m[c]).tobytes()


def _column(rows, y, boxes=None):
    return (np.asarray(rows),) + ref.svc_problem(y, np.ones(len(rows)) if boxes is None else boxes)


@functools.lru_cache(maxsize=None)
def _problem(name):   # (X, kernel, list columns, tol)
    from optiml_amd.ml.svm import kernels as kk
    if name == 'svc300':   # three classes by terciles of feature 0: the pairs, one weighted pair, one list of all rows
        X, y, gamma, *_ = ref.case_problem('svc300')
        codes = np.searchsorted(np.quantile(X[:, 0], [1 / 3, 2 / 3]), X[:, 0])
        cols = []
        for i, j in ((0, 1), (0, 2), (1, 2), (0, 2)):
            rows = np.flatnonzero((codes == i) | (codes == j))
            yp = np.where(codes[rows] == j, 1.0, -1.0)
            cols.append(_column(rows, yp, np.where(yp > 0, ref.CLASS_WEIGHT[1.0], ref.CLASS_WEIGHT[-1.0]) if len(cols) == 3 else None))
        return X, kk.GaussianKernel(gamma), cols + [_column(np.arange(300), y)], 1e-3
    X, _ = ref.seeded('svc', 4200, 8)   # 'edges': random ascending lists at the slice edges, labels from a linear rule
    rng, cols = np.random.default_rng(5), []
    for m in (MR_SLICE - 1, MR_SLICE, MR_SLICE + 1, 2 * MR_SLICE + 1):
        rows = np.sort(rng.choice(4200, m, replace=False))
        cols.append(_column(rows, np.where(X[rows, 0] + 0.5 * X[rows, 1] > 0, 1.0, -1.0)))
    return X, kk.GaussianKernel(0.2), cols, 1e-2


@functools.lru_cache(maxsize=None)
def _reference(name):
    """(K as the device makes it, per column the reference's run on K[rows][:, rows] and its trace at n = 300)"""
    X, kern, cols, tol = _problem(name)
    with closing(ListBatch(X, kern, cols[:1], tol)) as s:
        K = s.rows(np.arange(len(X)))
    wants = []
    for rows, signs, p, Cb in cols:
        trace = []
        wants.append((ref.solve(K[np.ix_(rows, rows)], signs, p, Cb, tol, trace=trace if len(X) <= 300 else None), trace))
        assert wants[-1][0].status == 'optimal'
    return K, wants


def test_single_steps_follow_the_reference(amd):
    X, kern, cols, tol = _problem('svc300')
    _, wants = _reference('svc300')
    with closing(ListBatch(X, kern, cols, tol)) as s:
        for k in range(200):
            steps, fin = s.run(1)
            for c, (want, trace) in enumerate(wants):
                if k >= want.steps:
                    assert (steps[c], fin[c]) == (want.steps, 1)
                    continue
                sc = s.scalars(c)
                assert (steps[c], sc['i'], sc['j']) == (k + 1,) + want.pairs[k], f'column {c} step {k}'
                assert s.vectors(c) == (trace[k][0].tobytes(), trace[k][1].tobytes()), f'alpha, G of column {c} after step {k}'
        steps, fin = s.finish()
        for c, (want, _) in enumerate(wants):
            _same_end(s, c, want, steps[c], fin[c])
        assert s.stats()['hits'] + s.stats()['misses'] == 2 * sum(steps)
        whole = s.vectors(4)
    with closing(Batch(X, kern, [cols[4][1:]], tol)) as s:   # the list of all rows is the full column
        s.finish()
        assert s.vectors(0) == whole


def test_slice_edges(amd):
    X, kern, cols, tol = _problem('edges')
    K, wants = _reference('edges')
    with closing(ListBatch(X, kern, cols, tol)) as s:
        steps, fin = s.finish(256)
        for c, (want, _) in enumerate(wants):
            _same_end(s, c, want, steps[c], fin[c])
        assert s.stats()['hits'] + s.stats()['misses'] == 2 * sum(steps)
    with closing(ListBatch(X, kern, [cols[2]], tol, cache_rows=2)) as s:   # alone, the smallest cache, cut into 7-step calls
        steps, fin = s.finish(7)
        _same_end(s, 0, wants[2][0], steps[0], fin[0])


def test_identical_pairs_share_every_row(amd):
    X, kern, cols, tol = _problem('svc300')
    _, wants = _reference('svc300')
    with closing(ListBatch(X, kern, [cols[0]], tol)) as s:
        s.finish()
        alone = s.stats()
    with closing(ListBatch(X, kern, [cols[0], cols[0], cols[2]], tol)) as s:
        steps, fin = s.finish()
        for c, w in enumerate((0, 0, 2)):
            _same_end(s, c, wants[w][0], steps[c], fin[c])
        three = s.stats()
    with closing(ListBatch(X, kern, [cols[2]], tol)) as s:
        s.finish()
        other = s.stats()
    assert alone['cache_rows'] == 300 and three['hits'] + three['misses'] == 2 * sum(steps)
    assert three['misses'] <= alone['misses'] + other['misses']   # the second copy of pair (0, 1) adds no miss ...
    assert three['misses'] <= len(np.union1d(cols[0][0], cols[2][0]))   # ... and no row is made twice
    with closing(ListBatch(X, kern, [cols[0], cols[0]], tol)) as s:
        s.finish()
        assert s.stats()['misses'] == alone['misses']


def _ovo(batch_smo, storage='stream', **kw):
    from optiml_amd.ml.svm import OneVsOneSVC, losses
    model = OneVsOneSVC(loss=losses.hinge, dual=True, optimizer='smo', storage=storage, tol=1e-6, C=2.0, **kw)
    model.batch_smo = batch_smo
    return model


def _confidences(model, T):   # per pair, positive for the pair's larger class
    if model.batched_decision_:
        return model.decision_batch_(T)
    return np.stack([np.ravel(e.decision_function(T)) for e in model.estimators_], axis=1)


def test_one_vs_one_against_sklearn(amd):
    from sklearn.multiclass import OneVsOneClassifier
    from sklearn.svm import SVC as SkSVC
    from optiml_amd.ml.svm import kernels as kk
    rng = np.random.default_rng(11)
    X = rng.standard_normal((260, 4))
    y = np.argmax(X + 0.3 * rng.standard_normal((260, 4)), axis=1)
    T = np.vstack((X, _points(4)))
    ours = _ovo('rows', kernel=kk.GaussianKernel(0.4)).fit(X, y)
    assert ours.rows_ and ours.batched_ and len(ours.estimators_) == 6
    assert all(type(e.optimizer).__name__ == 'RowSMOClassifier' and e.optimizer.status == 'optimal' for e in ours.estimators_)
    sk = dict(kernel='rbf', gamma=0.4, C=2.0, tol=1e-6, shrinking=False)
    theirs = SkSVC(decision_function_shape='ovo', **sk).fit(X, y).decision_function(T)   # sklearn: positive for the smaller class
    assert np.abs(_confidences(ours, T) + theirs).max() <= 1e-5
    assert (ours.predict(T) == OneVsOneClassifier(SkSVC(**sk)).fit(X, y).predict(T)).all()
    cw = {0: 3.0, 2: 0.5}
    weighted = _ovo('rows', kernel=kk.GaussianKernel(0.4), class_weight=cw).fit(X, y)
    single = _ovo(None, kernel=kk.GaussianKernel(0.4), class_weight=cw).fit(X, y)
    assert weighted.rows_ and not single.batched_
    assert np.abs(_confidences(weighted, T) - _confidences(single, T)).max() <= 1e-5
    for est in _ovo('rows', kernel=kk.LinearKernel()).fit(X, y).estimators_:
        np.testing.assert_allclose(est.coef_, est.dual_coef_ @ est.support_vectors_, rtol=1e-12, atol=1e-13)
    with pytest.raises(ValueError):
        _ovo('rows', storage='f64', kernel=kk.GaussianKernel(0.4)).fit(X, y)


BAD = {'descending': dict(rows=[3, 2, 5]), 'repeated': dict(rows=[2, 2, 5]), 'below 0': dict(rows=[-1, 2, 5]),
       'beyond n': dict(rows=[2, 5, 64]), 'empty column': dict(offsets=[0, 3, 3]), 'offsets not from 0': dict(offsets=[1, 3, 6]),
       'offsets descend': dict(offsets=[0, 4, 3]), 'k = 0': dict(k=0), 'k = 1025': dict(k=1025), 'cache of 3 rows': dict(cache_rows=3),
       'box': dict(box=np.inf), 'zero box': dict(box=0.0), 'sign': dict(sign=0.5), 'lin': dict(lin=np.nan), 'tol': dict(tol=0.0),
       'resident': dict(storage='f64')}


@pytest.mark.parametrize('case', BAD)
def test_create_refuses_what_it_does_not_solve(amd, case):
    from optiml_amd import _lib
    from optiml_amd.ml.svm import kernels as kk
    X, y = ref.seeded('svc', 64, 3)
    kw = dict(BAD[case])
    rows = np.array(kw.pop('rows', [2, 4, 5]))
    first = [rows, y[[2, 4, 5]].copy(), -np.ones(3), np.ones(3)]
    for at, name in ((1, 'sign'), (2, 'lin'), (3, 'box')):
        first[at][1] = kw.pop(name, first[at][1])
    with pytest.raises(_lib.BcqpError) as err:
        ListBatch(X, kk.GaussianKernel(0.5), [tuple(first), _column([1, 7, 9], y[[1, 7, 9]])], **kw)
    assert err.value.code == _lib.ERR_BADARG


def test_a_column_of_one_sign_finishes_at_its_first_selection(amd):
    from optiml_amd.ml.svm import kernels as kk
    X, y = ref.seeded('svc', 64, 3)
    rows = np.arange(0, 64, 2)
    with closing(ListBatch(X, kk.GaussianKernel(0.5), [_column(rows, np.ones(32)), _column(rows, y[rows])], cache_rows=4)) as s:
        assert s.run(1)[1][0] == 1 and s.scalars(0)['steps'] == 0 and not s.get(s._lib.RSMO_ALPHAS, 0, 32).any()
        steps, fin = s.finish()
        assert steps[0] == 0 and fin == [1, 1] and steps[1] > 0
