"""The batched row-based SMO (bq_mrsmo_*, csrc/bq_mrsmo.hip): its rows against the exact-argument reference (gram_reference.py) at
the kernel's column, k-block, staging-chunk and group edges; every column step for step against the NumPy restatement
(smo_rows_reference.py) on those rows, alone or in any batch, any cache, any cut; the models against sklearn; the refusals."""
import ctypes as C
import functools
from contextlib import closing

import numpy as np
import pytest

import gram_reference as gr
import smo_rows_reference as ref
from test_gpu_smo_rows import _kernel, _points, amd  # noqa: F401 (the fixture: library loaded, long double checked)

pytestmark = pytest.mark.gpu

COLS = CHUNK = 256   # MR_COLS, MR_KC of csrc/bq_mrsmo.hip: image columns per workgroup, features staged in LDS at a time


class Batch:   # the C entry points themselves (single steps, rows, stats), which RowSMOBatch does not expose
    def __init__(self, X, kernel, columns, tol=1e-3, cache_rows=0, storage='stream', k=None):
        from optiml_amd import _lib
        from optiml_amd.opti import KernelQuadratic
        self._lib, self.lib, self.n, self.k, self.h = _lib, _lib.load(), len(X), len(columns) if k is None else k, C.c_void_p()
        signs, lin, boxes = (np.ascontiguousarray(np.stack(part), dtype=float) for part in zip(*columns))
        self.quad = KernelQuadratic(X, np.zeros(self.n), 'plain', kernel, storage=storage)
        self.N = signs.shape[1]
        rc = self.lib.bq_mrsmo_create(self.quad.device_problem().handle, self.k, self.N, _lib.ptr(signs), _lib.ptr(lin),
                                      _lib.ptr(boxes), float(tol), 0, int(cache_rows), C.byref(self.h))
        if rc:
            self.quad.release()
        _lib.check(rc)

    def close(self):
        self.lib.bq_mrsmo_destroy(self.h)
        self.quad.release()

    def run(self, max_steps):
        steps, fin = (C.c_int64 * self.k)(), (C.c_int * self.k)()
        self._lib.check(self.lib.bq_mrsmo_run(self.h, max_steps, steps, fin))
        return list(steps), list(fin)

    def finish(self, chunk=64):
        steps, fin = self.run(chunk)
        while not all(fin):
            steps, fin = self.run(chunk)
        return steps, fin

    def get(self, what, c, size):
        out = np.empty(size)
        self._lib.check(self.lib.bq_mrsmo_get(self.h, what, c, self._lib.ptr(out)))
        return out

    def vectors(self, c):
        return self.get(self._lib.RSMO_ALPHAS, c, self.N).tobytes(), self.get(self._lib.RSMO_GRADIENT, c, self.N).tobytes()

    def scalars(self, c):
        return dict(zip(('rho', 'gmax', 'gmax2', 'i', 'j', 'steps'), self.get(self._lib.RSMO_SCALARS, c, 6)))

    def stats(self):
        return dict(zip(('hits', 'misses', 'cache_rows'), map(int, self.get(self._lib.RSMO_STATS, 0, 3))))

    def rows(self, idx):
        idx, out = np.ascontiguousarray(idx, dtype=np.int64), np.empty((len(idx), self.n))
        self._lib.check(self.lib.bq_mrsmo_rows(self.h, len(idx), idx.ctypes.data_as(C.POINTER(C.c_int64)), self._lib.ptr(out)))
        return out


MAPS = (('linear', 1), ('poly', 2), ('poly', 3), ('poly', 5), ('rbf', 1), ('sigmoid', 1))
ROW_NS = (129, COLS - 1, COLS, COLS + 1)
ROW_DS = (1, 3, 4, 5, 17)


def _row_cases():
    cases = []
    for k, (name, degree) in enumerate(MAPS):
        for q, n in enumerate(ROW_NS):   # every map meets every n; the d rotate through them
            cases.append(gr.Case('mrsmo', name, degree, n, None, ROW_DS[len(cases) % 5], 9500 + len(cases), (k + q) % 3))
    for name in ('linear', 'rbf', 'poly'):   # the 16 rows staged in two chunks
        cases.append(gr.Case('mrsmo', name, 3, 129, None, CHUNK + 1, 9500 + len(cases), 1))
    return cases


@pytest.mark.parametrize('c', _row_cases(), ids=gr.case_id)
def test_rows_against_the_exact_reference(amd, c):
    sp, X, _, want = gr.exact_reference(c)
    n = c.m
    col = ref.svc_problem(np.where(np.arange(n) % 2 == 0, 1.0, -1.0), np.ones(n))
    with closing(Batch(X, _kernel(sp), [col], cache_rows=40)) as s:
        K = s.rows(np.arange(n))   # calls of 39 rows: groups of 16, 16 and 7, every row a miss
        assert s.stats()['misses'] >= n - 1 and s.stats()['cache_rows'] == 40
        gr.check_exact(gr.case_id(c), c.name, K, want)
        assert K.tobytes() == np.ascontiguousarray(K.T).tobytes(), 'K is not symmetric bit for bit'
        if c.name == 'rbf':
            assert (np.diag(K) == 1.0).all()
        first = 0   # rows 0 .. 79 left the 40 slots long ago; m = 16 and 33 end with a repeat of their first row (a hit)
        for m in (1, 15, 16, 17, 33):   # groups of 1; 15; 15; 16 + 1; 16 + 16 missing rows
            fresh = m - (m in (16, 33))
            idx = list(range(first, first + fresh)) + [first] * (m - fresh)
            first += fresh
            before = s.stats()
            got = s.rows(idx)
            after = s.stats()
            assert (after['hits'] - before['hits'], after['misses'] - before['misses']) == (m - fresh, fresh), m
            assert got.tobytes() == K[idx].tobytes(), f'{m} requested rows'
        before = s.stats()
        assert s.rows([0]).tobytes() == K[[0]].tobytes()   # alone and a miss again: 79 rows went through 40 slots since
        assert s.rows([0]).tobytes() == K[[0]].tobytes()   # ... and a hit
        after = s.stats()
        assert (after['hits'] - before['hits'], after['misses'] - before['misses']) == (1, 1)


@functools.lru_cache(maxsize=None)
def _problem(name):   # (X, kernel, columns, tol) of a seeded batch
    from optiml_amd.ml.svm import kernels as kk
    if name == 'svc300':
        X, y, gamma, *_ = ref.case_problem('svc300')
        y1 = np.where(X[:, 2] + 0.5 * X[:, 3] > 0, 1.0, -1.0)
        y2 = np.where(X[:, 0] > 0, 1.0, -1.0)
        weighted = np.where(y1 > 0, ref.CLASS_WEIGHT[1.0], ref.CLASS_WEIGHT[-1.0])   # the boxes of the `weighted` case's rule
        cols = [ref.svc_problem(y, np.ones(300)), ref.svc_problem(y1, weighted), ref.svc_problem(y2, np.ones(300)),
                ref.svc_problem(y, np.full(300, 0.25))]
        return X, kk.GaussianKernel(gamma), cols, 1e-3
    if name == 'svr300':
        X, y, gamma, *_ = ref.case_problem('svr300')
        cols = [ref.svr_problem(y, np.ones(300), ref.EPSILON), ref.svr_problem(np.cos(X[:, 1]), np.ones(300), ref.EPSILON),
                ref.svr_problem(0.5 * y, np.full(300, 2.0), 0.05)]
        return X, kk.GaussianKernel(gamma), cols, 1e-3
    X, _ = ref.seeded('svc', 1500, 8)   # 'svc1500x17': six label vectors on seventeen columns, six workgroups per column
    labels = [np.where(X[:, c] > 0, 1.0, -1.0) for c in range(6)]
    return X, kk.GaussianKernel(0.2), [ref.svc_problem(labels[c % 6], np.ones(1500)) for c in range(17)], 1e-2


@functools.lru_cache(maxsize=None)
def _reference(name):
    """(K as the device makes it, the reference's run per distinct column, with its trace at n = 300)"""
    X, kern, cols, tol = _problem(name)
    with closing(Batch(X, kern, cols, tol)) as s:
        K = s.rows(np.arange(len(X)))
    wants, seen = [], {}
    for signs, p, Cb in cols:
        key = (signs.tobytes(), p.tobytes(), Cb.tobytes())
        if key not in seen:
            trace = []
            seen[key] = (ref.solve(K, signs, p, Cb, tol, trace=trace if len(X) <= 300 else None), trace)
            assert seen[key][0].status == 'optimal'
        wants.append(seen[key])
    return K, wants


def _same_end(s, c, want, steps, fin):
    assert (steps, fin) == (want.steps, 1), f'column {c}'
    assert s.vectors(c) == (want.alpha.tobytes(), want.G.tobytes()), f'column {c}'
    sc = s.scalars(c)
    np.testing.assert_allclose(sc['rho'], want.rho, rtol=1e-12, atol=0)
    assert (sc['gmax'], sc['gmax2'], sc['steps'], (sc['i'], sc['j'])) == (want.gmax, want.gmax2, want.steps, want.pairs[-1])


@pytest.mark.parametrize('name', ['svc300', 'svr300'])
def test_single_steps_follow_the_reference(amd, name):
    X, kern, cols, tol = _problem(name)
    K, wants = _reference(name)
    counts = [w.steps for w, _ in wants]
    assert len(set(counts)) == len(counts) and max(counts) > 200   # the columns drop out one by one
    with closing(Batch(X, kern, cols, tol)) as s:
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
        assert s.stats()['hits'] + s.stats()['misses'] == 2 * sum(counts)


def test_seventeen_columns_on_several_workgroups_run_to_the_end(amd):
    X, kern, cols, tol = _problem('svc1500x17')
    K, wants = _reference('svc1500x17')
    assert K.tobytes() == np.ascontiguousarray(K.T).tobytes() and (np.diag(K) == 1.0).all()
    with closing(Batch(X, kern, cols, tol)) as s:
        steps, fin = s.finish(256)
        for c, (want, _) in enumerate(wants):
            _same_end(s, c, want, steps[c], fin[c])
        assert s.stats()['hits'] + s.stats()['misses'] == 2 * sum(steps) and s.stats()['misses'] <= len(K)


@pytest.mark.parametrize('cache_rows,chunk', [(2, 64), (300, 64), (0, 1), (5, 7)])
def test_a_column_alone_has_the_bits_it_has_in_the_batch(amd, cache_rows, chunk):
    X, kern, cols, tol = _problem('svc300')
    want = _reference('svc300')[1][1][0]   # the weighted column, held to the reference inside the batch of four above
    with closing(Batch(X, kern, [cols[1]], tol, cache_rows=cache_rows)) as s:
        steps, fin = s.finish(chunk)
        _same_end(s, 0, want, steps[0], fin[0])
        assert (sum(s.stats().values()) - s.stats()['cache_rows'], s.stats()['cache_rows']) == (2 * want.steps, cache_rows or 300)


def test_identical_columns_share_every_row(amd):
    X, kern, cols, tol = _problem('svc300')
    want = _reference('svc300')[1][2][0]
    with closing(Batch(X, kern, [cols[2]], tol)) as s:
        s.finish()
        alone = s.stats()
    with closing(Batch(X, kern, [cols[2], cols[2]], tol)) as s:
        steps, fin = s.finish()
        for c in range(2):
            _same_end(s, c, want, steps[c], fin[c])
        both = s.stats()
    assert both['misses'] == alone['misses'] and both['hits'] + both['misses'] == 2 * sum(steps)


def _ovr(batch_smo, **kw):
    from optiml_amd.ml.svm import OneVsRestSVC, losses
    model = OneVsRestSVC(loss=losses.hinge, dual=True, optimizer='smo', storage='stream', tol=1e-6, C=2.0, **kw)
    model.batch_smo = batch_smo
    return model


def _consistent(ests, X, gamma=None):
    from sklearn.metrics.pairwise import linear_kernel, rbf_kernel
    T = _points(X.shape[1])
    for est in ests:
        Kt = linear_kernel(T, X[est.support_]) if gamma is None else rbf_kernel(T, X[est.support_], gamma=gamma)
        np.testing.assert_allclose(est.decision_function(T), Kt @ est.dual_coef_ + est.intercept_, rtol=0, atol=1e-11)
        assert est.support_vectors_.tobytes() == X[est.support_].tobytes()
        assert est.intercept_ == est.optimizer.b == -est.optimizer.rho
        assert est.optimizer.status == 'optimal' and est.optimizer.iter > 0
    st = ests[0].optimizer.cache_stats   # the shared cache's counts
    assert st['hits'] + st['misses'] == 2 * sum(est.optimizer.iter for est in ests)


def test_one_vs_rest_against_sklearn(amd):
    from sklearn.multiclass import OneVsRestClassifier
    from sklearn.svm import SVC as SkSVC
    from optiml_amd.ml.svm import kernels as kk
    rng = np.random.default_rng(11)
    X = rng.standard_normal((210, 4))
    y = np.argmax(X[:, :3] + 0.3 * rng.standard_normal((210, 3)), axis=1)
    T = np.vstack((X, _points(4)))
    ours = _ovr('rows', kernel=kk.GaussianKernel(0.4)).fit(X, y)
    assert ours.rows_ and ours.batched_ and [type(e.optimizer).__name__ for e in ours.estimators_] == ['RowSMOClassifier'] * 3
    theirs = OneVsRestClassifier(SkSVC(kernel='rbf', gamma=0.4, C=2.0, tol=1e-6, shrinking=False)).fit(X, y)
    assert np.abs(ours.decision_function(T) - theirs.decision_function(T)).max() <= 1e-5
    assert (ours.predict(T) == theirs.predict(T)).all()
    _consistent(ours.estimators_, X, 0.4)
    balanced = _ovr('rows', kernel=kk.GaussianKernel(0.4), class_weight='balanced').fit(X, y)
    single = _ovr(None, kernel=kk.GaussianKernel(0.4), class_weight='balanced').fit(X, y)
    assert not single.batched_ and np.abs(balanced.decision_function(T) - single.decision_function(T)).max() <= 1e-5
    _consistent(balanced.estimators_, X, 0.4)
    lin = _ovr('rows', kernel=kk.LinearKernel()).fit(X, y)
    for est in lin.estimators_:
        np.testing.assert_allclose(est.coef_, est.dual_coef_ @ est.support_vectors_, rtol=1e-12, atol=1e-13)
    _consistent(lin.estimators_, X)


def test_multi_output_against_sklearn(amd):
    from sklearn.svm import SVR as SkSVR
    from optiml_amd.ml.svm import MultiOutputSVR, kernels as kk, losses
    X, y = ref.seeded('svr', 210, 4)
    Y = np.stack((y, np.cos(X[:, 1]), 0.5 * y + X[:, 2]), axis=1)
    T = np.vstack((X, _points(4)))
    ours = MultiOutputSVR(loss=losses.epsilon_insensitive, dual=True, optimizer='smo', storage='stream', tol=1e-6, C=1.0,
                          epsilon=ref.EPSILON, kernel=kk.GaussianKernel(0.5))
    ours.batch_smo = 'rows'
    assert ours.fit(X, Y).rows_
    for c in range(3):
        theirs = SkSVR(kernel='rbf', gamma=0.5, C=1.0, tol=1e-6, epsilon=ref.EPSILON, shrinking=False).fit(X, Y[:, c])
        assert np.abs(ours.predict(T)[:, c] - theirs.predict(T)).max() <= 1e-5
    _consistent(ours.estimators_, X, 0.5)


def test_create_refuses_what_it_does_not_solve(amd):
    from optiml_amd import _lib
    from optiml_amd.ml.svm import kernels as kk
    X, y = ref.seeded('svc', 64, 3)
    kern, good = kk.GaussianKernel(0.5), ref.svc_problem(y, np.ones(64))
    bad_box, bad_sign, bad_lin = (tuple(a.copy() for a in good) for _ in range(3))
    bad_box[2][5], bad_sign[0][7], bad_lin[1][9] = np.inf, 0.5, np.nan
    svr_signs = ref.svr_problem(y, np.ones(64), 0.1)
    svr_signs[0][3] = -1.0   # 2n variables whose signs are not [+1 ..; -1 ..]
    for kw in (dict(storage='f64'), dict(k=0), dict(cache_rows=3), dict(columns=[good, bad_box]), dict(columns=[bad_sign, good]),
               dict(columns=[good, bad_lin]), dict(columns=[svr_signs]), dict(tol=0.0)):
        args = dict(columns=[good, good], tol=1e-3, cache_rows=0, storage='stream', k=None)
        args.update(kw)
        with pytest.raises(_lib.BcqpError) as err:
            Batch(X, kern, **args)
        assert err.value.code == _lib.ERR_BADARG, kw
    with closing(Batch(X, kern, [good, good], cache_rows=4)) as s:   # the same arguments, accepted at the minimum cache
        assert s.finish()[1] == [1, 1]


def test_two_rank_context_is_not_implemented(amd):
    import threading
    from optiml_amd import device
    from optiml_amd.dist import ThreadComm
    from optiml_amd.ml.svm import RowSMOBatch, RowSMOClassifier, kernels as kk
    from optiml_amd.opti import KernelQuadratic
    X, y = ref.seeded('svc', 64, 3)
    members, res = ThreadComm.group(2, timeout=60.0), [None, None]

    def run(k):
        try:
            ctx = device.Context(device=0, comm=members[k], exchange='host')
            quad = KernelQuadratic(X, -np.ones(64), 'svc', kk.GaussianKernel(0.5), y=y, storage='stream', rank_one=False)
            cols = [RowSMOClassifier(quad, X, y, None, kk.GaussianKernel(0.5), 1.0) for _ in range(2)]
            try:
                RowSMOBatch(cols, ctx=ctx).minimize()
            except NotImplementedError:
                res[k] = True
            finally:
                ctx.close()
        except BaseException as exc:  # noqa: BLE001
            res[k] = exc
            members[k].abort()
    threads = [threading.Thread(target=run, args=(k,)) for k in range(2)]
    [t.start() for t in threads]
    [t.join() for t in threads]
    assert res == [True, True]
