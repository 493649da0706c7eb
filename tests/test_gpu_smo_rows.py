"""The row-based SMO (bq_rsmo_*, csrc/bq_rsmo.hip) on the device: libsvm's WSS2 decomposition on kernel rows made on demand from
a streamed problem's image, rows kept in an LRU cache managed on the device.

1. rows       bq_rsmo_rows against the exact-argument long-double reference of tests/gram_reference.py (its inputs, its bound:
              8 u |ref|, equal bits for the integer linear kernel) for linear, poly 2 / 3 / 5, rbf and sigmoid at n = 255, 256, 257
              (the row kernel's 256-column workgroup slice) and 129 (the image's 128-row padding), d in {1, 17, 65}, and d = 515 (x_i
              staged in two chunks of 512 features); K = K' bit for bit, the RBF diagonal exactly 1, a row read as a miss and as a
              hit has the same bits.  (A streamed problem still refuses the Laplacian kernel — test_gpu_gram_edges.py — so no
              Laplacian row exists to check.)
2. steps      K from bq_rsmo_rows goes to the NumPy restatement (tests/smo_rows_reference.py); the device, single-stepped, takes
              the same (i, j) and has alpha and G with the same bits at each of the first 200 steps of the n = 300 SVC, SVR and
              class-weighted problems, then at the end (tol 1e-3) the same step count, bits and rho; the same at n = 1500 (six
              workgroups).
3. cache      cache_rows 2, 3, 17 and n: identical pairs and bits, hits + misses = 2 steps, and the counts a host model of the
              cache under the victim rule predicts — with n rows at most n misses, with 2 two misses on every step whose rows
              both change.
4. cuts       max_steps 1, 7 and 64 reach the same bits and step count.
5. models     SVC / SVR(optimizer='smo', storage='stream') at tol 1e-6 against sklearn's fits with the same gamma and C: decision
              values to 1e-5 (the bound of test_smo_rows_host.py: both stop at a violation of tol, measured 1 - 4 tol there);
              attribute consistency, the linear kernel's coef_, sample_weight with dropped rows, class_weight='balanced', and
              OneVsRestSVC against one fit per class.
6. scope      BQ_ERR_BADARG for a resident problem, cache_rows = 1, one-class labels and a non-finite box; NotImplementedError on
              a two-rank context; the iteration cap (hook rsmo_max_steps) gives 'stopped' and the ConvergenceWarning."""
import ctypes as C
import functools
import warnings

import numpy as np
import pytest

import gram_reference as gr
import smo_rows_reference as ref
from conftest import set_hooks

pytestmark = pytest.mark.gpu

SLICE = 256   # RSMO_T of csrc/bq_rsmo.hip: columns per workgroup


@pytest.fixture(scope='module')
def amd():
    from optiml_amd import _lib
    from optiml_amd.device import get_context
    assert np.finfo(gr.LD).nmant >= 63
    _lib.load()
    get_context()


def _kernel(sp):
    from optiml_amd.ml.svm import kernels as kk
    name, gamma, coef0, degree = sp
    return {'linear': lambda: kk.LinearKernel(), 'poly': lambda: kk.PolyKernel(degree, gamma, coef0),
            'rbf': lambda: kk.GaussianKernel(gamma), 'sigmoid': lambda: kk.SigmoidKernel(gamma, coef0)}[name]()


class Solver:
    """bq_rsmo_* on a streamed KernelQuadratic"""

    def __init__(self, X, kernel, task, y, boxes, epsilon=0.0, tol=1e-3, cache_rows=0, storage='stream'):
        from optiml_amd import _lib
        from optiml_amd.opti import KernelQuadratic
        self._lib, self.lib = _lib, _lib.load()
        self.n = len(X)
        self.N = 2 * self.n if task == 'svr' else self.n
        self.quad = KernelQuadratic(X, np.zeros(self.n), 'plain', kernel, storage=storage)
        self.h = C.c_void_p()
        y, boxes = _lib.as_f64(y, self.n), _lib.as_f64(boxes, self.n)
        try:
            _lib.check(self.lib.bq_rsmo_create(self.quad.device_problem().handle, _lib.SVR if task == 'svr' else _lib.SVC,
                                               _lib.ptr(y), _lib.ptr(boxes), float(epsilon), float(tol), int(cache_rows),
                                               C.byref(self.h)))
        except Exception:
            self.quad.release()
            raise

    def close(self):
        self.lib.bq_rsmo_destroy(self.h)
        self.quad.release()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def run(self, max_steps):
        steps, fin = C.c_int64(0), C.c_int(0)
        self._lib.check(self.lib.bq_rsmo_run(self.h, max_steps, C.byref(steps), C.byref(fin)))
        return steps.value, fin.value

    def finish(self, chunk=64):
        steps, fin = self.run(chunk)
        while not fin:
            steps, fin = self.run(chunk)
        return steps, fin

    def get(self, what, size):
        out = np.empty(size)
        self._lib.check(self.lib.bq_rsmo_get(self.h, what, self._lib.ptr(out)))
        return out

    def alpha(self):
        return self.get(self._lib.RSMO_ALPHAS, self.N)

    def gradient(self):
        return self.get(self._lib.RSMO_GRADIENT, self.N)

    def scalars(self):
        rho, gmax, gmax2, i, j, steps = self.get(self._lib.RSMO_SCALARS, 6)
        return dict(rho=rho, gmax=gmax, gmax2=gmax2, i=int(i), j=int(j), steps=int(steps))

    def stats(self):
        hits, misses, rows = self.get(self._lib.RSMO_STATS, 3)
        return dict(hits=int(hits), misses=int(misses), cache_rows=int(rows))

    def rows(self, idx):
        idx = np.ascontiguousarray(idx, dtype=np.int64)
        out = np.empty((len(idx), self.n))
        self._lib.check(self.lib.bq_rsmo_rows(self.h, len(idx), idx.ctypes.data_as(C.POINTER(C.c_int64)), self._lib.ptr(out)))
        return out


# ---- 1. rows ---------------------------------------------------------------------------------------------------------------------------
MAPS = (('linear', 1), ('poly', 2), ('poly', 3), ('poly', 5), ('rbf', 1), ('sigmoid', 1))
ROW_NS = (129, SLICE - 1, SLICE, SLICE + 1)
ROW_DS = (1, 17, 65)


def _row_cases():
    cases = []
    for k, (name, degree) in enumerate(MAPS):
        for q, n in enumerate(ROW_NS):   # every map meets every n, and every d at one of them
            cases.append(gr.Case('rsmo', name, degree, n, None, ROW_DS[(k + q) % 3], 9000 + len(cases), (k + q) % 3))
    for name in ('linear', 'rbf', 'poly'):   # x_i staged in two chunks
        cases.append(gr.Case('rsmo', name, 3, 129, None, 515, 9000 + len(cases), 1))
    return cases


@pytest.mark.parametrize('c', _row_cases(), ids=gr.case_id)
def test_rows_against_the_exact_reference(amd, c):
    sp, X, _, want = gr.exact_reference(c)
    n = c.m
    y = np.where(np.arange(n) % 2 == 0, 1.0, -1.0)
    with Solver(X, _kernel(sp), 'svc', y, np.ones(n), cache_rows=3) as s:
        K = s.rows(np.arange(n))
        before = s.stats()
        again = s.rows([n - 1, n - 1, 0])        # a hit, a hit, a miss (three slots, n - 1 was the last row in)
        after = s.stats()
    gr.check_exact(gr.case_id(c), c.name, K, want)
    assert K.tobytes() == np.ascontiguousarray(K.T).tobytes(), 'K is not symmetric bit for bit'
    if c.name == 'rbf':
        assert (np.diag(K) == 1.0).all()
    assert before['misses'] >= n - 1 and before['cache_rows'] == 3
    assert (after['hits'] - before['hits'], after['misses'] - before['misses']) == (2, 1)
    assert again.tobytes() == K[[n - 1, n - 1, 0]].tobytes()


# ---- 2. step for step --------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _seeded(name, weighted=False):
    from optiml_amd.ml.svm import kernels as kk
    task, n, d, gamma, Cval = ref.CASES[name]
    X, y, gamma, signs, p, Cfull = ref.case_problem(name, weighted)
    return task, X, y, kk.GaussianKernel(gamma), signs, p, Cfull, Cfull[:n]


def _open(name, weighted=False, tol=1e-3, cache_rows=0):
    task, X, y, kern, signs, p, Cfull, boxes = _seeded(name, weighted)
    return Solver(X, kern, task, y, boxes, ref.EPSILON if task == 'svr' else 0.0, tol, cache_rows)


@functools.lru_cache(maxsize=None)
def _reference(name, weighted=False, tol=1e-3):
    """(K as the device makes it, the reference's run on it with its trace)"""
    task, X, y, kern, signs, p, Cfull, boxes = _seeded(name, weighted)
    with _open(name, weighted, tol) as s:
        K = s.rows(np.arange(len(X)))
    trace = []
    want = ref.solve(K, signs, p, Cfull, tol, trace=trace if len(X) <= 300 else None)
    assert want.status == 'optimal'
    return K, want, trace


def _same_end(s, want, steps, fin):
    assert (steps, fin) == (want.steps, 1)
    assert s.alpha().tobytes() == want.alpha.tobytes()
    assert s.gradient().tobytes() == want.G.tobytes()
    sc = s.scalars()
    np.testing.assert_allclose(sc['rho'], want.rho, rtol=1e-12, atol=0)
    assert (sc['gmax'], sc['gmax2'], sc['steps']) == (want.gmax, want.gmax2, want.steps)
    assert (sc['i'], sc['j']) == want.pairs[-1]


@pytest.mark.parametrize('name,weighted', [('svc300', False), ('svr300', False), ('svc300', True)])
def test_single_steps_follow_the_reference(amd, name, weighted):
    K, want, trace = _reference(name, weighted)
    assert want.steps > 200
    with _open(name, weighted) as s:
        assert s.run(1) == (1, 0) or want.steps == 1
        for k in range(200):
            if k:
                assert s.run(1) == (k + 1, 0)
            sc = s.scalars()
            assert (sc['i'], sc['j']) == want.pairs[k], f'step {k}'
            assert s.alpha().tobytes() == trace[k][0].tobytes(), f'alpha after step {k}'
            assert s.gradient().tobytes() == trace[k][1].tobytes(), f'G after step {k}'
        _same_end(s, want, *s.finish())
        st = s.stats()
        assert st['hits'] + st['misses'] == 2 * want.steps
    print(f'{name} weighted={weighted}: {want.steps} steps, {st}')


@pytest.mark.parametrize('name', ['svc1500', 'svr1500'])
def test_several_workgroups_run_to_the_end(amd, name):
    K, want, _ = _reference(name)
    assert K.tobytes() == np.ascontiguousarray(K.T).tobytes() and (np.diag(K) == 1.0).all()
    with _open(name) as s:
        _same_end(s, want, *s.finish(512))
        st = s.stats()
    assert st['hits'] + st['misses'] == 2 * want.steps and st['misses'] <= len(K)
    print(f'{name}: {want.steps} steps, {st}')


# ---- 3. the cache does not exist -----------------------------------------------------------------------------------------------------
def _cache_model(pairs, n, R):
    """hits and misses of the device's cache on the requests i_0, j_0, i_1, j_1, ...: least recently used goes, never the slot of the
    pair's other row; (hits, misses, steps whose two rows both missed)"""
    stamp, clock, hits, misses, both = {}, 0, 0, 0, 0
    for i, j in pairs:
        ri, rj = i % n, j % n
        missed = 0
        for row, keep in ((ri, None), (rj, ri)):
            clock += 1
            if row in stamp:
                hits += 1
            else:
                misses += 1
                missed += 1
                if len(stamp) == R:
                    del stamp[min((r for r in stamp if r != keep), key=stamp.get)]
            stamp[row] = clock
        both += missed == 2
    return hits, misses, both


def test_nothing_depends_on_the_cache(amd):
    K, want, trace = _reference('svc300')
    n = len(K)
    for R in (2, 3, 17, n):
        pairs = []
        with _open('svc300', cache_rows=R) as s:
            steps, fin = s.run(1)
            while not fin:
                sc = s.scalars()
                pairs.append((sc['i'], sc['j']))
                steps, fin = s.run(1)
            if len(pairs) < steps:   # the step that also finished the run
                sc = s.scalars()
                pairs.append((sc['i'], sc['j']))
            _same_end(s, want, steps, fin)
            st = s.stats()
        assert pairs == want.pairs, f'cache_rows={R}'
        hits, misses, both = _cache_model(want.pairs, n, R)
        print(f'cache_rows={R}: {st}, model {hits} hits {misses} misses')
        assert st['cache_rows'] == R and st['hits'] + st['misses'] == 2 * want.steps
        assert (st['hits'], st['misses']) == (hits, misses)
        if R == n:
            assert st['misses'] <= n
        if R == 2:
            # two slots hold exactly the previous pair's rows: a step misses twice iff both of its rows changed (and the first step)
            changed = sum(1 for k in range(1, len(pairs)) if not {v % n for v in pairs[k]} & {v % n for v in pairs[k - 1]})
            assert both == changed + 1


# ---- 4. however the run is cut -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('chunk', [1, 7, 64])
def test_cuts_reach_the_same_bits(amd, chunk):
    K, want, _ = _reference('svr300')
    with _open('svr300', cache_rows=5) as s:
        _same_end(s, want, *s.finish(chunk))


# ---- 5. model level ---------------------------------------------------------------------------------------------------------------------
def _svc(**kw):
    from optiml_amd.ml.svm import SVC, losses
    return SVC(loss=losses.hinge, dual=True, optimizer='smo', storage='stream', tol=1e-6, **kw)


def _svr(**kw):
    from optiml_amd.ml.svm import SVR, losses
    return SVR(loss=losses.epsilon_insensitive, dual=True, optimizer='smo', storage='stream', tol=1e-6, **kw)


def _points(d):
    return np.random.default_rng(7).standard_normal((64, d))


def _consistent(model, X, gamma):
    from sklearn.metrics.pairwise import rbf_kernel
    T = _points(X.shape[1])
    dec = rbf_kernel(T, X[model.support_], gamma=gamma) @ model.dual_coef_ + model.intercept_
    np.testing.assert_allclose(model.decision_function(T), dec, rtol=0, atol=1e-11)
    assert model.support_vectors_.tobytes() == X[model.support_].tobytes()
    assert model.intercept_ == model.optimizer.b == -model.optimizer.rho
    assert model.optimizer.status == 'optimal' and model.optimizer.iter > 0
    st = model.optimizer.cache_stats
    assert st['hits'] + st['misses'] == 2 * model.optimizer.iter


def test_svc_against_sklearn(amd):
    from sklearn.svm import SVC as SkSVC
    from optiml_amd.ml.svm import kernels as kk
    task, n, d, gamma, Cval = ref.CASES['svc300']
    X, y = ref.seeded(task, n, d)
    T = _points(d)
    for cw in (None, 'balanced'):
        ours = _svc(kernel=kk.GaussianKernel(gamma), C=Cval, class_weight=cw).fit(X, y)
        theirs = SkSVC(kernel='rbf', gamma=gamma, C=Cval, tol=1e-6, shrinking=False, class_weight=cw).fit(X, y)
        err = np.abs(ours.decision_function(np.vstack((X, T))) - theirs.decision_function(np.vstack((X, T)))).max()
        print(f'SVC class_weight={cw}: {ours.optimizer.iter} steps (sklearn {theirs.n_iter_}), max decision difference {err:.3e}')
        assert err <= 1e-5
        assert (ours.predict(T) == theirs.predict(T)).all()
        _consistent(ours, X, gamma)


def test_svc_sample_weight_drops_rows(amd):
    from sklearn.svm import SVC as SkSVC
    from optiml_amd.ml.svm import kernels as kk
    task, n, d, gamma, Cval = ref.CASES['svc300']
    X, y = ref.seeded(task, n, d)
    w = np.random.default_rng(3).uniform(0.5, 2.0, n)
    w[::7] = 0.0
    keep = w > 0
    ours = _svc(kernel=kk.GaussianKernel(gamma), C=Cval).fit(X, y, sample_weight=w)
    kept = _svc(kernel=kk.GaussianKernel(gamma), C=Cval).fit(X[keep], y[keep], sample_weight=w[keep])
    assert (ours.alphas_[~keep] == 0).all() and ours.alphas_[keep].tobytes() == kept.alphas_.tobytes()
    assert (ours.alphas_ <= Cval * w).all() and not np.isin(np.flatnonzero(~keep), ours.support_).any()
    theirs = SkSVC(kernel='rbf', gamma=gamma, C=Cval, tol=1e-6, shrinking=False).fit(X, y, sample_weight=w)
    err = np.abs(ours.decision_function(X) - theirs.decision_function(X)).max()
    print(f'SVC sample_weight: max decision difference {err:.3e}')
    assert err <= 1e-5


def test_svr_against_sklearn(amd):
    from sklearn.svm import SVR as SkSVR
    from optiml_amd.ml.svm import kernels as kk
    task, n, d, gamma, Cval = ref.CASES['svr300']
    X, y = ref.seeded(task, n, d)
    T = _points(d)
    ours = _svr(kernel=kk.GaussianKernel(gamma), C=Cval, epsilon=ref.EPSILON).fit(X, y)
    theirs = SkSVR(kernel='rbf', gamma=gamma, C=Cval, tol=1e-6, epsilon=ref.EPSILON, shrinking=False).fit(X, y)
    err = np.abs(ours.predict(np.vstack((X, T))) - theirs.predict(np.vstack((X, T)))).max()
    print(f'SVR: {ours.optimizer.iter} steps (sklearn {theirs.n_iter_}), max decision difference {err:.3e}')
    assert err <= 1e-5
    _consistent(ours, X, gamma)
    assert abs(float((ours.optimizer.alphas_p - ours.optimizer.alphas_n).sum())) <= 1e-9 and (np.abs(ours.dual_coef_) <= Cval).all()


def test_linear_kernel_coef(amd):
    from optiml_amd.ml.svm import kernels as kk
    task, n, d, gamma, Cval = ref.CASES['svc300']
    X, y = ref.seeded(task, n, d)
    ours = _svc(kernel=kk.LinearKernel(), C=Cval).fit(X, y)
    np.testing.assert_allclose(ours.coef_, ours.dual_coef_ @ ours.support_vectors_, rtol=1e-12, atol=1e-13)
    T = _points(d)
    np.testing.assert_allclose(ours.decision_function(T), T @ ours.coef_ + ours.intercept_, rtol=0, atol=1e-12)
    assert abs(float(ours.optimizer.alphas @ ours.optimizer.y)) <= 1e-9


def test_one_vs_rest_runs_one_fit_per_class(amd):
    from optiml_amd.ml.svm import OneVsRestSVC, kernels as kk, losses
    rng = np.random.default_rng(11)
    X = rng.standard_normal((210, 4))
    y = np.argmax(X[:, :3] + 0.3 * rng.standard_normal((210, 3)), axis=1)
    kw = dict(loss=losses.hinge, dual=True, optimizer='smo', storage='stream', tol=1e-4, kernel=kk.GaussianKernel(0.4), C=2.0)
    ovr = OneVsRestSVC(**kw).fit(X, y)
    assert not ovr.batched_ and len(ovr.estimators_) == 3
    from optiml_amd.ml.svm import SVC
    for c, est in enumerate(ovr.estimators_):
        one = SVC(**kw).fit(X, (y == c).astype(int))
        assert est.alphas_.tobytes() == one.alphas_.tobytes() and est.intercept_ == one.intercept_
        assert type(est.optimizer).__name__ == 'RowSMOClassifier'
    assert (ovr.predict(X) == y).mean() > 0.7


# ---- 6. scope and errors -----------------------------------------------------------------------------------------------------------------
def test_create_refuses_what_it_does_not_solve(amd):
    from optiml_amd import _lib
    from optiml_amd.ml.svm import kernels as kk
    X, y = ref.seeded('svc', 64, 3)
    kern, ones = kk.GaussianKernel(0.5), np.ones(64)
    bad_box = ones.copy()
    bad_box[5] = np.inf
    for kw in (dict(storage='f64'), dict(cache_rows=1), dict(y=ones), dict(boxes=bad_box), dict(boxes=np.zeros(64))):
        args = dict(y=y, boxes=ones, cache_rows=0, storage='stream')
        args.update(kw)
        with pytest.raises(_lib.BcqpError) as err:
            Solver(X, kern, 'svc', args['y'], args['boxes'], cache_rows=args['cache_rows'], storage=args['storage'])
        assert err.value.code == _lib.ERR_BADARG, kw
    with Solver(X, kern, 'svc', y, ones) as s:   # the same arguments, accepted
        assert s.finish()[1] == 1


def test_two_rank_context_is_not_implemented(amd):
    import threading
    from optiml_amd import device
    from optiml_amd.dist import ThreadComm
    from optiml_amd.ml.svm import RowSMOClassifier, kernels as kk
    from optiml_amd.opti import KernelQuadratic
    X, y = ref.seeded('svc', 64, 3)

    def body(member):
        ctx = device.Context(device=0, comm=member, exchange='host')
        try:
            quad = KernelQuadratic(X, -np.ones(64), 'svc', kk.GaussianKernel(0.5), y=y, storage='stream', rank_one=False)
            with pytest.raises(NotImplementedError):
                RowSMOClassifier(quad, X, y, None, kk.GaussianKernel(0.5), 1.0, ctx=ctx).minimize()
        finally:
            ctx.close()
        return True

    members, res = ThreadComm.group(2, timeout=60.0), [None, None]

    def run(k):
        try:
            res[k] = body(members[k])
        except BaseException as exc:  # noqa: BLE001
            res[k] = exc
            members[k].abort()
    threads = [threading.Thread(target=run, args=(k,)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert res == [True, True]


def test_iteration_cap_stops_with_a_warning(amd, monkeypatch):
    from optiml_amd.ml.svm import kernels as kk
    from optiml_amd.ml.svm._base import ConvergenceWarning
    task, n, d, gamma, Cval = ref.CASES['svc300']
    X, y = ref.seeded(task, n, d)
    set_hooks(monkeypatch, rsmo_max_steps=10)
    with pytest.warns(ConvergenceWarning):
        model = _svc(kernel=kk.GaussianKernel(gamma), C=Cval).fit(X, y)
    assert model.optimizer.status == 'stopped' and model.optimizer.iter == 10
    set_hooks(monkeypatch, rsmo_max_steps=None)
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        model = _svc(kernel=kk.GaussianKernel(gamma), C=Cval).fit(X, y)
    assert model.optimizer.status == 'optimal'
