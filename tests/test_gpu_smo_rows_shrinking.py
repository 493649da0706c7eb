"""Shrinking in the row-based SMO (bq_rsmo_set_shrinking, csrc/bq_rsmo_shrink.h) on the device, against the restatement WITHOUT
shrinking (tests/smo_rows_reference.py): on the seeded cases the shrunk run takes the reference's pairs, so the reference is a
step-for-step oracle up to the first gradient reconstruction.

1. steps      single steps of svc300, weighted svc300 and svr300 (every 20 and 64) and svc1500 (every 20; two workgroups of list
              positions, six of the shrink pass): until the first reconstruction the pair and alpha have the reference's bits and so
              has G at the active variables; after every shrink pass the active count is that of libsvm's be_shrunk applied in NumPy
              to the reference's state; the list gets shorter than N.  After the step that follows a pass (its rows were made on the
              shrunk list) bq_rsmo_rows on the shrunk solver itself gives the pair's rows whole, with K's bits.
2. rebuild    after the call that makes the first reconstruction (nothing has moved since: G is the full gradient of the device's
              alpha) G against lin + s o (K b) in long double from the same K: per entry within the bound of an n-term sum,
              (n + 2) u sum_j |K_tj b_j| + 2 u |G_t|.
3. end        on to `finished`: optimal; libsvm's violation recomputed from the returned full G over all N variables below
              tol + twice that bound; hits + misses = 2 steps + the rows asked in 1.
4. cuts       svc300, every 20: max_steps 1, 7, 64 per call and cache_rows 2, 17, n give the same steps, alpha bits and shrink
              statistics after every call as cache_rows = n (a stale slot that served a value from outside its list would show here).
5. models     SVC / SVR with `shrinking = True` and RowOneClassSVM(shrinking=True) at tol 1e-6 against sklearn's shrinking=True fits:
              decision values to 1e-5 (the bound of test_smo_rows_host.py), at least one shrink pass.
6. refusals   BQ_ERR_BADARG for a Solver_NU solver, every < 0, a call after the first step, and BQ_RSMO_SHRINK_STATS without shrinking;
              ValueError for GeneralRowSMO(rule='nu', shrinking=True).

Measured on MI355X: the largest |G - reference| / bound of 2 is 0.011 (svc300), 0.013 (weighted), 0.016 (svr300), < 0.0005
(svc1500); smallest active counts 79 / 117 / 156 / 522, two reconstructions per case, the reference's step counts (286, 542, 676,
5950) and violations 9.3e-4 .. 9.9e-4 at the end; of the rows asked from the shrunk solver 5 to 210 per case sat in a slot made on a
shrunk list and were made whole; models within 1.1e-6 (SVC), 8.7e-7 (SVR), 4.9e-7 (one-class) of sklearn."""
import ctypes as C
import functools

import numpy as np
import pytest

import gram_reference as gr
import smo_rows_reference as ref
from test_gpu_smo_rows import Solver, _open, _points, _seeded, amd  # noqa: F401 (the fixture: library loaded, long double checked)

pytestmark = pytest.mark.gpu

TOL = 1e-3


def _shrinking(s, every):
    s._lib.check(s.lib.bq_rsmo_set_shrinking(s.h, every))
    return s


def _stats(s):
    active, smallest, shrinks, rebuilt = s.get(s._lib.RSMO_SHRINK_STATS, 4)
    return dict(active=int(active), smallest=int(smallest), shrinks=int(shrinks), rebuilt=int(rebuilt))


def _be_shrunk(y, alpha, Cb, G, active):
    """libsvm's be_shrunk on the Gmax1 / Gmax2 of the active set"""
    up = np.where(y > 0, alpha < Cb, alpha > 0) & active
    low = np.where(y > 0, alpha > 0, alpha < Cb) & active
    g1 = np.where(y > 0, -G, G)[up].max() if up.any() else -np.inf
    g2 = np.where(y > 0, G, -G)[low].max() if low.any() else -np.inf
    upper = np.where(y > 0, -G > g1, -G > g2)
    lower = np.where(y > 0, G > g2, G > g1)
    return np.where(alpha >= Cb, upper, np.where(alpha <= 0, lower, False))


@functools.lru_cache(maxsize=None)
def _reference(name, weighted):
    """(K as the device makes it, the run without shrinking and its trace)"""
    task, X, y, kern, signs, p, Cfull, boxes = _seeded(name, weighted)
    with _open(name, weighted, TOL) as s:
        K = s.rows(np.arange(len(X)))
    trace = []
    want = ref.solve(K, signs, p, Cfull, TOL, trace=trace)
    assert want.status == 'optimal'
    return K, want, trace


def _rebuilt_bound(K, signs, p, alpha, G):
    """(lin + s o (K b) in long double, the bound of an n-term sum per entry)"""
    n, rep = len(K), len(signs) // len(K)
    b = (signs * alpha).astype(gr.LD).reshape(rep, n).sum(axis=0)
    Kb = K.astype(gr.LD) @ b
    exact = p.astype(gr.LD) + signs.astype(gr.LD) * np.tile(Kb, rep)
    bound = (n + 2) * gr.U * np.tile(np.abs(K).astype(gr.LD) @ np.abs(b), rep) + 2 * gr.U * np.abs(G).astype(gr.LD)
    return exact, bound


CASES = [('svc300', False, 20), ('svc300', False, 64), ('svc300', True, 20), ('svc300', True, 64), ('svr300', False, 20),
         ('svr300', False, 64), ('svc1500', False, 20)]


@pytest.mark.parametrize('name,weighted,every', CASES)
def test_shrunk_run_follows_the_reference(amd, name, weighted, every):
    K, want, trace = _reference(name, weighted)
    task, X, y, kern, signs, p, Cfull, boxes = _seeded(name, weighted)
    N = len(signs)
    active, shrinks, asked, remade = np.ones(N, dtype=bool), 0, 0, 0
    with _shrinking(_open(name, weighted, TOL), every) as s:
        # 1. until the first reconstruction
        for k in range(want.steps):
            steps, fin = s.run(1)
            st = _stats(s)
            if st['rebuilt']:
                break
            assert (steps, fin) == (k + 1, 0)
            if st['shrinks'] > shrinks:   # a pass before step k, on the state after step k - 1
                assert st['shrinks'] == shrinks + 1 and k % every == 0
                shrinks += 1
                active &= ~_be_shrunk(signs, trace[k - 1][0], Cfull, trace[k - 1][1], active)
            assert st['active'] == active.sum(), f'active count at step {k}'
            sc = s.scalars()
            assert (sc['i'], sc['j']) == want.pairs[k], f'step {k}'
            assert s.alpha().tobytes() == trace[k][0].tobytes(), f'alpha after step {k}'
            assert s.gradient()[active].tobytes() == trace[k][1][active].tobytes(), f'active G after step {k}'
            if k and k % every == 0 and st['active'] < N:
                # the step after a pass made its rows on the shrunk list: bq_rsmo_rows on THIS solver still gives whole rows
                pair, before = np.array(want.pairs[k]) % len(K), s.stats()['misses']
                assert s.rows(pair).tobytes() == K[pair].tobytes(), f'rows {pair} asked after step {k}'
                asked, remade = asked + 2, remade + s.stats()['misses'] - before
        assert st['rebuilt'] == 1 and shrinks >= 1 and st['smallest'] < N, 'the run never shrank'
        assert remade >= 1, 'no asked row sat in a slot made on a shrunk list'
        smallest, first = st['smallest'], steps
        # 2. the reconstructed gradient
        alpha, G = s.alpha(), s.gradient()
        exact, bound = _rebuilt_bound(K, signs, p, alpha, G)
        ratio = float((np.abs(G.astype(gr.LD) - exact) / bound).max())
        print(f'{name} weighted={weighted} every={every}: first reconstruction in the call to step {first}, active {smallest} of {N}, '
              f'|G - exact| / bound <= {ratio:.2e}')
        assert ratio <= 1.0
        # 3. the end
        steps, fin = s.finish()
        st, cache = _stats(s), s.stats()
        alpha, G = s.alpha(), s.gradient()
    assert fin == 1 and st['active'] == N
    up = np.where(signs > 0, alpha < Cfull, alpha > 0)
    low = np.where(signs > 0, alpha > 0, alpha < Cfull)
    violation = np.where(signs > 0, -G, G)[up].max() + np.where(signs > 0, G, -G)[low].max()
    slack = 2 * float(_rebuilt_bound(K, signs, p, alpha, G)[1].max())
    print(f'    {steps} steps (reference {want.steps}), violation {violation:.3e}, {st}, {cache}, {remade} of {asked} asked rows remade')
    assert violation < TOL + slack
    assert cache['hits'] + cache['misses'] == 2 * steps + asked


# ---- 4. cuts and cache ----------------------------------------------------------------------------------------------------------------------
def _calls(chunk, cache_rows):
    """(steps, alpha, shrink statistics) after every call of a svc300 run with a shrink pass every 20 steps"""
    out = []
    with _shrinking(_open('svc300', cache_rows=cache_rows), 20) as s:
        fin = 0
        while not fin:
            steps, fin = s.run(chunk)
            out.append((steps, s.alpha().tobytes(), tuple(_stats(s).values())))
        cache = s.stats()
    assert fin == 1 and cache['hits'] + cache['misses'] == 2 * steps
    return out


@functools.lru_cache(maxsize=None)
def _whole_cache(chunk):
    return _calls(chunk, ref.CASES['svc300'][1])


@pytest.mark.parametrize('chunk', [1, 7, 64])
def test_cuts_and_cache_sizes_reach_the_same_run(amd, chunk):
    base = _whole_cache(chunk)
    assert base[-1][2][1] < 300 and base[-1][2][3] >= 1
    assert base[-1] == _whole_cache(64)[-1]
    for R in (2, 17):
        got = _calls(chunk, R)
        assert len(got) == len(base)
        for k, (a, b) in enumerate(zip(got, base)):
            assert a == b, f'cache_rows={R}, call {k}'


# ---- 5. models -------------------------------------------------------------------------------------------------------------------------------
def test_models_against_sklearn_with_shrinking(amd):
    from sklearn import svm as sk
    from optiml_amd.ml.svm import SVC, SVR, RowOneClassSVM, kernels as kk, losses
    kw = dict(dual=True, optimizer='smo', storage='stream', tol=1e-6)
    for task, ours, theirs in (
            ('svc', lambda g, c: SVC(loss=losses.hinge, kernel=kk.GaussianKernel(g), C=c, **kw),
             lambda g, c: sk.SVC(kernel='rbf', gamma=g, C=c, tol=1e-6, shrinking=True)),
            ('svr', lambda g, c: SVR(loss=losses.epsilon_insensitive, kernel=kk.GaussianKernel(g), C=c, epsilon=ref.EPSILON, **kw),
             lambda g, c: sk.SVR(kernel='rbf', gamma=g, C=c, tol=1e-6, epsilon=ref.EPSILON, shrinking=True)),
            ('one', lambda g, c: RowOneClassSVM(kernel=kk.GaussianKernel(g), nu=0.3, tol=1e-6, shrinking=True),
             lambda g, c: sk.OneClassSVM(kernel='rbf', gamma=g, nu=0.3, tol=1e-6, shrinking=True))):
        _, n, d, gamma, Cval = ref.CASES['svr300' if task == 'svr' else 'svc300']
        X, y = ref.seeded('svr' if task == 'svr' else 'svc', n, d)
        T = np.vstack((X, _points(d)))
        a = ours(gamma, Cval)
        a.shrinking = True
        a.fit(X, y)
        b = theirs(gamma, Cval).fit(X, y)
        mine = a.predict(T) if task == 'svr' else a.decision_function(T)
        err = np.abs(mine - (b.predict(T) if task == 'svr' else b.decision_function(T))).max()
        st = a.shrink_stats_ if task == 'one' else a.optimizer.shrink_stats
        print(f'{task}: max decision difference {err:.3e}, {st}')
        assert err <= 1e-5
        assert st['shrinks'] >= 1 and st['active'] == (2 * n if task == 'svr' else n)


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------------------------
def test_refusals(amd):
    from optiml_amd import _lib
    from optiml_amd.ml.svm.nu_rows import GeneralRowSMO
    lib = _lib.load()

    def refused(call):
        with pytest.raises(_lib.BcqpError) as err:
            _lib.check(call())
        return err.value.code == _lib.ERR_BADARG

    with _open('svc300') as s:
        assert refused(lambda: lib.bq_rsmo_set_shrinking(s.h, -1))
        assert refused(lambda: lib.bq_rsmo_get(s.h, _lib.RSMO_SHRINK_STATS, _lib.ptr(np.empty(4))))
        assert refused(lambda: lib.bq_rsmo_get(s.h, _lib.RSMO_SHRINK_STATS + 1, _lib.ptr(np.empty(8))))
        assert refused(lambda: lib.bq_rsmo_get(s.h, _lib.RSMO_NU_SCALARS, _lib.ptr(np.empty(7))))
        s.run(1)
        assert refused(lambda: lib.bq_rsmo_set_shrinking(s.h, 20))
        task, X, y, kern, signs, p, Cfull, boxes = _seeded('svc300')
        h = C.c_void_p()
        _lib.check(lib.bq_rsmo_create_general(s.quad.device_problem().handle, _lib.RSMO_RULE_NU, len(y), _lib.ptr(signs),
                                              _lib.ptr(np.zeros(len(y))), _lib.ptr(np.ones(len(y))), _lib.ptr(np.full(len(y), 0.25)),
                                              TOL, 0, 0, C.byref(h)))
        try:
            assert refused(lambda: lib.bq_rsmo_set_shrinking(h, 20))
        finally:
            lib.bq_rsmo_destroy(h)
        with pytest.raises(ValueError):
            GeneralRowSMO(s.quad, X, signs, np.zeros(len(y)), np.ones(len(y)), np.full(len(y), 0.25), 'nu', shrinking=True)
