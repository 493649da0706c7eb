"""The general entry of the row-based SMO (bq_rsmo_create_general, csrc/bq_rsmo.hip) on the device: libsvm's Solver from a nonzero
start (the one-class dual) and Solver_NU (nu-SVC, nu-SVR) on kernel rows made on demand.  K always comes from bq_rsmo_rows, and the
NumPy restatement (tests/smo_nu_reference.py) is seeded with the device's own alpha0 and G0.

1. start      alpha read back has alpha0's bits; G0 against the long-double sum_j K_ij b_j of the rows, per entry within
              (n + 16) 2^-53 sum_j |K_ij b_j| — derived, not measured: any summation order of n terms, plus 8 u per entry for each
              of the two Gram routes (the row kernel's and the product's; test_gpu_gram_edges / gram_reference); nu-SVR (alpha and
              alpha* start equal, b = 0): G0 has p's bits.  At n = 300 and at n = 129, 257.
2. steps      the three n = 300 cases at tol 1e-3, single-stepped: the same (i, j), alpha and G bits at each of the first 200 steps,
              then the same end (steps, bits, rho, r, both stop sums); the three n = 1500 cases (six workgroups) to the end.
3. edges      the two-row pass: nu-SVC at n = 255, 256, 257 with d = 515 (x staged in two chunks) and n = 129 with d = 17,
              alternating labels, nu = 0.5, cache_rows = 3 (rows recomputed constantly, alone and in pairs): 30 single steps, bits.
4. cache      cache_rows 3, 4, 17, n on nu-SVC 300 and 2, 3, n on one-class 300: identical pairs and bits; hits and misses equal a
              host model of the cache replayed on the restatement's trace (requests per step ip, in, j; a request for a row the
              step already holds is a hit; a missing side requests nothing); with n rows at most n misses.
5. cuts       runs cut into calls of 1, 7 and 64 steps on nu-SVR 300 with cache_rows 5: the same bits and step count.
6. models     RowOneClassSVM / RowNuSVC / RowNuSVR at tol 1e-6 against sklearn's feature-space fits (same gamma, nu, C,
              shrinking=False) on the n = 300 cases plus 64 fresh points: the bounds of test_smo_nu_host.py (1e-5; nu-SVC on
              r x decision), predict agreement where |decision| > 1e-4, attribute consistency, group masses, boxes, and
              hits + misses equal to the model's count.
7. scope      BQ_ERR_BADARG for a resident problem, NU with cache_rows 2, alpha0 above its box, one-sign NU labels, a NaN in lin;
              an infeasible nu raises ValueError before device work; max_iter = 10 gives 'stopped', n_iter_ == 10 and the warning;
              a two-rank context raises NotImplementedError; NuSVC(storage='stream') still refuses."""
import ctypes as C
import functools
import warnings

import numpy as np
import pytest

import gram_reference as gr
import smo_nu_reference as nu
import smo_rows_reference as ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def amd():
    from optiml_amd import _lib
    from optiml_amd.device import get_context
    assert np.finfo(gr.LD).nmant >= 63
    _lib.load()
    get_context()


def _gaussian(gamma):
    from optiml_amd.ml.svm import kernels as kk
    return kk.GaussianKernel(gamma)


class Solver:
    """bq_rsmo_create_general on a streamed KernelQuadratic"""

    def __init__(self, X, kernel, signs, lin, boxes, alpha0, rule, tol=1e-3, max_steps=0, cache_rows=0, storage='stream'):
        from optiml_amd import _lib
        from optiml_amd.opti import KernelQuadratic
        self._lib, self.lib = _lib, _lib.load()
        self.n, self.N, self.rule = len(X), len(signs), rule
        self.quad = KernelQuadratic(X, np.zeros(self.n), 'plain', kernel, storage=storage)
        self.h = C.c_void_p()
        vecs = [_lib.as_f64(v, self.N) for v in (signs, lin, boxes, alpha0)]
        try:
            _lib.check(self.lib.bq_rsmo_create_general(self.quad.device_problem().handle,
                                                       _lib.RSMO_RULE_NU if rule == 'nu' else _lib.RSMO_RULE_PLAIN, self.N,
                                                       *(_lib.ptr(v) for v in vecs), float(tol), int(max_steps), int(cache_rows),
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
        """the solver's scalars under the restatement's names"""
        if self.rule == 'nu':
            rho, r, gap_p, gap_n, i, j, steps = self.get(self._lib.RSMO_NU_SCALARS, 7)
            assert self.get(self._lib.RSMO_SCALARS, 6)[0] == rho   # BQ_RSMO_SCALARS of a NU solver: the same rho in slot 0
            return dict(rho=rho, r=r, gap_p=gap_p, gap_n=gap_n, i=int(i), j=int(j), steps=int(steps))
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


# ---- the problems ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case(name):
    """(X, kernel, (signs, p, C, alpha0), rule) of a seeded case of smo_nu_reference, or of an edge case 'kind-n-d'"""
    if name in nu.CASES:
        X, y, gamma, (signs, p, Cb, alpha0, rule) = nu.case_problem(name)
        return X, _gaussian(gamma), (signs, p, Cb, alpha0), rule
    kind, n, d = name.split('-')
    n, d = int(n), int(d)
    X = np.random.default_rng(1000 * n + d).standard_normal((n, d))
    if kind == 'oc':
        signs, p, Cb, alpha0, rule = nu.one_class_problem(n, 0.3)
    else:
        signs, p, Cb, alpha0, rule = nu.nu_svc_problem(np.where(np.arange(n) % 2 == 0, 1.0, -1.0), 0.5)
    return X, _gaussian(1.0 / d), (signs, p, Cb, alpha0), rule


def _open(name, tol=1e-3, cache_rows=0, max_steps=0):
    X, kern, (signs, p, Cb, alpha0), rule = _case(name)
    return Solver(X, kern, signs, p, Cb, alpha0, rule, tol, max_steps, cache_rows)


@functools.lru_cache(maxsize=None)
def _start(name):
    """(K as the device makes it, the device's alpha0 and G0)"""
    with _open(name) as s:
        a0, G0 = s.alpha(), s.gradient()
        K = s.rows(np.arange(s.n))
    for v in (K, a0, G0):
        v.setflags(write=False)
    return K, a0, G0


@functools.lru_cache(maxsize=None)
def _reference(name, tol=1e-3):
    """(K, the restatement's run on it from the device's start, its trace for n <= 300)"""
    X, kern, (signs, p, Cb, alpha0), rule = _case(name)
    K, a0, G0 = _start(name)
    trace = []
    want = nu.solve(rule, K, signs, p, Cb, tol, a0, G0, trace=trace if len(X) <= 300 else None)
    assert want.status == 'optimal'
    return K, want, trace


# ---- 1. the start ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['oc300', 'nusvc300', 'nusvr300', 'oc-129-17', 'nusvc-129-17', 'oc-257-17', 'nusvc-257-17'])
def test_start_alpha_and_gradient(amd, name):
    X, kern, (signs, p, Cb, alpha0), rule = _case(name)
    K, a0, G0 = _start(name)
    n, N = len(X), len(signs)
    assert a0.tobytes() == alpha0.tobytes()
    assert K.tobytes() == np.ascontiguousarray(K.T).tobytes()
    b = (signs * alpha0).reshape(N // n, n).sum(axis=0)
    if name == 'nusvr300':
        assert not b.any() and G0.tobytes() == p.tobytes()
        return
    assert b.any() and not p.any()
    KL, bL = K.astype(gr.LD), b.astype(gr.LD)
    want = np.tile(KL @ bL, N // n)                      # long double: sum_j K_ij b_j
    mass = np.tile(np.abs(KL) @ np.abs(bL), N // n)      # sum_j |K_ij b_j|
    err = np.abs((signs * G0).astype(gr.LD) - want)      # G0 = s o (K b): lin = 0
    bound = (n + 16) * gr.LD(2.0) ** -53 * mass
    print(f'{name}: max error / bound {float((err / bound).max()):.3f}')
    assert (err <= bound).all()


# ---- 2. step for step --------------------------------------------------------------------------------------------------------------------
def _same_end(s, want, steps, fin):
    assert (steps, fin) == (want.steps, 1)
    assert s.alpha().tobytes() == want.alpha.tobytes()
    assert s.gradient().tobytes() == want.G.tobytes()
    sc = s.scalars()
    assert sc['rho'] == want.rho and sc['steps'] == want.steps
    if s.rule == 'nu':
        assert (sc['r'], sc['gap_p'], sc['gap_n']) == (want.r, want.gap_p, want.gap_n)
    else:
        assert (sc['gmax'], sc['gmax2']) == (want.gmax, want.gmax2)
    assert (sc['i'], sc['j']) == want.pairs[-1]


def _requests(want, n, rule):
    """the rows a run asks the cache for, step by step: ((row, rows to keep), ...) per step"""
    steps = []
    for k, (i, j) in enumerate(want.pairs):
        if rule == 'nu':
            ip, i_n = want.sides[k]
            rp, rn = (ip % n if ip >= 0 else None), (i_n % n if i_n >= 0 else None)
            reqs = []
            if rp is not None:
                reqs.append((rp, ()))
            if rn is not None:
                reqs.append((rn, (rp,)))
            reqs.append((j % n, (rp, rn)))
        else:
            reqs = [(i % n, ()), (j % n, (i % n,))]
        steps.append(reqs)
    return steps


def _cache_model(want, n, R, rule, cut=None):
    """hits and misses of the device's cache: least recently used goes, never a row the step holds; a row the step already holds
    (or any row in the cache) is a hit.  cut: the run was stopped after `cut` steps — the selection of the next step has asked for
    its rows (not yet for j's)"""
    stamp, clock, hits, misses = {}, 0, 0, 0
    steps = _requests(want, n, rule)
    if cut is not None:
        steps = steps[:cut] + [steps[cut][:-1]]
    for reqs in steps:
        for row, keep in reqs:
            clock += 1
            if row in stamp:
                hits += 1
            else:
                misses += 1
                if len(stamp) == R:
                    del stamp[min((r for r in stamp if r not in keep), key=stamp.get)]
            stamp[row] = clock
    return hits, misses


@pytest.mark.parametrize('name', ['oc300', 'nusvc300', 'nusvr300'])
def test_single_steps_follow_the_reference(amd, name):
    K, want, trace = _reference(name)
    assert want.steps > 200
    with _open(name) as s:
        for k in range(200):
            assert s.run(1) == (k + 1, 0)
            sc = s.scalars()
            assert (sc['i'], sc['j']) == want.pairs[k], f'step {k}'
            assert s.alpha().tobytes() == trace[k][0].tobytes(), f'alpha after step {k}'
            assert s.gradient().tobytes() == trace[k][1].tobytes(), f'G after step {k}'
        _same_end(s, want, *s.finish())
        st = s.stats()
    assert st['hits'] + st['misses'] == sum(len(r) for r in _requests(want, len(K), s.rule))
    print(f'{name}: {want.steps} steps, {st}')


@pytest.mark.parametrize('name', ['oc1500', 'nusvc1500', 'nusvr1500'])
def test_several_workgroups_run_to_the_end(amd, name):
    K, want, _ = _reference(name)
    with _open(name) as s:
        _same_end(s, want, *s.finish(512))
        st = s.stats()
    assert st['hits'] + st['misses'] == sum(len(r) for r in _requests(want, len(K), s.rule)) and st['misses'] <= len(K)
    print(f'{name}: {want.steps} steps, {st}')


# ---- 3. the edges of the two-row pass ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['nusvc-255-515', 'nusvc-256-515', 'nusvc-257-515', 'nusvc-129-17'])
def test_two_row_pass_at_the_slice_and_chunk_edges(amd, name):
    X, kern, (signs, p, Cb, alpha0), rule = _case(name)
    K, a0, G0 = _start(name)
    trace = []
    want = nu.solve_nu(K, signs, p, Cb, 1e-3, a0, G0, steps_only=31, trace=trace)   # (step 31: the rows its selection asks for)
    assert want.steps == 31
    with _open(name, cache_rows=3) as s:
        for k in range(30):
            assert s.run(1) == (k + 1, 0)
            sc = s.scalars()
            assert (sc['i'], sc['j']) == want.pairs[k], f'step {k}'
            assert s.alpha().tobytes() == trace[k][0].tobytes(), f'alpha after step {k}'
            assert s.gradient().tobytes() == trace[k][1].tobytes(), f'G after step {k}'
        st = s.stats()
    hits, misses = _cache_model(want, len(X), 3, 'nu', cut=30)
    print(f'{name}: {st}, model {hits} hits {misses} misses')
    assert (st['hits'], st['misses']) == (hits, misses) and misses > 30   # rows are made again and again, alone and in pairs


# ---- 4. the cache does not exist ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,sizes', [('nusvc300', (3, 4, 17, 300)), ('oc300', (2, 3, 300))])
def test_nothing_depends_on_the_cache(amd, name, sizes):
    K, want, trace = _reference(name)
    n = len(K)
    for R in sizes:
        pairs = []
        with _open(name, cache_rows=R) as s:
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
        hits, misses = _cache_model(want, n, R, s.rule)
        print(f'{name} cache_rows={R}: {st}, model {hits} hits {misses} misses')
        assert st['cache_rows'] == R
        assert (st['hits'], st['misses']) == (hits, misses)
        if R == n:
            assert st['misses'] <= n


# ---- 5. however the run is cut -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('chunk', [1, 7, 64])
def test_cuts_reach_the_same_bits(amd, chunk):
    K, want, _ = _reference('nusvr300')
    with _open('nusvr300', cache_rows=5) as s:
        _same_end(s, want, *s.finish(chunk))


# ---- 6. model level ----------------------------------------------------------------------------------------------------------------------
def _points(d):
    return np.random.default_rng(7).standard_normal((64, d))


def _model_checks(name, model, X, gamma):
    """what the three estimators share: the run is the restatement's at tol 1e-6 (bits and request count), the attributes agree"""
    from sklearn.metrics.pairwise import rbf_kernel
    K, want, _ = _reference(name, 1e-6)
    assert model.status_ == 'optimal' and model.n_iter_ == want.steps
    assert model.alphas_.tobytes() == want.alpha.tobytes()
    st = model.cache_stats_
    assert st['hits'] + st['misses'] == sum(len(r) for r in _requests(want, len(X), 'plain' if name == 'oc300' else 'nu'))
    assert model.kkt_violation_ < 1e-6
    T = _points(X.shape[1])
    dec = rbf_kernel(T, model.support_vectors_, gamma=gamma) @ model.dual_coef_ + model.intercept_
    np.testing.assert_allclose(model.decision_function(T), dec, rtol=0, atol=1e-11 * max(1.0, float(np.abs(model.dual_coef_).sum())))
    assert model.support_vectors_.tobytes() == X[model.support_].tobytes()
    return want, T


def test_one_class_against_sklearn(amd):
    from sklearn.svm import OneClassSVM as Sk
    from optiml_amd.ml.svm import RowOneClassSVM
    kind, n, d, gamma, nu_, Cval = nu.CASES['oc300']
    X = nu.one_class_data(n, d)
    ours = RowOneClassSVM(kernel=_gaussian(gamma), nu=nu_, tol=1e-6).fit(X)
    want, T = _model_checks('oc300', ours, X, gamma)
    theirs = Sk(kernel='rbf', gamma=gamma, nu=nu_, tol=1e-6, shrinking=False).fit(X)
    P = np.vstack((X, T))
    a, b = ours.decision_function(P), theirs.decision_function(P)
    err = float(np.abs(a - b).max())
    print(f'one-class: {ours.n_iter_} steps (sklearn {theirs.n_iter_}), max decision difference {err:.3e}')
    assert err <= 1e-5
    sure = np.abs(b) > 1e-4
    assert (ours.predict(P)[sure] == theirs.predict(P)[sure]).all()
    assert ours.offset_ == want.rho == -ours.intercept_
    assert (ours.alphas_ >= 0).all() and (ours.alphas_ <= 1).all()
    assert abs(float(ours.alphas_.sum()) - nu_ * n) <= 1e-12 * nu_ * n
    assert (ours.dual_coef_ == ours.alphas_[ours.support_]).all() and (ours.alphas_[ours.support_] > 0).all()
    np.testing.assert_allclose(ours.score_samples(T) - ours.offset_, ours.decision_function(T), rtol=0, atol=0)


def test_nu_svc_against_sklearn(amd):
    from sklearn.svm import NuSVC as Sk
    from optiml_amd.ml.svm import RowNuSVC
    kind, n, d, gamma, nu_, Cval = nu.CASES['nusvc300']
    X, y = ref.seeded('svc', n, d)
    ours = RowNuSVC(kernel=_gaussian(gamma), nu=nu_, tol=1e-6).fit(X, y)
    want, T = _model_checks('nusvc300', ours, X, gamma)
    theirs = Sk(kernel='rbf', gamma=gamma, nu=nu_, tol=1e-6, shrinking=False).fit(X, y)
    P = np.vstack((X, T))
    a, b = ours.decision_function(P), theirs.decision_function(P)
    r = ours.margin_scale_
    err = float(np.abs(r * a - r * b).max())   # r x decision: the unscaled dual's, which tol bounds
    print(f'nu-SVC: {ours.n_iter_} steps (sklearn {theirs.n_iter_}), r = {r:.4g}, max difference of r x decision {err:.3e} '
          f'(raw {float(np.abs(a - b).max()):.3e})')
    assert err <= 1e-5
    sure = np.abs(b) > 1e-4
    assert (ours.predict(P)[sure] == theirs.predict(P)[sure]).all()
    assert r == want.r and r > 0 and ours.intercept_ == -want.rho / r
    assert (ours.alphas_ >= 0).all() and (ours.alphas_ <= 1).all()
    for g in (y > 0, y < 0):
        assert abs(float(ours.alphas_[g].sum()) - nu_ * n / 2) <= 1e-12 * nu_ * n / 2
    assert (ours.dual_coef_ == (y * ours.alphas_)[ours.support_] / r).all()
    assert list(ours.classes_) == [-1.0, 1.0]


def test_nu_svr_against_sklearn(amd):
    from sklearn.svm import NuSVR as Sk
    from optiml_amd.ml.svm import RowNuSVR
    kind, n, d, gamma, nu_, Cval = nu.CASES['nusvr300']
    X, y = ref.seeded('svr', n, d)
    ours = RowNuSVR(kernel=_gaussian(gamma), nu=nu_, C=Cval, tol=1e-6).fit(X, y)
    want, T = _model_checks('nusvr300', ours, X, gamma)
    theirs = Sk(kernel='rbf', gamma=gamma, nu=nu_, C=Cval, tol=1e-6, shrinking=False).fit(X, y)
    P = np.vstack((X, T))
    err = float(np.abs(ours.predict(P) - theirs.predict(P)).max())
    print(f'nu-SVR: {ours.n_iter_} steps (sklearn {theirs.n_iter_}), max decision difference {err:.3e}, epsilon {ours.epsilon_:.4g}')
    assert err <= 1e-5
    assert ours.intercept_ == -want.rho and ours.epsilon_ == -want.r and ours.epsilon_ > 0
    assert (ours.alphas_ >= 0).all() and (ours.alphas_ <= Cval).all()
    for half in (ours.alphas_[:n], ours.alphas_[n:]):
        assert abs(float(half.sum()) - Cval * nu_ * n / 2) <= 1e-12 * Cval * nu_ * n / 2
    assert (ours.dual_coef_ == (ours.alphas_[:n] - ours.alphas_[n:])[ours.support_]).all() and (ours.dual_coef_ != 0).all()


# ---- 7. scope and errors -----------------------------------------------------------------------------------------------------------------
def test_create_refuses_what_it_does_not_solve(amd):
    from optiml_amd import _lib
    X, y = ref.seeded('svc', 64, 3)
    kern = _gaussian(0.5)
    signs, p, Cb, alpha0, rule = nu.nu_svc_problem(y, 0.3)
    above = alpha0.copy()
    above[int(np.argmax(alpha0))] = 1.5
    nan_lin = p.copy()
    nan_lin[7] = np.nan
    good = dict(signs=signs, lin=p, boxes=Cb, alpha0=alpha0, rule='nu', cache_rows=0, storage='stream')
    for kw in (dict(storage='f64'), dict(cache_rows=2), dict(alpha0=above), dict(signs=np.ones(64)), dict(lin=nan_lin)):
        a = dict(good, **kw)
        with pytest.raises(_lib.BcqpError) as err:
            Solver(X, kern, a['signs'], a['lin'], a['boxes'], a['alpha0'], a['rule'], cache_rows=a['cache_rows'], storage=a['storage'])
        assert err.value.code == _lib.ERR_BADARG, kw
    with Solver(X, kern, signs, p, Cb, alpha0, 'nu', cache_rows=3) as s:   # the same arguments, accepted
        assert s.finish()[1] == 1
    with Solver(X, kern, np.ones(64), p, Cb, nu.one_class_start(64, 0.3), 'plain', cache_rows=2) as s:   # one sign, two rows: PLAIN takes both
        assert s.finish()[1] == 1


def test_infeasible_nu_raises_before_device_work(amd, monkeypatch):
    from optiml_amd.ml.svm import RowNuSVC, nu_rows
    X, y = ref.seeded('svc', 64, 3)
    y[:60] = 1.0
    y[60:] = -1.0

    def no_device(*a, **k):
        raise AssertionError('device work before the feasibility check')
    monkeypatch.setattr(nu_rows, 'KernelQuadratic', no_device)
    with pytest.raises(ValueError, match='infeasible'):
        RowNuSVC(kernel=_gaussian(0.5), nu=0.5).fit(X, y)


def test_max_iter_stops_with_a_warning(amd):
    from optiml_amd.ml.svm import RowNuSVC, RowNuSVR, RowOneClassSVM
    from optiml_amd.ml.svm._base import ConvergenceWarning
    X, y = ref.seeded('svc', 300, 5)
    for make, args in ((lambda **kw: RowNuSVC(nu=0.3, **kw), (X, y)), (lambda **kw: RowNuSVR(nu=0.5, **kw), (X, np.sin(X[:, 0]))),
                       (lambda **kw: RowOneClassSVM(nu=0.2, **kw), (X,))):
        with pytest.warns(ConvergenceWarning):
            model = make(kernel=_gaussian(0.5), max_iter=10).fit(*args)
        assert model.status_ == 'stopped' and model.n_iter_ == 10
        with warnings.catch_warnings():
            warnings.simplefilter('error')
            model = make(kernel=_gaussian(0.5)).fit(*args)
        assert model.status_ == 'optimal' and model.n_iter_ > 10


def test_two_rank_context_is_not_implemented(amd):
    import threading
    from optiml_amd import device
    from optiml_amd.dist import ThreadComm
    from optiml_amd.ml.svm.nu_rows import GeneralRowSMO
    from optiml_amd.opti import KernelQuadratic
    X, y = ref.seeded('svc', 64, 3)
    signs, p, Cb, alpha0, rule = nu.nu_svc_problem(y, 0.3)

    def body(member):
        ctx = device.Context(device=0, comm=member, exchange='host')
        try:
            quad = KernelQuadratic(X, np.zeros(64), 'plain', _gaussian(0.5), storage='stream')
            with pytest.raises(NotImplementedError):
                GeneralRowSMO(quad, X, signs, p, Cb, alpha0, rule, ctx=ctx).minimize()
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


def test_resident_nu_classes_still_refuse_stream(amd):
    from optiml_amd.ml.svm import NuSVC, OneClassSVM
    X, y = ref.seeded('svc', 64, 3)
    with pytest.raises(NotImplementedError):
        NuSVC(kernel=_gaussian(0.5), nu=0.3, storage='stream').fit(X, y)
    with pytest.raises(NotImplementedError):
        OneClassSVM(kernel=_gaussian(0.5), nu=0.3, storage='stream').fit(X)
