"""The general entries of the batched row-based SMO (bq_mrsmo_create_general / _create_lists_general, csrc/bq_mrsmo_nu.h): the start
gradient of nonzero starts against a NumPy loop of its definition, bit for bit; every column — libsvm's Solver from the one-class
start, Solver_NU on nu-SVC / nu-SVR, full columns and row lists — step for step against the NumPy restatement
(smo_nu_reference.py) on the device's own rows, seeded with the device's own alpha0 and G0; the slice edges; one-sided and empty
columns; RowOneVsOneNuSVC and the three paths against sklearn; the refusals.

hits + misses counts every request: the rows of the start (each row of the union once) plus the restatement's (ip, in, j) >= 0."""
import ctypes as C
import functools
from contextlib import closing

import numpy as np
import pytest

import smo_nu_reference as nu
import smo_rows_reference as ref
from test_gpu_smo_rows import _points, amd  # noqa: F401 (the fixture: library loaded, long double checked)
from test_gpu_smo_rows_batched import Batch

pytestmark = pytest.mark.gpu

MR_SLICE = 2048   # RSMO_T * ML_PER of csrc/bq_mrsmo.hip


class NuBatch(Batch):   # the general entries; columns: (signs, lin, boxes, alpha0), with `lists` one ascending row list per column
    def __init__(self, X, kernel, columns, rule, lists=None, tol=1e-3, cache_rows=0, storage='stream', k=None):
        from optiml_amd import _lib
        from optiml_amd.opti import KernelQuadratic
        self._lib, self.lib, self.n, self.k, self.h = _lib, _lib.load(), len(X), len(columns) if k is None else k, C.c_void_p()
        self.rule, self.m = rule, [len(col[0]) for col in columns]
        join = np.stack if lists is None else np.concatenate
        vecs = [_lib.as_f64(np.ravel(join(part))) for part in zip(*columns)]
        self.quad = KernelQuadratic(X, np.zeros(self.n), 'plain', kernel, storage=storage)
        code = _lib.RSMO_RULE_NU if rule == 'nu' else _lib.RSMO_RULE_PLAIN
        dev, tail = self.quad.device_problem().handle, (float(tol), 0, int(cache_rows), C.byref(self.h))
        if lists is None:
            rc = self.lib.bq_mrsmo_create_general(dev, code, self.k, self.m[0], *(_lib.ptr(v) for v in vecs), *tail)
        else:
            offsets = np.ascontiguousarray(np.concatenate(([0], np.cumsum(self.m))), dtype=np.int64)
            rows = _lib.as_i32(np.concatenate(lists))
            rc = self.lib.bq_mrsmo_create_lists_general(dev, code, self.k, offsets.ctypes.data_as(C.POINTER(C.c_int64)), _lib.iptr(rows),
                                                        *(_lib.ptr(v) for v in vecs), *tail)
        if rc:
            self.quad.release()
        _lib.check(rc)

    def vectors(self, c):
        return self.get(self._lib.RSMO_ALPHAS, c, self.m[c]), self.get(self._lib.RSMO_GRADIENT, c, self.m[c])

    def scalars(self, c):
        if self.rule == 'nu':
            sc = dict(zip(('rho', 'r', 'gap_p', 'gap_n', 'i', 'j', 'steps'), self.get(self._lib.RSMO_NU_SCALARS, c, 7)))
            # BQ_RSMO_SCALARS of a NU solver: the same rho in slot 0 (NaN for a column whose every variable sits at one bound)
            np.testing.assert_array_equal(self.get(self._lib.RSMO_SCALARS, c, 6)[0], sc['rho'])
            return sc
        return super().scalars(c)


def _gauss(gamma):
    from optiml_amd.ml.svm import kernels as kk
    return kk.GaussianKernel(gamma)


def _terciles(X):
    return np.searchsorted(np.quantile(X[:, 0], [1 / 3, 2 / 3]), X[:, 0])


@functools.lru_cache(maxsize=None)
def _problem(name):
    """(X, kernel, columns, rule, lists or None, tol, cache_rows) of a seeded batch"""
    Xs, ys = ref.seeded('svc', 300, 5)
    if name == 'oc':
        return nu.one_class_data(300, 5), _gauss(0.5), [nu.one_class_problem(300, v)[:4] for v in (0.1, 0.2, 0.35)], 'plain', None, 1e-3, 0
    if name in ('nusvc', 'nusvc3k'):   # 3k: the start's union goes through six slots at a time, every group short of 16 rows
        return Xs, _gauss(0.5), [nu.nu_svc_problem(ys, v)[:4] for v in (0.2, 0.3)], 'nu', None, 1e-3, 6 if name == 'nusvc3k' else 0
    if name == 'nusvr':
        Xr, yr = ref.seeded('svr', 300, 5)
        return Xr, _gauss(0.5), [nu.nu_svr_problem(yr, 1.0, 0.5)[:4], nu.nu_svr_problem(np.cos(Xr[:, 1]), 2.0, 0.3)[:4]], 'nu', None, 1e-3, 0
    if name == 'lists':   # three class pairs by terciles of feature 0 and the list of all rows (the nusvc case's second column)
        codes, cols, lists = _terciles(Xs), [], []
        for i, j in ((0, 1), (0, 2), (1, 2)):
            lists.append(np.flatnonzero((codes == i) | (codes == j)))
            cols.append(nu.nu_svc_problem(np.where(codes[lists[-1]] == j, 1.0, -1.0), 0.3)[:4])
        return Xs, _gauss(0.5), cols + [nu.nu_svc_problem(ys, 0.3)[:4]], 'nu', lists + [np.arange(300)], 1e-3, 0
    if name == 'sided':   # all positive boxes filled (ip = -1 throughout); optimal before the first step; a live column
        y90, alt = np.where(np.arange(300) < 90, 1.0, -1.0), np.where(np.arange(300) % 2 == 0, 1.0, -1.0)
        return Xs, _gauss(0.5), [nu.nu_svc_problem(y90, 0.6)[:4], nu.nu_svc_problem(alt, 1.0)[:4], nu.nu_svc_problem(ys, 0.3)[:4]], 'nu', None, 1e-3, 0
    if name.startswith('full'):   # the slice edges of the full form: alternating labels, two nu, three slots per column
        n = int(name[4:])
        X, alt = np.random.default_rng(1000 * n + 5).standard_normal((n, 5)), np.where(np.arange(n) % 2 == 0, 1.0, -1.0)
        return X, _gauss(0.2), [nu.nu_svc_problem(alt, v)[:4] for v in (0.5, 0.25)], 'nu', None, 1e-3, 6
    X, _ = ref.seeded('svc', 4200, 8)   # 'edges': random ascending lists at the slice edges, labels from a linear rule
    rng, cols, lists = np.random.default_rng(5), [], []
    for m in (MR_SLICE - 1, MR_SLICE, MR_SLICE + 1, 2 * MR_SLICE + 1):
        lists.append(np.sort(rng.choice(4200, m, replace=False)))
        cols.append(nu.nu_svc_problem(np.where(X[lists[-1], 0] + 0.5 * X[lists[-1], 1] > 0, 1.0, -1.0), 0.2)[:4])
    return X, _gauss(0.2), cols, 'nu', lists, 1e-2, 0


def _open(name, only=None, **kw):
    X, kern, cols, rule, lists, tol, cache_rows = _problem(name)
    if only is not None:
        cols, lists = [cols[only]], None if lists is None else [lists[only]]
    return NuBatch(X, kern, cols, rule, lists, tol, **dict(dict(cache_rows=cache_rows), **kw))


@functools.lru_cache(maxsize=None)
def _reference(name, steps_only=None):
    """(K as the device makes it, per column (the restatement's run from the device's alpha0 and G0, its trace), the start's union)"""
    X, kern, cols, rule, lists, tol, _ = _problem(name)
    with closing(_open(name)) as s:
        starts = [s.vectors(c) for c in range(s.k)]
        K = s.rows(np.arange(len(X)))
    wants, union = [], set()
    for c, (signs, p, Cb, a0) in enumerate(cols):
        rows = np.arange(len(X)) if lists is None else lists[c]
        trace = []
        wants.append((nu.solve(rule, K[np.ix_(rows, rows)], signs, p, Cb, tol, *starts[c], steps_only=steps_only,
                               trace=trace if len(X) <= 300 else None), trace))
        assert steps_only is not None or wants[-1][0].status == 'optimal'
        b = (signs * a0).reshape(-1, len(rows))
        union |= set(rows[np.flatnonzero(b[0] + b[1] if len(b) == 2 else b[0])])
    return K, wants, len(union)


def _requests(want, rule):
    """the non-negative requests of the restatement's run"""
    if rule == 'nu':
        return sum((ip >= 0) + (i_n >= 0) + 1 for ip, i_n in want.sides)
    return 2 * want.steps


# ---- 1. the start ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['oc', 'nusvc', 'nusvr', 'lists', 'nusvc3k'])
def test_start_alpha_and_gradient(amd, name):
    X, kern, cols, rule, lists, tol, _ = _problem(name)
    K, firsts, union = _reference(name, steps_only=1)
    with closing(_open(name)) as s:
        st = s.stats()
        for c, (signs, lin, Cb, a0) in enumerate(cols):
            rows = np.arange(len(X)) if lists is None else lists[c]
            Ks, rep = K[np.ix_(rows, rows)], len(signs) // len(rows)
            alpha, G0 = s.vectors(c)
            assert alpha.tobytes() == a0.tobytes()
            b = (signs * a0).reshape(rep, -1)
            b = b[0] + b[1] if rep == 2 else b[0]
            if not b.any():
                assert name == 'nusvr' and G0.tobytes() == lin.tobytes()
                continue
            acc = np.zeros(len(rows))
            for r in np.flatnonzero(b):   # ascending; one rounded product and one rounded add per row
                acc = acc + Ks[:, r] * b[r]
            assert G0.tobytes() == (lin + signs * np.tile(acc, rep)).tobytes(), f'column {c}'
    # the start asked for each row of the union once (nu-SVR: for none), the first selection for its violators' rows
    first = sum(_requests(w, rule) - (rule == 'nu') * w.steps for w, _ in firsts) // (1 if rule == 'nu' else 2)
    assert st['hits'] + st['misses'] == union + first and (union == 0) == (name == 'nusvr')


# ---- 2. step for step ------------------------------------------------------------------------------------------------------------------
def _same_step(s, c, want, trace, k):
    sc = s.scalars(c)
    assert (sc['steps'], sc['i'], sc['j']) == (k + 1,) + want.pairs[k], f'column {c} step {k}'
    alpha, G = s.vectors(c)
    assert (alpha.tobytes(), G.tobytes()) == (trace[k][0].tobytes(), trace[k][1].tobytes()), f'alpha, G of column {c} after step {k}'


def _same_end(s, c, want, steps, fin):
    assert (steps, fin) == (want.steps, 1), f'column {c}'
    alpha, G = s.vectors(c)
    assert (alpha.tobytes(), G.tobytes()) == (want.alpha.tobytes(), want.G.tobytes()), f'column {c}'
    sc = s.scalars(c)
    names = ('rho', 'steps', 'r', 'gap_p', 'gap_n') if s.rule == 'nu' else ('rho', 'steps', 'gmax', 'gmax2')
    np.testing.assert_array_equal([sc[f] for f in names], [getattr(want, f) for f in names])   # (an empty column's rho is NaN twice)
    assert want.steps == 0 or (sc['i'], sc['j']) == want.pairs[-1]


@pytest.mark.parametrize('name', ['oc', 'nusvc', 'nusvr', 'lists', 'nusvc3k'])
def test_single_steps_follow_the_reference(amd, name):
    K, wants, union = _reference(name)
    assert max(w.steps for w, _ in wants) > 200
    with closing(_open(name)) as s:
        for k in range(200):
            steps, fin = s.run(1)
            for c, (want, trace) in enumerate(wants):
                if k >= want.steps:
                    assert (steps[c], fin[c]) == (want.steps, 1)
                else:
                    _same_step(s, c, want, trace, k)
        steps, fin = s.finish()
        for c, (want, _) in enumerate(wants):
            _same_end(s, c, want, steps[c], fin[c])
        st = s.stats()
        assert st['hits'] + st['misses'] == union + sum(_requests(w, s.rule) for w, _ in wants)
        if name == 'lists':   # the list of all rows is the same column in the full form
            with closing(_open('nusvc', only=1)) as full:
                _same_end(full, 0, wants[3][0], *(v[0] for v in full.finish()))


# ---- 3. the edges ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [255, 256, 257])
def test_full_columns_at_the_slice_edges(amd, n):
    K, wants, _ = _reference(f'full{n}', steps_only=30)
    with closing(_open(f'full{n}')) as s:
        for k in range(30):
            s.run(1)
            for c, (want, trace) in enumerate(wants):
                _same_step(s, c, want, trace, k)


def test_list_columns_at_the_slice_edges(amd):
    K, wants, union = _reference('edges')
    with closing(_open('edges')) as s:
        steps, fin = s.finish(256)
        for c, (want, _) in enumerate(wants):
            _same_end(s, c, want, steps[c], fin[c])
        st = s.stats()
        assert st['hits'] + st['misses'] == union + sum(_requests(w, 'nu') for w, _ in wants) and st['misses'] <= len(K)
    with closing(_open('edges', only=2, cache_rows=3)) as s:   # alone, three slots, cut into 7-step calls
        steps, fin = s.finish(7)
        _same_end(s, 0, wants[2][0], steps[0], fin[0])


# ---- 4. one-sided and empty columns ----------------------------------------------------------------------------------------------------
def test_one_sided_and_empty_columns_beside_a_live_one(amd):
    K, wants, _ = _reference('sided')
    sided, empty, live = (w for w, _ in wants)
    assert sided.steps > 100 and all(ip == -1 for ip, _ in sided.sides) and _problem('sided')[2][0][3][:90].sum() == 90.0
    assert empty.steps == 0 and live.steps > 100
    with closing(_open('sided')) as s:
        steps, fin = s.finish()
        for c, (want, _) in enumerate(wants):
            _same_end(s, c, want, steps[c], fin[c])
    with closing(_open('sided', only=2)) as s:   # the live column alone
        _same_end(s, 0, live, *(v[0] for v in s.finish()))


# ---- 5. models -------------------------------------------------------------------------------------------------------------------------
def test_one_vs_one_against_sklearn(amd):
    from sklearn.multiclass import OneVsOneClassifier
    from sklearn.svm import NuSVC as Sk
    from optiml_amd.ml.svm import RowOneVsOneNuSVC
    X, _ = ref.seeded('svc', 300, 5)
    y, P = _terciles(X), np.vstack((X, _points(5)))
    ours = RowOneVsOneNuSVC(kernel=_gauss(0.5), nu=0.3, tol=1e-6).fit(X, y)
    theirs = OneVsOneClassifier(Sk(kernel='rbf', gamma=0.5, nu=0.3, tol=1e-6, shrinking=False)).fit(X, y)
    assert ours.batched_ and len(ours.estimators_) == 3 and list(ours.classes_) == [0, 1, 2]
    sure = np.ones(len(P), dtype=bool)
    for a, b in zip(ours.estimators_, theirs.estimators_):
        da, db = a.decision_function(P), b.decision_function(P)
        err = float(np.abs(a.margin_scale_ * (da - db)).max())   # r x decision: the unscaled dual's, which tol bounds
        print(f'pair: {a.n_iter_} steps (sklearn {b.n_iter_}), max difference of r x decision {err:.3e}')
        assert a.status_ == 'optimal' and err <= 1e-5
        sure &= np.abs(db) > 1e-4
    assert (ours.predict(P)[sure] == theirs.predict(P)[sure]).all()


def _paths():
    from sklearn import svm
    from optiml_amd.ml.svm import (RowNuSVC, RowNuSVR, RowOneClassSVM, row_nu_svc_path, row_nu_svr_path, row_one_class_nu_path)
    Xs, ys = ref.seeded('svc', 300, 5)
    Xr, yr = ref.seeded('svr', 300, 5)
    kw, sk = dict(kernel=_gauss(0.5), tol=1e-6), dict(kernel='rbf', gamma=0.5, tol=1e-6, shrinking=False)
    return {'svc': (lambda ps: row_nu_svc_path(RowNuSVC(**kw), Xs, ys, [p['nu'] for p in ps]), [dict(nu=0.2), dict(nu=0.3)],
                    lambda p: svm.NuSVC(**sk, **p).fit(Xs, ys), Xs),
            'svr': (lambda ps: row_nu_svr_path(RowNuSVR(**kw), Xr, yr, ps), [dict(nu=0.5, C=1.0), dict(nu=0.3, C=2.0)],
                    lambda p: svm.NuSVR(**sk, **p).fit(Xr, yr), Xr),
            'oc': (lambda ps: row_one_class_nu_path(RowOneClassSVM(**kw), nu.one_class_data(300, 5), [p['nu'] for p in ps]),
                   [dict(nu=0.1), dict(nu=0.2)], lambda p: svm.OneClassSVM(**sk, **p).fit(nu.one_class_data(300, 5)), nu.one_class_data(300, 5))}


@pytest.mark.parametrize('kind', ['svc', 'svr', 'oc'])
def test_paths_against_sklearn_and_their_columns_alone(amd, kind):
    path, params, theirs, X = _paths()[kind]
    P = np.vstack((X, _points(5)))
    for p, est in zip(params, path(params)):
        alone, sk = path([p])[0], theirs(p)
        assert est.status_ == 'optimal' and est.get_params()['nu'] == p['nu']
        assert (est.alphas_.tobytes(), est.n_iter_) == (alone.alphas_.tobytes(), alone.n_iter_)
        scale = est.margin_scale_ if kind == 'svc' else 1.0
        da, db = est.decision_function(P), np.ravel(sk.decision_function(P) if kind != 'svr' else sk.predict(P))
        err = float(np.abs(scale * (da - db)).max())
        print(f'{kind} {p}: {est.n_iter_} steps (sklearn {sk.n_iter_}), max difference {err:.3e}')
        assert err <= 1e-5
        if kind != 'svr':
            sure = np.abs(db) > 1e-4
            assert (est.predict(P)[sure] == sk.predict(P)[sure]).all()


# ---- 6. scope --------------------------------------------------------------------------------------------------------------------------
def test_create_refuses_what_it_does_not_solve(amd):
    from optiml_amd import _lib
    X, y = ref.seeded('svc', 64, 3)
    col = nu.nu_svc_problem(y, 0.3)[:4]
    above = col[3].copy()
    above[int(np.argmax(above))] = 1.5
    for cols, kw in (([col], dict(storage='f64')), ([col, col], dict(cache_rows=5)), ([col], dict(k=513)),
                     ([col[:3] + (above,)], {}), ([(np.ones(64),) + col[1:]], {})):
        with pytest.raises(_lib.BcqpError) as err:
            NuBatch(X, _gauss(0.5), cols, 'nu', **kw)
        assert err.value.code == _lib.ERR_BADARG, kw
    with closing(NuBatch(X, _gauss(0.5), [col, col], 'nu', cache_rows=6)) as s:   # the same columns, accepted
        assert s.finish()[1] == [1, 1]


def test_infeasible_pair_and_stream_refusals(amd, monkeypatch):
    from optiml_amd.ml.svm import OneVsOneNuSVC, RowOneVsOneNuSVC, nu_rows
    X, _ = ref.seeded('svc', 64, 3)
    y = np.repeat([0, 1, 2], (30, 30, 4))

    def no_device(*a, **k):
        raise AssertionError('device work before the feasibility check')
    monkeypatch.setattr(nu_rows, 'KernelQuadratic', no_device)
    with pytest.raises(ValueError, match='infeasible'):
        RowOneVsOneNuSVC(kernel=_gauss(0.5), nu=0.5).fit(X, y)
    with pytest.raises(NotImplementedError):
        OneVsOneNuSVC(kernel=_gauss(0.5), nu=0.1, storage='stream').fit(X, y)
