"""The batched decision function on the device: `bq_decision_function_multi` (bq_decide.hip: the kernel values of every (test tile,
SV tile) pair formed once and contracted with all k coefficient columns on the fp64 matrix cores) against the oracle's Gram matrix
and the single-column path, its invariances (call, batch, unit split, test chunk: equal bits), and the meta-estimators that predict
through it.

Shapes: m = 300 support vectors (three 128-row tiles, ragged last), t = 165 test points (two tiles, ragged last), d = 12 (one
16-deep k-chunk, padded) and d = 20 (two chunks: the peeled tail of the tile product), k in {1, 5, 16, 17, 35} (a partial group of
16 columns, a full one, one column into the second group, a partial third group)."""
import functools

import numpy as np
import pytest

from conftest import set_hooks

pytestmark = pytest.mark.gpu

M, T, KMAX = 300, 165, 35
KS = (1, 5, 16, 17, 35)
CASES = {   # oracle name, gamma, coef0, degree
    'rbf': ('rbf', 0.3, 0.0, 1),
    'poly3': ('poly', 0.1, 1.0, 3),
    'poly2': ('poly', 0.1, 1.0, 2),
    'sigmoid': ('sigmoid', 0.1, 0.5, 1),
    'linear': ('linear', 0.0, 0.0, 1),
}
PARAMS = [(name, d) for name in CASES for d in (12, 20)]


@pytest.fixture(scope='module')
def amd():
    from optiml_amd import _lib
    from optiml_amd.device import get_context
    _lib.load()
    get_context()


def _kind(name):
    from optiml_amd import _lib
    return {'rbf': _lib.KERNEL_RBF, 'poly': _lib.KERNEL_POLY, 'sigmoid': _lib.KERNEL_SIGMOID, 'linear': _lib.KERNEL_LINEAR}[name]


@functools.lru_cache(maxsize=None)
def _inputs(d):
    """SV, Xt (standard normal scaled by 0.5), W, b (standard normal) from a fixed seed; shared by the tests, which leave them
    unchanged."""
    rs = np.random.RandomState(100 + d)
    SV, Xt = 0.5 * rs.standard_normal((M, d)), 0.5 * rs.standard_normal((T, d))
    W, b = rs.standard_normal((KMAX, M)), rs.standard_normal(KMAX)
    for a in (SV, Xt, W, b):
        a.setflags(write=False)
    return SV, Xt, W, b


@functools.lru_cache(maxsize=None)
def _gram(case, d):
    """the oracle's kernel(Xt, SV), t x m, computed once per case"""
    from oracle import svm_oracle as so
    name, gamma, coef0, degree = CASES[case]
    SV, Xt, _, _ = _inputs(d)
    K = so.gram(name, Xt, SV, gamma=gamma, coef0=coef0, degree=degree)
    K.setflags(write=False)
    return K


def _multi(case, SV, W, b, Xt):
    """k x t"""
    from optiml_amd import _lib
    from optiml_amd.device import get_context
    name, gamma, coef0, degree = CASES[case]
    SV, W, Xt = (np.ascontiguousarray(a, dtype=float) for a in (SV, W, Xt))
    b = None if b is None else np.ascontiguousarray(b, dtype=float)
    (k, m), (t, d) = W.shape, Xt.shape
    out = np.full((k, t), np.nan)
    _lib.check(_lib.load().bq_decision_function_multi(get_context().handle, _kind(name), gamma, coef0, degree, m, d, _lib.ptr(SV),
                                                      k, _lib.ptr(W), None if b is None else _lib.ptr(b), t, _lib.ptr(Xt),
                                                      _lib.ptr(out)))
    return out


def _single(case, SV, w, b, Xt):
    from optiml_amd import _lib
    from optiml_amd.device import get_context
    name, gamma, coef0, degree = CASES[case]
    w = np.ascontiguousarray(w, dtype=float)
    out = np.full(Xt.shape[0], np.nan)
    _lib.check(_lib.load().bq_decision_function(get_context().handle, _kind(name), gamma, coef0, degree, SV.shape[0], SV.shape[1],
                                                _lib.ptr(SV), _lib.ptr(w), float(b), Xt.shape[0], _lib.ptr(Xt), _lib.ptr(out)))
    return out


def _tol(K):
    """The tolerance test_decision_function_is_chunked_over_test_points holds the single-column path to (same coefficient scale)."""
    return dict(rtol=1e-11, atol=1e-11 * np.abs(K).sum(axis=1).max())


@pytest.mark.parametrize('case,d', PARAMS)
def test_against_the_oracle_and_the_single_column_path(amd, monkeypatch, case, d):
    set_hooks(monkeypatch, decision_multi_unit=None, decision_multi_chunk_rows=None)
    SV, Xt, W, b = _inputs(d)
    K = _gram(case, d)
    ref = (K @ W.T + b).T   # k x t
    singles = np.stack([_single(case, SV, W[c], b[c], Xt) for c in range(KMAX)])
    np.testing.assert_allclose(singles, ref, **_tol(K))
    for k in KS:
        out = _multi(case, SV, W[:k], b[:k], Xt)
        print('%s d=%d k=%d: max |multi - oracle| %.3e, max |multi - single| %.3e, atol %.3e'
              % (case, d, k, np.abs(out - ref[:k]).max(), np.abs(out - singles[:k]).max(), _tol(K)['atol']))
        np.testing.assert_allclose(out, ref[:k], **_tol(K))
        np.testing.assert_allclose(out, singles[:k], **_tol(K))
    # no intercepts
    np.testing.assert_allclose(_multi(case, SV, W[:5], None, Xt), ref[:5] - b[:5, None], **_tol(K))
    # units of two and of three SV tiles (the walk in the registers) associate the tiles' sums differently: the oracle's tolerance
    for unit in (2, 3):
        set_hooks(monkeypatch, decision_multi_unit=unit)
        np.testing.assert_allclose(_multi(case, SV, W, b, Xt), ref, **_tol(K))


@pytest.mark.parametrize('case,d', PARAMS)
def test_invariance(amd, monkeypatch, case, d):
    """Equal bits: call and call again; a column alone, in the full batch of 35 and in the reversed batch (another group, another
    slot, the other instantiation of the kernel); one SV tile per unit against the default split; 128-row chunks of test points
    against one chunk."""
    set_hooks(monkeypatch, decision_multi_unit=None, decision_multi_chunk_rows=None)
    SV, Xt, W, b = _inputs(d)
    full = _multi(case, SV, W, b, Xt)
    assert np.isfinite(full).all()
    np.testing.assert_array_equal(_multi(case, SV, W, b, Xt), full)
    np.testing.assert_array_equal(_multi(case, SV, W[::-1], b[::-1], Xt)[::-1], full)
    for c in range(KMAX):
        np.testing.assert_array_equal(_multi(case, SV, W[c:c + 1], b[c:c + 1], Xt)[0], full[c], err_msg='column %d alone' % c)
    np.testing.assert_array_equal(_multi(case, SV, W[:17], b[:17], Xt), full[:17])
    # at this shape (2 test tiles, 3 SV tiles) the default split already is one SV tile per unit; units of 2 and 3 tiles, which
    # associate the tiles' sums differently, are held to the oracle in test_against_the_oracle_and_the_single_column_path
    set_hooks(monkeypatch, decision_multi_unit=1)
    np.testing.assert_array_equal(_multi(case, SV, W, b, Xt), full)
    np.testing.assert_array_equal(_multi(case, SV, W[:5], b[:5], Xt), full[:5])
    set_hooks(monkeypatch, decision_multi_unit=None, decision_multi_chunk_rows=128)
    np.testing.assert_array_equal(_multi(case, SV, W, b, Xt), full)
    np.testing.assert_array_equal(_multi(case, SV, W[:5], b[:5], Xt), full[:5])


@pytest.mark.parametrize('case,d', PARAMS)
def test_rows_with_zero_coefficients(amd, monkeypatch, case, d):
    """40 % of the support vectors have a zero coefficient in every column.  Their kernel values meet a zero in sums of a fixed
    order, so the result has the same bits whatever those rows hold (here: the rows themselves, then zeros); and it agrees with
    the call on the compacted SV / W — the union the estimators pass — at the oracle's tolerance."""
    set_hooks(monkeypatch, decision_multi_unit=None, decision_multi_chunk_rows=None)
    SV, Xt, W, b = _inputs(d)
    dead = np.random.RandomState(9).permutation(M)[:int(0.4 * M)]
    Wz = W.copy()
    Wz[:, dead] = 0.0
    out = _multi(case, SV, Wz, b, Xt)
    np.testing.assert_array_equal(_multi(case, SV, Wz, b, Xt), out)
    SVz = SV.copy()
    SVz[dead] = 0.0
    np.testing.assert_array_equal(_multi(case, SVz, Wz, b, Xt), out)
    live = np.setdiff1d(np.arange(M), dead)
    K = _gram(case, d)
    np.testing.assert_allclose(out, (K @ Wz.T + b).T, **_tol(K))
    np.testing.assert_allclose(_multi(case, SV[live], Wz[:, live], b, Xt), out, **_tol(K))


def test_exact_on_small_integers(amd, monkeypatch):
    """Linear kernel on small-integer data and coefficients: every product and sum is exact, so any wrong lane map of the second
    MFMA's A, B or C/D fragments, any wrong row-block permutation of the coefficient fragment or any wrong tile shows as unequal
    bits.  W is asymmetric by construction."""
    set_hooks(monkeypatch, decision_multi_unit=None, decision_multi_chunk_rows=None)
    rs = np.random.RandomState(11)
    m, t, d, k = 300, 165, 5, 35
    SV, Xt = rs.randint(-3, 4, size=(m, d)).astype(float), rs.randint(-3, 4, size=(t, d)).astype(float)
    W, b = rs.randint(-4, 5, size=(k, m)).astype(float), rs.randint(-4, 5, size=k).astype(float)
    want = W @ (SV @ Xt.T) + b[:, None]
    for kk in KS:
        np.testing.assert_array_equal(_multi('linear', SV, W[:kk], b[:kk], Xt), want[:kk])
    set_hooks(monkeypatch, decision_multi_unit=3)
    np.testing.assert_array_equal(_multi('linear', SV, W, b, Xt), want)


@functools.lru_cache(maxsize=None)
def _blobs5():
    from optiml_amd.datasets import make_multiclass_blobs
    X, y = make_multiclass_blobs(400, 8, 5, seed=1)
    return X[:300], X[300:], y[:300]


def _svc_kw(**more):
    from optiml_amd.ml.svm.kernels import GaussianKernel
    from optiml_amd.ml.svm.losses import hinge
    from optiml_amd.opti.constrained import ProjectedGradient
    kw = dict(loss=hinge, kernel=GaussianKernel(gamma=0.7), C=1.0, reg_intercept=True, dual=True, max_iter=20,
              optimizer=ProjectedGradient)
    kw.update(more)
    return kw


def _ovo_loop(est, X):
    from optiml_amd.ml.svm.onevsone import ovo_decision
    conf = np.stack([np.ravel(e.decision_function(X)) for e in est.estimators_], axis=1)
    Y = ovo_decision((conf > 0).astype(int), conf, len(est.classes_))
    return Y[:, 1] if len(est.classes_) == 2 else Y


def _ovr_loop(est, X):
    scores = np.stack([e.decision_function(X) for e in est.estimators_], axis=1)
    return scores[:, 0] if len(est.classes_) == 2 else scores


def _labels(est, scores):
    if len(est.classes_) == 2:
        return est.classes_[(scores > 0).astype(int)]
    return est.classes_[np.argmax(scores, axis=1)]


@pytest.mark.parametrize('which', ['ovo', 'ovr'])
def test_classifiers_equal_the_loop_over_their_estimators(amd, which):
    from optiml_amd.ml.svm import OneVsOneSVC, OneVsRestSVC
    Xtr, Xte, ytr = _blobs5()
    est = (OneVsOneSVC if which == 'ovo' else OneVsRestSVC)(**_svc_kw()).fit(Xtr, ytr)
    assert est.batched_ and est.batched_decision_ is True
    loop = (_ovo_loop if which == 'ovo' else _ovr_loop)(est, Xte)
    ours = est.decision_function(Xte)
    assert ours.shape == loop.shape == (100, 5)
    np.testing.assert_allclose(ours, loop, rtol=1e-9, atol=1e-9)
    np.testing.assert_array_equal(est.predict(Xte), _labels(est, loop))
    np.testing.assert_array_equal(est.decision_function(Xte), ours)
    if which == 'ovo':
        # the union is shared: a training row is a support vector of up to 4 pairs and a row of SV once
        batch = est.decision_batch_
        assert batch.W.shape == (10, batch.SV.shape[0]) and len(batch.b) == 10
        assert batch.SV.shape[0] <= len(Xtr)
        assert batch.SV.shape[0] < sum(len(e.support_) for e in est.estimators_)
        assert len({tuple(r) for r in batch.SV}) == batch.SV.shape[0]   # no ghost rows (all zero), no row twice


def test_regressor_equals_the_loop_over_its_estimators(amd):
    from optiml_amd.datasets import make_regression
    from optiml_amd.ml.svm import MultiOutputSVR
    from optiml_amd.ml.svm.kernels import GaussianKernel
    from optiml_amd.ml.svm.losses import epsilon_insensitive
    from optiml_amd.opti.constrained import ProjectedGradient
    X, _ = make_regression(400, 8, seed=1)
    rs = np.random.RandomState(7)
    Y = np.tanh(X @ rs.standard_normal((8, 3)) / np.sqrt(8) / 4) + 0.1 * rs.standard_normal((400, 3))
    est = MultiOutputSVR(loss=epsilon_insensitive, epsilon=0.1, kernel=GaussianKernel(gamma=0.2), C=1.0, reg_intercept=True, dual=True,
                         max_iter=100, optimizer=ProjectedGradient).fit(X[:300], Y[:300])
    assert est.batched_ is True and est.batched_decision_ is True
    loop = np.stack([e.predict(X[300:]) for e in est.estimators_], axis=1)
    ours = est.predict(X[300:])
    assert ours.shape == (100, 3)
    np.testing.assert_allclose(ours, loop, rtol=1e-9, atol=1e-9)


def test_grid_search_inherits_the_path(amd):
    pytest.importorskip('sklearn')
    from sklearn.model_selection import StratifiedKFold
    from optiml_amd.ml.svm import OneVsRestSVC, SVCGridSearchCV
    Xtr, Xte, ytr = _blobs5()
    search = SVCGridSearchCV(OneVsRestSVC(**_svc_kw()), {'C': [0.3, 1.0]}, cv=StratifiedKFold(3)).fit(Xtr, ytr)
    best = search.best_estimator_
    assert best.batched_decision_ is True
    np.testing.assert_array_equal(search.decision_function(Xte), best.decision_function(Xte))
    np.testing.assert_array_equal(search.predict(Xte), best.predict(Xte))
    np.testing.assert_allclose(search.decision_function(Xte), _ovr_loop(best, Xte), rtol=1e-9, atol=1e-9)


@pytest.mark.parametrize('which', ['scale', 'two-classes', 'active-set'])
def test_the_rule_in_action(amd, which):
    """gamma='scale' (the default kernel), a single column and a fallback optimizer keep the loop over the estimators: equal bits,
    because it is the loop."""
    from optiml_amd.ml.svm import OneVsOneSVC, OneVsRestSVC
    from optiml_amd.ml.svm.kernels import GaussianKernel
    from optiml_amd.opti.constrained import ActiveSet
    Xtr, Xte, ytr = _blobs5()
    kw = _svc_kw()
    if which == 'scale':
        kw = _svc_kw(kernel=GaussianKernel('scale'))
    elif which == 'two-classes':
        keep = ytr < 2
        Xtr, ytr = Xtr[keep], ytr[keep]
    else:
        kw = _svc_kw(optimizer=ActiveSet)
    for cls, loop in ((OneVsOneSVC, _ovo_loop), (OneVsRestSVC, _ovr_loop)):
        est = cls(**kw).fit(Xtr, ytr)
        assert est.batched_decision_ is False and est.decision_batch_ is None
        assert est.batched_ is (which == 'two-classes' or (which == 'scale' and cls is OneVsRestSVC))
        np.testing.assert_array_equal(est.decision_function(Xte), loop(est, Xte))
        np.testing.assert_array_equal(est.predict(Xte), _labels(est, loop(est, Xte)))
