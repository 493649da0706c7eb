"""The decision kernels at the shapes the first suite (test_gpu_decision_batch.py: m = 300, t = 165, d in {12, 20}, k <= 35, degrees 2
and 3) never reaches: more than 64 columns (further passes in blockIdx.z), exactly four full groups (k = 64, the meeting buffer
fills the tile LDS), the `pow` instantiation (DEG = 0), the default unit split with more than one SV tile per unit, 1 ... 6
k-chunks of the tile product under the live output accumulators, degenerate and exact-edge shapes, RBF values that are exactly 1
and exactly 0, the single-column path for the sigmoid and the Laplacian kernel, and an estimator with 66 columns.

Reference and bound.  SV and test points lie on a dyadic grid (multiples of 2^-6, |x| <= 2), gamma and coef0 are powers of two or
short dyadics: every dot product, squared norm, distance and kernel argument is then exact in fp64 — asserted on the CPU against
np.longdouble (`_same`) — so the device and the reference differ in the kernel map and the contraction only.  Kernel values are
NumPy's `exp`, `tanh` and `**` on those arguments; the contraction and the intercept are in np.longdouble (>= 63 mantissa bits).
Per output entry, with u = 2^-53:

    |out - ref| <= (m + 8) u sum_j |W[c][j]| |K[j][i]| + u |ref|

m u sum |terms| bounds an m-term sum in any fixed order; 8 u covers the map (bq_exp <= 2 ulp, the degree 2 / 3 maps <= 1 ulp from
pow, both pinned elsewhere in the suite) and the reference's own rounding of it.  No entry is left out of any comparison, and no
reference kernel value underflows except in `test_rbf_underflow`, which asserts that they do.  Integer cases (linear kernel, small
integers everywhere) are compared for equal bits with the integer product.

Every comparison prints max |out - ref| / bound.  Observed on an MI355X (gfx950), largest over the cases of each kernel, with the
8 as it stands (no case came near 1, so no map was measured on its own and no figure replaced the 8):
    rbf        0.89  (m = 1, t = 165, k = 17: one term, the bound is 9 u; at m >= 100 at most 0.016, at m = 65 700 below 1e-4)
    poly       0.014 (degree 5, d = 20; degree 4: 0.008; degree 3 at k = 129: 0.013 with three SV tiles per unit)
    sigmoid    0.65  (single-column path, m = 1; 0.002 at m = 300)
    laplacian  0.65  (single-column path, m = 1; 0.002 at m = 300)
    OneVsOneSVC with 66 pairs against the loop over its estimators: largest relative deviation 4.4e-16.

One case differs from the shapes the plan of these tests named: at m = 65 700 the default split is two SV tiles per unit for
t <= 128 (514 SV tiles, 512 workgroups wanted), but with two test tiles (t = 129) `decide_unit_tiles` wants 256 units and gives
ceil(514 / 256) = 3 tiles per unit, not 2.  `test_default_unit_split` therefore holds the t = 129 default run to the bits of the
`decision_multi_unit=3` run, and the `decision_multi_unit=2` run at t = 129 to the bits of the t = 100 run on the rows they share."""
import functools

import numpy as np
import pytest

from conftest import set_hooks

pytestmark = pytest.mark.gpu

LD = np.longdouble
U = LD(2.0) ** -53
MAP_U = {'rbf': 8, 'poly': 8, 'sigmoid': 8, 'laplacian': 8, 'linear': 8}   # the map's share of the bound, in units of u
M, T = 300, 165


@pytest.fixture(scope='module')
def amd():
    from optiml_amd import _lib
    from optiml_amd.device import get_context
    assert np.finfo(LD).nmant >= 63
    _lib.load()
    get_context()


def _no_hooks(monkeypatch, **kw):
    hooks = dict(decision_multi_unit=None, decision_multi_chunk_rows=None, decision_chunk_rows=None)
    hooks.update(kw)
    set_hooks(monkeypatch, **hooks)


def _kind(name):
    from optiml_amd import _lib
    return {'rbf': _lib.KERNEL_RBF, 'poly': _lib.KERNEL_POLY, 'sigmoid': _lib.KERNEL_SIGMOID, 'linear': _lib.KERNEL_LINEAR,
            'laplacian': _lib.KERNEL_LAPLACIAN}[name]


LINEAR = ('linear', 0.0, 0.0, 1)


def _rbf(d, xmax=2.0):
    """gamma: the largest power of two with gamma * (largest squared distance on the grid) <= 12, so exp >= e^-12"""
    return ('rbf', 2.0 ** np.floor(np.log2(12.0 / (4.0 * xmax * xmax * d))), 0.0, 1)


def _multi(spec, SV, W, b, Xt):
    """k x t"""
    from optiml_amd import _lib
    from optiml_amd.device import get_context
    name, gamma, coef0, degree = spec
    SV, W, Xt = (np.ascontiguousarray(a, dtype=float) for a in (SV, W, Xt))
    b = None if b is None else np.ascontiguousarray(b, dtype=float)
    (k, m), (t, d) = W.shape, Xt.shape
    assert SV.shape == (m, d) and (b is None or b.shape == (k,))
    out = np.full((k, t), np.nan)
    _lib.check(_lib.load().bq_decision_function_multi(get_context().handle, _kind(name), gamma, coef0, degree, m, d, _lib.ptr(SV),
                                                      k, _lib.ptr(W), None if b is None else _lib.ptr(b), t, _lib.ptr(Xt),
                                                      _lib.ptr(out)))
    return out


def _single(spec, SV, w, b, Xt):
    """t"""
    from optiml_amd import _lib
    from optiml_amd.device import get_context
    name, gamma, coef0, degree = spec
    SV, w, Xt = (np.ascontiguousarray(a, dtype=float) for a in (SV, w, Xt))
    (m, d), t = SV.shape, Xt.shape[0]
    assert w.shape == (m,) and Xt.shape[1] == d
    out = np.full(t, np.nan)
    _lib.check(_lib.load().bq_decision_function(get_context().handle, _kind(name), gamma, coef0, degree, m, d, _lib.ptr(SV),
                                                _lib.ptr(w), float(b), t, _lib.ptr(Xt), _lib.ptr(out)))
    return out


# ---- inputs and the reference ----------------------------------------------------------------------------------------------------
def _grid(rs, shape, xmax=2.0):
    """multiples of 2^-6 in [-xmax, xmax]"""
    n = int(round(xmax * 64))
    return rs.randint(-n, n + 1, size=shape) / 64.0


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def _real(seed, m, t, d, k, xmax=2.0):
    """SV, Xt on the grid, W, b standard normal; shared by the tests, which leave them unchanged"""
    rs = np.random.RandomState(seed)
    return _frozen(_grid(rs, (m, d), xmax), _grid(rs, (t, d), xmax), rs.standard_normal((k, m)), rs.standard_normal(k))


@functools.lru_cache(maxsize=None)
def _ints(seed, m, t, d, k, hi=3, whi=4):
    """SV, Xt in {-hi .. hi}, W in {-whi .. whi}, b in {-4 .. 4} and the integer product W (SV Xt') + b: every product and every
    partial sum is an integer far below 2^53, so fp64 in any order is exact"""
    rs = np.random.RandomState(seed)
    SV, Xt = rs.randint(-hi, hi + 1, size=(m, d)).astype(float), rs.randint(-hi, hi + 1, size=(t, d)).astype(float)
    W, b = rs.randint(-whi, whi + 1, size=(k, m)).astype(float), rs.randint(-4, 5, size=k).astype(float)
    want = W @ (SV @ Xt.T) + b[:, None]
    assert np.abs(W).sum(axis=1).max() * hi * hi * d + 4 < 2.0 ** 50
    return _frozen(SV, Xt, W, b, want)


def _same(a64, ald):
    """the fp64 value is the long-double value: the argument is exact"""
    assert a64.dtype == np.float64 and ald.dtype == LD and a64.shape == ald.shape
    assert np.array_equal(a64.astype(LD), ald)


def _kernel_values(spec, SV, Xt, zeros=False):
    """kernel(SV, Xt), m x t in fp64: NumPy's map on arguments that are asserted exact.  zeros: whether exponentials that
    underflow to 0 are expected (asserted either way; without them every value is a normal number)."""
    name, gamma, coef0, degree = spec
    A, B = SV.astype(LD), Xt.astype(LD)
    if name == 'laplacian':
        arg = -gamma * np.abs(SV[:, None, :] - Xt[None, :, :]).sum(axis=2)
        _same(arg, -LD(gamma) * np.abs(A[:, None, :] - B[None, :, :]).sum(axis=2))
        K = np.exp(arg)
    else:
        dot, dotl = SV @ Xt.T, A @ B.T
        _same(dot, dotl)
        if name == 'linear':
            return dot
        if name == 'rbf':
            arg = -gamma * ((SV * SV).sum(axis=1)[:, None] + (Xt * Xt).sum(axis=1)[None, :] - 2.0 * dot)
            _same(arg, -LD(gamma) * ((A * A).sum(axis=1)[:, None] + (B * B).sum(axis=1)[None, :] - 2 * dotl))
            assert (arg <= 0).all()
            K = np.exp(arg)
        else:
            arg = gamma * dot + coef0
            _same(arg, LD(gamma) * dotl + LD(coef0))
            return arg ** degree if name == 'poly' else np.tanh(arg)
    assert bool((K == 0).any()) is zeros
    assert zeros or K.min() >= np.finfo(float).tiny
    return K


def _reference(K, W, b):
    """(ref, S): W K + b and |W| |K| in long double, k x t (a column at a time on the transpose: NumPy's long-double matrix
    product is several times slower at m = 65 700)"""
    Kt, Wl = np.ascontiguousarray(K.T.astype(LD)), W.astype(LD)
    ref = np.stack([Kt @ w for w in Wl])
    if b is not None:
        ref = ref + b.astype(LD)[:, None]
    Kt = np.abs(Kt)
    return ref, np.stack([Kt @ w for w in np.abs(Wl)])


def _within(label, name, out, ref, S, m):
    """assert the bound on every entry and print the largest |out - ref| / bound"""
    assert out.shape == ref.shape == S.shape and np.isfinite(out).all(), label
    bound = (m + MAP_U[name]) * U * S + U * np.abs(ref)
    err = np.abs(out.astype(LD) - ref)
    live = bound > 0
    ratio = float((err[live] / bound[live]).max()) if live.any() else 0.0
    print('%s [%s]: max |out - ref| / bound = %.3g (max |out - ref| = %.3e)' % (label, name, ratio, float(err.max())))
    worst = np.unravel_index(np.argmax(err - bound), err.shape)
    assert (err <= bound).all(), '%s: entry %s: |out - ref| = %.3e, bound %.3e' % (label, worst, float(err[worst]), float(bound[worst]))


# ---- A. column passes ------------------------------------------------------------------------------------------------------------
KA = 129
KS_A = (48, 64, 65, 80, 129)   # three groups; four full groups; second pass, one group / one full group; third pass
SPECS_A = {'rbf': _rbf(12), 'poly3': ('poly', 0.125, 1.0, 3)}


@functools.lru_cache(maxsize=None)
def _reference_a(case):
    SV, Xt, W, b = _real(1, M, T, 12, KA)
    return _frozen(*_reference(_kernel_values(SPECS_A[case], SV, Xt), W, b))


@pytest.mark.parametrize('k', KS_A)
def test_column_passes_on_integers(amd, monkeypatch, k):
    _no_hooks(monkeypatch)
    SV, Xt, W, b, want = _ints(2, M, T, 12, KA)
    np.testing.assert_array_equal(_multi(LINEAR, SV, W[:k], b[:k], Xt), want[:k])
    np.testing.assert_array_equal(_multi(LINEAR, SV, W[:k], None, Xt), want[:k] - b[:k, None])


@pytest.mark.parametrize('case', sorted(SPECS_A))
def test_column_passes_within_the_bound(amd, monkeypatch, case):
    _no_hooks(monkeypatch)
    SV, Xt, W, b = _real(1, M, T, 12, KA)
    ref, S = _reference_a(case)
    for k in KS_A:
        _within('A k=%d' % k, SPECS_A[case][0], _multi(SPECS_A[case], SV, W[:k], b[:k], Xt), ref[:k], S[:k], M)


@pytest.mark.parametrize('unit', [None, 3])
@pytest.mark.parametrize('case', sorted(SPECS_A))
def test_a_column_past_64_has_the_bits_it_has_alone(amd, monkeypatch, case, unit):
    """Column c of the 129-column call (passes 0, 1 and 2) against: c alone (the GMAX = 1 instantiation), c in a batch of 64 at
    another slot of another group, c in the reversed batch (another pass)."""
    _no_hooks(monkeypatch, decision_multi_unit=unit)
    spec = SPECS_A[case]
    SV, Xt, W, b = _real(1, M, T, 12, KA)
    full = _multi(spec, SV, W, b, Xt)
    _within('A k=129 unit=%s' % unit, spec[0], full, *_reference_a(case), M)
    rev = _multi(spec, SV, W[::-1], b[::-1], Xt)[::-1]
    for c in (0, 63, 64, 65, 127, 128):
        np.testing.assert_array_equal(_multi(spec, SV, W[c:c + 1], b[c:c + 1], Xt)[0], full[c], err_msg='column %d alone' % c)
        slot = (c + 21) % 64
        cols = (c - slot + np.arange(64)) % KA
        assert cols[slot] == c and slot != c % 64 and slot // 16 != (c % 64) // 16
        np.testing.assert_array_equal(_multi(spec, SV, W[cols], b[cols], Xt)[slot], full[c], err_msg='column %d at slot %d' % (c, slot))
        np.testing.assert_array_equal(rev[c], full[c], err_msg='column %d in the reversed batch' % c)


@pytest.mark.parametrize('unit', [None, 3])
def test_eighty_columns_under_the_unit_and_chunk_hooks(amd, monkeypatch, unit):
    """k = 80 (two passes) with the SV tiles in one unit of three or one each, and the test points in chunks of 128 rows: the bits of
    one chunk, the bits of the first 80 columns of the 129-column call, the bound, and the integer product."""
    SV, Xt, W, b = _real(1, M, T, 12, KA)
    SVi, Xti, Wi, bi, want = _ints(2, M, T, 12, KA)
    for case in sorted(SPECS_A):
        spec = SPECS_A[case]
        ref, S = _reference_a(case)
        _no_hooks(monkeypatch, decision_multi_unit=unit)
        one = _multi(spec, SV, W[:80], b[:80], Xt)
        _within('A k=80 unit=%s' % unit, spec[0], one, ref[:80], S[:80], M)
        np.testing.assert_array_equal(_multi(spec, SV, W, b, Xt)[:80], one)
        _no_hooks(monkeypatch, decision_multi_unit=unit, decision_multi_chunk_rows=128)
        np.testing.assert_array_equal(_multi(spec, SV, W[:80], b[:80], Xt), one)
    for chunk in (None, 128):
        _no_hooks(monkeypatch, decision_multi_unit=unit, decision_multi_chunk_rows=chunk)
        np.testing.assert_array_equal(_multi(LINEAR, SVi, Wi[:80], bi[:80], Xti), want[:80])


# ---- B. pow degrees --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('d', [12, 20])
@pytest.mark.parametrize('degree', [1, 4, 5])
def test_pow_degrees(amd, monkeypatch, degree, d):
    """(x / 8 + 1 / 2)^degree through `pow`: some arguments are negative (an odd degree keeps the sign, degree 4 does not)"""
    _no_hooks(monkeypatch)
    spec = ('poly', 0.125, 0.5, degree)
    SV, Xt, W, b = _real(3, M, T, d, 17)
    K = _kernel_values(spec, SV, Xt)
    assert (0.125 * (SV @ Xt.T) + 0.5 < 0).any() and ((K < 0).any() == (degree % 2 == 1))
    ref, S = _reference(K, W, b)
    for k in (5, 17):
        _within('B degree=%d d=%d k=%d' % (degree, d, k), 'poly', _multi(spec, SV, W[:k], b[:k], Xt), ref[:k], S[:k], M)


@pytest.mark.parametrize('d', [12, 20])
def test_degree_one_is_the_linear_kernel(amd, monkeypatch, d):
    """x ** 1 = x: degree 1 with gamma = 1 and coef0 = 0 has the bits of the linear kernel, and on integers those of the integer
    product.  The device's pow(x, 1.0) is not x for every x (this test failed on 47 % of the entries while degree 1 went through
    `pow`), so degree 1 has its own instantiation of the map (DEG = 1)."""
    _no_hooks(monkeypatch)
    SV, Xt, W, b = _real(3, M, T, d, 17)
    for k in (5, 17):
        np.testing.assert_array_equal(_multi(('poly', 1.0, 0.0, 1), SV, W[:k], b[:k], Xt), _multi(LINEAR, SV, W[:k], b[:k], Xt))
    SV, Xt, W, b, want = _ints(4, M, T, d, 17)
    np.testing.assert_array_equal(_multi(('poly', 1.0, 0.0, 1), SV, W, b, Xt), want)


# ---- C. the default unit split ---------------------------------------------------------------------------------------------------
MC, TC = 65700, 129   # 514 SV tiles


@functools.lru_cache(maxsize=None)
def _reference_c():
    SV, Xt, W, b = _real(5, MC, TC, 3, 17)
    return _frozen(*_reference(_kernel_values(_rbf(3), SV, Xt), W, b))


@pytest.mark.parametrize('k', [2, 17])
def test_default_unit_split(amd, monkeypatch, k):
    """m = 65 700, d = 3: at t = 100 (one test tile) the default is two SV tiles per unit, at t = 129 (two test tiles) three — see
    the module's docstring.  The default run has the bits of the run with the unit forced to that figure, and not those of the
    run with one tile per unit, which is held to the bound like the others."""
    spec = _rbf(3)
    SV, Xt, W, b = _real(5, MC, TC, 3, 17)
    W, b = W[:k], b[:k]
    ref, S = (a[:k] for a in _reference_c())
    _no_hooks(monkeypatch)
    default100, default129 = _multi(spec, SV, W, b, Xt[:100]), _multi(spec, SV, W, b, Xt)
    _within('C t=100 default k=%d' % k, 'rbf', default100, ref[:, :100], S[:, :100], MC)
    _within('C t=129 default k=%d' % k, 'rbf', default129, ref, S, MC)
    _no_hooks(monkeypatch, decision_multi_unit=2)
    two100, two129 = _multi(spec, SV, W, b, Xt[:100]), _multi(spec, SV, W, b, Xt)
    np.testing.assert_array_equal(default100, two100)
    np.testing.assert_array_equal(two129[:, :100], two100)
    _within('C t=129 unit=2 k=%d' % k, 'rbf', two129, ref, S, MC)
    _no_hooks(monkeypatch, decision_multi_unit=3)
    np.testing.assert_array_equal(_multi(spec, SV, W, b, Xt), default129)
    _no_hooks(monkeypatch, decision_multi_unit=1)
    one100 = _multi(spec, SV, W, b, Xt[:100])
    _within('C t=100 unit=1 k=%d' % k, 'rbf', one100, ref[:, :100], S[:, :100], MC)
    assert (one100 != default100).any() and (two129 != default129).any()   # the splits do associate the sums differently


@pytest.mark.parametrize('k', [2, 17])
def test_default_unit_split_on_integers(amd, monkeypatch, k):
    """entries in {-1, 0, 1}, W in {-2 .. 2}: |sums| <= 3 * 2 * 65 700, exact under every split"""
    SV, Xt, W, b, want = _ints(6, MC, TC, 3, 17, hi=1, whi=2)
    for unit in (None, 2, 1):
        _no_hooks(monkeypatch, decision_multi_unit=unit)
        np.testing.assert_array_equal(_multi(LINEAR, SV, W[:k], b[:k], Xt[:100]), want[:k, :100])
        np.testing.assert_array_equal(_multi(LINEAR, SV, W[:k], b[:k], Xt), want[:k])


# ---- D. k-chunks of the tile product ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('d', [1, 16, 17, 40, 64, 70, 90])   # 1, 1, 2, 3, 4, 5 and 6 chunks of 16
def test_k_chunks(amd, monkeypatch, d):
    _no_hooks(monkeypatch)
    xmax = 1.0 if d == 90 else 2.0
    spec = _rbf(d, xmax)
    SV, Xt, W, b = _real(7, M, T, d, 35, xmax)
    ref, S = _reference(_kernel_values(spec, SV, Xt), W, b)
    SVi, Xti, Wi, bi, want = _ints(8, M, T, d, 35)
    for k in (5, 35):
        _within('D d=%d k=%d' % (d, k), 'rbf', _multi(spec, SV, W[:k], b[:k], Xt), ref[:k], S[:k], M)
        np.testing.assert_array_equal(_multi(LINEAR, SVi, Wi[:k], bi[:k], Xti), want[:k])


# ---- E. degenerate and exact-edge shapes -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('k', [1, 17])
@pytest.mark.parametrize('m,t,d', [(1, 1, 12), (1, 1, 1), (1, 165, 12), (300, 1, 12), (128, 128, 12), (129, 129, 12), (100, 300, 12)])
def test_degenerate_shapes(amd, monkeypatch, m, t, d, k):
    _no_hooks(monkeypatch)
    spec = _rbf(d)
    SV, Xt, W, b = _real(9, m, t, d, k)
    K = _kernel_values(spec, SV, Xt)
    _within('E m=%d t=%d d=%d k=%d' % (m, t, d, k), 'rbf', _multi(spec, SV, W, b, Xt), *_reference(K, W, b), m)
    SVi, Xti, Wi, bi, want = _ints(10, m, t, d, k)
    np.testing.assert_array_equal(_multi(LINEAR, SVi, Wi, bi, Xti), want)
    # columns without a coefficient: the intercept, exactly, and 0.0 without intercepts — alone (k = 1) and beside live columns
    dead = [0] if k == 1 else [0, 7, 16]
    Wz = W.copy()
    Wz[dead] = 0.0
    refz, Sz = _reference(K, Wz, b)
    for sp, sv, xt in ((spec, SV, Xt), (LINEAR, SVi, Xti)):
        out = _multi(sp, sv, Wz, b, xt)
        np.testing.assert_array_equal(out[dead], np.repeat(b[dead, None], t, axis=1))
        none = _multi(sp, sv, Wz, None, xt)
        np.testing.assert_array_equal(none[dead], np.zeros((len(dead), t)))
        if sp is spec:
            _within('E zero columns m=%d t=%d d=%d k=%d' % (m, t, d, k), 'rbf', out, refz, Sz, m)
            _within('E zero columns, no intercepts', 'rbf', none, *_reference(K, Wz, None), m)


# ---- F. RBF edge values ----------------------------------------------------------------------------------------------------------
def test_rbf_test_points_equal_to_support_vectors(amd, monkeypatch):
    """40 test points are copies of support vectors: the distance clamps to 0 and the kernel value is exactly 1, so a column whose
    only coefficient is a 1 on that support vector returns 1 + b there, exactly"""
    _no_hooks(monkeypatch)
    spec = _rbf(12)
    SV, Xt, W, b = _real(11, M, T, 12, 40)
    src = np.random.RandomState(12).permutation(M)[:40]
    at = np.random.RandomState(13).permutation(T)[:40]
    Xt = Xt.copy()
    Xt[at] = SV[src]
    K = _kernel_values(spec, SV, Xt)
    assert (K[src, at] == 1.0).all()
    for k in (17, 40):
        _within('F copies k=%d' % k, 'rbf', _multi(spec, SV, W[:k], b[:k], Xt), *_reference(K, W[:k], b[:k]), M)
    hot = np.zeros((40, M))
    hot[np.arange(40), src] = 1.0
    out = _multi(spec, SV, hot, b, Xt)
    np.testing.assert_array_equal(out[np.arange(40), at], 1.0 + b)
    _within('F one-hot k=40', 'rbf', out, *_reference(K, hot, b), M)
    for c in (0, 39):   # one column: the other instantiation
        np.testing.assert_array_equal(_multi(spec, SV, hot[c:c + 1], b[c:c + 1], Xt)[0, at[c]], 1.0 + b[c])
        np.testing.assert_array_equal(_multi(spec, SV, hot[c:c + 1], None, Xt)[0, at[c]], 1.0)


@pytest.mark.parametrize('k', [5, 17])
def test_rbf_underflow(amd, monkeypatch, k):
    """d = 1, gamma = 64: arguments down to -64 * 4^2 = -1024.  Beyond -745.2 the reference value is exactly 0 (asserted: the one
    place where reference zeros occur), between -708 and -745 it is subnormal."""
    _no_hooks(monkeypatch)
    spec = ('rbf', 64.0, 0.0, 1)
    SV, Xt, W, b = _real(14, M, T, 1, 17)
    arg = -64.0 * (SV[:, 0][:, None] - Xt[:, 0][None, :]) ** 2
    assert arg.min() < -745.2 and ((arg < -708.4) & (arg > -745.1)).any()
    K = _kernel_values(spec, SV, Xt, zeros=True)
    assert (K[arg < -745.2] == 0).all() and (K == 0).sum() > 1000
    _within('F underflow k=%d' % k, 'rbf', _multi(spec, SV, W[:k], b[:k], Xt), *_reference(K, W[:k], b[:k]), M)


# ---- G. the single-column path ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('m,t,d', [(300, 165, 12), (300, 165, 20), (1, 165, 12), (300, 1, 12)])
@pytest.mark.parametrize('name', ['sigmoid', 'laplacian'])
def test_single_column_sigmoid_and_laplacian(amd, monkeypatch, name, m, t, d):
    """`bq_decision_function`: sigmoid tanh(x / 16 + 1 / 2) and Laplacian exp(-gamma sum |a - b|) with gamma sum <= 10"""
    _no_hooks(monkeypatch)
    spec = ('sigmoid', 0.0625, 0.5, 1) if name == 'sigmoid' else ('laplacian', 2.0 ** np.floor(np.log2(10.0 / (4.0 * d))), 0.0, 1)
    SV, Xt, W, b = _real(15, m, t, d, 2)
    K = _kernel_values(spec, SV, Xt)
    ref, S = _reference(K, W, b)
    outs = np.stack([_single(spec, SV, W[c], b[c], Xt) for c in range(2)])
    _within('G m=%d t=%d d=%d' % (m, t, d), name, outs, ref, S, m)
    _no_hooks(monkeypatch, decision_chunk_rows=128)
    np.testing.assert_array_equal(np.stack([_single(spec, SV, W[c], b[c], Xt) for c in range(2)]), outs)


def test_single_column_exact_values(amd, monkeypatch):
    """Laplacian: a test point equal to the only support vector gives w + b (exp(0) = 1); sigmoid: a test point at the origin
    with coef0 = 0 gives b (tanh(0) = 0) — alone and among other test points"""
    _no_hooks(monkeypatch)
    SV, Xt, W, b = _real(16, M, T, 12, 1)
    Xt = Xt.copy()
    Xt[[0, 130]] = 0.0
    out = _single(('sigmoid', 0.0625, 0.0, 1), SV, W[0], b[0], Xt)
    np.testing.assert_array_equal(out[[0, 130]], b[0])
    np.testing.assert_array_equal(_single(('sigmoid', 0.0625, 0.0, 1), SV, W[0], b[0], Xt[:1]), b[:1])
    lap = ('laplacian', 0.125, 0.0, 1)
    Xt[[0, 130]] = SV[7]
    np.testing.assert_array_equal(_single(lap, SV[7:8], W[0, 7:8], b[0], Xt)[[0, 130]], W[0, 7] + b[0])
    np.testing.assert_array_equal(_single(lap, SV[7:8], W[0, 7:8], b[0], SV[7:8]), W[0, 7:8] + b[0])


# ---- H. an estimator past 64 columns ---------------------------------------------------------------------------------------------
def test_one_vs_one_with_66_pairs(amd, monkeypatch):
    from optiml_amd.datasets import make_multiclass_blobs
    from optiml_amd.ml.svm import OneVsOneSVC
    from optiml_amd.ml.svm.kernels import GaussianKernel
    from optiml_amd.ml.svm.losses import hinge
    from optiml_amd.ml.svm.onevsone import ovo_decision
    from optiml_amd.opti.constrained import ProjectedGradient
    _no_hooks(monkeypatch)
    X, y = make_multiclass_blobs(610, 8, 12, seed=1)
    Xtr, ytr, Xte = X[:480], y[:480], X[480:]
    est = OneVsOneSVC(loss=hinge, kernel=GaussianKernel(gamma=0.5), C=1.0, reg_intercept=True, dual=True, max_iter=20,
                      optimizer=ProjectedGradient).fit(Xtr, ytr)
    assert len(est.classes_) == 12 and est.batched_ and est.batched_decision_ is True and len(est.estimators_) == 66
    assert est.decision_batch_.W.shape[0] == 66
    conf = np.stack([np.ravel(e.decision_function(Xte)) for e in est.estimators_], axis=1)
    loop = ovo_decision((conf > 0).astype(int), conf, 12)
    ours = est.decision_function(Xte)
    assert ours.shape == loop.shape == (130, 12)
    print('H: max |batched - loop| = %.3e, max relative %.3e' % (np.abs(ours - loop).max(), (np.abs(ours - loop) / np.abs(loop)).max()))
    np.testing.assert_allclose(ours, loop, rtol=1e-11)
    np.testing.assert_array_equal(est.predict(Xte), est.classes_[np.argmax(loop, axis=1)])
