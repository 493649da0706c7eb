"""The packed symmetric panel stores each strip (8 tiles of a tile row) as its own row-major 256 x W block (csrc/bq_sym_layout.h).
Only addresses changed, so every reader and writer of the panel is walked here at the sizes where the address map can go wrong:
nb = 1 (n = 200), nb = 8 (n = 2048: the last tile row is exactly one full strip), nb = 9 (n = 2049, 2304: a second strip of one
tile, W = 256) and nb = 17 (n = 4200: three strips, the last ragged, ragged n).

Against a problem built with BQ_FULL_PANEL (whole rows, gemv_rows_kernel — no packed address anywhere):
  * the panel download is held to the oracle's Gram matrix at the existing rtol 1e-12 / atol 1e-14 (tests/test_gpu_smo.py) — the
    two downloads were never bit-identical above the diagonal tiles (K_ij and K_ji come from different MFMA tiles);
  * matvec / gram_matvec: the packed product and the row product never were bit-identical (other summation order); they are held to
    the tolerance tests/test_gpu_parity.py::test_symmetric_tile_product_against_oracle holds the packed product to
    (rtol 1e-11, atol 1e-11 x the largest absolute row sum);
  * the four-column, sixteen-column and pair-routed products are products of the packed panel only (bq_symm.hip: "needs a resident packed panel"): they are held at
    that same tolerance to NumPy's product with the full panel's download;
  * a PG and an FW solve of 30 iterations: held to the tolerance tests/test_gpu_parity.py::test_ragged_sizes_dense holds these
    solvers to (f history rtol 1e-8 / atol 1e-10, x rtol 1e-6 / atol 1e-8).
Bit for bit: compact download == plain download; the per-segment products (the eight shares (k, 8)) added in order == the one-rank
product and == every share (k, G)'s product over its segments, G = 2, 3; SMO on the compact panel == SMO on the plain panel."""
import numpy as np
import pytest

from conftest import set_hooks

pytestmark = pytest.mark.gpu

SIZES = [200, 2048, 2049, 2304, 4200]


@pytest.fixture(scope='module')
def amd():
    from optiml_amd import _lib
    from optiml_amd.device import get_context
    _lib.load()
    get_context()


_cache = {}


def _data(n):
    """(X, y, gamma, oracle K) of size n: computed once and shared, never written to"""
    if n not in _cache:
        from oracle import svm_oracle as so
        from optiml_amd.datasets import make_blobs
        X, y = make_blobs(n, 12, seed=n)
        gamma = 0.5 * 14 * np.log(2) / (4 * (X * X).sum(axis=1).max())   # eligible for the compact layout (bq_c7_eligible)
        K = so.gram('rbf', X, gamma=gamma)
        for a in (X, y, K):
            a.setflags(write=False)
        _cache[n] = (X, y, gamma, K)
    return _cache[n]


def _quad(n, storage='f64', kernel=None, **kw):
    from optiml_amd.opti import KernelQuadratic
    from optiml_amd.ml.svm.kernels import GaussianKernel
    X, y, gamma, _ = _data(n)
    return KernelQuadratic(X, -np.ones(n), 'svc', kernel or GaussianKernel(gamma=gamma), y=y, storage=storage, **kw)


def _elems(n):
    nb = (n + 255) // 256
    return 65536 * nb * (nb + 1) // 2


@pytest.mark.parametrize('n', SIZES)
def test_downloaded_panel_equals_the_oracle_gram_matrix(amd, monkeypatch, n):
    from oracle import svm_oracle as so
    from optiml_amd.ml.svm.kernels import PolyKernel
    X, y, gamma, K = _data(n)
    got = {}
    for name, hook, storage in (('compact', None, 'f64'), ('plain', 0, 'f64'), ('f32', None, 'f32')):
        set_hooks(monkeypatch, compact_panel=hook)
        quad = _quad(n, storage)
        esz = {'compact': 7, 'plain': 8, 'f32': 4}[name]
        assert quad.device_problem().layout()['panel_bytes'] == _elems(n) * esz, name
        got[name] = quad.gram()
        quad.release()
    set_hooks(monkeypatch, compact_panel=None)
    np.testing.assert_allclose(got['compact'], K, rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(got['plain'], K, rtol=1e-12, atol=1e-14)
    assert np.array_equal(got['compact'], got['plain'])   # bit for bit
    # fp32 storage: the fp64 value rounded once to fp32 (half an ulp: 2^-24 relative), on top of the fp64 bound
    np.testing.assert_allclose(got['f32'], K, rtol=2.0 ** -24 + 1e-12, atol=1e-14)
    quad = _quad(n, kernel=PolyKernel(3, gamma, 1.))
    Kp = so.gram('poly', X, gamma=gamma, coef0=1., degree=3)
    np.testing.assert_allclose(quad.gram(), Kp, rtol=1e-12, atol=1e-14)
    quad.release()
    full = _quad(n, full_panel=True)
    np.testing.assert_allclose(full.gram(), K, rtol=1e-12, atol=1e-14)
    full.release()


def _solve(quad, n):
    from optiml_amd.opti.constrained import ProjectedGradient, FrankWolfe
    res = {}
    for name, cls in (('pg', ProjectedGradient), ('fw', FrankWolfe)):
        hist = []
        cb = lambda o: hist.append(o.f_x)
        cb._bq_needs_state = False
        opt = cls(quad=quad, ub=np.ones(n), max_iter=30, callback=cb).minimize()
        res[name] = (opt.x, np.array(hist))
    return res


@pytest.mark.parametrize('n', SIZES)
def test_products_and_solves_against_the_full_panel(amd, monkeypatch, n):
    from optiml_amd.ml.svm._batched import _gram_matmat
    X, y, gamma, K = _data(n)
    rs = np.random.RandomState(n)
    v = rs.standard_normal(n)
    W = rs.standard_normal((16, n))
    full = _quad(n, full_panel=True)
    assert not full.device_problem().layout()['packed']
    Kf = full.gram()
    want = {'matvec': full.device_problem().matvec(v), 'gram_matvec': full.device_problem().gram_matvec(v), 'mm': W @ Kf}
    want_solve = _solve(full, n)
    full.release()
    Q = (K + 1) * np.outer(y, y)
    tolQ, tolK = 1e-11 * np.abs(Q).sum(1).max(), 1e-11 * np.abs(K).sum(1).max()
    for hook in (None, 0):   # the compact and the plain fp64 layout
        set_hooks(monkeypatch, compact_panel=hook)
        quad = _quad(n)
        dev = quad.device_problem()
        assert dev.layout()['packed']
        np.testing.assert_allclose(dev.matvec(v), want['matvec'], rtol=1e-11, atol=tolQ)
        np.testing.assert_allclose(dev.gram_matvec(v), want['gram_matvec'], rtol=1e-11, atol=tolK)
        np.testing.assert_allclose(_gram_matmat(dev, W[:4], wide=False), want['mm'][:4], rtol=1e-11, atol=tolK * np.abs(W).max())
        np.testing.assert_allclose(_gram_matmat(dev, W, wide=True), want['mm'], rtol=1e-11, atol=tolK * np.abs(W).max())
        got = _solve(quad, n)
        for s in ('pg', 'fw'):
            np.testing.assert_allclose(got[s][1], want_solve[s][1], rtol=1e-8, atol=1e-10, err_msg=s)
            np.testing.assert_allclose(got[s][0], want_solve[s][0], rtol=1e-6, atol=1e-8, err_msg=s)
        quad.release()
    set_hooks(monkeypatch, compact_panel=None)


@pytest.mark.parametrize('ct', [[0, 1, 2], [0, 3, 9], [0, 3, 12, 17], [0, 8, 16, 17]])
def test_pair_routed_product_across_the_strip_seams(amd, monkeypatch, ct):
    """class blocks that start anywhere: their strips of 8 (single column) and 4 (diagonal) tiles straddle the layout's strips"""
    from optiml_amd.ml.svm.onevsone import gram_matmat_pairs, ovo_pairs
    from optiml_amd.opti import KernelQuadratic
    from optiml_amd.ml.svm.kernels import GaussianKernel
    n = 256 * ct[-1]
    rs = np.random.RandomState(ct[-1])
    X = rs.standard_normal((n, 6))
    gamma = 0.5 * 14 * np.log(2) / (4 * (X * X).sum(axis=1).max())
    pairs = ovo_pairs(len(ct) - 1)
    W = np.zeros((len(pairs), n))
    masks = []
    for p, (a, b) in enumerate(pairs):
        m = np.zeros(n, bool)
        m[256 * ct[a]:256 * ct[a + 1]] = m[256 * ct[b]:256 * ct[b + 1]] = True
        W[p, m] = rs.standard_normal(m.sum())
        masks.append(m)
    full = KernelQuadratic(X, -np.ones(n), 'svc', GaussianKernel(gamma=gamma), y=np.ones(n), full_panel=True)
    Kf = full.gram()
    full.release()
    want = np.stack([m * (Kf @ W[p]) for p, m in enumerate(masks)])
    outs = []
    for hook in (None, 0):
        set_hooks(monkeypatch, compact_panel=hook)
        quad = KernelQuadratic(X, -np.ones(n), 'svc', GaussianKernel(gamma=gamma), y=np.ones(n))
        outs.append(gram_matmat_pairs(quad.device_problem(), np.array(ct, np.int32), pairs, W))
        quad.release()
    set_hooks(monkeypatch, compact_panel=None)
    np.testing.assert_allclose(outs[0], want, rtol=1e-11, atol=1e-11 * np.abs(Kf).sum(1).max() * np.abs(W).max())
    assert np.array_equal(outs[0], outs[1])   # compact and plain layout: bit for bit


def _share_products(monkeypatch, n, v, G):
    """{(hook, k): share (k, G)'s product} for the compact (hook None) and the plain (hook 0) layout"""
    from optiml_amd import device
    parts = {}
    for hook in (None, 0):
        set_hooks(monkeypatch, compact_panel=hook)
        rows = 0
        for k in range(G):
            ctx = device.Context(device=0, share=(k, G))
            quad = _quad(n)
            dev = quad.device_problem(ctx)
            _, _, r0, r1 = dev.dims()
            assert (r0, r1) == device.row_block(n, k, G, symmetric=True)
            rows += r1 - r0
            parts[hook, k] = dev.matvec(v)
            quad.release()
            ctx.close()
        assert rows == n
    set_hooks(monkeypatch, compact_panel=None)
    return parts


def test_share_context_segments_sum_to_the_one_rank_product(amd, monkeypatch):
    """Share context (k, G) holds the tile rows from I0 > 0 on and returns 0 + s_lo + s_lo+1 + ..., its own canonical segments added in
    segment order (bq_sym_seg_first: share k owns segments [8k / G, 8(k + 1) / G)).  A share of G = 8 is ONE segment, so the eight
    (k, 8) products are the per-segment products.  Bit for bit, for the compact and the plain layout: the eight added in order are the
    one-rank product, and the product of every share (k, G), G = 2, 3, is the in-order sum of the segments it owns.  (The shares of
    G = 2, 3 added to each other have another association than the one-rank product: that sum is held to the rtol 1e-12 /
    atol 1e-12 max|.| of tests/test_distributed.py's share test, on top.)"""
    n = 4200
    v = np.random.RandomState(7).standard_normal(n)
    one = _quad(n)
    want = one.device_problem().matvec(v)
    one.release()
    seg = _share_products(monkeypatch, n, v, 8)
    for hook in (None, 0):
        acc = np.zeros(n)
        for s in range(8):
            acc = acc + seg[hook, s]
        assert np.array_equal(acc, want), hook
    for G in (2, 3):
        parts = _share_products(monkeypatch, n, v, G)
        for hook in (None, 0):
            total = np.zeros(n)
            for k in range(G):
                acc = np.zeros(n)
                for s in range(8 * k // G, 8 * (k + 1) // G):
                    acc = acc + seg[hook, s]
                assert np.array_equal(parts[hook, k], acc), (G, k, hook)
                total = total + parts[hook, k]
            np.testing.assert_allclose(total, want, rtol=1e-12, atol=1e-12 * np.abs(want).max())


def test_smo_on_the_compact_panel_follows_the_plain_panel(amd, monkeypatch):
    from optiml_amd.opti import KernelQuadratic
    from optiml_amd.ml.svm.kernels import GaussianKernel
    from optiml_amd.ml.svm.smo import SMOClassifier
    n = 2304
    X, y, gamma, _ = _data(n)
    kern = GaussianKernel(gamma=gamma)
    res = []
    for hook in (None, 0):
        set_hooks(monkeypatch, compact_panel=hook)
        quad = KernelQuadratic(X, -np.ones(n), 'svc', kern, y=y, rank_one=False)
        assert quad.device_problem().layout()['panel_bytes'] == _elems(n) * (7 if hook is None else 8)
        opt = SMOClassifier(quad, X, y, None, kern, 1., 1e-3, False).minimize()
        res.append((opt.iter, opt.steps, opt.alphas, opt.errors, opt.b))
        quad.release()
    set_hooks(monkeypatch, compact_panel=None)
    assert res[0][0] == res[1][0] and res[0][1] == res[1][1] and res[0][1] > 0   # the same pair steps
    assert np.array_equal(res[0][2], res[1][2]) and np.array_equal(res[0][3], res[1][3]) and res[0][4] == res[1][4]


def test_dense_symmetric_quadratic_product(amd):
    from optiml_amd.opti import Quadratic
    n = 2304
    rs = np.random.RandomState(3)
    G = rs.standard_normal((n, 40))
    Q = G @ G.T / 40 + np.diag(rs.uniform(0.5, 1.0, n))
    Q = (Q + Q.T) / 2
    v = rs.standard_normal(n)
    for lower in (False, True):
        quad = Quadratic(np.tril(Q) if lower else Q, rs.standard_normal(n), symmetric=True if lower else None)
        dev = quad.device_problem()
        assert dev.layout()['packed'] and dev.layout()['panel_bytes'] == _elems(n) * 8
        np.testing.assert_allclose(dev.matvec(v), Q @ v, rtol=1e-11, atol=1e-11 * np.abs(Q).sum(1).max())
        quad.release()
