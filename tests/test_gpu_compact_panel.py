"""The compact fp64 panel layout (csrc/bq_c7.h): eligible RBF panels are stored in 7 bytes per element and every reader decodes
them.  No arithmetic changes, so every product, solve and panel download must equal the plain layout (hook compact_panel=0) bit
for bit; panels that are not eligible keep 8 bytes per element."""
import numpy as np
import pytest

from conftest import set_hooks

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def amd():
    from optiml_amd import _lib
    from optiml_amd.device import get_context
    _lib.load()
    get_context()


def _elems(n):
    nb = (n + 255) // 256
    return 65536 * nb * (nb + 1) // 2


def _gamma(X, frac=0.5):
    """a gamma that keeps exp(-gamma 4 max|x|^2) at 2^(-14 frac): eligible for frac < 1"""
    return frac * 14 * np.log(2) / (4 * (X * X).sum(axis=1).max())


def _svc(X, y, gamma, storage='f64'):
    from optiml_amd.opti import KernelQuadratic
    from optiml_amd.ml.svm.kernels import GaussianKernel
    return KernelQuadratic(X, -np.ones(len(X)), 'svc', GaussianKernel(gamma=gamma), y=y, storage=storage)


def _both(monkeypatch, make, run):
    """run(quad) on the plain layout (hook compact_panel=0) and on the compact one; the layouts are checked on the way"""
    out = []
    for compact in (True, False):   # compact first: the plain panel does not fit in its cached allocation (panels >= 1 GiB)
        set_hooks(monkeypatch, compact_panel=None if compact else 0)
        quad = make()
        dev = quad.device_problem()
        n = dev.dims()[1]
        want, got = _elems(n) * (7 if compact else 8), dev.layout()['panel_bytes']
        assert got == want or (want >= 2 ** 30 and want < got <= want * 1.25), (compact, got, want)   # or a cached panel
        out.append(run(quad))
        quad.release()
    set_hooks(monkeypatch, compact_panel=None)
    return out[::-1]


def _equal(a, b):
    if isinstance(a, dict):
        assert a.keys() == b.keys()
        for k in a:
            assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k
    else:
        assert np.array_equal(np.asarray(a), np.asarray(b))


def _blobs(n, d, seed=0):
    from optiml_amd.datasets import make_blobs
    return make_blobs(n, d, seed=seed)


@pytest.mark.parametrize('n', [200, 1000, 2049])
def test_products_and_panel_rows_equal_the_plain_layout(amd, monkeypatch, n):
    X, y = _blobs(n, 16, seed=n)
    g = _gamma(X)
    v = np.random.RandomState(1).standard_normal(n)

    def run(quad):
        dev = quad.device_problem()
        return {'matvec': dev.matvec(v), 'gram_matvec': dev.gram_matvec(v), 'rows': dev.panel_rows(0, n)}
    plain, comp = _both(monkeypatch, lambda: _svc(X, y, g), run)
    _equal(plain, comp)
    assert np.all(comp['rows'][np.tril_indices(n)] >= 2.0 ** -14)


@pytest.mark.parametrize('n', [300, 1000])
def test_pg_and_fw_iterates_equal_the_plain_layout(amd, monkeypatch, n):
    from optiml_amd.opti.constrained import ProjectedGradient, FrankWolfe
    X, y = _blobs(n, 12, seed=3)
    g = _gamma(X)

    def run(quad):
        res = {}
        for name, cls in (('pg', ProjectedGradient), ('fw', FrankWolfe)):
            hist = []
            cb = lambda o: hist.append(o.f_x)
            cb._bq_needs_state = False
            opt = cls(quad=quad, ub=np.ones(n), max_iter=50, callback=cb).minimize()
            res[name + '_x'], res[name + '_f'] = opt.x, np.array(hist)
        res['g'] = quad.device_problem().eval(res['pg_x'])[1]
        return res
    plain, comp = _both(monkeypatch, lambda: _svc(X, y, g), run)
    _equal(plain, comp)


def test_smo_ip_and_active_set_equal_the_plain_layout(amd, monkeypatch):
    from optiml_amd.ml.svm import SVC
    from optiml_amd.ml.svm.kernels import GaussianKernel
    from optiml_amd.ml.svm.losses import hinge
    from optiml_amd.opti.constrained import InteriorPoint, ActiveSet
    n = 300
    X, y = _blobs(n, 8, seed=7)
    g = _gamma(X, 0.9)

    def run(quad):
        res = {}
        res['ip_x'] = InteriorPoint(quad=quad, ub=np.ones(n), max_iter=30).minimize().x
        res['as_x'] = ActiveSet(quad=quad, ub=np.ones(n), max_iter=60).minimize().x
        return res
    plain, comp = _both(monkeypatch, lambda: _svc(X, y, g), run)
    _equal(plain, comp)
    # SMO on a compact panel (SVC.fit keeps SMO's panel at 8 bytes: BQ_PLAIN_PANEL, below)
    from optiml_amd.opti import KernelQuadratic
    from optiml_amd.ml.svm.smo import SMOClassifier
    kern = GaussianKernel(gamma=g)
    make = lambda: KernelQuadratic(X, -np.ones(n), 'svc', kern, y=y, rank_one=False)
    plain, comp = _both(monkeypatch, make, lambda q: SMOClassifier(q, X, y, None, kern, 1., 1e-3, False).minimize().alphas)
    _equal(plain, comp)
    est = SVC(loss=hinge, kernel=kern, C=1., dual=True, optimizer='smo').fit(X, y)
    assert est.obj.device_problem().layout()['panel_bytes'] == _elems(n) * 8


def test_multi_column_products_equal_the_plain_layout(amd, monkeypatch):
    from optiml_amd.ml.svm.multiclass import _gram_matmat
    from optiml_amd.ml.svm.onevsone import gram_matmat_pairs, sort_plan, ovo_pairs
    sizes = [255, 300, 1, 500]
    rs = np.random.RandomState(0)
    codes = np.concatenate([np.full(s, c) for c, s in enumerate(sizes)])
    rs.shuffle(codes)
    X0 = rs.standard_normal((len(codes), 6)) + codes[:, None]
    index, ct, n_pad = sort_plan(codes, len(sizes))
    Xp = np.zeros((n_pad, 6))
    Xp[index] = X0
    g = _gamma(Xp)
    pairs = ovo_pairs(len(sizes))
    W = rs.standard_normal((40, n_pad))

    def run(quad):
        dev = quad.device_problem()
        return {'ovr': _gram_matmat(dev, W[:7], wide=False), 'wide': _gram_matmat(dev, W, wide=True),
                'pairs': gram_matmat_pairs(dev, ct, pairs, W[:len(pairs)])}
    plain, comp = _both(monkeypatch, lambda: _svc(Xp, np.ones(n_pad), g), run)
    _equal(plain, comp)


@pytest.mark.parametrize('world', [2, 8])
def test_share_contexts_equal_the_plain_layout(amd, monkeypatch, world):
    from optiml_amd import device
    n = 3000
    X, y = _blobs(n, 16, seed=5)
    g = _gamma(X)
    v = np.random.RandomState(1).standard_normal(n)
    for k in range(world):
        parts = []
        for hook in (0, None):
            set_hooks(monkeypatch, compact_panel=hook)
            ctx = device.Context(device=0, share=(k, world))
            quad = _svc(X, y, g)
            dev = quad.device_problem(ctx)
            _, _, r0, r1 = dev.dims()
            parts.append((dev.matvec(v), dev.panel_rows(r0, min(r1 - r0, 3)) if r1 > r0 else np.zeros(0),
                          dev.layout()['panel_bytes']))
            quad.release()
            ctx.close()
        set_hooks(monkeypatch, compact_panel=None)
        assert np.array_equal(parts[0][0], parts[1][0]) and np.array_equal(parts[0][1], parts[1][1]), k
        assert parts[1][2] * 8 == parts[0][2] * 7 or parts[0][2] <= 1, k


def test_headline_fixture_equals_the_plain_layout(amd, monkeypatch):
    """the bench's data at n = 100 000 is eligible with gamma='scale' (exp(-gamma 4 max|x|^2) ~ 2^-9)"""
    from optiml_amd.opti.constrained import ProjectedGradient
    from optiml_amd.ml.svm.kernels import gaussian
    from optiml_amd.opti import KernelQuadratic
    n = 100000
    X, y = _blobs(n, 128, seed=0)
    v = np.random.RandomState(2).standard_normal(n)

    def run(quad):
        dev = quad.device_problem()
        rows = np.array([0, 255, 256, 50000, 99999])
        res = {'matvec': dev.matvec(v), 'gram_matvec': dev.gram_matvec(v),
               'rows': np.concatenate([dev.panel_rows(r, 1)[0] for r in rows])}
        res['pg_x'] = ProjectedGradient(quad=quad, ub=np.ones(n), max_iter=5).minimize().x
        return res
    plain, comp = _both(monkeypatch, lambda: KernelQuadratic(X, -np.ones(n), 'svc', gaussian, y=y), run)
    _equal(plain, comp)


@pytest.mark.parametrize('case', ['poly', 'linear', 'big_gamma', 'f32', 'laplacian'])
def test_ineligible_panels_keep_the_plain_layout(amd, case):
    from optiml_amd.opti import KernelQuadratic
    from optiml_amd.ml.svm.kernels import GaussianKernel, PolyKernel, linear, LaplacianKernel
    n = 700
    X, y = _blobs(n, 8, seed=2)
    kern = {'poly': PolyKernel(3, 'scale', 1.), 'linear': linear, 'big_gamma': GaussianKernel(gamma=_gamma(X, 1.5)),
            'f32': GaussianKernel(gamma=_gamma(X)), 'laplacian': LaplacianKernel(gamma=0.001)}[case]
    quad = KernelQuadratic(X, -np.ones(n), 'svc', kern, y=y, storage='f32' if case == 'f32' else 'f64')
    assert quad.device_problem().layout()['panel_bytes'] == _elems(n) * (4 if case == 'f32' else 8)
    quad.release()
