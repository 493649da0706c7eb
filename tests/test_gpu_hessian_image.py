"""The Hessian image (csrc/bq_h52.h): for a compact RBF panel with the rank-one term the one-column product of ProjectedGradient /
FrankWolfe streams fl(K + 1) in 6.5 bytes per element from a second allocation instead of K in 7 bytes from the panel.  Every FMA sees
the operand it saw, so everything here is held BIT FOR BIT against the same build with the hook hessian_image=0 (the panel's product):
single products (random, sparse, duplicate rows of X: K = 1 off the diagonal, the escape code), 30-iteration trajectories of PG and FW
on the SVC dual and PG on the SVR dual (x, g, every per-step record), the share contexts' segment products, and every fallback — each of
which must also name its reason through bq_problem_hessian_image.  Sizes: n = 300 (one ragged tile row), 513, 2 100 (nb = 9: tile row 8
has a second strip of one tile), 4 200 (strips of 8, 8 and 1 tiles, ragged last tile); d = 8.

The product's output vector keeps pad rows up to nb * 256 on the device; the test entry bq_problem_last_product (hook product_rows=1)
hands out all of them, and test_pad_rows_of_the_product_are_equal compares every one."""
import numpy as np
import pytest

from conftest import set_hooks

pytestmark = pytest.mark.gpu

SIZES = [300, 513, 2100, 4200]
MANY = 1e9   # expected products: the image always repays its build


@pytest.fixture(scope='module')
def amd():
    from optiml_amd import _lib
    from optiml_amd.device import get_context
    _lib.load()
    get_context()


@pytest.fixture(autouse=True)
def _keep_the_image_at_test_sizes(monkeypatch):
    """The library keeps an image only where its product, timed on the problem, beats the panel's; at these sizes a product is a few
    microseconds of launch latency, so the tests switch that comparison off (hessian_image_gain=0) except where it is the subject."""
    set_hooks(monkeypatch, hessian_image_gain=0)


_cache = {}


def _data(n, dup=False):
    """(X, y, gamma) of size n, shared and never written to; dup: rows of X repeated inside a tile, across tiles and across strips"""
    if (n, dup) not in _cache:
        from optiml_amd.datasets import make_blobs
        X, y = make_blobs(n, 8, seed=n)
        if dup:
            X = X.copy()
            for i in range(1, n, 7):
                X[i] = X[(i * 5) % 3]   # one of three source rows: many pairs i != j with K_ij = 1 exactly
        gamma = 0.5 * 14 * np.log(2) / (4 * (X * X).sum(axis=1).max())   # eligible for the compact layout (bq_c7_eligible)
        for a in (X, y):
            a.setflags(write=False)
        _cache[n, dup] = (X, y, gamma)
    return _cache[n, dup]


def _elems(n):
    nb = (n + 255) // 256
    return 65536 * nb * (nb + 1) // 2


def _quad(n, structure='svc', dup=False, expected=MANY, **kw):
    from optiml_amd.opti import KernelQuadratic
    from optiml_amd.ml.svm.kernels import GaussianKernel
    X, y, gamma = _data(n, dup)
    if structure == 'svc':
        return KernelQuadratic(X, -np.ones(n), 'svc', GaussianKernel(gamma=gamma), y=y, expected_products=expected, **kw)
    t = np.sin(X[:, 0]) + 0.1 * X[:, 1]
    return KernelQuadratic(X, np.hstack((-t, t)) + 0.1, 'svr', GaussianKernel(gamma=gamma), expected_products=expected, **kw)


def _solver(dev, kind):
    from optiml_amd.opti.constrained._base import _DeviceSolver
    N = dev.dims()[0]
    return _DeviceSolver(dev, kind, np.zeros(N), np.ones(N), np.full(N, 0.5), 1e-6, 10 ** 9)


def _with_image(n, ctx=None, **kw):
    """(quad, dev, solver): a problem whose image is built (the first PG solver builds it); the compact panel is asserted"""
    from optiml_amd import _lib
    quad = _quad(n, **kw)
    dev = quad.device_problem(ctx)
    solver = _solver(dev, _lib.PG)
    return quad, dev, solver


def _vectors(N, seed):
    rs = np.random.RandomState(seed)
    dense = rs.standard_normal(N)
    sparse = np.where(rs.uniform(size=N) < 0.03, rs.standard_normal(N), 0.0)
    return {'random': dense, 'sparse': sparse, 'one_hot': np.eye(1, N, N - 1)[0]}


@pytest.mark.parametrize('dup', [False, True], ids=['blobs', 'duplicate_rows'])
@pytest.mark.parametrize('n', SIZES)
def test_product_through_the_image_equals_the_panel_product(amd, monkeypatch, n, dup):
    quad, dev, solver = _with_image(n, dup=dup)
    img = dev.hessian_image()
    assert dev.layout()['panel_bytes'] == _elems(n) * 7   # the panel is compact
    assert img['state'] == 'built' and img['bytes'] == _elems(n) * 13 // 2 and img['build_ms'] > 0.0, img
    if dup:
        K = quad.gram()
        off = K[~np.eye(n, dtype=bool)]
        assert (off == 1.0).sum() >= n // 7, 'the escape code is exercised off the diagonal'
    for name, v in _vectors(n, n).items():
        set_hooks(monkeypatch, hessian_image=None)
        got = dev.matvec(v)
        set_hooks(monkeypatch, hessian_image=0)
        want = dev.matvec(v)
        assert np.array_equal(got, want), name
        assert np.abs(want).max() > 0.0
    set_hooks(monkeypatch, hessian_image=None)
    # K alone (no rank-one term) never reads the image: the same call with and without it
    v = _vectors(n, 1)['random']
    a = dev.gram_matvec(v)
    set_hooks(monkeypatch, hessian_image=0)
    assert np.array_equal(a, dev.gram_matvec(v))
    set_hooks(monkeypatch, hessian_image=None)
    solver.close()
    quad.release()


@pytest.mark.parametrize('dup', [False, True], ids=['blobs', 'duplicate_rows'])
@pytest.mark.parametrize('n', [300, 4200])
def test_pad_rows_of_the_product_are_equal(amd, monkeypatch, n, dup):
    """all nb * 256 entries of the product's output on the device, the pad rows past n included, image against panel"""
    set_hooks(monkeypatch, product_rows=1)
    quad, dev, solver = _with_image(n, dup=dup)
    assert dev.hessian_image()['state'] == 'built'
    nb = (n + 255) // 256
    for name, v in _vectors(n, n + 1).items():
        set_hooks(monkeypatch, hessian_image=None)
        dev.matvec(v)
        got = dev.last_product()
        set_hooks(monkeypatch, hessian_image=0)
        dev.matvec(v)
        want = dev.last_product()
        assert got.shape == (nb * 256,) and np.array_equal(got.view(np.uint64), want.view(np.uint64)), name
        if name == 'random':
            assert np.abs(want[n:]).max() > 0.0   # the pad rows of K + 1 are rows of ones: they carry sum(w), not zero
    set_hooks(monkeypatch, hessian_image=None, product_rows=None)
    solver.close()
    quad.release()


def _trajectory(monkeypatch, n, structure, kind, hook):
    from optiml_amd import _lib
    set_hooks(monkeypatch, hessian_image=hook)
    quad = _quad(n, structure)
    dev = quad.device_problem()
    solver = _solver(dev, kind)
    state = dev.hessian_image()['state']
    rows, status = solver.run(30)
    out = (rows.tobytes(), solver.get(_lib.GET_X_NOW).tobytes(), solver.get(_lib.GET_G_NOW).tobytes(), len(rows), status)
    solver.close()
    quad.release()
    set_hooks(monkeypatch, hessian_image=None)
    return state, out


@pytest.mark.parametrize('structure,kind', [('svc', 'PG'), ('svc', 'FW'), ('svr', 'PG')])
@pytest.mark.parametrize('n', SIZES)
def test_trajectories_are_byte_identical(amd, monkeypatch, n, structure, kind):
    from optiml_amd import _lib
    state_off, off = _trajectory(monkeypatch, n, structure, getattr(_lib, kind), 0)
    state_on, on = _trajectory(monkeypatch, n, structure, getattr(_lib, kind), None)
    assert (state_off, state_on) == ('switched_off', 'built')
    assert off[3] == 30 and on[3] == 30
    assert on == off   # every per-step record, x and g


def _share_products(monkeypatch, n, v, G):
    """{(hook, k): share (k, G)'s product}: through the image (hook None) and with the hook off (0), on one problem per share"""
    from optiml_amd import device
    parts = {}
    for k in range(G):
        ctx = device.Context(device=0, share=(k, G))
        quad, dev, solver = _with_image(n, ctx=ctx)
        r0, r1 = dev.dims()[2:]
        want_state = 'built' if r1 > r0 else 'not_eligible'   # a share without a tile row has nothing to convert
        assert dev.hessian_image()['state'] == want_state, (k, G)
        for hook in (None, 0):
            set_hooks(monkeypatch, hessian_image=hook)
            parts[hook, k] = dev.matvec(v)
        set_hooks(monkeypatch, hessian_image=None)
        solver.close()
        quad.release()
        ctx.close()
    return parts


def test_share_context_segment_products(amd, monkeypatch):
    """share (k, G) returns its own canonical segments added in segment order (the segment path of bq_panel_product); a share of G = 8
    is one segment"""
    n = 4200
    v = _vectors(n, 7)['random']
    quad, dev, solver = _with_image(n)
    assert dev.hessian_image()['state'] == 'built'
    want = dev.matvec(v)
    solver.close()
    quad.release()
    seg = _share_products(monkeypatch, n, v, 8)
    acc = np.zeros(n)
    for s in range(8):
        assert np.array_equal(seg[None, s], seg[0, s]), s
        acc = acc + seg[None, s]
    assert np.array_equal(acc, want)   # the eight one-segment shares, added in order, are the one-rank product
    for G in (2, 3):
        parts = _share_products(monkeypatch, n, v, G)
        for k in range(G):
            assert np.array_equal(parts[None, k], parts[0, k]), (G, k)
            own = np.zeros(n)
            for s in range(8 * k // G, 8 * (k + 1) // G):
                own = own + seg[None, s]
            assert np.array_equal(parts[None, k], own), (G, k)


FALLBACKS = [
    ('out_of_domain', {'hessian_image_bad': 1}, {}),
    ('alloc_failed', {'alloc_fail_above': None}, {}),   # threshold filled in below: just under the image's size
    ('no_repay', {}, {'expected': 1}),
    ('no_repay', {}, {'expected': 0}),                  # unknown counts as 0
    ('not_eligible', {}, {'rank_one': False}),
    ('switched_off', {'hessian_image': 0}, {}),
    ('not_faster', {'hessian_image_gain': 1e6}, {}),   # the image's product would have to be a million times faster than the panel's
]


@pytest.mark.parametrize('state,hooks,kw', FALLBACKS, ids=['flag', 'alloc', 'few_products', 'unknown_products', 'no_rank_one', 'hook_off', 'not_faster'])
def test_fallbacks_keep_the_panel_and_say_why(amd, monkeypatch, state, hooks, kw):
    from optiml_amd import _lib
    n = 513
    v = _vectors(n, 3)['random']
    # the reference: the panel's product and trajectory of the same problem, image switched off
    set_hooks(monkeypatch, hessian_image=0)
    ref = _quad(n, **kw)
    want = ref.device_problem().matvec(v)
    s = _solver(ref.device_problem(), _lib.PG)
    want_rows = s.run(10)[0].tobytes()
    s.close()
    ref.release()
    set_hooks(monkeypatch, hessian_image=None)
    if 'alloc_fail_above' in hooks:
        hooks = {'alloc_fail_above': _elems(n) * 13 // 2 - 1}
    set_hooks(monkeypatch, **hooks)
    quad = _quad(n, **kw)
    dev = quad.device_problem()
    assert dev.hessian_image()['state'] == 'none'   # nothing is decided before the first PG / FW solver
    solver = _solver(dev, _lib.PG)
    img = dev.hessian_image()
    assert img['state'] == state and img['bytes'] == 0, img
    assert np.array_equal(dev.matvec(v), want)
    assert solver.run(10)[0].tobytes() == want_rows
    solver.close()
    quad.release()
    set_hooks(monkeypatch, **{k: None for k in hooks})
    set_hooks(monkeypatch, hessian_image_gain=0)


def test_a_failing_allocation_takes_the_image_back(amd, monkeypatch):
    """bq_alloc.cpp: a device allocation that fails gives the images back like the held placement candidates; the product goes on
    from the panel with the same bits"""
    from optiml_amd.opti import Quadratic
    n = 513
    v = _vectors(n, 5)['random']
    quad, dev, solver = _with_image(n)
    assert dev.hessian_image()['state'] == 'built'
    want = dev.matvec(v)
    set_hooks(monkeypatch, alloc_fail_above=1 << 20)
    rs = np.random.RandomState(3)
    G = rs.standard_normal((600, 640))
    dq = Quadratic(G @ G.T / 600, rs.standard_normal(600))   # its 2.9 MB panel "fails" once under the hook: the image is given back
    dq.device_problem()
    set_hooks(monkeypatch, alloc_fail_above=None)
    img = dev.hessian_image()
    assert img['state'] == 'given_back' and img['bytes'] == 0, img
    assert np.array_equal(dev.matvec(v), want)
    dq.release()
    solver.close()
    quad.release()


def test_device_memory_returns_after_the_problem_is_destroyed(amd):
    from optiml_amd.ml.svm._batched import device_free_bytes

    def cycle():
        quad, dev, solver = _with_image(2100)
        assert dev.hessian_image()['state'] == 'built'
        held = device_free_bytes()
        solver.run(3)
        solver.close()
        quad.release()
        return held

    cycle()   # the first problem of a process also creates what the context keeps (events, the library's code objects)
    start = device_free_bytes()
    during = cycle()
    assert during <= start - _elems(2100) * 13 // 2   # panel + image were resident
    assert device_free_bytes() == start
