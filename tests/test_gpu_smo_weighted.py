"""GPU tests of sample_weight / class_weight in SMO: the walkers with one box per row (`bq_smo_create_weighted`,
`bq_msmo_create_weighted`, csrc/bq_smo.hip) and the estimators that reach them.

Bars.  A constant box vector walks the scalar walker's path: equality of bits with `bq_smo_create` / `bq_msmo_create`.  A weighted
single fit is held step for step to tests/smo_weighted_reference.py with the kernel's tie rule and summation order on the device's
own Gram entries (rtol 1e-12, tests/test_gpu_smo.py's bar (1)).  A weighted batched column is the weighted single fit: equality of
bits; a row-list column is held to the reference on the sub-problem.  The estimators are held to sklearn by a derived objective
bound and, on the batched meta-estimator paths, to the per-column weighted `SVC.fit` bit for bit.

Shapes are the goldens' 200 / 600 (classification) and 150 / 400 (regression) rows: a partial 64-row batch, several batches, rows
on both sides of the 256-row tile edge.  The linear-kernel regression duals take tens of thousands of outer iterations under boxes
up to 20, so those cases compare the state after a capped number of outer iterations — still step for step.
"""
import ctypes as C
import math

import numpy as np
import pytest

import scoring_reference as sr
import smo_weighted_reference as wr
from conftest import load_golden

pytestmark = pytest.mark.gpu

TOL = 1e-3
SVC_FIELDS = ('alphas', 'errors', 'b', 'b_up', 'b_low', 'b_up_idx', 'b_low_idx', 'iter', 'steps')
SVR_FIELDS = ('alphas_p', 'alphas_n') + SVC_FIELDS[1:]


@pytest.fixture(scope='module')
def amd():
    import optiml_amd
    from optiml_amd import _lib
    from optiml_amd.device import get_context
    _lib.load()
    get_context()
    return optiml_amd


def _kernel(kname):
    from optiml_amd.ml.svm.kernels import gaussian, linear
    return {'rbf': gaussian, 'linear': linear}[kname]


def _svc_data(n):
    g = load_golden('smo.npz')
    X, y = g[f'svc{n}_X'], g[f'svc{n}_y']
    return X, np.where(y == np.unique(y)[-1], 1., -1.)


def _svr_data(n):
    g = load_golden('smo.npz')
    return g[f'svr{n}_X'], g[f'svr{n}_y']


def _svc_quad(X, yb, kname, **kw):
    from optiml_amd.opti import KernelQuadratic
    return KernelQuadratic(X, -np.ones(len(yb)), 'svc', _kernel(kname), y=yb, rank_one=False, **kw)


def _svr_quad(X, y, kname, **kw):
    from optiml_amd.opti import KernelQuadratic
    return KernelQuadratic(X, np.hstack((-y, y)) + 0.1, 'svr', _kernel(kname), rank_one=False, **kw)


def _folds(n):
    idx = np.arange(n)
    return [(np.setdiff1d(idx, idx[f::3]), idx[f::3]) for f in range(3)]


def _boxes(kind, y, n):
    if kind == 'ratio5':
        return np.where(y == 1, 5., 1.)
    if kind == 'ratio1/5':
        return np.where(y == 1, 0.2, 1.)
    return np.random.RandomState(7).uniform(0.05, 20., n)   # 'random': sample weights in [0.05, 20], C = 1


def _single(quad, task, y, Cw=None, Cv=1., eps=0., tol=TOL, max_outer=None):
    """One single solver through the C ABI (`bq_smo_create_weighted` with Cw, else `bq_smo_create` with Cv) run to its end or for
    max_outer outer iterations: the dict `solve_batched_smo` returns for a column, plus 'finished' and the helper statistics."""
    from optiml_amd import _lib
    lib = _lib.load()
    n = len(y)
    h = C.c_void_p()
    y = np.ascontiguousarray(y, dtype=float)
    if Cw is None:
        _lib.check(lib.bq_smo_create(quad.device_problem().handle, task, _lib.ptr(y), float(Cv), float(eps), float(tol), C.byref(h)))
    else:
        Cw = np.ascontiguousarray(Cw, dtype=float)
        _lib.check(lib.bq_smo_create_weighted(quad.device_problem().handle, task, _lib.ptr(y), _lib.ptr(Cw), float(eps), float(tol),
                                              C.byref(h)))
    outer, fin = C.c_int64(0), C.c_int(0)
    try:
        while not fin.value and (max_outer is None or outer.value < max_outer):
            _lib.check(lib.bq_smo_run(h, 64 if max_outer is None else min(64, max_outer - outer.value), C.byref(outer), C.byref(fin)))
        a = np.empty(n if task == _lib.SVC else 2 * n)
        sc, st, err = np.empty(6), np.empty(4), np.empty(n)
        _lib.check(lib.bq_smo_get(h, _lib.SMO_ALPHAS, _lib.ptr(a)))
        _lib.check(lib.bq_smo_get(h, _lib.SMO_SCALARS, _lib.ptr(sc)))
        _lib.check(lib.bq_smo_get(h, _lib.SMO_STATS, _lib.ptr(st)))
        _lib.check(lib.bq_smo_get(h, _lib.SMO_ERRORS, _lib.ptr(err)))
    finally:
        lib.bq_smo_destroy(h)
    r = dict(b_up=sc[0], b_low=sc[1], b_up_idx=int(sc[2]), b_low_idx=int(sc[3]), steps=int(sc[4]), b=sc[5], iter=int(outer.value),
             errors=err, finished=bool(fin.value), helpers=int(st[0]), rejected=(int(st[2]), int(st[3])))
    if task == _lib.SVC:
        r['alphas'] = a
    else:
        r['alphas_p'], r['alphas_n'] = a[:n].copy(), a[n:].copy()
    return r


def _columns(quad, task, Y, Cs, eps, boxes=None, max_outer=None):
    """`solve_batched_smo`'s per-column dicts; with max_outer, the columns' state after that many launches instead of at their end"""
    from optiml_amd.ml.svm._batched import _DeviceSMOSolver, smo_column_result, solve_batched_smo
    if max_outer is None:
        return solve_batched_smo(quad.device_problem(), task, Y, Cs, eps, TOL, boxes=boxes)
    solver = _DeviceSMOSolver(quad.device_problem(), task, Y, Cs, eps, TOL, None, boxes)
    try:
        outer, _, failed = solver.run(max_outer)
        assert not failed.any()
        return [smo_column_result(solver, c, outer[c]) for c in range(solver.k)]
    finally:
        solver.close()


def _same(a, b, fields, what):
    for f in fields:
        assert np.array_equal(a[f], b[f]), (what, f)


def _follows(r, ref, rows, keys, what):
    """bar (1) of tests/test_gpu_smo.py: counts equal, multipliers / thresholds / error cache at rtol 1e-12"""
    assert r['iter'] == ref['iter'] and r['steps'] == ref['steps'], (what, r['iter'], ref['iter'], r['steps'], ref['steps'])
    for k in keys:
        np.testing.assert_allclose(r[k][rows], ref[k], rtol=1e-12, atol=1e-15, err_msg=str(what))
    np.testing.assert_allclose([r['b'], r['b_up'], r['b_low']], [ref['b'], ref['b_up'], ref['b_low']], rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(r['errors'][rows], ref['errors'], rtol=1e-12, atol=1e-13)


# ---- 6. a constant box vector has the scalar walker's bits --------------------------------------------------------------------------
@pytest.mark.parametrize('full', [False, True], ids=['packed', 'square'])
@pytest.mark.parametrize('kname', ['rbf', 'linear'])
@pytest.mark.parametrize('n', [200, 600])
def test_svc_constant_boxes_have_the_scalar_bits(amd, n, kname, full):
    from optiml_amd import _lib
    from optiml_amd.ml.svm._batched import solve_batched_smo
    X, yb = _svc_data(n)
    quad = _svc_quad(X, yb, kname, full_panel=full)
    Cs = np.array([0.1, 1., 10.])
    Y = np.stack([yb, yb, -yb])
    plain = solve_batched_smo(quad.device_problem(), _lib.SVC, Y, Cs, None, TOL)
    boxed = solve_batched_smo(quad.device_problem(), _lib.SVC, Y, Cs, None, TOL, boxes=Cs[:, None] * np.ones((3, n)))
    for c in range(3):
        _same(boxed[c], plain[c], SVC_FIELDS, ('batched', c))
        one, wone = _single(quad, _lib.SVC, Y[c], Cv=Cs[c]), _single(quad, _lib.SVC, Y[c], Cw=Cs[c] * np.ones(n))
        _same(wone, one, SVC_FIELDS, ('single', c))
        _same(wone, plain[c], SVC_FIELDS, ('single against batched', c))
        assert wone['rejected'] == (0, 0) and one['rejected'] == (0, 0)
    quad.release()


@pytest.mark.parametrize('full', [False, True], ids=['packed', 'square'])
@pytest.mark.parametrize('kname', ['rbf', 'linear'])
@pytest.mark.parametrize('n', [150, 400])
def test_svr_constant_boxes_have_the_scalar_bits(amd, n, kname, full):
    from optiml_amd import _lib
    X, y = _svr_data(n)
    quad = _svr_quad(X, y, kname, full_panel=full)
    Cs, eps = np.array([0.1, 1., 3.]), [0.05, 0.1, 0.]
    Y = np.stack([y, y, -2. * y])
    cap = None if kname == 'rbf' else 192   # the linear duals take thousands of outer iterations: their first 192, three runs of 64
    plain = _columns(quad, _lib.SVR, Y, Cs, eps, max_outer=cap)
    boxed = _columns(quad, _lib.SVR, Y, Cs, eps, boxes=Cs[:, None] * np.ones((3, n)), max_outer=cap)
    for c in range(3):
        _same(boxed[c], plain[c], SVR_FIELDS, ('batched', c))
        one = _single(quad, _lib.SVR, Y[c], Cv=Cs[c], eps=eps[c], max_outer=cap)
        wone = _single(quad, _lib.SVR, Y[c], Cw=Cs[c] * np.ones(n), eps=eps[c], max_outer=cap)
        _same(wone, one, SVR_FIELDS, ('single', c))
        _same(wone, plain[c], SVR_FIELDS, ('single against batched', c))
        assert wone['rejected'] == (0, 0)
    quad.release()


def test_fp32_panel_constant_boxes_have_the_scalar_bits(amd):
    from optiml_amd import _lib
    from optiml_amd.ml.svm._batched import solve_batched_smo
    X, yb = _svc_data(200)
    quad = _svc_quad(X, yb, 'rbf', storage='f32')
    Cs = np.array([0.1, 1., 10.])
    Y = np.stack([yb] * 3)
    plain = solve_batched_smo(quad.device_problem(), _lib.SVC, Y, Cs, None, TOL)
    boxed = solve_batched_smo(quad.device_problem(), _lib.SVC, Y, Cs, None, TOL, boxes=Cs[:, None] * np.ones((3, 200)))
    for c in range(3):
        _same(boxed[c], plain[c], SVC_FIELDS, c)
        _same(_single(quad, _lib.SVC, yb, Cw=Cs[c] * np.ones(200)), _single(quad, _lib.SVC, yb, Cv=Cs[c]), SVC_FIELDS, c)
    X, y = _svr_data(150)
    quad = _svr_quad(X, y, 'rbf', storage='f32')
    _same(_single(quad, _lib.SVR, y, Cw=2. * np.ones(150), eps=0.1), _single(quad, _lib.SVR, y, Cv=2., eps=0.1), SVR_FIELDS, 'svr')


# ---- 7. weighted single fits against the reference, step for step -------------------------------------------------------------------
@pytest.mark.parametrize('boxes', ['ratio5', 'ratio1/5', 'random'])
@pytest.mark.parametrize('n,kname,full', [(200, 'rbf', False), (200, 'linear', True), (600, 'rbf', True), (600, 'linear', False)])
def test_weighted_classifier_follows_the_reference(amd, n, kname, full, boxes):
    from optiml_amd import _lib
    X, yb = _svc_data(n)
    quad = _svc_quad(X, yb, kname, full_panel=full)
    Cw = _boxes(boxes, yb, n)
    r = _single(quad, _lib.SVC, yb, Cw=Cw)
    ref = wr.smo_svc_weighted(quad.gram(), yb, Cw, tol=TOL, tie='index', dot='tree')
    assert r['finished'] and ref['finished'] and r['helpers'] > 0 and r['rejected'] == (0, 0)
    _follows(r, ref, slice(None), ('alphas',), (n, kname, boxes))
    assert (r['alphas'] <= Cw).all() and (r['alphas'] == Cw).any()   # rows at their own box
    quad.release()


@pytest.mark.parametrize('n,kname,full,eps,cap', [(150, 'rbf', False, 0., None), (150, 'rbf', True, 0.1, None),
                                                  (400, 'rbf', True, 0., 60), (400, 'rbf', False, 0.1, None),
                                                  (150, 'linear', True, 0.1, 300), (400, 'linear', False, 0., 60)])
def test_weighted_regression_follows_the_reference(amd, n, kname, full, eps, cap):
    from optiml_amd import _lib
    X, y = _svr_data(n)
    quad = _svr_quad(X, y, kname, full_panel=full)
    Cw = _boxes('random', y, n)
    r = _single(quad, _lib.SVR, y, Cw=Cw, eps=eps, max_outer=cap)
    ref = wr.smo_svr_weighted(quad.gram(), y, Cw, epsilon=eps, tol=TOL, tie='index', dot='tree', max_outer=cap or 10 ** 9)
    assert r['finished'] == ref['finished'] and (cap is not None or r['finished']) and r['rejected'] == (0, 0)
    _follows(r, ref, slice(None), ('alphas_p', 'alphas_n'), (n, kname, eps))
    assert (r['alphas_p'] <= Cw).all() and (r['alphas_n'] <= Cw).all()
    assert (np.maximum(r['alphas_p'], r['alphas_n']) > 1.).any()   # a box above the unweighted one is used
    quad.release()


# ---- 8. a weighted batched column is the weighted single fit --------------------------------------------------------------------------
@pytest.mark.parametrize('chunk', [1, 64])
def test_weighted_columns_equal_weighted_single_fits(amd, chunk):
    from optiml_amd import _lib
    from optiml_amd.ml.svm._batched import solve_batched_smo
    X, yb = _svc_data(200)
    quad = _svc_quad(X, yb, 'rbf')
    W, ones = _boxes('random', yb, 200), np.ones(200)
    wone = _single(quad, _lib.SVC, yb, Cw=W)
    flat = {Cv: _single(quad, _lib.SVC, yb, Cv=Cv) for Cv in (0.1, 1., 10.)}
    assert wone['iter'] != flat[1.]['iter'] or wone['steps'] != flat[1.]['steps']   # another problem than the unweighted one
    for order in ([1., 'w', 10., 'w', 0.1], ['w', 0.1, 1.], [10., 1., 'w']):   # first, last and between; beside constant rows
        boxes = np.stack([W if o == 'w' else o * ones for o in order])
        res = solve_batched_smo(quad.device_problem(), _lib.SVC, np.stack([yb] * len(order)), 1., None, TOL, chunk=chunk, boxes=boxes)
        for o, r in zip(order, res):
            _same(r, wone if o == 'w' else flat[o], SVC_FIELDS, (order, o))
    quad.release()
    X, y = _svr_data(150)
    quad = _svr_quad(X, y, 'rbf')
    W, ones = _boxes('random', y, 150), np.ones(150)
    wone, one = _single(quad, _lib.SVR, y, Cw=W, eps=0.1), _single(quad, _lib.SVR, y, Cv=1., eps=0.05)
    res = solve_batched_smo(quad.device_problem(), _lib.SVR, np.stack([y] * 3), 1., [0.05, 0.1, 0.05], TOL, chunk=chunk,
                            boxes=np.stack([ones, W, ones]))
    _same(res[0], one, SVR_FIELDS, 0)
    _same(res[1], wone, SVR_FIELDS, 1)
    _same(res[2], one, SVR_FIELDS, 2)
    quad.release()


def test_weighted_row_list_columns_follow_the_reference_and_read_no_box_outside_their_list(amd):
    from optiml_amd import _lib
    from optiml_amd.ml.svm._batched import solve_batched_smo
    X, yb = _svc_data(600)
    quad = _svc_quad(X, yb, 'rbf')
    Kdev = quad.gram()
    folds = _folds(600)
    kinds = ['ratio5', 'random', 'ratio1/5']
    boxes = np.full((3, 600), np.nan)   # NaN on the rows outside a column's list: they are not read
    for f, (tr, _) in enumerate(folds):
        boxes[f, tr] = _boxes(kinds[f], yb, 600)[tr]
    res = solve_batched_smo(quad.device_problem(), _lib.SVC, np.stack([yb] * 3), 1., None, TOL, rows=[tr for tr, _ in folds],
                            boxes=boxes)
    for f, (tr, te) in enumerate(folds):
        ref = wr.smo_svc_weighted(Kdev[tr][:, tr], yb[tr], boxes[f, tr], tol=TOL, tie='index', dot='tree')
        _follows(res[f], ref, tr, ('alphas',), ('svc fold', f))
        assert not res[f]['alphas'][te].any() and np.isfinite(res[f]['alphas']).all() and np.isfinite(res[f]['b'])
    quad.release()
    X, y = _svr_data(400)
    quad = _svr_quad(X, y, 'rbf')
    Kdev = quad.gram()
    folds = _folds(400)
    boxes = np.full((3, 400), np.nan)
    for f, (tr, _) in enumerate(folds):
        boxes[f, tr] = np.random.RandomState(f).uniform(0.05, 20., 400)[tr]
    res = solve_batched_smo(quad.device_problem(), _lib.SVR, np.stack([y] * 3), 1., [0.1] * 3, TOL, rows=[tr for tr, _ in folds],
                            boxes=boxes)
    for f, (tr, te) in enumerate(folds):
        ref = wr.smo_svr_weighted(Kdev[tr][:, tr], y[tr], boxes[f, tr], epsilon=0.1, tol=TOL, tie='index', dot='tree')
        _follows(res[f], ref, tr, ('alphas_p', 'alphas_n'), ('svr fold', f))
        assert not res[f]['alphas_p'][te].any() and not res[f]['alphas_n'][te].any()
    quad.release()


def test_boxes_are_checked_before_any_device_call(amd):
    from optiml_amd import _lib
    lib = _lib.load()
    X, yb = _svc_data(200)
    quad = _svc_quad(X, yb, 'rbf')
    dev = quad.device_problem()
    h = C.c_void_p()
    i64, i32 = C.POINTER(C.c_int64), C.POINTER(C.c_int32)
    for bad in (0., -1., float('nan'), float('inf')):
        Cw = np.ones(200)
        Cw[137] = bad
        assert lib.bq_smo_create_weighted(dev.handle, _lib.SVC, _lib.ptr(yb), _lib.ptr(Cw), 0., TOL, C.byref(h)) == _lib.ERR_BADARG
        assert b'box' in lib.bq_last_error() and not h.value
        CW = np.ones((2, 200))
        CW[1, 137] = bad
        Y = np.ascontiguousarray(np.stack([yb, yb]))
        assert lib.bq_msmo_create_weighted(dev.handle, _lib.SVC, 2, _lib.ptr(Y), _lib.ptr(CW), None, TOL, None, None,
                                           C.byref(h)) == _lib.ERR_BADARG
        assert b'box' in lib.bq_last_error() and not h.value
        # ... on a row outside the column's list the same entry is not looked at
        rows = np.delete(np.arange(200, dtype=np.int32), 137)
        row_ptr = np.array([0, 199, 398], dtype=np.int64)
        flat = np.ascontiguousarray(np.concatenate([rows, rows]))
        assert lib.bq_msmo_create_weighted(dev.handle, _lib.SVC, 2, _lib.ptr(Y), _lib.ptr(CW), None, TOL, row_ptr.ctypes.data_as(i64),
                                           flat.ctypes.data_as(i32), C.byref(h)) == _lib.OK
        lib.bq_msmo_destroy(h)
        h = C.c_void_p()
    Cw = np.ones(200)
    assert lib.bq_smo_create_weighted(dev.handle, _lib.SVC, _lib.ptr(yb), None, 0., TOL, C.byref(h)) == _lib.ERR_BADARG
    assert lib.bq_smo_create_weighted(dev.handle, _lib.SVC, _lib.ptr(yb), _lib.ptr(Cw), 0., 0., C.byref(h)) == _lib.ERR_BADARG
    assert lib.bq_smo_create_weighted(dev.handle, _lib.SVR, _lib.ptr(yb), _lib.ptr(Cw), -1., TOL, C.byref(h)) == _lib.ERR_BADARG
    assert lib.bq_smo_create_weighted(dev.handle, 7, _lib.ptr(yb), _lib.ptr(Cw), 0., TOL, C.byref(h)) == _lib.ERR_BADARG
    assert not h.value
    plain_bytes = dev.layout()['panel_bytes']
    quad.release()
    # the 7-byte panel (a small gamma keeps every entry in [2^-14, 1]) has no row-box walker: refused, not mis-read
    from optiml_amd.ml.svm.kernels import GaussianKernel
    from optiml_amd.opti import KernelQuadratic
    cq = KernelQuadratic(X, -np.ones(200), 'svc', GaussianKernel(gamma=0.01), y=yb, rank_one=False, compact=True)
    cdev = cq.device_problem()
    assert cdev.layout()['panel_bytes'] < plain_bytes
    assert lib.bq_smo_create_weighted(cdev.handle, _lib.SVC, _lib.ptr(yb), _lib.ptr(Cw), 0., TOL, C.byref(h)) == _lib.ERR_BADARG
    assert b'panel' in lib.bq_last_error() and not h.value
    Y = np.ascontiguousarray(np.stack([yb, yb]))
    assert lib.bq_msmo_create_weighted(cdev.handle, _lib.SVC, 2, _lib.ptr(Y), _lib.ptr(np.ones((2, 200))), None, TOL, None, None,
                                       C.byref(h)) == _lib.ERR_BADARG
    assert b'panel' in lib.bq_last_error() and not h.value
    cq.release()


# ---- 9. the held-out scorers on a weighted solver -----------------------------------------------------------------------------------
def test_heldout_scorers_read_a_weighted_solver(amd):
    from optiml_amd import _lib
    from optiml_amd.ml.svm._batched import _DeviceSMOSolver, _gram_matmat, run_batched_smo
    from optiml_amd.ml.svm.kernels import GaussianKernel
    from optiml_amd.opti import KernelQuadratic
    n = 400
    X, y = _svr_data(n)
    folds = _folds(n)
    held = np.zeros((3, n), dtype=np.uint8)
    for f, (_, te) in enumerate(folds):
        held[f, te] = 1
    rows = [tr for tr, _ in folds]
    boxes = np.stack([np.random.RandomState(f).uniform(0.05, 20., n) for f in range(3)])
    quad = KernelQuadratic(X, np.hstack((-y, y)) + 0.1, 'svr', GaussianKernel(gamma=0.1), rank_one=False, compact=False)
    dev = quad.device_problem()
    solver = _DeviceSMOSolver(dev, _lib.SVR, np.stack([y] * 3), 1., [0.1] * 3, TOL, rows, boxes)
    try:
        _, failed = run_batched_smo(solver)
        assert not failed.any()
        b, n_sv, sse, n_held = solver.svr_heldout([0, 1, 2], held)
        W = np.zeros((3, n))
        for c in range(3):
            a, sc = solver.get(c, _lib.SMO_ALPHAS), solver.get(c, _lib.SMO_SCALARS)
            sv = (a[:n] > 1e-6) | (a[n:] > 1e-6)
            W[c][sv] = a[:n][sv] - a[n:][sv]
            assert b[c] == sc[5] and n_sv[c] == sv.sum() and n_held[c] == len(folds[c][1]), c
            assert (np.maximum(a[:n], a[n:]) > 1.).any()   # the weights took effect
        U = _gram_matmat(dev, W, wide=True)
        for c, (_, te) in enumerate(folds):
            ref = math.fsum(float(t) for t in (y[te] - (U[c][te] + b[c])) ** 2)
            sr.check_sse('weighted svr column %d' % c, float(sse[c]), ref, len(te))
    finally:
        solver.close()
        quad.release()
    n = 600
    X, yb = _svc_data(n)
    folds = _folds(n)
    held = np.zeros((3, n), dtype=np.uint8)
    for f, (_, te) in enumerate(folds):
        held[f, te] = 1
    boxes = np.stack([_boxes(kind, yb, n) for kind in ('ratio5', 'random', 'ratio1/5')])
    quad = KernelQuadratic(X, -np.ones(n), 'svc', GaussianKernel(gamma=0.1), y=yb, rank_one=False, compact=False)
    dev = quad.device_problem()
    solver = _DeviceSMOSolver(dev, _lib.SVC, np.stack([yb] * 3), 1., None, TOL, [tr for tr, _ in folds], boxes)
    try:
        _, failed = run_batched_smo(solver)
        assert not failed.any()
        b, n_sv, fit = solver.svc_heldout([0, 1, 2], held, [0, 1, 2], 3, decisions=True)
        W = np.zeros((3, n))
        for c in range(3):
            a, sc = solver.get(c, _lib.SMO_ALPHAS), solver.get(c, _lib.SMO_SCALARS)
            W[c][a > 1e-6] = (a * yb)[a > 1e-6]
            assert b[c] == sc[5] and n_sv[c] == (a > 1e-6).sum(), c
        U = _gram_matmat(dev, W, wide=True)
        dec = np.zeros((3, n))
        for c, (_, te) in enumerate(folds):
            dec[c][te] = U[c][te] + b[c]
        assert np.array_equal(fit['dec'], dec)   # u + b on the scored rows, 0 elsewhere
        for c, (_, te) in enumerate(folds):
            assert int(fit['n_pos'][c]) == (yb[te] == 1).sum() and int(fit['n_neg'][c]) == (yb[te] == -1).sum()
    finally:
        solver.close()
        quad.release()


# ---- 10. estimators -------------------------------------------------------------------------------------------------------------------
GAMMA = 0.5


@pytest.fixture(scope='module')
def blobs():
    """imbalanced two-class blobs: n = 300, 10 % positives, overlapping"""
    rs = np.random.RandomState(4)
    y = np.zeros(300, dtype=int)
    y[rs.permutation(300)[:30]] = 1
    X = rs.standard_normal((300, 4)) + 1.2 * y[:, None]
    return np.ascontiguousarray(X), y


def _smo_svc(**kw):
    from optiml_amd.ml.svm import SVC
    from optiml_amd.ml.svm.kernels import GaussianKernel
    from optiml_amd.ml.svm.losses import hinge
    return SVC(loss=hinge, kernel=GaussianKernel(gamma=GAMMA), C=1., dual=True, optimizer='smo', tol=TOL, **kw)


def _objective(K, yb, a):
    c = a * yb
    return 0.5 * c @ K @ c - a.sum()


@pytest.mark.parametrize('case', ['balanced', 'dict and sample_weight'])
def test_weighted_svc_is_sklearns_weighted_svc_within_the_derived_bound(amd, blobs, case):
    from sklearn.metrics.pairwise import rbf_kernel
    from sklearn.svm import SVC as SkSVC
    from sklearn.utils.class_weight import compute_class_weight
    X, y = blobs
    yb = np.where(y == 1, 1., -1.)
    cw, sw = ('balanced', None) if case == 'balanced' else ({1: 6., 0: 0.8}, np.random.RandomState(2).uniform(0.2, 3., 300))
    est = _smo_svc(class_weight=cw).fit(X, y, sample_weight=sw)
    plain = _smo_svc().fit(X, y)
    box = compute_class_weight(cw, classes=np.array([0, 1]), y=y)[y] * (1. if sw is None else sw)
    assert (est.alphas_ <= box * (1 + 1e-15)).all() and (est.alphas_ > 1.).any() and abs(est.alphas_ @ yb) < 1e-9
    sk = SkSVC(kernel='rbf', gamma=GAMMA, C=1., class_weight=cw, tol=1e-8).fit(X, y, sample_weight=sw)
    a_sk = np.zeros(300)
    a_sk[sk.support_] = np.abs(sk.dual_coef_[0])
    K = rbf_kernel(X, X, gamma=GAMMA)
    f, f_sk = _objective(K, yb, est.alphas_), _objective(K, yb, a_sk)
    print(case, 'objective', f, 'sklearn', f_sk, 'slack', 2 * TOL * box.sum())
    # derived (tests/test_smo_weighted_host.py): a point whose violation is <= 2 tol has f - f* <= 2 tol sum_i C_i
    assert f <= f_sk + 2 * TOL * box.sum()
    recall = lambda e: float(np.mean(e.predict(X[y == 1]) == 1))   # noqa: E731
    print(case, 'minority recall', recall(est), 'unweighted', recall(plain))
    assert recall(est) >= recall(plain)
    assert est.optimizer.helper_stats['rejected_list_hash'] == 0 and est.optimizer.helper_stats['rejected_checksum'] == 0


def test_box_solvers_take_the_row_boxes_as_their_upper_bounds(amd, blobs):
    from optiml_amd.ml.svm import SVC, SVR
    from optiml_amd.ml.svm._base import row_boxes
    from optiml_amd.ml.svm.kernels import GaussianKernel
    from optiml_amd.ml.svm.losses import hinge, epsilon_insensitive
    from optiml_amd.opti import KernelQuadratic
    from optiml_amd.opti.constrained import FrankWolfe, ProjectedGradient
    X, y = blobs
    yb = np.where(y == 1, 1., -1.)
    sw = np.random.RandomState(5).uniform(0.2, 3., 300)
    kw = dict(loss=hinge, kernel=GaussianKernel(gamma=GAMMA), C=2., dual=True, reg_intercept=True, optimizer=ProjectedGradient,
              max_iter=200)
    est = SVC(class_weight={1: 4.}, **kw).fit(X, y, sample_weight=sw)
    box = row_boxes(2., y, np.array([0, 1]), {1: 4.}, sw)
    assert np.array_equal(box, 2. * sw * np.where(y == 1, 4., 1.))
    hand = SVC(**kw)   # the same optimizer on ub = C_i built by hand
    hand._run(KernelQuadratic(X, -np.ones(300), 'svc', hand.kernel, y=yb, storage=hand.storage, tune_placement=hand._streams_panel(),
                              expected_products=hand.max_iter), box)
    assert np.array_equal(est.alphas_, hand.alphas_) and (est.alphas_ > 2.).any() and (est.alphas_ <= box).all()
    assert est.optimizer.iter == hand.optimizer.iter and est.optimizer.f_x == hand.optimizer.f_x
    t = X[:, 0] + 0.3 * np.sin(3 * X[:, 1])
    kw = dict(loss=epsilon_insensitive, epsilon=0.1, kernel=GaussianKernel(gamma=GAMMA), C=2., dual=True, reg_intercept=True,
              optimizer=FrankWolfe, max_iter=200)
    reg = SVR(**kw).fit(X, t, sample_weight=sw)
    hand = SVR(**kw)
    hand._run(KernelQuadratic(X, np.hstack((-t, t)) + 0.1, 'svr', hand.kernel, storage=hand.storage,
                              tune_placement=hand._streams_panel(), expected_products=hand.max_iter), np.hstack((2. * sw, 2. * sw)))
    assert np.array_equal(reg.alphas_, hand.alphas_) and reg.optimizer.iter == hand.optimizer.iter
    assert (reg.alphas_ <= np.hstack((2. * sw, 2. * sw))).all()


def test_zero_weight_rows_are_dropped_and_squared_losses_refuse_weights(amd, blobs):
    from optiml_amd.ml.svm import SVC, SVR
    from optiml_amd.ml.svm.kernels import GaussianKernel
    from optiml_amd.ml.svm.losses import squared_hinge, epsilon_insensitive, squared_epsilon_insensitive
    from optiml_amd.opti.unconstrained.stochastic import Adam
    X, y = blobs
    sw = np.random.RandomState(6).uniform(0.2, 3., 300)
    sw[::4] = 0.
    keep = np.flatnonzero(sw > 0)
    est = _smo_svc(class_weight={1: 3.}).fit(X, y, sample_weight=sw)
    rest = _smo_svc(class_weight={1: 3.}).fit(X[keep], y[keep], sample_weight=sw[keep])
    assert est.alphas_.shape == (300,) and np.array_equal(est.alphas_[keep], rest.alphas_) and not est.alphas_[::4].any()
    assert np.array_equal(est.support_, keep[rest.support_]) and est.intercept_ == rest.intercept_
    assert np.array_equal(est.support_vectors_, rest.support_vectors_) and np.array_equal(est.dual_coef_, rest.dual_coef_)
    assert np.array_equal(est.predict(X), rest.predict(X))
    t = X[:, 0] + 0.3 * np.sin(3 * X[:, 1])
    kw = dict(loss=epsilon_insensitive, epsilon=0.1, kernel=GaussianKernel(gamma=GAMMA), C=1., dual=True, optimizer='smo', tol=TOL)
    reg, rreg = SVR(**kw).fit(X, t, sample_weight=sw), SVR(**kw).fit(X[keep], t[keep], sample_weight=sw[keep])
    assert np.array_equal(reg.alphas_[np.concatenate((keep, 300 + keep))], rreg.alphas_) and not reg.alphas_[:300][::4].any()
    assert np.array_equal(reg.support_, keep[rreg.support_]) and reg.intercept_ == rreg.intercept_
    sq = dict(kernel=GaussianKernel(gamma=GAMMA), dual=True, optimizer=Adam, learning_rate=0.01, max_iter=5)
    with pytest.raises(NotImplementedError, match='squared hinge'):
        SVC(loss=squared_hinge, class_weight='balanced', **sq).fit(X, y)
    with pytest.raises(NotImplementedError, match='squared hinge'):
        SVC(loss=squared_hinge, **sq).fit(X, y, sample_weight=sw)
    with pytest.raises(NotImplementedError, match='squared epsilon-insensitive'):
        SVR(loss=squared_epsilon_insensitive, **sq).fit(X, t, sample_weight=sw)


# ---- 11. the batched meta-estimators ------------------------------------------------------------------------------------------------
def _same_estimator(a, b, what):
    for f in SVC_FIELDS:
        assert np.array_equal(getattr(a.optimizer, f), getattr(b.optimizer, f)), (what, f)
    assert np.array_equal(a.optimizer.box, b.optimizer.box), what
    assert np.array_equal(a.alphas_, b.alphas_) and a.intercept_ == b.intercept_, what
    assert np.array_equal(a.support_, b.support_) and np.array_equal(a.dual_coef_, b.dual_coef_), what
    assert np.array_equal(a.support_vectors_, b.support_vectors_), what


def test_one_vs_rest_balanced_equals_one_weighted_svc_per_class(amd):
    from optiml_amd.datasets import make_multiclass_blobs
    from optiml_amd.ml.svm import SVC, OneVsRestSVC
    from optiml_amd.ml.svm.kernels import GaussianKernel
    from optiml_amd.ml.svm.losses import hinge
    X, y = make_multiclass_blobs(400, 6, 5, seed=5)
    kw = dict(loss=hinge, kernel=GaussianKernel(gamma=0.2), C=1., dual=True, optimizer='smo', tol=TOL, class_weight='balanced')
    est = OneVsRestSVC(**kw).fit(X, y)   # five classes: the default dispatch takes the batched solve
    assert est.batched_ is True and est.smo_ is True and len(est.estimators_) == 5
    flat = OneVsRestSVC(**dict(kw, class_weight=None)).fit(X, y)
    for c, e in enumerate(est.estimators_):
        one = SVC(**kw).fit(X, (y == est.classes_[c]).astype(int))
        _same_estimator(e, one, c)
        assert e.class_weight == 'balanced' and (e.alphas_ > 1.).any()   # 1 : 4 problems: the minority's box is 2.5
        assert not np.array_equal(e.alphas_, flat.estimators_[c].alphas_)
    assert est.score(X, y) > 0.5


@pytest.mark.parametrize('cw', ['balanced', {0: 2., 3: 0.5}], ids=['balanced', 'dict'])
def test_one_vs_one_weighted_equals_one_weighted_svc_per_pair(amd, cw):
    """n = 240: one tile row, where a pair's own Gram build has the shared panel's bits (tests/test_gpu_ovo_smo.py)"""
    from optiml_amd.datasets import make_multiclass_blobs
    from optiml_amd.ml.svm import SVC, OneVsOneSVC
    from optiml_amd.ml.svm.kernels import GaussianKernel
    from optiml_amd.ml.svm.losses import hinge
    from optiml_amd.ml.svm.onevsone import ovo_pairs, pair_problem
    X, y = make_multiclass_blobs(240, 5, 4, seed=3)
    y = np.where(np.arange(240) % 5 == 0, 0, y)   # unequal classes, so that 'balanced' is not the unweighted fit
    kw = dict(loss=hinge, kernel=GaussianKernel(gamma=0.2), C=1., dual=True, optimizer='smo', tol=TOL)
    est = OneVsOneSVC(class_weight=cw, **kw).fit(X, y)   # six pairs: the default dispatch takes the batched solve
    assert est.batched_ is True and est.smo_ is True and len(est.estimators_) == 6
    for q, (i, j) in enumerate(ovo_pairs(4)):
        rows, yp = pair_problem(y, i, j)
        pair_cw = cw if cw == 'balanced' else {0: cw.get(i, 1.), 1: cw.get(j, 1.)}
        one = SVC(class_weight=pair_cw, **kw).fit(X[rows], (yp > 0).astype(int))
        _same_estimator(est.estimators_[q], one, (i, j))
        assert est.estimators_[q].class_weight == pair_cw
    loop = OneVsOneSVC(class_weight=cw, **kw)
    loop.batch_smo = False
    loop.fit(X, y)
    assert loop.batched_ is False
    for q in range(6):
        _same_estimator(est.estimators_[q], loop.estimators_[q], q)


def test_grid_search_over_a_class_weighted_estimator_runs_per_fold(amd, blobs):
    from sklearn.model_selection import GridSearchCV
    from optiml_amd.ml.svm import SVCGridSearchCV
    X, y = blobs
    folds = [(tr, te) for tr, te in _folds(300)]
    est = _smo_svc(class_weight='balanced')
    search = SVCGridSearchCV(est, {'C': [0.5, 2.]}, cv=folds, refit=False).fit(X, y)
    assert search.batched_ is False and search.smo_ is False
    sk = GridSearchCV(_smo_svc(class_weight='balanced'), {'C': [0.5, 2.]}, cv=folds, refit=False).fit(X, y)
    for f in range(3):
        assert np.array_equal(search.cv_results_['split%d_test_score' % f], sk.cv_results_['split%d_test_score' % f])
    flat = SVCGridSearchCV(_smo_svc(), {'C': [0.5, 2.]}, cv=folds, refit=False).fit(X, y)
    assert any(not np.array_equal(search.cv_results_['split%d_test_score' % f], flat.cv_results_['split%d_test_score' % f])
               for f in range(3))   # the weights reached the fold fits
