"""Working-set decomposition in the row-based SMO (bq_rsmo_set_working_set, csrc/bq_rsmo_ws.h) on the device.

The reference of a case is the dual's optimum: tests/smo_rows_reference.py::solve at tol 1e-10 on the Gram matrix of
tests/gram_reference.py (exact arguments, the map in long double).  The mode promises that optimum within tol, not a trajectory.

1. optimum    {SVC rbf, SVC poly 3, SVR rbf (N = 2n), SVC with per-row boxes} x (n, d, q) in {(50, 3, 128): n < q, W is everything;
              (130, 37, 16): many outer iterations, both lists short of candidates near the end, the 128-row tile edge;
              (257, 16, 128): a ragged third tile; (600, 5, 64): five lists to merge}, tol 1e-3: alpha in its box exactly, the
              equality within 4 u N max C, and four deviations — libsvm's violation on a long-double gradient recomputed from the
              returned alpha, the objective above the optimum, rho, the returned gradient against the long-double one — each within
              8 x what the two-variable mode (working_set=False) shows on the same case (its sums are fma chains, these are MFMA
              tiles).  The violation's deviation is its distance from the solver's own Gmax + Gmax2.
2. bits       two runs, and a run enqueued one outer iteration per call, end with the same bits in alpha and G.
3. counts     outer >= 2 at q = 16; outer == 1 at n < q with tol 0.25: the inner rule stops at max(tol, 0.1 x the gap at entry),
              the gap at entry is 2 (alpha = 0, G = -1), so at tol 1e-3 the first outer iteration ends at 0.2 and more follow;
              inner >= outer; no kernel row was asked of the cache.
   tree       svc_rbf at n = 2100, q = 16 is held to the same bounds: 17 workgroups, so the merge tree has two levels.
4. rows       bq_rsmo_rows on a finished working-set solver: every row against the exact-argument reference, each one a miss.
5. refusals   BQ_ERR_BADARG for Solver_NU's rule, q odd / 0 / 130, shrinking with a working set in either order, a call after the
              first run; ValueError from RowNuSVC / RowNuSVR(working_set=True); SVC(optimizer='smo', storage='stream') predicts the same labels
              with and without `working_set = True`."""
import ctypes as C
import functools

import numpy as np
import pytest

import gram_reference as gr
import smo_rows_reference as ref
from test_gpu_smo_rows import Solver, _kernel, amd  # noqa: F401 (the fixture: library loaded, long double checked)

pytestmark = pytest.mark.gpu

TOL = 1e-3
DUALS = ('svc_rbf', 'svc_poly3', 'svr_rbf', 'svc_boxes')
SHAPES = ((50, 3, 128), (130, 37, 16), (257, 16, 128), (600, 5, 64))


@functools.lru_cache(maxsize=None)
def _problem(dual, n, d):
    """(kernel spec, X, y, boxes, signs, p, C, K in long double, the optimum)"""
    name = 'poly' if dual == 'svc_poly3' else 'rbf'
    sp, X, _, K = gr.exact_reference(gr.Case('ws', name, 3, n, None, d, 4000 + n, 0))
    rs = np.random.RandomState(n)
    noise = rs.standard_normal(n)
    boxes = 0.5 + rs.uniform(size=n) if dual == 'svc_boxes' else np.ones(n)
    if dual == 'svr_rbf':
        y = np.sin(X[:, 0]) + 0.1 * noise
        signs, p, Cfull = ref.svr_problem(y, boxes, ref.EPSILON)
    else:
        y = np.where(X[:, 0] * X[:, 1] + 0.3 * noise > 0, 1.0, -1.0)
        signs, p, Cfull = ref.svc_problem(y, boxes)
    best = ref.solve(K.astype(float), signs, p, Cfull, 1e-10)
    assert best.status == 'optimal'
    return gr.frozen(X, y, boxes, signs, p, Cfull, K) + (sp, best)


def _run(dual, n, d, working_set, tol=TOL, run_steps=None):
    from optiml_amd.ml.svm.smo_rows import RowSMOClassifier, RowSMORegression
    from optiml_amd.opti import KernelQuadratic
    X, y, boxes, signs, p, Cfull, K, sp, best = _problem(dual, n, d)
    kernel = _kernel(sp)
    quad = KernelQuadratic(X, np.zeros(n), 'plain', kernel, storage='stream')
    try:
        if dual == 'svr_rbf':
            opt = RowSMORegression(quad, X, y, None, kernel, 1.0, ref.EPSILON, tol, box=boxes, working_set=working_set)
        else:
            opt = RowSMOClassifier(quad, X, y, None, kernel, 1.0, tol, box=boxes, working_set=working_set)
        if run_steps:
            opt.run_steps = run_steps
        opt.minimize()
    finally:
        quad.release()
    assert opt.status == 'optimal'
    return opt


@functools.lru_cache(maxsize=None)
def _deviations(dual, n, d, working_set):
    """(the finished solver, alpha, [violation's, objective's, rho's, gradient's deviation], the violation in long double)"""
    X, y, boxes, signs, p, Cfull, K, sp, best = _problem(dual, n, d)
    opt = _run(dual, n, d, working_set)
    alpha, rep = opt._all_alphas(), len(signs) // n
    b = (signs * alpha).astype(gr.LD).reshape(rep, n).sum(axis=0)
    G = p.astype(gr.LD) + signs * np.tile(K @ b, rep)
    up, low = np.where(signs > 0, alpha < Cfull, alpha > 0), np.where(signs > 0, alpha > 0, alpha < Cfull)
    violation = np.where(signs > 0, -G, G)[up].max() + np.where(signs > 0, G, -G)[low].max()
    objective = 0.5 * (alpha.astype(gr.LD) @ (G + p))
    dev = [abs(violation - (opt.gmax + opt.gmax2)), objective - best.objective, abs(opt.rho - best.rho), np.abs(opt.gradient - G).max()]
    return opt, alpha, [float(v) for v in dev], float(violation)


TREE = ('svc_rbf', 2100, 8, 16)   # 17 workgroups: two levels of the merge tree, lists cut to q = 16


@pytest.mark.parametrize('dual,n,d,q', [(dual,) + shape for dual in DUALS for shape in SHAPES] + [TREE])
def test_optimum_and_kkt(amd, dual, n, d, q):
    X, y, boxes, signs, p, Cfull, K, sp, best = _problem(dual, n, d)
    _, _, base, _ = _deviations(dual, n, d, False)
    opt, alpha, dev, violation = _deviations(dual, n, d, q)
    print(f'{dual} n={n} d={d} q={q}: {opt.ws_stats}, violation {violation:.3e}; deviations (violation, objective, rho, gradient) '
          f'two-variable {base[0]:.2e} {base[1]:.2e} {base[2]:.2e} {base[3]:.2e}  working set {dev[0]:.2e} {dev[1]:.2e} {dev[2]:.2e} {dev[3]:.2e}')
    assert (alpha >= 0).all() and (alpha <= Cfull).all()
    assert abs((signs * alpha).astype(gr.LD).sum()) <= 4 * float(gr.U) * len(signs) * Cfull.max()
    assert violation < TOL + 8 * base[0]
    assert dev[1] <= 8 * base[1] and dev[2] <= 8 * base[2] and dev[3] <= 8 * base[3]


def test_same_bits_on_every_run_and_cut(amd):
    runs = [_run('svc_rbf', 130, 37, 16), _run('svc_rbf', 130, 37, 16), _run('svc_rbf', 130, 37, 16, run_steps=1)]
    assert runs[0].ws_stats['outer'] >= 2
    for other in runs[1:]:
        assert other.alphas.tobytes() == runs[0].alphas.tobytes() and other.gradient.tobytes() == runs[0].gradient.tobytes()
        assert other.ws_stats == runs[0].ws_stats


def test_counts(amd):
    many, _, _, _ = _deviations('svc_rbf', 130, 37, 16)
    once = _run('svc_rbf', 50, 3, 128, tol=0.25)
    print(many.ws_stats, once.ws_stats)
    assert many.ws_stats['working_set'] == 16 and many.ws_stats['outer'] >= 2 and many.iter == many.ws_stats['outer']
    assert once.ws_stats['outer'] == 1
    for opt in (many, once):
        assert opt.ws_stats['inner'] >= opt.ws_stats['outer']
        assert opt.cache_stats['misses'] == 0 and opt.cache_stats['hits'] == 0


def test_rows_of_a_finished_working_set_solver(amd):
    X, y, boxes, signs, p, Cfull, K, sp, best = _problem('svc_rbf', 130, 37)
    with Solver(X, _kernel(sp), 'svc', y, boxes) as s:
        s._lib.check(s.lib.bq_rsmo_set_working_set(s.h, 16))
        assert s.finish()[1] == 1
        rows, st = s.rows(np.arange(len(y))), s.stats()
    gr.check_exact('rows after a working-set run', 'rbf', rows, K)
    assert (st['hits'], st['misses']) == (0, len(y))   # the row the first selection asked for is made like any other


def test_refusals_and_the_public_route(amd):
    from optiml_amd import _lib
    from optiml_amd.ml.svm import SVC, RowNuSVC, RowNuSVR, kernels as kk, losses
    lib = _lib.load()

    def refused(call):
        with pytest.raises(_lib.BcqpError) as err:
            _lib.check(call())
        return err.value.code == _lib.ERR_BADARG

    X, y, boxes, signs, p, Cfull, K, sp, best = _problem('svc_rbf', 130, 37)
    n = len(y)
    with Solver(X, _kernel(sp), 'svc', y, boxes) as s:
        for q in (0, 15, 130):
            assert refused(lambda: lib.bq_rsmo_set_working_set(s.h, q))
        assert refused(lambda: lib.bq_rsmo_get(s.h, _lib.RSMO_WS_STATS, _lib.ptr(np.empty(3))))
        _lib.check(lib.bq_rsmo_set_working_set(s.h, 16))
        assert refused(lambda: lib.bq_rsmo_set_working_set(s.h, 16))
        assert refused(lambda: lib.bq_rsmo_set_shrinking(s.h, 20))
        h = C.c_void_p()
        _lib.check(lib.bq_rsmo_create_general(s.quad.device_problem().handle, _lib.RSMO_RULE_NU, n, _lib.ptr(signs), _lib.ptr(np.zeros(n)),
                                              _lib.ptr(np.ones(n)), _lib.ptr(np.full(n, 0.25)), TOL, 0, 0, C.byref(h)))
        try:
            assert refused(lambda: lib.bq_rsmo_set_working_set(h, 16))
        finally:
            lib.bq_rsmo_destroy(h)
    with Solver(X, _kernel(sp), 'svc', y, boxes) as s:
        _lib.check(lib.bq_rsmo_set_shrinking(s.h, 20))
        assert refused(lambda: lib.bq_rsmo_set_working_set(s.h, 16))
    with Solver(X, _kernel(sp), 'svc', y, boxes) as s:
        s.run(1)
        assert refused(lambda: lib.bq_rsmo_set_working_set(s.h, 16))
    for refuses in (RowNuSVC, RowNuSVR):
        with pytest.raises(ValueError):
            refuses(working_set=True)
    fits = []
    for working_set in (False, True):
        est = SVC(loss=losses.hinge, kernel=kk.GaussianKernel(sp[1]), C=1.0, dual=True, optimizer='smo', storage='stream', tol=TOL)
        est.working_set = working_set
        fits.append(est.fit(X, y))
    assert fits[1].optimizer.ws_stats['working_set'] == 128 and fits[0].optimizer.ws_stats is None
    assert (fits[0].predict(X) == fits[1].predict(X)).all()
