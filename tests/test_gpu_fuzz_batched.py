"""Differential run of the batched solvers on seeded draws (tests/batched_fuzz_reference.py): the label columns on the 4- and
16-column products, one box per column, SVR columns, pair columns on the class-sorted panel and the four simplex layouts
(bq_msolver.hip, bq_simplex.hip, bq_symm.hip, bq_symmw.hip, bq_symmp.hip), with n at the tile and strip edges, k at the chunk
edges, held-out masks, start points, columns that leave mid-run, three storage formats and three cuts of the run.  A case is one
block of a family's seeds; every draw is solved once with solve_batched and held to:

  (a) exact, every column: 0 <= x <= ub bitwise; x exactly 0 where ub is 0 (held-out rows, ghost rows, rows outside a pair's
      classes); for the pair families d exactly 0 outside the pair's classes and g exactly its linear term there (0 for the simplex
      blocks; -1 for the SVC pair columns, whose dual has q = -1 on every row: the product's part of g is exactly 0); the records'
      iter field is 0 ... iter; the status is 'optimal' or 'stopped'.
  (b) batch invariance, bit for bit: the last column and one drawn column solved alone, the whole batch reversed, and the batch
      with another run cut give the same records (NaN equal to NaN), x, g, status and offsets as the first solve.
  (c) start state: g of every checked or re-solved column at the start point (a solve of the same columns whose stop tolerance ends
      it at iteration 0) against Q x0 + q in np.longdouble on the downloaded panel, elementwise within
      (m + 4) 2^-53 (|Q||x0| + |q|), m the number of terms summed: the forward bound of a sum in any order, without a margin.
  (d) trajectory, the checked columns (column 0, the last, the first of the second product chunk, the leaver): against the
      reference on the downloaded panel, which is first held to the oracle's Gram matrix.  Where the reference's four runs (K and
      three one-ulp perturbations) agree on status and iteration count, the device's are equal; the f history agrees within the
      larger of 10 x the column's own spread and 1e-9 max |f|, the final x within the larger of 10 x its spread and 1e-9 max ub;
      where they do not agree, f alone over the records all four runs have.  The simplex families' offsets are the reference's
      statements on the device's own x and g: counts exact, a mean over the free rows within the bound of a sum taken in another
      order, a midpoint exact.

18 draws per family (16 in four blocks, 2 at the strip edge), 162 in all: the CPU references of more do not fit the minute of
tests/test_batched_fuzz_host.py.  REGRESSION_DRAWS names the draws that exposed a bug.

The run exposed one bug, fixed with it: ProjectedGradient's ratio step x + t d with t = (lb - x_i) / d_i, and FrankWolfe's x + a (y - x),
are one rounded product and one rounded sum, and fl(x_i + fl(t d_i)) need not be the bound itself.  Before the fix (bq_pgfw_compute in
bq_epilogue.h now keeps the stepped x in its box, and the snapshot's host-side step with it) bar (a)'s box failed in labels4 (5 columns of
2 draws), boxes16 (15 of 4), svr (8 of 3), svr_boxes (10 of 5) and pairs (82 of 8): 1 to 5 entries per column below 0 by 1.7e-21 ...
2.8e-17 under ProjectedGradient, and one FrankWolfe column (boxes16 seed 114) with an entry 2.1e-22 above ub.  The simplex families held
the box bitwise.  (The CPU oracle, which restates the reference's `x += t * d`, leaves the box in the same way: pairs seed 401 column 1
ends with one entry at -1.1e-19.)

Measured on an MI355X, every checked column of a family (f and x spreads are the reference's own under one ulp of K; the
distances are the device's from the reference; g0 is the largest start-gradient error as a share of its bound), and the wall time
of the five cases (four blocks of 4 draws, the strip block of 2):
  labels4    49 columns: f spread <= 1.3e-07, |f - f_ref| <= 2.4e-07 (0.04 of its bar); x spread <= 6.3e-10, |x - x_ref| <= 1.2e-09
             (0.12 of its bar); g0 <= 0.01; 1.9 0.8 0.6 0.9 1.3 s
  boxes16    43 columns: f spread <= 2.4e-09, |f - f_ref| <= 4.0e-09 (0.01); x spread <= 2.1e-12, |x - x_ref| <= 3.6e-12; g0 <= 0.11;
             1.5 0.5 0.2 0.3 1.2 s
  svr        44 columns: f spread <= 2.4e-10, |f - f_ref| <= 8.4e-10; x spread <= 1.3e-13, |x - x_ref| <= 7.4e-14; g0 <= 0.05;
             1.5 0.2 0.9 0.8 1.8 s
  svr_boxes  38 columns: f spread <= 2.9e-10, |f - f_ref| <= 9.4e-10; x spread <= 7.2e-13, |x - x_ref| <= 4.4e-13; g0 <= 0.07;
             1.6 1.1 0.2 0.6 1.7 s
  pairs      39 columns: f spread <= 1.9e-09, |f - f_ref| <= 3.7e-09; x spread <= 8.2e-13, |x - x_ref| <= 7.0e-13; g0 <= 0.02;
             2.1 0.5 0.7 0.6 1.3 s
  sx_one     47 columns: f spread <= 7.6e-11, |f - f_ref| <= 1.3e-10; x spread <= 2.2e-12, |x - x_ref| <= 5.4e-12 (0.01); g0 <= 0.08;
             1.5 0.5 0.5 0.3 0.9 s
  sx_labels  44 columns: f spread <= 2.2e-11, |f - f_ref| <= 1.5e-11; x spread <= 6.8e-14, |x - x_ref| <= 2.4e-13; g0 <= 0.06;
             1.8 0.6 0.2 0.4 1.0 s
  sx_paired  40 columns, 2 of them not unanimous on the device's panel (x spread 8.3e-09: compared on f alone): f spread
             <= 6.7e-12, |f - f_ref| <= 5.2e-12; |x - x_ref| <= 4.7e-14; g0 <= 0.01; 1.6 0.4 0.3 0.2 0.8 s
  sx_blocks  38 columns: f spread <= 5.9e-12, |f - f_ref| <= 4.9e-12; x spread <= 1.5e-13, |x - x_ref| <= 7.1e-14; g0 <= 0.03;
             1.6 0.6 0.6 0.4 1.0 s
Where no share is given the distance is below 0.005 of its bar, which the 1e-9 floors set in almost every column.
"""
import time

import numpy as np
import pytest

import batched_fuzz_reference as bf
from conftest import set_hooks

pytestmark = pytest.mark.gpu

START_EPS = 1e300   # a stop tolerance that ends every column at iteration 0: x = x0 and g = g(x0) stay on the device

# (family, seed, what the draw exposed): solved like a block of one draw
REGRESSION_DRAWS = (
    ('labels4', 9, 'ProjectedGradient on the 4-column product: a ratio step left entries of 4 columns at -4.3e-19 ... -2.8e-17, not 0'),
    ('pairs', 413, 'the same on the routed product: 9 columns, up to 4 entries each'),
    ('svr_boxes', 309, 'the same on SVR columns with one box each (2n variables)'),
    ('boxes16', 114, "FrankWolfe's full step x + 1 (ub - x) ended one entry 2.1e-22 above ub"),
)

CASES = [(f, 'block%d' % b, block) for f in bf.FAMILIES for b, block in enumerate(bf.BLOCKS[f])]
CASES += [(f, 'regression%d' % s, (s,)) for f, s, _ in REGRESSION_DRAWS]


@pytest.fixture(scope='module')
def amd():
    from optiml_amd import _lib
    from optiml_amd.device import get_context
    _lib.load()
    get_context()


def _quad(dr):
    from optiml_amd.ml.svm.kernels import GaussianKernel, LinearKernel, PolyKernel
    from optiml_amd.opti import KernelQuadratic
    name, g, coef0, degree = dr.kernel
    kernel = GaussianKernel(gamma=g) if name == 'rbf' else PolyKernel(degree=degree, gamma=g, coef0=coef0) if name == 'poly' else LinearKernel()
    n = dr.n
    storage = 'f32' if dr.storage == 'f32' else 'f64'
    if dr.structure == 'svc':
        return KernelQuadratic(dr.X, -np.ones(n), 'svc', kernel, y=np.ones(n), storage=storage)
    return KernelQuadratic(dr.X, np.zeros(dr.m if dr.structure == 'svr' else n), dr.structure, kernel, storage=storage)


def _solver(dev, dr, cols, eps, max_iter):
    from optiml_amd import _lib
    from optiml_amd.ml.svm import _batched as B
    from optiml_amd.ml.svm.onevsone import _DevicePairSolver
    sub = lambda A: None if A is None else np.ascontiguousarray(A[cols])   # noqa: E731
    box = lambda: dr.UB if dr.UB.ndim == 1 else sub(dr.UB)                  # noqa: E731
    kind = {'pg': _lib.PG, 'fw': _lib.FW, None: None}[dr.kind]
    x0, fam = sub(dr.x0), dr.family
    if fam in ('labels4', 'boxes16'):
        return B._DeviceMultiSolver(dev, kind, sub(dr.Y), box(), eps, max_iter, dr.t, x0)
    if fam in ('svr', 'svr_boxes'):
        return B._DeviceSVRSolver(dev, kind, sub(dr.QL), box(), eps, max_iter, dr.t, x0)
    pairs = None if dr.pairs is None else [dr.pairs[c] for c in cols]
    if fam == 'pairs':
        return _DevicePairSolver(dev, kind, dr.ct, pairs, sub(dr.Y), box(), eps, max_iter, t=dr.t, x0=x0)
    if fam == 'sx_one':
        return B._DeviceSimplexSolver(dev, box(), sub(dr.mass), eps, max_iter, x0)
    if fam == 'sx_blocks':
        return B._DeviceSimplexPairSolver(dev, dr.ct, pairs, box(), sub(dr.mass), eps, max_iter, x0)
    return B._DeviceSimplex2Solver(dev, sub(dr.S), box(), sub(dr.mass), sub(dr.q), eps, max_iter, x0)


def _solve(dev, dr, cols, chunk, eps=None, max_iter=None):
    """Columns `cols` of the draw in that order, run in calls of `chunk` iterations: per column solve_batched's dict, with d for
    the pair families and rho, n_sv, n_free (one entry per group) for the simplex families"""
    from optiml_amd import _lib
    from optiml_amd.ml.svm._batched import solve_batched
    cols = list(cols)
    held = {}

    def last(solver, _):
        if dr.family in bf.SIMPLEX_FAMILIES:
            held['off'] = solver.offsets()
        if dr.family in bf.PAIR_FAMILIES:
            held['d'] = [solver.get(j, _lib.GET_D) for j in range(len(cols))]

    solver = _solver(dev, dr, cols, dr.eps if eps is None else eps, dr.max_iter if max_iter is None else max_iter)
    res = solve_batched(dev, None, np.zeros((len(cols), 1)), None, solver=solver, before_close=last, chunk=chunk)
    for j, r in enumerate(res):
        if 'd' in held:
            r['d'] = held['d'][j]
        if dr.family == 'sx_one':
            rho, n_sv, n_free = held['off']
            r.update(rho=[rho[j]], n_sv=[int(n_sv[j])], n_free=[int(n_free[j])])
        elif 'off' in held:
            r1, r2, n_sv, n_free = held['off']
            r.update(rho=[r1[j], r2[j]], n_sv=[int(v) for v in n_sv[j]], n_free=[int(v) for v in n_free[j]])
    return res


def _assert_same_bits(a, b, where):
    assert a['status'] == b['status'] and a['iter'] == b['iter'], where
    assert len(a['rows']) == len(b['rows']), where
    for name in a['rows'].dtype.names:   # (the records hold NaN where a solver has no such figure)
        assert np.array_equal(a['rows'][name], b['rows'][name], equal_nan=True), (where, name)
    assert np.array_equal(a['x'], b['x']) and np.array_equal(a['g'], b['g']), where
    if 'rho' in a:
        assert np.array_equal(a['rho'], b['rho'], equal_nan=True), where
        assert a['n_sv'] == b['n_sv'] and a['n_free'] == b['n_free'], where


def _exact(dr, c, r, where):
    """bar (a)"""
    ub = bf.ub_of(dr, c)
    assert np.all(r['x'] >= 0) and np.all(r['x'] <= ub), (where, float(r['x'].min()), float((r['x'] - ub).max()))
    assert not r['x'][ub == 0].any(), where
    assert r['status'] in ('optimal', 'stopped') and 0 <= r['iter'] <= dr.max_iter, where
    assert np.array_equal(r['rows']['iter'], np.arange(r['iter'] + 1)), where
    if dr.family in bf.PAIR_FAMILIES:
        i, j = dr.pairs[c]
        out = (dr.pcode != i) & (dr.pcode != j)
        assert not r['d'][out].any(), where
        assert np.all(r['g'][out] == (-1.0 if dr.family == 'pairs' else 0.0)), where


def _start_state(dr, c, K, start, where):
    """bar (c); returns the largest error as a share of its bound"""
    x, g = start['x'], start['g']
    assert start['status'] == 'optimal' and start['iter'] == 0, where
    if dr.x0 is not None:
        assert np.array_equal(x, dr.x0[c]), where
    elif dr.family in bf.BOX_FAMILIES:
        assert np.array_equal(x, bf.ub_of(dr, c) / 2), where
    rows, want, bound = bf.start_gradient(dr, c, K, x)
    err = np.abs(g[rows].astype(np.longdouble) - want).astype(float)
    assert np.all(err <= bound), (where, float(err.max()), float((err / np.maximum(bound, 1e-300)).max()))
    return float((err / np.maximum(bound, 1e-300)).max())


def _trajectory(dr, c, r, sens, where):
    """bar (d)"""
    base = sens['base']
    idx = sens['idx']
    f_dev = r['rows']['f']
    if sens['unanimous']:
        assert r['status'] == base['status'] and r['iter'] == base['iter'], (where, r['status'], r['iter'], base['status'], base['iter'])
        assert len(f_dev) == len(base['f']), where
    m = min(sens['common'], len(f_dev))
    assert m >= 1, where
    f_err = float(np.abs(f_dev[:m] - base['f'][:m]).max())
    f_tol = bf.f_bar(sens)
    x_err, x_tol = float('nan'), bf.x_bar(dr, c, sens)
    print('%s: unanimous=%s %s at %d, f spread %.2e, |f - f_ref| %.2e (bar %.2e), x spread %.2e' %
          (where, sens['unanimous'], base['status'], base['iter'], sens['f_spread'], f_err, f_tol, sens['x_spread']), end='')
    assert f_err <= f_tol, (where, f_err, f_tol)
    if sens['unanimous']:
        x_err = float(np.abs(r['x'][idx] - base['x']).max())
        print(', |x - x_ref| %.2e (bar %.2e)' % (x_err, x_tol), end='')
        assert x_err <= x_tol, (where, x_err, x_tol)
    print()
    if dr.family in bf.SIMPLEX_FAMILIES:
        for name, got, want, bound in bf.offset_check(dr, c, r):
            if bound == 0:
                assert got == want, (where, name, got, want)
            else:
                assert abs(got - want) <= bound, (where, name, got, want, bound)


def _run_draw(family, seed, monkeypatch):
    dr = bf.draw(family, seed)
    k = dr.k
    set_hooks(monkeypatch, compact_panel=0 if dr.storage == 'f64_plain' else None)
    quad = _quad(dr)
    try:
        K = quad.gram()
        rtol, atol = bf.gram_tolerance(dr)
        np.testing.assert_allclose(K, bf.oracle_gram(dr), rtol=rtol, atol=atol, err_msg='%s seed %d: the panel' % (family, seed))
        dev = quad.device_problem()
        every = list(range(k))
        first = _solve(dev, dr, every, dr.chunk)
        for c in every:
            _exact(dr, c, first[c], '%s seed %d column %d' % (family, seed, c))
        # (b)
        alone = sorted({k - 1, dr.extra})
        for c in alone:
            _assert_same_bits(_solve(dev, dr, [c], dr.chunk)[0], first[c], '%s seed %d column %d alone' % (family, seed, c))
        for j, r in enumerate(_solve(dev, dr, every[::-1], dr.chunk)):
            _assert_same_bits(r, first[k - 1 - j], '%s seed %d column %d reversed' % (family, seed, k - 1 - j))
        for c, r in enumerate(_solve(dev, dr, every, dr.chunk2)):
            _assert_same_bits(r, first[c], '%s seed %d column %d in runs of %d' % (family, seed, c, dr.chunk2))
        # (c)
        some = sorted(set(dr.checked) | set(alone))
        start = _solve(dev, dr, some, dr.chunk, eps=START_EPS, max_iter=1)
        worst = max(_start_state(dr, c, K, start[j], '%s seed %d column %d start' % (family, seed, c)) for j, c in enumerate(some))
        print('%s seed %d: n=%d k=%d %s %s storage=%s chunk=%d x0=%s leaver=%s; |g0 - g0_ref| at most %.2f of its bound' %
              (family, seed, dr.n, k, dr.kernel[0], dr.kind, dr.storage, dr.chunk, dr.start, dr.leaver, worst))
        # (d)
        sens = bf.sensitivities(dr, dr.checked, K)
        for c in dr.checked:
            _trajectory(dr, c, first[c], sens[c], '%s seed %d column %d' % (family, seed, c))
        if seed in bf.LEAVERS[family]:
            assert first[dr.leaver]['status'] == 'optimal' and first[dr.leaver]['iter'] < dr.max_iter
            assert any(r['status'] == 'stopped' and r['iter'] == dr.max_iter for r in first)
    finally:
        quad.release()
        set_hooks(monkeypatch, compact_panel=None)


@pytest.mark.parametrize('family,name,block', CASES, ids=['%s-%s' % (f, name) for f, name, _ in CASES])
def test_draws_against_the_reference(amd, monkeypatch, family, name, block):
    t0 = time.perf_counter()
    for seed in block:
        _run_draw(family, seed, monkeypatch)
    print('%s %s: %d draws in %.2f s' % (family, name, len(block), time.perf_counter() - t0))
