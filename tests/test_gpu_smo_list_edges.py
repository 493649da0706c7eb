"""The SMO walker (csrc/bq_smo.hip) held to the CPU oracle where its support list is long: past the SMO_T = 1024 entries one trip of
`sup_apply`'s shift loops moves, and past the SMO_CAP = 4096 entries mirrored in LDS.

tests/test_gpu_smo.py compares the single walker step for step with the oracle at n <= 600, where every shift is one trip and the whole
list lives in LDS; the tests that reach past the mirror (test_gpu_smo_batched.py, the helper test of test_gpu_smo.py) compare the kernel
with itself.  Here every case runs a problem whose list passes 4096 entries (tests/smo_list_reference.py: 4800 coin-flip labels, a noisy
SVR target on 4600 rows) for MAX_OUTER outer iterations, one `bq_smo_run(h, 1)` at a time, and holds the device after EVERY outer
iteration to the oracle with the kernel's tie rule and summation order (tie='index', dot='tree') on the device's own Gram panel: step
count and finished flag, the support set, the multipliers and both thresholds, and after the last iteration the error cache.  A run is cut
after six outer iterations — the edges lie in the second full sweep, outer iteration 3 (tests/test_smo_list_host.py) — so the oracle costs
seconds.  Before anything is compared the oracle's own run on the device's panel must have met every edge: shifts of more than SMO_T
entries, entries moving across position SMO_CAP in both directions, error sums over more than SMO_CAP entries.

Cases.  SVC on the packed fp64 panel, the square one, the compact 7-byte panel and the fp32 panel; the packed and the compact panel also
with the helper workgroups off (hook smo_helpers=0) and at their minimum (16) — each run against the oracle, none against another run;
SVR on the packed and the compact panel, helpers default and off; and column 1 of a two-column batched solve (`bq_msmo_*`) on a 6000-row
panel whose row list leaves out every fifth row: the one path with list entries that are panel rows, not positions (SmoRows).  Neither
draw is eligible for the compact layout at gamma='scale' (exp(-4 gamma max|x|^2) is 1e-6 / 1e-7, the layout needs 2^-14), so the
compact cases run at `compact_gamma` (2^-12.6), where the host test re-checks the edges; their oracle run is the one of the plain fp64
panel at that gamma, which the compact panel must equal bit for bit.

REGRESSION_DRAWS names the draws that exposed a bug: none so far — every case passed on the first run.

Measured on an MI355X.  The largest difference from the oracle was 0 in every case, over every multiplier, threshold and error-cache
entry of every outer iteration, so the comparisons assert equality (the project's bar for this comparison is rtol 1e-12, atol 1e-15).
Per distinct panel: long inserts / long erases / crossing inserts / crossing erases / long dots of the oracle's run on it, the longest
list, the step count after each outer iteration; per case: helpers and sums they delivered (both rejection counters 0 everywhere), the
wall time of the device side (panel build, download, six launches) and of the whole case with its share of the oracle runs (0.5 - 0.7 s
per distinct panel there):
  svc packed fp64   155 / 43 / 162 / 53 / 1197, list <= 4767, steps 4789 4800 4803 5460 5521 5543
                    default: 48 helpers, 255365 sums, 1.4 s (first case: context start), 2.1 s; helpers=0: 0.3 s, 0.4 s;
                    helpers=16: 89428 sums, 0.3 s, 0.4 s
  svc square fp64   153 / 41 / 160 / 50 / 1180, list <= 4765, steps 4789 4800 4803 5443 5499 5520 (not the packed panel's bits: its own
                    oracle run); 48 helpers, 252580 sums, 0.2 s, 0.8 s
  svc compact       188 / 49 / 197 / 57 / 1182, list <= 4763, steps 4779 4788 4792 5465 5515 5529; bit-equal to the plain fp64 panel at
                    its gamma; default: 48 helpers, 243982 sums, 0.3 s, 1.1 s (with the plain panel's build and the oracle run);
                    helpers=0: 0.4 s, 0.5 s; helpers=16: 89585 sums, 0.3 s, 0.5 s
  svc fp32          153 / 40 / 160 / 50 / 1182, list <= 4766, steps 4789 4800 4803 5445 5501 5522; 48 helpers, 245398 sums, 0.3 s, 0.9 s
  svr packed fp64   10 / 123 / 12 / 141 / 1356, list <= 4595, steps 4599 4656 4667 5528 5806 5915
                    default: 48 helpers, 253266 sums, 0.2 s, 1.0 s; helpers=0: 0.3 s, 0.4 s
  svr compact       5 / 79 / 5 / 101 / 1209, list <= 4596, steps 4599 4624 4629 5339 5535 5616; bit-equal to the plain panel
                    default: 48 helpers, 235263 sums, 0.3 s, 1.2 s; helpers=0: 0.4 s, 0.5 s
  svc row list      175 / 42 / 192 / 51 / 1280, list <= 4760, steps 4779 4794 4798 4799 5584 5675 (the second full sweep is outer
                    iteration 4 here); no helpers in a batched solve; 0.4 s, 1.1 s
13 cases in 11.5 s, so MAX_OUTER stays at 6.

What the file notices, tried on scratch builds with a planted fault that stays in bounds: (A) trips of the error sum past the first
adding their eight products in descending order, in `wave_dot` and `helper_sums` alike — every case fails at outer iteration 0 on
multipliers that differ by 1e-16 to 1e-15, which only the equality bar sees there, while tests/test_gpu_smo.py, test_gpu_smo_batched.py
and test_gpu_ovo_smo.py pass; (B) `sup_cf` reading the coefficient one position before, past the mirror — every case fails at outer
iteration 0 on the step count or the support set.
"""
import ctypes as C
import hashlib
import time

import numpy as np
import pytest

import smo_list_reference as lr
from conftest import set_hooks

pytestmark = pytest.mark.gpu

MAX_OUTER = 6
REGRESSION_DRAWS = ()   # (draw, what it exposed)


@pytest.fixture(scope='module')
def amd():
    import optiml_amd
    from optiml_amd import _lib
    from optiml_amd.device import get_context
    _lib.load()
    get_context()
    return optiml_amd


def _digest(K):
    return hashlib.blake2b(memoryview(np.ascontiguousarray(K)).cast('B'), digest_size=16).hexdigest()


class _Oracle:
    """one oracle run per distinct (problem, Gram panel): cases that download bit-equal panels share it"""

    def __init__(self):
        self.runs, self.seconds = {}, {}
        self.plain = {}   # problem: the key of its run on the plain fp64 panel at the compact cases' gamma

    def run(self, name, kind, K, y, par):
        key = (name, _digest(K))
        shared = key in self.runs
        if not shared:
            t = time.perf_counter()
            run = lr.run_oracle(kind, K, y, MAX_OUTER, **par)
            self.seconds[key] = time.perf_counter() - t
            # the condition that makes the comparison worth anything, on the panel the device walks
            assert not lr.missing_events(run['counts']), (name, run['counts'])
            assert run['largest'] > lr.SMO_CAP and len(run['snap'].rows) == MAX_OUTER
            self.runs[key] = run
        return self.runs[key], key, shared, self.seconds[key]


@pytest.fixture(scope='module')
def oracle():
    return _Oracle()


def _elems(n):
    nb = (n + 255) // 256
    return 65536 * nb * (nb + 1) // 2


PANELS = {   # KernelQuadratic arguments, bytes per panel element (packed panels), the gamma rule
    'packed': (dict(compact=False), 8, lr.rbf_gamma),
    'square': (dict(compact=False, full_panel=True), None, lr.rbf_gamma),
    'compact': (dict(compact=True), 7, lr.compact_gamma),
    'f32': (dict(storage='f32'), 4, lr.rbf_gamma),
}


def _quad(kind, X, y, eps, panel):
    """(quad, kernel) of the reg_intercept=False dual on the given panel; the layout is checked"""
    from optiml_amd.opti import KernelQuadratic
    from optiml_amd.ml.svm.kernels import GaussianKernel
    kw, esz, gamma_of = PANELS[panel]
    kern = GaussianKernel(gamma=gamma_of(X))
    n = len(X)
    if kind == 'svc':
        quad = KernelQuadratic(X, -np.ones(n), 'svc', kern, y=y, rank_one=False, **kw)
    else:
        quad = KernelQuadratic(X, np.hstack((-y, y)) + eps, 'svr', kern, rank_one=False, **kw)
    lay = quad.device_problem().layout()
    if esz is not None:   # 7 bytes per element: the panel is in fact compact (tests/test_gpu_compact_panel.py)
        assert lay['panel_bytes'] == _elems(n) * esz, (panel, lay)
    return quad


def _single_outer_states(quad, task, y, Cv, eps, tol, pull):
    """the single solver, one outer iteration per call: [(multipliers, scalars, finished)], the error cache, the helper statistics"""
    from optiml_amd import _lib
    lib = _lib.load()
    h = C.c_void_p()
    _lib.check(lib.bq_smo_create(quad.device_problem().handle, task, _lib.ptr(np.ascontiguousarray(y)), float(Cv), float(eps),
                                 float(tol), C.byref(h)))
    states = []
    outer, fin = C.c_int64(0), C.c_int(0)
    try:
        while not fin.value and len(states) < MAX_OUTER:
            _lib.check(lib.bq_smo_run(h, 1, C.byref(outer), C.byref(fin)))
            assert outer.value == len(states) + 1
            a, sc = np.empty(pull), np.empty(6)
            _lib.check(lib.bq_smo_get(h, _lib.SMO_ALPHAS, _lib.ptr(a)))
            _lib.check(lib.bq_smo_get(h, _lib.SMO_SCALARS, _lib.ptr(sc)))
            states.append((a, sc, bool(fin.value)))
        err, st = np.empty(len(y)), np.empty(4)
        _lib.check(lib.bq_smo_get(h, _lib.SMO_ERRORS, _lib.ptr(err)))
        _lib.check(lib.bq_smo_get(h, _lib.SMO_STATS, _lib.ptr(st)))
    finally:
        lib.bq_smo_destroy(h)
    stats = dict(helpers=int(st[0]), delivered=int(st[1]), rejected_list_hash=int(st[2]), rejected_checksum=int(st[3]))
    return states, err, stats


def _hold(what, got, want, diffs):
    """equality: the measured run differed nowhere (module docstring); tests/test_gpu_smo.py's bar (1) is rtol 1e-12, atol 1e-15, and
    1e-13 absolute for the error cache"""
    got, want = np.asarray(got, dtype=float), np.asarray(want, dtype=float)
    diffs.append(float(np.abs(got - want).max()))
    if diffs[-1]:
        print('%s: largest difference %.3g' % (what, diffs[-1]))
    assert np.array_equal(got, want), (what, diffs[-1])


def _hold_to_oracle(states, errors, run, pick=None):
    """the device after every outer iteration against the oracle's snapshots; pick: the listed rows of a row-list column (SVC).
    Returns the largest difference seen."""
    snap, ref = run['snap'], run['ref']
    assert len(states) == MAX_OUTER
    diffs = []
    for it, (a, sc, fin) in enumerate(states):
        if pick is not None:
            rest = np.ones(len(a), dtype=bool)
            rest[pick] = False
            assert not a[rest].any(), it   # an unlisted row is never examined
            a = a[pick]
        assert int(sc[4]) == snap.steps[it], (it, int(sc[4]), snap.steps[it])
        assert fin == (bool(ref['finished']) and it + 1 == ref['iter']), it
        assert np.array_equal(np.flatnonzero(a), np.flatnonzero(snap.rows[it])), it
        _hold('multipliers after outer iteration %d' % it, a, snap.rows[it], diffs)
        _hold('thresholds after outer iteration %d' % it, sc[:2], [snap.up[it], snap.low[it]], diffs)
    _hold('error cache after outer iteration %d' % (MAX_OUTER - 1), errors if pick is None else errors[pick], ref['errors'], diffs)
    return max(diffs)


def _report(case, run, shared, oracle_s, diff, stats, device_s):
    print('%-22s events %s largest list %d steps %s | max |device - oracle| %.3g | helpers %s | device %.2f s, oracle %.2f s%s'
          % (case, run['counts'], run['largest'], run['snap'].steps, diff, stats, device_s, oracle_s, ' (shared)' if shared else ''))


def _check_stats(stats, helpers):
    assert stats['rejected_list_hash'] == 0 and stats['rejected_checksum'] == 0, stats
    if helpers is None:
        assert stats['helpers'] > 0, stats
    else:
        assert stats['helpers'] == int(helpers), stats
    assert (stats['delivered'] > 0) == (stats['helpers'] > 0), stats


def _single_case(amd, monkeypatch, oracle, kind, panel, helpers):
    from optiml_amd import _lib
    X, y, par = lr.svc_draw() if kind == 'svc' else lr.svr_draw()
    eps = par.get('epsilon', 0.0)
    set_hooks(monkeypatch, smo_helpers=helpers)
    t = time.perf_counter()
    quad = _quad(kind, X, y, eps, panel)
    Kdev = quad.gram()
    states, errors, stats = _single_outer_states(quad, _lib.SVC if kind == 'svc' else _lib.SVR, y, par['C'], eps, par['tol'],
                                                 len(y) * (1 if kind == 'svc' else 2))
    quad.release()
    device_s = time.perf_counter() - t
    name = kind + ('-compact-gamma' if panel == 'compact' else '')
    if panel == 'compact' and name not in oracle.plain:   # lossless: the oracle run of the plain fp64 panel at this gamma
        from optiml_amd.opti import KernelQuadratic
        from optiml_amd.ml.svm.kernels import GaussianKernel
        kern = GaussianKernel(gamma=lr.compact_gamma(X))
        plain = (KernelQuadratic(X, -np.ones(len(y)), 'svc', kern, y=y, rank_one=False, compact=False) if kind == 'svc' else
                 KernelQuadratic(X, np.hstack((-y, y)) + eps, 'svr', kern, rank_one=False, compact=False))
        assert plain.device_problem().layout()['panel_bytes'] == _elems(len(y)) * 8
        Kplain = plain.gram()
        plain.release()
        assert np.array_equal(Kdev, Kplain)
        oracle.plain[name] = oracle.run(name, kind, Kplain, y, par)[1]
        del Kplain
    run, key, shared, oracle_s = oracle.run(name, kind, Kdev, y, par)
    assert panel != 'compact' or (shared and key == oracle.plain[name])
    diff = _hold_to_oracle(states, errors, run)
    _check_stats(stats, helpers)
    _report('%s %s helpers=%s' % (kind, panel, helpers), run, shared, oracle_s, diff, stats, device_s)


SVC_CASES = [('packed', None), ('packed', '0'), ('packed', '16'), ('square', None), ('compact', None), ('compact', '0'),
             ('compact', '16'), ('f32', None)]
SVR_CASES = [('packed', None), ('packed', '0'), ('compact', None), ('compact', '0')]


def _ids(cases):
    return ['%s-%s' % (p, 'default' if h is None else 'helpers' + h) for p, h in cases]


@pytest.mark.parametrize('panel,helpers', SVC_CASES, ids=_ids(SVC_CASES))
def test_svc_walker_follows_the_oracle_past_the_list_edges(amd, monkeypatch, oracle, panel, helpers):
    _single_case(amd, monkeypatch, oracle, 'svc', panel, helpers)


@pytest.mark.parametrize('panel,helpers', SVR_CASES, ids=_ids(SVR_CASES))
def test_svr_walker_follows_the_oracle_past_the_list_edges(amd, monkeypatch, oracle, panel, helpers):
    _single_case(amd, monkeypatch, oracle, 'svr', panel, helpers)


def test_row_list_column_follows_the_oracle_past_the_list_edges(amd, oracle):
    """a column whose list entries are panel rows, not positions: 4800 listed rows of a 6000-row panel, in column 1.  (One `row_ptr`
    serves all columns of a solve, so the column on all rows carries the identity list.)"""
    from optiml_amd import _lib
    from optiml_amd.ml.svm._batched import _DeviceSMOSolver
    X, Y, rows, par = lr.row_list_draw()
    tr = rows[1]
    t = time.perf_counter()
    quad = _quad('svc', X, Y[1], 0.0, 'packed')
    Kdev = quad.gram()
    solver = _DeviceSMOSolver(quad.device_problem(), _lib.SVC, Y, [par['C']] * 2, None, par['tol'], rows)
    states = []
    try:
        for call in range(1, MAX_OUTER + 1):
            outer, fin, failed = solver.run(1)
            assert not failed.any() and outer[1] == call
            states.append((solver.get(1, _lib.SMO_ALPHAS), solver.get(1, _lib.SMO_SCALARS), bool(fin[1])))
        errors = solver.get(1, _lib.SMO_ERRORS)
    finally:
        solver.close()
    quad.release()
    device_s = time.perf_counter() - t
    run, _, shared, oracle_s = oracle.run('row list', 'svc', Kdev[tr][:, tr], Y[1][tr], par)
    diff = _hold_to_oracle(states, errors, run, pick=tr)
    _report('svc row list, column 1', run, shared, oracle_s, diff, 'none (batched)', device_s)
