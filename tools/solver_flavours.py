#!/usr/bin/env python3
"""One small fit per flavour of the single-problem side of the library — the solvers of bq_solver_create / bq_al_solver_create / bq_smo_create,
x_star, the dense problems, the streamed mode and the one-shot entry points (decision functions, Gram matrix, Cholesky solve) — and a
SHA-256 of everything each produces: x, g, the iteration records, f, the one-shots' outputs.  Two builds of the library that print
the same file compute the same bits (tools/msolver_flavours.py does the same for the batched solver):

    python3 tools/solver_flavours.py [path/to/libbcqp_hip.so] > flavours.txt

n = 300, d = 6 (two 256-row tiles, the second ragged), RBF gamma 0.5 unless a flavour says otherwise.  Every flavour creates and
destroys its own problem and solver (one does so twice in a row: destroy, cache, create), and every run is cut into bq_solver_run
calls of growing length, so that the solver's record buffer regrows.  At n = 300 every O(n) kernel is ONE block of 1024 elements,
so the `several_blocks` flavours repeat one solver of each family at n = 2500 (first-order: three vector blocks, the last ragged,
ten closing blocks of 256 rows) and n = 1300 (factorising: two vector blocks, three for the 2n of SVR, six to eleven closing
blocks): there the last-block ticket is taken by a block that is not alone.  The `minres` flavours reach the three forms of the
MINRES fallback.  No flavour uses an entry point younger than the tool, so it runs on an older build of the library too.
"""
import ctypes as C
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from optiml_amd import _lib  # noqa: E402

if len(sys.argv) > 1:
    from tools._with_lib import use_library
    use_library(sys.argv[1])

from optiml_amd.device import Context  # noqa: E402

N, D, GAMMA = 300, 6, 0.5
LIB = _lib.load()
CTX = Context()


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def show(name, **arrays):
    for key, a in arrays.items():
        print('%-34s %-10s %s' % (name, key, sha(a)))


def note(name, key, value):
    print('%-34s %-10s %s' % (name, key, value))


class hooks:
    """BQ_TEST_HOOKS (and plain environment switches) for the length of a flavour; the library reads them at every use"""

    def __init__(self, test_hooks=None, **env):
        self.env = dict(env)
        if test_hooks:
            self.env['BQ_TEST_HOOKS'] = test_hooks

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.env}
        os.environ.update(self.env)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def data(seed, n=N):
    rs = np.random.RandomState(seed)
    X = rs.standard_normal((n, D))
    y = np.where(X @ rs.standard_normal(D) + 0.3 * rs.standard_normal(n) > 0, 1.0, -1.0)
    t = np.sin(X @ rs.standard_normal(D)) + 0.1 * rs.standard_normal(n)
    return rs, X, y, t


def kernel_problem(structure, X, y, q, kernel=_lib.KERNEL_RBF, diag_add=0.0, storage=_lib.F64, flags=0):
    h = C.c_void_p()
    _lib.check(LIB.bq_problem_create_kernel(CTX.handle, structure | flags, len(X), D, _lib.ptr(X), _lib.ptr(y), kernel, GAMMA, 0.0, 3,
                                            diag_add, _lib.ptr(q), storage, C.byref(h)))
    return h


def svc_problem(seed, n=N, **kw):
    rs, X, y, _ = data(seed, n)
    return kernel_problem(_lib.SVC, _lib.as_f64(X), _lib.as_f64(y), -np.ones(n), **kw), y


def svr_problem(seed, n=N, **kw):
    rs, X, _, t = data(seed, n)
    q = np.concatenate([0.1 - t, 0.1 + t])
    return kernel_problem(_lib.SVR, _lib.as_f64(X), None, _lib.as_f64(q), **kw), t


def run_cut(s, name, first=5, rounds=12):
    """bq_solver_run in pieces of 5, 10, 20, ... steps (each longer than the record buffer: it regrows) until the solver stops; the
    records of every piece, then the state"""
    recs, steps = [], first
    status = C.c_int(0)
    for _ in range(rounds):
        buf = np.zeros(steps + 1, dtype=_lib.STAT_DTYPE)
        got = C.c_int64(0)
        _lib.check(LIB.bq_solver_run(s, steps, buf.ctypes.data_as(C.POINTER(_lib.IterStat)), steps + 1, C.byref(got), C.byref(status)))
        recs.append(buf[:got.value])
        if status.value != 0:
            break
        steps *= 2
    return np.concatenate(recs), status.value


def state(s):
    it, st, f = C.c_int64(0), C.c_int(0), C.c_double(0)
    _lib.check(LIB.bq_solver_state(s, C.byref(it), C.byref(st), C.byref(f)))
    return it.value, st.value, f.value


def get(s, what, n):
    out = np.zeros(n)
    _lib.check(LIB.bq_solver_get(s, what, _lib.ptr(out)))
    return out


def finish(s, name, n_dual, recs, extra=()):
    it, st, f = state(s)
    show(name, x=get(s, _lib.GET_X_NOW, n_dual), g=get(s, _lib.GET_G_NOW, n_dual), records=recs, state=np.array([it, f]),
         **{key: get(s, what, n) for key, what, n in extra})
    inner = C.c_int64(0)
    _lib.check(LIB.bq_solver_inner_iters(s, C.byref(inner)))
    note(name, 'status', '%s after %d iterations, %d inner' % (_lib.STATUS[st], it, inner.value))


def box_solver(p, kind, n_dual, eps=1e-6, max_iter=400, fw_t=0.0):
    s = C.c_void_p()
    _lib.check(LIB.bq_solver_create(p, kind, None, _lib.ptr(np.ones(n_dual)), None, eps, max_iter, fw_t, C.byref(s)))
    return s


def solve(name, p, kind, n_dual, extra=(), **kw):
    s = box_solver(p, kind, n_dual, **kw)
    recs, _ = run_cut(s, name)
    finish(s, name, n_dual, recs, extra)
    LIB.bq_solver_destroy(s)
    LIB.bq_problem_destroy(p)


def first_order():
    solve('svc_pg', svc_problem(1)[0], _lib.PG, N)
    solve('svc_pg_again', svc_problem(1)[0], _lib.PG, N)   # the same once more: destroy, the context's cache, create
    solve('svc_fw_t0', svc_problem(2)[0], _lib.FW, N, eps=1e-3)
    solve('svc_fw_t05', svc_problem(2)[0], _lib.FW, N, eps=1e-3, fw_t=0.5)
    solve('svr_pg', svr_problem(3)[0], _lib.PG, 2 * N)
    solve('svc_pg_stream', svc_problem(4, storage=_lib.STREAM)[0], _lib.PG, N)


def masks(n):
    return (('mask_l', _lib.GET_MASK_L, n), ('mask_u', _lib.GET_MASK_U, n))


MASKS = masks(N)


def active_set():
    solve('svc_as_dense', svc_problem(5)[0], _lib.AS, N, MASKS)
    # with a diagonal term the preconditioner's model leaves every sample enough of its diagonal and is kept (the inner iteration
    # counts differ between the families); without one every family is built, found wanting and dropped
    for cls in range(4):   # the preconditioner's feature families; 3 forces the order-2 remainder
        with hooks('as_cg_pc_class=%d' % cls):
            solve('svc_as_cg_class%d' % cls, svc_problem(6, diag_add=0.5)[0], _lib.AS_CG, N, MASKS)
    solve('svc_as_cg_dropped', svc_problem(6)[0], _lib.AS_CG, N, MASKS)
    solve('svc_as_cg_linear', svc_problem(7, kernel=_lib.KERNEL_LINEAR, diag_add=0.5)[0], _lib.AS_CG, N, MASKS)
    with hooks(BQ_AS_CG_PC='0'):
        solve('svc_as_cg_no_pc', svc_problem(6, diag_add=0.5)[0], _lib.AS_CG, N, MASKS)


def active_set_resumed():
    """a dense ActiveSet stopped after 12 iterations and continued in a new solver from (x, g, masks)"""
    name = 'svc_as_resumed'
    p, _ = svc_problem(8)
    s = box_solver(p, _lib.AS, N)
    buf = np.zeros(13, dtype=_lib.STAT_DTYPE)
    got, status = C.c_int64(0), C.c_int(0)
    _lib.check(LIB.bq_solver_run(s, 12, buf.ctypes.data_as(C.POINTER(_lib.IterStat)), 13, C.byref(got), C.byref(status)))
    x, g, ml, mu = np.zeros(N), np.zeros(N), np.zeros(N), np.zeros(N)
    snap = _lib.SolverState(x=_lib.ptr(x), g=_lib.ptr(g), mask_l=_lib.ptr(ml), mask_u=_lib.ptr(mu))
    _lib.check(LIB.bq_solver_get_state(s, C.byref(snap)))
    show(name + '.stopped', x=x, g=g, mask_l=ml, mask_u=mu, records=buf[:got.value])
    LIB.bq_solver_destroy(s)
    s = box_solver(p, _lib.AS, N)
    snap.have = _lib.STATE_X | _lib.STATE_G | _lib.STATE_MASKS
    _lib.check(LIB.bq_solver_set_state(s, C.byref(snap)))
    recs, _ = run_cut(s, name)
    finish(s, name, N, recs, MASKS)
    LIB.bq_solver_destroy(s)
    LIB.bq_problem_destroy(p)


def mult(n):
    return (('lp', _lib.GET_LP, n), ('lm', _lib.GET_LM, n))


def interior_point():
    solve('svc_ip', svc_problem(9)[0], _lib.IP, N, mult(N), max_iter=60)
    solve('svr_ip', svr_problem(10)[0], _lib.IP, 2 * N, mult(2 * N), max_iter=60)


def lagrangian(name, schedules, n=N):
    """the augmented-Lagrangian solver with an equality row and both bounds; schedules: how often they are set before the run"""
    p, y = svc_problem(11, n)
    rs = np.random.RandomState(12)
    prm = _lib.AlParams(rule=_lib.RULE_ADAM, momentum_type=_lib.MOM['none'], step_size=0.05, momentum=0.0, beta1=0.9, beta2=0.999,
                        decay=0.9, offset=1e-8, rho=1.0, tol=1e-9, epochs=90)
    s = C.c_void_p()
    _lib.check(LIB.bq_al_solver_create(p, C.byref(prm), _lib.ptr(_lib.as_f64(y)), _lib.ptr(np.zeros(n)), _lib.ptr(np.ones(n)),
                                       _lib.ptr(rs.uniform(size=n)), None, C.byref(s)))
    for k in range(schedules):   # the second call releases the first one's device arrays
        steps = 0.05 / (1.0 + 0.02 * np.arange(40 + 10 * k))
        _lib.check(LIB.bq_al_solver_set_schedules(s, _lib.ptr(steps), None, len(steps)))
    nd = C.c_int64(0)
    _lib.check(LIB.bq_al_solver_dual_size(s, C.byref(nd)))
    recs, _ = run_cut(s, name)
    it, st, f = state(s)
    show(name, x=get(s, _lib.GET_X_NOW, n), g=get(s, _lib.GET_G, n), step=get(s, _lib.GET_D, n), dual=get(s, _lib.GET_DUAL, nd.value),
         records=recs, state=np.array([it, f]))
    note(name, 'status', '%s after %d iterations' % (_lib.STATUS[st], it))
    LIB.bq_solver_destroy(s)
    LIB.bq_problem_destroy(p)


def smo(name, task):
    rs, X, y, t = data(13)
    p = kernel_problem(_lib.PLAIN, _lib.as_f64(X), None, np.zeros(N), flags=_lib.PLAIN_PANEL)
    s = C.c_void_p()
    _lib.check(LIB.bq_smo_create(p, task, _lib.ptr(_lib.as_f64(y if task == _lib.SVC else t)), 1.0, 0.1 if task == _lib.SVR else 0.0,
                                 1e-3, C.byref(s)))
    outer, fin = C.c_int64(0), C.c_int(0)
    while not fin.value and outer.value < 2000:
        _lib.check(LIB.bq_smo_run(s, 16, C.byref(outer), C.byref(fin)))
    out = {}
    for key, what, n in (('alphas', _lib.SMO_ALPHAS, N if task == _lib.SVC else 2 * N), ('errors', _lib.SMO_ERRORS, N),
                         ('scalars', _lib.SMO_SCALARS, 6)):   # (not SMO_STATS: how many sums the helpers delivered is a matter of timing)
        out[key] = np.zeros(n)
        _lib.check(LIB.bq_smo_get(s, what, _lib.ptr(out[key])))
    show(name, **out)
    note(name, 'sweeps', '%d, finished %d' % (outer.value, fin.value))
    LIB.bq_smo_destroy(s)
    LIB.bq_problem_destroy(p)


def x_star():
    rs, X, _, t = data(14)
    p = kernel_problem(_lib.PLAIN, _lib.as_f64(X), None, _lib.as_f64(-t), diag_add=0.5)
    x, method, iters = np.zeros(N), C.c_int(0), C.c_int64(0)
    _lib.check(LIB.bq_problem_x_star(p, _lib.ptr(x), C.byref(method), C.byref(iters)))
    show('x_star', x=x)
    note('x_star', 'method', '%d, %d minres iterations' % (method.value, iters.value))
    LIB.bq_problem_destroy(p)


def x_star_minres():
    """no diagonal term and a linear kernel: the Hessian X X' has rank 6, the factorisation fails and scipy's MINRES takes over
    (bq_xstar.hip: the recurrence on the host)"""
    rs, X, _, t = data(17)
    p = kernel_problem(_lib.PLAIN, _lib.as_f64(X), None, _lib.as_f64(-t), kernel=_lib.KERNEL_LINEAR)
    x, method, iters = np.zeros(N), C.c_int(0), C.c_int64(0)
    _lib.check(LIB.bq_problem_x_star(p, _lib.ptr(x), C.byref(method), C.byref(iters)))
    assert method.value == 1, 'x_star_minres: the factorisation succeeded, MINRES was not reached'
    show('x_star_minres', x=x)
    note('x_star_minres', 'method', '%d, %d minres iterations' % (method.value, iters.value))
    LIB.bq_problem_destroy(p)


def active_set_minres():
    """a linear kernel: Q[A,A] is singular while the free set is larger than the rank, and ActiveSet takes its MINRES branch — in
    the persistent workgroup, and under minres_big_min=0 in the multi-workgroup form (as tests/test_gpu_parity.py switches it)"""
    for name, hook in (('svc_as_minres', None), ('svc_as_minres_big', 'minres_big_min=0')):
        with hooks(hook):
            p, _ = svc_problem(18, kernel=_lib.KERNEL_LINEAR)
            s = box_solver(p, _lib.AS, N, max_iter=60)
            recs, _ = run_cut(s, name)
            finish(s, name, N, recs, MASKS)
            calls = C.c_int64(0)
            _lib.check(LIB.bq_solver_counter(s, _lib.COUNT_MINRES, C.byref(calls)))
            assert calls.value > 0, name + ': the MINRES branch was not reached'
            note(name, 'minres', '%d iterations through the fallback' % calls.value)
            LIB.bq_solver_destroy(s)
            LIB.bq_problem_destroy(p)


def several_blocks():
    """one solver of each family on more than one vector block (see the module docstring)"""
    n1, n2 = 2500, 1300
    solve('svc_pg_n2500', svc_problem(19, n1)[0], _lib.PG, n1, max_iter=60)
    solve('svr_fw_n1300', svr_problem(20, n2)[0], _lib.FW, 2 * n2, eps=1e-3, max_iter=60)
    lagrangian('svc_al_n2500', 0, n1)
    solve('svc_as_cg_n1300', svc_problem(21, n2, diag_add=0.5)[0], _lib.AS_CG, n2, masks(n2), max_iter=40)
    solve('svc_as_dense_n1300', svc_problem(22, n2)[0], _lib.AS, n2, masks(n2), max_iter=60)
    solve('svc_ip_n1300', svc_problem(23, n2)[0], _lib.IP, n2, mult(n2), max_iter=30)


def dense(name, symmetric, storage):
    rs = np.random.RandomState(15)
    A = rs.standard_normal((N, N))
    Q = A @ A.T / N + np.eye(N)
    if not symmetric:
        Q = Q + 0.01 * np.triu(rs.standard_normal((N, N)), 1)
    p = C.c_void_p()
    _lib.check(LIB.bq_problem_create_dense(CTX.handle, N, _lib.ptr(_lib.as_f64(Q)), _lib.ptr(rs.standard_normal(N)), storage, C.byref(p)))
    packed = C.c_int(0)
    _lib.check(LIB.bq_problem_layout(p, C.byref(packed), None, None))
    note(name, 'packed', packed.value)
    solve(name, p, _lib.PG, N)


def one_shots():
    rs, X, y, t = data(16)
    SV, Xt = _lib.as_f64(X), _lib.as_f64(rs.standard_normal((N, D)))
    coef = _lib.as_f64(rs.standard_normal(N))
    out = np.zeros(N)
    with hooks('decision_chunk_rows=256'):   # two chunks of test points
        _lib.check(LIB.bq_decision_function(CTX.handle, _lib.KERNEL_RBF, GAMMA, 0.0, 3, N, D, _lib.ptr(SV), _lib.ptr(coef), 0.25, N,
                                            _lib.ptr(Xt), _lib.ptr(out)))
    show('decision_function', out=out)
    W, b, outm = _lib.as_f64(rs.standard_normal((5, N))), _lib.as_f64(rs.standard_normal(5)), np.zeros((5, N))
    _lib.check(LIB.bq_decision_function_multi(CTX.handle, _lib.KERNEL_RBF, GAMMA, 0.0, 3, N, D, _lib.ptr(SV), 5, _lib.ptr(W), _lib.ptr(b),
                                              N, _lib.ptr(Xt), _lib.ptr(outm)))
    show('decision_function_multi', out=outm)
    K = np.zeros((N, N))
    _lib.check(LIB.bq_gram_matrix(CTX.handle, _lib.KERNEL_RBF, GAMMA, 0.0, 3, N, D, _lib.ptr(SV), N, None, _lib.ptr(K)))
    show('gram_matrix_self', out=K)
    Xb = _lib.as_f64(Xt[:77])
    Kb = np.zeros((N, 77))
    _lib.check(LIB.bq_gram_matrix(CTX.handle, _lib.KERNEL_RBF, GAMMA, 0.0, 3, N, D, _lib.ptr(SV), 77, _lib.ptr(Xb), _lib.ptr(Kb)))
    show('gram_matrix_cross', out=Kb)
    A = _lib.as_f64(K + 0.5 * np.eye(N))
    x = np.zeros(N)
    _lib.check(LIB.bq_cholesky_solve(CTX.handle, N, _lib.ptr(A), _lib.ptr(_lib.as_f64(t)), _lib.ptr(x), None))
    show('cholesky_solve', x=x)


if __name__ == '__main__':
    first_order()
    active_set()
    active_set_resumed()
    interior_point()
    lagrangian('svc_al', 0)
    lagrangian('svc_al_schedules', 1)
    lagrangian('svc_al_schedules_twice', 2)
    smo('smo_svc', _lib.SVC)
    smo('smo_svr', _lib.SVR)
    x_star()
    x_star_minres()
    active_set_minres()
    several_blocks()
    dense('dense_sym_f64', True, _lib.F64)
    dense('dense_asym_f32', False, _lib.F32)
    one_shots()
