"""NumPy restatement of the row-based SMO's general entry (bq_rsmo_create_general, optiml_amd/csrc/bq_rsmo.hip; scalar rules in
csrc/bq_rsmo_step.h) on

    min 1/2 a'Qa + p'a,   0 <= a_t <= C_t,   Q_st = y_s y_t K_st,   from a start alpha0 with gradient G0

`solve_plain` is smo_rows_reference.solve (libsvm's Solver, one equality y'a = const) from (alpha0, G0) instead of (0, p): the
one-class dual.  `solve_nu` is libsvm's Solver_NU (svm.cpp: Solver_NU::select_working_set, Solver_NU::calculate_rho), which keeps
the mass of each sign: `ip` the arg-max of -G over y = +1 with a < C, `in` the arg-max of G over y = -1 with a > 0, ties to the
LARGER index; a candidate j scored against the row of its own sign (grad_diff = Gmaxp + G_j or Gmaxn - G_j), i = ip or in
according to y_j; stop when max(Gmaxp + Gmaxp2, Gmaxn + Gmaxn2) < tol; r1 / r2 per sign, rho = (r1 - r2) / 2, r = (r1 + r2) / 2.
The pair update is smo_rows_reference.pair_update, the gradient update its two rounded products, their rounded sum, one rounded add.

Also here: libsvm's three starts (solve_one_class, solve_nu_svc, solve_nu_svr) and libsvm's own start gradient (the sum of
alpha_i Q_i in ascending i), which the device replaces by one Gram product — for the host comparison only.
"""
import collections

import numpy as np

import smo_rows_reference as ref
from smo_rows_reference import TAU, _last, pair_update

NuResult = collections.namedtuple('NuResult', 'pairs sides alpha G rho r steps status gap_p gap_n')


# ---- the starts, as svm.cpp has them ---------------------------------------------------------------------------------------------------
def one_class_start(n, nu):
    a = np.zeros(n)
    m = int(nu * n)
    a[:m] = 1.0
    if m < n:
        a[m] = nu * n - m
    return a


def nu_svc_start(y, nu):
    n = len(y)
    left = {1: nu * n / 2, -1: nu * n / 2}
    a = np.zeros(n)
    for t in range(n):
        s = 1 if y[t] > 0 else -1
        a[t] = min(1.0, left[s])
        left[s] -= a[t]
    return a


def nu_svr_start(n, C, nu):
    left = C * nu * n / 2
    a = np.zeros(2 * n)
    for t in range(n):
        a[t] = a[t + n] = min(left, C)
        left -= a[t]
    return a


def one_class_problem(n, nu):
    """(signs, p, C, alpha0, rule)"""
    return np.ones(n), np.zeros(n), np.ones(n), one_class_start(n, nu), 'plain'


def nu_svc_problem(y, nu):
    y = np.asarray(y, dtype=float)
    return y.copy(), np.zeros(len(y)), np.ones(len(y)), nu_svc_start(y, nu), 'nu'


def nu_svr_problem(y, C, nu):
    y = np.asarray(y, dtype=float)
    n = len(y)
    return (np.concatenate((np.ones(n), -np.ones(n))), np.concatenate((-y, y)), np.full(2 * n, float(C)), nu_svr_start(n, C, nu),
            'nu')


def libsvm_start_gradient(K, signs, p, alpha0):
    """G = p + sum_i alpha_i Q_i over the i above their lower bound, in ascending i (Solver::Solve's initialisation)"""
    n, N = len(K), len(signs)
    rep = N // n
    G = np.asarray(p, dtype=float).copy()
    for i in range(N):
        if alpha0[i] > 0:
            G = G + alpha0[i] * ((signs[i] * signs) * np.tile(K[i % n], rep))
    return G


def product_start_gradient(K, signs, p, alpha0):
    """the device's formula in NumPy: lin + s o (K b), b folded to the rows (the rounding of the product is the BLAS's, not the
    device's: a test seeds the restatement with the device's own G0)"""
    n, N = len(K), len(signs)
    b = (signs * alpha0).reshape(N // n, n).sum(axis=0)
    if not b.any():
        return np.asarray(p, dtype=float).copy()
    return p + signs * np.tile(K @ b, N // n)


# ---- the solvers -----------------------------------------------------------------------------------------------------------------------
def _prepare(K, signs, p, C, alpha0, G0):
    K = np.asarray(K, dtype=float)
    n, N = len(K), len(signs)
    assert N in (n, 2 * n) and K.shape == (n, n)
    rep = N // n
    return (K, n, N, rep, np.asarray(signs, dtype=float), np.asarray(p, dtype=float), np.asarray(C, dtype=float),
            np.tile(np.diag(K).copy(), rep), np.array(alpha0, dtype=float), np.array(G0, dtype=float))


def _step(K, n, rep, y, C, QD, alpha, G, i, j, Ki):
    Kj = Ki if j % n == i % n else np.tile(K[j % n], rep)
    old_i, old_j = float(alpha[i]), float(alpha[j])
    a_i, a_j = pair_update(float(y[i]), float(y[j]), float(G[i]), float(G[j]), float(QD[i]), float(QD[j]), float(Ki[j]),
                           float(C[i]), float(C[j]), old_i, old_j)
    alpha[i], alpha[j] = a_i, a_j
    d_i, d_j = a_i - old_i, a_j - old_j
    Q_i, Q_j = (y[i] * y) * Ki, (y[j] * y) * Kj
    return G + ((Q_i * d_i) + (Q_j * d_j))


def solve_plain(K, signs, p, C, tol, alpha0, G0, max_steps=None, steps_only=None, trace=None):
    """smo_rows_reference.solve from (alpha0, G0); the same Result"""
    K, n, N, rep, y, p, C, QD, alpha, G = _prepare(K, signs, p, C, alpha0, G0)
    cap = max(10 ** 7, 100 * N) if max_steps is None else max_steps
    pairs, status, gmax, gmax2 = [], 'running', -np.inf, -np.inf
    while True:
        up = np.where(y > 0, alpha < C, alpha > 0)
        low = np.where(y > 0, alpha > 0, alpha < C)
        upval, lowval = np.where(y > 0, -G, G), np.where(y > 0, G, -G)
        gmax = upval[up].max() if up.any() else -np.inf
        gmax2 = lowval[low].max() if low.any() else -np.inf
        if not up.any() or gmax + gmax2 < tol:
            status = 'optimal'
            break
        if len(pairs) >= cap:
            status = 'stopped'
            break
        if steps_only is not None and len(pairs) >= steps_only:
            break
        i = _last(up & (upval == gmax))
        Ki = np.tile(K[i % n], rep)
        grad_diff = gmax + lowval
        cand = low & (grad_diff > 0)
        if not cand.any():
            status = 'optimal'
            break
        quad = (QD[i] + QD) - 2.0 * Ki
        quad = np.where(quad > 0, quad, TAU)
        with np.errstate(invalid='ignore', over='ignore'):
            obj = -((grad_diff * grad_diff) / quad)
        j = _last(cand & (obj == obj[cand].min()))
        G = _step(K, n, rep, y, C, QD, alpha, G, i, j, Ki)
        pairs.append((i, j))
        if trace is not None:
            trace.append((alpha.copy(), G.copy()))
    objective = 0.5 * float(alpha @ (G + p))
    return ref.Result(pairs, alpha, G, ref.calculate_rho(y, alpha, C, G), len(pairs), status, objective, float(gmax), float(gmax2))


def calculate_rho_nu(y, alpha, C, G):
    """(rho, r) of Solver_NU::calculate_rho: per sign the mean of G over the free variables in ascending order, else the midpoint
    of the bounds"""
    side = []
    for mask in (y > 0, y < 0):
        upper, lower = mask & (alpha >= C), mask & (alpha < C) & (alpha <= 0)
        free = mask & ~upper & ~lower
        if free.any():
            s = 0.0
            for v in G[free]:
                s = s + float(v)
            side.append(s / int(free.sum()))
        else:
            ub = float(G[lower].min()) if lower.any() else np.inf
            lb = float(G[upper].max()) if upper.any() else -np.inf
            side.append((ub + lb) / 2.0)
    r1, r2 = side
    return (r1 - r2) / 2.0, (r1 + r2) / 2.0


def solve_nu(K, signs, p, C, tol, alpha0, G0, max_steps=None, steps_only=None, trace=None):
    """Solver_NU.  `sides` holds (ip, in) of every step taken (-1: a side without a maximal violator): with `pairs` the rows a step
    requests, in the order ip, in, j."""
    K, n, N, rep, y, p, C, QD, alpha, G = _prepare(K, signs, p, C, alpha0, G0)
    cap = max(10 ** 7, 100 * N) if max_steps is None else max_steps
    pos = y > 0
    pairs, sides, status, gap_p, gap_n = [], [], 'running', -np.inf, -np.inf
    while True:
        up = np.where(pos, alpha < C, alpha > 0)
        low = np.where(pos, alpha > 0, alpha < C)
        upval, lowval = np.where(pos, -G, G), np.where(pos, G, -G)
        up_p, up_n, low_p, low_n = up & pos, up & ~pos, low & pos, low & ~pos
        gmaxp = upval[up_p].max() if up_p.any() else -np.inf
        gmaxn = upval[up_n].max() if up_n.any() else -np.inf
        gmaxp2 = lowval[low_p].max() if low_p.any() else -np.inf
        gmaxn2 = lowval[low_n].max() if low_n.any() else -np.inf
        gap_p, gap_n = gmaxp + gmaxp2, gmaxn + gmaxn2
        if not up.any() or max(gap_p, gap_n) < tol:
            status = 'optimal'
            break
        if len(pairs) >= cap:
            status = 'stopped'
            break
        if steps_only is not None and len(pairs) >= steps_only:
            break
        ip = _last(up_p & (upval == gmaxp)) if up_p.any() else -1
        i_n = _last(up_n & (upval == gmaxn)) if up_n.any() else -1
        zero = np.zeros(N)
        Kp = np.tile(K[ip % n], rep) if ip >= 0 else zero
        Kn = np.tile(K[i_n % n], rep) if i_n >= 0 else zero
        Kside = np.where(pos, Kp, Kn)
        qd_side = np.where(pos, QD[ip] if ip >= 0 else 0.0, QD[i_n] if i_n >= 0 else 0.0)
        grad_diff = np.where(pos, gmaxp, gmaxn) + lowval
        cand = low & (grad_diff > 0)
        if not cand.any():
            status = 'optimal'
            break
        quad = (qd_side + QD) - 2.0 * Kside
        quad = np.where(quad > 0, quad, TAU)
        with np.errstate(invalid='ignore', over='ignore'):
            obj = -((grad_diff * grad_diff) / quad)
        j = _last(cand & (obj == obj[cand].min()))
        i = ip if pos[j] else i_n
        G = _step(K, n, rep, y, C, QD, alpha, G, i, j, Kp if pos[j] else Kn)
        pairs.append((i, j))
        sides.append((ip, i_n))
        if trace is not None:
            trace.append((alpha.copy(), G.copy()))
    rho, r = calculate_rho_nu(y, alpha, C, G)
    return NuResult(pairs, sides, alpha, G, rho, r, len(pairs), status, float(gap_p), float(gap_n))


def solve(rule, *args, **kw):
    return (solve_nu if rule == 'nu' else solve_plain)(*args, **kw)


# ---- the seeded problems of the tests ---------------------------------------------------------------------------------------------------
def one_class_data(n, d):
    """default_rng(0): X standard normal, every 9th row scaled by 3 (the outliers)"""
    X = np.random.default_rng(0).standard_normal((n, d))
    X[::9] *= 3.0
    return X


# name -> (kind, n, d, gamma, nu, C); the nu-SVC / nu-SVR data are smo_rows_reference's svc / svr problems of that size
CASES = {'oc300': ('oc', 300, 5, 0.5, 0.2, 1.0), 'oc1500': ('oc', 1500, 8, 0.2, 0.1, 1.0),
         'nusvc300': ('nusvc', 300, 5, 0.5, 0.3, 1.0), 'nusvc1500': ('nusvc', 1500, 8, 0.2, 0.2, 1.0),
         'nusvr300': ('nusvr', 300, 5, 0.5, 0.5, 1.0), 'nusvr1500': ('nusvr', 1500, 8, 0.2, 0.2, 1.0)}


def case_problem(name):
    """(X, y or None, gamma, (signs, p, C, alpha0, rule)) of a seeded case"""
    kind, n, d, gamma, nu, Cval = CASES[name]
    if kind == 'oc':
        return one_class_data(n, d), None, gamma, one_class_problem(n, nu)
    X, y = ref.seeded('svc' if kind == 'nusvc' else 'svr', n, d)
    return X, y, gamma, nu_svc_problem(y, nu) if kind == 'nusvc' else nu_svr_problem(y, Cval, nu)
