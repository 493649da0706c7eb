"""NumPy restatement of the row-based SMO (optiml_amd/csrc/bq_rsmo.hip, scalar rules in csrc/bq_rsmo_step.h): libsvm's Solver::Solve
without shrinking (svm.cpp) on

    min 1/2 a'Qa + p'a,   y'a = 0,   0 <= a_t <= C_t,   Q_st = y_s y_t K_st

    SVC: p = -1, y the labels;  SVR: 2n variables [alpha; alpha*], p = [eps - y; eps + y], signs [+1 ..; -1 ..], the variables t and
    t + n share kernel row t (SVR_Q).

Start alpha = 0, G = p.  select_working_set is WSS2 with TAU = 1e-12 and ties to the LARGER index (libsvm's `>=` / `<=` scans), the
update has both clipping cascades in libsvm's order, the gradient takes G_t + (Q_it d_i + Q_jt d_j) — two rounded products, their
rounded sum, one rounded add; NumPy's element-wise loops fuse nothing — and calculate_rho sums the free variables in ascending
order.  The device solver and the host program around bq_rsmo_step.h are held to this file bit for bit, this file to sklearn's libsvm
(tests/test_smo_rows_host.py).
"""
import collections

import numpy as np

TAU = 1e-12
Result = collections.namedtuple('Result', 'pairs alpha G rho steps status objective gmax gmax2')


def svc_problem(y, boxes):
    """(signs, p, C) of the SVC dual"""
    y = np.asarray(y, dtype=float)
    return y.copy(), -np.ones(len(y)), np.asarray(boxes, dtype=float).copy()


def svr_problem(y, boxes, epsilon):
    """(signs, p, C) of the SVR dual on 2n variables"""
    y = np.asarray(y, dtype=float)
    n = len(y)
    boxes = np.asarray(boxes, dtype=float)
    return (np.concatenate((np.ones(n), -np.ones(n))), np.concatenate((epsilon - y, epsilon + y)),
            np.concatenate((boxes, boxes)))


def _last(mask):
    """the largest index at which mask holds"""
    return len(mask) - 1 - int(np.argmax(mask[::-1]))


def pair_update(y_i, y_j, G_i, G_j, qd_i, qd_j, k_ij, C_i, C_j, a_i, a_j):
    quad = (qd_i + qd_j) - 2.0 * k_ij
    if not quad > 0:
        quad = TAU
    if y_i != y_j:
        delta = (-G_i - G_j) / quad
        diff = a_i - a_j
        a_i = a_i + delta
        a_j = a_j + delta
        if diff > 0:
            if a_j < 0:
                a_j, a_i = 0.0, diff
        else:
            if a_i < 0:
                a_i, a_j = 0.0, -diff
        if diff > C_i - C_j:
            if a_i > C_i:
                a_i, a_j = C_i, C_i - diff
        else:
            if a_j > C_j:
                a_j, a_i = C_j, C_j + diff
    else:
        delta = (G_i - G_j) / quad
        tot = a_i + a_j
        a_i = a_i - delta
        a_j = a_j + delta
        if tot > C_i:
            if a_i > C_i:
                a_i, a_j = C_i, tot - C_i
        else:
            if a_j < 0:
                a_j, a_i = 0.0, tot
        if tot > C_j:
            if a_j > C_j:
                a_j, a_i = C_j, tot - C_j
        else:
            if a_i < 0:
                a_i, a_j = 0.0, tot
    return a_i, a_j


def calculate_rho(y, alpha, C, G):
    yG = np.where(y > 0, G, -G)
    upper, lower = alpha >= C, alpha <= 0
    free = ~upper & ~lower
    if free.any():
        s = 0.0
        for v in yG[free]:
            s = s + float(v)
        return s / int(free.sum())
    ub_set = (upper & (y < 0)) | (~upper & lower & (y > 0))
    lb_set = (upper & (y > 0)) | (~upper & lower & (y < 0))
    ub = float(yG[ub_set].min()) if ub_set.any() else np.inf
    lb = float(yG[lb_set].max()) if lb_set.any() else -np.inf
    return (ub + lb) / 2.0


def solve(K, signs, p, C, tol, max_steps=None, steps_only=None, trace=None):
    """K: n x n kernel rows as the solver sees them.  max_steps: the iteration cap (libsvm: max(10^7, 100 N)); steps_only: stop
    after that many updates without a verdict (status 'running'), for step-for-step comparisons; trace: a list that receives
    (alpha, G) after every update."""
    K = np.asarray(K, dtype=float)
    n, N = len(K), len(signs)
    assert N in (n, 2 * n) and K.shape == (n, n)
    rep = N // n
    y = np.asarray(signs, dtype=float)
    p = np.asarray(p, dtype=float)
    C = np.asarray(C, dtype=float)
    QD = np.tile(np.diag(K).copy(), rep)
    alpha, G = np.zeros(N), p.copy()
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
        best = obj[cand].min()
        j = _last(cand & (obj == best))
        Kj = Ki if j % n == i % n else np.tile(K[j % n], rep)
        old_i, old_j = float(alpha[i]), float(alpha[j])
        a_i, a_j = pair_update(float(y[i]), float(y[j]), float(G[i]), float(G[j]), float(QD[i]), float(QD[j]), float(Ki[j]),
                               float(C[i]), float(C[j]), old_i, old_j)
        alpha[i], alpha[j] = a_i, a_j
        d_i, d_j = a_i - old_i, a_j - old_j
        Q_i, Q_j = (y[i] * y) * Ki, (y[j] * y) * Kj
        G = G + ((Q_i * d_i) + (Q_j * d_j))
        pairs.append((i, j))
        if trace is not None:
            trace.append((alpha.copy(), G.copy()))
    objective = 0.5 * float(alpha @ (G + p))
    return Result(pairs, alpha, G, calculate_rho(y, alpha, C, G), len(pairs), status, objective, float(gmax), float(gmax2))


# ---- the seeded problems of the tests ---------------------------------------------------------------------------------------------
def rbf(X, gamma):
    sq = (X * X).sum(axis=1)
    D = np.maximum(sq[:, None] + sq[None, :] - 2.0 * (X @ X.T), 0.0)
    np.fill_diagonal(D, 0.0)
    return np.exp(-gamma * D)


def seeded(task, n, d):
    """default_rng(0): X standard normal, then the noise; SVC labels sign(x0 x1 + 0.3 noise), SVR targets sin x0 + 0.1 noise"""
    rng = np.random.default_rng(0)
    X = rng.standard_normal((n, d))
    noise = rng.standard_normal(n)
    if task == 'svc':
        y = np.where(X[:, 0] * X[:, 1] + 0.3 * noise > 0, 1.0, -1.0)
    else:
        y = np.sin(X[:, 0]) + 0.1 * noise
    return X, y


# (task, n, d, gamma, C): the cases of the issue; epsilon = 0.1 for SVR
CASES = {'svc300': ('svc', 300, 5, 0.5, 1.0), 'svc1500': ('svc', 1500, 8, 0.2, 10.0),
         'svr300': ('svr', 300, 5, 0.5, 1.0), 'svr1500': ('svr', 1500, 8, 0.2, 10.0)}
EPSILON = 0.1
CLASS_WEIGHT = {1.0: 5.0, -1.0: 1.0}   # the weighted case: the svc300 problem with these class weights


def case_problem(name, weighted=False):
    """(X, y, gamma, signs, p, C) of a seeded case"""
    task, n, d, gamma, Cval = CASES[name]
    X, y = seeded(task, n, d)
    boxes = np.full(n, Cval)
    if weighted:
        assert task == 'svc'
        boxes = Cval * np.where(y > 0, CLASS_WEIGHT[1.0], CLASS_WEIGHT[-1.0])
    signs, p, C = svc_problem(y, boxes) if task == 'svc' else svr_problem(y, boxes, EPSILON)
    return X, y, gamma, signs, p, C
