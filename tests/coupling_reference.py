"""NumPy restatement of the pairwise-coupling kernel (bq_couple.hip) and the inputs the coupling tests share.

`coupling_reference` is libsvm's multiclass_probability (svm.cpp; Wu, Lin & Weng 2004, second method), statement for statement,
on Python floats: every product and sum is one IEEE operation, every sum sequential in ascending index, no fused multiply-add —
the order of operations the kernel is specified by.  Its input is the clipped pair probabilities s (P entries in `ovo_pairs`
order; column q = (a, b), a < b, has class b positive: r[b][a] = s, r[a][b] = 1 - s), which the kernel hands back as R, so the
comparison does not depend on either side's exp.
"""
import numpy as np

CLIP = 1e-7
KMAX = 64


def pairs(k):
    return [(a, b) for a in range(k) for b in range(a + 1, k)]


def sigmoid(F, A, B):
    """the clipped pair probabilities of decision values F (.. x P) under the sigmoids A, B, in the overflow-free form"""
    z = np.asarray(F, dtype=float) * np.asarray(A, dtype=float) + np.asarray(B, dtype=float)
    e = np.exp(-np.abs(z))
    s = np.where(z >= 0, e / (1. + e), 1. / (1. + e))
    return np.minimum(np.maximum(s, CLIP), 1. - CLIP)


def coupling_reference(s, k):
    """(p, iters, stop_margin) of one test point.  iters: the sweeps taken (max(100, k) when the cap was reached); stop_margin:
    the smallest |max_error - eps| / eps over the stop tests taken — a point whose margin is far above rounding takes the same
    number of sweeps under any correct evaluation."""
    s = [float(v) for v in s]
    r = [[0.] * k for _ in range(k)]
    for q, (a, b) in enumerate(pairs(k)):
        r[b][a] = s[q]
        r[a][b] = 1. - s[q]
    p = [1. / k] * k
    Q = [[0.] * k for _ in range(k)]
    for t in range(k):
        for j in range(k):
            if j != t:
                Q[t][t] += r[j][t] * r[j][t]
                Q[t][j] = -r[j][t] * r[t][j]
    eps = 0.005 / k
    max_iter = max(100, k)
    Qp = [0.] * k
    margin = np.inf
    it = 0
    while it < max_iter:
        pQp = 0.
        for t in range(k):
            Qp[t] = 0.
            for j in range(k):
                Qp[t] += Q[t][j] * p[j]
            pQp += p[t] * Qp[t]
        max_error = 0.
        for t in range(k):
            error = abs(Qp[t] - pQp)
            if error > max_error:
                max_error = error
        margin = min(margin, abs(max_error - eps) / eps)
        if max_error < eps:
            break
        for t in range(k):
            diff = (-Qp[t] + pQp) / Q[t][t]
            p[t] += diff
            pQp = (pQp + diff * (diff * Q[t][t] + 2. * Qp[t])) / (1. + diff) / (1. + diff)
            for j in range(k):
                Qp[j] = (Qp[j] + diff * Q[t][j]) / (1. + diff)
                p[j] /= (1. + diff)
        it += 1
    return np.array(p), it, float(margin)


def couple_rows(S, k):
    """`coupling_reference` of every row of S (t x P) at once: (prob t x k, iters t, stop margins t).  The same statements with a
    NumPy vector over the points in place of each scalar — an elementwise NumPy operation is the scalar one per element, so a
    point's bits are `coupling_reference`'s (test_coupling_host.py asserts it); a point that has stopped leaves the vectors."""
    S = np.atleast_2d(np.asarray(S, dtype=float))
    n = len(S)
    r = np.zeros((k, k, n))
    for q, (a, b) in enumerate(pairs(k)):
        r[b, a] = S[:, q]
        r[a, b] = 1. - S[:, q]
    Q = np.zeros((k, k, n))
    for t in range(k):
        for j in range(k):
            if j != t:
                Q[t, t] += r[j, t] * r[j, t]
                Q[t, j] = -r[j, t] * r[t, j]
    eps = 0.005 / k
    max_iter = max(100, k)
    prob, iters, margin = np.empty((n, k)), np.full(n, max_iter, dtype=np.int32), np.full(n, np.inf)
    idx = np.arange(n)   # the points still iterating; p, Qp, Q hold their columns only
    p = np.full((k, n), 1. / k)
    for it in range(max_iter + 1):
        if it == max_iter or not len(idx):
            break
        Qp = np.zeros((k, len(idx)))
        pQp = np.zeros(len(idx))
        for t in range(k):
            for j in range(k):
                Qp[t] += Q[t, j] * p[j]
            pQp += p[t] * Qp[t]
        max_error = np.zeros(len(idx))
        for t in range(k):
            error = np.abs(Qp[t] - pQp)
            max_error = np.where(error > max_error, error, max_error)
        margin[idx] = np.minimum(margin[idx], np.abs(max_error - eps) / eps)
        stop = max_error < eps
        prob[idx[stop]] = p[:, stop].T
        iters[idx[stop]] = it
        idx, p, Qp, pQp, Q = idx[~stop], p[:, ~stop], Qp[:, ~stop], pQp[~stop], Q[:, :, ~stop]
        for t in range(k):
            diff = (-Qp[t] + pQp) / Q[t, t]
            p[t] += diff
            pQp = (pQp + diff * (diff * Q[t, t] + 2. * Qp[t])) / (1. + diff) / (1. + diff)
            for j in range(k):
                Qp[j] = (Qp[j] + diff * Q[t, j]) / (1. + diff)
                p[j] /= (1. + diff)
    prob[idx] = p.T   # the cap
    return prob, iters, margin


# ---- the shared inputs: the target pair probabilities of the kernel tests -----------------------------------------------------------
CLASSES = (2, 3, 7, 33, 64)
POINTS = (1, 63, 64, 65, 257)
FAMILIES = ('uniform', 'half', 'clipped', 'dominant')
SAFE_MARGIN = 1e-9   # points whose stop tests are all decided by more than this (relative) are compared
SAFE_SHARE = 0.95    # and at least this share of every case's points must be such


def target_probabilities(family, k, t, seed=0):
    """t x P pair probabilities: uniform random; all 0.5 (stops in sweep 0 with p = 1 / k); every entry at a clip value (both
    values, at random); one dominant class per point (it wins its pairs with 0.9 to 0.99, the rest are uniform)."""
    P = k * (k - 1) // 2
    rng = np.random.default_rng([seed, k, t, FAMILIES.index(family)])
    if family == 'uniform':
        return rng.uniform(0.01, 0.99, (t, P))
    if family == 'half':
        return np.full((t, P), 0.5)
    if family == 'clipped':
        return np.where(rng.random((t, P)) < 0.5, CLIP, 1. - CLIP)
    if family == 'dominant':
        S = rng.uniform(0.2, 0.8, (t, P))
        top = rng.integers(0, k, t)
        for q, (a, b) in enumerate(pairs(k)):
            win = rng.uniform(0.9, 0.99, t)
            S[:, q] = np.where(top == b, win, np.where(top == a, 1. - win, S[:, q]))
        return S
    raise KeyError(family)


def decision_values(S):
    """F with sigmoid(F, -1, 0) = S up to rounding: s = 1 / (1 + exp(-f)), f = log(s / (1 - s)); the clip values are overshot so
    that the clip decides them"""
    S = np.asarray(S, dtype=float)
    F = np.log(S / (1. - S))
    return np.where(S <= CLIP, -40., np.where(S >= 1. - CLIP, 40., F))


# Measured on an MI355X (profiles/coupling/parity.json) and taken 16-fold, as platt_reference does (the headroom is for another
# compiler's exp).  The coupling itself is compared bit for bit and has no bound.  SIGMOID: the largest relative deviation of the
# device's clipped s (R) from `sigmoid` over the kernel tests' inputs.  AB, PROBA: the largest relative deviations of the batched
# estimator's probA_ / probB_ and of its predict_proba on 50 fresh rows from its loop path's, over the estimator tests'
# configurations.
SIGMOID_MEASURED = 3.130859919789007e-16
AB_MEASURED = 1.1949771949766719e-13
PROBA_MEASURED = 2.2622933145389298e-13
SIGMOID_RTOL = 16 * SIGMOID_MEASURED
AB_RTOL = 16 * AB_MEASURED
PROBA_RTOL = 16 * PROBA_MEASURED
