"""NumPy reference of the batched Platt fit (bq_platt.hip) and the inputs the calibration tests share.

`platt_reference` is libsvm's sigmoid_train (Lin, Lin & Weng 2007), statement for statement, with NumPy sums: the targets
(N+ + 1) / (N+ + 2) and 1 / (N- + 2), the start A = 0, B = log((N- + 1) / (N+ + 1)), sigma = 1e-12 on the Hessian's diagonal, the
stop test |g_A|, |g_B| < 1e-5, the step halved while f_new >= f + 1e-4 step g'd down to 1e-10, at most 100 iterations, and the loss
in the branch-stable form.  It also reports what the tests need to know about an input: how often a step was halved and how close
a gradient entry came to the stop value without being on the other side of it.
"""
import numpy as np

LINE_SEARCH, MAX_ITER, EMPTY = 1, 2, 4
STOP = 1e-5


def _loss(f, t, A, B):
    z = f * A + B
    pos = z >= 0
    out = np.empty_like(z)
    out[pos] = t[pos] * z[pos] + np.log1p(np.exp(-z[pos]))
    out[~pos] = (t[~pos] - 1.) * z[~pos] + np.log1p(np.exp(z[~pos]))
    return float(out.sum())


def platt_reference(f, labels):
    """dict(A, B, iters, loss, n_pos, n_neg, flags, halvings, stop_ratio, search_margin, cond) of one calibrator; rows with label 0 are not in the
    sample.  stop_ratio: over every stop test taken, the largest min(g, STOP) / max(g, STOP) of the larger gradient entry g, which
    decides the test; a value below 1 / 1.1 says no test was decided by less than a factor 1.1.  search_margin: over every
    line-search test, the smallest distance of the new loss from the acceptance bound, relative to the loss.  cond: the largest
    condition number of the 2 x 2 Hessians."""
    f = np.asarray(f, dtype=float)
    labels = np.asarray(labels, dtype=float)
    keep = labels != 0
    f, labels = f[keep], labels[keep]
    n_pos, n_neg = int((labels > 0).sum()), int((labels < 0).sum())
    if n_pos + n_neg == 0:
        return dict(A=0., B=0., iters=0, loss=0., n_pos=0, n_neg=0, flags=EMPTY, halvings=0, stop_ratio=0., cond=1., search_margin=np.inf)
    t = np.where(labels > 0, (n_pos + 1.) / (n_pos + 2.), 1. / (n_neg + 2.))
    A, B = 0., float(np.log((n_neg + 1.) / (n_pos + 1.)))
    fval = _loss(f, t, A, B)
    flags, halvings, ratio, cond, margin = 0, 0, 0., 1., np.inf
    it = 0
    while it < 100:
        z = f * A + B
        e = np.exp(-np.abs(z))
        p = np.where(z >= 0, e / (1. + e), 1. / (1. + e))
        q = np.where(z >= 0, 1. / (1. + e), e / (1. + e))
        d2 = p * q
        d1 = t - p
        h11 = 1e-12 + float((f * f * d2).sum())
        h22 = 1e-12 + float(d2.sum())
        h21 = float((f * d2).sum())
        g1, g2 = float((f * d1).sum()), float(d1.sum())
        cond = max(cond, float(np.linalg.cond(np.array([[h11, h21], [h21, h22]]))))
        gmax = max(abs(g1), abs(g2))   # the test stops exactly when the larger entry is below STOP
        ratio = max(ratio, min(gmax, STOP) / max(gmax, STOP))
        if abs(g1) < STOP and abs(g2) < STOP:
            break
        det = h11 * h22 - h21 * h21
        dA = -(h22 * g1 - h21 * g2) / det
        dB = -(-h21 * g1 + h11 * g2) / det
        gd = g1 * dA + g2 * dB
        step = 1.
        while step >= 1e-10:
            newA, newB = A + step * dA, B + step * dB
            newf = _loss(f, t, newA, newB)
            margin = min(margin, abs(newf - (fval + 1e-4 * step * gd)) / max(abs(fval), abs(newf)))
            if newf < fval + 1e-4 * step * gd:
                A, B, fval = newA, newB, newf
                break
            step /= 2.
            halvings += 1
        if step < 1e-10:
            flags |= LINE_SEARCH
            break
        it += 1
    if it >= 100:
        flags |= MAX_ITER
    return dict(A=A, B=B, iters=it, loss=fval, n_pos=n_pos, n_neg=n_neg, flags=flags, halvings=halvings, stop_ratio=ratio,
                cond=cond, search_margin=margin)


NOISY_N = (37, 300, 1000, 1025, 2049)
EDGE_CASES = ('separated', 'margin', 'inverted', 'tiny', 'one-class')


def noisy_input(n):
    rng = np.random.default_rng(n)
    y = np.where(rng.random(n) < 0.4, 1., -1.)
    return 0.8 * y + rng.standard_normal(n), y


def edge_input(case):
    n = 300
    rng = np.random.default_rng(5)
    y = np.where(np.arange(n) % 3 == 0, 1., -1.)
    if case == 'separated':
        return y * (20. + 30. * rng.random(n)), y
    if case == 'margin':
        return y * (1. + rng.random(n)), y
    if case == 'inverted':
        return -0.8 * y + rng.standard_normal(n), y
    if case == 'tiny':
        return 1e-3 * (0.8 * y + rng.standard_normal(n)), y
    if case == 'one-class':
        return rng.standard_normal(n) - 1., -np.ones(n)
    raise KeyError(case)


def masked_input():
    """the noisy input of n = 1000 with every second label set to 0"""
    f, y = noisy_input(1000)
    y = y.copy()
    y[1::2] = 0.
    return f, y


def backtracking_candidate(seed):
    """A strongly bimodal f with a few mislabelled extremes: f = y (c + N(0,1)), c in [2, 10), and 1 to 3 rows moved to the wrong
    side and stretched by a factor in [1, 30); n in [20, 300)."""
    rng = np.random.default_rng(seed)
    n = int(rng.integers(20, 300))
    y = np.where(rng.random(n) < rng.uniform(0.1, 0.9), 1., -1.)
    f = y * (rng.uniform(2, 10) + rng.standard_normal(n))
    wrong = rng.choice(n, int(rng.integers(1, 4)), replace=False)
    f[wrong] = -f[wrong] * rng.uniform(1, 30)
    return f, y


# seeds of backtracking_candidate at which the reference halves a step twice, no stop test is decided by less than a factor 2 and
# every line-search test by more than 1e-9 of the loss (a search of 2000 seeds finds 47 inputs that halve a step at all)
BACKTRACK_SEEDS = (66, 490)


# Measured on an MI355X (profiles/calibration/platt_parity.json) and taken 16-fold (the headroom is for another compiler's exp /
# log1p).  PLATT: the largest relative deviation of A, B and the loss of the device fit from `platt_reference` over every input
# above.  DECISION: the largest deviation of the batched columns' decision values from single fits', relative to the largest value.
PLATT_MEASURED = 3.4326207965759507e-16
DECISION_MEASURED = 2.9381973403307334e-12
PLATT_RTOL = 16 * PLATT_MEASURED
DECISION_RTOL = 16 * DECISION_MEASURED

# A line-search test compares two losses, each a sum of m positive terms: a term carries a few roundings (exp, log1p, a product, a
# sum), a tree or pairwise sum log2(m) more, so two correct evaluations of one loss differ by at most about (4 + log2 m) 2^-53 of it
# — 16 2^-53 for the m <= 2049 used here — and the two sides of a test together by twice that.  A test whose reference margin
# (`search_margin`, relative to the loss) is above this cannot be decided differently by rounding.
SEARCH_MARGIN = 32 * 2.0 ** -53
