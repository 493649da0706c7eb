"""The held-out scoring kernels of bq_mscore.hip restated in their simplest form (pure NumPy / math, no device): one loop-free
statement per figure, every floating sum taken by math.fsum, so exactly rounded.  Each function takes the downloaded x, the decision
inputs u (one row of K coef per column), the boxes and the labels or targets of ONE column.

    svr_scores    msvr_score_kernel                       b, n_sv, sse, n_held
    svc_scores    mscore_intercept / mheldout_kernel      b, n_sv, dec, lab
    nu_scores     msx_score_kernel<PAIRED>                n_held, n_correct, sse
    (the vote: ovo_decision(...).argmax, which test_gpu_ovo_search._check_against_host already states on the host)

The counts, labels and decision values are compared with ==.  The floating sums are compared with `intercept_bound` and `sse_bound`,
which follow from the arithmetic (their docstrings); nothing in them is measured.

The second half of the file builds the pinned inputs that tests/test_gpu_scoring_edges.py runs on the device and
tests/test_scoring_edges_host.py checks with the CPU oracle first (`svr_case`, `svc_case`): a state is pinned through the box, not
uploaded.  A pinned row is an outlier in feature space (its RBF kernel value to every other row is 0 in fp64) with ub = x0 = c and a
linear term that pushes it outward; ProjectedGradient freezes a coordinate that sits at its bound with the gradient pointing out,
so x stays c bit for bit however many iterations run.
"""
import math

import numpy as np

U53 = 2.0 ** -53
SV = 1e-6                                   # a row is a support vector when x > SV
LO, HI = SV, float(np.nextafter(SV, 1.0))   # the two caps a row is pinned to: not a support vector, a support vector


def _fsum(v):
    return math.fsum(float(t) for t in v)


# ---- the kernels, restated --------------------------------------------------------------------------------------------------------
def svr_scores(x, u, y, ub, eps, b_used=None):
    """msvr_score_kernel for one column: x, ub of 2n entries, u, y of n.  Support rows: x+ or x- above 1e-6.
    b = (fsum(y - u over them) - eps) / n_sv, NaN without one.  Held rows: ub == 0 on BOTH halves (-0.0 is 0).
    sse = fsum((y - (u + b_used))**2 over them); b_used defaults to b — the tests pass the device's b, so that the intercept's
    rounding is not counted a second time in the squared error.  Returns b, n_sv, sse, n_held."""
    n = len(y)
    sv = (x[:n] > SV) | (x[n:] > SV)
    n_sv = int(sv.sum())
    b = (_fsum(y[sv] - u[sv]) - eps) / n_sv if n_sv else math.nan
    held = (ub[:n] == 0) & (ub[n:] == 0)
    used = b if b_used is None else b_used
    sse = _fsum((y[held] - (u[held] + used)) ** 2)
    return b, n_sv, (math.nan if math.isnan(used) else sse), int(held.sum())


def svc_scores(x, u, sgn, ub, b_used=None, pair=None, ct=None, data_row=None):
    """mscore_intercept<false> and mheldout_kernel for one column of n rows.  b = fsum(sgn - u over x > 1e-6) / n_sv, NaN without one.
    dec = u + b_used (default b) and lab = sgn on the held rows (ub == 0), 0 on every other row.  With pair = (a, b), ct (the classes'
    tile rows of 256) and data_row (1: a data row, 0: a ghost row), the held rows are the data rows with ub == 0 of the panel rows of
    classes a and b only.  Returns b, n_sv, dec, lab."""
    n = len(u)
    sv = x > SV
    n_sv = int(sv.sum())
    b = _fsum(sgn[sv] - u[sv]) / n_sv if n_sv else math.nan
    held = ub == 0
    if pair is not None:
        rows = np.arange(n)
        mine = np.zeros(n, dtype=bool)
        for cls in pair:
            mine |= (rows >= 256 * int(ct[cls])) & (rows < min(256 * int(ct[cls + 1]), n))
        held &= mine & (np.asarray(data_row) != 0)
    used = b if b_used is None else b_used
    dec, lab = np.zeros(n), np.zeros(n)
    dec[held] = u[held] + used
    lab[held] = sgn[held]
    return b, n_sv, dec, lab


def nu_scores(x, u, y, ub, r1, r2, paired):
    """msx_score_kernel for one column: rho = (r1 - r2) / 2, scale = (r1 + r2) / 2 from the column's two offsets.  LABELS (ub of n
    entries): the held rows have ub == 0; pred = +1 if (u - rho) / scale > 0 else -1; n_correct counts the held rows with pred == y;
    sse = 0.  PAIRED (ub of 2n): the held rows have ub == 0 on BOTH halves; sse = fsum((y - (u - rho))**2 over them); n_correct = 0.
    x is not read (the kernel reads it through u alone) and may be None.  Returns n_held, n_correct, sse."""
    n = len(u)
    rho, scale = (r1 - r2) / 2, (r1 + r2) / 2
    if paired:
        held = (ub[:n] == 0) & (ub[n:] == 0)
        return int(held.sum()), 0, _fsum((y[held] - (u[held] - rho)) ** 2)
    held = ub == 0
    with np.errstate(divide='ignore', invalid='ignore'):
        pred = np.where((u - rho) / scale > 0, 1., -1.)
    return int(held.sum()), int((pred[held] == y[held]).sum()), 0.


# ---- the bounds -------------------------------------------------------------------------------------------------------------------
def intercept_bound(terms, eps, m):
    """|b_dev - b_ref| <= (m + 3) 2^-53 (fsum |t| + |eps|) / m for b = (sum of the m terms t - eps) / m.

    Both sides sum the same terms (the same bits of y - u).  A floating sum of m terms in any order is within (m - 1) 2^-53 sum |t|
    of the exact one, to first order; that is the device's tree.  The reference's sum is exactly rounded: one unit.  The subtraction
    of eps rounds a number of magnitude <= sum |t| + |eps| and the division rounds the quotient: one unit each, and one to spare.
    Everything is divided by m.  (Both sides round the subtraction and the division, on operands that differ by the sums' error: a
    worst case that counts them on each side comes to m + 4.  The narrower figure is kept; with m <= 2 both sums are one rounding
    of the same exact value and b agrees bit for bit.)"""
    return (m + 3) * U53 * (_fsum(np.abs(terms)) + abs(eps)) / m


def sse_bound(sse_ref, m):
    """|sse_dev - sse_ref| <= (2 m + 4) 2^-53 sse_ref for a sum of m squares.

    Both sides square the same residuals (the same u, y and intercept bits).  The terms are non-negative, so sum |t| is the sum
    itself and the device's order costs (m - 1) units of it.  Each square is rounded on the reference's side and may or may not be
    fused into the add on the device's: at most one unit of the term on each side, 2 units of the sum.  The reference's sum is
    rounded once.  That is (m - 1) + 2 + 1 = m + 2 units of the sum; the bound is twice that."""
    return (2 * m + 4) * U53 * sse_ref


class Ratios:
    """the largest observed difference-to-bound ratios of a run, printed beside every comparison"""
    b = 0.0
    sse = 0.0


def check_intercept(what, b_dev, b_ref, terms, eps, m):
    bound = intercept_bound(terms, eps, m)
    diff = abs(b_dev - b_ref)
    Ratios.b = max(Ratios.b, diff / bound if bound else 0.0)
    print('%s: |b_dev - b_ref| = %.3e (bound %.3e, ratio %.3f; largest so far %.3f)' % (
        what, diff, bound, diff / bound if bound else 0.0, Ratios.b))
    assert diff <= bound, (what, b_dev, b_ref, bound)


def check_sse(what, sse_dev, sse_ref, m):
    bound = sse_bound(sse_ref, m)
    diff = abs(sse_dev - sse_ref)
    Ratios.sse = max(Ratios.sse, diff / bound if bound else 0.0)
    print('%s: |sse_dev - sse_ref| = %.3e (bound %.3e, ratio %.3f; largest so far %.3f)' % (
        what, diff, bound, diff / bound if bound else 0.0, Ratios.sse))
    assert diff <= bound, (what, sse_dev, sse_ref, bound)


# ---- the pinned inputs ------------------------------------------------------------------------------------------------------------
SIZES = (1024, 1025, 2049)   # one trip of the 1024-thread loop, one row into the second, one row into the third
BOX_ITERS, SIMPLEX_ITERS = 40, 60
SVR_GAMMA, SVC_GAMMA = 0.1, 1.0 / 3


def folds(n):
    """The held rows of a case's columns: two interleaved folds (i % 3 == 0, 1) and, past n = 1024, the block [1024, n)."""
    idx = np.arange(n)
    out = [idx[idx % 3 == 0], idx[idx % 3 == 1]]
    if n > 1024:
        out.append(idx[1024:])
    return out


def pin_rows(n, kinds):
    """Two rows per kind, all with i % 3 == 2 (no interleaved fold above holds them) except row 1024 of n = 1025, the only row past
    1024 there.  The second row of every kind has index >= 1024 where n allows: at n = 2049 they include row 2048, the one row of the
    third trip; at n = 1025 row 1024 takes the LAST kind, a support vector.  Returns [(row, kind)]."""
    k = len(kinds)
    low = [2 + 3 * j for j in range(2 * k)]
    if n >= 2049:
        high = [1025 + 3 * j for j in range(k - 1)] + [2048]
        rows = low[:k] + high
    elif n > 1024:
        rows = low[:2 * k - 1] + [1024]
    else:
        rows = low
    return [(r, kinds[j % k]) for j, r in enumerate(rows)]


def _outliers(X, rows, gamma):
    """X with the rows `rows` moved far out along the first axis: 40 / sqrt(gamma) and more from every other row and from each
    other, so exp(-gamma d^2) <= exp(-1600) = 0 in fp64"""
    X = X.copy()
    step = 40.0 / math.sqrt(gamma) + 2.0 * float(np.linalg.norm(X, axis=1).max())
    for j, r in enumerate(rows):
        X[r] = 0.
        X[r, 0] = (j + 1) * step
    return X


SVR_KINDS = (('+', LO), ('-', LO), ('-', HI), ('+', HI))   # the pinned half and its cap; the other half stays at 0 in a box of C
NO_SV_EPS = 100.0 * 50.0                                  # far above max |y|: the linear term is positive everywhere


def svr_case(n):
    """The SVR input of size n: X, y of test_gpu_svr_cv._data(n) with the pinned rows moved out and their targets set to +-50 (a '+'
    row's x+ wants to grow, a '-' row's x-), and per column (C, eps, held rows): the folds of `folds(n)` and last a column that holds
    out i % 3 == 2, starts at 0 with eps = NO_SV_EPS and so ends without a support vector.  A pin is in force in the columns that do
    not hold its row out.  Column 0 has a -0.0 box pair on held row 3 and (+0.0, -0.0) on held row 6.
    Returns dict(X, y, QL, UB, eps, x0, pins (per column [(row, half, cap)]), held, empty)."""
    from test_gpu_svr_cv import _data
    X, y = _data(n)
    pins = pin_rows(n, SVR_KINDS)
    X = _outliers(X, [r for r, _ in pins], SVR_GAMMA)
    y = y.copy()
    for r, (half, _) in pins:
        y[r] = 50. if half == '+' else -50.
    helds = folds(n) + [np.arange(n)[np.arange(n) % 3 == 2]]
    params = [(1.0, 0.1), (0.5, 0.05), (2.0, 0.2)][:len(helds) - 1] + [(1.0, NO_SV_EPS)]
    empty = len(helds) - 1
    QL, UB, X0, col_pins = [], [], [], []
    for c, (held, (C_, e)) in enumerate(zip(helds, params)):
        ub = np.full(2 * n, C_)
        ub[held] = 0.
        ub[n + held] = 0.
        x0 = ub / 2
        mine = []
        for r, (half, cap) in pins:
            if ub[r] == 0 or c == empty:
                continue
            at, other = (r, n + r) if half == '+' else (n + r, r)
            ub[at], x0[at], x0[other] = cap, cap, 0.
            mine.append((r, half, cap))
        if c == 0:
            ub[3], ub[n + 3], ub[n + 6] = -0.0, -0.0, -0.0
        if c == empty:
            x0[:] = 0.
        QL.append(np.hstack((-y, y)) + e)
        UB.append(ub)
        X0.append(x0)
        col_pins.append(mine)
    return dict(X=X, y=y, QL=np.stack(QL), UB=np.stack(UB), eps=np.array([e for _, e in params]), x0=np.stack(X0), pins=col_pins,
                held=helds, empty=empty)


SVC_KINDS = (LO, HI)
SVC_PUSH = -1e4


def svc_case(n):
    """The SVC input of size n: X and labels of test_gpu_nu._data(n, 23) with the pinned rows moved out, and per column (C, held
    rows): the folds of `folds(n)` and last a column on all rows that feeds no calibrator.  The dual's Hessian is (K + 1) o yy', so a
    pinned row's gradient is 2 x_i + q_i + y_i s with s the sum of y_j x_j over the other rows.  ProjectedGradient's s swings between
    about -20 and +20 on this data, so the usual q_i = -1 does not hold the row at its cap; the problem's linear term is the test's to
    choose, and q_i = SVC_PUSH = -1e4 does: |s| <= sum ub <= 2 x 2049 for every point of the box, so the gradient points outward
    whatever the other rows do.  The scoring kernels do not read q.  Column 0 has a -0.0 box on held row 3.
    The interleaved folds share calibrator 0.  The block fold overlaps them (every third row of [1024, n) is in both), and columns of
    one calibrator must hold out disjoint rows, so it feeds calibrator 1 of its own.
    Returns dict(X, q, Y, UB, x0, cal_of, ncal, pins (per column [(row, cap)]), held, empty (None))."""
    from test_gpu_nu import _data
    X, y, _ = _data(n, 23)
    pins = pin_rows(n, SVC_KINDS)
    X = _outliers(X, [r for r, _ in pins], SVC_GAMMA)
    y = y.copy()
    q = -np.ones(n)
    q[[r for r, _ in pins]] = SVC_PUSH
    helds = folds(n) + [np.arange(0)]
    Cs = [1.0, 0.5, 2.0][:len(helds) - 1] + [1.0]
    UB, X0, col_pins = [], [], []
    for c, (held, C_) in enumerate(zip(helds, Cs)):
        ub = np.full(n, C_)
        ub[held] = 0.
        x0 = ub / 2
        mine = []
        for r, cap in pins:
            if ub[r] == 0:
                continue
            ub[r], x0[r] = cap, cap
            mine.append((r, cap))
        if c == 0:
            ub[3] = -0.0
        UB.append(ub)
        X0.append(x0)
        col_pins.append(mine)
    cal_of = np.array([0, 0, 1, -1] if n > 1024 else [0, 0, -1], dtype=np.int32)
    return dict(X=X, q=q, Y=np.tile(y, (len(helds), 1)), UB=np.stack(UB), x0=np.stack(X0), cal_of=cal_of, ncal=2 if n > 1024 else 1,
                pins=col_pins, held=helds, empty=None)


def half_zero_rows(n):
    """The extra rows of the PAIRED column 0 (which holds out i % 3 == 0; these have i % 3 == 1): ub = 0 on the first half only, and
    on the second half only; one of each past 1024 where n allows.  None of them is held out."""
    if n >= 2049:
        return [1, 1027], [4, 1030]
    if n > 1024:
        return [1, 1024], [4, 7]
    return [1, 7], [4, 10]
