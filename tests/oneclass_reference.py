"""NumPy restatement of the nu-one-class solver (test infrastructure, like platt_reference.py): the Euclidean projection onto a
capped simplex {0 <= p <= u, sum p = r}, exact by sorted breakpoints, the nonmonotone spectral projected-gradient loop around
it, and libsvm's offset rho.  The device code (csrc/bq_simplex.hip) follows the same statements; the tests hold it against this
file.
"""
import numpy as np


def project(v, u, r):
    """P(v) = clip(v - tau, 0, u) with tau a root of phi(tau) = sum clip(v_i - tau, 0, u_i) = r, in the dtype of v (float64 or
    np.longdouble).  phi is piecewise linear and non-increasing with breakpoints v_i and v_i - u_i (rows with u_i > 0): they are
    sorted, phi is evaluated at every one by cumulative sums, and tau is the root of the one linear piece that crosses r.  The
    result is clipped by comparison with the breakpoints, so 0 <= P <= u holds bitwise and P_i = 0 where u_i = 0.  r >= sum u
    returns u itself."""
    v = np.asarray(v)
    dt = np.longdouble if v.dtype == np.longdouble else np.float64
    v = v.astype(dt)
    u = np.asarray(u).astype(dt)
    r = dt(r)
    act = u > 0
    P = np.zeros_like(v)
    if not act.any():
        return P
    va, ua = v[act], u[act]
    if r >= ua.sum():
        P[act] = ua
        return P
    lo_bp = va - ua
    bp = np.unique(np.concatenate((va, lo_bp)))   # ascending
    # phi at every breakpoint t: sum over rows of clip(v - t, 0, u) = sum_{lo_bp >= t} u + sum_{lo_bp < t < v} (v - t)
    vs, ls = np.sort(va), np.sort(lo_bp)
    us_by_l = ua[np.argsort(lo_bp, kind='stable')]
    cu = np.concatenate(([0], np.cumsum(us_by_l)))             # sum of u over the j smallest lo_bp
    cv, cl = np.concatenate(([0], np.cumsum(vs))), np.concatenate(([0], np.cumsum(ls)))
    n_l_lt = np.searchsorted(ls, bp, side='left')              # rows with lo_bp < t
    n_v_le = np.searchsorted(vs, bp, side='right')             # rows with v <= t
    sat = cu[-1] - cu[n_l_lt]                                  # rows with lo_bp >= t: u
    # rows with lo_bp < t: (v - t) if v > t else 0; every row with v <= t has lo_bp < t
    free_cnt = n_l_lt - n_v_le
    # sum of v over rows with lo_bp < t and v > t = (sum v over lo_bp < t) - (sum v over v <= t); v over lo_bp < t = lo_bp + u
    free_v = (cl[n_l_lt] + cu[n_l_lt]) - cv[n_v_le]
    phi = sat + free_v - free_cnt * bp
    # phi is non-increasing along bp: the piece [bp[j], bp[j + 1]] with phi[j] >= r > phi[j + 1]
    j = int(np.searchsorted(-phi, -r, side='right')) - 1
    j = min(max(j, 0), len(bp) - 2)
    # on the open piece the free rows are those with lo_bp <= bp[j] and v >= bp[j + 1]
    free = (lo_bp <= bp[j]) & (va >= bp[j + 1])
    cnt = int(free.sum())
    # tau = bp[j] + delta is never rounded into one number: a free row is (v - bp[j]) - delta, a difference of neighbours first.
    # (After a step of 1e10 along a direction of non-positive curvature v is of the order 1e12 and v - fl(tau) would carry
    # ulp(1e12) = 1e-4 into P and into sum P.)
    delta = dt(0)
    if cnt > 0:
        s_free = (va[free] - bp[j]).sum()
        s_sat = ua[lo_bp >= bp[j + 1]].sum()
        delta = ((s_free + s_sat) - r) / cnt
        delta = min(max(delta, dt(0)), bp[j + 1] - bp[j])
    Pa = np.where(va <= bp[j], 0, np.where(lo_bp >= bp[j + 1], ua, np.minimum(np.maximum((va - bp[j]) - delta, 0), ua)))
    P[act] = Pa
    return P


def violation(x, g, u):
    """libsvm's maximal-violating-pair measure of the one-class dual at x: max_{x_i > 0} g_i - min_{x_i < u_i} g_i over the rows
    with u_i > 0 (-inf when either set is empty)."""
    A = (u > 0) & (x > 0)
    B = (u > 0) & (x < u)
    if not A.any() or not B.any():
        return -np.inf
    return float(g[A].max() - g[B].min())


def solve(K, u, r, tol=1e-3, max_iter=1000, x0=None):
    """min 1/2 x'Kx over {0 <= x <= u, sum x = r}: the loop of the issue, statement for statement.  Returns a dict: x, g, status,
    iter, rows (one (it, f, viol, alpha, s) per record)."""
    K = np.asarray(K, dtype=float)
    u = np.asarray(u, dtype=float)
    n = len(u)
    x = project(np.zeros(n), u, r) if x0 is None else np.array(x0, dtype=float)
    g = K @ x
    f = 0.5 * float(x @ g)
    s, alpha = 1.0, 0.0
    last = [f]
    rows = []
    it = 0
    while True:
        viol = violation(x, g, u)
        rows.append((it, f, viol, alpha, s))
        if viol <= tol:
            status = 'optimal'
            break
        if it == max_iter:
            status = 'stopped'
            break
        d = project(x - s * g, u, r) - x
        gd = float(g @ d)
        if gd >= 0:
            status = 'optimal'
            break
        Qd = K @ d
        dQd = float(d @ Qd)
        if f + gd + 0.5 * dQd <= max(last) + 1e-4 * gd:
            alpha = 1.0
        else:
            alpha = -gd / dQd
        f = f + (alpha * gd + 0.5 * alpha * alpha * dQd)
        x = x + alpha * d
        g = g + alpha * Qd
        last = (last + [f])[-10:]
        s = min(max(float(d @ d) / dQd, 1e-10), 1e10) if dQd > 0 else 1e10
        it += 1
    return dict(x=x, g=g, status=status, iter=it, rows=np.array(rows, dtype=float), f=f)


def rho(x, g, u):
    """libsvm's calculate_rho over the rows with u_i > 0, exact comparisons: the mean of g over the free rows (0 < x_i < u_i),
    summed in index order; without a free row the midpoint of min_{x_i = 0} g_i and max_{x_i = u_i} g_i.  Returns (rho, n_sv,
    n_free)."""
    act = u > 0
    free = act & (x > 0) & (x < u)
    n_sv = int((act & (x > 0)).sum())
    n_free = int(free.sum())
    if n_free:
        s = 0.0
        for gi in g[free]:
            s += float(gi)
        return s / n_free, n_sv, n_free
    lo = g[act & (x == 0)]
    up = g[act & (x == u)]
    ub = float(lo.min()) if len(lo) else np.inf
    lb = float(up.max()) if len(up) else -np.inf
    return (ub + lb) / 2, n_sv, n_free


def fit(K, nu, tol=1e-3, max_iter=1000):
    """OneClassSVM on the Gram matrix K in libsvm's scaling: u = 1, r = nu n.  The `solve` dict plus rho, n_sv, n_free."""
    n = K.shape[0]
    u = np.ones(n)
    out = solve(K, u, nu * n, tol, max_iter)
    out['rho'], out['n_sv'], out['n_free'] = rho(out['x'], out['g'], u)
    return out


# ---- shared inputs and bounds of the host and device tests -----------------------------------------------------------------------
def one_class_data(n, d, seed=0):
    """Seeded Gaussian rows, a twentieth of them scaled by 3 (the outliers)."""
    rs = np.random.RandomState(seed)
    X = rs.standard_normal((n, d))
    X[::20] *= 3
    return X


def projection_inputs(n, scale, seed=0):
    """v (scaled by `scale`, every 7th entry tied), a box u drawn from {0, 0.5, 1} with a non-zero entry, and the three masses of the
    tests: 0.37 sum u, sum u (the single point u) and half the smallest non-zero box."""
    rs = np.random.RandomState(1000 * seed + n)
    v = rs.standard_normal(n) * scale
    v[::7] = v[0]
    u = rs.choice([0., 0.5, 1.], n)
    if not (u > 0).any():
        u[0] = 1.
    return v, u, [0.37 * u.sum(), u.sum(), 0.5 * u[u > 0].min()]


def projection_figures(P, v, u, r):
    """The two error figures of a projection P of v: |sum P - r| and max |P - P_ext|, both evaluated in np.longdouble, P_ext being
    `project` run in np.longdouble."""
    ext = project(np.asarray(v, dtype=np.longdouble), u, r)
    Pl = np.asarray(P, dtype=np.longdouble)
    return float(abs(Pl.sum() - np.longdouble(r))), float(np.abs(Pl - ext).max())


def projection_bounds(v, u, r):
    """What an fp64 projection other than the reference may show in the two figures: 8 x the reference's own, with a floor of
    2^-50 max(1, |v|_inf).  With tau in one double, sum P moves in steps of (free rows) x ulp(tau), so no fp64 result meets r to
    the floor in general: the reference's own figures are the yardstick."""
    fs, fi = projection_figures(project(v, u, r), v, u, r)
    floor = 2.0 ** -50 * max(1.0, float(np.abs(v).max()))
    return max(8 * fs, floor), max(8 * fi, floor)
