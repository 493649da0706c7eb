"""NumPy restatement of the two-group simplex solver behind NuSVC and NuSVR (test infrastructure, like oneclass_reference.py, whose
`project`, `violation` and `rho` it calls once per group).

A column has m variables in two disjoint groups; group t is the capped simplex {0 <= x <= u on its variables, sum x = mass[t]}.
With signs s_j and b = sum_j s_j x_j scattered to panel row j mod n the objective is 1/2 b'Kb + q'x and the gradient
g_j = q_j + s_j (K b)_{j mod n}.  The two equality rows of libsvm's nu-duals, sum s x = 0 and sum x = R, say that each group sums
to R / 2, so the feasible set is the product of the two simplices and its Euclidean projection the two projections taken
independently.

  LABELS (nu-SVC, libsvm solve_nu_svc): m = n, s = the labels, group 0 the rows with s = +1, u = 1, mass = nu n / 2, q = 0
  PAIRED (nu-SVR, libsvm solve_nu_svr): m = 2n, s = (+1, -1), group 0 the first n, u = C, mass = C nu n / 2, q = (-y, +y)

The device code (csrc/bq_simplex.hip: the LABELS and PAIRED instantiations of the sx_* kernels) follows these statements; the tests hold it against this file.
"""
import numpy as np

import oneclass_reference as ocr


class Layout:
    """The signs, the panel row of every variable and the two groups' index arrays (ascending)."""

    def __init__(self, n, sgn=None):
        self.n = n
        if sgn is None:   # PAIRED
            self.m = 2 * n
            self.s = np.concatenate((np.ones(n), -np.ones(n)))
            self.row = np.concatenate((np.arange(n), np.arange(n)))
            self.groups = (np.arange(n), np.arange(n, 2 * n))
        else:             # LABELS
            sgn = np.asarray(sgn, dtype=float)
            self.m = n
            self.s = sgn
            self.row = np.arange(n)
            self.groups = (np.flatnonzero(sgn > 0), np.flatnonzero(sgn < 0))

    def fold(self, x):
        """b = sum_j s_j x_j scattered to row j mod n: s o x (LABELS), x_i - x_{n + i} (PAIRED)"""
        return self.s * x if self.m == self.n else x[:self.n] - x[self.n:]


def project2(v, u, mass, lay):
    """The projection onto the product of the two capped simplices: one `project` per group."""
    P = np.zeros_like(v)
    for idx, r in zip(lay.groups, mass):
        P[idx] = ocr.project(v[idx], u[idx], r)
    return P


def violation2(x, g, u, lay):
    """libsvm's Solver_NU measure: the larger of the two groups' maximal-violating-pair values (-inf for a group with an empty
    side)."""
    return max(ocr.violation(x[idx], g[idx], u[idx]) for idx in lay.groups)


def solve(K, u, mass, sgn=None, q=None, tol=1e-3, max_iter=1000, x0=None):
    """min 1/2 b'Kb + q'x over the two groups' simplices; sgn: the n labels (LABELS) or None (PAIRED, u and q of 2n entries).
    oneclass_reference.solve's loop with the signed gradient and the per-group projection.  Returns its dict, and f_rounding: the
    rounding bound of the start value of f (below; `assert_f_history`)."""
    K = np.asarray(K, dtype=float)
    u = np.asarray(u, dtype=float)
    lay = Layout(K.shape[0], sgn)
    q = np.zeros(lay.m) if q is None else np.asarray(q, dtype=float)
    s_, row = lay.s, lay.row
    x = project2(np.zeros(lay.m), u, mass, lay) if x0 is None else np.array(x0, dtype=float)
    g = q + s_ * (K @ lay.fold(x))[row]
    f = 0.5 * float(x @ (g - q)) + float(q @ x)
    # The forward error bound of that value as a floating-point sum of 2m products, m eps (1/2 |x|'|g - q| + |q|'|x|): what an
    # evaluation of it in another order may differ by.  A PAIRED column with equal boxes and masses starts at alpha = alpha*, where
    # f is 0 in exact arithmetic and every computed value is rounding alone, which no relative tolerance describes.
    f_rounding = lay.m * 2.0 ** -53 * (0.5 * float(np.abs(x) @ np.abs(g - q)) + float(np.abs(q) @ np.abs(x)))
    s, alpha = 1.0, 0.0
    last = [f]
    rows = []
    it = 0
    while True:
        viol = violation2(x, g, u, lay)
        rows.append((it, f, viol, alpha, s))
        if viol <= tol:
            status = 'optimal'
            break
        if it == max_iter:
            status = 'stopped'
            break
        d = project2(x - s * g, u, mass, lay) - x
        gd = float(g @ d)
        if gd >= 0:
            status = 'optimal'
            break
        Qd = s_ * (K @ lay.fold(d))[row]
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
    return dict(x=x, g=g, status=status, iter=it, rows=np.array(rows, dtype=float), f=f, f_rounding=f_rounding)


def assert_f_history(f, ref):
    """The f history `f` of another evaluation of `ref`'s column: every value to rtol 1e-9, except where the reference's own value is
    below the rounding bound of its start value (`solve`'s f_rounding): such a value — the exact 0 at which a PAIRED column starts —
    is rounding alone, and there the difference is held to that bound."""
    want, floor = ref['rows'][:, 1], ref['f_rounding']
    f = np.asarray(f, dtype=float)
    assert f.shape == want.shape
    real = np.abs(want) > floor
    np.testing.assert_allclose(f[real], want[real], rtol=1e-9)
    assert np.all(np.abs(f[~real] - want[~real]) <= floor)


def offsets(x, g, u, sgn=None):
    """libsvm's Solver_NU::calculate_rho: `rho` of oneclass_reference per group.  Returns (r1, r2, n_sv (2), n_free (2))."""
    lay = Layout(len(x) if sgn is not None else len(x) // 2, sgn)
    (r1, s1, f1), (r2, s2, f2) = (ocr.rho(x[idx], g[idx], u[idx]) for idx in lay.groups)
    return r1, r2, (s1, s2), (f1, f2)


def fit_nu_svc(K, y, nu, tol=1e-3, max_iter=1000):
    """NuSVC on the Gram matrix K with labels y = +-1, libsvm's way: alpha in [0, 1], each class summing to nu n / 2; r = (r1 + r2) / 2,
    rho = (r1 - r2) / 2; the decision function is sum_i (y_i alpha_i / r) k(x_i, .) - rho / r."""
    n = K.shape[0]
    u = np.ones(n)
    out = solve(K, u, (nu * n / 2, nu * n / 2), sgn=y, tol=tol, max_iter=max_iter)
    r1, r2, out['n_sv'], out['n_free'] = offsets(out['x'], out['g'], u, y)
    out['r'], out['rho'] = (r1 + r2) / 2, (r1 - r2) / 2
    out['coef'] = y * out['x'] / out['r']
    out['intercept'] = -out['rho'] / out['r']
    return out


def fit_nu_svr(K, y, C, nu, tol=1e-3, max_iter=1000):
    """NuSVR: x = (alpha, alpha*) in [0, C], each half summing to C nu n / 2, q = (-y, y); the prediction is
    sum_i (alpha_i - alpha*_i) k(x_i, .) - rho and the tube's width is -(r1 + r2) / 2."""
    n = K.shape[0]
    u = np.full(2 * n, float(C))
    out = solve(K, u, (C * nu * n / 2, C * nu * n / 2), q=np.concatenate((-y, y)), tol=tol, max_iter=max_iter)
    r1, r2, out['n_sv'], out['n_free'] = offsets(out['x'], out['g'], u)
    out['epsilon'], out['rho'] = -(r1 + r2) / 2, (r1 - r2) / 2
    out['coef'] = out['x'][:n] - out['x'][n:]
    out['intercept'] = -out['rho']
    return out


# ---- shared inputs of the host and device tests ------------------------------------------------------------------------------------
GAMMAS = (1.0 / 8, 0.02)
SVC_GRID = [(g, nu) for g in GAMMAS for nu in (0.5017, 0.7017, 0.9017)] + [(1.0 / 8, 0.3517)]
SVR_GRID = [(g, C, nu) for g in GAMMAS for C, nu in ((1.0, 0.2517), (1.0, 0.5017), (0.5, 0.8017))]
TOLS = (1e-3, 1e-6)


def nu_data():
    """X (600 x 8), Xnew (50 x 8), yc (+-1: 314 / 286 rows) and yr, drawn in this order from RandomState(0)."""
    n, d = 600, 8
    rs = np.random.RandomState(0)
    X = rs.standard_normal((n, d))
    Xnew = rs.standard_normal((50, d)) * 1.5
    yc = np.where(X[:, 0] + 0.5 * X[:, 1] ** 2 + 0.6 * rs.standard_normal(n) > 0.4, 1, -1)
    yr = np.sin(X[:, 0]) + 0.5 * X[:, 1] + 0.2 * rs.standard_normal(n)
    return X, Xnew, yc, yr
