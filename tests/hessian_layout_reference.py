"""Case builders for the Hessian-assembly tests (test_hessian_layouts_host.py, test_gpu_hessian_layouts.py).  No GPU here.

InteriorPoint, ActiveSet and x_star() assemble a dense H from the resident panel one element at a time (csrc/bq_qelem.h), and the
reference factorises with scipy's `cho_factor`, which reads ONE triangle of what it is given (the upper one by default).  On a
Q that is not symmetric the triangle decides the answer, so the cases below make the two triangles differ by far more than any
tolerance the GPU tests use — the host tests check that they do.
"""
import numpy as np
import scipy.linalg

from oracle import bcqp_oracle as bo

NONSYM_SIZES = (5, 33, 130, 257, 520)   # 33: one 32x32 tile of the assembly; 130: one Cholesky block; 257 / 520: one / two 256-row tiles
OTHER_SIZES = (33, 257)
IP_ITERS = 6                            # InteriorPoint is compared over its first iterations only (n = 257 never converges)

# what the GPU tests hold the device to (test_ragged_sizes_dense, test_quadratic_x_star_and_f_star)
F_TOL = dict(rtol=1e-8, atol=1e-10)
X_TOL = dict(rtol=1e-6, atol=1e-8)
XSTAR_RTOL = 1e-9


def xstar_tol(ref):
    return dict(rtol=XSTAR_RTOL, atol=1e-12 * np.abs(ref).max())


def as_iters(n):
    return min(3 * n + 50, 500)


def rounded(Q, storage):
    """The matrix the device holds: fp32 storage rounds every entry once."""
    return Q.astype(np.float32).astype(np.float64) if storage == 'f32' else Q


def _box(rs, n):
    q = rs.standard_normal(n)
    ub = rs.uniform(0.5, 2.0, n)
    lb = -rs.uniform(0.0, 0.5, n)
    return q, ub, lb


def nonsymmetric_case(n):
    """A positive definite S plus a strictly lower triangular perturbation: reading the upper triangle gives S, the lower one
    S + E + E', and the products see S + E."""
    rs = np.random.RandomState(700 + n)
    G = rs.standard_normal((n, n + 3))
    S = G @ G.T / n + 0.05 * np.eye(n)
    Q = S + (1e-3 / np.sqrt(n)) * np.tril(rs.standard_normal((n, n)), -1)
    q, ub, lb = _box(rs, n)
    return Q, q, ub, lb


def lower_only_case(n):
    """(Q as handed to `symmetric=True`, the matrix it stands for, q, ub, lb): the strict upper triangle of Q is garbage, the
    oracle runs on the matrix mirrored from the lower triangle."""
    rs = np.random.RandomState(800 + n)
    G = rs.standard_normal((n, n + 3))
    S = G @ G.T / n + 0.05 * np.eye(n)
    L = np.tril(S)
    Q = L + np.triu(10.0 * rs.standard_normal((n, n)), 1)
    mirrored = L + np.tril(S, -1).T
    q, ub, lb = _box(rs, n)
    return Q, mirrored, q, ub, lb


def rounding_case(n):
    """An exactly symmetric Q that the caller passes with `symmetric=False`: row blocks, both triangles hold the same bits."""
    rs = np.random.RandomState(900 + n)
    G = rs.standard_normal((n, n + 3))
    S = G @ G.T / n + 0.05 * np.eye(n)
    Q = (S + S.T) / 2
    assert np.array_equal(Q, Q.T)
    q, ub, lb = _box(rs, n)
    return Q, q, ub, lb


# ---- kernel problems on a full panel ---------------------------------------------------------------------------------------------
# gamma = 0.5 on six standard normal features: off-diagonal entries of K around exp(-6), cond(K + 1) below 2e4 at n = 300.  The
# device builds K itself, a few ulps from so.gram's, and x* moves by cond(Q) times that: at this gamma an ulp of K moves x* by
# about 0.01 of the x_star tolerance (test_hessian_layouts_host.py measures it), at the default 'scale' by more than the tolerance.
GAMMA = 0.5
SVC_SIZES = (40, 129, 300)   # one tile; a one-row second Cholesky block; two 256-row tiles
SVR_SIZES = (40, 129)        # 2n = 80, 258
SVR_EPSILON = 0.1
SQHINGE_C = 10.0


def kernel_data(n):
    """(X, labels in +-1, regression targets), fixed by n."""
    rs = np.random.RandomState(1000 + n)
    X = rs.standard_normal((n, 6))
    y = np.where(X[:, 0] + 0.7 * rs.standard_normal(n) > 0, 1., -1.)
    t = np.sin(X[:, 0]) + 0.5 * X[:, 1] + 0.1 * rs.standard_normal(n)
    return X, y, t


def perturbed(K, ulps=1.0):
    """K with every entry moved by about `ulps` ulps (symmetric, fixed seed): what another correct Gram build may return."""
    rs = np.random.RandomState(0)
    Kp = K * (1 + ulps * 2.0 ** -52 * rs.standard_normal(K.shape))
    return np.triu(Kp) + np.triu(Kp, 1).T


def svc_case(n, K=None):
    from oracle import svm_oracle as so
    X, y, _ = kernel_data(n)
    Q, q, ub = so.svc_dual(so.gram('rbf', X, gamma=GAMMA) if K is None else K, y, 1.0)
    return X, y, Q, q, ub


def svr_case(n, K=None):
    from oracle import svm_oracle as so
    X, _, t = kernel_data(n)
    Q, q, ub = so.svr_dual(so.gram('rbf', X, gamma=GAMMA) if K is None else K, t, 1.0, SVR_EPSILON)
    return X, Q, q, ub


def plain_case(n, diag=0.5):
    from oracle import svm_oracle as so
    X, _, _ = kernel_data(n)
    q = np.random.RandomState(1100 + n).standard_normal(n)
    return X, so.gram('rbf', X, gamma=GAMMA) + diag * np.eye(n), q, np.ones(n), diag


def sqhinge_case(n):
    """The squared-hinge dual K*yy' + yy' + I/(2C), ub = +inf, started at x0 = 1 (BASELINE config 5's shape)."""
    X, y, Q, q, _ = svc_case(n)
    diag = 1.0 / (2 * SQHINGE_C)
    return X, y, Q + diag * np.eye(n), q, np.full(n, np.inf), np.ones(n), diag


def with_asymmetry(Q, ulps):
    """A symmetric Q with max |Q_ij - Q_ji| = `ulps` ulps of max |Q| (give or take the rounding of one addition): three entries
    below the diagonal are moved, in the first row block, across the last tile edge and in the last row."""
    n = len(Q)
    Q = Q.copy()
    step = ulps * 2.0 ** -52 * np.abs(Q).max()
    for i, j in ((1, 0), (n - 1, n // 2), (n - 1, n - 2)):
        Q[i, j] += step
    return Q


def asymmetry_ulps(Q):
    return float(np.abs(Q - Q.T).max() / (2.0 ** -52 * np.abs(Q).max()))


def oracle_with_triangle(fn, triangle, *args, **kw):
    """fn(*args, **kw) of oracle.bcqp_oracle with every `cho_factor` reading the named triangle ('upper': scipy's default, what
    the reference does; 'lower')."""
    if triangle not in ('upper', 'lower'):
        raise ValueError(triangle)
    saved = bo.cho_factor
    bo.cho_factor = lambda a: scipy.linalg.cho_factor(a, lower=(triangle == 'lower'))
    try:
        return fn(*args, **kw)
    finally:
        bo.cho_factor = saved


def margin(got, ref, rtol, atol):
    """How many tolerances `got` is away from `ref` under assert_allclose's test |got - ref| <= atol + rtol |ref| (inf when
    the two do not even have the same length: trajectories that part ways end at different iterations)."""
    got, ref = np.atleast_1d(np.asarray(got, dtype=float)), np.atleast_1d(np.asarray(ref, dtype=float))
    if got.shape != ref.shape:
        return np.inf
    return float(np.max(np.abs(got - ref) / (atol + rtol * np.abs(ref))))


def solve_all(Q, q, ub, lb, triangle, n):
    """The three quantities the GPU tests compare, for ActiveSet, InteriorPoint (first IP_ITERS iterations) and x_star."""
    a = oracle_with_triangle(bo.active_set, triangle, Q, q, ub, lb=lb, max_iter=as_iters(n), trace=True)
    ip = oracle_with_triangle(bo.interior_point, triangle, Q, q, ub, lb=lb, max_iter=IP_ITERS)
    xs, method = oracle_with_triangle(bo.x_star, triangle, Q, q)
    return {'as': a, 'ip': ip, 'x_star': xs, 'x_star_method': method}
