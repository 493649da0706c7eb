"""The seeded draws, per-column references and bars of the batched solvers' differential run (test infrastructure, plain NumPy, no
device): tests/test_batched_fuzz_host.py holds the draws and the references to their preconditions, tests/test_gpu_fuzz_batched.py
solves every draw on the device and holds it to the bars.  Both import this file, so they see the same draws.

A draw is one batched solve: a family (which create call), the panel's rows and kernel, k columns with their boxes, labels or
linear terms, masses and start points, a storage format, a run cut, and the columns that get a trajectory reference.  Everything
comes from np.random.RandomState(seed); a seed of STRIP_BASE or more draws the strip-edge shapes (n in N_STRIP, k <= 5, 5
iterations).  A column's reference is the oracle's solver (oracle/bcqp_oracle.py) or the simplex references (oneclass_reference,
nu_reference) on the column's own problem: the sub-Gram of its trained rows, cut from the panel K that the caller passes.
"""
import functools
from types import SimpleNamespace

import numpy as np

import nu_reference as nur
import oneclass_reference as ocr
from oracle import bcqp_oracle as bo
from oracle import svm_oracle as so

TILE = 256
U53 = 2.0 ** -53

BOX_FAMILIES = ('labels4', 'boxes16', 'svr', 'svr_boxes', 'pairs')
SIMPLEX_FAMILIES = ('sx_one', 'sx_labels', 'sx_paired', 'sx_blocks')
FAMILIES = BOX_FAMILIES + SIMPLEX_FAMILIES
PAIR_FAMILIES = ('pairs', 'sx_blocks')

N_POOL = (2, 3, 64, 255, 256, 257, 300, 511, 513, 1023, 1025, 1100)
N_STRIP = (2049, 2305)              # a strip is 2048 columns
K_POOL = (1, 3, 4, 5, 15, 16, 17, 33, 40)
K_STRIP = (1, 3, 4, 5)
CLASS_SIZES = (1, 5, 130, 256, 257, 300, 513)
C_POOL = (0.1, 1.0, 10.0)
SX_GAMMA_D = ((1.0, 2), (3.0, 2), (3.0, 3), (3.0, 4))   # gamma in {1, 3}, d in {2, 3, 4}, gamma / d > 0.4
NUS = (0.0517, 0.2517, 0.8017)
# PAIRED leaves out 0.0517: at C nu n / 2 <= 5 a handful of rows carry the whole mass, the reference reaches its optimum to the
# last bit inside the 15 iterations and rounding decides where it stops (4 of 58 checked columns were not unanimous with it, above
# the 5 % cap of tests/test_batched_fuzz_host.py; without it: see that test's figures)
NUS_PAIRED = (0.2517, 0.8017)
STORAGES = ('f64', 'f64_plain', 'f32')   # f64: compact when eligible; f64_plain: the hook compact_panel=0
CHUNKS = (1, 7, 256)
BOX_ITERS, SX_ITERS, STRIP_ITERS = 30, 15, 5
BOX_EPS = 1e-6                      # the box solvers' stop tolerance (their default); the simplex families run at tol = 0
LEAVER_C = 1e-6                     # the box of a column that is to stop early: x = ub is its optimum (g = Q ub - 1 < 0 for an RBF panel)
STRIP_BASE = 1000
WIDTH = {'labels4': 4, 'svr': 4}    # columns per product chunk; every other family: 16

# ---- the seed lists: BLOCKS[family] are the cases of the device test, LEAVERS[family] the named draws in which the reference stops
# a column ('optimal') before the cap while another column runs to it (found on the CPU; the host test asserts it) ----------------------
# Family number i has the seeds 100 i ... 100 i + 15 in four blocks of four, and the strip block (STRIP_BASE + 10 i, + 1): 18 draws.
BLOCKS = {f: tuple(tuple(range(100 * i + 4 * b, 100 * i + 4 * b + 4)) for b in range(4)) + ((STRIP_BASE + 10 * i, STRIP_BASE + 10 * i + 1),)
          for i, f in enumerate(FAMILIES)}
LEAVERS = {'labels4': (6, 7, 12, 14), 'boxes16': (100, 104, 111, 113, 114), 'svr': (206, 210, 213, 215),
           'svr_boxes': (304, 308), 'pairs': (405, 407, 412, 413), 'sx_one': (500, 502, 507, 511, 512, 513, 514),
           'sx_labels': (604, 607), 'sx_paired': (701, 702, 704, 705, 706, 711), 'sx_blocks': (800, 807, 809, 810, 811)}


def seeds(family):
    return tuple(s for block in BLOCKS[family] for s in block)


def _fold_mask(rs, n):
    """None, or the rows of one of three interleaved folds (True: held out)"""
    f = int(rs.randint(-1, 3))
    if f < 0 or n < 64:
        return np.zeros(n, dtype=bool)
    return np.arange(n) % 3 == f


def _common(rs, seed, pool_n, simplex):
    strip = seed >= STRIP_BASE
    dr = SimpleNamespace(seed=seed, strip=strip)
    dr.n = N_STRIP[seed % 2] if strip else int(rs.choice(pool_n))
    dr.k = int(rs.choice(K_STRIP if strip else K_POOL))
    dr.storage = str(rs.choice(STORAGES))
    dr.chunk = int(rs.choice(CHUNKS))
    dr.chunk2 = int(rs.choice([c for c in CHUNKS if c != dr.chunk]))
    dr.start = bool(rs.rand() < 0.5)
    dr.leave = bool(dr.k >= 2 and rs.rand() < 0.3 and not strip)
    dr.leaver = int(rs.randint(dr.k)) if dr.leave else None
    dr.extra = int(rs.randint(dr.k))
    dr.max_iter = STRIP_ITERS if strip else SX_ITERS if simplex else BOX_ITERS
    dr.eps = 0.0 if simplex else BOX_EPS
    return dr


def _pair_panel(rs, dr, d, first_min):
    """The class-sorted, ghost-padded panel of 2 to 5 classes with sizes from CLASS_SIZES (the first at least first_min rows; a
    strip draw's first class has dr.n rows): Xp, cls_tiles, pcode, ghost, rank (a data row's position within its class)."""
    from optiml_amd.ml.svm.onevsone import sort_plan
    ncls = int(rs.randint(2, 6))
    sizes = [int(s) for s in rs.choice(CLASS_SIZES, ncls)]
    sizes[0] = dr.n if dr.strip else int(rs.choice([s for s in CLASS_SIZES if s >= first_min]))
    codes = rs.permutation(np.repeat(np.arange(ncls), sizes))
    centers = 1.2 * rs.standard_normal((ncls, d))
    X = centers[codes] + rs.standard_normal((len(codes), d))
    index, ct, n_pad = sort_plan(codes, ncls)
    dr.sizes, dr.ct, dr.index = sizes, ct, index
    dr.n = n_pad
    dr.X = np.zeros((n_pad, d))
    dr.X[index] = X
    dr.ghost = np.ones(n_pad, dtype=bool)
    dr.ghost[index] = False
    dr.pcode = np.repeat(np.arange(ncls), np.diff(ct) * TILE)
    dr.rank = np.arange(n_pad) - (np.asarray(ct[:-1], dtype=np.int64) * TILE)[dr.pcode]
    return ncls


def _pair_boxes(rs, dr, pairs, C):
    """k x n boxes: C[c] on the data rows of pair c's classes, 0 on a held-out fold of them (classes of 5 or more rows)"""
    UB = np.zeros((dr.k, dr.n))
    for c, (i, j) in enumerate(pairs):
        f = int(rs.randint(-1, 3))
        mine = ((dr.pcode == i) | (dr.pcode == j)) & ~dr.ghost
        big = np.asarray(dr.sizes)[dr.pcode] >= 5
        held = big & (dr.rank % 3 == f) if f >= 0 else np.zeros(dr.n, dtype=bool)
        UB[c, mine & ~held] = C[c]
    return UB


def _box_kernel(rs, dr, X, data):
    """RBF at gamma = 1 / (d var X), (2 x'y / max |x|^2 + 1)^3, or the linear kernel with X scaled to max |x|^2 <= 16: |K| < 32, so
    an fp32 panel rounds an entry by less than 2^-20 and the existing tests' atol of 1e-6 for fp32 panels holds for every kernel.
    `data`: the rows of X that are data rows (a pair panel's ghost rows are 0)."""
    name = str(rs.choice(['rbf', 'poly', 'linear']))
    if dr.leave and dr.family in ('labels4', 'boxes16', 'pairs'):
        name = 'rbf'   # LEAVER_C's claim needs |K| <= 1
    r2 = float((X[data] ** 2).sum(axis=1).max())
    if name == 'linear':
        X *= np.sqrt(min(1.0, 16.0 / r2))
    if name == 'poly':
        return name, 2.0 / r2, 1.0, 3
    return name, 1.0 / (X.shape[1] * X[data].var()), 0.0, 3


def _draw_box(family, seed):
    rs = np.random.RandomState(seed)
    dr = _common(rs, seed, N_POOL, False)
    dr.family = family
    dr.kind = str(rs.choice(['pg', 'fw']))
    dr.t = float(rs.choice([0.0, 0.1])) if dr.kind == 'fw' else 0.0
    d = int(rs.choice([2, 5, 16]))
    k = dr.k
    svr = family in ('svr', 'svr_boxes')
    shared = family in ('labels4', 'svr')
    if family == 'labels4' and dr.leave:
        dr.kind, dr.t = 'pg', 0.0   # the shared box is LEAVER_C: FrankWolfe would stop every column
    if dr.leave and dr.kind == 'pg':
        dr.start = True             # ProjectedGradient leaves from its start point, FrankWolfe after its first steps
    if family == 'pairs':
        ncls = _pair_panel(rs, dr, d, 1)
        allp = [(i, j) for i in range(ncls) for j in range(i + 1, ncls)]
        dr.pairs = [allp[int(p)] for p in rs.randint(len(allp), size=k)]
        X = dr.X
        dr.kernel = _box_kernel(rs, dr, X, ~dr.ghost)
    else:
        X = dr.X = rs.standard_normal((dr.n, d))
        dr.kernel = _box_kernel(rs, dr, X, slice(None))
    n = dr.n
    dr.structure = 'svr' if svr else 'svc'
    dr.m = 2 * n if svr else n
    C = rs.choice(C_POOL, k)
    if shared:
        C[:] = C[0]
    if dr.leave and not svr:
        if shared:
            C[:] = LEAVER_C
        else:
            C[dr.leaver] = LEAVER_C
    if family == 'pairs':
        dr.UB = _pair_boxes(rs, dr, dr.pairs, C)
        dr.Y = np.stack([np.where(dr.pcode == j, 1., -1.) for _, j in dr.pairs])
    elif svr:
        w = rs.standard_normal((k, d))
        T = np.tanh(X @ w.T / np.sqrt(d)).T + 0.1 * rs.standard_normal((k, n))
        eps = rs.choice([0.05, 0.1, 0.2], k)
        if dr.leave:
            eps[dr.leaver] = 100.0 * float(np.abs(T[dr.leaver]).max())   # q > 0 everywhere: 0 is the optimum
        dr.T, dr.epsilon = T, eps
        dr.QL = np.hstack((-T, T)) + eps[:, None]
        if shared:
            dr.UB = np.full(2 * n, C[0])
        else:
            dr.UB = np.stack([np.tile(np.where(_fold_mask(rs, n), 0., C[c]), 2) for c in range(k)])
    else:
        Y = np.where(rs.standard_normal((k, n)) > 0, 1., -1.)
        if shared:
            dr.UB = np.full(n, C[0])
            tr = np.ones((k, n), dtype=bool)
        else:
            dr.UB = np.stack([np.where(_fold_mask(rs, n), 0., C[c]) for c in range(k)])
            tr = dr.UB > 0
        for c in range(k):   # both signs among the trained rows
            first = np.flatnonzero(tr[c])[:2]
            Y[c, first] = (1., -1.)
        dr.Y = Y
    dr.C = C
    ub_all = np.broadcast_to(dr.UB, (k, dr.m))
    dr.x0 = None
    if dr.start:
        dr.x0 = ub_all * rs.uniform(size=(k, dr.m))
        if dr.leave and dr.kind == 'pg':
            dr.x0[dr.leaver] = 0. if svr else ub_all[dr.leaver]
    return dr


def _sx_data(rs, n, d):
    X = rs.standard_normal((n, d))
    X[::20] *= 3
    return X


def _draw_simplex(family, seed):
    rs = np.random.RandomState(seed)
    dr = _common(rs, seed, [n for n in N_POOL if n >= 64], True)
    dr.family, dr.structure, dr.kind, dr.t = family, 'plain', None, 0.0
    gamma, d = SX_GAMMA_D[int(rs.randint(len(SX_GAMMA_D)))]
    dr.kernel = ('rbf', gamma, 0.0, 3)
    k = dr.k
    nus = rs.choice(NUS_PAIRED if family == 'sx_paired' else NUS, k)
    dr.S = dr.q = dr.pairs = None
    if family == 'sx_blocks':
        ncls = _pair_panel(rs, dr, d, 130)
        allp = [(i, j) for i in range(ncls) for j in range(i + 1, ncls) if dr.sizes[i] + dr.sizes[j] >= 64]
        dr.pairs = [allp[int(p)] for p in rs.randint(len(allp), size=k)]
        n = dr.n
        dr.m = n
        dr.UB = _pair_boxes(rs, dr, dr.pairs, np.ones(k))
        dr.groups = [(np.flatnonzero(dr.pcode == j), np.flatnonzero(dr.pcode == i)) for i, j in dr.pairs]   # class b is +1
    else:
        n = dr.n
        X = dr.X = _sx_data(rs, n, d)
        masks = np.stack([~_fold_mask(rs, n) for _ in range(k)]).astype(float)
        if family == 'sx_one':
            dr.m = n
            dr.UB = masks
            for c in range(k):
                if rs.rand() < 0.25:
                    dr.UB[c, ::5] *= 0.5
            dr.groups = [(np.arange(n),)] * k
        elif family == 'sx_labels':
            dr.m = n
            y = np.where(X[:, 0] + 0.5 * X[:, 1] ** 2 + 0.6 * rs.standard_normal(n) > 0.4, 1., -1.)
            dr.S = np.stack([y if rs.rand() < 0.5 else -y for _ in range(k)])
            dr.UB = masks
            dr.groups = [(np.flatnonzero(dr.S[c] > 0), np.flatnonzero(dr.S[c] < 0)) for c in range(k)]
        else:   # sx_paired
            dr.m = 2 * n
            t = np.sin(X[:, 0]) + 0.5 * X[:, 1] + 0.2 * rs.standard_normal(n)
            Cs = rs.choice([1.0, 0.5], k)
            dr.UB = np.hstack((masks, masks)) * Cs[:, None]
            dr.q = np.tile(np.concatenate((-t, t)), (k, 1))
            dr.groups = [(np.arange(n), np.arange(n, 2 * n))] * k
    mass = np.empty((k, len(dr.groups[0])))
    for c in range(k):
        sums = [float(dr.UB[c][idx].sum()) for idx in dr.groups[c]]
        if family == 'sx_one':
            mass[c] = nus[c] * sums[0]
        elif family == 'sx_paired':
            mass[c] = nus[c] * sums[0] / 2
        else:
            mass[c] = nus[c] * min(sums)
        if dr.leave and c == dr.leaver:
            mass[c] = sums   # every group's mass is its whole box: x = ub, no row can move, 'optimal' at iteration 0
    dr.mass = mass[:, 0].copy() if family == 'sx_one' else mass
    dr.x0 = None
    if dr.start:   # a feasible start: the projection of a random v, per group
        dr.x0 = np.zeros((k, dr.m))
        for c in range(k):
            v = 0.5 * rs.standard_normal(dr.m)
            for idx, r in zip(dr.groups[c], mass[c]):
                dr.x0[c, idx] = ocr.project(v[idx], dr.UB[c][idx], r)
    return dr


@functools.lru_cache(maxsize=None)
def draw(family, seed):
    """Everything one solve of `family` needs, from np.random.RandomState(seed) alone.  The result is shared: leave it unchanged."""
    dr = (_draw_simplex if family in SIMPLEX_FAMILIES else _draw_box)(family, int(seed))
    for v in vars(dr).values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    width = WIDTH.get(family, 16)
    cols = [0, dr.k - 1] + ([width] if dr.k > width else []) + ([dr.leaver] if dr.leave else [])
    dr.checked = sorted(set(cols))
    return dr


def ub_of(dr, c):
    return dr.UB if dr.UB.ndim == 1 else dr.UB[c]


def oracle_gram(dr):
    """The oracle's Gram matrix of the draw's panel rows (ghost rows included), to which the downloaded panel is held first"""
    name, g, coef0, degree = dr.kernel
    return so.gram(name, dr.X, None, g, coef0, degree)


def gram_tolerance(dr):
    """(rtol, atol) of the panel against `oracle_gram`: the fp32 panels' 1e-6, and for fp64 test_gpu_multiclass's product bound
    (rtol 1e-12, atol 1e-12 |w|_1) at w = a unit vector"""
    return (0.0, 1e-6) if dr.storage == 'f32' else (1e-12, 1e-12)


def trained(dr, c):
    """(idx, rows): the variables of column c with a box (ascending) and their panel rows"""
    idx = np.flatnonzero(ub_of(dr, c) > 0)
    return idx, idx % dr.n


def _solve_on(dr, c, idx, Ks, Qsvr=None):
    """The reference's run of column c on Ks, the Gram matrix of its trained panel rows (Qsvr: svr_dual's Hessian of Ks)"""
    u = ub_of(dr, c)[idx]
    x0 = None if dr.x0 is None else dr.x0[c][idx]
    fam = dr.family
    if fam in BOX_FAMILIES:
        if dr.structure == 'svr':
            Q, q = Qsvr, dr.QL[c][idx]
        else:
            Q, q, _ = so.svc_dual(Ks, dr.Y[c][idx], 1.0)
        if dr.kind == 'pg':
            r = bo.projected_gradient(Q, q, u, x0=x0, eps=dr.eps, max_iter=dr.max_iter)
        else:
            r = bo.frank_wolfe(Q, q, u, x0=x0, eps=dr.eps, max_iter=dr.max_iter, t=dr.t)
        return dict(status=r['status'], iter=int(r['iter']), f=np.asarray(r['f_hist'], dtype=float), x=r['x'], floor=0.0)
    if fam == 'sx_one':
        r = ocr.solve(Ks, u, float(dr.mass[c]), tol=dr.eps, max_iter=dr.max_iter, x0=x0)
        floor = 0.0
    else:
        if fam == 'sx_labels':
            sgn, q = dr.S[c][idx], None
        elif fam == 'sx_paired':
            sgn, q = None, dr.q[c][idx]
        else:
            sgn, q = np.where(dr.pcode[idx] == dr.pairs[c][1], 1., -1.), None
        r = nur.solve(Ks, u, tuple(dr.mass[c]), sgn=sgn, q=q, tol=dr.eps, max_iter=dr.max_iter, x0=x0)
        floor = r['f_rounding']
    return dict(status=r['status'], iter=int(r['iter']), f=r['rows'][:, 1].copy(), x=r['x'], g=r['g'], floor=floor)


def sensitivities(dr, cols, K):
    """Per column of `cols`: the reference on the panel K and on three seeded, symmetric one-ulp perturbations of K
    (test_gpu_oneclass._trajectory_reference's construction, made symmetric).  A dict column -> dict: `base`, the run on K
    (status, iter, the f history, x on the trained variables `idx`); whether the four runs agree on status and iteration count
    (`unanimous`); the length of the f history that all four have (`common`); the spread of f over it and of the final x."""
    runs = {c: [] for c in cols}
    for seed in (None, 0, 1, 2):
        held = {}   # columns with the same trained rows share the perturbed sub-Gram (and the SVR Hessian built from it)
        for c in cols:
            idx, rows = trained(dr, c)
            if dr.m == 2 * dr.n:
                rows = rows[:len(rows) // 2]   # both halves have the same trained rows
            key = rows.tobytes()
            if key not in held:
                Ks = np.ascontiguousarray(K[np.ix_(rows, rows)])
                if seed is not None:
                    up = np.triu(np.random.RandomState(seed).rand(*Ks.shape) < 0.5)
                    Ks = np.nextafter(Ks, np.where(up | up.T, np.inf, -np.inf))
                held = {key: (Ks, so.svr_dual(Ks, np.zeros(len(rows)), 1.0, 0.0)[0] if dr.structure == 'svr' else None)}
            runs[c].append(_solve_on(dr, c, idx, *held[key]))
    out = {}
    for c in cols:
        base = runs[c][0]
        common = min(len(r['f']) for r in runs[c])
        out[c] = dict(base=base, idx=trained(dr, c)[0], common=common,
                      unanimous=all(r['status'] == base['status'] and r['iter'] == base['iter'] for r in runs[c]),
                      f_spread=max(float(np.abs(r['f'][:common] - base['f'][:common]).max()) for r in runs[c]),
                      x_spread=max(float(np.abs(r['x'] - base['x']).max()) for r in runs[c]))
    return out


def sensitivity(dr, c, K):
    return sensitivities(dr, [c], K)[c]


# ---- the bars ---------------------------------------------------------------------------------------------------------------------------
def f_bar(sens):
    """Bar (d) on the f history: the larger of 10 x the column's own spread and 1e-9 max |f| (the fixed-shape trajectory tests' bar);
    a PAIRED start at an exact 0 is rounding alone and is held to nu_reference.assert_f_history's floor."""
    f = sens['base']['f'][:sens['common']]
    return max(10 * sens['f_spread'], 1e-9 * float(np.abs(f).max()), sens['base']['floor'])


def x_bar(dr, c, sens):
    return max(10 * sens['x_spread'], 1e-9 * float(ub_of(dr, c).max()))


def start_gradient(dr, c, K, x0):
    """Bar (c): g0 = Q x0 + q of column c (the simplex families' own g0) in np.longdouble on the panel K, and the elementwise forward
    bound (m + 4) 2^-53 (|Q||x0| + |q|) of a sum of m terms in any order (m = n, or 2n for SVR and PAIRED); `rows`: the entries the
    bar applies to (a pair column: the rows of its two classes, g is held to an exact value elsewhere; a simplex column: its variables
    with a box, on which alone its dual and the reference define g)."""
    n = dr.n
    L = np.longdouble
    x = np.asarray(x0, dtype=L)
    fam = dr.family
    rows = np.arange(dr.m)
    if fam in PAIR_FAMILIES:
        i, j = dr.pairs[c]
        rows = np.flatnonzero((dr.pcode == i) | (dr.pcode == j))
    if fam in SIMPLEX_FAMILIES:
        rows = rows[ub_of(dr, c)[rows] > 0]   # the simplex duals define g on a column's own variables only
    live = np.flatnonzero(x0[:n] != 0) if dr.m == n else np.flatnonzero((x0[:n] != 0) | (x0[n:] != 0))
    r1 = rows[rows < n] if dr.m == 2 * n else rows
    Kl = K[np.ix_(r1, live)].astype(L)
    if dr.structure == 'svc':
        s = dr.Y[c].astype(L)
        w = (s * x)[live]
        g = s[r1] * (Kl @ w + w.sum()) - 1
        mag = np.abs(Kl) @ np.abs(w) + np.abs(w).sum() + 1
        terms = n
    elif dr.structure == 'svr' or fam == 'sx_paired':
        w = (x[:n] - x[n:])[live]
        a = (np.abs(x[:n]) + np.abs(x[n:]))[live]
        q = (dr.QL if fam != 'sx_paired' else dr.q)[c].astype(L)[rows]
        u = Kl @ w + (w.sum() if fam != 'sx_paired' else 0)
        mag = np.abs(Kl) @ a + (a.sum() if fam != 'sx_paired' else 0)
        g = np.concatenate((u, -u)) + q
        mag = np.concatenate((mag, mag)) + np.abs(q)
        terms = 2 * n
    else:
        s = np.ones(n, dtype=L)
        if fam == 'sx_labels':
            s = dr.S[c].astype(L)
        elif fam == 'sx_blocks':
            s = np.where(dr.pcode == dr.pairs[c][1], L(1), L(-1))
        w = (s * x)[live]
        g = s[r1] * (Kl @ w)
        mag = np.abs(Kl) @ np.abs(w)
        terms = n
    return rows, g, (terms + 4) * U53 * mag


def offset_check(dr, c, res):
    """Bar (d), offsets of a simplex column: oneclass_reference.rho / nu_reference.offsets on the device's own x and g.  Returns
    a list of (name, device value, reference value, bound); counts have bound 0; a mean over free rows may be summed in another
    order and gets test_gpu_svr_cv's bound, 4 n 2^-53 sum |g_free| / n_free; a midpoint of two entries of g is exact."""
    u = ub_of(dr, c)
    x, g = res['x'], res['g']
    out = []
    for t, idx in enumerate(dr.groups[c]):
        idx = idx[u[idx] > 0]
        rho, n_sv, n_free = ocr.rho(x[idx], g[idx], u[idx])
        free = (x[idx] > 0) & (x[idx] < u[idx])
        bound = 4 * dr.n * U53 * float(np.abs(g[idx][free]).sum()) / n_free if n_free else 0.0
        out.append(('rho%d' % t, float(res['rho'][t]), rho, bound))
        out.append(('n_sv%d' % t, int(res['n_sv'][t]), n_sv, 0))
        out.append(('n_free%d' % t, int(res['n_free'][t]), n_free, 0))
    return out


def valid(dr):
    """The preconditions of a draw, as a list of complaints (empty: valid)"""
    bad = []
    k, m = dr.k, dr.m
    UB = np.broadcast_to(dr.UB, (k, m))
    if not (UB >= 0).all():
        bad.append('ub < 0')
    if dr.x0 is not None and not ((dr.x0 >= 0) & (dr.x0 <= UB)).all():
        bad.append('x0 outside its box')
    for c in range(k):
        tr = UB[c] > 0
        if dr.structure == 'svc' and set(np.unique(dr.Y[c][tr])) != {-1., 1.}:
            bad.append('column %d: labels of one sign' % c)
        if dr.family in PAIR_FAMILIES:
            i, j = dr.pairs[c]
            if not (0 <= i < j < len(dr.sizes)):
                bad.append('column %d: pair outside the class list' % c)
            if (tr & ~((dr.pcode == i) | (dr.pcode == j))).any() or (tr & dr.ghost).any():
                bad.append('column %d: a box outside the pair' % c)
        if dr.family in SIMPLEX_FAMILIES:
            for idx, r in zip(dr.groups[c], np.atleast_1d(dr.mass[c])):
                total = float(UB[c][idx].sum())
                if not 0 < r <= total:
                    bad.append('column %d: mass %g outside (0, %g]' % (c, r, total))
                if dr.x0 is not None and abs(float(dr.x0[c][idx].sum()) - r) > len(idx) * 2.0 ** -52 * r:
                    bad.append('column %d: x0 does not sum to its mass' % c)
    return bad
