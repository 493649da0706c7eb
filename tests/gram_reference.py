"""Inputs, long-double references and per-entry bounds of the Gram-build tests (test_gpu_gram_edges.py on the device,
test_gram_edges_host.py for the oracle and for the tests' own sensitivity).

Exact-argument family.  Entries of the operands are multiples of 2^-6 with |x| <= 2, gamma is a power of two and coef0 a multiple
of 1/4: every dot product, squared norm, RBF distance, L1 distance and map argument is exact in fp64 whatever the order of the sums
(all are multiples of 2^-12 gamma far below 2^53 of them).  `arguments` asserts it entry by entry against the same quantities formed
in np.longdouble.  The device and the reference then differ in the map only: the reference is `exp`, `tanh`, `**` in np.longdouble
on those arguments, and with u = 2^-53

    |K - ref| <= MAP_U u |ref|                     (+ 2^-24 |ref| for a panel stored in fp32: one rounding of the fp64 value)

The linear kernel runs on the grid scaled to integers (|x| <= 128): the Gram matrix is the integer product, compared for equal bits
(in fp32 too: every entry is below 2^24).

Cancellation family.  Ordinary fp64 rows with a common offset of 20 standard deviations, every 7th row a copy of another plus 1e-7
noise: the true squared distance lies far below |x|^2, nothing is exact.  The reference forms everything in np.longdouble
(distances as sums of squared differences: no cancellation), the bounds are first order in u, hold for any order of the sums, and
take absdot = |A| |B|':
    linear      (d + 2) u absdot
    rbf         K (gamma (d + 4) u (|a|^2 + |b|^2 + 2 absdot) + 4 u)
    sigmoid     (d + 4) u (gamma absdot + |coef0|) + 4 u
    poly        deg (|z| + dz)^(deg - 1) dz + 4 u |z|^deg,   dz = (d + 4) u (gamma absdot + |coef0|)
    laplacian   K (gamma (d + 2) u D + 4 u)
"""
import collections
import functools

import numpy as np

LD = np.longdouble
U = LD(2.0) ** -53
F32 = LD(2.0) ** -24
TINY = LD(2.0) ** -1000
MAPS = ('linear', 'poly', 'rbf', 'sigmoid', 'laplacian')
MAP_U = {'linear': 8, 'poly': 8, 'rbf': 8, 'sigmoid': 8, 'laplacian': 8}   # the map's share of the bound, in units of u
CHUNK = 1 << 22   # entries of a row block: the long-double temporaries of the large cases stay below 100 MB each

# the geometry of csrc/bq_gram.hip and csrc/bq_sym_layout.h
GT, GRAM_STRIP, GRAM_RECT_R, GRAM_RECT_S, SYM_TILE = 128, 8, 16, 4, 256


def walk_geometry(m, t):
    """run_gram's choice of the workgroup order for an m x t build: the XCD-rectangle walk is taken when
    tiles_m * strips >= 8 * GRAM_RECT_R * GRAM_RECT_S"""
    tiles_m, tiles_n = -(-m // GT), -(-t // GT)
    strips = -(-tiles_n // GRAM_STRIP)
    g = dict(tiles_m=tiles_m, strips=strips, walk=tiles_m * strips >= 8 * GRAM_RECT_R * GRAM_RECT_S, rect_rb=0, rect_sb=0, rects=0)
    if g['walk']:
        g['rect_rb'], g['rect_sb'] = -(-tiles_m // GRAM_RECT_R), -(-strips // GRAM_RECT_S)
        g['rects'] = -(-(g['rect_rb'] * g['rect_sb']) // 8) * 8   # padded to the 8 XCDs
    return g


def panel_elems(n):
    nb = -(-n // SYM_TILE)
    return SYM_TILE * SYM_TILE * nb * (nb + 1) // 2


# ---- the cases -----------------------------------------------------------------------------------------------------------------------
# group: which entry point the GPU module sends the case through; t None: kernel(X) (a `same` build), else kernel(A, B) with A m x d
# and B t x d; every case has its own seed, and `shift` moves its gamma (and coef0) away from its neighbours'
Case = collections.namedtuple('Case', 'group name degree m t d seed shift')


def case_id(c):
    name = c.name + (str(c.degree) if c.name == 'poly' else '')
    return '%s-%s-%s-d%d' % (c.group, name, '%d' % c.m if c.t is None else '%dx%d' % (c.m, c.t), c.d)


SQUARES = (1, 129, 130, 257, 385)
RECTS = ((1, 1), (129, 257), (257, 129), (300, 1025))
DS = (1, 16, 17, 33, 48, 65)
DEGREES = (2, 3, 5)


def _cases():
    seed = [1000]

    def case(group, name, degree, m, t, d):
        seed[0] += 1
        return Case(group, name, degree if name == 'poly' else 1, m, t, d, seed[0], seed[0] % 3)

    rect, panel, cancel, walk, stream = [], [], [], [], []
    # 1. every d meets every map at one square and one rectangular shape, every shape meets every map (the pairing turns with the map)
    for k, name in enumerate(MAPS):
        for i, d in enumerate(DS):
            rect.append(case('rect', name, DEGREES[(i + k) % 3], SQUARES[(i + k) % 5], None, d))
            m, t = RECTS[(i + k) % 4]
            rect.append(case('rect', name, DEGREES[(i + k + 1) % 3], m, t, d))
    # 2. the resident panel: one case per map and size, walked through every layout by the test
    for name in MAPS:
        for n, d, degree in ((129, 17, 2), (257, 33, 3), (385, 48, 5), (2049, 5, 3)):
            panel.append(case('panel', name, degree, n, None, d))
    # 3. cancellation
    for name in MAPS:
        cancel.append(case('cancel', name, 3, 385, None, 33))
        cancel.append(case('cancel', name, 5, 300, 257, 48))
    for name in ('rbf', 'laplacian'):
        cancel.append(case('cancel', name, 1, 130, None, 1))
    # 4. the XCD-rectangle walk
    for name in ('rbf', 'linear'):
        walk.append(case('walkpanel', name, 1, 8200, None, 4))
        walk.append(case('walkrect', name, 1, 65700, 130, 4))
        walk.append(case('walkrect', name, 1, 32900, 1100, 4))
    # 5. the streamed product
    for name in ('linear', 'poly', 'rbf', 'sigmoid'):
        for n, d in ((129, 17), (1300, 9)):
            stream.append(case('stream', name, 3, n, None, d))
    return rect, panel, cancel, walk, stream


RECT_CASES, PANEL_CASES, CANCEL_CASES, WALK_CASES, STREAM_CASES = _cases()
ALL_CASES = RECT_CASES + PANEL_CASES + CANCEL_CASES + WALK_CASES + STREAM_CASES
assert len({c.seed for c in ALL_CASES}) == len(ALL_CASES)


# ---- inputs --------------------------------------------------------------------------------------------------------------------------
def frozen(*arrays):
    for a in arrays:
        if a is not None:
            a.setflags(write=False)
    return arrays


def grid(rs, shape, xmax=2.0):
    """multiples of 2^-6 in [-xmax, xmax]"""
    n = int(round(xmax * 64))
    return rs.randint(-n, n + 1, size=shape) / 64.0


@functools.lru_cache(maxsize=8)
def operands(c):
    """(A, B): A m x d, B t x d or None (kernel(A)); shared by the tests, which leave them unchanged"""
    rs = np.random.RandomState(c.seed)
    if c.group == 'cancel':
        A = 20.0 + rs.standard_normal((c.m, c.d))
        if c.t is None:
            dup = np.arange(6, c.m, 7)
            A[dup] = A[dup - 1] + 1e-7 * rs.standard_normal((len(dup), c.d))
            return frozen(A, None)
        B = 20.0 + rs.standard_normal((c.t, c.d))
        dup = np.arange(6, c.m, 7)
        A[dup] = B[dup % c.t] + 1e-7 * rs.standard_normal((len(dup), c.d))
        return frozen(A, B)
    scale = 64.0 if c.name == 'linear' else 1.0   # the linear kernel: the grid as integers
    A = grid(rs, (c.m, c.d)) * scale
    B = None if c.t is None else grid(rs, (c.t, c.d)) * scale
    return frozen(A, B)


def near_duplicates(c):
    """(rows, columns) of the near-duplicate pairs of a cancellation case"""
    dup = np.arange(6, c.m, 7)
    return (dup, dup - 1) if c.t is None else (dup, dup % c.t)


def spec(c):
    """(name, gamma, coef0, degree) of a case"""
    A, B = operands(c)
    d = c.d
    if c.name == 'linear':
        return ('linear', 0.0, 0.0, 1)
    if c.group == 'cancel':   # ordinary figures: the arguments are of order one
        f = 1.0 + 0.1 * c.shift
        return {'rbf': ('rbf', 0.4 * f / d, 0.0, 1), 'laplacian': ('laplacian', 0.7 * f / d, 0.0, 1),
                'poly': ('poly', f / (400.0 * d), 0.3, c.degree), 'sigmoid': ('sigmoid', f / (400.0 * d), -0.9, 1)}[c.name]
    down = 2.0 ** -c.shift
    if c.name == 'rbf':
        # the largest power of two with exp(-gamma 4 max |x|^2) >= 2^-14: every value lies in [2^-14, 1], the rule under which a
        # packed fp64 panel takes the 7-byte layout (bq_c7_eligible); `down` only moves the values up
        m2 = max(1.0, max((X * X).sum(axis=1).max() for X in (A, B) if X is not None))
        return ('rbf', down * 2.0 ** np.floor(np.log2(14.0 * np.log(2.0) / (4.0 * m2))), 0.0, 1)
    if c.name == 'laplacian':   # gamma * (largest L1 distance on the grid) <= 10
        return ('laplacian', down * 2.0 ** np.floor(np.log2(10.0 / (4.0 * d))), 0.0, 1)
    if c.name == 'poly':        # |gamma x.y| <= 8
        return ('poly', down * 2.0 ** np.floor(np.log2(2.0 / d)), 0.25 * (1 + c.seed % 4), c.degree)
    return ('sigmoid', down * 2.0 ** np.floor(np.log2(d ** -0.5)), 0.25 * (c.seed % 4) - 0.5, 1)


# ---- the exact-argument reference ----------------------------------------------------------------------------------------------------
def _same(a64, ald):
    """the fp64 value is the long-double value: the argument is exact"""
    assert a64.dtype == np.float64 and ald.dtype == LD and a64.shape == ald.shape
    assert np.array_equal(a64, ald)   # (NumPy compares the pair in long double: the fp64 side widens exactly)


def _l1(A, B):
    D = np.zeros((len(A), len(B)), dtype=A.dtype)
    for k in range(A.shape[1]):   # a feature at a time: no m x t x d temporary
        D += np.abs(A[:, k][:, None] - B[:, k][None, :])
    return D


def _arguments_block(sp, A, B):
    name, gamma, coef0, _ = sp
    Al, Bl = A.astype(LD), B.astype(LD)
    if name == 'laplacian':
        arg = -gamma * _l1(A, B)
        _same(arg, -LD(gamma) * _l1(Al, Bl))
        assert (arg <= 0).all()
        return arg
    dot, dotl = A @ B.T, Al @ Bl.T
    _same(dot, dotl)
    if name == 'linear':
        assert np.array_equal(dot, np.rint(dot))
        return dot
    if name == 'rbf':
        a2, b2 = (A * A).sum(axis=1), (B * B).sum(axis=1)
        _same(a2, (Al * Al).sum(axis=1))
        _same(b2, (Bl * Bl).sum(axis=1))
        arg = (-2.0 * dot + a2[:, None]) + b2[None, :]   # the distance in the device's order; any order is exact
        assert (arg >= 0).all()
        arg *= -gamma   # a power of two: the argument is exact where the distance is
        dotl *= -2      # (in place: these are the 67 M entry temporaries of the largest cases)
        dotl += (Al * Al).sum(axis=1)[:, None]
        dotl += (Bl * Bl).sum(axis=1)[None, :]
        dotl *= -LD(gamma)
        _same(arg, dotl)
        return arg
    arg = gamma * dot + coef0
    _same(arg, LD(gamma) * dotl + LD(coef0))
    return arg


def _blocks(m, t):
    rows = max(1, CHUNK // max(t, 1))
    return [(r, min(m, r + rows)) for r in range(0, m, rows)]


def arguments(sp, A, B=None):
    """The map's argument of every entry of kernel(A, B) in fp64 (the inner product itself for the linear kernel), asserted equal
    to the same quantity in long double"""
    assert np.finfo(LD).nmant >= 63
    assert sp[0] == 'linear' or np.log2(sp[1]) % 1 == 0, 'gamma is a power of two'
    assert (sp[2] * 4) % 1 == 0, 'coef0 is a short dyadic'
    assert all(np.array_equal(X * 64, np.rint(X * 64)) for X in (A, B) if X is not None), 'the operands lie on the grid'
    if B is not None:
        arg = np.empty((len(A), len(B)))
        for r0, r1 in _blocks(len(A), len(B)):
            arg[r0:r1] = _arguments_block(sp, A[r0:r1], B)
        return arg
    # kernel(A): a row block against the rows up to its own end; the exact values are symmetric, so the rest is their mirror image
    arg = np.empty((len(A), len(A)))
    for r0, r1 in _blocks(len(A), len(A)):
        arg[r0:r1, :r1] = _arguments_block(sp, A[r0:r1], A[:r1])
        arg[:r0, r0:r1] = arg[r0:r1, :r0].T
    return arg


def apply_map(sp, arg, wide=True):
    """The map on exact arguments: in long double, or (wide=False, the 67 M entry cases) in fp64, <= 1 ulp from it.  No value lies
    below 2^-1000 — an exact zero stands only where a polynomial's or the sigmoid's argument is exactly zero, or in the integer
    product."""
    name, _, _, degree = sp
    if name == 'linear':
        return arg.astype(LD) if wide else arg
    out = np.empty(arg.shape, dtype=LD if wide else np.float64)
    for r0, r1 in _blocks(*arg.shape):
        a = arg[r0:r1].astype(LD) if wide else arg[r0:r1]
        ref = np.exp(a) if name in ('rbf', 'laplacian') else np.tanh(a) if name == 'sigmoid' else a ** degree
        small = np.abs(ref) < (TINY if wide else 2.0 ** -1000)
        assert not small.any() if name in ('rbf', 'laplacian') else (a[small] == 0).all()
        out[r0:r1] = ref
    return out


@functools.lru_cache(maxsize=4)
def exact_reference(c, wide=True):
    """(spec, A, B, ref) of an exact-argument case"""
    assert c.group != 'cancel'
    A, B = operands(c)
    sp = spec(c)
    return (sp, A, B) + frozen(apply_map(sp, arguments(sp, A, B), wide))


def exact_bound(name, ref, f32=False):
    b = MAP_U[name] * (U if ref.dtype == LD else 2.0 ** -53) * np.abs(ref)
    return b + (F32 if ref.dtype == LD else 2.0 ** -24) * np.abs(ref) if f32 else b


# ---- the cancellation reference ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=4)
def cancel_reference(c):
    """(spec, A, B, ref, bound) of a cancellation case, all in long double"""
    assert c.group == 'cancel' and np.finfo(LD).nmant >= 63
    A, B = operands(c)
    name, gamma, coef0, degree = sp = spec(c)
    Al, Bl = A.astype(LD), (A if B is None else B).astype(LD)
    d, g = c.d, LD(gamma)
    dot, absdot = Al @ Bl.T, np.abs(Al) @ np.abs(Bl).T
    if name == 'linear':
        ref, bound = dot, (d + 2) * U * absdot
    elif name == 'rbf':
        D = np.zeros_like(dot)
        for k in range(d):
            D += (Al[:, k][:, None] - Bl[:, k][None, :]) ** 2
        ref = np.exp(-g * D)
        sq = (Al * Al).sum(axis=1)[:, None] + (Bl * Bl).sum(axis=1)[None, :]
        bound = ref * (g * (d + 4) * U * (sq + 2 * absdot) + 4 * U)
    elif name == 'laplacian':
        D = _l1(Al, Bl)
        ref = np.exp(-g * D)
        bound = ref * (g * (d + 2) * U * D + 4 * U)
    else:
        z, dz = g * dot + LD(coef0), (d + 4) * U * (g * absdot + abs(LD(coef0)))
        if name == 'sigmoid':
            ref, bound = np.tanh(z), dz + 4 * U
        else:
            ref, bound = z ** degree, degree * (np.abs(z) + dz) ** (degree - 1) * dz + 4 * U * np.abs(z) ** degree
    return (sp, A, B) + frozen(ref, bound)


# ---- the comparison ------------------------------------------------------------------------------------------------------------------
def within(label, name, K, ref, bound):
    """Assert |K - ref| <= bound on every entry (no entry is left out) and print and return the largest |K - ref| / bound.  Where
    the bound is 0 the values must be equal.  In fp64 where the reference is fp64 (the largest cases): the difference of two
    doubles within a factor of two of each other is exact, and so is 8 u |ref|."""
    assert K.dtype == np.float64 and K.shape == ref.shape == bound.shape, label
    ratio, worst_err = 0.0, 0.0
    for r0, r1 in _blocks(*K.shape) if K.ndim == 2 else [(0, len(K))]:
        k, r, b = K[r0:r1], ref[r0:r1], bound[r0:r1]
        assert np.isfinite(k).all(), label
        err = np.abs(k.astype(ref.dtype) - r)
        bad = err > b
        if bad.any():
            at = np.unravel_index(np.argmax(np.where(bad, err - b, -np.inf)), err.shape)
            entry = (at[0] + r0,) + tuple(at[1:])
            raise AssertionError('%s [%s]: entry %s: K = %r, ref = %r, |K - ref| = %.3e, bound %.3e; %d entries of this block miss'
                                 % (label, name, entry, float(k[at]), float(r[at]), float(err[at]), float(b[at]), int(bad.sum())))
        live = b > 0
        if live.any():
            ratio = max(ratio, float((err[live] / b[live]).max()))
        worst_err = max(worst_err, float(err.max()) if err.size else 0.0)
    print('%s [%s]: max |K - ref| / bound = %.3g (max |K - ref| = %.3e)' % (label, name, ratio, worst_err))
    return ratio


def same_bits(label, K, want):
    """the integer linear kernel: equal bits, no tolerance"""
    assert K.dtype == np.float64 and K.shape == want.shape, label
    want = want.astype(np.float64)
    if not np.array_equal(K, want):
        at = np.unravel_index(np.argmax(K != want), K.shape)
        raise AssertionError('%s [linear]: entry %s: K = %r, integer product %r; %d entries differ'
                             % (label, at, float(K[at]), float(want[at]), int((K != want).sum())))
    print('%s [linear]: equal bits' % label)
    return 0.0


def check_exact(label, name, K, ref, f32=False):
    """an exact-argument Gram matrix against its reference: equal bits for the integer linear kernel, the map's bound otherwise"""
    if name == 'linear':
        assert not f32 or np.abs(ref).max() < 2 ** 24
        return same_bits(label, K, ref)
    return within(label, name, K, ref, exact_bound(name, ref, f32))


# ---- the streamed product ------------------------------------------------------------------------------------------------------------
def dyadic_vector(c):
    """multiples of 2^-6 in [-2, 2]; small integers for the integer linear case"""
    rs = np.random.RandomState(c.seed + 50000)
    v = rs.randint(-4, 5, size=c.m).astype(float) if c.name == 'linear' else grid(rs, c.m)
    v.setflags(write=False)
    return v


def product_reference(ref, v):
    """(K v, |K| |v|) in long double"""
    Kl, vl = ref.astype(LD), v.astype(LD)
    return Kl @ vl, np.abs(Kl) @ np.abs(vl)


def product_bound(name, n, ref, S):
    """n-term sum in any order plus the map"""
    return (n + MAP_U[name]) * U * S + U * np.abs(ref)
