"""The blocked Cholesky (csrc/bq_chol.hip, bq_potrf_diag.hip) at the places where it changes behaviour, reached at orders up to 3200
through the test hooks chol_lookahead, chol_passes, chol_super_min, chol_fwd_slice and sweep_block and the diagnostic entry
bq_cholesky_probe (optiml_amd.linalg._cholesky_probe): the two-stream look-ahead, P = 1 .. 4 passes per super-pass, the super-tile
order of the wide update, the sliced forward sweep, the prepared sweeps over several big blocks with a ragged last one and a start
past the first, the factor itself and the index info reports.

Input: A = diag(d) + U U^T, d uniform in [1, 2], U n x 64 standard normal / sqrt(max(n, 64)), seed n: dense in every tile,
condition number below 5, cheap to build.

Yardstick: the algorithm's backward-error bound, evaluated on the host in fp64 (u = 2^-53, np = n rounded up to 128):
  factor  rho   = max_{i >= j} |A - L L^T|_ij / (u (|L| |L|^T)_ij)   <= 2 np + 2   (gamma of the factorisation + gamma of the host's product)
  solve   sigma = max_i |b - A x|_i / (u (|L| |L|^T |x|)_i)          <= 4 np + 4   (Higham, Accuracy and Stability, Thms 10.3, 10.4)
The device forms triangular inverses of the diagonal blocks, in theory a factor kappa(L_KK) <= sqrt(kappa(A)) < 3 here.  scipy's LAPACK
factor of these matrices gives rho = 2.7 / 5.5 / 6.0 / 6.2 and sigma = 2.0 / 7.4 / 7.3 / 11.6 at n = 129 / 1500 / 2304 / 3200, so the
caps leave three orders of magnitude for another correct summation order, and a single dropped tile update gives rho ~ 1e15.
Every test prints the figures it measured before it asserts.  Measured on an MI355X (largest over P = 1 .. 4) / scipy on the same matrix:
  rho    n=127 6.4 / 3.2   128 8.5 / 3.3   129 7.5 / 3.0   256 8.7 / 4.4   383 9.4 / 3.9   640 8.5 / 3.6   1025 8.0 / 5.0   1536 9.1 / 5.6
         2049 9.6 / 6.0   2304 10.2 / 5.7   2500 12.4 / 5.9   3200 11.2 / 7.3
  sigma  (largest over the start rows and solve modes)   n=1024 11.4 / 8.4   1025 7.4 / 8.3   2304 12.5 / 11.2   3200 15.1 / 11.4"""
import functools

import numpy as np
import pytest

from conftest import set_hooks

pytestmark = pytest.mark.gpu

U_ROUND = 2.0 ** -53
ORDERS = [1, 127, 128, 129, 256, 383, 640, 1025, 1536, 2049, 2304, 2500, 3200]   # 1, 2, 3, 5, 9, 12, 17, 18, 20, 25 block columns
PASSES = [1, 2, 3, 4]
CHOL_HOOKS = ('chol_lookahead', 'chol_passes', 'chol_super_min', 'chol_fwd_slice', 'sweep_block')


@pytest.fixture(scope='module')
def probe():
    from optiml_amd import _lib
    from optiml_amd.device import get_context
    from optiml_amd.linalg import _cholesky_probe
    _lib.load()
    get_context()
    return _cholesky_probe


def hooks(monkeypatch, **kw):
    """exactly these Cholesky hooks for the rest of the test (the others of the process stay)"""
    set_hooks(monkeypatch, **{**{h: None for h in CHOL_HOOKS}, **kw})


@functools.lru_cache(maxsize=None)
def matrix(n):
    rs = np.random.RandomState(n)
    d = rs.uniform(1.0, 2.0, n)
    U = rs.standard_normal((n, 64)) / np.sqrt(max(n, 64))
    A = U @ U.T
    A[np.diag_indices(n)] += d
    A.setflags(write=False)
    return A


def padded(n):
    return -(-n // 128) * 128


def rho(A, L):
    """backward error of the factor in units of u |L| |L|^T, over the lower triangle"""
    R = np.abs(A - L @ L.T)
    aL = np.abs(L)
    D = aL @ aL.T
    low = np.tril_indices(A.shape[0])
    return float(np.max(R[low] / (U_ROUND * D[low])))


def sigma(A, L, b, x):
    """backward error of one solve in units of u |L| |L|^T |x|"""
    aL = np.abs(L)
    return float(np.max(np.abs(b - A @ x) / (U_ROUND * (aL @ (aL.T @ np.abs(x))))))


def factor(probe, n):
    X, L, info = probe(matrix(n))
    assert info == 0
    assert X.shape == (0, n)
    return L


# ---- 1. the factor against its definition ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('P', PASSES)
@pytest.mark.parametrize('n', ORDERS)
def test_factor_satisfies_its_backward_error_bound(probe, monkeypatch, n, P):
    hooks(monkeypatch, chol_lookahead=0, chol_passes=P)
    L = factor(probe, n)
    assert np.isfinite(L).all()
    assert not np.triu(L, 1).any(), 'the strict upper triangle of L is not exactly zero'
    r = rho(matrix(n), L)
    print(f'factor n={n} P={P}: rho = {r:.2f} (cap {2 * padded(n) + 2})')
    assert r <= 2 * padded(n) + 2


# ---- 2. look-ahead = single stream, bit for bit ---------------------------------------------------------------------------------
@pytest.mark.parametrize('P', PASSES)
@pytest.mark.parametrize('n', ORDERS)
def test_lookahead_order_gives_the_single_stream_factor_bit_for_bit(probe, monkeypatch, n, P):
    """the kernels and their kdim are the same; only the issue order and the streams differ"""
    hooks(monkeypatch, chol_lookahead=0, chol_passes=P)
    single = factor(probe, n)
    hooks(monkeypatch, chol_lookahead=1, chol_passes=P)
    two = factor(probe, n)
    assert np.array_equal(single, two), f'{np.count_nonzero(single != two)} entries differ'


@pytest.mark.parametrize('n', [2049, 2304, 3200])
def test_default_path_is_two_passes_with_lookahead_bit_for_bit(probe, monkeypatch, n):
    """17 block columns and more: without hooks the driver takes P = 2 on two streams, and the hooks that force it change nothing"""
    hooks(monkeypatch)
    plain = factor(probe, n)
    hooks(monkeypatch, chol_lookahead=1, chol_passes=2)
    forced = factor(probe, n)
    assert np.array_equal(plain, forced), f'{np.count_nonzero(plain != forced)} entries differ'
    r = rho(matrix(n), plain)
    print(f'factor n={n} no hooks: rho = {r:.2f} (cap {2 * padded(n) + 2})')
    assert r <= 2 * padded(n) + 2


# ---- 3. super-tile order = row-major order, bit for bit -------------------------------------------------------------------------
@pytest.mark.parametrize('P', [1, 2])
@pytest.mark.parametrize('n', [1536, 2304, 3200])
def test_super_tile_order_gives_the_row_major_factor_bit_for_bit(probe, monkeypatch, n, P):
    """chol_super_min=1: every wide update takes the 8 x 8 super-tile map (at 3200 with P = 1 the first trailing triangle has 21 tile
    rows: three ragged rows of super-tiles)"""
    hooks(monkeypatch, chol_lookahead=0, chol_passes=P)
    row_major = factor(probe, n)
    hooks(monkeypatch, chol_lookahead=0, chol_passes=P, chol_super_min=1)
    super_tiles = factor(probe, n)
    assert np.array_equal(row_major, super_tiles), f'{np.count_nonzero(row_major != super_tiles)} entries differ'


# ---- 4. solves --------------------------------------------------------------------------------------------------------------------
def right_hand_sides(n, starts):
    rs = np.random.RandomState(n + 1)
    B = np.zeros((len(starts), n))
    for row, f in zip(B, starts):
        row[f:] = rs.standard_normal(n - f)
    return B


def check_solves(probe, n, starts, sweeps, label):
    A = matrix(n)
    B = right_hand_sides(n, starts)
    X, L, info = probe(A, B, first_nonzero=starts, sweeps=sweeps)
    assert info == 0
    assert np.isfinite(X).all() and not np.triu(L, 1).any()   # with the sweeps prepared the device's upper triangle holds L^T: not in L
    cap = 4 * padded(n) + 4
    sig = [sigma(A, L, b, x) for b, x in zip(B, X)]
    print(f'solve n={n} {label}: sigma = ' + ' '.join(f'{f}:{s:.2f}' for f, s in zip(starts, sig)) + f' (cap {cap})')
    assert max(sig) <= cap, dict(zip(starts, sig))
    return L


def starts_of(n):
    return [f for f in dict.fromkeys((0, 1, 127, 128, 1023, 1024, 1500, n - 129, n - 1)) if 0 <= f < n]


SOLVE_MODES = [('blocks', None), ('sweeps1024', 1024), ('sweeps2048', 2048)]


@pytest.mark.parametrize('mode', SOLVE_MODES, ids=[m[0] for m in SOLVE_MODES])
@pytest.mark.parametrize('n', [1024, 1025, 2304, 3200])
def test_solves_satisfy_their_backward_error_bound(probe, monkeypatch, n, mode):
    """block by block, and the prepared sweeps over one to four big blocks (the last ragged at 2304 and 3200), from start rows in the
    first block, on a block edge, in a later big block and in the last row"""
    label, bb = mode
    hooks(monkeypatch, chol_lookahead=0, **({} if bb is None else {'sweep_block': bb}))
    L = check_solves(probe, n, starts_of(n), bb is not None, label)
    assert rho(matrix(n), L) <= 2 * padded(n) + 2


def test_solves_with_one_ragged_big_block(probe, monkeypatch):
    hooks(monkeypatch, chol_lookahead=0, sweep_block=4096)
    check_solves(probe, 3200, starts_of(3200), True, 'sweeps4096')


@pytest.mark.parametrize('n', [2304, 3200])
def test_forward_sweep_in_two_to_four_slices(probe, monkeypatch, n):
    """chol_fwd_slice=512: the block rows' panel products are cut into 2, 3 and 4 column slices (default: one slice up to 16 384)"""
    hooks(monkeypatch, chol_lookahead=0, chol_fwd_slice=512)
    check_solves(probe, n, [0, 700], False, 'slices512')


# ---- 5. the first rejected pivot --------------------------------------------------------------------------------------------------
PIVOTS = [((700, 2200), -1.0), ((2175, 2176), -1.0), ((0,), -1.0), ((2303,), -1.0), ((1300,), float('nan'))]


def spoiled(positions, value):
    A = matrix(2304).copy()
    for k in positions:
        A[k, k] = value
    return A


@pytest.mark.parametrize('P', PASSES)
@pytest.mark.parametrize('case', PIVOTS, ids=['700+2200', '2175+2176', 'first', 'last', 'nan1300'])
def test_info_is_the_first_rejected_pivot(probe, monkeypatch, case, P):
    positions, value = case
    A = spoiled(positions, value)
    for la in (0, 1):
        hooks(monkeypatch, chol_lookahead=la, chol_passes=P)
        X, L, info = probe(A, np.ones((1, 2304)))
        assert info == min(positions) + 1, (la, info)
        assert np.isnan(X).all() and np.isnan(L).all(), 'X and L are left untouched'


def test_cho_solve_spd_names_the_rejected_minor(probe, monkeypatch):
    from optiml_amd.linalg import cho_solve_spd
    hooks(monkeypatch)
    with pytest.raises(np.linalg.LinAlgError, match='701-th leading minor'):
        cho_solve_spd(spoiled(*PIVOTS[0]), np.ones(2304))


# ---- 6. refusals --------------------------------------------------------------------------------------------------------------------
def test_probe_refuses_start_rows_that_do_not_fit_the_right_hand_side(probe):
    from optiml_amd import _lib
    A = matrix(256)
    b = np.ones((1, 256))
    for f in (-1, 256, 1 << 40):
        with pytest.raises(_lib.BcqpError) as e:
            probe(A, b, first_nonzero=[f])
        assert e.value.code == _lib.ERR_BADARG, f
    for f in (1, 255):   # b[0] is not zero
        with pytest.raises(_lib.BcqpError) as e:
            probe(A, b, first_nonzero=[f])
        assert e.value.code == _lib.ERR_BADARG, f
    b[0, :200] = 0.0
    X, L, info = probe(A, b, first_nonzero=[200])
    assert info == 0 and sigma(A, L, b[0], X[0]) <= 4 * 256 + 4
