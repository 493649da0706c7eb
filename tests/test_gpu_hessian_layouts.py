"""The Hessian the factorising solvers assemble element by element (csrc/bq_qelem.h: InteriorPoint, ActiveSet's restricted systems
and kept-factor columns, x_star), on every panel layout that is not the packed symmetric one the rest of the suite uses:

  dense row blocks   a Q that is not symmetric (the reference's cho_factor reads its UPPER triangle), an exactly symmetric Q forced
                     into rows, and — packed, for contrast — a Q whose upper triangle is garbage under `symmetric=True`;
  full panels        kernel problems with `full_panel=True` (whole rows of pitch round_up(n, 1024)), SVC / SVR / plain structure.

The reference is always the oracle on the host matrix (for fp32 storage: on the matrix rounded to fp32), never another device
layout.  Tolerances are test_ragged_sizes_dense's: status and iteration count equal, f history rtol 1e-8 / atol 1e-10, x rtol
1e-6 / atol 1e-8; x_star rtol 1e-9 as test_quadratic_x_star_and_f_star.  tests/test_hessian_layouts_host.py shows that the inputs
tell the triangles apart by >= 100 of these tolerances and that the references do not hang on the last bits of K.

Measured on one MI355X (70 cases, 5.5 s).  Largest distance from the oracle, in tolerances: x_star 0.016 (full-panel SVC, n = 300),
f histories 3.3e-4, x 1.9e-6.  Before the fix (the library of the commit before this file) 61 of the first 64 cases failed:
  non-symmetric rows   the LOWER triangle was factorised: x_star 2.8e6 (n = 5) to 1.1e9 (n = 520) tolerances off, InteriorPoint's f
                       history 6.4e3 to 8.8e5, ActiveSet's 6.6e5 to 1.0e7 and its x 4.3e2 to 1.6e5 — to the digit what the host test
                       gets for the oracle reading the other triangle;
  product-free f       against the oracle reading that same lower triangle the re-factorising ActiveSet took every step the oracle
                       took (x within 5e-8 tolerances) but recorded f 6e-5 to 7e-3 relative off (6.0e3 to 6.4e5 tolerances; with hook
                       as_f_chain=0: 4e-6 tolerances);
  kept factor          with the triangle right and the product-free f off, the 'reuse' modes were still 4.9e2 to 9.9e4 tolerances off
                       in f and 2.6e2 to 3.3e4 in x: a pinned base variable enters through the mirrored H, not through Q as given;
  full panels          SVC / SVR / K + 1 entries were read at the packed address: x_star fell into MINRES (1.6e7 to 4.2e10
                       tolerances off), ActiveSet ran to its iteration cap, InteriorPoint on SVR raised "non-positive pivot", the
                       squared-hinge ActiveSet stopped at its cap 9e7 tolerances off.  The plain structure was read right.
The packed 'lower' cases passed before and after.
"""
import functools

import numpy as np
import pytest

import hessian_layout_reference as hl
from conftest import set_hooks
from oracle import bcqp_oracle as bo

pytestmark = pytest.mark.gpu

AS_MODES = {'refactor': dict(as_schur=0), 'reuse': dict(as_schur_min=0), 'reuse-block4096': dict(as_schur_min=0, sweep_block=4096)}


def _set_mode(monkeypatch, mode):
    """test_gpu_parity.py's as_factor_mode: re-factorise every iteration, or keep a base factor from the first iteration on"""
    set_hooks(monkeypatch, **{'as_schur': None, 'as_schur_min': None, 'sweep_block': None, **AS_MODES[mode]})


@pytest.fixture(scope='module')
def amd():
    import optiml_amd
    from optiml_amd import _lib
    from optiml_amd.device import get_context
    _lib.load()
    get_context()
    return optiml_amd


def _kernel():
    from optiml_amd.ml.svm.kernels import GaussianKernel
    return GaussianKernel(gamma=hl.GAMMA)


def _minimize(name, quad, ub, lb=None, x=None, max_iter=1000):
    """(optimizer after minimize(), the f history its callback saw)"""
    from optiml_amd.opti.constrained import ActiveSet, InteriorPoint
    hist = []
    cb = lambda o: hist.append(o.f_x)
    cb._bq_needs_state = False
    opt = {'as': ActiveSet, 'ip': InteriorPoint}[name](quad=quad, ub=ub, lb=lb, x=x, max_iter=max_iter, callback=cb).minimize()
    return opt, np.array(hist)


def _check_run(opt, hist, ref, label):
    print(f'{label}: {opt.status} after {opt.iter} iterations (oracle: {ref["status"]}, {ref["iter"]}), f history '
          f'{hl.margin(hist, ref["f_hist"], **hl.F_TOL):.3g} tolerances from the oracle, x {hl.margin(opt.x, ref["x"], **hl.X_TOL):.3g}')
    assert (opt.status, opt.iter) == (ref['status'], ref['iter']), label
    np.testing.assert_allclose(hist, ref['f_hist'], err_msg=label, **hl.F_TOL)
    np.testing.assert_allclose(opt.x, ref['x'], err_msg=label, **hl.X_TOL)


def _check_x_star(quad, ref_x, ref_method, label):
    x = quad.x_star()
    print(f'{label}: x_star by {quad.x_opt_method}, {hl.margin(x, ref_x, **hl.xstar_tol(ref_x)):.3g} tolerances from the oracle')
    assert quad.x_opt_method == ref_method == 'cholesky', label   # a garbage H fails its pivot test and hides in MINRES
    np.testing.assert_allclose(x, ref_x, err_msg=label, **hl.xstar_tol(ref_x))


# ---- references: computed once per case, read by several tests, never written to -------------------------------------------------
@functools.lru_cache(maxsize=None)
def _dense_ref(kind, n, storage='f64'):
    if kind == 'nonsym':
        Q, q, ub, lb = hl.nonsymmetric_case(n)
        given = host = hl.rounded(Q, storage)
    elif kind == 'lower':
        given, host, q, ub, lb = hl.lower_only_case(n)
    else:
        Q, q, ub, lb = hl.rounding_case(n)
        given = host = Q
    ref = hl.solve_all(host, q, ub, lb, 'upper', n)
    return given, q, ub, lb, ref


def _dense_quad(kind, n, storage='f64'):
    from optiml_amd.opti import Quadratic
    given, q, ub, lb, ref = _dense_ref(kind, n, storage)
    # fp32 storage is handed the fp64 matrix: the device rounds it, the oracle ran on the rounded one
    Q = hl.nonsymmetric_case(n)[0] if kind == 'nonsym' else given
    quad = Quadratic(Q, q, storage=storage, symmetric=(kind == 'lower'))
    assert quad.device_problem().layout()['packed'] is (kind == 'lower')
    return quad, ub, lb, ref


NONSYM = [(n, s) for n in hl.NONSYM_SIZES for s in ('f64', 'f32') if not (n == 520 and s == 'f32')]


# ---- dense row blocks, Q not symmetric -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n,storage', NONSYM)
def test_nonsymmetric_rows_x_star(amd, n, storage):
    quad, ub, lb, ref = _dense_quad('nonsym', n, storage)
    _check_x_star(quad, ref['x_star'], ref['x_star_method'], f'nonsym x_star n={n} {storage}')
    quad.release()


@pytest.mark.parametrize('n,storage', NONSYM)
def test_nonsymmetric_rows_interior_point(amd, n, storage):
    quad, ub, lb, ref = _dense_quad('nonsym', n, storage)
    opt, hist = _minimize('ip', quad, ub, lb, max_iter=hl.IP_ITERS)
    _check_run(opt, hist, ref['ip'], f'nonsym ip n={n} {storage}')
    quad.release()


@pytest.mark.parametrize('n,storage,mode', [(n, s, m) for n, s in NONSYM for m in AS_MODES if n != 520 or m == 'reuse'])
def test_nonsymmetric_rows_active_set(amd, monkeypatch, n, storage, mode):
    """The restricted systems come from the upper triangle, the right-hand sides, f and g from Q as given.  The kept factor and
    the product-free f of ratio steps both need the two to be one matrix: on such a Q they are off, whatever the hooks ask."""
    _set_mode(monkeypatch, mode)
    quad, ub, lb, ref = _dense_quad('nonsym', n, storage)
    opt, hist = _minimize('as', quad, ub, lb, max_iter=hl.as_iters(n))
    _check_run(opt, hist, ref['as'], f'nonsym as n={n} {storage} {mode}')
    assert opt.minres_iterations == 0
    assert opt.product_free_iterations == 0
    assert opt.reused_factor_iterations == 0
    quad.release()


# ---- dense, the two other layouts ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', hl.OTHER_SIZES)
@pytest.mark.parametrize('kind', ['lower', 'rounding'])
def test_dense_lower_only_and_symmetric_rows(amd, monkeypatch, kind, n):
    """'lower': symmetric=True on a Q whose strict upper triangle is garbage — packed, only the lower triangle may be read.
    'rounding': an exactly symmetric Q under symmetric=False — row blocks, the layout alone differs from the usual tests."""
    quad, ub, lb, ref = _dense_quad(kind, n)
    _check_x_star(quad, ref['x_star'], ref['x_star_method'], f'{kind} x_star n={n}')
    opt, hist = _minimize('ip', quad, ub, lb, max_iter=hl.IP_ITERS)
    _check_run(opt, hist, ref['ip'], f'{kind} ip n={n}')
    for mode in ('refactor', 'reuse'):
        _set_mode(monkeypatch, mode)
        opt, hist = _minimize('as', quad, ub, lb, max_iter=hl.as_iters(n))
        _check_run(opt, hist, ref['as'], f'{kind} as n={n} {mode}')
        assert opt.minres_iterations == 0
        # H == Q in both: the kept factor and the product-free f stay on, in the packed layout and in row blocks alike
        assert (opt.reused_factor_iterations > 0) == (mode == 'reuse') and opt.product_free_iterations > 0
    quad.release()


@pytest.mark.parametrize('ulps,shortcuts', [(1, True), (32, True), (128, False)])
@pytest.mark.parametrize('n', hl.OTHER_SIZES)
def test_rows_symmetric_up_to_rounding_keep_the_shortcuts(amd, monkeypatch, n, ulps, shortcuts):
    """A Q assembled in floating point differs from its transpose in last bits and lands in row blocks by itself.  The kept factor
    and the product-free f err there by that asymmetry, so they stay on while max |Q_ij - Q_ji| <= 64 ulps of max |Q| and go off
    beyond: either side of the threshold, the run is the oracle's (128 ulps of asymmetry are 3e-14, far below every tolerance)."""
    from optiml_amd.opti import Quadratic
    Q, q, ub, lb = hl.rounding_case(n)
    Q = hl.with_asymmetry(Q, ulps)
    ref = bo.active_set(Q, q, ub, lb=lb, max_iter=hl.as_iters(n))
    _set_mode(monkeypatch, 'reuse')
    quad = Quadratic(Q, q)
    assert quad.device_problem().layout()['packed'] is False
    opt, hist = _minimize('as', quad, ub, lb, max_iter=hl.as_iters(n))
    _check_run(opt, hist, ref, f'{ulps} ulps of asymmetry n={n}')
    assert (opt.reused_factor_iterations > 0) == shortcuts and (opt.product_free_iterations > 0) == shortcuts
    quad.release()


# ---- kernel problems on a full panel ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _svc_ref(n):
    X, y, Q, q, ub = hl.svc_case(n)
    xs, method = bo.x_star(Q, q)
    return {'x_star': xs, 'x_star_method': method, 'ip': bo.interior_point(Q, q, ub, max_iter=200),
            'as': bo.active_set(Q, q, ub, max_iter=hl.as_iters(n))}


def _svc_quad(n):
    from optiml_amd.opti import KernelQuadratic
    X, y, Q, q, ub = hl.svc_case(n)
    quad = KernelQuadratic(X, q, 'svc', _kernel(), y=y, full_panel=True)
    assert quad.device_problem().layout()['packed'] is False
    return quad, ub


@pytest.mark.parametrize('n', hl.SVC_SIZES)
def test_full_panel_svc_x_star_and_interior_point(amd, n):
    quad, ub = _svc_quad(n)
    ref = _svc_ref(n)
    _check_x_star(quad, ref['x_star'], ref['x_star_method'], f'full-panel svc x_star n={n}')
    opt, hist = _minimize('ip', quad, ub, max_iter=200)
    _check_run(opt, hist, ref['ip'], f'full-panel svc ip n={n}')
    quad.release()


@pytest.mark.parametrize('mode', ['refactor', 'reuse'])
@pytest.mark.parametrize('n', hl.SVC_SIZES)
def test_full_panel_svc_active_set(amd, monkeypatch, n, mode):
    _set_mode(monkeypatch, mode)
    quad, ub = _svc_quad(n)
    opt, hist = _minimize('as', quad, ub, max_iter=hl.as_iters(n))
    _check_run(opt, hist, _svc_ref(n)['as'], f'full-panel svc as n={n} {mode}')
    assert opt.minres_iterations == 0
    assert (opt.reused_factor_iterations > 0) == (mode == 'reuse')   # the kept factor's columns read the panel too
    quad.release()


@functools.lru_cache(maxsize=None)
def _svr_ref(n):
    X, Q, q, ub = hl.svr_case(n)
    return {'ip': bo.interior_point(Q, q, ub, max_iter=200), 'as': bo.active_set(Q, q, ub, max_iter=hl.as_iters(2 * n))}


def _svr_quad(n):
    from optiml_amd.opti import KernelQuadratic
    X, Q, q, ub = hl.svr_case(n)
    quad = KernelQuadratic(X, q, 'svr', _kernel(), full_panel=True)
    assert quad.device_problem().layout()['packed'] is False
    return quad, ub


@pytest.mark.parametrize('form', ['reduced', 'full-2n'])
@pytest.mark.parametrize('n', hl.SVR_SIZES)
def test_full_panel_svr_interior_point(amd, monkeypatch, n, form):
    """The default n x n system in u = dx+ - dx- (K + 1 read once per entry) and the reference's own 2n x 2n one (hook
    ip_svr_reduced=0: the four blocks of the panel's mirror images)."""
    if form == 'full-2n':
        set_hooks(monkeypatch, ip_svr_reduced=0)
    quad, ub = _svr_quad(n)
    opt, hist = _minimize('ip', quad, ub, max_iter=200)
    _check_run(opt, hist, _svr_ref(n)['ip'], f'full-panel svr ip n={n} {form}')
    quad.release()


@pytest.mark.parametrize('n', hl.SVR_SIZES)
def test_full_panel_svr_active_set(amd, n):
    """ActiveSet on the singular 2n x 2n SVR Hessian starts in the reference's minres branch, whose candidates carry rounding noise
    along a+ + a-: the oracle's own f history moves by 5.4e5 (n = 40) and 680 (n = 129) tolerances when K moves by one ulp
    (test_hessian_layouts_host.py), while status, end point and final objective stay within a tenth of a tolerance.  Those three
    are held to the oracle; both H assemblies of the solver (the factorised lower triangle, the full square of the minres branch)
    have to read the full panel right for the end point to be the optimum."""
    quad, ub = _svr_quad(n)
    ref = _svr_ref(n)['as']
    opt, hist = _minimize('as', quad, ub, max_iter=hl.as_iters(2 * n))
    print(f'full-panel svr as n={n}: {opt.status} after {opt.iter} iterations (oracle {ref["iter"]}), {opt.minres_iterations} through '
          f'minres, x {hl.margin(opt.x, ref["x"], **hl.X_TOL):.3g} tolerances from the oracle, f {hl.margin(opt.f_x, ref["f_x"], **hl.F_TOL):.3g}')
    assert opt.status == ref['status'] == 'optimal'
    np.testing.assert_allclose(opt.f_x, ref['f_x'], **hl.F_TOL)
    np.testing.assert_allclose(opt.x, ref['x'], **hl.X_TOL)
    quad.release()


def test_full_panel_plain_with_diagonal(amd, monkeypatch):
    from optiml_amd.opti import KernelQuadratic
    n = 129
    X, Q, q, ub, diag = hl.plain_case(n)
    quad = KernelQuadratic(X, q, 'plain', _kernel(), diag=diag, full_panel=True)
    assert quad.device_problem().layout()['packed'] is False
    xs, method = bo.x_star(Q, q)
    _check_x_star(quad, xs, method, 'full-panel plain x_star')
    ref = bo.active_set(Q, q, ub, max_iter=hl.as_iters(n))
    for mode in ('refactor', 'reuse'):
        _set_mode(monkeypatch, mode)
        opt, hist = _minimize('as', quad, ub, max_iter=hl.as_iters(n))
        _check_run(opt, hist, ref, f'full-panel plain as {mode}')
        assert opt.minres_iterations == 0
    quad.release()


def test_full_panel_squared_hinge_active_set(amd, monkeypatch):
    from optiml_amd.opti import KernelQuadratic
    n = 129
    X, y, Q, q, ub, x0, diag = hl.sqhinge_case(n)
    quad = KernelQuadratic(X, q, 'svc', _kernel(), y=y, diag=diag, full_panel=True)
    assert quad.device_problem().layout()['packed'] is False
    ref = bo.active_set(Q, q, ub, x0=x0, max_iter=hl.as_iters(n))
    for mode in ('refactor', 'reuse'):
        _set_mode(monkeypatch, mode)
        opt, hist = _minimize('as', quad, ub, x=x0, max_iter=hl.as_iters(n))
        _check_run(opt, hist, ref, f'full-panel squared hinge as {mode}')
        assert opt.minres_iterations == 0
        assert int((opt.x > 1e-6).sum()) == int((ref['x'] > 1e-6).sum())
    quad.release()
