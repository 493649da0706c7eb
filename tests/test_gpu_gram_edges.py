"""Every path of the Gram build (csrc/bq_gram.hip) against a long-double reference, entry by entry — the suite before this module held
the builder to an independent reference for RBF and degree-3 polynomial fp64 panels at the strip-layout sizes only; the sigmoid map,
the Laplacian kernel beyond one 64 x 64 tile, the XCD-rectangle walk, ragged rectangular builds, fp32 stores of anything but RBF
and the streamed product had none (test_streamed_product_matches_the_resident_panel compares two runs of the same epilogue).

Reference and bound (tests/gram_reference.py; the host side, test_gram_edges_host.py, holds the fp64 oracle to the same bounds and
shows that one entry moved by 16 u |ref| or one rolled column fails them).  Exact-argument family: operands on a dyadic grid
(multiples of 2^-6, |x| <= 2), gamma a power of two, coef0 a multiple of 1/4 — every dot product, norm, distance and map argument
is exact in fp64 (asserted against np.longdouble), the device and the reference differ in the map only, the reference is the map
in np.longdouble, and with u = 2^-53

    |K - ref| <= MAP_U u |ref|,  MAP_U = 8                  (+ 2^-24 |ref| for a panel stored in fp32)

The linear kernel runs on the grid scaled to integers and is compared for equal bits (in fp32 too).  No reference value lies below
2^-1000.  Cancellation family: rows with a common offset of 20 standard deviations and near-duplicate rows, reference all in long
double, first-order bounds that hold for any order of the sums (gram_reference's docstring).  No entry is masked or sampled in any
comparison; every case has its own seed and gamma, so a tile that is never written cannot hold a right value left by another case.

Which branch of bq_gram.hip each group exists for:
  1. test_rectangular_entry (kernel(X), kernel(A, B); bq_launch_gram_matrix, same = 1 and 0): the edge epilogue instance (every
     shape here has ragged tiles; 257, 385 and 300 x 1025 have whole ones beside them, which take the diagonal, degree-2,
     degree-3 and `any` instances), `store_elem` (odd t: 1, 129, 257, 385, 1025) against `store_pair` (130, even ragged), a
     second GRAM_STRIP of one column (t = 1025), 1, 2, 3 and 5 MFMA k-chunks (dp = 16, 32, 48, 80: odd and even counts),
     gram_l1_kernel's chunk tails (dp = 16, 48, 80 against LK = 32: 1, 2, 3 chunks) and its guarded edge stores.
  2. test_resident_panel (KernelQuadratic(...).gram()): lower_only builds into the packed layout — the diagonal instance (RBF),
     the degree-2, degree-3 and `any` (pow, tanh, linear) instances on interior tiles (n = 257, 385, 2049 have whole tiles), the
     tile-row limit of lower_only, bq_sym_addr past the first tile and in a second strip (n = 2049: nb = 9), gram_l1_kernel's
     lower_only skip, store_pair / store_elem of float, double and the three planes of the 7-byte layout, and the full panel
     (whole rows, same = 1, not packed).
  3. test_cancellation: the distance -2 x.y + |x|^2 + |y|^2 where it cancels, the clamp fmax(dist, 0) away from the diagonal
     (near-duplicate pairs must not exceed 1), the exact 1 on the diagonal of a `same` build.
  4. test_rectangle_walk_*: the XCD-rectangle walk (run_gram: tiles_m * strips >= 512) and its three early returns — padding
     rectangles (15 padded to 16, 33 to 40), a partial tile-row group (bx >= tiles_m), a partial strip group (by >= strips; in the
     tall case by = 1, 2, 3 of every rectangle) — and under lower_only the strips above the diagonal (j0 >= j1).
  5. test_streamed_product: gram_stream_sym_kernel per map (linear, degree 3, RBF with its diagonal instance, sigmoid) against
     (long-double K) v, bound (n + 8) u sum_j |K_ij| |v_j| + u |ref|; one tile per unit and stream_unit = 3.  That bound is 137 u
     and more, so on top every column K e_j (one term times 1, the rest times 0: exact sums) is held to the map's own 8 u |ref|.
     The Laplacian kernel is still refused in streamed mode.

The references of the walk cases (8.5 M to 67 M entries) are the fp64 map on the exact arguments: its own rounding (<= 1 ulp) is
inside the 8.  Everywhere else the reference is long double.

Observed on an MI355X (gfx950): largest max |K - ref| / bound per map and entry point, and the case it came from.
With the 8 as it stands — no map came near 1 on exact arguments, so none was measured on its own and no figure replaced the 8
(the integer linear kernel has equal bits at every entry point and no ratio):
    entry point                 poly    rbf     sigmoid  laplacian   (largest ratio at)
    rectangular, kernel(A[, B]) 0.248   0.160   0.169    0.148       poly3 300 x 1025 d 17, rbf 385 d 17, sigmoid 257 d 1, laplacian 129 d 17
    packed fp64 panel           0.233   0.148   0.169    0.146       poly3 2049 d 5, rbf 2049 d 5, sigmoid 385 d 48, laplacian 385 d 48
    compact (7-byte) panel              0.148                        rbf 2049 d 5: the bits of the packed fp64 panel
    packed fp32 panel           0.999   0.998   0.997    0.979       poly3 2049 d 5, rbf 257 d 33, sigmoid 257 d 33, laplacian 257 d 33
    full panel                  0.233   0.148   0.169    0.146       as the packed fp64 panel
    streamed, K e_j, all j      0.245   0.150   0.169                poly3 (both n), rbf 1300 d 9, sigmoid 1300 d 9: the map's bound alone
    streamed, K v               0.0097  0.0042  0.0024               n = 129 (at n = 1300 below 3e-4): the bound of an n-term sum
    rectangle walk                      0.25                         all four RBF builds alike: 1 ulp of the fp64 reference at a value next to 1/2
The fp32 figures are the rounding to fp32 itself (half an ulp of fp32 is the whole of 2^-24 |ref| just above a power of two).
Cancellation family (another bound, see above): linear 0.175, poly 0.142, rbf 0.140, sigmoid 0.079, laplacian 0.274 through the
rectangular entry (385 d 33; rbf and laplacian at 130 d 1); the packed fp64 panel at 385 d 33 has the ratios of the rectangular
entry there (rbf 0.110, laplacian 0.173).  On the host the fp64 oracle lies at 0.08 to 0.30 of the same bounds.
No comparison failed on the device: this module found no fault in csrc/bq_gram.hip."""
import numpy as np
import pytest

import gram_reference as gr
from conftest import set_hooks

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def amd():
    from optiml_amd import _lib
    from optiml_amd.device import get_context
    assert np.finfo(gr.LD).nmant >= 63
    _lib.load()
    get_context()


def _no_hooks(monkeypatch, **kw):
    hooks = dict(compact_panel=None, stream_unit=None)
    hooks.update(kw)
    set_hooks(monkeypatch, **hooks)


def _kernel(sp):
    from optiml_amd.ml.svm import kernels as kk
    name, gamma, coef0, degree = sp
    return {'linear': lambda: kk.LinearKernel(), 'poly': lambda: kk.PolyKernel(degree, gamma, coef0),
            'rbf': lambda: kk.GaussianKernel(gamma), 'sigmoid': lambda: kk.SigmoidKernel(gamma, coef0),
            'laplacian': lambda: kk.LaplacianKernel(gamma)}[name]()


def _rect(sp, A, B):
    """the rectangular entry: kernel(A) or kernel(A, B), m x t"""
    kern = _kernel(sp)
    return kern(A) if B is None else kern(A, B)


def _panel(sp, X, storage='f64', full_panel=False, stream=False):
    from optiml_amd.opti import KernelQuadratic
    return KernelQuadratic(X, np.zeros(len(X)), 'plain', _kernel(sp), storage='stream' if stream else storage, full_panel=full_panel)


def _flipped(X):
    """the rows in reverse order: the Gram matrix of the flipped rows is the Gram matrix flipped, K[::-1, ::-1] — a second build of
    one case that stores 8-byte values too (the full panel after the packed one, the packed one after the rectangular entry)
    runs on the flipped rows, so no address can hold its right value from the first"""
    return np.ascontiguousarray(X[::-1])


def _resident(label, c, sp, X, ref, storage='f64', full_panel=False, esz=None, flip=False):
    """build the resident panel, assert its size, download it and hold every entry to the reference"""
    quad = _panel(sp, _flipped(X) if flip else X, storage, full_panel)
    try:
        lay = quad.device_problem().layout()
        assert lay['packed'] is (not full_panel) and not lay['streamed'], label
        if esz is not None:
            assert lay['panel_bytes'] == gr.panel_elems(len(X)) * esz, label
        K = quad.gram()
    finally:
        quad.release()
    if flip:
        K = K[::-1, ::-1]
    return K, gr.check_exact(label, c.name, K, ref, f32=storage == 'f32')


# ---- 1. the rectangular entry --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('c', gr.RECT_CASES, ids=gr.case_id)
def test_rectangular_entry(amd, monkeypatch, c):
    _no_hooks(monkeypatch)
    sp, A, B, ref = gr.exact_reference(c)
    K = _rect(sp, A, B)
    gr.check_exact(gr.case_id(c), c.name, K, ref)
    if B is None and c.name in ('rbf', 'laplacian'):
        assert (np.diag(K) == 1.0).all()


# ---- 2. the resident panel -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('c', gr.PANEL_CASES, ids=gr.case_id)
def test_resident_panel(amd, monkeypatch, c):
    sp, X, _, ref = gr.exact_reference(c)
    cid = gr.case_id(c)
    _no_hooks(monkeypatch)
    if c.name == 'rbf':   # eligible for the 7-byte layout by the choice of gamma; hook compact_panel=0 keeps 8 bytes
        compact, _ = _resident(cid + ' compact', c, sp, X, ref, esz=7)
        _no_hooks(monkeypatch, compact_panel=0)
        plain, _ = _resident(cid + ' packed f64', c, sp, X, ref, esz=8)
        _no_hooks(monkeypatch)
        assert np.array_equal(compact, plain)
        assert (np.diag(plain) == 1.0).all()
    else:
        K, _ = _resident(cid + ' packed f64', c, sp, X, ref, esz=8)
        if c.name == 'laplacian':
            assert (np.diag(K) == 1.0).all()
    _resident(cid + ' packed f32', c, sp, X, ref, storage='f32', esz=4)
    _resident(cid + ' full panel', c, sp, X, ref, full_panel=True, flip=True)


# ---- 3. cancellation -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('c', gr.CANCEL_CASES, ids=gr.case_id)
def test_cancellation(amd, monkeypatch, c):
    _no_hooks(monkeypatch)
    sp, A, B, ref, bound = gr.cancel_reference(c)
    cid = gr.case_id(c)
    got = [('rect', _rect(sp, A, B))]
    if (c.m, c.t, c.d) == (385, None, 33):   # ... and through the packed fp64 panel (not eligible for the 7-byte layout: |x|^2 ~ 400 d)
        quad = _panel(sp, _flipped(A))
        try:
            assert quad.device_problem().layout()['panel_bytes'] == gr.panel_elems(c.m) * 8
            got.append(('packed f64', quad.gram()[::-1, ::-1]))
        finally:
            quad.release()
    rows, cols = gr.near_duplicates(c)
    for entry, K in got:
        gr.within('%s %s' % (cid, entry), c.name, K, ref, bound)
        if c.name in ('rbf', 'laplacian'):
            assert (K <= 1.0).all() and (K[rows, cols] <= 1.0).all(), entry   # the clamp
            assert float(K[rows, cols].min()) > 1.0 - 1e-5, entry
            if B is None:
                assert (np.diag(K) == 1.0).all(), entry


# ---- 4. the XCD-rectangle walk -------------------------------------------------------------------------------------------------------
def test_which_shapes_take_the_rectangle_walk():
    """the arithmetic of run_gram (tiles_m * strips >= 8 * 16 * 4), on the host"""
    assert gr.walk_geometry(8200, 8200) == dict(tiles_m=65, strips=9, walk=True, rect_rb=5, rect_sb=3, rects=16)
    assert gr.walk_geometry(65700, 130) == dict(tiles_m=514, strips=1, walk=True, rect_rb=33, rect_sb=1, rects=40)
    g = gr.walk_geometry(32900, 1100)
    assert g['walk'] and (g['tiles_m'], g['strips']) == (258, 2)
    assert not gr.walk_geometry(8000, 8000)['walk']
    assert all(gr.walk_geometry(c.m, c.m if c.t is None else c.t)['walk'] for c in gr.WALK_CASES)


WALK_PANEL = [c for c in gr.WALK_CASES if c.group == 'walkpanel']
WALK_RECT = [c for c in gr.WALK_CASES if c.group == 'walkrect']


@pytest.mark.parametrize('c,layout', [(c, layout) for c in WALK_PANEL for layout in (('compact', 'plain') if c.name == 'rbf' else ('plain',))],
                         ids=lambda v: gr.case_id(v) if isinstance(v, gr.Case) else v)
def test_rectangle_walk_packed_panel(amd, monkeypatch, c, layout):
    """n = 8200: 65 tile rows x 9 strips, lower_only; the RBF panel in the 7-byte layout (eligible by the choice of gamma) and in 8 bytes"""
    sp, X, _, ref = gr.exact_reference(c, False)
    _no_hooks(monkeypatch, compact_panel=None if layout == 'compact' else 0)
    K, _ = _resident('%s %s' % (gr.case_id(c), layout), c, sp, X, ref, esz=7 if layout == 'compact' else 8)
    if c.name == 'rbf':
        assert (np.diag(K) == 1.0).all()


@pytest.mark.parametrize('c', WALK_RECT, ids=gr.case_id)
def test_rectangle_walk_rectangular(amd, monkeypatch, c):
    """514 tile rows x 1 strip and 258 x 2"""
    _no_hooks(monkeypatch)
    sp, A, B, ref = gr.exact_reference(c, False)
    gr.check_exact(gr.case_id(c), c.name, _rect(sp, A, B), ref)


# ---- 5. the streamed product ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('unit', [None, 3])
@pytest.mark.parametrize('c', gr.STREAM_CASES, ids=gr.case_id)
def test_streamed_product(amd, monkeypatch, c, unit):
    """K v against (long-double K) v under the bound of an n-term sum; and K e_j for every j: one term K_ij * 1 and n - 1 terms
    K_ik * 0 — products with zero and sums of zeros are exact, so the streamed product returns column j as its epilogue formed it,
    through the row sums (tile rows below j's) and the column sums (tile rows above), and the columns together are every entry of
    K under the bound of the map alone."""
    sp, X, _, ref = gr.exact_reference(c)
    v = gr.dyadic_vector(c)
    want, S = gr.product_reference(ref, v)
    _no_hooks(monkeypatch, stream_unit=unit)
    quad = _panel(sp, X, stream=True)
    try:
        dev = quad.device_problem()
        assert dev.layout()['streamed']
        outs = [('matvec', dev.matvec(v)), ('gram_matvec', dev.gram_matvec(v))]
        K, e = np.empty((c.m, c.m)), np.zeros(c.m)
        for j in range(c.m):
            e[j] = 1.0
            K[:, j] = dev.gram_matvec(e)
            e[j] = 0.0
    finally:
        quad.release()
    for entry, out in outs:
        label = '%s unit=%s %s' % (gr.case_id(c), unit, entry)
        if c.name == 'linear':
            gr.same_bits(label, out, want)
        else:
            gr.within(label, c.name, out, want, gr.product_bound(c.name, c.m, want, S))
    gr.check_exact('%s unit=%s one-hot columns' % (gr.case_id(c), unit), c.name, K, ref)
    if c.name == 'rbf':
        assert (np.diag(K) == 1.0).all()


def test_the_streamed_mode_refuses_the_laplacian_kernel(amd, monkeypatch):
    from optiml_amd import _lib
    _no_hooks(monkeypatch)
    c = next(c for c in gr.PANEL_CASES if c.name == 'laplacian' and c.m == 129)
    quad = _panel(gr.spec(c), gr.operands(c)[0], stream=True)
    with pytest.raises(_lib.BcqpError):
        quad.device_problem()
