"""The host side of test_gpu_gram_edges.py (no GPU): for every case of that module the generators' exactness assertions hold and
the fp64 oracle `so.gram` lies within the very bound the device is held to, against the same long-double reference — the bounds
leave a correct fp64 implementation room; and the comparison is sensitive: one reference entry moved by 16 u |ref|, or one
reference column rolled by one, fails it for every map.  (That is how the sensitivity of the device tests is shown: the kernels
are not broken to show it.)"""
import numpy as np
import pytest

import gram_reference as gr
from gram_reference import LD, U


def _oracle(sp, A, B):
    from oracle import svm_oracle as so
    name, gamma, coef0, degree = sp
    return so.gram(name, A, B, gamma=gamma if name != 'linear' else 1.0, coef0=coef0, degree=degree)


def test_long_double_is_wide_enough():
    assert np.finfo(LD).nmant >= 63


@pytest.mark.parametrize('c', gr.RECT_CASES + gr.PANEL_CASES + gr.STREAM_CASES + gr.WALK_CASES, ids=gr.case_id)
def test_exact_arguments_and_the_oracle_within_the_bound(c):
    wide = not c.group.startswith('walk')
    sp, A, B, ref = gr.exact_reference(c, wide)   # asserts the exactness of every argument and the 2^-1000 floor
    assert ref.shape == (c.m, c.m if c.t is None else c.t) and ref.dtype == (LD if wide else np.float64)
    K = _oracle(sp, A, B)
    ratio = gr.check_exact(gr.case_id(c), c.name, K, ref)
    assert ratio <= 1.0
    if c.name in ('rbf', 'laplacian'):
        assert float(ref.min()) >= 2.0 ** -1000 and float(ref.max()) <= 1.0
        if c.t is None:
            assert (np.diag(K) == 1.0).all() and (np.diag(ref) == 1).all()
    if c.name == 'rbf' and c.group in ('panel', 'walkpanel'):
        assert float(ref.min()) >= 2.0 ** -14   # the range of the 7-byte layout
    if c.group == 'stream':
        v = gr.dyadic_vector(c)
        want, S = gr.product_reference(ref, v)
        if c.name == 'linear':
            gr.same_bits(gr.case_id(c) + ' K v', K @ v, want)
        else:
            gr.within(gr.case_id(c) + ' K v', c.name, K @ v, want, gr.product_bound(c.name, c.m, want, S))


@pytest.mark.parametrize('c', gr.CANCEL_CASES, ids=gr.case_id)
def test_cancellation_bounds_hold_for_the_oracle(c):
    sp, A, B, ref, bound = gr.cancel_reference(c)
    K = _oracle(sp, A, B)
    ratio = gr.within(gr.case_id(c), c.name, K, ref, bound)
    assert 0.0 < ratio <= 1.0   # the bound is met and is not vacuous
    rows, cols = gr.near_duplicates(c)
    assert len(rows) >= 18
    if c.name in ('rbf', 'laplacian'):
        assert (K <= 1.0).all() and (K[rows, cols] <= 1.0).all()
        assert float(ref[rows, cols].min()) > 1.0 - 1e-5   # near-duplicates: the true value is next to 1
        if c.t is None:
            assert (np.diag(K) == 1.0).all()
    if c.name == 'rbf':
        # the distance does cancel: formed as the device forms it, it comes out below zero somewhere, so the clamp is live
        Bv = A if B is None else B
        dist = (-2.0 * (A @ Bv.T) + (A * A).sum(axis=1)[:, None]) + (Bv * Bv).sum(axis=1)[None, :]
        print('%s: %d of %d near-duplicate distances come out negative' % (gr.case_id(c), (dist[rows, cols] < 0).sum(), len(rows)))
        assert (dist[rows, cols] < 0).any()


def _one_case_per_map():
    out = []
    for name in gr.MAPS:
        out.append(next(c for c in gr.RECT_CASES if c.name == name and c.t is not None and c.m > 1))
    return out


@pytest.mark.parametrize('c', _one_case_per_map(), ids=gr.case_id)
def test_the_comparison_sees_one_wrong_entry_and_one_shifted_column(c):
    sp, A, B, ref = gr.exact_reference(c)
    K = _oracle(sp, A, B)
    gr.check_exact('as it is', c.name, K, ref)
    i, j = np.unravel_index(np.argmax(np.abs(ref)), ref.shape)
    assert ref[i, j] != 0
    moved = ref.copy()
    moved[i, j] += 16 * U * np.abs(ref[i, j]) if c.name != 'linear' else 1
    with pytest.raises(AssertionError, match='entry'):
        gr.check_exact('one entry moved', c.name, K, moved)
    if c.name != 'linear':   # ... in fp32 storage the same entry moved by 4 x 2^-24 |ref|
        K32 = K.astype(np.float32).astype(np.float64)
        gr.check_exact('fp32 as it is', c.name, K32, ref, f32=True)
        moved[i, j] = ref[i, j] + 4 * gr.F32 * np.abs(ref[i, j])
        with pytest.raises(AssertionError, match='entry'):
            gr.check_exact('fp32, one entry moved', c.name, K32, moved, f32=True)
    rolled = ref.copy()
    rolled[:, j] = np.roll(ref[:, j], 1)
    assert (rolled[:, j] != ref[:, j]).any()
    with pytest.raises(AssertionError, match='entry'):
        gr.check_exact('one column rolled', c.name, K, rolled)


def test_the_product_comparison_sees_one_wrong_entry():
    c = next(c for c in gr.STREAM_CASES if c.name == 'rbf' and c.m == 129)
    sp, A, B, ref = gr.exact_reference(c)
    v = gr.dyadic_vector(c)
    want, S = gr.product_reference(ref, v)
    out = _oracle(sp, A, B) @ v
    bound = gr.product_bound(c.name, c.m, want, S)
    gr.within('as it is', c.name, out, want, bound)
    off = out.copy()
    off[77] += 2.0 * float(bound[77]) + 1e-300
    with pytest.raises(AssertionError, match='entry'):
        gr.within('one entry moved', c.name, off, want, bound)


def test_which_shapes_take_the_rectangle_walk():
    """the arithmetic of run_gram: tiles_m * strips >= 8 * 16 * 4"""
    g = gr.walk_geometry(8200, 8200)
    assert g == dict(tiles_m=65, strips=9, walk=True, rect_rb=5, rect_sb=3, rects=16)
    g = gr.walk_geometry(65700, 130)
    assert g == dict(tiles_m=514, strips=1, walk=True, rect_rb=33, rect_sb=1, rects=40)
    g = gr.walk_geometry(32900, 1100)
    assert g['walk'] and (g['tiles_m'], g['strips'], g['rect_rb'], g['rect_sb']) == (258, 2, 17, 1)
    assert not gr.walk_geometry(8000, 8000)['walk'] and not gr.walk_geometry(8064, 8064)['walk']
    assert gr.walk_geometry(8065, 8065)['walk']   # the smallest symmetric build that takes it
    for c in gr.WALK_CASES:
        assert gr.walk_geometry(c.m, c.m if c.t is None else c.t)['walk']
    for c in gr.RECT_CASES + gr.PANEL_CASES + gr.CANCEL_CASES:
        assert not gr.walk_geometry(c.m, c.m if c.t is None else c.t)['walk']


def test_the_case_table_covers_what_it_is_meant_to():
    for name in gr.MAPS:
        mine = [c for c in gr.RECT_CASES if c.name == name]
        assert {c.d for c in mine if c.t is None} == set(gr.DS) == {c.d for c in mine if c.t is not None}
        assert {c.m for c in mine if c.t is None} == set(gr.SQUARES)
        assert {(c.m, c.t) for c in mine if c.t is not None} == set(gr.RECTS)
    assert {c.degree for c in gr.RECT_CASES if c.name == 'poly'} == {2, 3, 5}
    assert {(c.name, c.m) for c in gr.PANEL_CASES} == {(name, n) for name in gr.MAPS for n in (129, 257, 385, 2049)}
    gammas = [gr.spec(c)[1] for c in gr.RECT_CASES if c.name != 'linear']
    assert len(set(gammas)) >= 8   # the cases do not share one gamma
