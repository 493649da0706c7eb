"""The draws and references of the batched solvers' differential run (tests/batched_fuzz_reference.py), held to their own
preconditions without a device: a draw is a function of its seed, every draw is a valid problem, the named leaver draws have a
column that the reference stops before the cap while another runs to it, and the reference alone decides status and iteration
count of at least 95 % of the checked columns of every family (a column on which one ulp of K moves either is compared on its f
history only, so a seed list with many of them would test little).

Measured on the seed lists as they stand (18 draws per family, the oracle's Gram matrix, fp32 draws on K rounded to fp32), checked
columns that are not unanimous: labels4 0 of 49, boxes16 0 of 43, svr 0 of 44, svr_boxes 0 of 38, pairs 0 of 39, sx_one 0 of 47,
sx_labels 0 of 44, sx_paired 0 of 40 (4 of 58 with nu = 0.0517 in its pool: batched_fuzz_reference.NUS_PAIRED), sx_blocks 0 of 38."""
import numpy as np
import pytest

import batched_fuzz_reference as bf

CAP = 0.05   # the share of a family's checked columns that may be non-unanimous: a condition on the seed lists, not a measurement


def _host_panel(dr):
    """the oracle's Gram matrix, rounded to fp32 where the draw stores the panel in fp32"""
    K = bf.oracle_gram(dr)
    return K.astype(np.float32).astype(float) if dr.storage == 'f32' else K


@pytest.fixture(scope='module')
def surveyed():
    """(family, seed) -> the checked columns' sensitivities, computed once for the tests below"""
    out = {}
    for family in bf.FAMILIES:
        for seed in bf.seeds(family):
            dr = bf.draw(family, seed)
            out[family, seed] = bf.sensitivities(dr, dr.checked, _host_panel(dr))
    return out


def _same(a, b):
    if isinstance(a, np.ndarray):
        return isinstance(b, np.ndarray) and a.dtype == b.dtype and np.array_equal(a, b)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return a == b


@pytest.mark.parametrize('family', bf.FAMILIES)
def test_draw_is_deterministic(family):
    for seed in bf.seeds(family)[::5] + bf.BLOCKS[family][-1]:
        a, b = vars(bf.draw(family, seed)), vars(bf.draw.__wrapped__(family, seed))
        assert set(a) == set(b)
        for key, v in b.items():
            assert _same(a[key], v), (family, seed, key)


@pytest.mark.parametrize('family', bf.FAMILIES)
def test_every_draw_is_valid(family):
    """Feasible masses and start points, labels of both signs among the trained rows, ub >= 0, pairs inside the class list; the
    pools' edges are met: a strip draw of each n, and a draw with more columns than one product chunk."""
    seen_n = set()
    for seed in bf.seeds(family):
        dr = bf.draw(family, seed)
        assert bf.valid(dr) == [], (family, seed)
        assert 1 <= len(dr.checked) <= 4 and all(0 <= c < dr.k for c in dr.checked)
        if dr.strip:
            assert dr.k <= 5 and dr.max_iter == bf.STRIP_ITERS and dr.n >= 2049
            seen_n.add(dr.seed % 2)
    assert seen_n == {0, 1}
    assert any(bf.draw(family, s).k > bf.WIDTH.get(family, 16) for s in bf.seeds(family))
    assert set(bf.LEAVERS[family]) <= set(bf.seeds(family)) and len(bf.LEAVERS[family]) >= 1


@pytest.mark.parametrize('family', bf.FAMILIES)
def test_leaver_precondition(surveyed, family):
    """In every named draw the reference stops the leaver 'optimal' before the cap, and another checked column runs to the cap"""
    for seed in bf.LEAVERS[family]:
        dr = bf.draw(family, seed)
        sens = surveyed[family, seed]
        assert dr.leave and dr.leaver in dr.checked, (family, seed)
        lv = sens[dr.leaver]
        assert lv['base']['status'] == 'optimal' and lv['base']['iter'] < dr.max_iter and lv['unanimous'], (family, seed)
        others = [sens[c]['base'] for c in dr.checked if c != dr.leaver]
        assert any(o['status'] == 'stopped' and o['iter'] == dr.max_iter for o in others), (family, seed)


@pytest.mark.parametrize('family', bf.FAMILIES)
def test_the_reference_alone_decides_most_columns(surveyed, family):
    total = bad = 0
    for seed in bf.seeds(family):
        for c, s in surveyed[family, seed].items():
            total += 1
            bad += not s['unanimous']
            assert s['common'] >= 1 and np.isfinite(s['f_spread']) and np.isfinite(s['x_spread']), (family, seed, c)
    print('%s: %d of %d checked columns are not unanimous' % (family, bad, total))
    assert total >= 30 and bad <= CAP * total, (family, bad, total)
