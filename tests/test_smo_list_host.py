"""Host side of the support-list edge tests (no GPU): the list model of tests/smo_list_reference.py against a brute-force rebuild, and
the condition that keeps tests/test_gpu_smo_list_edges.py honest — within the outer iterations that test runs, the oracle's support list
meets every edge of the walker's (csrc/bq_smo.hip: shifts of more than SMO_T entries, entries moving across position SMO_CAP, error sums
over more than SMO_CAP entries) on every problem the GPU test uses, here on NumPy's Gram matrix."""
import numpy as np
import pytest

import smo_list_reference as lr

MAX_OUTER = 6


def _brute(before, after, idx):
    """what one edit of sample idx did, from the two lists alone: (kind, position of idx, entries that changed position, an entry went
    SMO_CAP - 1 -> SMO_CAP, an entry went SMO_CAP -> SMO_CAP - 1)"""
    was, now = np.flatnonzero(before), np.flatnonzero(after)
    pos = int(np.searchsorted(was, idx))
    kind = {(False, False): 'none', (True, True): 'update', (False, True): 'insert', (True, False): 'erase'}[
        bool(before[idx]), bool(after[idx])]
    where_was = np.full(len(before), -1)
    where_was[was] = np.arange(len(was))
    where_now = np.full(len(before), -1)
    where_now[now] = np.arange(len(now))
    both = before & after
    moved = both & (where_was != where_now)
    right = bool(np.any(moved & (where_was == lr.SMO_CAP - 1) & (where_now == lr.SMO_CAP)))
    left = bool(np.any(moved & (where_was == lr.SMO_CAP) & (where_now == lr.SMO_CAP - 1)))
    return kind, pos, int(moved.sum()), right, left


def test_list_model_equals_a_brute_force_rebuild():
    n = 5200
    rs = np.random.RandomState(5)
    model = lr.SupportListModel(n)
    start = np.sort(rs.choice(n, lr.SMO_CAP + 3, replace=False))
    for j in start:   # appends and inserts up to just past the mirror
        model.apply(int(j), True)
    assert model.nnz == lr.SMO_CAP + 3 and np.array_equal(np.flatnonzero(model.member), start)

    def sample_at(q):
        return int(np.flatnonzero(model.member)[q])

    def gap_before(q):
        """a non-member whose insert position is q, if the samples leave room"""
        nz = np.flatnonzero(model.member)
        lo = -1 if q == 0 else int(nz[q - 1])
        hi = n if q >= len(nz) else int(nz[q])
        return lo + 1 if hi - lo > 1 else None

    seen = set()
    kinds = []

    def edit(idx, member):
        before = model.member.copy()
        nnz = model.nnz
        e = model.apply(idx, member)
        kind, pos, moved, right, left = _brute(before, model.member, idx)
        assert (e.kind, e.pos, e.shifted) == (kind, pos, moved), (idx, member, e)
        assert e.crossing == (right or left) and not (right and kind != 'insert') and not (left and kind != 'erase'), e
        assert e.trips == -(-moved // lr.SMO_T)
        assert model.nnz == nnz + {'insert': 1, 'erase': -1}.get(kind, 0) == np.count_nonzero(model.member)
        seen.add((kind, pos))
        kinds.append(kind)
        return e

    # the named positions: 0, the end, SMO_CAP - 1 and SMO_CAP, erased and inserted again
    for q in (0, lr.SMO_CAP - 1, lr.SMO_CAP, model.nnz - 1):
        j = sample_at(q)
        assert edit(j, True).kind == 'update'
        assert edit(j, False).kind == 'erase'
        assert edit(j, False).kind == 'none'
        e = edit(j, True)
        assert e.kind == 'insert' and e.pos == q
    for q in (0, lr.SMO_CAP - 1, lr.SMO_CAP, lr.SMO_CAP + 1):
        j = gap_before(q)
        if j is not None:
            assert edit(j, True).pos == q
            edit(j, False)
    free = np.flatnonzero(~model.member)
    e = edit(int(free[-1]) if free[-1] > sample_at(model.nnz - 1) else n - 1, True)   # an append, or an update of the last sample
    assert e.shifted == 0
    # a list of exactly SMO_CAP entries: an insert at its end moves nothing, one before it crosses
    while model.nnz > lr.SMO_CAP:
        edit(sample_at(model.nnz - 1), False)
    j = sample_at(lr.SMO_CAP - 1)
    edit(j, False)
    assert model.nnz == lr.SMO_CAP - 1
    assert not edit(j, True).crossing                   # fills position SMO_CAP - 1: nothing behind it
    j0 = sample_at(0)
    assert not edit(j0, False).crossing                 # SMO_CAP entries: the last one moves to SMO_CAP - 2
    e = edit(j0, True)
    assert e.shifted == lr.SMO_CAP - 1 and e.trips == 4 and not e.crossing
    g = gap_before(1)
    if g is None:
        g = int(np.flatnonzero(~model.member)[0])
    e = edit(g, True)                                   # SMO_CAP entries before: the last one goes to position SMO_CAP
    assert e.crossing and e.kind == 'insert'
    e = edit(g, False)
    assert e.crossing and e.kind == 'erase'
    # random edits around the mirror's edge
    for _ in range(400):
        j = int(rs.randint(n))
        r = rs.uniform()
        edit(j, bool(model.member[j]) if r < 0.2 else (not model.member[j] if r < 0.9 else bool(rs.randint(2))))
    assert {'none', 'update', 'insert', 'erase'} <= set(kinds)
    assert ('insert', 0) in seen and ('erase', 0) in seen
    assert ('insert', lr.SMO_CAP - 1) in seen and ('erase', lr.SMO_CAP) in seen


def test_pair_step_counts_the_sum_before_the_edits():
    model = lr.SupportListModel(lr.SMO_CAP + 10)
    for j in range(lr.SMO_CAP):
        model.apply(j, True)
    model.pair_step(lr.SMO_CAP, lr.SMO_CAP + 1, True, True, True)    # summed over SMO_CAP entries: not past the mirror
    assert model.counts['long_dots'] == 0 and model.nnz == lr.SMO_CAP + 2
    model.pair_step(0, lr.SMO_CAP + 2, False, True, False)           # a cached error: no sum
    assert model.counts['long_dots'] == 0
    model.pair_step(1, 2, False, False, True)
    assert model.counts['long_dots'] == 1
    assert model.counts == dict(long_inserts=0, long_erases=3, crossing_inserts=0, crossing_erases=3, long_dots=1)
    assert model.largest == lr.SMO_CAP + 2


def _problems():
    X, y, par = lr.svc_draw()
    yield 'svc', 'svc', X, y, par
    X, y, par = lr.svr_draw()
    yield 'svr', 'svr', X, y, par
    X, Y, rows, par = lr.row_list_draw()
    yield 'row list', 'svc', X, Y[1], dict(par, rows=rows[1])


@pytest.mark.parametrize('name,gamma_of', [('svc', lr.rbf_gamma), ('svc', lr.compact_gamma), ('svr', lr.rbf_gamma),
                                           ('svr', lr.compact_gamma), ('row list', lr.rbf_gamma)],
                         ids=['svc-scale', 'svc-compact', 'svr-scale', 'svr-compact', 'row_list-scale'])
def test_every_event_class_occurs_within_the_run(name, gamma_of):
    """both draws at the gamma of gamma='scale' and at the one the compact-panel cases use, and the row-list column"""
    (_, kind, X, y, par), = [p for p in _problems() if p[0] == name]
    par = dict(par)
    rows = par.pop('rows', None)
    K = lr.rbf_gram(X, gamma_of(X))
    if rows is not None:
        K, y = K[rows][:, rows], y[rows]
    run = lr.run_oracle(kind, K, y, MAX_OUTER, **par)
    print(name, gamma_of.__name__, run['counts'], 'largest list', run['largest'], 'steps', run['snap'].steps)
    assert not lr.missing_events(run['counts']), run['counts']
    assert run['largest'] > lr.SMO_CAP and len(run['snap'].rows) == MAX_OUTER and not run['ref']['finished']
    # the edges lie in the second full sweep (outer iteration 3): a run cut before it would not do
    assert lr.missing_events(run['snap'].events[1]) and not lr.missing_events(run['snap'].events[3])
