"""Cross-validated grid search over `OneVsOneSVC`: the result of sklearn's `GridSearchCV(OneVsOneSVC(**kw), param_grid, cv=cv,
refit=refit)` with accuracy scoring — the search `GridSearchCV(sklearn.svm.SVC, {'C': ...})` runs on multi-class data, whose SVC is
one-vs-one — with every (candidate, fold, pair) a column on ONE class-sorted Gram panel per resolved kernel.

`OneVsOneSVC`'s panel carries over (onevsone.py: rows sorted by class, every class padded by ghost rows to whole tiles, one column
per pair), and so do the searches' two facts (model_selection.py): a training fold's dual is the full dual with a zero box on the
held-out rows, and C is only the box.  Column (candidate, fold, pair (a, b)) has ub = C on the data rows of a and b in the fold's
training part and 0 everywhere else; the columns run on the pair-routed solver (`bq_msolver_create_pairs`), which streams the panel at
most once per iteration for all live columns.

Scoring a (candidate, fold) needs every pair's decision value at every held-out row of every class — the routed product writes exact
zeros outside a pair's two classes — and `OneVsOneClassifier`'s vote.  Both happen where the solver's state lives
(`bq_msolver_pairs_vote_heldout`): the coefficients and intercepts of all columns, one 16-column product of them on all rows, the vote
of every held-out row (`ovo_decision` and argmax, statement for statement: `ovo_vote` is the same kernel on host arrays) and the
count of the rows whose vote is their class.  Per column an intercept and a support count come back and per (candidate, fold) two
integers: no columns x n array crosses the bus.

The batched path applies when `uses_batched_ovo_search` holds: `OneVsOneSVC`'s own batched configuration for every candidate, an fp64
panel (an fp32 panel does not hold `decision_function`'s values), a grid over C and kernel only, 2 to 64 classes, and every class in
every fold's training rows (else the fold's own `OneVsOneSVC` has other `classes_`).  If the columns of one (candidate, fold) do not
fit the device memory budget of a solve, that is decided before any solve.  Every other configuration runs exactly the calls
`SVCGridSearchCV` makes for a `OneVsOneSVC`: `fit` on the fold's training rows and `score` on its held-out rows, per candidate and
fold.

A (candidate, fold) with a pair that ends without a support vector is a failed fit (`SVC.fit`'s intercept divides by zero;
GridSearchCV's error_score): it scores NaN, has `n_iter_` -1 and `status_` 'failed', and one RuntimeWarning names the number of such
fits; if every fit fails the search raises ValueError, as GridSearchCV does.

With `optimizer='smo'` (`uses_batched_ovo_smo_search`, the same conditions over `uses_batched_ovo_smo`) every (candidate, fold, pair)
is one walker column of the batched SMO solver (`bq_msmo_*`) on ONE unsorted panel of all n rows per resolved kernel: its row list
is the fold's training rows of the pair's two classes, ascending — the sweep order of the fold's own per-pair fit — and no box is
needed.  The columns run to their end in whole (candidate, fold) groups (`smo_groups_per_solve`) and are scored where the walkers'
state lives (`bq_msmo_vote_heldout`): the coefficients from the multipliers, the solver's own intercepts, one 16-column product on
all rows, the same vote with a row's class read from its code; `n_iter_` holds the columns' outer iterations and `status_` is '',
as an SMO fit records none; a group with a failed walker scores NaN as above.  `smo_` says that this path ran; `batch_smo` (None,
True, False) forces the choice where the configuration allows it, None going by the number of columns (`takes_batched_smo`).  A
column follows the fold's per-pair `SVC.fit` step for step on the shared panel's entries; that fit builds its own Gram matrix on
the pair's rows (see onevsone.py for how the two compare), so against the per-fold path the split scores agree where no held-out
decision of a pair lies within 12 tol of zero.
"""
import numpy as np

from ... import _lib
from ...device import get_context
from ._base import has_class_weight
from ._batched import (MAX_COLUMNS, MEMORY_SHARE, _DeviceSMOSolver, column_bytes, device_panel, run_batched_smo, smo_column_bytes,
                       solve_batched, solver_kind, takes_batched_smo)
from .coupling import MAX_CLASSES
from .model_selection import BATCHED_KEYS, _base_params, _GridSearchCV, _kernel_key, _make
from .onevsone import (TILE, OneVsOneSVC, _DevicePairSolver, ovo_pairs, pair_problem, pairs_slab_bytes, sort_plan, uses_batched_ovo,
                       uses_batched_ovo_smo)

__all__ = ['OneVsOneGridSearchCV', 'ovo_vote', 'uses_batched_ovo_search', 'plan_ovo_columns', 'groups_per_solve',
           'uses_batched_ovo_smo_search', 'takes_batched_ovo_smo_search', 'plan_ovo_smo_columns', 'smo_groups_per_solve']


def ovo_vote(D, ncls, details=False):
    """The predicted class codes of t rows from their pair decision values D (t x P, `ovo_pairs` order, positive towards the larger
    class), by the vote kernel (`bq_ovo_vote`): `ovo_decision((D > 0).astype(int), D, ncls).argmax(axis=1)`, the first NaN of a row
    winning as np.argmax has it.  details: (pred, Y) instead, Y being the t x ncls decision matrix with `ovo_decision`'s bits."""
    ncls = int(ncls)
    P = ncls * (ncls - 1) // 2
    D = np.ascontiguousarray(D, dtype=float)
    if D.ndim == 1 and P == 1:
        D = D.reshape(-1, 1)
    if D.ndim != 2 or (P > 0 and D.shape[1] != P):
        raise ValueError('D must be t x %d (one column per pair of %d classes), got shape %s' % (P, ncls, D.shape))
    t = len(D)
    pred = np.empty(t, dtype=np.int32)
    Y = np.empty((t, ncls)) if details else None
    _lib.check(_lib.load().bq_ovo_vote(get_context().handle, ncls, t, _lib.ptr(D), _lib.iptr(pred), _lib.ptr(Y)))
    return (pred, Y) if details else pred


def uses_batched_ovo_search(estimator, candidates, splits, y, world, path=uses_batched_ovo):
    """True when `OneVsOneGridSearchCV` solves every (candidate, fold, pair) on shared class-sorted panels and scores on the device:
    the estimator is an `OneVsOneSVC` whose every candidate is on its batched path (`path`: `uses_batched_ovo`), the panel is 'f64',
    the grid varies only C and kernel with no string gamma other than 'auto', y holds 2 to 64 classes, and every fold's training
    rows hold every one of them."""
    if not isinstance(estimator, OneVsOneSVC):
        return False
    if any(not set(p) <= BATCHED_KEYS for p in candidates):
        return False
    base = _base_params(estimator)
    for p in candidates:
        proto = _make(OneVsOneSVC, base, p)._prototype()
        if has_class_weight(proto) or not path(proto, world) or proto.storage != 'f64':   # the search's columns carry one C each
            return False
        if isinstance(getattr(proto.kernel, 'gamma', None), str) and proto.kernel.gamma != 'auto':
            return False
    y = np.asarray(y)
    classes = np.unique(y)
    if not 2 <= len(classes) <= MAX_CLASSES:
        return False
    return all(np.array_equal(np.unique(y[tr]), classes) for tr, _ in splits)


def _panel_key(kernel):
    """One panel per resolved kernel; gamma='auto' is 1 / d on any rows, which `_kernel_key`'s probe rows would not show"""
    if getattr(kernel, 'gamma', None) == 'auto':
        return (type(kernel).__name__, 'auto') + tuple(kernel.device_spec(np.zeros((1, 1))))[2:]
    return _kernel_key(kernel)


def plan_ovo_columns(codes, ncls, splits, candidates, base_C, base_kernel):
    """The batched search's panels and columns as plain arrays, for class codes 0..ncls-1 and (train, test) splits.  A dict of
    index, cls_tiles, n_pad (`sort_plan`); data_row (n_pad, 1 a data row, 0 a ghost row); pcode (the class of every panel row);
    pairs (`ovo_pairs`); and groups, one per resolved kernel with one panel each: dicts {kernel; fits: [(candidate, fold, C)], the
    (candidate, fold) groups of columns in candidate-major order; cols: [(fit number, pair number)], group-major, the pairs in
    `ovo_pairs` order; Y, UB (columns x n_pad): the labels (+1 on the rows of the pair's larger class) and the boxes — C on the
    pair's data rows in the fold's training part, 0 on the fold's held-out rows, on ghost rows and on the rows of every other class;
    held (fits x n_pad, uint8): 1 on the fold's test rows at their panel positions}."""
    codes = np.asarray(codes)
    index, cls_tiles, n_pad = sort_plan(codes, ncls)
    data_row = np.zeros(n_pad, dtype=np.uint8)
    data_row[index] = 1
    pcode = np.repeat(np.arange(ncls), np.diff(cls_tiles) * TILE)
    pairs = ovo_pairs(ncls)
    train, test = [], []
    for tr, te in splits:
        for rows, masks in ((tr, train), (te, test)):
            mask = np.zeros(n_pad, dtype=bool)
            mask[index[rows]] = True
            masks.append(mask)
    inpair = [((pcode == i) | (pcode == j)) & (data_row > 0) for i, j in pairs]
    labels = [np.where(pcode == j, 1., -1.) for _, j in pairs]
    groups, where = [], {}
    for ci, p in enumerate(candidates):
        Cv, kernel = p.get('C', base_C), p.get('kernel', base_kernel)
        key = _panel_key(kernel)
        if key not in where:
            where[key] = len(groups)
            groups.append(dict(kernel=kernel, fits=[], cols=[], Y=[], UB=[], held=[]))
        g = groups[where[key]]
        for f in range(len(splits)):
            fit = len(g['fits'])
            g['fits'].append((ci, f, Cv))
            g['held'].append(test[f].astype(np.uint8))
            for q in range(len(pairs)):
                g['cols'].append((fit, q))
                g['Y'].append(labels[q])
                g['UB'].append(np.where(inpair[q] & train[f], float(Cv), 0.))
    for g in groups:
        for name in ('Y', 'UB', 'held'):
            g[name] = np.stack(g[name])
    return dict(index=index, cls_tiles=cls_tiles, n_pad=n_pad, data_row=data_row, pcode=pcode, pairs=pairs, groups=groups)


def groups_per_solve(pairs, cls_tiles, n_pad, free_bytes, wide_slab_bytes):
    """(candidate, fold) groups one batched solve may take with `free_bytes` of device memory free after the panel, 0 when not even
    one fits.  `pair_chunks`' budget — MEMORY_SHARE of it; per column `column_bytes` and its pair's slab region — must also hold the
    scoring's scratch: the 16-column product's slab (`wide_slab_bytes`) and its input and output, two n-vectors per column rounded
    up to 16 columns (`bq_msolver_pairs_vote_heldout`).  At most MAX_COLUMNS columns.  The split does not change any group's bits."""
    P = len(pairs)
    vec = 8 * (n_pad + 256)
    per_group = sum(column_bytes(n_pad) + pairs_slab_bytes(cls_tiles, [p]) for p in pairs) + 2 * P * vec
    budget = int(free_bytes * MEMORY_SHARE) - int(wide_slab_bytes) - 2 * 15 * vec   # (the last chunk's padding columns)
    return int(max(0, min(MAX_COLUMNS // P, budget // per_group)))


def uses_batched_ovo_smo_search(estimator, candidates, splits, y, world):
    """True when `OneVsOneGridSearchCV` can solve every (candidate, fold, pair) as one batched-SMO column on shared unsorted panels
    and score on the device (`bq_msmo_vote_heldout`): `uses_batched_ovo_search`'s conditions with `uses_batched_ovo_smo` as the
    estimator's path — an 'f64' panel, a grid over C and kernel only, no string gamma but 'auto', 2 to 64 classes, every class in
    every fold's training rows."""
    return uses_batched_ovo_search(estimator, candidates, splits, y, world, path=uses_batched_ovo_smo)


def takes_batched_ovo_smo_search(estimator, candidates, splits, y, world, force=None):
    """The search's dispatch: the configuration allows pair columns (`uses_batched_ovo_smo_search`) and `takes_batched_smo` takes
    its candidates x folds x pairs columns — `force` (`OneVsOneGridSearchCV.batch_smo`: True / False) where given."""
    if not uses_batched_ovo_smo_search(estimator, candidates, splits, y, world):
        return False
    ncls = len(np.unique(y))
    return takes_batched_smo(len(candidates) * len(splits) * (ncls * (ncls - 1) // 2), force)


def plan_ovo_smo_columns(codes, ncls, splits, candidates, base_C, base_kernel):
    """The batched SMO search's panels and columns as plain arrays, for class codes 0..ncls-1 and (train, test) splits: a list of
    groups, one per resolved kernel (`_panel_key`) with one unsorted panel of all n rows each — dicts {kernel; fits: [(candidate,
    fold, C)], the (candidate, fold) groups of columns in candidate-major order; cols: [(fit number, pair number)], group-major,
    the pairs in `ovo_pairs` order; Y (columns x n): +1 on the rows of the pair's larger class, -1 elsewhere; rows: per column the
    fold's training rows of the pair's two classes, ascending — the sweep order of the fold's own per-pair fit; C (columns); held
    (fits x n, uint8): 1 on the fold's test rows}.  None when a fold repeats a training row or tests on one: that is another
    problem than a row list's, and the search runs the per-fold calls."""
    codes = np.asarray(codes)
    n = len(codes)
    pairs = ovo_pairs(ncls)
    labels = [np.where(codes == j, 1., -1.) for _, j in pairs]
    rows, held = [], []
    for tr, te in splits:
        train = np.zeros(n, dtype=bool)
        train[tr] = True
        if int(train.sum()) != len(tr) or train[te].any():
            return None
        rows.append([pair_problem(np.where(train, codes, -1), i, j)[0] for i, j in pairs])
        mask = np.zeros(n, dtype=np.uint8)
        mask[te] = 1
        held.append(mask)
    groups, where = [], {}
    for ci, p in enumerate(candidates):
        Cv, kernel = p.get('C', base_C), p.get('kernel', base_kernel)
        key = _panel_key(kernel)
        if key not in where:
            where[key] = len(groups)
            groups.append(dict(kernel=kernel, fits=[], cols=[], Y=[], rows=[], C=[], held=[]))
        g = groups[where[key]]
        for f in range(len(splits)):
            fit = len(g['fits'])
            g['fits'].append((ci, f, Cv))
            g['held'].append(held[f])
            for q in range(len(pairs)):
                g['cols'].append((fit, q))
                g['Y'].append(labels[q])
                g['rows'].append(rows[f][q])
                g['C'].append(float(Cv))
    for g in groups:
        g['Y'], g['held'], g['C'] = np.stack(g['Y']), np.stack(g['held']), np.array(g['C'])
    return groups


def smo_groups_per_solve(P, n, free_bytes, wide_slab_bytes):
    """(candidate, fold) groups of P pair columns one batched SMO solve may take with `free_bytes` of device memory free after the
    panel of n rows, 0 when not even one fits.  The budget — MEMORY_SHARE of it — holds per group P walker columns
    (`smo_column_bytes`) and the scoring's scratch (`bq_msmo_vote_heldout`): its input and output, two n-vectors per column, and
    once the 16-column product's slab (`wide_slab_bytes`) and the two vectors of the last chunk's 15 padding columns.  At most
    MAX_COLUMNS columns.  The split does not change any group's bits."""
    vec = 8 * (n + 256)
    per_group = P * smo_column_bytes(n, _lib.SVC) + 2 * P * vec
    budget = int(free_bytes * MEMORY_SHARE) - int(wide_slab_bytes) - 2 * 15 * vec
    return int(max(0, min(MAX_COLUMNS // P, budget // per_group)))


class OneVsOneGridSearchCV(_GridSearchCV):
    """Exhaustive search over `param_grid` for an `OneVsOneSVC` scored by accuracy, as sklearn's GridSearchCV.  An int `cv` is
    StratifiedKFold(cv) without shuffling.

    After `fit`: `cv_results_` (params, param_<key>, split<i>_test_score, mean / std / rank_test_score — no timing keys: the
    candidates' fits are one batched solve and have no fit time of their own), `best_index_` (first among ties), `best_params_`,
    `best_score_`, `n_splits_`, `best_estimator_` (a plain `OneVsOneSVC.fit` on all the data, refit=True), `n_iter_` / `status_` of
    shape (candidates, splits, pairs) and `batched_`, which says which path ran.  On the batched path a (candidate, fold) with a pair
    that has no support vector scores NaN with `n_iter_` -1 and `status_` 'failed' under one RuntimeWarning for the search, and a
    search whose fits all fail raises ValueError.  `predict`, `decision_function` and `score` are the best estimator's.

    `smo_`: the batched path was the batched SMO solver's (`uses_batched_ovo_smo_search`: every (candidate, fold, pair) a row-list
    column on one unsorted panel, scored by `bq_msmo_vote_heldout`); `batch_smo` (None, True, False) forces that choice where the
    configuration allows it (None: by the number of columns, `takes_batched_smo`).
    """

    _estimator_type = OneVsOneSVC
    _type_error = 'estimator must be a OneVsOneSVC'
    _column_records = True
    _counts_failed = True
    batch_smo = None

    def _uses_batched(self, first, candidates, splits, y):
        world = get_context().world
        self.smo_ = takes_batched_ovo_smo_search(first, candidates, splits, y, world, self.batch_smo)
        return self.smo_ or uses_batched_ovo_search(first, candidates, splits, y, world)

    def _fit_batched_smo(self, X, y, splits, candidates, first):
        """Every (candidate, fold, pair) one batched-SMO column on the unsorted panel of its resolved kernel, run to the end and
        scored where the walkers' state lives; None — before any solve — when a fold's rows make no row list
        (`plan_ovo_smo_columns`) or the P columns of one (candidate, fold) do not fit the memory budget of a solve."""
        proto = first._prototype()
        classes = np.unique(y)
        codes = np.searchsorted(classes, y)
        ncls, n = len(classes), len(y)
        P = ncls * (ncls - 1) // 2
        nc, ns = len(candidates), len(splits)
        plan = plan_ovo_smo_columns(codes, ncls, splits, candidates, proto.C, proto.kernel)
        if plan is None:
            return None
        scores = np.full((nc, ns), np.nan)
        n_iter = np.full((nc, ns, P), -1, dtype=np.int64)
        status = np.full((nc, ns, P), 'failed', dtype=object)
        for gi, g in enumerate(plan):   # one panel at a time, built as SVC.fit's SMO branch builds it
            with device_panel(X, -np.ones(n), 'svc', g['kernel'], y=g['Y'][0], storage=proto.storage, rank_one=False,
                              compact=False) as (_, dev, free, slab):
                take = smo_groups_per_solve(P, n, free, slab)
                if take == 0 and gi == 0:
                    return None
                take = max(1, take)
                for f0 in range(0, len(g['fits']), take):
                    fits = g['fits'][f0:f0 + take]
                    cols = slice(f0 * P, (f0 + len(fits)) * P)
                    solver = _DeviceSMOSolver(dev, _lib.SVC, g['Y'][cols], g['C'][cols], None, proto.tol, g['rows'][cols])
                    try:
                        outer, _ = run_batched_smo(solver)
                        _, _, n_held, n_correct = solver.vote_heldout(ncls, codes, np.repeat(np.arange(len(fits)), P),
                                                                      np.tile(np.arange(P), len(fits)),
                                                                      g['held'][f0:f0 + len(fits)])
                    finally:
                        solver.close()
                    for j, (ci, f, _) in enumerate(fits):
                        if n_correct[j] < 0:   # a pair whose walker failed: a failed fit
                            continue
                        scores[ci, f] = float(n_correct[j]) / float(n_held[j])
                        n_iter[ci, f], status[ci, f] = outer[j * P:(j + 1) * P], ''   # an SMO fit records no status
        return scores, n_iter, status

    def _fit_batched(self, X, y, splits, candidates, base, first):
        """(scores, n_iter, status), or None — decided on the first panel, before any solve — when the P columns of one (candidate,
        fold) do not fit the memory budget of a solve."""
        if self.smo_:
            result = self._fit_batched_smo(X, y, splits, candidates, first)
            self.smo_ = result is not None
            return result
        proto = first._prototype()
        classes = np.unique(y)
        codes = np.searchsorted(classes, y)
        ncls = len(classes)
        plan = plan_ovo_columns(codes, ncls, splits, candidates, proto.C, proto.kernel)
        index, cls_tiles, n_pad, pairs = plan['index'], plan['cls_tiles'], plan['n_pad'], plan['pairs']
        P = len(pairs)
        nc, ns = len(candidates), len(splits)
        scores = np.full((nc, ns), np.nan)
        n_iter = np.full((nc, ns, P), -1, dtype=np.int64)
        status = np.full((nc, ns, P), 'failed', dtype=object)
        Xp = np.zeros((n_pad, X.shape[1]))
        Xp[index] = X
        kind = solver_kind(proto.optimizer)
        for gi, g in enumerate(plan['groups']):   # one panel at a time
            with device_panel(Xp, -np.ones(n_pad), 'svc', g['kernel'], y=np.ones(n_pad), storage=proto.storage,
                              tune_placement=proto._streams_panel(), expected_products=proto.max_iter) as (_, dev, free, slab):
                take = groups_per_solve(pairs, cls_tiles, n_pad, free, slab)
                if take == 0 and gi == 0:
                    return None
                take = max(1, take)
                for f0 in range(0, len(g['fits']), take):
                    fits = g['fits'][f0:f0 + take]
                    cols = slice(f0 * P, (f0 + len(fits)) * P)
                    Y, UB = g['Y'][cols], g['UB'][cols]
                    group_of = np.repeat(np.arange(len(fits), dtype=np.int32), P)
                    held = {}

                    def score(solver, _):
                        _, _, held['n_held'], held['n_correct'] = solver.vote_heldout_pairs(plan['data_row'], group_of,
                                                                                            g['held'][f0:f0 + len(fits)])

                    solver = _DevicePairSolver(dev, kind, cls_tiles, pairs * len(fits), Y, UB, 1e-6, proto.max_iter)
                    res = solve_batched(dev, kind, Y, UB, max_iter=proto.max_iter, solver=solver, before_close=score,
                                        vectors=False)
                    for j, (ci, f, _) in enumerate(fits):
                        if held['n_correct'][j] < 0:   # a pair without a support vector: a failed fit
                            continue
                        # (np.mean of the matches: their count over their number)
                        scores[ci, f] = float(held['n_correct'][j]) / float(held['n_held'][j])
                        for q in range(P):
                            n_iter[ci, f, q], status[ci, f, q] = res[j * P + q]['iter'], res[j * P + q]['status']
        return scores, n_iter, status
