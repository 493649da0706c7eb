#!/usr/bin/env python3
"""One fit per flavour of the batched solver (csrc/bq_msolver.hip, bq_mscore.hip) at the smallest shapes that reach its edges, and a
SHA-256 of everything a column produces: x, g, its iteration records, and every output of the held-out calls and of the simplex
offsets.  Two builds of the library that print the same file compute the same bits:

    python3 tools/msolver_flavours.py [path/to/libbcqp_hip.so] > flavours.txt

n = 300 (two 256-row tiles, the second ragged); k = 5 on the 4-column product and k = 17 on the 16-column one (a full chunk and a
ragged one); three classes of unequal sizes for the pairs (the class-sorted panel has ghost rows); two calibrators over disjoint
held-out folds; the simplex solver in its three layouts (one group; labels with a start point; paired with a linear term), all with
zero-width rows, and its two-group columns on the pairs' class-sorted panel with the routed product (a pair twice, a start point
that is a vertex on one column); the held-out scores of the two-group columns (LABELS and PAIRED) and the one-vs-one vote of two
(candidate, fold) groups on the pairs' panel; the runs are cut into several bq_msolver_run calls, and the columns stop at different iterations (the printed
iteration counts), so pos[] renumbers.
"""
import hashlib
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from optiml_amd import _lib  # noqa: E402

if len(sys.argv) > 1:
    from tools._with_lib import use_library
    use_library(sys.argv[1])

from optiml_amd.ml.svm import MultiOutputSVR, OneVsRestSVC, multiclass, multioutput  # noqa: E402
from optiml_amd.ml.svm._batched import (_DeviceMultiSolver, _DeviceSimplex2Solver, _DeviceSimplexPairSolver,  # noqa: E402
                                        _DeviceSimplexSolver, _DeviceSVRSolver)
from optiml_amd.ml.svm.coupling import chunk_calibrators, coupling_columns  # noqa: E402
from optiml_amd.ml.svm.kernels import GaussianKernel  # noqa: E402
from optiml_amd.ml.svm.losses import epsilon_insensitive, hinge  # noqa: E402
from optiml_amd.ml.svm.onevsone import _DevicePairSolver, sort_plan  # noqa: E402
from optiml_amd.ml.svm.ovo_search import plan_ovo_columns  # noqa: E402
from optiml_amd.opti import KernelQuadratic  # noqa: E402
from optiml_amd.opti.unconstrained.stochastic import AdaGrad  # noqa: E402

N, D = 300, 6
KERNEL = GaussianKernel(gamma=0.5)
warnings.simplefilter('ignore')


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def show(name, **arrays):
    for key, a in arrays.items():
        print('%-34s %-10s %s' % (name, key, sha(a)))


def data(seed=0):
    rs = np.random.RandomState(seed)
    X = rs.standard_normal((N, D))
    return rs, X


def labels(rs, X, k):
    """k label rows +-1 of different difficulty: column c separates along its own random direction with its own offset"""
    W = rs.standard_normal((k, D))
    off = np.linspace(-1.0, 1.0, k)
    return np.where(X @ W.T + off > 0, 1.0, -1.0).T.copy()


def folds(k, nfold, C=1.0):
    """k x N boxes: column c holds out fold c % nfold (rows r with r % nfold == fold), except every (nfold + 1)-th column, which
    trains on all rows; cal_of: two calibrators, each fed by the nfold fold columns of one label row"""
    UB = np.full((k, N), C)
    cal_of = np.full(k, -1, dtype=np.int32)
    rows = np.arange(N)
    for c in range(k):
        f = c % (nfold + 1)
        if f < nfold:
            UB[c, rows % nfold == f] = 0.0
            if c // (nfold + 1) < 2:
                cal_of[c] = c // (nfold + 1)
    return UB, cal_of


def run_to_end(solver, name, steps=48, rounds=12):
    """bq_msolver_run in pieces of `steps` until every column has stopped; the records of every piece, then the state"""
    recs = [[] for _ in range(solver.k)]
    for _ in range(rounds):
        part, status = solver.run(steps)
        for c in range(solver.k):
            recs[c].append(part[c])
        if 'unknown' not in status:
            break
    iters = []
    for c in range(solver.k):
        it, st, f = solver.state(c)
        iters.append(it)
        show('%s[%d]' % (name, c), x=solver.get(c, _lib.GET_X_NOW), g=solver.get(c, _lib.GET_G_NOW),
             records=np.concatenate(recs[c]), state=np.array([it, f]))
        print('%-34s %-10s %s' % ('%s[%d]' % (name, c), 'status', st))
    print('%-34s %-10s %s' % (name, 'iters', iters))


def fit_show(name, fit):
    show(name, **{k: v for k, v in fit.items()})


def plain(kind, kname, eps):
    rs, X = data(1)
    Y = labels(rs, X, 5)
    obj = KernelQuadratic(X, -np.ones(N), 'svc', KERNEL, y=Y[0])
    s = _DeviceMultiSolver(obj.device_problem(), kind, Y, np.ones(N), eps, 400)
    run_to_end(s, 'svc_%s_k5' % kname)
    s.close()
    obj.release()


def boxes():
    rs, X = data(2)
    Y = np.repeat(labels(rs, X, 6), 3, axis=0)[:17]   # (label row, fold 0 / fold 1 / all the data)
    UB, cal_of = folds(17, 2)
    obj = KernelQuadratic(X, -np.ones(N), 'svc', KERNEL, y=Y[0])
    s = _DeviceMultiSolver(obj.device_problem(), _lib.PG, Y, UB, 1e-4, 400)
    run_to_end(s, 'svc_boxes_k17')
    b, n_sv, fit = s.heldout_svc(cal_of, 2, decisions=True)
    show('svc_boxes_k17.heldout', intercept=b, n_sv=n_sv)
    fit_show('svc_boxes_k17.heldout', fit)
    s.close()
    obj.release()


def pairs():
    rs, X = data(3)
    codes = np.repeat([0, 1, 2], [150, 100, 50])[rs.permutation(N)]
    X = X + 0.8 * rs.standard_normal((3, D))[codes]
    rows = np.arange(N)
    splits = [(rows[rows % 2 != f], rows[rows % 2 == f]) for f in range(2)]
    plan = coupling_columns(codes, 3, splits, 1.0)
    Xp = np.zeros((plan['n_pad'], D))
    Xp[plan['index']] = X
    obj = KernelQuadratic(Xp, -np.ones(plan['n_pad']), 'svc', KERNEL, y=np.ones(plan['n_pad']))
    cal_of, cal_pairs = chunk_calibrators(plan['cols'])
    chunk = [plan['pairs'][p] for p, _ in plan['cols']]
    s = _DevicePairSolver(obj.device_problem(), _lib.PG, plan['cls_tiles'], chunk, plan['Y'], plan['UB'], 1e-4, 400)
    run_to_end(s, 'svc_pairs_k%d' % len(chunk))
    b, n_sv, fit = s.heldout_pairs(plan['data_row'], cal_of, len(cal_pairs), decisions=True)
    show('svc_pairs.heldout', intercept=b, n_sv=n_sv)
    fit_show('svc_pairs.heldout', fit)
    s.close()
    obj.release()


def svr(k, with_boxes):
    rs, X = data(4 + k)
    T = np.sin(X @ rs.standard_normal((D, k))).T + 0.1 * rs.standard_normal((k, N))
    T[2] = 0.0   # q > 0: the column ends at x = 0 after a few iterations, and is scored without a support vector (NaN)
    eps = np.linspace(0.05, 0.3, k)
    QL = np.concatenate([-T, T], axis=1) + eps[:, None]
    obj = KernelQuadratic(X, QL[0], 'svr', KERNEL)
    if with_boxes:
        UB1, _ = folds(k, 2)
        ub = np.concatenate([UB1, UB1], axis=1)
    else:
        ub = np.ones(2 * N)
    name = 'svr_boxes_k%d' % k if with_boxes else 'svr_k%d' % k
    s = _DeviceSVRSolver(obj.device_problem(), _lib.PG, QL, ub, 1e-4, 400)
    run_to_end(s, name)
    if with_boxes:
        # every column is scored against one target vector: what is compared is the sums' bits
        b, n_sv, sse, n_held = s.heldout(T[0], eps)
        show(name + '.heldout', intercept=b, n_sv=n_sv, sse=sse, n_held=n_held)
    s.close()
    obj.release()


def simplex():
    rs, X = data(9)
    nus = np.linspace(0.05, 0.85, 17)
    UB, _ = folds(17, 2, C=1.0)
    mass = np.array([nus[c] * np.count_nonzero(UB[c]) for c in range(17)])
    obj = KernelQuadratic(X, np.zeros(N), 'plain', KERNEL)
    s = _DeviceSimplexSolver(obj.device_problem(), UB, mass, 1e-4, 400)
    run_to_end(s, 'simplex_k17')
    rho, n_sv, n_free = s.offsets()
    show('simplex_k17.offsets', rho=rho, n_sv=n_sv, n_free=n_free)
    s.close()
    obj.release()


def simplex2(paired):
    """the two-group solver at simplex()'s shapes: LABELS with a start point (a vertex of every group's set), PAIRED from P(0) with
    a linear term; both with the fold boxes (zero-width rows) and NuSVC's own bound on the masses, nu min(n0, n1)"""
    rs, X = data(11)
    S = labels(rs, X, 17)
    t = np.sin(X @ rs.standard_normal(D)) + 0.1 * rs.standard_normal(N)
    nus = np.linspace(0.05, 0.85, 17)
    UB, _ = folds(17, 2, C=1.0)
    groups = [[np.flatnonzero((UB[c] > 0) & (S[c] == sg)) for sg in (1.0, -1.0)] for c in range(17)]
    mass = np.array([[nus[c] * min(len(g) for g in groups[c])] * 2 for c in range(17)])
    obj = KernelQuadratic(X, np.zeros(N), 'plain', KERNEL)
    if paired:
        name = 'simplex2_paired_k17'
        s = _DeviceSimplex2Solver(obj.device_problem(), None, np.concatenate([UB, UB], axis=1), mass,
                                  np.tile(np.concatenate((-t, t)), (17, 1)), 1e-4, 400)
    else:
        name = 'simplex2_labels_k17'
        x0 = np.zeros((17, N))
        for c in range(17):
            for g, rows in enumerate(groups[c]):   # ones on the group's first rows, the remainder on the next
                whole = int(mass[c, g])
                x0[c, rows[:whole]] = 1.0
                x0[c, rows[whole]] = mass[c, g] - whole
        s = _DeviceSimplex2Solver(obj.device_problem(), S, UB, mass, None, 1e-4, 400, x0=x0)
    run_to_end(s, name)
    r1, r2, n_sv, n_free = s.offsets()
    show(name + '.offsets', r1=r1, r2=r2, n_sv=n_sv, n_free=n_free)
    # every column is scored against one label / target vector: what is compared is the sums' bits
    r1, r2, n_sv, n_free, n_held, n_correct, sse = s.heldout(t if paired else S[0])
    show(name + '.heldout', r1=r1, r2=r2, n_sv=n_sv, n_free=n_free, n_held=n_held, n_correct=n_correct, sse=sse)
    s.close()
    obj.release()


def pairs_vote():
    """the one-vs-one vote on pairs()'s three unequal classes: two (candidate, fold) groups of the three pairs, group g holding out
    the rows r with r % 2 == g, with different boxes"""
    rs, X = data(13)
    codes = np.repeat([0, 1, 2], [150, 100, 50])[rs.permutation(N)]
    X = X + 0.8 * rs.standard_normal((3, D))[codes]
    rows = np.arange(N)
    splits = [(rows[rows % 2 != f], rows[rows % 2 == f]) for f in range(2)]
    plan = plan_ovo_columns(codes, 3, splits, [{'C': 1.0}], 1.0, KERNEL)
    g = plan['groups'][0]
    Xp = np.zeros((plan['n_pad'], D))
    Xp[plan['index']] = X
    UB = g['UB'] * np.repeat([1.0, 0.5], 3)[:, None]
    obj = KernelQuadratic(Xp, -np.ones(plan['n_pad']), 'svc', KERNEL, y=np.ones(plan['n_pad']))
    s = _DevicePairSolver(obj.device_problem(), _lib.PG, plan['cls_tiles'], plan['pairs'] * 2, g['Y'], UB, 1e-4, 400)
    run_to_end(s, 'svc_pairs_vote_k6')
    b, n_sv, n_held, n_correct, pred = s.vote_heldout_pairs(plan['data_row'], np.repeat(np.arange(2, dtype=np.int32), 3), g['held'],
                                                            predictions=True)
    show('svc_pairs_vote_k6.vote', intercept=b, n_sv=n_sv, n_held=n_held, n_correct=n_correct, pred=pred)
    s.close()
    obj.release()


def simplex2_blocks_pairs():
    """the two-group columns of the class pairs on pairs()'s three unequal classes (the class-sorted panel has ghost rows) with the
    routed product: five columns, pairs (0, 1) and (0, 2) twice, four of them holding out a third of their rows (zero-width
    rows); every column starts from a point of its set, column 1 from a vertex (ones on each group's first rows), the others
    from the uniform point"""
    rs, X = data(12)
    codes = np.repeat([0, 1, 2], [150, 100, 50])[rs.permutation(N)]
    X = X + 0.8 * rs.standard_normal((3, D))[codes]
    index, cls_tiles, n_pad = sort_plan(codes, 3)
    Xp = np.zeros((n_pad, D))
    Xp[index] = X
    chunk = [(0, 1), (0, 2), (1, 2), (0, 2), (0, 1)]
    nus = [0.3, 0.5, 0.7, 0.15, 0.6]
    k = len(chunk)
    UB, mass, x0 = np.zeros((k, n_pad)), np.zeros((k, 2)), np.zeros((k, n_pad))
    for c, (i, j) in enumerate(chunk):
        groups = []
        for cls in (j, i):   # group 0: the larger class
            rows = np.flatnonzero(codes == cls)
            if c != 4:
                rows = rows[rows % 3 != c % 3]
            groups.append(index[rows])
            UB[c, index[rows]] = 1.0
        for g, prow in enumerate(groups):
            mass[c, g] = nus[c] * min(len(q) for q in groups)
            if c == 1:
                whole = int(mass[c, g])
                x0[c, prow[:whole]] = 1.0
                x0[c, prow[whole]] = mass[c, g] - whole
            else:
                x0[c, prow] = mass[c, g] / len(prow)
    obj = KernelQuadratic(Xp, np.zeros(n_pad), 'plain', KERNEL)
    s = _DeviceSimplexPairSolver(obj.device_problem(), cls_tiles, chunk, UB, mass, 1e-4, 400, x0=x0)
    name = 'simplex2_blocks_pairs_k%d' % k
    run_to_end(s, name)
    r1, r2, n_sv, n_free = s.offsets()
    show(name + '.offsets', r1=r1, r2=r2, n_sv=n_sv, n_free=n_free)
    s.close()
    obj.release()


def lagrangian():
    """the augmented-Lagrangian batch through its estimators (the rule's parameters are theirs to build): what
    solve_batched_al hands back for every column"""
    def hashed(module, name):
        inner = module.solve_batched_al

        def wrapped(solver, *a, **kw):
            out = inner(solver, *a, **kw)
            for c, r in enumerate(out):
                show('%s[%d]' % (name, c), x=r['x'], past_x=r['past_x'], g=r['g'], step=r['step'], dual=r['dual'], records=r['rows'],
                     state=np.array([r['iter'], r['f_x']]))
            print('%-34s %-10s %s' % (name, 'iters', [int(r['iter']) for r in out]))
            return out
        module.solve_batched_al = wrapped

    hashed(multiclass, 'al_svc_k5')
    hashed(multioutput, 'al_svr_k5')
    rs, X = data(10)
    codes = rs.randint(0, 5, N)
    X = X + 1.5 * rs.standard_normal((5, D))[codes]
    kw = dict(kernel=KERNEL, C=1.0, reg_intercept=False, dual=True, optimizer=AdaGrad, learning_rate=1., max_iter=300, tol=0.05, random_state=1)
    est = OneVsRestSVC(loss=hinge, **kw).fit(X, codes)
    assert est.batched_ and est.lagrangian_
    T = np.sin(X @ rs.standard_normal((D, 5)))
    est = MultiOutputSVR(loss=epsilon_insensitive, epsilon=0.1, **kw).fit(X, T)
    assert est.batched_ and est.lagrangian_


if __name__ == '__main__':
    plain(_lib.PG, 'pg', 1e-2)
    plain(_lib.FW, 'fw', 1e-1)
    boxes()
    pairs()
    svr(5, False)
    svr(17, True)
    simplex()
    simplex2(False)
    simplex2(True)
    lagrangian()
    simplex2_blocks_pairs()
    pairs_vote()
