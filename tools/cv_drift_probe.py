"""Where a cross-validation column and SVC.fit on its fold part: per-iteration alphas of the three solves of one fold dual.

    python tools/cv_drift_probe.py [--iters 100] [--out FILE] [--dump NPZ]

The search case of tests/test_gpu_cv.py (binary blobs, n = 240, d = 4, gaussian gamma = 0.2, StratifiedKFold(5), C in
{0.1, 1, 10}, PG).  For every (C, fold):
  column  the fold's column in ONE batched solve of all 15 columns on the n-row panel (bq_msolver_create_boxes), one step at a time
  fold    the single-column device solver on the fold's own panel (what SVC.fit runs), one step at a time
  oracle  bcqp_oracle.projected_gradient on Q[tr][:, tr] in fp64 NumPy
x_i is the point iteration i is evaluated at (the oracle's x_at[i]).  Each device solve runs twice in the process and is compared
bit for bit.  Per iteration it records max |x_column - x_fold| and both against the oracle, and, for column against fold, the first
iteration where the free set (0 < x < C, to 1e-12) differs.  --dump writes every x so that two processes can be compared bit for
bit.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=100)
    ap.add_argument('--out', default=None)
    ap.add_argument('--dump', default=None)
    a = ap.parse_args()
    from sklearn.model_selection import StratifiedKFold
    from optiml_amd import _lib
    from optiml_amd.datasets import make_multiclass_blobs
    from optiml_amd.ml.svm.kernels import GaussianKernel
    from optiml_amd.ml.svm.model_selection import plan_columns
    from optiml_amd.ml.svm.multiclass import _DeviceMultiSolver
    from optiml_amd.opti import KernelQuadratic
    from optiml_amd.opti.constrained._base import _DeviceSolver
    from oracle import bcqp_oracle as bo, svm_oracle as so

    N = a.iters
    X, y = make_multiclass_blobs(240, 4, 2, seed=3)
    n = len(y)
    kernel = GaussianKernel(gamma=0.2)
    splits = list(StratifiedKFold(5).split(X, y))
    cands = [{'C': 0.1}, {'C': 1.0}, {'C': 10.0}]
    groups, _ = plan_columns(X, y, splits, cands, 1.0, kernel, multiclass=False)
    g = groups[0]

    def column_run():
        quad = KernelQuadratic(X, -np.ones(n), 'svc', kernel, y=g['Y'][0])
        s = _DeviceMultiSolver(quad.device_problem(), _lib.PG, g['Y'], g['UB'], 1e-6, N + 1)
        xs = np.zeros((N + 1, len(g['cols']), n))
        for it in range(N + 1):   # after step it + 1 the solver's x is x_it (the step it decided is applied by the next update)
            s.run(1)
            for c in range(len(g['cols'])):
                xs[it, c] = s.get(c, _lib.GET_X_NOW)
        s.close()
        quad.release()
        return xs

    def fold_run(tr, C):
        yt = np.where(y[tr] == 1, 1., -1.)
        quad = KernelQuadratic(np.ascontiguousarray(X[tr]), -np.ones(len(tr)), 'svc', kernel, y=yt)
        ub = np.full(len(tr), C)
        s = _DeviceSolver(quad.device_problem(), _lib.PG, np.zeros(len(tr)), ub, ub / 2, 1e-6, N + 1)
        xs = np.zeros((N + 1, len(tr)))
        for it in range(N + 1):
            s.run(1)
            xs[it] = s.get(_lib.GET_X_NOW)
        s.close()
        quad.release()
        return xs

    col, col2 = column_run(), column_run()
    res = dict(iters=N, column_bitwise_repeatable=bool(np.array_equal(col, col2)), cases=[])
    dump = {}
    fold_repeatable = True
    K = so.gram('rbf', X, gamma=0.2)
    for j, (ci, f, _, C) in enumerate(g['cols']):
        tr = splits[f][0]
        fx, fx2 = fold_run(tr, C), fold_run(tr, C)
        fold_repeatable &= bool(np.array_equal(fx, fx2))
        Q, q, ub = so.svc_dual(K[np.ix_(tr, tr)], np.where(y[tr] == 1, 1., -1.), C)
        orc = bo.projected_gradient(Q, q, ub, max_iter=N, keep_x=range(N + 1))
        ox = np.array([orc['x_at'][i] for i in range(min(N, orc['iter']) + 1)])
        cx = col[:, j][:, tr]
        held_out_zero = bool(np.all(col[:, j][:, splits[f][1]] == 0))
        m = min(len(ox), N + 1)
        d_cf = np.abs(cx - fx).max(axis=1)
        d_co = np.abs(cx[:m] - ox).max(axis=1)
        d_fo = np.abs(fx[:m] - ox).max(axis=1)
        free = lambda x: (x > 1e-12) & (x < C - 1e-12)
        free_diff = [i for i in range(N + 1) if not np.array_equal(free(cx[i]), free(fx[i]))]
        case = dict(C=C, fold=f, held_out_zero=held_out_zero, oracle_iters=int(orc['iter']), oracle_status=orc['status'],
                    first_free_set_diff=free_diff[0] if free_diff else None,
                    first_nonzero_column_vs_fold=int(np.argmax(d_cf > 0)) if (d_cf > 0).any() else None,
                    column_vs_fold=[float(v) for v in d_cf[::10]] + [float(d_cf[-1])],
                    column_vs_oracle=[float(v) for v in d_co[::10]] + [float(d_co[-1])],
                    fold_vs_oracle=[float(v) for v in d_fo[::10]] + [float(d_fo[-1])])
        res['cases'].append(case)
        print(json.dumps(case), flush=True)
        dump['col_%d' % j], dump['fold_%d' % j] = cx, fx
    res['fold_bitwise_repeatable'] = fold_repeatable
    print(json.dumps({k: v for k, v in res.items() if k != 'cases'}), flush=True)
    if a.dump:
        np.savez(a.dump, **dump)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as fh:
            json.dump(res, fh, indent=1)


if __name__ == '__main__':
    main()
