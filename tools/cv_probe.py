"""Cross-validation probe: the 16-column MFMA product (bq_symmw.hip) against the 4-column VALU product (bq_symm.hip) inside a batched
PG iteration at the headline size (n = 100 000, d = 128, fp64, gaussian with numeric gamma), and an end-to-end search.

    python tools/cv_probe.py [--n 100000] [--steps 10] [--warmup 2] [--ks 1,4,16,17,32,64] [--search-n 20000] [--out FILE]

Same process, same panel: for every k a boxes solver (bq_msolver_create_boxes, the wide product) and a shared-box solver
(bq_msolver_create, bq_symm.hip) of k columns, each timed over `steps` iterations between two synchronisations, alternated.
Reports ms per iteration, the bytes of one product from shapes (panel + slab + vectors) with the fraction of 8 TB/s, and its
flop with the fraction of the 78.6 TF fp64 matrix peak.  Then the f32 panel at k = 16, and SVCGridSearchCV (5 folds x 8 C, PG)
against sklearn's GridSearchCV(SVC) at n = `search-n`: wall time of both (ours first and again after GridSearchCV) and whether
cv_results_ are equal.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

TILE = 256
PEAK_BW, PEAK_F64_MFMA = 8e12, 78.6e12


def _strips(nb, jg):
    return sum(i // jg + 1 for i in range(nb))


def product_cost(n, k, wide, esz=8):
    """(bytes, panel bytes, flop) of one product with k live columns, from what the kernels touch.
    wide (bq_symmw.hip, chunks of 16, 4-tile strips): the panel once per chunk; slab entries (a column part per off-diagonal tile
    and a row part per strip) written and read for the LIVE columns only; W read for all 16 slots of a chunk, W_I once per strip
    and W_J once per strip tile; OUT written for the live columns.
    4-column (bq_symm.hip, 2-tile strips): the panel once per chunk; slab entries written for all 4 slots of a chunk and read for
    the live ones; W of the 4 slots read per strip tile on the row and the column side and once per strip row; OUT for the live ones.
    flop: 4 per stored off-diagonal element and 2 per diagonal-tile element, per live column."""
    nb = -(-n // TILE)
    tiles = nb * (nb + 1) // 2
    vec = TILE * 8
    if wide:
        ck, jg = 16, 4
        strips = _strips(nb, jg)
        chunks = -(-k // ck)
        entries = (tiles - nb) + strips
        slab = 2 * entries * vec * k
        vecs = chunks * (strips + tiles) * vec * ck + nb * vec * k
    else:
        ck, jg = 4, 2
        strips = _strips(nb, jg)
        chunks = -(-k // ck)
        entries = (tiles - nb) + strips
        slab = entries * vec * (chunks * ck + k)
        vecs = chunks * (2 * tiles + strips) * vec * ck + nb * vec * k
    panel = chunks * tiles * TILE * TILE * esz
    flop = k * (4 * (tiles - nb) + 2 * nb) * TILE * TILE
    return panel + slab + vecs, panel, flop


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=100000)
    ap.add_argument('--d', type=int, default=128)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--ks', default='1,4,16,17,32,64')
    ap.add_argument('--search-n', type=int, default=20000)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    from optiml_amd import _lib
    from optiml_amd.datasets import make_multiclass_blobs
    from optiml_amd.ml.svm.kernels import GaussianKernel
    from optiml_amd.ml.svm.multiclass import _DeviceMultiSolver
    from optiml_amd.opti import KernelQuadratic

    ks = [int(v) for v in a.ks.split(',')]
    kmax = max(ks)
    n = a.n
    X, y = make_multiclass_blobs(n, a.d, 2, seed=0)
    rs = np.random.RandomState(0)
    Y = np.stack([np.where(y == 1, 1., -1.)] + [np.where(rs.uniform(size=n) < 0.5, 1., -1.) for _ in range(kmax - 1)])
    kernel = GaussianKernel(gamma=1.0 / a.d)
    big = 10 ** 9
    res = dict(n=n, d=a.d, steps=a.steps, warmup=a.warmup, kernel='gaussian gamma=1/d', k={})

    def timed(m):
        t = time.perf_counter()
        m.run(a.steps)
        return (time.perf_counter() - t) * 1e3 / a.steps

    def sweep(storage, kset):
        quad = KernelQuadratic(X, -np.ones(n), 'svc', kernel, y=Y[0], storage=storage)
        dev = quad.device_problem()
        esz = 8 if storage == 'f64' else 4
        out = {}
        for k in kset:
            UB = np.ones((k, n))
            wide = _DeviceMultiSolver(dev, _lib.PG, Y[:k].copy(), UB, 1e-30, big)
            old = _DeviceMultiSolver(dev, _lib.PG, Y[:k].copy(), np.ones(n), 1e-30, big)
            wide.run(a.warmup)
            old.run(a.warmup)
            w_ms, o_ms = [], []
            for _ in range(2):   # alternated
                w_ms.append(timed(wide))
                o_ms.append(timed(old))
            fw, fo = wide.state(0)[2], old.state(0)[2]
            wide.close()
            old.close()
            wb, wp, fl = product_cost(n, k, True, esz)
            ob, _, _ = product_cost(n, k, False, esz)
            wm, om = min(w_ms), min(o_ms)
            out[k] = dict(wide_ms=wm, symm4_ms=om, wide_runs_ms=w_ms, symm4_runs_ms=o_ms, speedup=om / wm,
                          wide_bytes=wb, wide_panel_bytes=wp, wide_frac_8tbs=wb / (wm * 1e-3) / PEAK_BW,
                          symm4_bytes=ob, symm4_frac_8tbs=ob / (om * 1e-3) / PEAK_BW,
                          flop=fl, wide_frac_mfma_peak=fl / (wm * 1e-3) / PEAK_F64_MFMA,
                          col0_rel_f_diff=float(abs(fw - fo) / abs(fo)))
            print(json.dumps({storage: {k: out[k]}}), flush=True)
        quad.release()
        return out

    res['k'] = sweep('f64', ks)
    res['f32_k16'] = sweep('f32', [16])[16]
    res['target_k16_le_12ms'] = bool(res['k'].get(16, {}).get('wide_ms', 1e9) <= 12.0) if 16 in ks else None

    if a.search_n > 0:
        from sklearn.model_selection import GridSearchCV, StratifiedKFold
        from optiml_amd.ml.svm import SVC, SVCGridSearchCV
        from optiml_amd.ml.svm.losses import hinge
        m = a.search_n
        Xs, ys = make_multiclass_blobs(m, 16, 2, seed=1)
        kw = dict(loss=hinge, dual=True, reg_intercept=True, kernel=GaussianKernel(gamma=0.05), max_iter=100)
        grid = {'C': [0.01, 0.03, 0.1, 0.3, 1.0, 3.0, 10.0, 30.0]}
        def search(kind):
            t = time.perf_counter()
            est = (SVCGridSearchCV if kind == 'ours' else GridSearchCV)(SVC(**kw), grid, cv=StratifiedKFold(5)).fit(Xs, ys)
            return est, time.perf_counter() - t
        ours, ours_first_s = search('ours')   # the first search in the process also loads code objects
        ref, ref_s = search('ref')
        ours, ours_s = search('ours')
        same = all(np.array_equal(ours.cv_results_[key], ref.cv_results_[key])
                   for key in ['split%d_test_score' % i for i in range(5)] + ['mean_test_score', 'rank_test_score'])
        res['search'] = dict(n=m, d=16, folds=5, candidates=8, max_iter=100, batched=bool(ours.batched_), ours_first_s=ours_first_s,
                             ours_s=ours_s,
                             gridsearchcv_s=ref_s, speedup=ref_s / ours_s, cv_results_equal=bool(same),
                             best_params_equal=ours.best_params_ == ref.best_params_)
        print(json.dumps({'search': res['search']}), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as fh:
            json.dump(res, fh, indent=1)


if __name__ == '__main__':
    main()
