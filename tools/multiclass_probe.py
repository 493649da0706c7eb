"""Batched one-vs-rest PG iteration against the single-class one at the headline size (n = 100 000, d = 128, fp64, gaussian).

    python tools/multiclass_probe.py [--n 100000] [--steps 20] [--warmup 3] [--ks 1,2,4,8,10,16,17] [--out FILE]

Same process, same panel: a single-class ProjectedGradient solver (bq_solver_*) and batched solvers (bq_msolver_*) of k classes;
after a warm-up each is timed over `steps` iterations (one run of `steps` iterations between two synchronisations), the
single-class solver before every batched one (alternated).  Prints / writes JSON: ms per iteration, the ratio to the single-class
iteration, the bytes of one batched product from shapes (panel + slab + vectors) and the resulting fraction of 8 TB/s, and the
f of class 0 (the problem's own labels) after `steps` iterations of every batched solve against the single-class solve
(rtol 1e-12).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CK, SJG, TILE = 4, 2, 256   # bq_common.h BQ_SYMM_CK, bq_symm.hip SJG


def product_bytes(n, k, esz=8):
    """Bytes one batched product moves for k live classes: the panel once per chunk of CK, each chunk's slab written and read,
    the vectors (W read per strip tile, OUT written)."""
    nb = -(-n // TILE)
    tiles = nb * (nb + 1) // 2
    strips = sum(i // SJG + 1 for i in range(nb))
    chunks = -(-k // CK)
    panel = tiles * TILE * TILE * esz
    slab_entries = (tiles - nb) + strips   # column parts of the off-diagonal tiles + one row part per strip, per column
    slab = 2 * slab_entries * TILE * 8 * CK
    vecs = (strips * SJG * 2 + nb) * TILE * 8 * CK   # W (row and column side of each strip tile) + OUT, per column
    return chunks * (panel + slab + vecs), chunks * panel


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=100000)
    ap.add_argument('--d', type=int, default=128)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--ks', default='1,2,4,8,10,16,17')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    from optiml_amd import _lib
    from optiml_amd.datasets import make_multiclass_blobs
    from optiml_amd.ml.svm.kernels import gaussian
    from optiml_amd.ml.svm.multiclass import _DeviceMultiSolver
    from optiml_amd.opti import KernelQuadratic
    from optiml_amd.opti.constrained._base import _DeviceSolver

    ks = [int(v) for v in a.ks.split(',')]
    kmax = max(ks)
    X, y = make_multiclass_blobs(a.n, a.d, kmax, seed=0)
    Y = np.stack([np.where(y == c, 1., -1.) for c in range(kmax)])
    n = a.n
    ub = np.ones(n)
    quad = KernelQuadratic(X, -np.ones(n), 'svc', gaussian, y=Y[0])
    t0 = time.perf_counter()
    dev = quad.device_problem()
    build_s = time.perf_counter() - t0
    big = 10 ** 9

    def timed(run):
        t = time.perf_counter()
        run(a.steps)
        return (time.perf_counter() - t) * 1e3 / a.steps

    # the single-class solver runs on the problem's own labels, class 0's: the correctness check is class 0's f after `steps`
    # iterations, batched against alone (every class against its own SVC is tests/test_gpu_multiclass.py's size case)
    ref = _DeviceSolver(dev, _lib.PG, np.zeros(n), ub, ub / 2, 1e-6, big)
    ref.run(a.warmup)
    alone = _DeviceSolver(dev, _lib.PG, np.zeros(n), ub, ub / 2, 1e-6, big)
    f0 = alone.run(a.steps)[0]['f'][-1]
    alone.close()

    res = dict(n=n, d=a.d, storage='f64', steps=a.steps, warmup=a.warmup, panel_build_s=build_s, k={})
    for k in ks:
        m = _DeviceMultiSolver(dev, _lib.PG, Y[:k].copy(), ub, 1e-6, big)
        recs, _ = m.run(a.warmup)
        single_ms = timed(ref.run)
        batched_ms = timed(m.run)
        m.close()
        chk = _DeviceMultiSolver(dev, _lib.PG, Y[:k].copy(), ub, 1e-6, big)
        recs, _ = chk.run(a.steps)
        chk.close()
        f = recs[0]['f'][-1]
        ok = bool(abs(f - f0) <= 1e-12 * abs(f0))
        nbytes, panel_bytes = product_bytes(n, k)
        res['k'][k] = dict(single_ms=single_ms, batched_ms=batched_ms, ratio=batched_ms / single_ms,
                           ratio_to_k_single=batched_ms / (k * single_ms), product_bytes=nbytes, panel_bytes=panel_bytes,
                           tb_per_s=nbytes / (batched_ms * 1e-3) / 1e12, frac_8tbs=nbytes / (batched_ms * 1e-3) / 8e12,
                           class0_f_matches_single_rtol_1e12=ok, class0_rel_f_err=float(abs(f - f0) / abs(f0)))
        print(json.dumps({k: res['k'][k]}), flush=True)
    ref.close()
    res['gates'] = {'k4_le_2x': res['k'].get(4, {}).get('ratio', 0) <= 2.0 if 4 in res['k'] else None,
                    'k10_le_3.5x': res['k'].get(10, {}).get('ratio', 0) <= 3.5 if 10 in res['k'] else None,
                    'never_slower_than_k_single': all(v['ratio_to_k_single'] <= 1.0 for kk, v in res['k'].items() if kk >= 2)}
    print(json.dumps(res['gates']))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as fh:
            json.dump(res, fh, indent=1)


if __name__ == '__main__':
    main()
