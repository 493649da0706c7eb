"""One-vs-one probe: the pair-routed product (bq_symmp.hip) inside a batched PG iteration over all k(k-1)/2 pairs, against the same
pairs as a boxes solve on the 16-column wide product (bq_symmw.hip) and against a single-class SVC iteration on all n, at the
headline size (n = 100 000, d = 128, fp64, gaussian with numeric gamma); then OneVsOneSVC end to end against sklearn's
OneVsOneClassifier(SVC).

    python tools/ovo_probe.py [--n 100000] [--ks 4,10,17] [--steps 10] [--warmup 2] [--e2e-n 20000] [--out FILE]

Per k: one class-sorted, tile-padded panel (classes as equal as n allows), and on it, in one process, alternated: the routed pair
solver (bq_msolver_create_pairs), the boxes solver of the same columns (bq_msolver_create_boxes) and the single-class solver
(bq_solver, the problem's own labels), each timed over `steps` iterations between two synchronisations.  Then the routed solver
with every pair but the first given a zero box, so that they stop in their first iteration: its time shows that stopped pairs'
blocks leave the stream.  Reports ms per iteration, the bytes of one routed product from shapes (panel tiles read, slab written
and read, W and OUT) with the fraction of 8 TB/s, and pair 0's f after `steps` iterations routed against boxes.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

TILE = 256
PEAK_BW = 8e12
VEC = TILE * 8


def _strips(n, g):
    return -(-n // g)


def routed_bytes(ct, pairs, live, esz=8):
    """(bytes, panel bytes) of one routed product with the pairs `live` (indices) running: every off-diagonal block of a live pair
    once, every diagonal block of a class with live pairs once per 16 of them; slab entries (a column part per off-diagonal tile and
    a row part per strip, per column that uses them) written once and read once; W per strip (row side: its tiles, column side: its
    tile row) and OUT once per live column."""
    tiles = [int(v) for v in np.diff(ct)]
    panel = slab = vecs = 0
    cnt = [0] * len(tiles)
    for p in live:
        a, b = pairs[p]
        cnt[a] += 1
        cnt[b] += 1
        na, nb_ = tiles[a], tiles[b]
        panel += na * nb_ * TILE * TILE * esz
        strips = nb_ * _strips(na, 8)
        slab += 2 * (na * nb_ + strips) * VEC
        vecs += (na * nb_ + strips) * VEC + (na + nb_) * VEC
    for c, t in enumerate(tiles):
        if cnt[c] == 0:
            continue
        chunks = -(-cnt[c] // 16)
        tri = t * (t + 1) // 2
        strips = sum(_strips(i + 1, 4) for i in range(t))
        panel += chunks * tri * TILE * TILE * esz
        slab += 2 * cnt[c] * ((tri - t) + strips) * VEC
        vecs += chunks * 16 * (tri + strips) * VEC
    return panel + slab + vecs, panel


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=100000)
    ap.add_argument('--d', type=int, default=128)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--ks', default='4,10,17')
    ap.add_argument('--e2e-n', type=int, default=20000)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    from optiml_amd import _lib
    from optiml_amd.datasets import make_multiclass_blobs
    from optiml_amd.ml.svm.kernels import GaussianKernel
    from optiml_amd.ml.svm.multiclass import _DeviceMultiSolver
    from optiml_amd.ml.svm.onevsone import _DevicePairSolver, ovo_pairs, sort_plan
    from optiml_amd.opti import KernelQuadratic
    from optiml_amd.opti.constrained._base import _DeviceSolver

    n, big = a.n, 10 ** 9
    kernel = GaussianKernel(gamma=1.0 / a.d)
    res = dict(n=n, d=a.d, storage='f64', kernel='gaussian gamma=1/d', steps=a.steps, warmup=a.warmup, k={})

    def timed(m):
        t = time.perf_counter()
        m.run(a.steps)
        return (time.perf_counter() - t) * 1e3 / a.steps

    for k in [int(v) for v in a.ks.split(',')]:
        X, y = make_multiclass_blobs(n, a.d, k, seed=0)
        index, ct, n_pad = sort_plan(y, k)
        Xp = np.zeros((n_pad, a.d))
        Xp[index] = X
        ghost = np.ones(n_pad, dtype=bool)
        ghost[index] = False
        pcode = np.repeat(np.arange(k), np.diff(ct) * TILE)
        pairs = ovo_pairs(k)
        m = len(pairs)
        Y = np.stack([np.where(pcode == j, 1., -1.) for _, j in pairs])
        UB = np.stack([np.where(((pcode == i) | (pcode == j)) & ~ghost, 1., 0.) for i, j in pairs])
        t0 = time.perf_counter()
        quad = KernelQuadratic(Xp, -np.ones(n_pad), 'svc', kernel, y=Y[0])
        dev = quad.device_problem()
        build_s = time.perf_counter() - t0
        routed = _DevicePairSolver(dev, _lib.PG, ct, pairs, Y, UB, 1e-30, big)
        boxes = _DeviceMultiSolver(dev, _lib.PG, Y, UB, 1e-30, big)
        single = _DeviceSolver(dev, _lib.PG, np.zeros(n_pad), np.ones(n_pad), np.full(n_pad, 0.5), 1e-30, big)
        for s in (routed, boxes, single):
            s.run(a.warmup)
        r_ms, b_ms, s_ms = [], [], []
        for _ in range(2):   # alternated
            r_ms.append(timed(routed))
            b_ms.append(timed(boxes))
            s_ms.append(timed(single))
        f_r, f_b = routed.state(0)[2], boxes.state(0)[2]
        routed.close()
        boxes.close()
        single.close()
        # every pair but the first stops in its first iteration (zero box): only pair 0's blocks stay in the stream
        UB1 = UB.copy()
        UB1[1:] = 0.
        one = _DevicePairSolver(dev, _lib.PG, ct, pairs, Y, UB1, 1e-30, big)
        one.run(a.warmup)
        one_ms = min(timed(one), timed(one))
        live_after = int(sum(1 for p in range(m) if one.state(p)[1] == 'unknown'))
        one.close()
        quad.release()
        nbytes, panel = routed_bytes(ct, pairs, range(m))
        one_bytes, one_panel = routed_bytes(ct, pairs, [0])
        rm, bm, sm = min(r_ms), min(b_ms), min(s_ms)
        res['k'][k] = dict(
            pairs=m, n_pad=n_pad, cls_tiles=[int(v) for v in ct], panel_build_s=build_s,
            routed_ms=rm, boxes_wide_ms=bm, single_ms=sm, routed_runs_ms=r_ms, boxes_wide_runs_ms=b_ms, single_runs_ms=s_ms,
            routed_vs_boxes_speedup=bm / rm, routed_over_single=rm / sm,
            routed_bytes=nbytes, routed_panel_bytes=panel, routed_frac_8tbs=nbytes / (rm * 1e-3) / PEAK_BW,
            one_live_ms=one_ms, one_live_pairs=live_after, one_live_bytes=one_bytes, one_live_panel_bytes=one_panel,
            pair0_rel_f_diff_routed_vs_boxes=float(abs(f_r - f_b) / abs(f_b)))
        print(json.dumps({k: res['k'][k]}), flush=True)
    if 10 in res['k']:
        res['gates'] = dict(k10_routed_faster_than_boxes=res['k'][10]['routed_ms'] < res['k'][10]['boxes_wide_ms'],
                            k10_routed_le_1_5x_single=res['k'][10]['routed_over_single'] <= 1.5)

    if a.e2e_n > 0:
        from sklearn.multiclass import OneVsOneClassifier
        from optiml_amd.ml.svm import SVC, OneVsOneSVC
        from optiml_amd.ml.svm.losses import hinge
        X, y = make_multiclass_blobs(a.e2e_n, 16, 10, seed=1)
        Xt, _ = make_multiclass_blobs(2000, 16, 10, seed=2)
        kw = dict(loss=hinge, dual=True, reg_intercept=True, kernel=GaussianKernel(gamma=0.05), max_iter=100)

        def fit(kind):
            t = time.perf_counter()
            est = OneVsOneSVC(**kw) if kind == 'ours' else OneVsOneClassifier(SVC(**kw))
            est.fit(X, y)
            return est, time.perf_counter() - t
        ours, ours_first_s = fit('ours')   # the first fit in the process also loads code objects
        ref, ref_s = fit('ref')
        ours, ours_s = fit('ours')
        res['e2e'] = dict(n=a.e2e_n, d=16, k=10, pairs=45, max_iter=100, batched=bool(ours.batched_), ours_first_s=ours_first_s,
                          ours_s=ours_s, one_vs_one_classifier_s=ref_s, speedup=ref_s / ours_s,
                          predictions_equal=bool(np.array_equal(ours.predict(Xt), ref.predict(Xt))),
                          max_abs_decision_diff=float(np.abs(ours.decision_function(Xt) - ref.decision_function(Xt)).max()))
        print(json.dumps({'e2e': res['e2e']}), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as fh:
            json.dump(res, fh, indent=1)


if __name__ == '__main__':
    main()
