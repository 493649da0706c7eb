"""tools/bench_nu.py iter|oneclass|labels|paired|ovo|ovo_pairs|ovo_labels [n] [d]: the two-group simplex solver (NuSVC / NuSVR) at size beside the one-class
solver on the same build, machine and panel (profiles/nu/).

iter      n = 100 000, d = 128, RBF (gamma = 1 / d), fp64 panel built once, 16 columns (nu = 0.05 ... 0.8), tol = 0.  Three rounds of
          (one-class, LABELS, PAIRED), each a fresh solver with 5 warm-up iterations and 50 timed by the host clock around
          bq_msolver_run (tools/bench_oneclass.py's figure: it includes the lagged polls and the final state copies).  Per flavour the
          three figures, their median and their spread (max - min); the one-class figure is the yardstick, and its spread over the
          three repeats the run-to-run spread the comparison is read against.
oneclass | labels | paired   one such solve alone, for `rocprofv3 --kernel-trace --stats` (a run of its own): the trace splits the
          iteration into the product (symmw_tiles_kernel + symmw_reduce_kernel), the projection (sx_dir_kernel, after sx_tau_kernel for
          the two-group layouts) and the closing (sx_close_kernel + sx_top_kernel).
ovo       one-vs-one nu-SVC at size (profiles/ovo_nu/): the same rows in 10 equal classes on the class-sorted, ghost-padded panel
          (n_pad = 102 400), 45 pair columns at nu = 0.5, tol = 0.  Three rounds of (ovo_pairs, ovo_labels), timed as above:
          ovo_pairs   bq_msolver_create_simplex2_pairs: the BLOCKS columns on the routed product (at most one panel stream);
          ovo_labels  the same 45 columns as LABELS columns with zero boxes outside the pair, through bq_msolver_create_simplex2
                      (three 16-column panel streams, every column kernel over all n_pad rows) — the route a library without
                      the pairs entry point has.
ovo_pairs | ovo_labels   one such solve alone (a kernel trace; ovo_labels also runs on a library of before the entry point).
One JSON line."""
import json
import os
import sys
import time
import warnings

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

mode = sys.argv[1]
n = int(sys.argv[2]) if len(sys.argv) > 2 else 100000
d = int(sys.argv[3]) if len(sys.argv) > 3 else 128
rs = np.random.RandomState(0)
# tools/bench_oneclass.py's rows: 8 latent Gaussian dimensions embedded isometrically in d; labels and targets from the latent rows
Z = rs.standard_normal((n, 8))
Z[::20] *= 3
X = Z @ (np.linalg.qr(rs.standard_normal((d, 8)))[0].T * np.sqrt(d))
y = np.where(Z[:, 0] + 0.5 * Z[:, 1] ** 2 + 0.6 * rs.standard_normal(n) > 0.4, 1., -1.)
t = np.sin(Z[:, 0]) + 0.5 * Z[:, 1] + 0.2 * rs.standard_normal(n)
gamma = 1.0 / d
warnings.simplefilter('ignore')

from optiml_amd.ml.svm import OneClassSVM   # noqa: E402
from optiml_amd.ml.svm import _batched   # noqa: E402
from optiml_amd.ml.svm._batched import _DeviceSimplex2Solver, _DeviceSimplexSolver   # noqa: E402
from optiml_amd.ml.svm.onevsone import ovo_pairs, sort_plan   # noqa: E402
from optiml_amd.ml.svm.kernels import GaussianKernel   # noqa: E402
from optiml_amd.opti import KernelQuadratic   # noqa: E402

kernel = GaussianKernel(gamma=gamma)
OneClassSVM(kernel=kernel, nu=0.2, max_iter=3).fit(X[:2048])   # context, library, allocator warm-up
k, warm, steps = 16, 5, 50
nus = np.linspace(0.05, 0.8, k)
flavours = ('oneclass', 'labels', 'paired')
rounds = 3 if mode in ('iter', 'ovo') else 1
ovo = mode.startswith('ovo')
if ovo:   # the class-sorted panel of 10 equal classes (shifted apart) and the 45 pair columns
    flavours = ('ovo_pairs', 'ovo_labels')
    ncls = 10
    codes = rs.permutation(np.arange(n) % ncls)
    X = X + 0.5 * np.sqrt(d) * rs.standard_normal((ncls, d))[codes]
    index, cls_tiles, n_pad = sort_plan(codes, ncls)
    Xp = np.zeros((n_pad, d))
    Xp[index] = X
    ghost = np.ones(n_pad, dtype=bool)
    ghost[index] = False
    pcode = np.repeat(np.arange(ncls), np.diff(cls_tiles) * 256)
    pairs = ovo_pairs(ncls)
    counts = np.bincount(codes)
    X, n, k = Xp, n_pad, len(pairs)
    UB = np.stack([np.where(((pcode == i) | (pcode == j)) & ~ghost, 1., 0.) for i, j in pairs])
    ovo_mass = np.array([[0.5 * (counts[i] + counts[j]) / 2] * 2 for i, j in pairs])
t0 = time.perf_counter()
quad = KernelQuadratic(X, np.zeros(n), 'plain', kernel, tune_placement=True, expected_products=rounds * 3 * (warm + steps))
dev = quad.device_problem()
build_s = time.perf_counter() - t0


def solver_of(flavour):
    if flavour == 'ovo_pairs':
        return _batched._DeviceSimplexPairSolver(dev, cls_tiles, pairs, UB, ovo_mass, 0.0, 10 ** 6)
    if flavour == 'ovo_labels':
        S = np.stack([np.where(pcode == j, 1., -1.) for _, j in pairs])
        return _DeviceSimplex2Solver(dev, S, UB, ovo_mass, None, 0.0, 10 ** 6)
    if flavour == 'oneclass':
        return _DeviceSimplexSolver(dev, np.ones((k, n)), nus * n, 0.0, 10 ** 6)
    mass = np.repeat(nus[:, None] * n / 2, 2, axis=1)
    if flavour == 'labels':
        return _DeviceSimplex2Solver(dev, np.tile(y, (k, 1)), np.ones((k, n)), mass, None, 0.0, 10 ** 6)
    return _DeviceSimplex2Solver(dev, None, np.ones((k, 2 * n)), mass, np.tile(np.concatenate((-t, t)), (k, 1)), 0.0, 10 ** 6)


def timed(flavour):
    solver = solver_of(flavour)
    solver.run(warm)
    t0 = time.perf_counter()
    rows, status = solver.run(steps)
    run_s = time.perf_counter() - t0
    solver.close()
    return dict(iteration_ms=1e3 * run_s / steps, live_throughout=int(sum(s == 'unknown' for s in status)),
                records=[int(len(r)) for r in rows])


out = dict(mode=mode, n=n, d=d, columns=k, warmup=warm, steps=steps, panel_build_s=build_s)
runs = {f: [] for f in (flavours if mode in ('iter', 'ovo') else (mode,))}
for _ in range(rounds):
    for f in runs:
        runs[f].append(timed(f))
for f, rr in runs.items():
    ms = [r['iteration_ms'] for r in rr]
    out[f] = dict(iteration_ms=ms, median_ms=float(np.median(ms)), spread_ms=max(ms) - min(ms),
                  live_throughout=[r['live_throughout'] for r in rr], records=rr[0]['records'])
if mode == 'iter':
    base = out['oneclass']['median_ms']
    out['labels_over_oneclass'] = out['labels']['median_ms'] / base
    out['paired_over_oneclass'] = out['paired']['median_ms'] / base
if mode == 'ovo':
    out['pairs_over_labels'] = out['ovo_pairs']['median_ms'] / out['ovo_labels']['median_ms']
print(json.dumps(out))
quad.release()
