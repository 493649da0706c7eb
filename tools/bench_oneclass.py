"""tools/bench_oneclass.py iter|fit|sklearn [n] [d]: the nu-one-class solver at size (profiles/oneclass/).

iter     n = 100 000, d = 128, RBF (gamma = 1 / d), fp64 panel, 16 columns (a nu path, nu = 0.05 ... 0.8), tol = 0 (a column
         still stops where its direction vanishes; `live_throughout` counts those that did not): 5 warm-up iterations, then 50
         timed by the host clock around bq_msolver_run — not by device events: the library hands out none,
         and the run ends in a synchronising copy, so the figure includes the lagged polls and the final state copies.  Under
         `rocprofv3 --kernel-trace --stats` (a run of its own: the device-side figure) the trace splits the iteration into the product
         (symmw_tiles_kernel + symmw_reduce_kernel), the projection (sx_dir_kernel) and the closing (sx_close_kernel + sx_top_kernel).
fit      OneClassSVM(nu = 0.2, tol = 1e-3).fit wall time on the same data, panel build included, after a small warm-up fit.
sklearn  sklearn.svm.OneClassSVM(nu = 0.2, tol = 1e-3).fit on the CPU at n = 20 000 by default (a size it finishes), the same d.
One JSON line each."""
import json
import os
import sys
import time
import warnings

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

mode = sys.argv[1]
n = int(sys.argv[2]) if len(sys.argv) > 2 else (20000 if mode == 'sklearn' else 100000)
d = int(sys.argv[3]) if len(sys.argv) > 3 else 128
rs = np.random.RandomState(0)
# 8 latent Gaussian dimensions embedded isometrically in d, scaled so that gamma = 1 / d acts as gamma = 1 on the latent rows (with
# d independent Gaussian columns every pair of rows is about equally far apart, K is nearly constant and the dual is solved in a few
# iterations); a twentieth of the rows scaled by 3
Z = rs.standard_normal((n, 8))
Z[::20] *= 3
X = Z @ (np.linalg.qr(rs.standard_normal((d, 8)))[0].T * np.sqrt(d))
gamma = 1.0 / d
warnings.simplefilter('ignore')

if mode == 'sklearn':
    from sklearn.svm import OneClassSVM
    t0 = time.perf_counter()
    est = OneClassSVM(kernel='rbf', gamma=gamma, nu=0.2, tol=1e-3, cache_size=4000).fit(X)
    print(json.dumps(dict(mode=mode, what='sklearn.svm.OneClassSVM.fit on the CPU', n=n, d=d, nu=0.2, tol=1e-3,
                          fit_s=time.perf_counter() - t0, n_iter=int(np.ravel(est.n_iter_)[0]), n_sv=int(len(est.support_)))))
    sys.exit(0)

from optiml_amd.ml.svm import OneClassSVM
from optiml_amd.ml.svm._batched import _DeviceSimplexSolver
from optiml_amd.ml.svm.kernels import GaussianKernel
from optiml_amd.opti import KernelQuadratic

kernel = GaussianKernel(gamma=gamma)
OneClassSVM(kernel=kernel, nu=0.2, max_iter=3).fit(X[:2048])   # context, library, allocator warm-up
if mode == 'fit':
    t0 = time.perf_counter()
    est = OneClassSVM(kernel=kernel, nu=0.2, tol=1e-3).fit(X)
    print(json.dumps(dict(mode=mode, what='OneClassSVM.fit, panel build included', n=n, d=d, nu=0.2, tol=1e-3,
                          fit_s=time.perf_counter() - t0, n_iter=est.n_iter_, status=est.status_, n_sv=int(len(est.support_)),
                          kkt_violation=est.kkt_violation_)))
else:
    k, warm, steps = 16, 5, 50
    nus = np.linspace(0.05, 0.8, k)
    t0 = time.perf_counter()
    quad = KernelQuadratic(X, np.zeros(n), 'plain', kernel, tune_placement=True, expected_products=warm + steps)
    dev = quad.device_problem()
    build_s = time.perf_counter() - t0
    solver = _DeviceSimplexSolver(dev, np.ones((k, n)), nus * n, 0.0, 10 ** 6)
    solver.run(warm)
    t0 = time.perf_counter()
    rows, status = solver.run(steps)
    run_s = time.perf_counter() - t0
    print(json.dumps(dict(mode=mode, n=n, d=d, columns=k, warmup=warm, steps=steps, panel_build_s=build_s,
                          iteration_ms=1e3 * run_s / steps, live_throughout=int(sum(s == 'unknown' for s in status)),
                          records=[int(len(r)) for r in rows], f_last=[float(r['f'][-1]) if len(r) else None for r in rows],
                          viol_last=[float(r['r1'][-1]) if len(r) else None for r in rows])))
    solver.close()
    quad.release()
