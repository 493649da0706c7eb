"""The batched SMO measured (`python tools/smo_batch_probe.py [N D CLASSES [OUT.json]]`, default 20000 32 10).

(a) `OneVsRestSVC(optimizer='smo').fit`, RBF gamma = 1/D, C = 1, tol 1e-3: the batched solve (`batch_smo = True`) against the same
    commit forced to one `SVC.fit` per class (`batch_smo = False`, the path every earlier commit takes).
(b) k = 1, 2, 4, 8, 16, 64, 256, 512 identical columns (class 0 against the rest) on one panel, `solve_batched_smo`, against one
    single fit (`SMOClassifier.minimize`, helpers on) on the same panel and the time of one panel build — the k single fits of the
    per-column path cost k times those two.
Host clock around calls that end in a device synchronise; two passes in one process, both recorded, the second is the one to
quote (the first warms code objects and the panel cache).  Prints one JSON record (profiles/smo_batched/)."""
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np

from optiml_amd import _lib
from optiml_amd.datasets import make_multiclass_blobs
from optiml_amd.ml.svm import OneVsRestSVC
from optiml_amd.ml.svm._batched import solve_batched_smo
from optiml_amd.ml.svm.kernels import GaussianKernel
from optiml_amd.ml.svm.losses import hinge
from optiml_amd.ml.svm.smo import SMOClassifier
from optiml_amd.opti import KernelQuadratic

n, d, classes = (int(a) for a in (sys.argv[1:4] if len(sys.argv) > 3 else (20000, 32, 10)))
X, y = make_multiclass_blobs(n, d, classes, seed=1)
kernel = GaussianKernel(gamma=1.0 / d)
kw = dict(loss=hinge, kernel=kernel, C=1., dual=True, optimizer='smo', tol=1e-3)
rec = dict(n=n, d=d, classes=classes, tol=1e-3, C=1.0)


def clock(fn):
    t0 = time.perf_counter()
    out = fn()
    return time.perf_counter() - t0, out


for rep in range(2):
    fits = {}
    for name, force in (('batched', True), ('per_class', False)):
        est = OneVsRestSVC(**kw)
        est.batch_smo = force
        fits[name] = clock(lambda: est.fit(X, y))
    (tb, eb), (tp, ep) = fits['batched'], fits['per_class']
    same = all(np.array_equal(a.alphas_, b.alphas_) and a.intercept_ == b.intercept_ for a, b in zip(eb.estimators_, ep.estimators_))
    rec['ovr_pass%d' % rep] = dict(batched_fit_s=tb, per_class_fit_s=tp, smo_=bool(eb.smo_), same_bits=bool(same),
                                   outer_iterations=[int(e.optimizer.iter) for e in eb.estimators_],
                                   pair_steps=[int(e.optimizer.steps) for e in eb.estimators_],
                                   n_sv=[int(len(e.support_)) for e in eb.estimators_])
    print('pass %d: OneVsRestSVC.fit batched %.3f s, per class %.3f s, same bits %s' % (rep, tb, tp, same), flush=True)

yb = np.where(y == 0, 1., -1.)
for rep in range(2):
    t_panel, quad = clock(lambda: (lambda q: (q.device_problem(), q)[1])(
        KernelQuadratic(X, -np.ones(n), 'svc', kernel, y=yb, rank_one=False, compact=False)))
    t_single, one = clock(lambda: SMOClassifier(quad, X, yb, None, kernel, 1., 1e-3).minimize())
    cols = {}
    for k in (1, 2, 4, 8, 16, 64, 256, 512):
        t, res = clock(lambda: solve_batched_smo(quad.device_problem(), _lib.SVC, np.stack([yb] * k), 1., None, 1e-3))
        cols[str(k)] = dict(batched_solve_s=t, k_single_fits_s=k * t_single, k_single_fits_with_panels_s=k * (t_single + t_panel),
                            same_bits=bool(all(np.array_equal(r['alphas'], one.alphas) for r in res)))
        print('pass %d: k = %3d: batched %.3f s, k single fits %.3f s (+ k panels: %.3f s)' %
              (rep, k, t, k * t_single, k * (t_single + t_panel)), flush=True)
    rec['columns_pass%d' % rep] = dict(panel_build_s=t_panel, single_fit_s=t_single, outer_iterations=int(one.iter),
                                       pair_steps=int(one.steps), helpers=one.helper_stats['helpers'], by_k=cols)
    quad.release()

if len(sys.argv) > 4:
    with open(sys.argv[4], 'w') as fh:
        json.dump(rec, fh, indent=1)
print(json.dumps(rec, indent=1))
