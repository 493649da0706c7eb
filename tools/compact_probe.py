"""Compact fp64 panel probe (csrc/bq_c7.h): the symmetric panel product on the plain 8-byte layout (hook compact_panel=0) and on the
compact 7-byte layout, in one process, at the headline shape (RBF SVC, make_blobs, gamma='scale', fp64).

    python tools/compact_probe.py [--n 100000] [--d 128] [--reps 20] [--rounds 3] [--out FILE]

One problem per layout at a time (two 40 GB panels do not fit together), `rounds` alternations of plain and compact.  Per round:
the Gram build (wall time of the problem's creation), the mean product time over `reps` launches (bq_problem_time_matvec: the
local product alone, no solver), the panel bytes the layout streams, and the read rate on those bytes.  Also checks that the two
layouts give the same product bits.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=100000)
    ap.add_argument('--d', type=int, default=128)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    from optiml_amd import _lib
    from optiml_amd.datasets import make_blobs
    from optiml_amd.device import get_context
    from optiml_amd.ml.svm.kernels import gaussian
    from optiml_amd.opti import KernelQuadratic
    _lib.load()
    get_context()
    X, y = make_blobs(a.n, a.d, seed=0)
    v = np.random.RandomState(2).standard_normal(a.n)
    base_hooks = os.environ.get('BQ_TEST_HOOKS', '')
    rows, ref = [], {}
    for r in range(a.rounds):
        for layout in ('plain', 'compact'):
            os.environ['BQ_TEST_HOOKS'] = ','.join(h for h in (base_hooks, 'compact_panel=0' if layout == 'plain' else '') if h)
            t0 = time.perf_counter()
            quad = KernelQuadratic(X, -np.ones(a.n), 'svc', gaussian, y=y)
            dev = quad.device_problem()
            build_s = time.perf_counter() - t0
            nbytes = dev.layout()['panel_bytes']
            out = dev.matvec(v)
            same = bool(np.array_equal(out, ref.setdefault('matvec', out)))
            ms = dev.time_matvec(a.reps)
            rows.append({'round': r, 'layout': layout, 'panel_bytes': nbytes, 'create_s': round(build_s, 4), 'product_ms': round(ms, 4),
                         'panel_tb_s': round(nbytes / (ms * 1e-3) / 1e12, 3), 'matvec_equal_first': same})
            print(json.dumps(rows[-1]), flush=True)
            quad.release()
    os.environ['BQ_TEST_HOOKS'] = base_hooks
    med = {k: float(np.median([r['product_ms'] for r in rows if r['layout'] == k])) for k in ('plain', 'compact')}
    res = {'n': a.n, 'd': a.d, 'reps': a.reps, 'rows': rows, 'median_product_ms': med,
           'speedup': round(med['plain'] / med['compact'], 4), 'all_equal': all(r['matvec_equal_first'] for r in rows)}
    print(json.dumps({k: res[k] for k in ('median_product_ms', 'speedup', 'all_equal')}))
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
