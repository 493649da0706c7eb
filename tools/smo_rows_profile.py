#!/usr/bin/env python3
"""Measure the row-based SMO (SVC(optimizer='smo', storage='stream'), bq_rsmo_*) on the shape of bench.py's headline data (two blobs,
RBF with gamma='scale', d = 128, C = 1, tol 1e-3, seed 0) and write profiles/smo_rows/README.md plus the raw JSON records.

    python tools/smo_rows_profile.py all [--out profiles/smo_rows] [--sizes a,b,c]
        (a) n = 100 000: the fit with storage 'stream' against 'f64' (the resident walker; the two solvers read tol differently,
            so both objectives are recorded), and one rocprofv3 --kernel-trace --stats run of the streamed fit for the row kernels
        (b) n = 400 000: the streamed fit, and the streamed product (one ProjectedGradient iteration's cost) measured again
        (c) n = 1 000 000: the fit if it ends inside its time limit, else the step rate over a fixed window
    python tools/smo_rows_profile.py fit --n N --storage stream|f64 --json FILE      one fit in this (fresh) process
    python tools/smo_rows_profile.py rate --n N --steps K --json FILE                K steps of the streamed solver, no verdict
    python tools/smo_rows_profile.py product --n N --json FILE                       the streamed Gram product, timed
    python tools/smo_rows_profile.py stages --n N --reps R --json FILE               R fits in one process, problem build and minimize apart
    python tools/smo_rows_profile.py nu-all [--out profiles/smo_nu_rows] [--sizes a,b]
        RowOneClassSVM (nu = 0.1) and RowNuSVC (nu = 0.2) on the same blobs: at a = 100 000 beside the resident OneClassSVM / NuSVC
        at the same tol, at b = 400 000 beside one streamed product
    python tools/smo_rows_profile.py nu-fit --model oneclass|nusvc --route rows|resident --n N --json FILE   one such fit

Every measurement runs in a process of its own under its own time limit, after a warm-up fit of n = 4000 on the same route; a wall
time ends after the solver's last read-back, which synchronises the stream."""
import argparse
import glob
import json
import os
import sqlite3
import subprocess
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
D, SIGMA, TOL = 128, 8.0, 1e-3


def _svc(storage):
    from optiml_amd.ml.svm import SVC
    from optiml_amd.ml.svm.kernels import gaussian
    from optiml_amd.ml.svm.losses import hinge
    return SVC(loss=hinge, kernel=gaussian, C=1., dual=True, optimizer='smo', tol=TOL, storage=storage)


def _data(n):
    from optiml_amd.datasets import make_blobs
    return make_blobs(n, D, seed=0, sigma=SIGMA)


def _image_bytes(n):
    return 8 * D * (-(-n // 128) * 128)   # one pass over the k-major image: d x padded n doubles


def cmd_fit(args):
    from optiml_amd.device import get_context
    Xw, yw = _data(4000)
    _svc(args.storage).fit(Xw, yw).obj.release()
    X, y = _data(args.n)
    t0 = time.perf_counter()
    est = _svc(args.storage).fit(X, y)
    wall = time.perf_counter() - t0
    opt = est.optimizer
    rec = {'what': 'fit', 'n': args.n, 'd': D, 'storage': args.storage, 'tol': TOL, 'wall_s': wall, 'n_sv': int(len(est.support_)),
           'includes': 'problem build (image or panel) + solve + read-back'}
    if args.storage == 'stream':
        st = opt.cache_stats
        rec.update(steps=int(opt.iter), status=opt.status, per_step_us=1e6 * wall / max(opt.iter, 1), objective=opt.objective(),
                   hits=st['hits'], misses=st['misses'], cache_rows=st['cache_rows'], hit_rate=st['hits'] / max(st['hits'] + st['misses'], 1),
                   gmax_plus_gmax2=float(opt.gmax + opt.gmax2), image_bytes_per_row=_image_bytes(args.n))
        if not args.no_probe:
            rec['read_GBs'] = get_context().probe_bandwidth()[0]
    else:
        yb = np.where(y == np.unique(y)[-1], 1., -1.)
        rec.update(steps=int(opt.steps), outer_iterations=int(opt.iter), per_step_us=1e6 * wall / max(opt.steps, 1),
                   objective=float(est.obj.function(est.alphas_)), b_up_minus_b_low=float(opt.b_up - opt.b_low), labels_checksum=float(yb.sum()))
    est.obj.release()
    json.dump(rec, open(args.json, 'w'), indent=1)
    print(json.dumps(rec))


def cmd_rate(args):
    import ctypes as C
    from optiml_amd import _lib
    from optiml_amd.ml.svm.kernels import gaussian
    from optiml_amd.opti import KernelQuadratic
    lib = _lib.load()
    X, y = _data(args.n)
    t0 = time.perf_counter()
    quad = KernelQuadratic(X, -np.ones(args.n), 'svc', gaussian, y=y, storage='stream', rank_one=False)
    h = C.c_void_p()
    dev = quad.device_problem()
    problem = time.perf_counter() - t0
    _lib.check(lib.bq_rsmo_create(dev.handle, _lib.SVC, _lib.ptr(y), _lib.ptr(np.ones(args.n)), 0.0, TOL, args.cache_rows, C.byref(h)))
    build = time.perf_counter() - t0
    steps, fin = C.c_int64(0), C.c_int(0)
    _lib.check(lib.bq_rsmo_run(h, 64, C.byref(steps), C.byref(fin)))   # warm
    first = steps.value
    t0 = time.perf_counter()
    while steps.value - first < args.steps and not fin.value:
        _lib.check(lib.bq_rsmo_run(h, 512, C.byref(steps), C.byref(fin)))
    wall = time.perf_counter() - t0
    st, sc = np.empty(3), np.empty(6)
    _lib.check(lib.bq_rsmo_get(h, _lib.RSMO_STATS, _lib.ptr(st)))
    _lib.check(lib.bq_rsmo_get(h, _lib.RSMO_SCALARS, _lib.ptr(sc)))
    t0 = time.perf_counter()
    lib.bq_rsmo_destroy(h)
    destroy = time.perf_counter() - t0
    rec = {'what': 'rate (NOT a fit)', 'n': args.n, 'd': D, 'build_s': build, 'problem_s': problem, 'solver_create_s': build - problem,
           'solver_destroy_s': destroy, 'window_steps': int(steps.value - first), 'window_s': wall,
           'per_step_us': 1e6 * wall / max(steps.value - first, 1), 'finished': int(fin.value), 'gmax_plus_gmax2': float(sc[1] + sc[2]),
           'hits': int(st[0]), 'misses': int(st[1]), 'cache_rows': int(st[2]), 'image_bytes_per_row': _image_bytes(args.n)}
    json.dump(rec, open(args.json, 'w'), indent=1)
    print(json.dumps(rec))


def cmd_stages(args):
    """the same streamed fit `--reps` times in one process: the whole fit, and inside it building the problem and `minimize` (solver
    create, steps, read-back, destroy)"""
    from optiml_amd.ml.svm import smo_rows
    from optiml_amd.opti import KernelQuadratic
    spent = {}

    def timed(cls, name, key):
        inner = getattr(cls, name)

        def outer(*a, **k):
            t0 = time.perf_counter()
            try:
                return inner(*a, **k)
            finally:
                spent[key] = time.perf_counter() - t0
        setattr(cls, name, outer)
    timed(KernelQuadratic, '_build_problem', 'build_problem_s')
    timed(smo_rows.RowSMO, 'minimize', 'minimize_s')
    Xw, yw = _data(4000)
    _svc('stream').fit(Xw, yw).obj.release()
    X, y = _data(args.n)
    rec = {'what': 'stages of repeated fits in one process', 'n': args.n, 'd': D, 'fits': []}
    for _ in range(args.reps):
        spent.clear()
        t0 = time.perf_counter()
        est = _svc('stream').fit(X, y)
        rec['fits'].append(dict(spent, fit_s=time.perf_counter() - t0, steps=int(est.optimizer.iter)))
        est.obj.release()
    json.dump(rec, open(args.json, 'w'), indent=1)
    print(json.dumps(rec))


def cmd_product(args):
    from optiml_amd.ml.svm.kernels import gaussian
    from optiml_amd.opti import KernelQuadratic
    X, y = _data(args.n)
    quad = KernelQuadratic(X, -np.ones(args.n), 'svc', gaussian, y=y, storage='stream')
    ms = quad.device_problem().time_matvec(3)
    rec = {'what': 'streamed product (one ProjectedGradient iteration is one product)', 'n': args.n, 'd': D, 'product_s': ms / 1e3}
    json.dump(rec, open(args.json, 'w'), indent=1)
    print(json.dumps(rec))


NU = {'oneclass': 0.1, 'nusvc': 0.2}


def _nu_model(model, route):
    from optiml_amd.ml.svm import NuSVC, OneClassSVM, RowNuSVC, RowOneClassSVM
    from optiml_amd.ml.svm.kernels import gaussian
    if route == 'rows':
        return (RowOneClassSVM if model == 'oneclass' else RowNuSVC)(kernel=gaussian, nu=NU[model], tol=TOL)
    return (OneClassSVM if model == 'oneclass' else NuSVC)(kernel=gaussian, nu=NU[model], tol=TOL, max_iter=100000, storage='f64')


def cmd_nu_fit(args):
    """one fit of a nu-family model in this (fresh) process after a warm-up fit of n = 4000 on the same route; on the row route
    also the streamed product of the same data — the start gradient of these duals is one such product"""
    from optiml_amd.opti import KernelQuadratic
    fit = (lambda m, X, y: m.fit(X)) if args.model == 'oneclass' else (lambda m, X, y: m.fit(X, y))
    fit(_nu_model(args.model, args.route), *_data(4000))
    X, y = _data(args.n)
    t0 = time.perf_counter()
    est = fit(_nu_model(args.model, args.route), X, y)
    wall = time.perf_counter() - t0
    rec = {'what': 'nu fit', 'model': type(est).__name__, 'nu': NU[args.model], 'n': args.n, 'd': D, 'route': args.route, 'tol': TOL,
           'wall_s': wall, 'steps': int(est.n_iter_), 'status': est.status_, 'n_sv': int(len(est.support_)),
           'kkt_violation': float(est.kkt_violation_), 'per_step_us': 1e6 * wall / max(int(est.n_iter_), 1),
           'includes': 'problem build (image or panel) + start + solve + read-back',
           'steps_are': 'pair updates' if args.route == 'rows' else 'projected-gradient iterations (one panel product each)'}
    if args.route == 'rows':
        st = est.cache_stats_
        rec.update(hits=st['hits'], misses=st['misses'], cache_rows=st['cache_rows'], hit_rate=st['hits'] / max(st['hits'] + st['misses'], 1),
                   image_bytes_per_row=_image_bytes(args.n))
        quad = KernelQuadratic(X, np.zeros(args.n), 'plain', est.kernel_, storage='stream')
        rec['start_product_s'] = quad.device_problem().time_matvec(3) / 1e3
        quad.release()
    json.dump(rec, open(args.json, 'w'), indent=1)
    print(json.dumps(rec))


def cmd_nu_all(args):
    out = os.path.join(REPO, args.out)
    os.makedirs(out, exist_ok=True)
    a, b = (int(v) for v in args.sizes.split(','))
    # a step that fails or runs into its limit ends the job: nothing more is started on the device after it
    plan = [('%s_%s_%s' % (tag, model, route), ['nu-fit', '--model', model, '--route', route, '--n', str(n)])
            for tag, n, route in (('a', a, 'rows'), ('b', b, 'rows'), ('a', a, 'resident')) for model in ('oneclass', 'nusvc')]
    have = os.path.join(out, 'records.json')   # records of an earlier call with the same --out are kept: the job may be cut in two
    R = {k: v for k, v in json.load(open(have)).items() if 'failed' not in v} if os.path.exists(have) else {}
    for name, argv in plan:
        if name in args.skip.split(',') or name in R:
            continue
        R[name] = _child(out, name, argv, args.fit_limit)
        _write_nu(out, R, (a, b))
        if 'failed' in R[name]:
            break


def _write_nu(out, R, sizes):
    json.dump(R, open(os.path.join(out, 'records.json'), 'w'), indent=1)
    lines = ['# Row-based one-class SVM and nu-SVC: measurements', '',
             'Written by `tools/smo_rows_profile.py nu-all` (sizes %s): bench.py\'s headline blobs (d = 128, RBF with gamma = \'scale\'), '
             'tol 1e-3, each fit in a fresh process warmed by an n = 4 000 fit; raw records: `records.json` and one JSON per measurement.  '
             'Steps of the row route are pair updates, of the resident route projected-gradient iterations: only the wall times compare.  '
             '`start product` is one streamed Gram product of the same data, timed apart (the start gradient is one such product).'
             % (sizes,), '',
             '| record | model | n | steps | status | wall s | start product s | us / step | hit rate | support vectors | note |',
             '|---|---|---|---|---|---|---|---|---|---|---|']
    for name, r in R.items():
        fmt = lambda key, f: f % r[key] if key in r else ''
        lines.append('| %s | %s | %s | %s | %s | %s | %s | %s | %s | %s | %s |' % (
            name, r.get('model', ''), r.get('n', ''), r.get('steps', ''), r.get('status', ''), fmt('wall_s', '%.3f'),
            fmt('start_product_s', '%.4f'), fmt('per_step_us', '%.1f'), fmt('hit_rate', '%.3f'), r.get('n_sv', ''),
            r.get('failed') or r.get('steps_are', '')))
    open(os.path.join(out, 'README.md'), 'w').write('\n'.join(lines) + '\n')


def _row_kernel_stats(trace_dir):
    """per kernel of bq_rsmo.hip: all launches, and those that computed a row (a launch on a hit only reads the cache: the two
    populations are split at the midpoint of the 10th and 99th percentile)"""
    dbs = glob.glob(os.path.join(trace_dir, '**', '*_results.db'), recursive=True)
    if not dbs:
        return None
    cur = sqlite3.connect(dbs[0]).cursor()
    out = {}
    for key in ('rsmo_select_kernel', 'rsmo_update_kernel'):
        d = np.array([r[0] for r in cur.execute('select duration from kernels where name like ?', ('%' + key + '%',))], dtype=float)
        if not len(d):
            continue
        cut = 0.5 * (np.percentile(d, 10) + np.percentile(d, 99))
        big = d[d >= cut]
        out[key] = {'launches': int(len(d)), 'total_ms': float(d.sum() / 1e6), 'median_us': float(np.median(d) / 1e3),
                    'row_launches': int(len(big)), 'row_mean_us': float(big.mean() / 1e3) if len(big) else None,
                    'cache_only_mean_us': float(d[d < cut].mean() / 1e3) if (d < cut).any() else None}
    return out


def _child(out, name, argv, limit, pre=()):
    path = os.path.join(out, name + '.json')
    cmd = list(pre) + [sys.executable, os.path.abspath(__file__)] + argv + ['--json', path]
    t0 = time.perf_counter()
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=limit, cwd=REPO)
        ok = r.returncode == 0 and os.path.exists(path)
        note = None if ok else 'rc=%d: %s' % (r.returncode, r.stderr[-400:])
    except subprocess.TimeoutExpired:
        ok, note = False, 'did not end inside its %d s limit' % limit
    print('[%s] %s in %.1f s' % (name, 'ok' if ok else note, time.perf_counter() - t0), flush=True)
    return json.load(open(path)) if ok else {'what': name, 'failed': note}


def cmd_all(args):
    out = os.path.join(REPO, args.out)
    os.makedirs(out, exist_ok=True)
    a, b, c = (int(v) for v in args.sizes.split(','))
    trace = tempfile.mkdtemp(prefix='smo_rows_trace_')   # the tracer's database: read here, never kept
    # bounded windows first, whole fits of unknown length last; a step that fails or runs into its limit ends the job: nothing more
    # is started on the device after it
    plan = [('a_stream', ['fit', '--n', str(a), '--storage', 'stream'], 240, ()),
            ('a_f64', ['fit', '--n', str(a), '--storage', 'f64'], 240, ()),
            ('b_product', ['product', '--n', str(b)], 240, ()),
            ('b_rate', ['rate', '--n', str(b), '--steps', '20000'], 240, ()),
            ('c_rate', ['rate', '--n', str(c), '--steps', '10000'], 300, ()),
            ('a_traced', ['fit', '--n', str(a), '--storage', 'stream', '--no-probe'], 360,
             ('rocprofv3', '--kernel-trace', '--stats', '-d', trace, '--')),
            ('b_stream', ['fit', '--n', str(b), '--storage', 'stream'], args.fit_limit, ()),
            ('c_stream', ['fit', '--n', str(c), '--storage', 'stream'], args.fit_limit, ())]
    R = {}
    for name, argv, limit, pre in plan:
        if name in args.skip.split(','):
            continue
        R[name] = _child(out, name, argv, limit, pre)
        if name == 'a_traced':
            R['a_kernels'] = _row_kernel_stats(trace)
            json.dump(R['a_kernels'], open(os.path.join(out, 'a_kernels.json'), 'w'), indent=1)
        _write(out, R, (a, b, c))
        if 'failed' in R[name]:
            break


def _write(out, R, sizes):
    json.dump(R, open(os.path.join(out, 'records.json'), 'w'), indent=1)
    lines = ['# Row-based SMO: measurements', '', 'Written by `tools/smo_rows_profile.py all` (sizes %s); raw records: `records.json` '
             'and one JSON per measurement.' % (sizes,), '', '| record | n | steps | wall s | us / step | hit rate | objective | note |',
             '|---|---|---|---|---|---|---|---|']
    for name, r in R.items():
        if not isinstance(r, dict) or 'what' not in r:
            continue
        steps = r.get('steps', r.get('window_steps'))
        wall = r.get('wall_s', r.get('window_s', r.get('product_s')))
        hr = r.get('hit_rate', (r['hits'] / max(r['hits'] + r['misses'], 1)) if 'hits' in r else None)
        lines.append('| %s | %s | %s | %s | %s | %s | %s | %s |' % (
            name, r.get('n'), steps, '%.3f' % wall if wall is not None else '', '%.1f' % r['per_step_us'] if 'per_step_us' in r else '',
            '%.3f' % hr if hr is not None else '', '%.9g' % r['objective'] if 'objective' in r else '', r.get('failed') or r['what']))
    k = R.get('a_kernels')
    if k:
        lines += ['', '## Row kernels at (a), from one rocprofv3 --kernel-trace --stats run', '',
                  '| kernel | launches | launches that computed a row | mean us of those | mean us on a hit | image GB/s of those |', '|---|---|---|---|---|---|']
        for name, s in k.items():
            gbs = _image_bytes(sizes[0]) / (s['row_mean_us'] * 1e-6) / 1e9 if s['row_mean_us'] else None
            lines.append('| %s | %d | %d | %s | %s | %s |' % (name, s['launches'], s['row_launches'], s['row_mean_us'], s['cache_only_mean_us'],
                                                         '%.0f' % gbs if gbs else ''))
    open(os.path.join(out, 'README.md'), 'w').write('\n'.join(lines) + '\n')


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest='cmd', required=True)
    p = sub.add_parser('all')
    p.add_argument('--out', default='profiles/smo_rows')
    p.add_argument('--sizes', default='100000,400000,1000000')
    p.add_argument('--fit-limit', type=int, default=360, help='time limit of the whole fits at (b) and (c), seconds')
    p.add_argument('--skip', default='', help='records to leave out, comma-separated')
    p.set_defaults(fn=cmd_all)
    p = sub.add_parser('fit')
    p.add_argument('--n', type=int, required=True)
    p.add_argument('--storage', default='stream', choices=['stream', 'f64'])
    p.add_argument('--no-probe', action='store_true')
    p.add_argument('--json', required=True)
    p.set_defaults(fn=cmd_fit)
    p = sub.add_parser('rate')
    p.add_argument('--n', type=int, required=True)
    p.add_argument('--steps', type=int, default=10000)
    p.add_argument('--cache-rows', type=int, default=0)
    p.add_argument('--json', required=True)
    p.set_defaults(fn=cmd_rate)
    p = sub.add_parser('stages')
    p.add_argument('--n', type=int, required=True)
    p.add_argument('--reps', type=int, default=3)
    p.add_argument('--json', required=True)
    p.set_defaults(fn=cmd_stages)
    p = sub.add_parser('nu-all')
    p.add_argument('--out', default='profiles/smo_nu_rows')
    p.add_argument('--sizes', default='100000,400000')
    p.add_argument('--fit-limit', type=int, default=300, help='time limit of each fit, seconds')
    p.add_argument('--skip', default='', help='records to leave out, comma-separated')
    p.set_defaults(fn=cmd_nu_all)
    p = sub.add_parser('nu-fit')
    p.add_argument('--model', required=True, choices=['oneclass', 'nusvc'])
    p.add_argument('--route', default='rows', choices=['rows', 'resident'])
    p.add_argument('--n', type=int, required=True)
    p.add_argument('--json', required=True)
    p.set_defaults(fn=cmd_nu_fit)
    p = sub.add_parser('product')
    p.add_argument('--n', type=int, required=True)
    p.add_argument('--json', required=True)
    p.set_defaults(fn=cmd_product)
    args = ap.parse_args()
    args.fn(args)


if __name__ == '__main__':
    main()
