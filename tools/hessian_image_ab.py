#!/usr/bin/env python3
"""Helpers of tools/profile_hessian_image.sh (profiles/hessian_image/):

    hessian_image_ab.py collate OUTDIR            the bench lines <step>_<build>_<k>.json of OUTDIR -> headline_ab.json, c2_ab.json, c4_ab.json, c5_ab.json
    hessian_image_ab.py fetch CSV OUT.json        rocprofv3 --pmc FETCH_SIZE counter_collection.csv -> bytes per launch of every kernel
    hessian_image_ab.py setup CONFIG...           builds bench.py's problem of each config, creates a ProjectedGradient solver and prints the
                                                  image's state, build time, candidates' times and the break-even product count (GPU)
"""
import csv
import glob
import json
import os
import statistics
import sys
from collections import defaultdict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BYTES_PREDICTION = 6.5 / 7.0   # tile bytes of the image over tile bytes of the compact panel


def _line(path):
    rows = [l for l in open(path).read().splitlines() if l.strip().startswith('{')]
    return json.loads(rows[-1])


def collate(out):
    for step, name in (('headline_ab', 'headline_ab'), ('c2_ab', 'c2_ab'), ('c4', 'c4_ab'), ('c5', 'c5_ab')):
        runs, side = [], {'parent': defaultdict(list), 'image': defaultdict(list)}
        files = sorted(glob.glob(os.path.join(out, f'{step}_*_[0-9].json')), key=lambda p: (p[-6], 'image' in os.path.basename(p)))
        for order, path in enumerate(files, 1):
            rec = _line(path)
            build = 'image' if '_image_' in os.path.basename(path) else 'parent'
            row = {'order': order, 'build': build, 'value': rec['value'], 'avg_launch_ms': rec['roofline']['avg_launch_ms'],
                   'problem_setup_s': rec.get('problem_setup_s'), 'frac': rec['roofline'].get('frac'),
                   'panel_placement_ms': rec['config'].get('panel_placement_ms')}
            runs.append(row)
            for k in ('value', 'avg_launch_ms', 'problem_setup_s'):
                side[build][k].append(row[k])
        if not runs:
            continue
        p, i = side['parent'], side['image']
        res = {'command': runs and f"python bench.py --gpus 1 --steps 50 --warmup 5{'' if step == 'headline_ab' else ' --config ' + step[:2]}, "
                                   'fresh processes alternating parent, image', 'runs': runs, 'parent': p, 'image': i}
        if p['value'] and i['value']:
            res['every_image_launch_below_every_parent'] = max(i['avg_launch_ms']) < min(p['avg_launch_ms'])
            res['every_image_value_above_every_parent'] = min(i['value']) > max(p['value'])
            res['median_launch_ratio'] = statistics.median(i['avg_launch_ms']) / statistics.median(p['avg_launch_ms'])
            res['median_value_ratio'] = statistics.median(i['value']) / statistics.median(p['value'])
            res['bytes_prediction_launch_ratio'] = 32.66 / 35.17
        json.dump(res, open(os.path.join(out, name + '.json'), 'w'), indent=1)
        print(name, {k: res.get(k) for k in ('every_image_launch_below_every_parent', 'every_image_value_above_every_parent',
                                              'median_launch_ratio', 'median_value_ratio')}, dict(p), dict(i))


def fetch(path, dst):
    acc = defaultdict(list)
    with open(path, newline='') as fh:
        for row in csv.DictReader(fh):
            if row['Counter_Name'] == 'FETCH_SIZE':
                acc[row['Kernel_Name'].split('(')[0].replace('void ', '')].append(float(row['Counter_Value']))
    out = {'units': 'FETCH_SIZE as the counter gives it (KiB), mean over launches; bytes = KiB x 1024, and x 2 with the gfx950 '
                    'wide-read correction tools/pmc_summary.py applies', 'kernels': {}}
    for k, v in sorted(acc.items(), key=lambda kv: -sum(kv[1])):
        mean = sum(v) / len(v)
        out['kernels'][k] = {'launches': len(v), 'fetch_size_kib_raw': mean, 'bytes_raw': mean * 1024.0, 'bytes_corrected_x2': mean * 2048.0}
    json.dump(out, open(dst, 'w'), indent=1)
    for k, v in list(out['kernels'].items())[:4]:
        print(f"{k[:80]:80s} {v['bytes_corrected_x2'] / 1e9:9.3f} GB/launch x{v['launches']}")


def setup(configs):
    sys.path.insert(0, ROOT)
    import numpy as np
    import bench
    from optiml_amd import _lib, device
    from optiml_amd.datasets import make_blobs
    from optiml_amd.ml.svm.kernels import gaussian
    from optiml_amd.opti import KernelQuadratic
    from optiml_amd.opti.constrained._base import _DeviceSolver
    res = {}
    for name in configs:
        cfg = bench.CONFIGS[name]
        n, d = cfg['n'], cfg['d']
        X, y = make_blobs(n, d, seed=0, sigma=8.0)
        quad = KernelQuadratic(X, -np.ones(n), 'svc', gaussian, y=y, tune_placement=True, expected_products=bench.STEADY_STATE_PRODUCTS)
        dev = quad.device_problem(device.get_context())
        import time
        t0 = time.perf_counter()
        solver = _DeviceSolver(dev, _lib.PG, np.zeros(n), np.ones(n), np.full(n, 0.5), 1e-6, 10 ** 9)
        t_solver = time.perf_counter() - t0
        img, placed = dev.hessian_image(), dev.placement()
        t_panel = dev.time_matvec(10)   # the tile kernel + closing kernel on the PANEL (this entry never reads the image)
        ctx = device.get_context()
        solver.run(5)
        ctx.profile(True)
        ctx.profile_read(_lib.PROF_MATVEC, reset=True)
        solver.run(25)
        ms, cnt = ctx.profile_read(_lib.PROF_MATVEC, reset=True)
        ctx.profile(False)
        t_tiles = ms / max(cnt, 1)      # the tile kernel as the solver launches it: on the image when it is built
        rec = {'n': n, 'd': d, 'panel_bytes': dev.layout()['panel_bytes'], 'panel_placement_ms': placed, 'image': img,
               'solver_create_s (image allocation, candidates, conversion)': t_solver,
               'panel_product_ms (tile + closing kernel, time_matvec)': t_panel, 'solver_tile_kernel_ms': t_tiles}
        if img['state'] == 'built' and placed:
            # the saving per product as measured here (the panel's tile kernel as the placement choice timed it, closing kernel
            # included, against the solver's tile kernel) and as the rule of bq_hessian_image_ensure prices it
            rec['break_even_products_rule'] = 1e3 * t_solver / ((1 - BYTES_PREDICTION) * min(placed))
        res[name] = rec
        solver.close()
        quad.release()
    print(json.dumps(res, indent=1))


if __name__ == '__main__':
    if sys.argv[1] == 'collate':
        collate(sys.argv[2])
    elif sys.argv[1] == 'fetch':
        fetch(sys.argv[2], sys.argv[3])
    else:
        setup(sys.argv[2:])
