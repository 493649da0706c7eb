#!/usr/bin/env python3
"""One run per flavour of the SMO walker (csrc/bq_smo.hip: smo_kernel, smo_batch_kernel) at the smallest shapes that reach its
edges, and a SHA-256 of everything a column produces: multipliers, error cache, the six scalars, outer iterations, pair steps and
finished / failed.  Two builds of the library that print the same file compute the same bits:

    python3 tools/smo_flavours.py [path/to/libbcqp_hip.so] > flavours.txt

n = 300 (two 256-row tiles, the second ragged), k = 5 columns with different C (and epsilon).  Classification and regression; the
single solver (with the helper workgroups at their default, at smo_helpers = 16 and without) and the batched one (with and without
row lists); the scalar box and one box per row; the packed fp64 panel, the square fp64 panel, the fp32 panel and the compact 7-byte
panel (scalar box only: row boxes are refused there).  Every run is cut into calls of two outer iterations, so the batched columns
finish at different launches (the printed counts).
"""
import ctypes as C
import hashlib
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from optiml_amd import _lib  # noqa: E402

if len(sys.argv) > 1:
    _lib.LIB_PATH = os.path.abspath(sys.argv[1])   # as tools/bench_with_lib.py

from optiml_amd.ml.svm._batched import _DeviceSMOSolver  # noqa: E402
from optiml_amd.ml.svm.kernels import GaussianKernel  # noqa: E402
from optiml_amd.opti import KernelQuadratic  # noqa: E402

N, D, K = 300, 6, 5
CS = np.array([0.1, 0.3, 1., 3., 10.])
EPS = np.array([0.05, 0.1, 0.2, 0., 0.3])
TOL = 1e-3
PIECE = 2   # outer iterations per *_run call
warnings.simplefilter('ignore')


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def show(name, **arrays):
    for key, a in arrays.items():
        print('%-44s %-10s %s' % (name, key, sha(a)))


def data(task):
    rs = np.random.RandomState(5)
    X = rs.standard_normal((N, D))
    W = rs.standard_normal((D, K))
    if task == _lib.SVC:
        Y = np.where(X @ W + 0.5 * rs.standard_normal((N, K)) > 0, 1., -1.).T.copy()
    else:
        Y = (np.sin(X @ W) + 0.3 * rs.standard_normal((N, K))).T.copy()
    # one box per row: a column's C scaled by 1/2, 1 or 2 from row to row
    return X, Y, CS[:, None] * np.array([0.5, 1., 2.])[np.arange(N) % 3][None, :]


def gamma_of(X, panel):
    if panel == 'compact':   # exp(-4 gamma max|x|^2) >= 2^-14: eligible for the 7-byte layout (tests/smo_list_reference.py)
        return 0.9 * 14 * np.log(2) / (4 * (X * X).sum(axis=1).max())
    return 1.0 / (X.shape[1] * X.var())


PANELS = {'packed': dict(compact=False), 'square': dict(compact=False, full_panel=True), 'f32': dict(storage='f32'),
          'compact': dict(compact=True)}
BYTES = {'packed': 8, 'f32': 4, 'compact': 7}


def quad_of(task, X, y, panel):
    kern = GaussianKernel(gamma=gamma_of(X, panel))
    if task == _lib.SVC:
        quad = KernelQuadratic(X, -np.ones(N), 'svc', kern, y=y, rank_one=False, **PANELS[panel])
    else:
        quad = KernelQuadratic(X, np.hstack((-y, y)) + 0.1, 'svr', kern, rank_one=False, **PANELS[panel])
    if panel in BYTES:
        assert quad.device_problem().layout()['panel_bytes'] == 3 * 65536 * BYTES[panel], panel
    return quad


def single(name, quad, task, y, Cv, Cw, eps):
    lib = _lib.load()
    h = C.c_void_p()
    y = np.ascontiguousarray(y)
    if Cw is None:
        _lib.check(lib.bq_smo_create(quad.device_problem().handle, task, _lib.ptr(y), float(Cv), float(eps), TOL, C.byref(h)))
    else:
        Cw = np.ascontiguousarray(Cw)
        _lib.check(lib.bq_smo_create_weighted(quad.device_problem().handle, task, _lib.ptr(y), _lib.ptr(Cw), float(eps), TOL,
                                              C.byref(h)))
    outer, fin = C.c_int64(0), C.c_int(0)
    trace = []
    try:
        while not fin.value:
            _lib.check(lib.bq_smo_run(h, PIECE, C.byref(outer), C.byref(fin)))
            sc = np.empty(6)
            _lib.check(lib.bq_smo_get(h, _lib.SMO_SCALARS, _lib.ptr(sc)))
            trace.append(np.concatenate((sc, [outer.value, fin.value])))
        a, err, st = np.empty(N * (2 if task == _lib.SVR else 1)), np.empty(N), np.empty(4)
        _lib.check(lib.bq_smo_get(h, _lib.SMO_ALPHAS, _lib.ptr(a)))
        _lib.check(lib.bq_smo_get(h, _lib.SMO_ERRORS, _lib.ptr(err)))
        _lib.check(lib.bq_smo_get(h, _lib.SMO_STATS, _lib.ptr(st)))
    finally:
        lib.bq_smo_destroy(h)
    assert st[2] == 0 and st[3] == 0, st   # rejected sums: must stay 0
    show(name, alphas=a, errors=err, scalars=trace[-1][:6], trace=np.stack(trace),
         state=np.array([outer.value, int(trace[-1][4]), fin.value]))
    print('%-44s %-10s outer %d steps %d helpers %d' % (name, 'counts', outer.value, int(trace[-1][4]), int(st[0])))


def batched(name, quad, task, Y, eps, rows, boxes):
    s = _DeviceSMOSolver(quad.device_problem(), task, Y, CS, eps, TOL, rows=rows, boxes=boxes)
    trace = []
    try:
        fin = np.zeros(K, dtype=bool)
        while not fin.all():
            outer, fin, failed = s.run(PIECE)
            trace.append(np.concatenate([np.concatenate((s.get(c, _lib.SMO_SCALARS), [outer[c], fin[c], failed[c]])) for c in range(K)]))
        for c in range(K):
            sc = s.get(c, _lib.SMO_SCALARS)
            show('%s[%d]' % (name, c), alphas=s.get(c, _lib.SMO_ALPHAS), errors=s.get(c, _lib.SMO_ERRORS), scalars=sc,
                 state=np.array([outer[c], int(sc[4]), int(fin[c]), int(failed[c])]))
        show(name, trace=np.stack(trace))
        print('%-44s %-10s outer %s calls %d' % (name, 'counts', [int(o) for o in outer], len(trace)))
    finally:
        s.close()


def flavours(task, tname):
    X, Y, CW = data(task)
    eps = None if task == _lib.SVC else EPS
    idx = np.arange(N)
    rows = [np.setdiff1d(idx, idx[c::4]) for c in range(4)] + [idx]   # four folds' training rows, and the identity list
    for panel in PANELS:
        quad = quad_of(task, X, Y[0], panel)
        e1 = 0.0 if eps is None else eps[1]
        for helpers in ((None, '16', '0') if panel == 'packed' else (None,)):
            if helpers is None:
                os.environ.pop('BQ_TEST_HOOKS', None)
            else:
                os.environ['BQ_TEST_HOOKS'] = 'smo_helpers=' + helpers
            tag = '%s_single_%s_helpers_%s' % (tname, panel, helpers or 'default')
            single(tag, quad, task, Y[1], CS[1], None, e1)
            if panel != 'compact':
                single(tag + '_rowboxes', quad, task, Y[1], None, CW[1], e1)
        os.environ.pop('BQ_TEST_HOOKS', None)
        for lists in (None, rows):
            tag = '%s_batch_%s%s' % (tname, panel, '_lists' if lists else '')
            batched(tag, quad, task, Y, eps, lists, None)
            if panel != 'compact':
                batched(tag + '_rowboxes', quad, task, Y, eps, lists, CW)
        quad.release()


if __name__ == '__main__':
    flavours(_lib.SVC, 'svc')
    flavours(_lib.SVR, 'svr')
