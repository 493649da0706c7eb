"""tools/coupling_parity.py [out.json]: the deviations the bounds of tests/coupling_reference.py are derived from, measured on the
device with the tests' own inputs and helpers (tests/test_gpu_coupling.py) — profiles/coupling/parity.json.
  coupling_points_that_differ  points of the kernel tests whose probabilities or sweep counts are not the restatement's bits
  sigmoid                      per (family, k): the largest relative deviation of the device's clipped s from NumPy's sigmoid
  ab, proba                    per estimator configuration: the batched path's probA_ / probB_ and predict_proba against the loop's
  heldout_platt                per optimizer and pair of the held-out test: the device sigmoids' A and B against the NumPy reference on
                               the same buffers (no bound is derived from it: that test holds them to platt_reference.PLATT_RTOL)
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
import coupling_reference as cr   # noqa: E402
import test_gpu_coupling as tg    # noqa: E402

rec = dict(coupling_points_that_differ=0, sigmoid={}, ab={}, proba={})
for k in cr.CLASSES:
    for family in cr.FAMILIES:
        worst = 0.
        for t in cr.POINTS:
            S = cr.target_probabilities(family, k, t)
            prob, iters, R = tg.couple(S, k)
            want, want_iters, _ = cr.couple_rows(R, k)
            rec['coupling_points_that_differ'] += int(((prob != want).any(axis=1) | (iters != want_iters)).sum())
            worst = max(worst, tg.rel_dev(R, cr.sigmoid(cr.decision_values(S), -1., 0.)))
        rec['sigmoid']['%s-%d' % (family, k)] = worst
for classes in (3, 4):
    for kind in ('pg', 'fw'):
        ab, proba = tg.estimator_deviations(classes, kind)
        rec['ab']['%d-%s' % (classes, kind)] = ab
        rec['proba']['%d-%s' % (classes, kind)] = proba
rec['heldout_platt'] = {'%s-pair%d' % (kind, p): dict(A=da, B=db, B_value=ref['B'], stop_ratio=ref['stop_ratio'])
                        for kind in ('pg', 'fw') for p, (ref, _, da, db) in enumerate(tg.heldout_platt_deviation(kind))}
for name in ('sigmoid', 'ab', 'proba'):
    rec[name + '_max_rel_dev'] = max(rec[name].values())
text = json.dumps(rec, indent=1)
print(text)
if len(sys.argv) > 1:
    with open(sys.argv[1], 'w') as f:
        f.write(text + '\n')
