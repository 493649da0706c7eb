"""CPU checks of the batched augmented-Lagrangian path of OneVsRestSVC / MultiOutputSVR: the two dispatch rules row by row, the older
rules they leave alone, and the C ABI symbol of the batched solver (no GPU needed)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

RULES = ['StochasticGradientDescent', 'Adam', 'AMSGrad', 'AdaMax', 'AdaGrad', 'AdaDelta', 'RMSProp']


def _rows(plain, squared):
    """(constructor keywords, world, ndim, expected) for a loss pair: `plain` with both bounds, `squared` with the diagonal"""
    from optiml_amd.opti.constrained import ProjectedGradient
    from optiml_amd.opti.unconstrained import stochastic as st
    base = dict(loss=plain, dual=True, reg_intercept=False, optimizer=st.AdaGrad, learning_rate=1.)
    rows = [(dict(base, optimizer=getattr(st, rule)), 1, None, True) for rule in RULES]
    rows += [
        (dict(base, optimizer=st.Adam, momentum_type='polyak', momentum=0.5), 1, None, True),
        (dict(base, loss=squared), 1, None, True),
        (dict(base, reg_intercept=True), 1, None, True),
        (dict(base, loss=squared, reg_intercept=True), 1, None, True),
        (dict(base, storage='f32'), 1, None, True),
        (dict(base), 1, 4, True),
        (dict(base), 1, 3, False),                                   # the optimizers keep x histories and run step by step
        (dict(base, optimizer=st.Adam, momentum_type='nesterov'), 1, None, False),
        (dict(base, optimizer=st.Adam, momentum_type='polyak', momentum=iter([0.5] * 2000)), 1, None, False),   # a schedule
        (dict(base, storage='stream'), 1, None, False),
        (dict(base), 2, None, False),
        (dict(base, dual=False), 1, None, False),
        (dict(base, optimizer=ProjectedGradient, reg_intercept=True), 1, None, False),
        (dict(base, optimizer='smo'), 1, None, False),
    ]
    return rows


N_ROWS = 21


@pytest.mark.parametrize('row', range(N_ROWS))
def test_svc_dispatch_rule(row):
    from optiml_amd.ml.svm import SVC
    from optiml_amd.ml.svm.losses import hinge, squared_hinge
    from optiml_amd.ml.svm.multiclass import uses_batched_lagrangian_path
    rows = _rows(hinge, squared_hinge)
    assert len(rows) == N_ROWS
    kw, world, ndim, want = rows[row]
    assert uses_batched_lagrangian_path(SVC(**kw), world, ndim) is want


@pytest.mark.parametrize('row', range(N_ROWS))
def test_svr_dispatch_rule(row):
    from optiml_amd.ml.svm import SVR
    from optiml_amd.ml.svm.losses import epsilon_insensitive, squared_epsilon_insensitive
    from optiml_amd.ml.svm.multioutput import uses_batched_lagrangian_svr_path
    kw, world, ndim, want = _rows(epsilon_insensitive, squared_epsilon_insensitive)[row]
    assert uses_batched_lagrangian_svr_path(SVR(**kw), world, ndim) is want


def test_the_older_rules_still_refuse_these_configurations():
    """ProjectedGradient / FrankWolfe batching, the searches and one-vs-one keep their scope: AdaGrad and the squared losses are not
    theirs."""
    from optiml_amd.ml.svm import SVC, SVR
    from optiml_amd.ml.svm.losses import epsilon_insensitive, hinge, squared_epsilon_insensitive, squared_hinge
    from optiml_amd.ml.svm.multiclass import uses_batched_path
    from optiml_amd.ml.svm.multioutput import uses_batched_svr_path
    from optiml_amd.opti.constrained import ProjectedGradient
    from optiml_amd.opti.unconstrained.stochastic import AdaGrad
    for reg in (False, True):
        assert uses_batched_path(SVC(loss=hinge, dual=True, reg_intercept=reg, optimizer=AdaGrad, learning_rate=1.), 1) is False
        assert uses_batched_svr_path(SVR(loss=epsilon_insensitive, dual=True, reg_intercept=reg, optimizer=AdaGrad,
                                         learning_rate=1.), 1) is False
    assert uses_batched_path(SVC(loss=squared_hinge, dual=True, reg_intercept=True, optimizer=ProjectedGradient), 1) is False
    assert uses_batched_svr_path(SVR(loss=squared_epsilon_insensitive, dual=True, reg_intercept=True,
                                     optimizer=ProjectedGradient), 1) is False


def test_batched_lagrangian_entry_is_declared_exported_and_bound():
    from optiml_amd import build, _lib
    build.build()
    lib = _lib.load()
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(REPO, 'include', 'bcqp.h')).read(), flags=re.S)
    assert re.search(r'#define BQ_ABI_VERSION 3\b', text)
    assert re.search(r'\bbq_msolver_create_al\s*\(', text)
    assert hasattr(lib, 'bq_msolver_create_al')
    assert 'bq_msolver_create_al' in _lib.PROTOTYPES and len(_lib.PROTOTYPES['bq_msolver_create_al'][1]) == 12
    assert _lib.ABI_VERSION == 3 and lib.bq_abi_version() == 3


def test_null_arguments_are_bad_arguments():
    from optiml_amd import build, _lib
    build.build()
    lib = _lib.load()
    v, prm, out = np.ones(4), _lib.AlParams(), C.c_void_p()
    assert lib.bq_msolver_create_al(None, C.byref(prm), 1, _lib.ptr(v), None, None, 0, None, None, _lib.ptr(v), None,
                                    C.byref(out)) == _lib.ERR_BADARG
    assert b'bad argument' in lib.bq_last_error() and b'NULL' in lib.bq_last_error()
    assert not out.value
