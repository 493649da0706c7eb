"""CPU checks of MultiOutputSVR: constructor validation, the 1-D target error, the batched-vs-fallback dispatch and the C ABI symbol of
the batched SVR solver (no GPU needed)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_svr_entry_is_declared_exported_and_bound():
    from optiml_amd import build, _lib
    build.build()
    lib = _lib.load()
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(REPO, 'include', 'bcqp.h')).read(), flags=re.S)
    assert re.search(r'#define BQ_ABI_VERSION 3\b', text)
    assert re.search(r'\bbq_msolver_create_svr\s*\(', text)
    assert hasattr(lib, 'bq_msolver_create_svr')
    assert 'bq_msolver_create_svr' in _lib.PROTOTYPES
    assert _lib.PROTOTYPES['bq_msolver_create_svr'] == _lib.PROTOTYPES['bq_msolver_create']   # the same argument list
    assert _lib.ABI_VERSION == 3 and lib.bq_abi_version() == 3


def test_null_arguments_are_bad_arguments():
    from optiml_amd import build, _lib
    build.build()
    lib = _lib.load()
    v = np.ones(4)
    out = C.c_void_p()
    assert lib.bq_msolver_create_svr(None, _lib.PG, 1, _lib.ptr(v), _lib.ptr(v), None, 1e-6, 10, 0., C.byref(out)) == _lib.ERR_BADARG
    assert b'bad argument' in lib.bq_last_error() and b'NULL' in lib.bq_last_error()
    assert lib.bq_msolver_create_svr(None, _lib.PG, 1, None, None, None, 1e-6, 10, 0., None) == _lib.ERR_BADARG
    assert b'NULL' in lib.bq_last_error()
    assert not out.value


def _dispatch_rows():
    from optiml_amd.ml.svm.losses import epsilon_insensitive, squared_epsilon_insensitive
    from optiml_amd.opti.constrained import ActiveSet, FrankWolfe, InteriorPoint, ProjectedGradient
    from optiml_amd.opti.unconstrained.stochastic import AdaGrad
    base = dict(loss=epsilon_insensitive, dual=True, reg_intercept=True, optimizer=ProjectedGradient)
    return [
        (dict(base), 1, True),
        (dict(base, optimizer=FrankWolfe), 1, True),
        (dict(base, storage='f32'), 1, True),
        (dict(base, epsilon=0.), 1, True),
        (dict(base, storage='stream'), 1, False),
        (dict(base), 2, False),
        (dict(base, optimizer=ActiveSet), 1, False),
        (dict(base, optimizer=InteriorPoint), 1, False),
        (dict(base, optimizer='smo', reg_intercept=False), 1, False),
        (dict(base, optimizer=AdaGrad, learning_rate=1.), 1, False),
        (dict(base, reg_intercept=False), 1, False),
        (dict(base, dual=False), 1, False),
        (dict(base, loss=squared_epsilon_insensitive), 1, False),
    ]


@pytest.mark.parametrize('row', range(13))
def test_dispatch_rule(row):
    from optiml_amd.ml.svm import SVR
    from optiml_amd.ml.svm.multioutput import uses_batched_svr_path
    kw, world, want = _dispatch_rows()[row]
    assert uses_batched_svr_path(SVR(**kw), world) is want


def test_one_dimensional_targets_raise_the_wrappers_error():
    mo = pytest.importorskip('sklearn.multioutput')
    from optiml_amd.ml.svm import SVR, MultiOutputSVR
    X, y = np.zeros((6, 2)), np.arange(6.)
    with pytest.raises(ValueError) as ref:
        mo.MultiOutputRegressor(SVR()).fit(X, y)
    with pytest.raises(ValueError) as ours:
        MultiOutputSVR().fit(X, y)
    assert str(ours.value) == str(ref.value)


def _bad_arguments():
    from optiml_amd.ml.svm.losses import hinge, epsilon_insensitive
    return [dict(loss=hinge), dict(epsilon=-0.1), dict(loss=epsilon_insensitive, epsilon=-1), dict(kernel='rbf'), dict(C=0),
            dict(reg_intercept='yes'), dict(dual=1), dict(optimizer=3), dict(tol=0)]


@pytest.mark.parametrize('i', range(9))
def test_constructor_rejects_what_svr_rejects(i):
    from optiml_amd.ml.svm import SVR, MultiOutputSVR
    kw = _bad_arguments()[i]
    with pytest.raises(Exception) as ref:
        SVR(**kw)
    with pytest.raises(type(ref.value)) as ours:
        MultiOutputSVR(**kw)
    assert str(ours.value) == str(ref.value)


def test_constructor_keeps_svr_arguments():
    import inspect
    from optiml_amd.ml.svm import SVR, MultiOutputSVR
    from optiml_amd.ml.svm.losses import epsilon_insensitive
    assert list(inspect.signature(MultiOutputSVR).parameters) == list(inspect.signature(SVR).parameters)
    est = MultiOutputSVR(loss=epsilon_insensitive, epsilon=0.3, C=3.0, dual=True, reg_intercept=True, max_iter=7)
    assert est.C == 3.0 and est.epsilon == 0.3 and est.max_iter == 7
    assert est.get_params()['epsilon'] == 0.3
    est.set_params(max_iter=9, epsilon=0.2)
    proto = est._prototype()
    assert proto.max_iter == 9 and proto.epsilon == 0.2
