"""Host side of the batched decision function: the entry point `bq_decision_function_multi` is declared, exported and bound, its
argument checks answer before any device call, and the rule that routes the meta-estimators' prediction (`uses_batched_decision`).
No GPU is needed."""
import ctypes as C
import os
import re

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def lib():
    from optiml_amd import build, _lib
    build.build()
    return _lib.load()


def test_entry_point_is_declared_exported_and_bound(lib):
    from optiml_amd import _lib
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(REPO, 'include', 'bcqp.h')).read(), flags=re.S)
    assert re.search(r'\bint\s+bq_decision_function_multi\s*\(', text)
    assert hasattr(lib, 'bq_decision_function_multi')
    assert 'bq_decision_function_multi' in _lib.PROTOTYPES
    assert re.search(r'#define\s+BQ_ABI_VERSION\s+3\b', text)
    assert lib.bq_abi_version() == 3 == _lib.ABI_VERSION


def test_bad_arguments_are_answered_before_any_device_call(lib):
    """NULL pointers, non-positive sizes and the Laplacian kernel: ERR_BADARG with a message.  The context here is a block of
    zeroed host memory, not a context: the checks must answer before the library reads it or calls the device."""
    from optiml_amd import _lib
    fake = C.cast(C.create_string_buffer(1 << 16), C.c_void_p)
    m, d, k, t = 5, 3, 2, 4
    SV, W, b, Xt, out = np.ones((m, d)), np.ones((k, m)), np.zeros(k), np.ones((t, d)), np.empty((k, t))
    p = _lib.ptr

    def call(ctx=fake, kernel=_lib.KERNEL_RBF, m=m, d=d, SV=SV, k=k, W=W, b=b, t=t, Xt=Xt, out=out):
        return lib.bq_decision_function_multi(ctx, kernel, 0.5, 0.0, 3, m, d, None if SV is None else p(SV), k,
                                              None if W is None else p(W), None if b is None else p(b), t,
                                              None if Xt is None else p(Xt), None if out is None else p(out))

    for kw in (dict(ctx=None), dict(SV=None), dict(W=None), dict(Xt=None), dict(out=None)):
        assert call(**kw) == _lib.ERR_BADARG, kw
        assert b'NULL' in lib.bq_last_error()
    for kw in (dict(m=0), dict(d=0), dict(t=0), dict(k=0), dict(m=-1), dict(k=-3)):
        assert call(**kw) == _lib.ERR_BADARG, kw
        assert b'm/d/t/k' in lib.bq_last_error()
    assert call(kernel=_lib.KERNEL_LAPLACIAN) == _lib.ERR_BADARG
    assert b'Laplacian' in lib.bq_last_error()
    assert call(kernel=17) == _lib.ERR_BADARG
    with pytest.raises(_lib.BcqpError):
        _lib.check(call(kernel=_lib.KERNEL_LAPLACIAN, b=None))


def test_no_support_vector_at_all_is_the_same_error_on_both_routes(lib, monkeypatch):
    """No estimator has a support vector: the union of `DecisionBatch` is empty.  The loop over the estimators does not return
    intercepts there: `SVM.decision_function` with an empty `support_vectors_` hands m = 0 to `bq_decision_function`, which
    answers ERR_BADARG before any device call, and `_lib.check` raises.  The batched route does the same through
    `bq_decision_function_multi`.  (The context is a block of zeroed host memory, as above.)"""
    from optiml_amd import _lib
    from optiml_amd.ml.svm import SVC
    from optiml_amd.ml.svm import _base, _batched
    from optiml_amd.ml.svm._batched import DecisionBatch
    from optiml_amd.ml.svm.kernels import GaussianKernel
    from optiml_amd.ml.svm.losses import hinge

    class FakeContext:
        handle = C.cast(C.create_string_buffer(1 << 16), C.c_void_p)
        world = 1

    monkeypatch.setattr(_base, 'get_context', lambda: FakeContext)
    monkeypatch.setattr(_batched, 'get_context', lambda: FakeContext)
    rs = np.random.RandomState(0)
    X, Xte = rs.standard_normal((20, 4)), rs.standard_normal((7, 4))
    kernel = GaussianKernel(gamma=0.5)
    est = SVC(loss=hinge, kernel=kernel, C=1.0, reg_intercept=True, dual=True)
    est.support_ = np.zeros(0, dtype=int)   # as `fitted_svc` and `SVC.fit` leave an estimator none of whose alphas passes 1e-6
    est.support_vectors_, est.dual_coef_, est.intercept_ = X[est.support_], np.zeros(0), 0.25
    with pytest.raises(_lib.BcqpError) as loop:
        est.decision_function(Xte)
    batch = DecisionBatch(kernel, X, np.zeros((3, 20)), [0.25, -1.0, 2.0])
    assert batch.SV.shape == (0, 4) and batch.W.shape == (3, 0) and len(batch.rows) == 0
    with pytest.raises(_lib.BcqpError) as batched:
        batch(Xte)
    assert loop.value.code == batched.value.code == _lib.ERR_BADARG
    assert 'm/d/t' in str(loop.value) and 'm/d/t/k' in str(batched.value)


def test_the_rule():
    from optiml_amd.ml.svm._batched import uses_batched_decision
    from optiml_amd.ml.svm.kernels import GaussianKernel, LaplacianKernel, PolyKernel, SigmoidKernel, gaussian, linear
    table = [
        (True, GaussianKernel(gamma=0.7), 3, 1, True),
        (True, PolyKernel(degree=3, gamma='auto', coef0=1.), 3, 1, True),
        (True, SigmoidKernel(gamma=0.1, coef0=0.5), 3, 1, True),
        (True, GaussianKernel(gamma='auto'), 2, 1, True),
        (True, GaussianKernel(gamma=0.7), 45, 1, True),
        (False, GaussianKernel(gamma='scale'), 3, 1, True),
        (False, gaussian, 3, 1, True),                         # the default: 'scale'
        (False, PolyKernel(degree=2), 3, 1, True),             # 'scale' as well
        (False, linear, 3, 1, True),
        (False, LaplacianKernel(gamma=0.3), 3, 1, True),
        (False, GaussianKernel(gamma=0.7), 1, 1, True),
        (False, GaussianKernel(gamma=0.7), 3, 2, True),
        (False, GaussianKernel(gamma=0.7), 3, 1, False),
    ]
    for want, kernel, k, world, batched in table:
        got = uses_batched_decision(kernel, k, world, batched)
        assert got is want, (type(kernel).__name__, getattr(kernel, 'gamma', None), k, world, batched)
