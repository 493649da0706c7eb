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
