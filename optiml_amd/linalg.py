"""Dense SPD solve on the device: the cho_factor/cho_solve pair of the interior-point and active-set solvers."""
import ctypes as C

import numpy as np

from . import _lib
from .device import get_context

__all__ = ['cho_solve_spd']


def cho_solve_spd(A, b, return_factor_ms=False):
    """x = A^-1 b for a symmetric positive definite A (lower triangle read); raises LinAlgError if A is not PD."""
    A = np.ascontiguousarray(A, dtype=float)
    n = A.shape[0]
    if A.ndim != 2 or A.shape[1] != n:
        raise ValueError('expected square matrix')
    b = _lib.as_f64(b, n, 'b')
    x = np.empty(n)
    ms = C.c_double(0)
    lib = _lib.load()
    rc = lib.bq_cholesky_solve(get_context().handle, n, _lib.ptr(A), _lib.ptr(b), _lib.ptr(x), C.byref(ms))
    if rc == _lib.ERR_NOT_PD:
        raise np.linalg.LinAlgError(lib.bq_last_error().decode())
    _lib.check(rc)
    return (x, ms.value) if return_factor_ms else x


def _cholesky_probe(A, B=None, first_nonzero=None, sweeps=False, want_factor=True):
    """Diagnostic (bq_cholesky_probe): factor A once and solve with every row of B the way the ActiveSet does — a start row per
    right-hand side, the solution through the solve's second output, block by block or with the prepared sweeps.  Returns
    (X, L, info): the solutions (nrhs x n), the factor's lower triangle with zeros above it (None unless want_factor) and LAPACK's
    info (0, or 1 + the index of the first rejected pivot; the library then leaves X and L untouched: all NaN)."""
    A = np.ascontiguousarray(A, dtype=float)
    n = A.shape[0]
    if A.ndim != 2 or A.shape[1] != n:
        raise ValueError('expected square matrix')
    B = np.zeros((0, n)) if B is None else np.ascontiguousarray(np.atleast_2d(B), dtype=float)
    if B.shape[1] != n:
        raise ValueError('B holds one right-hand side of n entries per row')
    nrhs = B.shape[0]
    fnz = None
    if first_nonzero is not None:
        fnz = np.ascontiguousarray(first_nonzero, dtype=np.int64)
        if fnz.shape != (nrhs,):
            raise ValueError('first_nonzero needs one entry per right-hand side')
    X = np.full((nrhs, n), np.nan)
    L = np.full((n, n), np.nan) if want_factor else None
    info = C.c_int(-1)
    lib = _lib.load()
    _lib.check(lib.bq_cholesky_probe(get_context().handle, n, _lib.ptr(A), nrhs, _lib.ptr(B),
                                     None if fnz is None else fnz.ctypes.data_as(C.POINTER(C.c_int64)), 1 if sweeps else 0,
                                     _lib.ptr(X), _lib.ptr(L), C.byref(info)))
    return X, L, info.value
