"""Point optiml_amd._lib at another build of libbcqp_hip.so (tools/bench_with_lib.py, tools/solver_flavours.py,
tools/msolver_flavours.py: before / after comparisons; the ABI version must match)."""
import ctypes as C
import os


def use_library(path):
    """An OLDER build lacks the entry points added since: their prototypes are dropped, so that the loader (which resolves every
    prototype, loudly) accepts it; a tool that then calls one of them fails with an AttributeError."""
    from optiml_amd import _lib
    _lib.LIB_PATH = os.path.abspath(path)
    lib = C.CDLL(_lib.LIB_PATH)
    for name in [n for n in _lib.PROTOTYPES if not hasattr(lib, n)]:
        del _lib.PROTOTYPES[name]
