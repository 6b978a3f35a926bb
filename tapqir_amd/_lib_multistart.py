"""
ctypes mirrors of the side-by-side EM entry points of ``libtapqir_hip.so`` (``tq_multistart_estep`` /
``tq_multistart_mstep``, include/tapqir_hip.h).  Import this module as a module (``from tapqir_amd import
_lib_multistart``); ``lib()`` returns the library of ``tapqir_amd._lib.load()`` with the two prototypes bound.
"""

import ctypes as C

from tapqir_amd import _lib

MULTISTART_MAX = 64  # TQ_MULTISTART_MAX


class MultistartEstepArgs(C.Structure):
    """``tq_multistart_estep_args`` (include/tapqir_hip.h)."""

    _fields_ = [
        ("p", C.c_void_p), ("theta", C.c_void_p), ("filt", C.c_void_p), ("rows", C.c_void_p), ("active", C.c_void_p),
        ("N", C.c_int32), ("F", C.c_int32), ("R", C.c_int32), ("U", C.c_int32), ("B", C.c_int32), ("prior", C.c_double),
    ]


class MultistartMstepArgs(C.Structure):
    """``tq_multistart_mstep_args`` (include/tapqir_hip.h)."""

    _fields_ = [
        ("rows", C.c_void_p), ("theta", C.c_void_p), ("trace", C.c_void_p), ("active", C.c_void_p),
        ("N", C.c_int32), ("it", C.c_int32), ("T", C.c_int32), ("R", C.c_int32), ("U", C.c_int32), ("B", C.c_int32),
        ("allow", C.c_uint32),
    ]


def allow_bits(allow):
    """The ``allow`` word of ``tq_multistart_mstep_args`` of an (M, M) array of booleans: bit i * M + j is allow[i][j]."""
    rows = [[bool(x) for x in row] for row in allow]
    M = len(rows)
    return sum(1 << (i * M + j) for i in range(M) for j in range(M) if rows[i][j])


def bind(lib):
    """Set the prototypes of the two entry points on a loaded library; returns it."""
    for name, args in (("tq_multistart_estep", MultistartEstepArgs), ("tq_multistart_mstep", MultistartMstepArgs)):
        fn = getattr(lib, name)
        fn.argtypes = [C.POINTER(args), C.c_void_p]
        fn.restype = C.c_int
    return lib


def lib():
    """The loaded HIP library (``HipExtensionError`` if it is not built) with the side-by-side entry points bound."""
    return bind(_lib.load())
