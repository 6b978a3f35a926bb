"""
ctypes mirrors of the entry points of the continuous-time hidden Markov chain of ``libtapqir_hip.so`` (``tq_timed_table`` /
``tq_timed_estep`` / ``tq_timed_mstep``, include/tapqir_hip.h).  Import this module as a module (``from tapqir_amd import
_lib_timed``); ``lib()`` returns the library of ``tapqir_amd._lib.load()`` with the three prototypes bound.
"""

import ctypes as C

from tapqir_amd import _lib


class TimedTableArgs(C.Structure):
    """``tq_timed_table_args`` (include/tapqir_hip.h)."""

    _fields_ = [
        ("theta", C.c_void_p), ("d", C.c_void_p), ("d_host", C.c_void_p), ("P", C.c_void_p), ("K", C.c_void_p),
        ("D", C.c_int32), ("U", C.c_int32), ("B", C.c_int32), ("allow", C.c_uint32),
    ]


class TimedEstepArgs(C.Structure):
    """``tq_timed_estep_args`` (include/tapqir_hip.h)."""

    _fields_ = [
        ("p", C.c_void_p), ("theta", C.c_void_p), ("P", C.c_void_p), ("K", C.c_void_p), ("cls", C.c_void_p),
        ("cls_host", C.c_void_p), ("filt", C.c_void_p), ("gamma", C.c_void_p), ("rows", C.c_void_p),
        ("N", C.c_int32), ("F", C.c_int32), ("D", C.c_int32), ("U", C.c_int32), ("B", C.c_int32), ("allow", C.c_uint32),
        ("prior", C.c_double),
    ]


class TimedMstepArgs(C.Structure):
    """``tq_timed_mstep_args`` (include/tapqir_hip.h)."""

    _fields_ = [
        ("rows", C.c_void_p), ("theta", C.c_void_p), ("trace", C.c_void_p), ("N", C.c_int32), ("it", C.c_int32),
        ("T", C.c_int32), ("U", C.c_int32), ("B", C.c_int32), ("allow", C.c_uint32),
    ]


def bind(lib):
    """Set the prototypes of the three entry points on a loaded library; returns it."""
    for name, args in (("tq_timed_table", TimedTableArgs), ("tq_timed_estep", TimedEstepArgs),
                       ("tq_timed_mstep", TimedMstepArgs)):
        fn = getattr(lib, name)
        fn.argtypes = [C.POINTER(args), C.c_void_p]
        fn.restype = C.c_int
    return lib


def lib():
    """The loaded HIP library (``HipExtensionError`` if it is not built) with the entry points bound."""
    return bind(_lib.load())
