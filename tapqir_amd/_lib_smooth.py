"""
ctypes mirrors of the hidden-Markov smoothing entry points of ``libtapqir_hip.so`` (``tq_smooth_estep`` /
``tq_smooth_mstep`` / ``tq_smooth_viterbi`` / ``tq_smooth_count`` / ``tq_smooth_dwell``, include/tapqir_hip.h).  Import
this module as a module (``from tapqir_amd import _lib_smooth``); ``lib()`` returns the library of
``tapqir_amd._lib.load()`` with the five prototypes bound.
"""

import ctypes as C

from tapqir_amd import _lib

SMOOTH_COLS = 6  # TQ_SMOOTH_COLS: E n01, E n0, E n10, E n1, loglik, gamma_0(1)
SMOOTH_MAX_F = 65536  # TQ_SMOOTH_MAX_F


class SmoothEstepArgs(C.Structure):
    """``tq_smooth_estep_args`` (include/tapqir_hip.h)."""

    _fields_ = [
        ("p", C.c_void_p), ("theta", C.c_void_p), ("filt", C.c_void_p), ("gamma", C.c_void_p), ("rows", C.c_void_p),
        ("N", C.c_int32), ("F", C.c_int32), ("prior", C.c_double),
    ]


class SmoothMstepArgs(C.Structure):
    """``tq_smooth_mstep_args`` (include/tapqir_hip.h)."""

    _fields_ = [("rows", C.c_void_p), ("theta", C.c_void_p), ("trace", C.c_void_p), ("N", C.c_int32), ("it", C.c_int32)]


class SmoothViterbiArgs(C.Structure):
    """``tq_smooth_viterbi_args`` (include/tapqir_hip.h)."""

    _fields_ = [
        ("p", C.c_void_p), ("theta", C.c_void_p), ("back", C.c_void_p), ("path", C.c_void_p),
        ("N", C.c_int32), ("F", C.c_int32), ("prior", C.c_double),
    ]


class SmoothCountArgs(C.Structure):
    """``tq_smooth_count_args`` (include/tapqir_hip.h)."""

    _fields_ = [
        ("filt", C.c_void_p), ("theta", C.c_void_p), ("counts", C.c_void_p), ("raster", C.c_void_p),
        ("N", C.c_int32), ("F", C.c_int32), ("S", C.c_int32), ("seed", C.c_uint64),
    ]


class SmoothDwellArgs(C.Structure):
    """``tq_smooth_dwell_args`` (include/tapqir_hip.h); ``mode`` is ``_lib.DWELL_COUNT`` or ``_lib.DWELL_EMIT``."""

    _fields_ = [
        ("filt", C.c_void_p), ("theta", C.c_void_p), ("counts", C.c_void_p), ("hist_bound", C.c_void_p),
        ("hist_unbound", C.c_void_p), ("tau", C.c_void_p), ("offsets", C.c_void_p), ("intervals", C.c_void_p),
        ("total", C.c_int64), ("N", C.c_int32), ("F", C.c_int32), ("S", C.c_int32), ("mode", C.c_int32),
        ("seed", C.c_uint64),
    ]


def bind(lib):
    """Set the prototypes of the five entry points on a loaded library; returns it."""
    for name, args in (("tq_smooth_estep", SmoothEstepArgs), ("tq_smooth_mstep", SmoothMstepArgs),
                       ("tq_smooth_viterbi", SmoothViterbiArgs), ("tq_smooth_count", SmoothCountArgs),
                       ("tq_smooth_dwell", SmoothDwellArgs)):
        fn = getattr(lib, name)
        fn.argtypes = [C.POINTER(args), C.c_void_p]
        fn.restype = C.c_int
    return lib


def lib():
    """The loaded HIP library (``HipExtensionError`` if it is not built) with the smoothing entry points bound."""
    return bind(_lib.load())
