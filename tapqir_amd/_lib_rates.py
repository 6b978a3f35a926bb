"""
ctypes mirrors of the two-state rate entry points of ``libtapqir_hip.so`` (``tq_rates_count`` / ``tq_rates_estimate``,
include/tapqir_hip.h).  Import this module as a module (``from tapqir_amd import _lib_rates``); ``lib()`` returns the
library of ``tapqir_amd._lib.load()`` with both prototypes bound.
"""

import ctypes as C

from tapqir_amd import _lib

RATES_COLS = 4  # TQ_RATES_COLS: n01, n0, n10, n1


class RatesCountArgs(C.Structure):
    """``tq_rates_count_args`` (include/tapqir_hip.h)."""

    _fields_ = [
        ("p", C.c_void_p), ("counts", C.c_void_p),
        ("N", C.c_int32), ("F", C.c_int32), ("S", C.c_int32), ("seed", C.c_uint64),
    ]


class RatesEstimateArgs(C.Structure):
    """``tq_rates_estimate_args`` (include/tapqir_hip.h)."""

    _fields_ = [
        ("counts", C.c_void_p), ("totals", C.c_void_p), ("estimand", C.c_void_p),
        ("N", C.c_int32), ("S", C.c_int32), ("resample", C.c_int32), ("seed", C.c_uint64),
    ]


def bind(lib):
    """Set the prototypes of the two entry points on a loaded library; returns it."""
    lib.tq_rates_count.argtypes = [C.POINTER(RatesCountArgs), C.c_void_p]
    lib.tq_rates_count.restype = C.c_int
    lib.tq_rates_estimate.argtypes = [C.POINTER(RatesEstimateArgs), C.c_void_p]
    lib.tq_rates_estimate.restype = C.c_int
    return lib


def lib():
    """The loaded HIP library (``HipExtensionError`` if it is not built) with the rate entry points bound."""
    return bind(_lib.load())
