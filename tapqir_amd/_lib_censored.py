"""
ctypes mirrors of the censored dwell-time entry points of ``libtapqir_hip.so`` (``tq_dwell_censored_hist`` /
``tq_dwell_censored_fit`` / ``tq_dwell_survival``, include/tapqir_hip.h).  Import this module as a module
(``from tapqir_amd import _lib_censored``); ``lib()`` returns the library of ``tapqir_amd._lib.load()`` with the three
prototypes bound.
"""

import ctypes as C

from tapqir_amd import _lib

CENSORED_MAX_G = 4  # populations tq_dwell_censored_hist accepts
SURVIVAL_MAX_F = 65536  # TQ_SMOOTH_MAX_F


class DwellCensoredHistArgs(C.Structure):
    """``tq_dwell_censored_hist_args`` (include/tapqir_hip.h)."""

    _fields_ = [
        ("intervals", C.c_void_p), ("pop", C.c_void_p), ("cens_bound", C.c_void_p), ("cens_unbound", C.c_void_p),
        ("total", C.c_int64), ("S", C.c_int32), ("N", C.c_int32), ("F", C.c_int32), ("G", C.c_int32),
    ]


class DwellCensoredFitArgs(C.Structure):
    """``tq_dwell_censored_fit_args`` (include/tapqir_hip.h)."""

    _fields_ = [
        ("values", C.c_void_p), ("weights", C.c_void_p), ("row_ptr", C.c_void_p), ("cvalues", C.c_void_p),
        ("cweights", C.c_void_p), ("crow_ptr", C.c_void_p), ("state", C.c_void_p), ("loss", C.c_void_p),
        ("S", C.c_int32), ("K", C.c_int32), ("step0", C.c_int32), ("n_steps", C.c_int32), ("stage_lds", C.c_int32),
        ("lr", C.c_double), ("beta1", C.c_double), ("beta2", C.c_double), ("eps", C.c_double),
    ]


class DwellSurvivalArgs(C.Structure):
    """``tq_dwell_survival_args`` (include/tapqir_hip.h)."""

    _fields_ = [("hist", C.c_void_p), ("cens", C.c_void_p), ("surv", C.c_void_p), ("R", C.c_int32), ("F", C.c_int32)]


def bind(lib):
    """Set the prototypes of the three entry points on a loaded library; returns it."""
    for name, args in (("tq_dwell_censored_hist", DwellCensoredHistArgs), ("tq_dwell_censored_fit", DwellCensoredFitArgs),
                       ("tq_dwell_survival", DwellSurvivalArgs)):
        fn = getattr(lib, name)
        fn.argtypes = [C.POINTER(args), C.c_void_p]
        fn.restype = C.c_int
    return lib


def lib():
    """The loaded HIP library (``HipExtensionError`` if it is not built) with the censored entry points bound."""
    return bind(_lib.load())
