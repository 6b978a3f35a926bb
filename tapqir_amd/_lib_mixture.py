"""
ctypes mirrors of the mixture-of-chains entry points of ``libtapqir_hip.so`` (``tq_mixture_mstep`` / ``tq_mixture_count`` /
``tq_mixture_estimate`` / ``tq_population_dwell``, include/tapqir_hip.h).  Import this module as a module
(``from tapqir_amd import _lib_mixture``); ``lib()`` returns the library of ``tapqir_amd._lib.load()`` with the prototypes
bound.
"""

import ctypes as C

from tapqir_amd import _lib

MIXTURE_MAX_POP = 4  # TQ_MIXTURE_MAX_POP
MIXTURE_SITE = 0xA05  # TQ_MIXTURE_SITE (tapqir_amd/csrc/tq_mixture.h)


class MixtureMstepArgs(C.Structure):
    """``tq_mixture_mstep_args`` (include/tapqir_hip.h)."""

    _fields_ = [
        ("rows", C.c_void_p), ("theta", C.c_void_p), ("phi", C.c_void_p), ("trace", C.c_void_p), ("resp", C.c_void_p),
        ("evidence", C.c_void_p), ("active", C.c_void_p),
        ("N", C.c_int32), ("it", C.c_int32), ("T", C.c_int32), ("P", C.c_int32), ("G", C.c_int32), ("U", C.c_int32),
        ("B", C.c_int32), ("allow", C.c_uint32),
    ]


class MixtureCountArgs(C.Structure):
    """``tq_mixture_count_args`` (include/tapqir_hip.h)."""

    _fields_ = [
        ("filt", C.c_void_p), ("theta", C.c_void_p), ("resp", C.c_void_p), ("counts", C.c_void_p), ("trans", C.c_void_p),
        ("pop", C.c_void_p), ("raster", C.c_void_p),
        ("N", C.c_int32), ("F", C.c_int32), ("S", C.c_int32), ("G", C.c_int32), ("U", C.c_int32), ("B", C.c_int32),
        ("seed", C.c_uint64),
    ]


class MixtureEstimateArgs(C.Structure):
    """``tq_mixture_estimate_args`` (include/tapqir_hip.h)."""

    _fields_ = [
        ("trans", C.c_void_p), ("pop", C.c_void_p), ("totals", C.c_void_p), ("members", C.c_void_p), ("estimand", C.c_void_p),
        ("N", C.c_int32), ("S", C.c_int32), ("G", C.c_int32), ("U", C.c_int32), ("B", C.c_int32), ("resample", C.c_int32),
        ("seed", C.c_uint64),
    ]


class PopulationDwellArgs(C.Structure):
    """``tq_population_dwell_args`` (include/tapqir_hip.h); ``mode`` is ``_lib.DWELL_COUNT`` or ``_lib.DWELL_EMIT``."""

    _fields_ = [
        ("filt", C.c_void_p), ("theta", C.c_void_p), ("resp", C.c_void_p), ("counts", C.c_void_p), ("pop", C.c_void_p),
        ("hist_bound", C.c_void_p), ("hist_unbound", C.c_void_p), ("tau", C.c_void_p), ("offsets", C.c_void_p),
        ("intervals", C.c_void_p), ("total", C.c_int64),
        ("N", C.c_int32), ("F", C.c_int32), ("S", C.c_int32), ("G", C.c_int32), ("U", C.c_int32), ("B", C.c_int32),
        ("mode", C.c_int32), ("seed", C.c_uint64),
    ]


def bind(lib):
    """Set the prototypes of the entry points on a loaded library; returns it."""
    for name, args in (("tq_mixture_mstep", MixtureMstepArgs), ("tq_mixture_count", MixtureCountArgs),
                       ("tq_mixture_estimate", MixtureEstimateArgs), ("tq_population_dwell", PopulationDwellArgs)):
        fn = getattr(lib, name)
        fn.argtypes = [C.POINTER(args), C.c_void_p]
        fn.restype = C.c_int
    return lib


def lib():
    """The loaded HIP library (``HipExtensionError`` if it is not built) with the mixture entry points bound."""
    return bind(_lib.load())
