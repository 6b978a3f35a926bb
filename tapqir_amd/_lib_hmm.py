"""
ctypes mirrors of the multi-state hidden-Markov smoothing entry points of ``libtapqir_hip.so`` (``tq_hmm_estep`` /
``tq_hmm_mstep`` / ``tq_hmm_viterbi`` / ``tq_hmm_count`` / ``tq_hmm_estimate`` / ``tq_chain_dwell``,
include/tapqir_hip.h).  Import this module as a module (``from tapqir_amd import _lib_hmm``); ``lib()`` returns the
library of ``tapqir_amd._lib.load()`` with the six prototypes bound.
"""

import ctypes as C

from tapqir_amd import _lib

HMM_MAX_STATES = 4  # TQ_HMM_MAX_STATES


def hmm_cols(M):
    """``TQ_HMM_COLS(M)``: E n_ij of the M * M pairs, gamma_0 of the M states, loglik."""
    return M * M + M + 1


class HmmEstepArgs(C.Structure):
    """``tq_hmm_estep_args`` (include/tapqir_hip.h)."""

    _fields_ = [
        ("p", C.c_void_p), ("theta", C.c_void_p), ("filt", C.c_void_p), ("gamma", C.c_void_p), ("rows", C.c_void_p),
        ("N", C.c_int32), ("F", C.c_int32), ("U", C.c_int32), ("B", C.c_int32), ("prior", C.c_double),
    ]


class HmmMstepArgs(C.Structure):
    """``tq_hmm_mstep_args`` (include/tapqir_hip.h)."""

    _fields_ = [("rows", C.c_void_p), ("theta", C.c_void_p), ("trace", C.c_void_p), ("N", C.c_int32), ("it", C.c_int32),
                ("U", C.c_int32), ("B", C.c_int32)]


class HmmViterbiArgs(C.Structure):
    """``tq_hmm_viterbi_args`` (include/tapqir_hip.h)."""

    _fields_ = [
        ("p", C.c_void_p), ("theta", C.c_void_p), ("back", C.c_void_p), ("path", C.c_void_p),
        ("N", C.c_int32), ("F", C.c_int32), ("U", C.c_int32), ("B", C.c_int32), ("prior", C.c_double),
    ]


class HmmCountArgs(C.Structure):
    """``tq_hmm_count_args`` (include/tapqir_hip.h)."""

    _fields_ = [
        ("filt", C.c_void_p), ("theta", C.c_void_p), ("counts", C.c_void_p), ("trans", C.c_void_p), ("raster", C.c_void_p),
        ("N", C.c_int32), ("F", C.c_int32), ("S", C.c_int32), ("U", C.c_int32), ("B", C.c_int32), ("seed", C.c_uint64),
    ]


class HmmEstimateArgs(C.Structure):
    """``tq_hmm_estimate_args`` (include/tapqir_hip.h)."""

    _fields_ = [
        ("trans", C.c_void_p), ("totals", C.c_void_p), ("estimand", C.c_void_p),
        ("N", C.c_int32), ("S", C.c_int32), ("U", C.c_int32), ("B", C.c_int32), ("resample", C.c_int32),
        ("seed", C.c_uint64),
    ]


class ChainDwellArgs(C.Structure):
    """``tq_chain_dwell_args`` (include/tapqir_hip.h); ``mode`` is ``_lib.DWELL_COUNT`` or ``_lib.DWELL_EMIT``."""

    _fields_ = [
        ("filt", C.c_void_p), ("theta", C.c_void_p), ("counts", C.c_void_p), ("hist_bound", C.c_void_p),
        ("hist_unbound", C.c_void_p), ("tau", C.c_void_p), ("offsets", C.c_void_p), ("intervals", C.c_void_p),
        ("total", C.c_int64), ("N", C.c_int32), ("F", C.c_int32), ("S", C.c_int32), ("U", C.c_int32), ("B", C.c_int32),
        ("mode", C.c_int32), ("seed", C.c_uint64),
    ]


def bind(lib):
    """Set the prototypes of the six entry points on a loaded library; returns it."""
    for name, args in (("tq_hmm_estep", HmmEstepArgs), ("tq_hmm_mstep", HmmMstepArgs), ("tq_hmm_viterbi", HmmViterbiArgs),
                       ("tq_hmm_count", HmmCountArgs), ("tq_hmm_estimate", HmmEstimateArgs),
                       ("tq_chain_dwell", ChainDwellArgs)):
        fn = getattr(lib, name)
        fn.argtypes = [C.POINTER(args), C.c_void_p]
        fn.restype = C.c_int
    return lib


def lib():
    """The loaded HIP library (``HipExtensionError`` if it is not built) with the multi-state entry points bound."""
    return bind(_lib.load())
