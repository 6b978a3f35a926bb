"""
ctypes mirrors of the two-channel chain entry points of ``libtapqir_hip.so`` (``tq_joint_estep`` / ``tq_joint_mstep`` /
``tq_joint_viterbi`` / ``tq_pair_dwell``, include/tapqir_hip.h).  Import this module as a module
(``from tapqir_amd import _lib_joint``); ``lib()`` returns the library of ``tapqir_amd._lib.load()`` with the prototypes
bound.
"""

import ctypes as C

from tapqir_amd import _lib
from tapqir_amd._lib_multistart import MULTISTART_MAX

JOINT_INDEPENDENT, JOINT_A_DRIVES_B, JOINT_B_DRIVES_A, JOINT_COUPLED, JOINT_FULL = range(5)  # TQ_JOINT_*
JOINT_STATES = 4  # s = z_a + 2 z_b
JOINT_THETA = JOINT_STATES * JOINT_STATES + JOINT_STATES
JOINT_COLS = JOINT_THETA + 1  # TQ_HMM_COLS(4)
# structure id -> (name, free parameters of A)
STRUCTURES = (("independent", 4), ("a-drives-b", 6), ("b-drives-a", 6), ("coupled", 8), ("full", 12))


class JointEstepArgs(C.Structure):
    """``tq_joint_estep_args`` (include/tapqir_hip.h)."""

    _fields_ = [
        ("p_a", C.c_void_p), ("p_b", C.c_void_p), ("theta", C.c_void_p), ("filt", C.c_void_p), ("gamma", C.c_void_p),
        ("rows", C.c_void_p), ("active", C.c_void_p), ("N", C.c_int32), ("F", C.c_int32), ("R", C.c_int32),
        ("prior_a", C.c_double), ("prior_b", C.c_double),
    ]


class JointMstepArgs(C.Structure):
    """``tq_joint_mstep_args`` (include/tapqir_hip.h)."""

    _fields_ = [
        ("rows", C.c_void_p), ("theta", C.c_void_p), ("trace", C.c_void_p), ("active", C.c_void_p),
        ("N", C.c_int32), ("it", C.c_int32), ("T", C.c_int32), ("R", C.c_int32), ("structure", C.c_int32 * MULTISTART_MAX),
    ]


class JointViterbiArgs(C.Structure):
    """``tq_joint_viterbi_args`` (include/tapqir_hip.h)."""

    _fields_ = [
        ("p_a", C.c_void_p), ("p_b", C.c_void_p), ("theta", C.c_void_p), ("back", C.c_void_p), ("path", C.c_void_p),
        ("N", C.c_int32), ("F", C.c_int32), ("prior_a", C.c_double), ("prior_b", C.c_double),
    ]


class PairDwellArgs(C.Structure):
    """``tq_pair_dwell_args`` (include/tapqir_hip.h); ``mode`` is ``_lib.DWELL_COUNT`` or ``_lib.DWELL_EMIT``."""

    _fields_ = [
        ("filt", C.c_void_p), ("theta", C.c_void_p), ("counts", C.c_void_p), ("hist_bound", C.c_void_p),
        ("hist_unbound", C.c_void_p), ("tau", C.c_void_p), ("tau_after", C.c_void_p), ("offsets", C.c_void_p),
        ("intervals", C.c_void_p), ("partner", C.c_void_p), ("total", C.c_int64),
        ("N", C.c_int32), ("F", C.c_int32), ("S", C.c_int32), ("which", C.c_int32), ("mode", C.c_int32), ("seed", C.c_uint64),
    ]


def structure_array(structures):
    """The ``structure`` field of ``tq_joint_mstep_args`` of a list of ids: the first len(structures) entries, zeros after."""
    ids = [int(s) for s in structures]
    return (C.c_int32 * MULTISTART_MAX)(*ids)


def bind(lib):
    """Set the prototypes of the entry points on a loaded library; returns it."""
    for name, args in (("tq_joint_estep", JointEstepArgs), ("tq_joint_mstep", JointMstepArgs),
                       ("tq_joint_viterbi", JointViterbiArgs), ("tq_pair_dwell", PairDwellArgs)):
        fn = getattr(lib, name)
        fn.argtypes = [C.POINTER(args), C.c_void_p]
        fn.restype = C.c_int
    return lib


def lib():
    """The loaded HIP library (``HipExtensionError`` if it is not built) with the two-channel entry points bound."""
    return bind(_lib.load())
