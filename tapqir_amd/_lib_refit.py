"""
ctypes mirrors of the bootstrap-refit entry points of ``libtapqir_hip.so`` (``tq_refit_weights`` / ``tq_refit_estep`` /
``tq_refit_mstep``, include/tapqir_hip.h).  Import this module as a module (``from tapqir_amd import _lib_refit``);
``lib()`` returns the library of ``tapqir_amd._lib.load()`` with the three prototypes bound.
"""

import ctypes as C

from tapqir_amd import _lib


class RefitWeightsArgs(C.Structure):
    """``tq_refit_weights_args`` (include/tapqir_hip.h)."""

    _fields_ = [
        ("weights", C.c_void_p), ("N", C.c_int32), ("R", C.c_int32), ("first", C.c_int32), ("seed", C.c_uint64),
    ]


class RefitEstepArgs(C.Structure):
    """``tq_refit_estep_args`` (include/tapqir_hip.h)."""

    _fields_ = [
        ("p", C.c_void_p), ("theta", C.c_void_p), ("filt", C.c_void_p), ("rows", C.c_void_p), ("active", C.c_void_p),
        ("weights", C.c_void_p),
        ("N", C.c_int32), ("F", C.c_int32), ("R", C.c_int32), ("U", C.c_int32), ("B", C.c_int32), ("prior", C.c_double),
    ]


class RefitMstepArgs(C.Structure):
    """``tq_refit_mstep_args`` (include/tapqir_hip.h)."""

    _fields_ = [
        ("rows", C.c_void_p), ("theta", C.c_void_p), ("trace", C.c_void_p), ("active", C.c_void_p), ("weights", C.c_void_p),
        ("N", C.c_int32), ("it", C.c_int32), ("T", C.c_int32), ("R", C.c_int32), ("U", C.c_int32), ("B", C.c_int32),
        ("allow", C.c_uint32),
    ]


def bind(lib):
    """Set the prototypes of the three entry points on a loaded library; returns it."""
    for name, args in (("tq_refit_weights", RefitWeightsArgs), ("tq_refit_estep", RefitEstepArgs),
                       ("tq_refit_mstep", RefitMstepArgs)):
        fn = getattr(lib, name)
        fn.argtypes = [C.POINTER(args), C.c_void_p]
        fn.restype = C.c_int
    return lib


def lib():
    """The loaded HIP library (``HipExtensionError`` if it is not built) with the bootstrap-refit entry points bound."""
    return bind(_lib.load())
