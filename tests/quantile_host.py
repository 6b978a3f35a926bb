"""ctypes driver of the g++ build of tests/hostcheck/quantile_check.cpp (numpy only: the timeout tests load it in a
fresh interpreter)."""

import ctypes as C

import numpy as np

dp = C.POINTER(C.c_double)


def open_lib(so):
    lib = C.CDLL(so)
    lib.hq_intervals.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_double, C.c_void_p, C.c_void_p, C.c_int64]
    lib.hq_intervals.restype = None
    lib.hq_igamma.argtypes = [C.c_double, C.c_double, dp, dp]
    lib.hq_igamma.restype = None
    lib.hq_ibeta.argtypes = [C.c_double] * 4 + [dp, dp]
    lib.hq_ibeta.restype = None
    return lib


def host_intervals(lib, kind, p0, p1, low, high, ci):
    p0 = np.ascontiguousarray(p0, dtype=np.float32)
    p1 = np.ascontiguousarray(p1, dtype=np.float32)
    ll, ul = np.empty(p0.size), np.empty(p0.size)
    lib.hq_intervals(kind, p0.ctypes.data, p1.ctypes.data, low, high, ci, ll.ctypes.data, ul.ctypes.data, p0.size)
    return ll, ul
