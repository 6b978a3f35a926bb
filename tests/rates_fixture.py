"""Test-side helpers of the two-state rate tests: the g++ build of tq_rates.h (row counter, index draw) and the numpy oracle
of the counts, which runs on the raster of the dwell-time fixture's ``host_raster`` and on no code of the feature."""

import ctypes as C
import os

import numpy as np

from helpers import build_host_check

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "hostcheck", "rates_check.cpp")


def build_rates_check(out_dir):
    """Compile tests/hostcheck/rates_check.cpp into ``out_dir`` and bind it."""
    so = os.path.join(str(out_dir), "libtq_rates_check.so")
    build_host_check(SRC, so)
    lib = C.CDLL(so)
    vp = C.c_void_p
    lib.hk_rates_count.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp]
    lib.hk_rates_count.restype = None
    lib.hk_rates_sample.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_uint64, vp]
    lib.hk_rates_sample.restype = None
    lib.hk_rates_index.argtypes = [C.c_uint64, C.c_int, C.c_uint32, C.c_uint32]
    lib.hk_rates_index.restype = C.c_uint32
    lib.hk_rates_indices.argtypes = [C.c_uint64, C.c_int, C.c_uint32, vp]
    lib.hk_rates_indices.restype = None
    lib.hk_rates_quotients.argtypes = [vp, vp]
    lib.hk_rates_quotients.restype = None
    return lib


def oracle_counts(z):
    """(..., 4) int64 counts n01, n0, n10, n1 of a 0/1 raster (..., F): numpy on the frame pairs of the last axis."""
    z = np.asarray(z).astype(np.int64)
    now, nxt = z[..., :-1], z[..., 1:]
    return np.stack([((1 - now) * nxt).sum(-1), (1 - now).sum(-1), (now * (1 - nxt)).sum(-1), now.sum(-1)], -1)


def oracle_estimands(totals):
    """(kon, koff) of (S, 4) integer totals: numpy float64 division (0 / 0 = NaN, x / 0 = inf, silently)."""
    t = np.asarray(totals).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return t[:, 0] / t[:, 1], t[:, 2] / t[:, 3]


def host_count(lib, z):
    """The g++ row counter on a (S, N, F) raster: counts (S, N, 4) int32."""
    z = np.ascontiguousarray(np.asarray(z), dtype=np.int32)
    S, N, F = z.shape
    counts = np.full((S, N, 4), -1, np.int32)
    lib.hk_rates_count(z.ctypes.data, S, N, F, counts.ctypes.data)
    return counts


def host_sample(lib, p, S, seed):
    """The g++ replay of tq_rates_count: counts (S, N, 4) int32."""
    p = np.ascontiguousarray(np.asarray(p, dtype=np.float32))
    N, F = p.shape
    counts = np.full((S, N, 4), -1, np.int32)
    lib.hk_rates_sample(p.ctypes.data, S, N, F, seed, counts.ctypes.data)
    return counts


def host_indices(lib, seed, S, N):
    """The (S, N) int64 AOI indices of a bootstrap with ``seed``."""
    out = np.full((S, N), -1, np.int64)
    lib.hk_rates_indices(seed, S, N, out.ctypes.data)
    return out
