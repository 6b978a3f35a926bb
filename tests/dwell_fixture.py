"""Test-side helpers of the dwell-time tests: the g++ build of tq_dwell.h, its replay of the sampler, and a float64 torch
restatement of the reference's K-exponential mixture MLE (exp_model of tapqir/utils/mle_analysis.py:107-130 with
torch.optim.Adam)."""

import ctypes as C
import os

import numpy as np
import pandas as pd
import torch

from helpers import adam64, build_host_check

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "hostcheck", "dwell_check.cpp")
COLUMNS = ["posterior_sample", "aoi", "start_frame", "stop_frame", "dwell_time", "low_or_high", "z"]


def build_dwell_check(out_dir):
    """Compile tests/hostcheck/dwell_check.cpp into ``out_dir`` and bind it."""
    so = os.path.join(str(out_dir), "libtq_dwell_check.so")
    build_host_check(SRC, so)
    lib = C.CDLL(so)
    vp = C.c_void_p
    lib.hk_dwell_walk.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, C.c_int64]
    lib.hk_dwell_walk.restype = None
    lib.hk_dwell_sample.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_uint64, vp, vp, vp, vp, C.c_int64]
    lib.hk_dwell_sample.restype = None
    lib.hk_dwell_raster.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_uint64, vp]
    lib.hk_dwell_raster.restype = None
    lib.hk_dwell_code.argtypes = [C.c_int, C.c_int, C.c_int]
    lib.hk_dwell_code.restype = C.c_int
    lib.hk_dwell_pair.argtypes = [vp, C.c_int, C.c_float, C.c_float, vp]
    lib.hk_dwell_pair.restype = C.c_int
    return lib


def _table(cols, total):
    return pd.DataFrame({name: cols[i, :total].astype(np.int64) for i, name in enumerate(COLUMNS)})


def host_walk(lib, z):
    """The g++ walker on a (S, N, F) 0/1 raster: (table, counts (S, N), hist_bound (S, F), hist_unbound (S, F))."""
    z = np.ascontiguousarray(np.asarray(z), dtype=np.int32)
    S, N, F = z.shape
    counts = np.zeros((S, N), np.int32)
    hb, hu = np.zeros((S, F), np.int32), np.zeros((S, F), np.int32)
    lib.hk_dwell_walk(z.ctypes.data, S, N, F, counts.ctypes.data, hb.ctypes.data, hu.ctypes.data, None, 0)
    total = int(counts.sum())
    cols = np.zeros((7, max(total, 1)), np.int32)
    lib.hk_dwell_walk(z.ctypes.data, S, N, F, None, None, None, cols.ctypes.data, total)
    return _table(cols, total), counts, hb, hu


def host_sample(lib, p, S, seed):
    """The g++ replay of tq_dwell_sample: (table, counts (S, N), hist_bound (S, F), hist_unbound (S, F))."""
    p = np.ascontiguousarray(np.asarray(p, dtype=np.float32))
    N, F = p.shape
    counts = np.zeros((S, N), np.int32)
    hb, hu = np.zeros((S, F), np.int32), np.zeros((S, F), np.int32)
    lib.hk_dwell_sample(p.ctypes.data, S, N, F, seed, counts.ctypes.data, hb.ctypes.data, hu.ctypes.data, None, 0)
    total = int(counts.sum())
    cols = np.zeros((7, max(total, 1)), np.int32)
    lib.hk_dwell_sample(p.ctypes.data, S, N, F, seed, None, None, None, cols.ctypes.data, total)
    return _table(cols, total), counts, hb, hu


def host_raster(lib, p, S, seed):
    p = np.ascontiguousarray(np.asarray(p, dtype=np.float32))
    N, F = p.shape
    z = np.zeros((S, N, F), np.int32)
    lib.hk_dwell_raster(p.ctypes.data, S, N, F, seed, z.ctypes.data)
    return z


def init_par(S, K):
    """The reference's initial values stored unconstrained (float32, then widened): log logspace(-K + 1, 0, K), a = 0."""
    k0 = torch.logspace(-K + 1, 0, K, dtype=torch.float32)
    par = torch.cat([k0.log(), torch.zeros(K)])
    return par.double().expand(S, 2 * K).clone()


def loglik64(par, data, K):
    """Per-sample log-likelihood of exp_model in float64: par (S, 2K) = (log k, softmax logits), data (S, M) padded with
    zeros (entries > 0 count)."""
    logk, a = par[:, :K], par[:, K:]
    logA = torch.log_softmax(a, dim=1)
    t = data.unsqueeze(-1)
    terms = torch.logsumexp(logA.unsqueeze(1) + logk.unsqueeze(1) - logk.exp().unsqueeze(1) * t, dim=-1)
    return torch.where(data > 0, terms, torch.zeros_like(terms)).sum(1)


def torch_fit64(data, K, n_steps=300, lr=5e-3):
    """The reference's fit restated in float64 torch: autograd + torch.optim.Adam from the same initial values."""
    data = data.double().cpu()
    p = adam64(init_par(data.shape[0], K), lambda par: loglik64(par, data, K), n_steps, lr)
    return {"k": p[:, :K].exp(), "A": torch.softmax(p[:, K:], dim=1), "par": p}
