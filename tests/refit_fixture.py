"""Test-side helpers of the bootstrap-refit tests.  The oracle runs no code of the feature: the
weights are the bincount of the index formula of ``tq_rates_index`` on the words of the Philox generator's host build, the
weighted M-step is numpy in float64 or long double, and the weighted EM is that M-step on the rows of
``hmm_fixture.oracle_estep`` -- the sequential forward-backward of the other chain fixtures -- for the AOIs of positive
weight.  Then the shared cases with their oracle results computed once, and the build and binding of the g++ host check of
tq_refit.h with a driver that mirrors ``mle_analysis.hmm_fit_refits`` on it."""

import ctypes as C
import functools
import os

import numpy as np
import torch

from helpers import build_host_check, load_hostcheck
from hmm_fixture import PRIOR, _floor, cols, oracle_estep, rule_excess  # noqa: F401 (re-exported)
from multistart_fixture import full
from smooth_fixture import synthetic_chain
from tapqir_amd import _lib_multistart
from tapqir_amd.utils.mle_analysis import multistart_em

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "hostcheck", "refit_check.cpp")
SITE = 0xA02  # TQ_RATES_SITE: the bootstrap over AOIs
BATCH = 64  # TQ_MULTISTART_MAX


# ---- oracle: weights ------------------------------------------------------------------------------------------------------
def oracle_indices(seed, first, R, N):
    """a (R, N) int64: a[r, i] = (w * N) >> 32 with w the first word of Philox stream (seed, step = first + r, site 0xA02,
    elem = i) -- the formula of ``tq_rates_index``, in Python integers."""
    hc = load_hostcheck()
    hc.hc_philox.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint64, C.POINTER(C.c_uint32), C.c_int]
    hc.hc_philox.restype = None
    buf = (C.c_uint32 * 1)()
    out = np.zeros((R, N), np.int64)
    for r in range(R):
        for i in range(N):
            hc.hc_philox(seed, first + r, SITE, i, buf, 1)
            out[r, i] = (int(buf[0]) * N) >> 32
    return out


def oracle_weights(seed, first, R, N):
    """weights (R, N) int32: how often resample first + r draws each AOI."""
    idx = oracle_indices(seed, first, R, N)
    return np.stack([np.bincount(idx[r], minlength=N) for r in range(R)]).astype(np.int32)


def refit_weights_all(seed, refits, N):
    """The weights of ``hmm_fit_refits``: replica 0 all ones, replica r >= 1 the resample r - 1."""
    ones = np.ones((1, N), np.int32)
    return ones if refits == 0 else np.concatenate([ones, oracle_weights(seed, 0, refits, N)])


# ---- oracle: weighted M-step and EM -----------------------------------------------------------------------------------------
def oracle_mstep_weighted(rows, w, theta, U, B, allow=None, dtype=np.float64):
    """The M-step of ``multistart_fixture.oracle_mstep_masked`` with row n counted w[n] times and sum(w) in the place of N;
    rows of weight 0 are left out before anything is read from them.  Returns (theta, weighted loglik)."""
    M = U + B
    w = np.asarray(w, np.int64)
    keep = w > 0
    s = (np.asarray(rows)[keep].astype(dtype) * w[keep].astype(dtype)[:, None]).sum(0)
    allow = full(M) if allow is None else np.asarray(allow, bool)
    s[: M * M] = np.where(allow.ravel(), s[: M * M], dtype(0))
    new = np.asarray(theta, np.float64).astype(dtype)
    for i in range(M):
        r = s[i * M:(i + 1) * M]
        if r.sum() > 0:
            new[i * M:(i + 1) * M] = _floor(r / r.sum(), dtype)
    new[M * M:] = _floor(s[M * M:M * M + M] / dtype(int(w.sum())), dtype)
    return new, s[-1]


def oracle_em_weighted(p, prior, theta0, U, B, w, num_iter, allow=None, dtype=np.float64):
    """``num_iter`` weighted EM iterations from ``theta0`` on the AOIs of positive weight: thetas (num_iter + 1, .), rounded
    to double between iterations as the device's is, and the trace (num_iter,) of weighted log evidences."""
    w = np.asarray(w, np.int64)
    keep = w > 0
    pk, wk = np.asarray(p)[keep], w[keep]
    thetas, trace = [np.array(theta0, dtype=np.float64)], []
    for _ in range(num_iter):
        rows = oracle_estep(pk, thetas[-1], U, B, prior, dtype)["rows"]
        new, ll = oracle_mstep_weighted(rows, wk, thetas[-1], U, B, allow, dtype)
        thetas.append(new.astype(np.float64))
        trace.append(ll)
    return np.array(thetas), np.array(trace, dtype=dtype)


def canonical(theta, U, B):
    """theta with the states of each class in descending A_ii (``hmm_canonical_order``), in numpy."""
    M = U + B
    A, rho = np.asarray(theta)[: M * M].reshape(M, M), np.asarray(theta)[M * M:]
    stay = np.diagonal(A)
    order = sorted(range(U), key=lambda i: -stay[i]) + sorted(range(U, M), key=lambda i: -stay[i])
    return np.concatenate([A[order][:, order].ravel(), rho[order]]), order


def two_state_theta(kon, koff, pi0):
    """(A, rho) of the chain (kon, koff, pi0) at U = B = 1."""
    return np.array([1.0 - kon, kon, koff, 1.0 - koff, 1.0 - pi0, pi0])


# ---- shared cases, computed once and left unchanged --------------------------------------------------------------------
FIT = {"N": 40, "F": 500, "refits": 8, "num_iter": 25, "seed": 3}
START = {(1, 1): two_state_theta(0.08, 0.15, 0.3),
         (1, 2): np.array([0.92, 0.05, 0.03, 0.10, 0.88, 0.02, 0.25, 0.03, 0.72, 0.6, 0.25, 0.15])}


@functools.lru_cache(maxsize=None)
def fit_data():
    """The synthetic chain of smooth_fixture (kon 0.05, koff 0.10) at N = 40, F = 500."""
    return synthetic_chain(FIT["N"], FIT["F"], seed=0)[0]


@functools.lru_cache(maxsize=None)
def fit_case(U, B):
    """R = 8 refits of 25 iterations from START[(U, B)] with tol = 0: the weights and the oracle's weighted EM of every
    replica in both precisions."""
    p, w = fit_data(), refit_weights_all(FIT["seed"], FIT["refits"], FIT["N"])
    o64 = [oracle_em_weighted(p, PRIOR, START[(U, B)], U, B, w[r], FIT["num_iter"]) for r in range(len(w))]
    o80 = [oracle_em_weighted(p, PRIOR, START[(U, B)], U, B, w[r], FIT["num_iter"], dtype=np.longdouble) for r in range(len(w))]
    return {"p": p, "weights": w, "start": START[(U, B)], "th64": np.array([o[0] for o in o64]),
            "tr64": np.array([o[1] for o in o64]), "th80": np.array([o[0] for o in o80]), "tr80": np.array([o[1] for o in o80])}


# ---- g++ host check -----------------------------------------------------------------------------------------------------
def build_refit_check(out_dir):
    """Compile tests/hostcheck/refit_check.cpp into ``out_dir`` and bind it."""
    so = os.path.join(str(out_dir), "libtq_refit_check.so")
    build_host_check(SRC, so)
    lib = C.CDLL(so)
    vp, i = C.c_void_p, C.c_int
    lib.hk_refit_weights.argtypes = [C.c_uint64, i, i, i, vp]
    lib.hk_refit_weights.restype = None
    lib.hk_refit_estep.argtypes = [vp, i, i, vp, i, i, i, C.c_double, vp, vp, vp, vp]
    lib.hk_refit_estep.restype = None
    lib.hk_refit_mstep.argtypes = [vp, vp, i, i, i, i, i, i, C.c_uint32, vp, vp, vp]
    lib.hk_refit_mstep.restype = None
    return lib


def _active_ptr(active):
    if active is None:
        return None, None
    a = np.ascontiguousarray(active, dtype=np.int32)
    return a, a.ctypes.data


def host_weights(lib, seed, first, R, N):
    out = np.full((R, N), -7, np.int32)  # the build zeroes what it counts into
    lib.hk_refit_weights(seed, first, R, N, out.ctypes.data)
    return out


def host_estep(lib, p, thetas, weights, U, B, prior, active=None, rows=None, filt=None):
    """The g++ refit E-step: rows (R, N, M^2 + M + 1), written into ``rows`` when given (NaN-filled otherwise)."""
    M = U + B
    p = np.ascontiguousarray(p, dtype=np.float32)
    thetas = np.ascontiguousarray(thetas, dtype=np.float64)
    weights = np.ascontiguousarray(weights, dtype=np.int32)
    (N, F), R = p.shape, len(thetas)
    assert weights.shape == (R, N)
    rows = np.full((R, N, cols(M)), np.nan) if rows is None else rows
    filt = np.empty((R, N, F, M)) if filt is None else filt
    assert filt.shape == (R, N, F, M) and filt.dtype == np.float64 and filt.flags.c_contiguous
    keep, ptr = _active_ptr(active)
    lib.hk_refit_estep(p.ctypes.data, N, F, thetas.ctypes.data, R, U, B, prior, ptr, weights.ctypes.data, filt.ctypes.data,
                       rows.ctypes.data)
    return rows


def host_mstep(lib, rows, weights, thetas, trace, it, U, B, allow=None, active=None):
    """The g++ refit M-step, ``thetas`` (R, .) and ``trace`` (R, T) float64 arrays updated in place."""
    M = U + B
    rows = np.ascontiguousarray(rows, dtype=np.float64)
    weights = np.ascontiguousarray(weights, dtype=np.int32)
    R, N = rows.shape[:2]
    assert weights.shape == (R, N)
    bits = _lib_multistart.allow_bits(full(M) if allow is None else allow)
    keep, ptr = _active_ptr(active)
    lib.hk_refit_mstep(rows.ctypes.data, weights.ctypes.data, N, R, trace.shape[1], it, U, B, bits, ptr, thetas.ctypes.data,
                       trace.ctypes.data)
    return thetas


def host_fit_refits(lib, p, prior, theta_hat, U, B, refits, seed=0, allow=None, num_iter=200, tol=1e-9, chunk=50):
    """``hmm_fit_refits`` with the g++ build in place of the kernels: its batches, its weights (replica 0 all ones, replica
    r the resample r - 1) and ``mle_analysis.multistart_em`` on host tensors.  Returns thetas (refits + 1, .) in the order
    the EM ran in, traces (refits + 1, num_iter), iterations, converged and the weights."""
    M = U + B
    p = np.ascontiguousarray(p, dtype=np.float32)
    N = len(p)
    out = {"thetas": [], "traces": [], "iterations": [], "converged": [], "weights": []}
    for g0 in range(0, refits + 1, BATCH):
        R = min(BATCH, refits + 1 - g0)
        if g0 == 0:
            w = np.ones((R, N), np.int32)
            if R > 1:
                w[1:] = host_weights(lib, seed, 0, R - 1, N)
        else:
            w = host_weights(lib, seed, g0 - 1, R, N)
        thetas = np.tile(np.asarray(theta_hat, np.float64), (R, 1))
        rows = np.full((R, N, cols(M)), np.nan)
        trace = torch.full((R, num_iter), float("nan"), dtype=torch.float64)
        active = torch.ones(R, dtype=torch.int32)
        its, conv = multistart_em(
            lambda: host_estep(lib, p, thetas, w, U, B, prior, active.numpy(), rows),
            lambda it: host_mstep(lib, rows, w, thetas, trace.numpy(), it, U, B, allow, active.numpy()), trace, active,
            num_iter, tol, chunk)
        out["thetas"].append(thetas)
        out["traces"].append(trace.numpy())
        out["weights"].append(w)
        out["iterations"] += its
        out["converged"] += conv
    return {k: np.concatenate(v) if k in ("thetas", "traces", "weights") else v for k, v in out.items()}
