"""Test-side helpers of the side-by-side EM tests: the masked M-step and EM of the numpy oracle of
hmm_fixture (the forbidden sums zeroed, then its floor), the stopping rule of ``hmm_fit`` applied to an oracle trace, the
shared cases with their oracle results computed once, and the build and binding of the g++ host check of tq_multistart.h
with a driver that runs ``mle_analysis.multistart_em`` -- the chunk and freezing logic of ``hmm_fit_restarts`` -- on it."""

import ctypes as C
import functools
import os

import numpy as np
import torch

from helpers import build_host_check
from hmm_fixture import PRIOR, _floor, cols, oracle_estep, rule_excess, synthetic_hmm  # noqa: F401 (re-exported)
from tapqir_amd import _lib_multistart
from tapqir_amd.utils.mle_analysis import hmm_random_starts, multistart_em

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "hostcheck", "multistart_check.cpp")
F_LIST = [1, 2, 3, 63, 64, 65, 129, 203]  # the batched E-step cases both builds share (N = 6, R = 3)
UB_LIST = [(1, 1), (1, 2), (2, 2)]


def full(M):
    return np.ones((M, M), bool)


def forbid(M, *pairs):
    allow = full(M)
    for i, j in pairs:
        allow[i, j] = False
    return allow


def normalised(starts, M):
    """``starts`` (R, M * M + M) after the normalisation that ``hmm_fit`` and ``hmm_fit_restarts`` apply once to a start
    they are given (the same expression, so the same bits): what the EM of either really starts from."""
    x = torch.as_tensor(np.asarray(starts), dtype=torch.float64)
    A, rho = x[:, : M * M].reshape(-1, M, M), x[:, M * M:]
    return torch.stack([torch.cat([(A[r] / A[r].sum(1, keepdim=True)).reshape(-1), rho[r] / rho[r].sum()])
                        for r in range(len(x))]).numpy().copy()


# ---- oracle -----------------------------------------------------------------------------------------------------------
def oracle_mstep_masked(rows, theta, U, B, allow, dtype=np.float64):
    """``hmm_fixture.oracle_mstep`` under the topology ``allow`` (M, M): the summed E n_ij of a forbidden pair is zeroed,
    then the quotients and the floor as there.  Returns (theta, loglik)."""
    M = U + B
    s = np.asarray(rows, dtype=dtype).sum(0)
    s[: M * M] = np.where(np.asarray(allow, bool).ravel(), s[: M * M], dtype(0))
    new = np.asarray(theta, np.float64).astype(dtype)
    for i in range(M):
        r = s[i * M:(i + 1) * M]
        if r.sum() > 0:
            new[i * M:(i + 1) * M] = _floor(r / r.sum(), dtype)
    new[M * M:] = _floor(s[M * M:M * M + M] / dtype(len(rows)), dtype)
    return new, s[-1]


def oracle_em_masked(p, prior, theta0, U, B, num_iter, allow=None, dtype=np.float64):
    """``hmm_fixture.oracle_em`` with the masked M-step: thetas (num_iter + 1, .) and trace (num_iter,)."""
    allow = full(U + B) if allow is None else allow
    thetas, trace = [np.array(theta0, dtype=np.float64)], []
    for _ in range(num_iter):
        new, ll = oracle_mstep_masked(oracle_estep(p, thetas[-1], U, B, prior, dtype)["rows"], thetas[-1], U, B, allow, dtype)
        thetas.append(new.astype(np.float64))
        trace.append(ll)
    return np.array(thetas), np.array(trace, dtype=dtype)


def oracle_loglik(p, prior, theta, U, B, dtype=np.float64):
    return oracle_estep(p, theta, U, B, prior, dtype)["rows"][:, -1].sum()


def chunk_ends(num_iter, chunk):
    return [min(s + chunk, num_iter) for s in range(0, num_iter, chunk)]


def oracle_stop(trace, tol, num_iter, chunk):
    """(iterations, converged) of the rule of ``hmm_fit`` on a trace: after each chunk, stop once some iteration so far has
    gained at most tol * |loglik| over the one before."""
    trace = np.asarray(trace, np.float64)
    for end in chunk_ends(num_iter, chunk):
        gain = np.diff(trace[:end])
        if (gain <= tol * np.abs(trace[1:end])).any():
            return end, True
    return num_iter, False


def threshold_margin(trace, tol):
    """The smallest relative distance of an iteration's gain from the threshold tol * |loglik|."""
    trace = np.asarray(trace, np.float64)
    thr = tol * np.abs(trace[1:])
    return float(np.abs(np.diff(trace) / thr - 1.0).min())


# ---- shared cases, computed once and left unchanged --------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def em_case():
    """(1, 2) on ``synthetic_hmm(20, 300, seed=0)``, the default start and 3 random starts of seed 0 (``raw``: as generated,
    for the entry points; ``starts``: normalised once, as they do it); the oracle's EM of 40 iterations from every start in
    both precisions (the EM test reads the first 15, the freezing test all of them)."""
    U, B = 1, 2
    p = synthetic_hmm(20, 300, seed=0)[0]
    raw = hmm_random_starts(U, B, 3, seed=0).numpy()
    starts = normalised(raw, U + B)
    o64 = [oracle_em_masked(p, PRIOR, s, U, B, 40) for s in starts]
    o80 = [oracle_em_masked(p, PRIOR, s, U, B, 40, dtype=np.longdouble) for s in starts]
    return {"U": U, "B": B, "p": p, "raw": raw, "starts": starts, "th64": np.array([o[0] for o in o64]), "tr64": np.array([o[1] for o in o64]),
            "th80": np.array([o[0] for o in o80]), "tr80": np.array([o[1] for o in o80])}


FREEZE = {"tol": 2e-5, "num_iter": 40, "chunk": 8}


@functools.lru_cache(maxsize=None)
def best_case():
    """(2, 2) on ``synthetic_hmm(30, 400, seed=0)``, restarts = 7, seed = 7, 120 iterations, tol = 0: the oracle's run from
    the default start in both precisions with its final log evidence."""
    U, B = 2, 2
    p = synthetic_hmm(30, 400, seed=0)[0]
    raw = hmm_random_starts(U, B, 7, seed=7).numpy()
    starts = normalised(raw, U + B)
    th64 = oracle_em_masked(p, PRIOR, starts[0], U, B, 120)[0][-1]
    th80 = oracle_em_masked(p, PRIOR, starts[0], U, B, 120, dtype=np.longdouble)[0][-1]
    return {"U": U, "B": B, "p": p, "raw": raw, "starts": starts, "ll64": oracle_loglik(p, PRIOR, th64, U, B),
            "ll80": oracle_loglik(p, PRIOR, th80, U, B, np.longdouble)}


def bic(loglik, n_params, N, F):
    return -2.0 * float(loglik) + n_params * np.log(N * F)


# ---- g++ host check -----------------------------------------------------------------------------------------------------
def build_multistart_check(out_dir):
    """Compile tests/hostcheck/multistart_check.cpp into ``out_dir`` and bind it."""
    so = os.path.join(str(out_dir), "libtq_multistart_check.so")
    build_host_check(SRC, so)
    lib = C.CDLL(so)
    vp, i = C.c_void_p, C.c_int
    lib.hk_multistart_estep.argtypes = [vp, i, i, vp, i, i, i, C.c_double, vp, vp, vp]
    lib.hk_multistart_estep.restype = None
    lib.hk_multistart_mstep.argtypes = [vp, i, i, i, i, i, i, C.c_uint32, vp, vp, vp]
    lib.hk_multistart_mstep.restype = None
    lib.hk_multistart_allow_ok.argtypes = [C.c_uint32, i]
    lib.hk_multistart_allow_ok.restype = i
    lib.hk_multistart_model.argtypes = [vp, i, i, vp]
    lib.hk_multistart_model.restype = None
    return lib


def host_model(lib, theta, U, B):
    """theta as every kernel reads it (tq_hmm_model): floored at 1e-9 and renormalised."""
    theta = np.ascontiguousarray(theta, dtype=np.float64)
    out = np.zeros_like(theta)
    lib.hk_multistart_model(theta.ctypes.data, U, B, out.ctypes.data)
    return out


def _active_ptr(active):
    if active is None:
        return None, None
    a = np.ascontiguousarray(active, dtype=np.int32)
    return a, a.ctypes.data


def host_estep(lib, p, thetas, U, B, prior, active=None, rows=None, filt=None):
    """The g++ batched E-step: rows (R, N, M^2 + M + 1), written into ``rows`` when given (NaN-filled otherwise); ``filt``
    (R, N, F, M) float64 receives the scratch of a_f when given."""
    M = U + B
    p = np.ascontiguousarray(p, dtype=np.float32)
    thetas = np.ascontiguousarray(thetas, dtype=np.float64)
    (N, F), R = p.shape, len(thetas)
    rows = np.full((R, N, cols(M)), np.nan) if rows is None else rows
    filt = np.empty((R, N, F, M)) if filt is None else filt
    assert filt.shape == (R, N, F, M) and filt.dtype == np.float64 and filt.flags.c_contiguous
    keep, ptr = _active_ptr(active)
    lib.hk_multistart_estep(p.ctypes.data, N, F, thetas.ctypes.data, R, U, B, prior, ptr, filt.ctypes.data, rows.ctypes.data)
    return rows


def host_mstep(lib, rows, thetas, trace, it, U, B, allow=None, active=None):
    """The g++ batched M-step, ``thetas`` (R, .) and ``trace`` (R, T) float64 arrays updated in place."""
    M = U + B
    rows = np.ascontiguousarray(rows, dtype=np.float64)
    R, N = rows.shape[:2]
    bits = _lib_multistart.allow_bits(full(M) if allow is None else allow)
    keep, ptr = _active_ptr(active)
    lib.hk_multistart_mstep(rows.ctypes.data, N, R, trace.shape[1], it, U, B, bits, ptr, thetas.ctypes.data, trace.ctypes.data)
    return thetas


def host_fit(lib, p, prior, starts, U, B, allow=None, num_iter=200, tol=1e-9, chunk=50):
    """``hmm_fit_restarts`` up to the choice of the best replica with the g++ build in place of the kernels: the chunks and
    the freezing are ``mle_analysis.multistart_em``'s, run on host tensors.  Returns thetas (R, .), traces (R, num_iter)
    with NaN where nothing was written, iterations, converged, logliks (R,) of the closing batched E-step, and best."""
    M = U + B
    p = np.ascontiguousarray(p, dtype=np.float32)
    thetas = np.array(starts, dtype=np.float64)
    R, N = len(thetas), len(p)
    rows = np.full((R, N, cols(M)), np.nan)
    trace = torch.full((R, num_iter), float("nan"), dtype=torch.float64)
    active = torch.ones(R, dtype=torch.int32)
    iterations, converged = multistart_em(
        lambda: host_estep(lib, p, thetas, U, B, prior, active.numpy(), rows),
        lambda it: host_mstep(lib, rows, thetas, trace.numpy(), it, U, B, allow, active.numpy()), trace, active, num_iter,
        tol, chunk)
    logliks = host_estep(lib, p, thetas, U, B, prior, None, rows)[:, :, -1].sum(1)
    return {"thetas": thetas, "traces": trace.numpy(), "iterations": iterations, "converged": converged, "logliks": logliks,
            "best": int(np.argmax(logliks))}
