"""Test-side helpers of the multi-state hidden-Markov smoothing tests: a numpy oracle that runs no
code of the feature (sequential scaled M-state forward-backward with the pair sums, the M-step and the EM loop, a Viterbi
that also returns its smallest decision margin, the exact conditional laws of the backward sampler and a replay of its
draws; each in float64 or ``np.longdouble``), the seeded generator of an M-state hidden chain with the calibrated evidence
of smooth_fixture, and the build and binding of the g++ host check of tq_hmm.h.  The tolerance rule is smooth_fixture's."""

import ctypes as C
import os

import numpy as np

from helpers import build_host_check, load_hostcheck
from smooth_fixture import PMIN, RMIN, rule_excess, synthetic_chain, with_special_rows  # noqa: F401 (re-exported)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "hostcheck", "hmm_check.cpp")
SITE = 0xA04  # TQ_HMM_SITE
F_LIST = [1, 2, 3, 63, 64, 65, 128, 129, 203]  # the E-step cases both builds share (N = 6; and 5000 at N = 2)
UB_LIST = [(1, 1), (1, 2), (2, 1), (2, 2), (1, 3)]
PRIOR = 1.0 / 3.0
# the reference chain: one unbound state, two bound states leaving at 0.02 and 0.3 per frame
A_REF = np.array([[0.95, 0.025, 0.025], [0.02, 0.98, 0.0], [0.3, 0.0, 0.7]])


def cols(M):
    return M * M + M + 1


def pack(A, rho):
    """theta = (A row-major, rho) as float64."""
    return np.concatenate([np.asarray(A, np.float64).ravel(), np.asarray(rho, np.float64)])


def default_start(U, B):
    """The documented default start of ``hmm_fit``: the r-th state of a class leaves with probability 0.3 / 4^r, spread
    evenly over the other M - 1 states; rho uniform."""
    M = U + B
    A = np.zeros((M, M))
    for i in range(M):
        leave = 0.3 / 4.0 ** (i if i < U else i - U)
        A[i] = leave / (M - 1)
        A[i, i] = 1.0 - leave
    return pack(A, np.full(M, 1.0 / M))


def fixed_theta(U, B, seed=0):
    """A fully connected chain without symmetry between the states of a class, for the tests at a fixed theta."""
    M = U + B
    rng = np.random.default_rng(1000 + 10 * U + B + 100 * seed)
    A = rng.uniform(0.02, 0.12, (M, M))
    for i in range(M):
        A[i, i] = 0.0
        A[i, i] = 1.0 - A[i].sum()
    rho = rng.uniform(0.5, 1.5, M)
    return pack(A, rho / rho.sum())


# ---- oracle -----------------------------------------------------------------------------------------------------------
def _floor(x, dtype):
    x = np.maximum(np.asarray(x).astype(dtype), dtype(np.float64(RMIN)))
    return x / x.sum(-1, keepdims=True)


def _model(theta, U, B, prior, dtype):
    """A (M, M) and rho (M,) floored and renormalised, the reciprocal prior (2,), in ``dtype``; theta and prior enter as
    the doubles they are."""
    M = U + B
    theta = np.asarray(theta, np.float64)
    assert theta.shape == (M * M + M,)
    prior = dtype(np.float64(prior))
    one = dtype(1)
    return (_floor(theta[: M * M].reshape(M, M), dtype), _floor(theta[M * M:], dtype),
            np.array([one / (one - prior), one / prior], dtype=dtype))


def _evidence(p, inv, U, B, dtype):
    """l (N, F, M) of float32 p, clamped at the doubles PMIN and 1 - PMIN: the class evidence, repeated over its states."""
    p = np.clip(np.asarray(p, dtype=np.float32).astype(dtype), dtype(np.float64(PMIN)), dtype(np.float64(1.0 - PMIN)))
    l0, l1 = (dtype(1) - p) * inv[0], p * inv[1]
    return np.stack([l0] * U + [l1] * B, -1)


def oracle_estep(p, theta, U, B, prior, dtype=np.float64):
    """Sequential scaled forward-backward of every row: ``filt``, ``gamma`` (N, F, M) and ``rows`` (N, M^2 + M + 1) = the
    E n_ij row-major, gamma_0, loglik; all in ``dtype``."""
    M = U + B
    A, rho, inv = _model(theta, U, B, prior, dtype)
    ell = _evidence(p, inv, U, B, dtype)
    N, F = ell.shape[:2]
    a = np.zeros((N, F, M), dtype)
    loglik = np.zeros(N, dtype)
    for f in range(F):
        u = (rho if f == 0 else a[:, f - 1] @ A) * ell[:, f]
        c = u.sum(-1)
        a[:, f] = u / c[:, None]
        loglik += np.log(c)
    gamma = np.zeros((N, F, M), dtype)
    beta = np.ones((N, M), dtype)
    gamma[:, F - 1] = a[:, F - 1]
    counts = np.zeros((N, M, M), dtype)
    for f in range(F - 2, -1, -1):
        w = ell[:, f + 1] * beta
        xi = a[:, f, :, None] * A[None] * w[:, None, :]
        counts += xi / xi.sum((1, 2))[:, None, None]
        beta = w @ A.T
        beta /= beta.sum(-1)[:, None]
        g = a[:, f] * beta
        gamma[:, f] = g / g.sum(-1)[:, None]
    rows = np.concatenate([counts.reshape(N, M * M), gamma[:, 0], loglik[:, None]], 1)
    return {"filt": a, "gamma": gamma, "rows": rows}


def oracle_mstep(rows, theta, U, B, dtype=np.float64):
    """theta after the M-step of ``rows`` (quotients, floor and renormalisation, an unoccupied state keeps its row as it
    is) and the total loglik."""
    M = U + B
    s = np.asarray(rows, dtype=dtype).sum(0)
    new = np.asarray(theta, np.float64).astype(dtype)
    for i in range(M):
        r = s[i * M:(i + 1) * M]
        if r.sum() > 0:
            new[i * M:(i + 1) * M] = _floor(r / r.sum(), dtype)
    new[M * M:] = _floor(s[M * M:M * M + M] / dtype(len(rows)), dtype)
    return new, s[-1]


def oracle_em(p, prior, theta0, U, B, num_iter, dtype=np.float64):
    """``num_iter`` EM iterations from ``theta0``: ``thetas`` (num_iter + 1, M^2 + M) with thetas[i] the value after i
    iterations, and ``trace`` (num_iter,) with trace[i] the loglik at thetas[i].  theta is rounded to double between
    iterations, as the device's is."""
    thetas, trace = [np.array(theta0, dtype=np.float64)], []
    for _ in range(num_iter):
        new, ll = oracle_mstep(oracle_estep(p, thetas[-1], U, B, prior, dtype)["rows"], thetas[-1], U, B, dtype)
        thetas.append(new.astype(np.float64))
        trace.append(ll)
    return np.array(thetas), np.array(trace, dtype=dtype)


def n_params(M):
    return M * (M - 1) + (M - 1)


def bic(loglik, M, N, F):
    return -2.0 * float(loglik) + n_params(M) * np.log(N * F)


def oracle_viterbi(p, theta, U, B, prior, dtype=np.longdouble):
    """MAP path (N, F) uint8 of hidden states in the log domain, a tie taking the lowest state, and the smallest gap
    between the best and the second best candidate of any decision taken."""
    M = U + B
    A, rho, inv = _model(theta, U, B, prior, dtype)
    lell, lA = np.log(_evidence(p, inv, U, B, dtype)), np.log(A)
    N, F = lell.shape[:2]
    delta = np.log(rho)[None] + lell[:, 0]
    back = np.zeros((N, F, M), np.uint8)
    margin = np.inf

    def gap(x, axis):
        top = np.sort(x, axis=axis)
        return float((np.take(top, -1, axis) - np.take(top, -2, axis)).min())

    for f in range(1, F):
        cand = delta[:, :, None] + lA[None]  # (N, i, j)
        margin = min(margin, gap(cand, 1))
        back[:, f] = cand.argmax(1)  # the first of equal maxima
        delta = cand.max(1) + lell[:, f]
        delta = delta - delta.max(-1, keepdims=True)
    margin = min(margin, gap(delta, 1))
    path = np.zeros((N, F), np.uint8)
    path[:, F - 1] = delta.argmax(1)
    rows = np.arange(N)
    for f in range(F - 1, 0, -1):
        path[:, f - 1] = back[rows, f, path[:, f]]
    return path, margin


def sampler_laws(filt, theta, U, B, dtype=np.longdouble):
    """The exact conditional laws of the backward sampler: ``t`` (N, F, M, M - 1), t[n, f, j, i - 1] the mass of the states
    >= i of P(state_f = . | state_{f+1} = j, frames <= f) ~ a_f(.) A[., j]; at f = F - 1 the mass under a_{F-1}, for
    every j."""
    M = U + B
    A, _, _ = _model(theta, U, B, 0.5, dtype)
    a = np.asarray(filt).astype(dtype)
    w = a[:, :, :, None] * A[None, None]  # (N, F, i, j)
    w[:, -1] = a[:, -1, :, None]
    tail = np.cumsum(w[:, :, ::-1], 2)[:, :, ::-1]  # mass of the states >= i
    return np.moveaxis(tail[:, :, 1:] / tail[:, :, :1], 2, 3)


def stream_uniforms(seed, S, N, F):
    """u (S, N, F) float32: u[s, n, k] the k-th uniform of Philox stream (seed, step = s, site, elem = n), the words of the
    host build of the generator mapped as tq_uniform maps them: 24 bits, centred."""
    hc = load_hostcheck()
    hc.hc_philox.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint64, C.POINTER(C.c_uint32), C.c_int]
    hc.hc_philox.restype = None
    words = np.zeros((S, N, F), np.uint32)
    buf = (C.c_uint32 * F)()
    for s in range(S):
        for n in range(N):
            hc.hc_philox(seed, s, SITE, n, buf, F)
            words[s, n] = np.frombuffer(buf, np.uint32)
    return ((words >> 8).astype(np.float32) * np.float32(2.0 ** -24) + np.float32(2.0 ** -25)).astype(np.float32)


def oracle_sample(filt, theta, U, B, S, seed):
    """The numpy replay of the sampler's draws: raster (S, N, F) uint8 of hidden states and the smallest |u - t| of all
    compares.  u_0 is for frame F - 1, then downwards; the draw is the number of thresholds above u."""
    N, F, M = np.asarray(filt).shape
    t = sampler_laws(filt, theta, U, B)
    u = stream_uniforms(seed, S, N, F).astype(np.longdouble)
    raster = np.zeros((S, N, F), np.uint8)
    nxt = np.zeros((S, N), np.int64)
    rows = np.arange(N)[None].repeat(S, 0)
    margin = np.inf
    for f in range(F - 1, -1, -1):
        tj = t[rows, f, nxt]  # (S, N, M - 1)
        uf = u[:, :, F - 1 - f, None]
        margin = min(margin, float(np.abs(uf - tj).min()))
        nxt = (uf < tj).sum(-1)
        raster[:, :, f] = nxt
    return raster, margin


def state_pair_counts(raster, M):
    """(..., M * M) int64: the number of frame pairs (f, f + 1) of each row of a raster (..., F) in states (i, j)."""
    z = np.asarray(raster).astype(np.int64)
    idx = z[..., :-1] * M + z[..., 1:]
    return np.stack([(idx == k).sum(-1) for k in range(M * M)], -1)


def oracle_estimate(trans, M, indices=None):
    """totals (S, M * M) int64 and estimand (S, M * M) of (S, N, M * M) counts; ``indices`` (S, N) resamples the AOIs."""
    trans = np.asarray(trans).astype(np.int64)
    if indices is not None:
        trans = np.take_along_axis(trans, np.asarray(indices)[:, :, None], 1)
    totals = trans.sum(1)
    t = totals.reshape(-1, M, M).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        est = t / t.sum(-1, keepdims=True)
    return totals, est.reshape(-1, M * M)


def class_view(x, U):
    """p(class 1) of a (..., M) array of state probabilities."""
    return np.asarray(x)[..., U:].sum(-1)


# ---- inputs -----------------------------------------------------------------------------------------------------------
def synthetic_hmm(N, F, seed, A=A_REF, U=1, prior=PRIOR):
    """An M-state hidden chain with the calibrated evidence of ``synthetic_chain``: the class of frame 0 is drawn from
    ``prior`` and its state evenly within the class; the per-frame log-likelihood ratio is N(+-2, 2^2) by class and p its
    posterior under ``prior``.  Returns (p float32 (N, F), states uint8 (N, F))."""
    A = np.asarray(A, np.float64)
    M = len(A)
    rng = np.random.default_rng(seed)
    s = np.zeros((N, F), np.uint8)
    bound = rng.random(N) < prior
    s[:, 0] = np.where(bound, U + rng.integers(0, M - U, N), rng.integers(0, U, N))
    cum = np.cumsum(A, 1)
    u = rng.random((N, F))
    for f in range(1, F):
        s[:, f] = np.minimum((u[:, f, None] >= cum[s[:, f - 1]]).sum(-1), M - 1)
    z = s >= U
    llr = rng.normal(np.where(z, 2.0, -2.0), 2.0)
    p = 1.0 / (1.0 + np.exp(-(llr + np.log(prior / (1.0 - prior)))))
    return p.astype(np.float32), s


# ---- g++ host check -----------------------------------------------------------------------------------------------------
def build_hmm_check(out_dir):
    """Compile tests/hostcheck/hmm_check.cpp into ``out_dir`` and bind it."""
    so = os.path.join(str(out_dir), "libtq_hmm_check.so")
    build_host_check(SRC, so)
    lib = C.CDLL(so)
    vp, i = C.c_void_p, C.c_int
    lib.hk_hmm_estep.argtypes = [vp, i, i, vp, i, i, C.c_double, vp, vp, vp]
    lib.hk_hmm_estep.restype = None
    lib.hk_hmm_mstep.argtypes = [vp, i, i, i, vp, vp]
    lib.hk_hmm_mstep.restype = C.c_double
    lib.hk_hmm_mstep_theta.argtypes = [vp, i, i, i, vp]
    lib.hk_hmm_mstep_theta.restype = None
    lib.hk_hmm_viterbi.argtypes = [vp, i, i, vp, i, i, C.c_double, vp, vp]
    lib.hk_hmm_viterbi.restype = None
    lib.hk_hmm_count.argtypes = [vp, vp, i, i, i, i, i, C.c_uint64, vp, vp, vp]
    lib.hk_hmm_count.restype = C.c_double
    lib.hk_hmm_estimate.argtypes = [vp, i, i, i, i, i, C.c_uint64, vp, vp]
    lib.hk_hmm_estimate.restype = None
    return lib


def host_estep(lib, p, theta, U, B, prior):
    """The g++ E-step: dict of ``filt``, ``gamma`` (N, F, M) and ``rows`` (N, M^2 + M + 1), float64."""
    M = U + B
    p = np.ascontiguousarray(p, dtype=np.float32)
    theta = np.ascontiguousarray(theta, dtype=np.float64)
    N, F = p.shape
    out = {"filt": np.full((N, F, M), np.nan), "gamma": np.full((N, F, M), np.nan), "rows": np.full((N, cols(M)), np.nan)}
    lib.hk_hmm_estep(p.ctypes.data, N, F, theta.ctypes.data, U, B, prior, out["filt"].ctypes.data,
                     out["gamma"].ctypes.data, out["rows"].ctypes.data)
    return out


def host_mstep(lib, rows, theta, U, B):
    """The g++ M-step: (new theta, loglik, sums)."""
    rows = np.ascontiguousarray(rows, dtype=np.float64)
    theta = np.array(theta, dtype=np.float64)
    sums = np.zeros(cols(U + B))
    ll = lib.hk_hmm_mstep(rows.ctypes.data, len(rows), U, B, theta.ctypes.data, sums.ctypes.data)
    return theta, ll, sums


def host_em(lib, p, prior, theta0, U, B, num_iter):
    """``oracle_em`` with the g++ build's E-step and M-step."""
    thetas, trace = [np.array(theta0, dtype=np.float64)], []
    for _ in range(num_iter):
        new, ll, _ = host_mstep(lib, host_estep(lib, p, thetas[-1], U, B, prior)["rows"], thetas[-1], U, B)
        thetas.append(new)
        trace.append(ll)
    return np.array(thetas), np.array(trace)


def host_viterbi(lib, p, theta, U, B, prior):
    """The g++ Viterbi path (N, F) uint8."""
    p = np.ascontiguousarray(p, dtype=np.float32)
    theta = np.ascontiguousarray(theta, dtype=np.float64)
    N, F = p.shape
    back = np.zeros(((F + 3) // 4) * N, np.uint32)
    path = np.full((N, F), 255, np.uint8)
    lib.hk_hmm_viterbi(p.ctypes.data, N, F, theta.ctypes.data, U, B, prior, back.ctypes.data, path.ctypes.data)
    return path


def host_count(lib, filt, theta, U, B, S, seed):
    """The g++ replay of tq_hmm_count: counts (S, N, 4), trans (S, N, M * M) int32, raster (S, N, F) uint8, and the
    smallest |u - t|."""
    M = U + B
    filt = np.ascontiguousarray(filt, dtype=np.float64)
    theta = np.ascontiguousarray(theta, dtype=np.float64)
    N, F = filt.shape[:2]
    counts = np.full((S, N, 4), -1, np.int32)
    trans = np.full((S, N, M * M), -1, np.int32)
    raster = np.full((S, N, F), 255, np.uint8)
    margin = lib.hk_hmm_count(filt.ctypes.data, theta.ctypes.data, U, B, S, N, F, seed, counts.ctypes.data,
                              trans.ctypes.data, raster.ctypes.data)
    return counts, trans, raster, margin


def host_estimate(lib, trans, U, B, resample, seed):
    """The g++ replay of tq_hmm_estimate: totals (S, M * M) int64 and estimand (S, M * M) float64."""
    M = U + B
    trans = np.ascontiguousarray(trans, dtype=np.int32)
    S, N = trans.shape[:2]
    totals, est = np.zeros((S, M * M), np.int64), np.zeros((S, M * M))
    lib.hk_hmm_estimate(trans.ctypes.data, S, N, U, B, int(resample), seed, totals.ctypes.data, est.ctypes.data)
    return totals, est
