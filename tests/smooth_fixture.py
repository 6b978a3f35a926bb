"""Test-side helpers of the hidden-Markov smoothing tests: a numpy oracle that runs no code of the feature (sequential
scaled forward-backward with the pair marginals, the EM loop, a Viterbi that also returns its smallest decision margin;
each in float64 or ``np.longdouble``), the seeded generator of the synthetic two-state chain with calibrated evidence, the
tolerance rule of DESIGN.md section 20, and the build and binding of the g++ host check of tq_smooth.h."""

import ctypes as C
import os

import numpy as np

from helpers import build_host_check

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "hostcheck", "smooth_check.cpp")
PMIN, RMIN = 1e-6, 1e-9  # TQ_SMOOTH_PMIN, TQ_SMOOTH_RMIN
F_LIST = [1, 2, 3, 63, 64, 65, 128, 129, 203]  # the E-step cases both builds share (the host adds 5000)


# ---- oracle -----------------------------------------------------------------------------------------------------------
def _model(theta, prior, dtype):
    """A (2, 2), rho (2,), and the reciprocal prior (2,) in ``dtype``; theta and prior enter as the doubles they are."""
    kon, koff, pi0 = (dtype(np.float64(v)) for v in theta)
    prior = dtype(np.float64(prior))
    one = dtype(1)
    A = np.array([[one - kon, kon], [koff, one - koff]], dtype=dtype)
    return A, np.array([one - pi0, pi0], dtype=dtype), np.array([one / (one - prior), one / prior], dtype=dtype)


def _evidence(p, inv, dtype):
    """l (N, F, 2) of float32 p, clamped at the doubles PMIN and 1 - PMIN."""
    p = np.clip(np.asarray(p, dtype=np.float32).astype(dtype), dtype(np.float64(PMIN)), dtype(np.float64(1.0 - PMIN)))
    return np.stack([(dtype(1) - p) * inv[0], p * inv[1]], -1)


def oracle_estep(p, theta, prior, dtype=np.float64):
    """Sequential scaled forward-backward of every row: ``filt``, ``gamma`` (N, F) and ``rows`` (N, 6) = E n01, E n0, E n10,
    E n1, loglik, gamma_0(1), all in ``dtype``."""
    A, rho, inv = _model(theta, prior, dtype)
    ell = _evidence(p, inv, dtype)
    N, F = ell.shape[:2]
    a = np.zeros((N, F, 2), dtype)
    loglik = np.zeros(N, dtype)
    for f in range(F):
        u = (rho if f == 0 else a[:, f - 1] @ A) * ell[:, f]
        c = u.sum(-1)
        a[:, f] = u / c[:, None]
        loglik += np.log(c)
    gamma = np.zeros((N, F, 2), dtype)
    beta = np.ones((N, 2), dtype)
    gamma[:, F - 1] = a[:, F - 1]
    counts = np.zeros((N, 4), dtype)
    for f in range(F - 2, -1, -1):
        w = ell[:, f + 1] * beta  # (N, 2) over j
        xi = a[:, f, :, None] * A[None] * w[:, None, :]
        xi /= xi.sum((1, 2))[:, None, None]
        counts[:, 0] += xi[:, 0, 1]
        counts[:, 1] += xi[:, 0].sum(-1)
        counts[:, 2] += xi[:, 1, 0]
        counts[:, 3] += xi[:, 1].sum(-1)
        beta = w @ A.T
        beta /= beta.sum(-1)[:, None]
        g = a[:, f] * beta
        gamma[:, f] = g / g.sum(-1)[:, None]
    rows = np.concatenate([counts, loglik[:, None], gamma[:, 0, 1:2]], 1)
    return {"filt": a[..., 1].copy(), "gamma": gamma[..., 1].copy(), "rows": rows}


def oracle_mstep(rows, theta, dtype=np.float64):
    """theta after the M-step of ``rows`` (quotients, clamps, 0 / 0 keeps the old value) and the total loglik."""
    s = np.asarray(rows, dtype=dtype).sum(0)
    lo, hi = dtype(np.float64(RMIN)), dtype(np.float64(1.0 - RMIN))
    new = [dtype(np.float64(v)) for v in theta]
    if s[1] > 0:
        new[0] = np.clip(s[0] / s[1], lo, hi)
    if s[3] > 0:
        new[1] = np.clip(s[2] / s[3], lo, hi)
    new[2] = np.clip(s[5] / dtype(len(rows)), lo, hi)
    return np.array(new, dtype=dtype), s[4]


def oracle_em(p, prior, theta0, num_iter, dtype=np.float64):
    """``num_iter`` EM iterations from ``theta0``: ``thetas`` (num_iter + 1, 3) with thetas[i] the value after i
    iterations, and ``trace`` (num_iter,) with trace[i] the loglik at thetas[i].  theta is rounded to double between
    iterations, as the device's is."""
    thetas, trace = [np.array(theta0, dtype=np.float64)], []
    for _ in range(num_iter):
        new, ll = oracle_mstep(oracle_estep(p, thetas[-1], prior, dtype)["rows"], thetas[-1], dtype)
        thetas.append(new.astype(np.float64))
        trace.append(ll)
    return np.array(thetas), np.array(trace, dtype=dtype)


def oracle_viterbi(p, theta, prior, dtype=np.longdouble):
    """MAP path (N, F) uint8 in the log domain, a tie taking state 0, and the smallest |difference| of any decision taken."""
    A, rho, inv = _model(theta, prior, dtype)
    lell, lA = np.log(_evidence(p, inv, dtype)), np.log(A)
    N, F = lell.shape[:2]
    delta = np.log(rho)[None] + lell[:, 0]
    back = np.zeros((N, F, 2), np.uint8)
    margin = np.inf
    for f in range(1, F):
        cand = delta[:, :, None] + lA[None]  # (N, i, j)
        diff = cand[:, 1] - cand[:, 0]
        margin = min(margin, np.abs(diff).min())
        back[:, f] = diff > 0
        delta = np.where(diff > 0, cand[:, 1], cand[:, 0]) + lell[:, f]
        delta = delta - delta.max(-1, keepdims=True)
    diff = delta[:, 1] - delta[:, 0]
    margin = min(margin, np.abs(diff).min())
    path = np.zeros((N, F), np.uint8)
    path[:, F - 1] = diff > 0
    rows = np.arange(N)
    for f in range(F - 1, 0, -1):
        path[:, f - 1] = back[rows, f, path[:, f]]
    return path, float(margin)


def path_logprob(path, p, theta, prior, dtype=np.longdouble):
    """Joint log-probability (N,) of the rows of a 0 / 1 ``path`` with the evidence."""
    A, rho, inv = _model(theta, prior, dtype)
    lell, lA = np.log(_evidence(p, inv, dtype)), np.log(A)
    z = np.asarray(path).astype(np.int64)
    out = np.log(rho)[z[:, 0]] + np.take_along_axis(lell, z[..., None], -1)[..., 0].sum(-1)
    return out + lA[z[:, :-1], z[:, 1:]].sum(-1)


# ---- tolerance rule ---------------------------------------------------------------------------------------------------
def rule_excess(x, x64, x80):
    """|X - X80| over the bound 32 max|X64 - X80| + 1e-13 max(1, max|X80|): at most 1 when X is within the rule."""
    x80 = np.asarray(x80, dtype=np.longdouble)
    bound = 32 * np.abs(np.asarray(x64).astype(np.longdouble) - x80).max() + 1e-13 * max(1.0, float(np.abs(x80).max()))
    return float(np.abs(np.asarray(x).astype(np.longdouble) - x80).max() / bound)


# ---- inputs -----------------------------------------------------------------------------------------------------------
def synthetic_chain(N, F, seed, kon=0.05, koff=0.10, prior=1.0 / 3.0):
    """A two-state chain started from ``prior`` with calibrated evidence: the per-frame log-likelihood ratio is
    N(+-2, 2^2) and p its posterior under ``prior``.  Returns (p float32 (N, F), z uint8 (N, F))."""
    rng = np.random.default_rng(seed)
    z = np.zeros((N, F), np.uint8)
    z[:, 0] = rng.random(N) < prior
    u = rng.random((N, F))
    for f in range(1, F):
        z[:, f] = np.where(z[:, f - 1] == 1, u[:, f] >= koff, u[:, f] < kon)
    llr = rng.normal(np.where(z == 1, 2.0, -2.0), 2.0)
    p = 1.0 / (1.0 + np.exp(-(llr + np.log(prior / (1.0 - prior)))))
    return p.astype(np.float32), z


def with_special_rows(p, prior):
    """Rows 0-3 of a copy of ``p`` replaced by all 0, all 1, alternating 0 / 1 and p = prior (as many as p has rows)."""
    p = np.array(p, dtype=np.float32)
    F = p.shape[1]
    for n, row in enumerate([np.zeros(F), np.ones(F), np.arange(F) % 2, np.full(F, prior)][: len(p)]):
        p[n] = row
    return p


def realised_rates(z):
    """kon, koff realised in a hidden raster: pooled transition counts over its frame pairs."""
    now, nxt = z[:, :-1].astype(np.int64), z[:, 1:].astype(np.int64)
    return ((1 - now) * nxt).sum() / (1 - now).sum(), (now * (1 - nxt)).sum() / now.sum()


# ---- g++ host check -----------------------------------------------------------------------------------------------------
def build_smooth_check(out_dir):
    """Compile tests/hostcheck/smooth_check.cpp into ``out_dir`` and bind it."""
    so = os.path.join(str(out_dir), "libtq_smooth_check.so")
    build_host_check(SRC, so)
    lib = C.CDLL(so)
    vp = C.c_void_p
    lib.hk_smooth_estep.argtypes = [vp, C.c_int, C.c_int, vp, C.c_double, vp, vp, vp]
    lib.hk_smooth_estep.restype = None
    lib.hk_smooth_mstep.argtypes = [vp, C.c_int, vp, vp]
    lib.hk_smooth_mstep.restype = C.c_double
    lib.hk_smooth_mstep_theta.argtypes = [vp, C.c_int, vp]
    lib.hk_smooth_mstep_theta.restype = None
    lib.hk_smooth_viterbi.argtypes = [vp, C.c_int, C.c_int, vp, C.c_double, vp, vp]
    lib.hk_smooth_viterbi.restype = None
    lib.hk_smooth_count.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_uint64, vp, vp]
    lib.hk_smooth_count.restype = C.c_double
    return lib


def host_estep(lib, p, theta, prior):
    """The g++ E-step: dict of ``filt``, ``gamma`` (N, F) and ``rows`` (N, 6), float64."""
    p = np.ascontiguousarray(p, dtype=np.float32)
    theta = np.ascontiguousarray(theta, dtype=np.float64)
    N, F = p.shape
    out = {"filt": np.full((N, F), np.nan), "gamma": np.full((N, F), np.nan), "rows": np.full((N, 6), np.nan)}
    lib.hk_smooth_estep(p.ctypes.data, N, F, theta.ctypes.data, prior, out["filt"].ctypes.data, out["gamma"].ctypes.data,
                        out["rows"].ctypes.data)
    return out


def host_mstep(lib, rows, theta):
    """The g++ M-step: (new theta (3,), loglik, sums (6,))."""
    rows = np.ascontiguousarray(rows, dtype=np.float64)
    theta = np.array(theta, dtype=np.float64)
    sums = np.zeros(6)
    ll = lib.hk_smooth_mstep(rows.ctypes.data, len(rows), theta.ctypes.data, sums.ctypes.data)
    return theta, ll, sums


def host_em(lib, p, prior, theta0, num_iter):
    """``oracle_em`` with the g++ build's E-step and M-step."""
    thetas, trace = [np.array(theta0, dtype=np.float64)], []
    for _ in range(num_iter):
        new, ll, _ = host_mstep(lib, host_estep(lib, p, thetas[-1], prior)["rows"], thetas[-1])
        thetas.append(new)
        trace.append(ll)
    return np.array(thetas), np.array(trace)


def host_viterbi(lib, p, theta, prior):
    """The g++ Viterbi path (N, F) uint8."""
    p = np.ascontiguousarray(p, dtype=np.float32)
    theta = np.ascontiguousarray(theta, dtype=np.float64)
    N, F = p.shape
    back = np.zeros(((F + 15) // 16) * N, np.uint32)
    path = np.full((N, F), 255, np.uint8)
    lib.hk_smooth_viterbi(p.ctypes.data, N, F, theta.ctypes.data, prior, back.ctypes.data, path.ctypes.data)
    return path


def host_count(lib, filt, theta, S, seed):
    """The g++ replay of tq_smooth_count: counts (S, N, 4) int32, raster (S, N, F) uint8, smallest |u - q|."""
    filt = np.ascontiguousarray(filt, dtype=np.float64)
    theta = np.ascontiguousarray(theta, dtype=np.float64)
    N, F = filt.shape
    counts = np.full((S, N, 4), -1, np.int32)
    raster = np.full((S, N, F), 255, np.uint8)
    margin = lib.hk_smooth_count(filt.ctypes.data, theta.ctypes.data, S, N, F, seed, counts.ctypes.data, raster.ctypes.data)
    return counts, raster, margin
