"""Test-side helpers of the continuous-time hidden-Markov tests: a numpy oracle that runs no code of
the feature -- the tables P = exp(Q d) and K by scaling and squaring of the explicit 2M x 2M Van Loan matrix, the sequential
scaled forward-backward with a transition per gap, the expected jumps and holding times through xi_ab / P_ab K (the other
formula than the kernels' rank-one one), the M-step and the EM loop; each in float64 or ``np.longdouble`` -- the gap
patterns, the two-speed record of the fit tests, and the build and binding of the g++ host check of tq_timed.h.  The
tolerance rule is smooth_fixture's."""

import ctypes as C
import functools
import os

import numpy as np

from helpers import build_host_check
from hmm_fixture import A_REF, PRIOR, _evidence, _floor, cols, pack  # noqa: F401 (re-exported)
from smooth_fixture import RMIN, rule_excess, with_special_rows  # noqa: F401 (re-exported)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "hostcheck", "timed_check.cpp")
F_LIST = [1, 2, 3, 63, 64, 65, 128, 129, 203]  # the E-step cases both builds share (N = 6; and 5000 at N = 2)
UB_LIST = [(1, 1), (1, 2), (2, 2)]
D_LIST = [1e-6, 0.3, 1.0, 5.0, 60.0, 1e4]  # no scaling, scaling, deep into stationarity
PATTERNS = ["equal", "two-speed", "jitter"]


# ---- topology and theta -------------------------------------------------------------------------------------------------
def allow_bits(M, forbidden=()):
    """The mask of the entry points: bit i * M + j set where q_ij is free; the diagonal bits are set."""
    bits = (1 << (M * M)) - 1
    for i, j in forbidden:
        bits &= ~(1 << (i * M + j))
    return bits


def allow_matrix(M, bits):
    return np.array([[bool((bits >> (i * M + j)) & 1) for j in range(M)] for i in range(M)])


def fixed_theta(U, B, seed=0):
    """A fully connected generator without symmetry between the states of a class: rates 0.02 .. 0.12 per unit time."""
    M = U + B
    rng = np.random.default_rng(3000 + 10 * U + B + 100 * seed)
    Q = rng.uniform(0.02, 0.12, (M, M))
    np.fill_diagonal(Q, 0.0)
    np.fill_diagonal(Q, -Q.sum(1))
    rho = rng.uniform(0.5, 1.5, M)
    return pack(Q, rho / rho.sum())


def ref_theta():
    """The rates of ``A_REF`` as a generator (1 unbound, 2 bound states) and the mask that forbids its two zeros."""
    Q = A_REF.copy()
    np.fill_diagonal(Q, 0.0)
    np.fill_diagonal(Q, -Q.sum(1))
    return pack(Q, [0.5, 0.3, 0.2]), allow_bits(3, [(1, 2), (2, 1)])


def default_start(U, B):
    """The documented start of ``timed_fit``: the off-diagonals of hmm_fixture.default_start's A as rates, rho uniform."""
    from hmm_fixture import default_start as hmm_start

    M = U + B
    t = hmm_start(U, B)
    Q = t[: M * M].reshape(M, M).copy()
    np.fill_diagonal(Q, 0.0)
    np.fill_diagonal(Q, -Q.sum(1))
    return pack(Q, t[M * M:])


# ---- gaps ---------------------------------------------------------------------------------------------------------------
def stamps(F, pattern, seed=0):
    """F strictly increasing time stamps: all gaps equal to 1; 1 then 5 with a pause of 60 in the middle; or 1 with a
    jitter of 2 % that makes every gap its own class."""
    if pattern == "equal" or F < 2:
        return np.arange(F, dtype=np.float64)
    gaps = np.ones(F - 1)
    if pattern == "two-speed":
        gaps[(F - 1) // 2:] = 5.0
        if F > 3:
            gaps[(F - 1) // 2] = 60.0
    elif pattern == "jitter":
        gaps = gaps * (1.0 + 0.02 * np.random.default_rng(77 + seed).uniform(-1, 1, F - 1))
    return np.concatenate([[0.0], np.cumsum(gaps)])


def gap_classes(times, dedup=True):
    """(d, cls, scale) as ``timed_gaps`` documents them -- the distinct gaps over their median, the class of every gap --
    or, ``dedup=False``, one class per gap in the order of the frames."""
    times = np.asarray(times, np.float64)
    gaps = np.diff(times)
    if len(gaps) == 0:
        return np.ones(1), np.zeros(0, np.int32), 1.0
    scale = float(np.sort(gaps)[(len(gaps) - 1) // 2])
    if dedup:
        d, cls = np.unique(gaps, return_inverse=True)
    else:
        d, cls = gaps, np.arange(len(gaps))
    return d / scale, cls.astype(np.int32), scale


# ---- oracle -------------------------------------------------------------------------------------------------------------
def _generator(theta, U, B, allow, dtype):
    """Q (M, M) as the readers take it -- free rates floored, forbidden ones 0, the diagonal minus the row's sum -- and rho
    floored and renormalised, in ``dtype``."""
    M = U + B
    theta = np.asarray(theta, np.float64)
    assert theta.shape == (M * M + M,)
    free = allow_matrix(M, allow)
    Q = np.maximum(theta[: M * M].reshape(M, M).astype(dtype), dtype(np.float64(RMIN)))
    Q = np.where(free, Q, dtype(0))
    Q[np.arange(M), np.arange(M)] = dtype(0)
    Q[np.arange(M), np.arange(M)] = -Q.sum(1)
    return Q, _floor(theta[M * M:], dtype)


def _expm(X, dtype):
    """exp of a stack (..., n, n) by scaling and squaring of the plain Taylor series, in ``dtype``."""
    norm = np.abs(X).sum(-1).max(-1).astype(np.float64)
    s = np.maximum(0, np.ceil(np.log2(np.maximum(norm, 1e-300))) + 2).astype(np.int64)
    Y = X * (dtype(1) / dtype(2) ** s.astype(dtype))[..., None, None]
    n = X.shape[-1]
    E = np.broadcast_to(np.eye(n, dtype=dtype), X.shape).copy()
    term = E.copy()
    for t in range(1, 26):
        term = term @ Y / dtype(t)
        E = E + term
    for q in range(int(s.max()) if s.size else 0):
        E = np.where((s > q)[..., None, None], E @ E, E)
    return E


def oracle_tables(theta, d, U, B, allow, dtype=np.float64):
    """P (D, M, M) and K (D, M, M, M, M): for every class and every pair (i, j) the upper-right block of
    exp(d [[Q, E_ij], [0, Q]]) is K[:, :, :, i, j], its upper-left block P."""
    M = U + B
    Q, _ = _generator(theta, U, B, allow, dtype)
    d = np.asarray(d, np.float64).astype(dtype)
    D = len(d)
    C_ = np.zeros((D, M, M, 2 * M, 2 * M), dtype)
    C_[..., :M, :M] = Q
    C_[..., M:, M:] = Q
    for i in range(M):
        for j in range(M):
            C_[:, i, j, i, M + j] = dtype(1)
    E = _expm(C_ * d[:, None, None, None, None], dtype)
    P = E[:, 0, 0, :M, :M].copy()
    K = np.moveaxis(E[..., :M, M:], (1, 2), (3, 4)).copy()  # (D, a, b, i, j)
    return P, K


def scipy_difference(theta, d, U, B, allow):
    """max |P - expm(Q d)| of the float64 oracle against scipy.linalg.expm, over the classes: reported, not asserted."""
    from scipy.linalg import expm

    Q, _ = _generator(theta, U, B, allow, np.float64)
    P, _ = oracle_tables(theta, d, U, B, allow)
    return max(float(np.abs(P[k] - expm(Q * dk)).max()) for k, dk in enumerate(np.asarray(d, np.float64)))


def oracle_estep(p, theta, d, cls, U, B, allow, prior, dtype=np.float64):
    """Sequential scaled forward-backward of every row with the transition of gap f read from P[cls[f]]: ``filt``, ``gamma``
    (N, F, M) and ``rows`` (N, M^2 + M + 1) = E N_ij off the diagonal and E T_i on it, gamma_0, loglik; all in ``dtype``.
    The expected jumps and times go through the pair marginals: xi_ab / P_ab K[a][b]."""
    M = U + B
    Q, rho = _generator(theta, U, B, allow, dtype)
    one = dtype(1)
    pr = dtype(np.float64(prior))
    inv = np.array([one / (one - pr), one / pr], dtype=dtype)
    ell = _evidence(p, inv, U, B, dtype)
    N, F = ell.shape[:2]
    P, K = oracle_tables(theta, d, U, B, allow, dtype)
    a = np.zeros((N, F, M), dtype)
    loglik = np.zeros(N, dtype)
    for f in range(F):
        u = (rho if f == 0 else a[:, f - 1] @ P[cls[f - 1]]) * ell[:, f]
        c = u.sum(-1)
        a[:, f] = u / c[:, None]
        loglik += np.log(c)
    gamma = np.zeros((N, F, M), dtype)
    beta = np.ones((N, M), dtype)
    gamma[:, F - 1] = a[:, F - 1]
    stats = np.zeros((N, M, M), dtype)
    qfac = np.where(np.eye(M, dtype=bool), one, Q)
    for f in range(F - 2, -1, -1):
        Pk, Kk = P[cls[f]], K[cls[f]]
        w = ell[:, f + 1] * beta
        xi = a[:, f, :, None] * Pk[None] * w[:, None, :]
        xi = xi / xi.sum((1, 2))[:, None, None]
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(Pk[None] > 0, xi / Pk[None], dtype(0))
        stats += np.einsum("nab,abij->nij", ratio, Kk) * qfac[None]
        beta = w @ Pk.T
        beta /= beta.sum(-1)[:, None]
        g = a[:, f] * beta
        gamma[:, f] = g / g.sum(-1)[:, None]
    rows = np.concatenate([stats.reshape(N, M * M), gamma[:, 0], loglik[:, None]], 1)
    return {"filt": a, "gamma": gamma, "rows": rows}


def oracle_mstep(rows, theta, U, B, allow, dtype=np.float64):
    """theta after the M-step of ``rows`` -- q_ij = sum E N_ij / sum E T_i floored where free, 0 where forbidden, the
    diagonal minus the row's sum, a state without expected time keeps its rates -- and the total loglik."""
    M = U + B
    free = allow_matrix(M, allow)
    s = np.asarray(rows, dtype=dtype).sum(0)
    new = np.asarray(theta, np.float64).astype(dtype)
    for i in range(M):
        T = s[i * M + i]
        tot = dtype(0)
        for j in range(M):
            if j == i:
                continue
            if not free[i, j]:
                q = dtype(0)
            elif T > 0:
                q = max(s[i * M + j] / T, dtype(np.float64(RMIN)))
            else:
                q = new[i * M + j]
            new[i * M + j] = q
            tot += q
        new[i * M + i] = -tot
    new[M * M:] = _floor(s[M * M:M * M + M] / dtype(len(rows)), dtype)
    return new, s[-1]


def oracle_em(p, prior, theta0, d, cls, U, B, allow, num_iter, dtype=np.float64):
    """``num_iter`` EM iterations from ``theta0``: ``thetas`` (num_iter + 1, M^2 + M) and ``trace`` (num_iter,), trace[i]
    the loglik at thetas[i].  theta is rounded to double between iterations, as the device's is."""
    thetas, trace = [np.array(theta0, dtype=np.float64)], []
    for _ in range(num_iter):
        rows = oracle_estep(p, thetas[-1], d, cls, U, B, allow, prior, dtype)["rows"]
        new, ll = oracle_mstep(rows, thetas[-1], U, B, allow, dtype)
        thetas.append(new.astype(np.float64))
        trace.append(ll)
    return np.array(thetas), np.array(trace, dtype=dtype)


def n_params(M, allow):
    free = allow_matrix(M, allow)
    return int(free.sum() - np.trace(free)) + M - 1


# ---- the two-speed record of the fit tests --------------------------------------------------------------------------------
KON, KOFF = 0.05, 0.10  # per second
RECORD_SEED = 0


def record_stamps(seed=RECORD_SEED):
    """250 frames 1 s apart, a pause of 60 s, 250 frames 5 s apart, every gap with a jitter of 2 %: seconds."""
    rng = np.random.default_rng(500 + seed)
    gaps = np.concatenate([np.ones(249), [60.0], np.full(249, 5.0)]) * (1.0 + 0.02 * rng.uniform(-1, 1, 499))
    return np.concatenate([[0.0], np.cumsum(gaps)])


@functools.lru_cache(maxsize=None)
def record(seed=RECORD_SEED, N=40):
    """(p float32 (N, 500), times (500,)): a two-state chain with kon 0.05 / s and koff 0.10 / s observed at
    ``record_stamps`` with the calibrated evidence of hmm_fixture.synthetic_hmm (log-likelihood ratio N(+-2, 2^2))."""
    times = record_stamps(seed)
    gaps = np.diff(times)
    rng = np.random.default_rng(900 + seed)
    tot = KON + KOFF
    decay = np.exp(-tot * gaps)
    p01 = KON / tot * (1 - decay)   # P(unbound -> bound) over the gap
    p10 = KOFF / tot * (1 - decay)
    F = len(times)
    z = np.zeros((N, F), bool)
    z[:, 0] = rng.random(N) < PRIOR
    u = rng.random((N, F))
    for f in range(1, F):
        z[:, f] = np.where(z[:, f - 1], u[:, f] >= p10[f - 1], u[:, f] < p01[f - 1])
    llr = rng.normal(np.where(z, 2.0, -2.0), 2.0)
    p = 1.0 / (1.0 + np.exp(-(llr + np.log(PRIOR / (1.0 - PRIOR)))))
    return p.astype(np.float32), times


@functools.lru_cache(maxsize=None)
def fit_case(U, B, num_iter=25):
    """The record, its gap classes, the default start and the oracle's EM of ``num_iter`` iterations in both precisions."""
    p, times = record()
    d, cls, scale = gap_classes(times)
    allow = allow_bits(U + B)
    start = default_start(U, B)
    th64, tr64 = oracle_em(p, PRIOR, start, d, cls, U, B, allow, num_iter)
    th80, tr80 = oracle_em(p, PRIOR, start, d, cls, U, B, allow, num_iter, dtype=np.longdouble)
    return {"p": p, "times": times, "d": d, "cls": cls, "scale": scale, "allow": allow, "start": start, "th64": th64,
            "tr64": tr64, "th80": th80, "tr80": tr80}


# ---- g++ host check -----------------------------------------------------------------------------------------------------
def build_timed_check(out_dir):
    """Compile tests/hostcheck/timed_check.cpp into ``out_dir`` and bind it."""
    so = os.path.join(str(out_dir), "libtq_timed_check.so")
    build_host_check(SRC, so)
    lib = C.CDLL(so)
    vp, i, u = C.c_void_p, C.c_int, C.c_uint32
    lib.hk_timed_table.argtypes = [vp, vp, i, i, i, u, vp, vp]
    lib.hk_timed_table.restype = None
    lib.hk_timed_estep.argtypes = [vp, i, i, vp, vp, vp, vp, i, i, u, C.c_double, vp, vp, vp]
    lib.hk_timed_estep.restype = None
    lib.hk_timed_mstep.argtypes = [vp, i, i, i, u, vp]
    lib.hk_timed_mstep.restype = C.c_double
    return lib


def host_tables(lib, theta, d, U, B, allow):
    M = U + B
    theta = np.ascontiguousarray(theta, dtype=np.float64)
    d = np.ascontiguousarray(d, dtype=np.float64)
    P, K = np.full((len(d), M, M), np.nan), np.full((len(d), M, M, M, M), np.nan)
    lib.hk_timed_table(theta.ctypes.data, d.ctypes.data, len(d), U, B, allow, P.ctypes.data, K.ctypes.data)
    return P, K


def host_estep(lib, p, theta, P, K, cls, U, B, allow, prior, gamma=True):
    """The g++ E-step: dict of ``filt``, ``gamma`` (N, F, M; None without) and ``rows`` (N, M^2 + M + 1), float64."""
    M = U + B
    p = np.ascontiguousarray(p, dtype=np.float32)
    theta = np.ascontiguousarray(theta, dtype=np.float64)
    P, K = np.ascontiguousarray(P, dtype=np.float64), np.ascontiguousarray(K, dtype=np.float64)
    cls = np.ascontiguousarray(cls, dtype=np.int32)
    N, F = p.shape
    out = {"filt": np.full((N, F, M), np.nan), "gamma": np.full((N, F, M), np.nan) if gamma else None,
           "rows": np.full((N, cols(M)), np.nan)}
    lib.hk_timed_estep(p.ctypes.data, N, F, theta.ctypes.data, P.ctypes.data, K.ctypes.data, cls.ctypes.data, U, B, allow,
                       prior, out["filt"].ctypes.data, out["gamma"].ctypes.data if gamma else None, out["rows"].ctypes.data)
    return out


def host_mstep(lib, rows, theta, U, B, allow):
    """The g++ M-step: (new theta, loglik)."""
    rows = np.ascontiguousarray(rows, dtype=np.float64)
    theta = np.array(theta, dtype=np.float64)
    ll = lib.hk_timed_mstep(rows.ctypes.data, len(rows), U, B, allow, theta.ctypes.data)
    return theta, ll


def host_em(lib, p, prior, theta0, d, cls, U, B, allow, num_iter):
    """``oracle_em`` with the g++ build's tables, E-step and M-step."""
    thetas, trace = [np.array(theta0, dtype=np.float64)], []
    for _ in range(num_iter):
        P, K = host_tables(lib, thetas[-1], d, U, B, allow)
        rows = host_estep(lib, p, thetas[-1], P, K, cls, U, B, allow, prior, gamma=False)["rows"]
        new, ll = host_mstep(lib, rows, thetas[-1], U, B, allow)
        thetas.append(new)
        trace.append(ll)
    return np.array(thetas), np.array(trace)


# ---- shared cases -------------------------------------------------------------------------------------------------------
def rule_bound(x64, x80):
    """The bound of the rule: 32 max|X64 - X80| + 1e-13 max(1, max|X80|)."""
    x80 = np.asarray(x80, dtype=np.longdouble)
    return float(32 * np.abs(np.asarray(x64).astype(np.longdouble) - x80).max() + 1e-13 * max(1.0, float(np.abs(x80).max())))


@functools.lru_cache(maxsize=None)
def table_case(name):
    """theta, (U, B), the mask and both oracles' tables at ``D_LIST`` for ``name`` in "m2", "m3", "m4", "ref"."""
    if name == "ref":
        (theta, allow), (U, B) = ref_theta(), (1, 2)
    else:
        U, B = {"m2": (1, 1), "m3": (1, 2), "m4": (2, 2)}[name]
        theta, allow = fixed_theta(U, B, seed=1), allow_bits(U + B)
    d = np.array(D_LIST)
    return {"theta": theta, "U": U, "B": B, "allow": allow, "d": d, "t64": oracle_tables(theta, d, U, B, allow),
            "t80": oracle_tables(theta, d, U, B, allow, np.longdouble)}


@functools.lru_cache(maxsize=None)
def estep_case(F, U, B, pattern, N=6, forbidden=False):
    """N rows (the first four special) of F frames at the stamps of ``pattern``, a fixed theta -- with ``forbidden`` the
    reference chain and its mask at (1, 2) -- and both oracles' E-steps."""
    from smooth_fixture import synthetic_chain

    if forbidden:
        theta, allow = ref_theta()
    else:
        theta, allow = fixed_theta(U, B), allow_bits(U + B)
    times = stamps(F, pattern, seed=F)
    d, cls, scale = gap_classes(times)
    p = with_special_rows(synthetic_chain(N, F, seed=F)[0], PRIOR)
    return {"p": p, "theta": theta, "allow": allow, "times": times, "d": d, "cls": cls, "scale": scale,
            "o64": oracle_estep(p, theta, d, cls, U, B, allow, PRIOR),
            "o80": oracle_estep(p, theta, d, cls, U, B, allow, PRIOR, np.longdouble)}
