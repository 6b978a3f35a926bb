"""Test-side helpers of the two-channel chain tests: a numpy oracle that runs no code of the feature
(the evidence product, the sequential scaled forward-backward with the pair sums, the five M-steps from their formulas,
the EM loop, a Viterbi that also returns its smallest decision margin; each in float64 or ``np.longdouble``), the seeded
generator of a four-state joint chain with the calibrated evidence of ``synthetic_chain`` per channel, the shared cases
with their oracle results computed once, and the build and binding of the g++ host check of tq_joint.h with a driver that
runs ``mle_analysis.multistart_em`` on it.  The tolerance rule is smooth_fixture's."""

import ctypes as C
import functools
import os

import numpy as np
import torch

from helpers import build_host_check
from smooth_fixture import F_LIST, PMIN, RMIN, rule_excess, with_special_rows  # noqa: F401 (re-exported)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "hostcheck", "joint_check.cpp")
M, THETA, COLS = 4, 20, 21
PRIORS = (1.0 / 3.0, 1.0 / 3.0)
NAMES = ("independent", "a-drives-b", "b-drives-a", "coupled", "full")
N_PARAMS = (7, 9, 9, 11, 15)  # free parameters of A + 3 of rho
A_A = np.array([[0.95, 0.05], [0.10, 0.90]])
A_B = np.array([[0.96, 0.04], [0.08, 0.92]])
A_INDEPENDENT = np.kron(A_B, A_A)  # state z_a + 2 z_b: b is the slow index
SWAP = [0, 2, 1, 3]  # the relabelling of the states when the channels are exchanged


def driven_chain(on0=0.005, on1=0.10, off=0.08):
    """A[s -> s'] = A_a[z_a, z_a'] P_b(z_b' | z_a, z_b): b binds at ``on0`` per frame without a and at ``on1`` with it."""
    A = np.zeros((4, 4))
    for s in range(4):
        za, zb = s & 1, s >> 1
        on = on1 if za else on0
        pb = [1.0 - on, on] if zb == 0 else [off, 1.0 - off]
        for t in range(4):
            A[s, t] = A_A[za, t & 1] * pb[t >> 1]
    return A


A_DRIVEN = driven_chain()


def pack(A, rho):
    return np.concatenate([np.asarray(A, np.float64).ravel(), np.asarray(rho, np.float64)])


def default_start():
    """The documented default start of ``joint_fit``: kron(A0, A0) with A0 = [[0.9, 0.1], [0.1, 0.9]], rho uniform."""
    A0 = np.array([[0.9, 0.1], [0.1, 0.9]])
    return pack(np.kron(A0, A0), np.full(4, 0.25))


def start_from(theta_a, theta_b):
    """kron of two two-state chains (kon, koff, pi0), b the slow index."""
    def two(t):
        return np.array([[1.0 - t[0], t[0]], [t[1], 1.0 - t[1]]]), np.array([1.0 - t[2], t[2]])
    (Aa, ra), (Ab, rb) = two(theta_a), two(theta_b)
    return pack(np.kron(Ab, Aa), np.kron(rb, ra))


def fixed_theta(seed=0):
    """A fully connected joint chain without symmetry, generated like ``hmm_fixture.fixed_theta(2, 2)``."""
    rng = np.random.default_rng(1000 + 10 * 2 + 2 + 100 * seed)
    A = rng.uniform(0.02, 0.12, (M, M))
    for i in range(M):
        A[i, i] = 0.0
        A[i, i] = 1.0 - A[i].sum()
    rho = rng.uniform(0.5, 1.5, M)
    return pack(A, rho / rho.sum())


def swap_theta(theta):
    """theta with the states 1 and 2 exchanged: the chain seen with the channels exchanged."""
    theta = np.asarray(theta, np.float64)
    return pack(theta[:16].reshape(4, 4)[SWAP][:, SWAP], theta[16:][SWAP])


def swap_rows(rows):
    rows = np.asarray(rows)
    lead = rows.shape[:-1]
    pairs = rows[..., :16].reshape(*lead, 4, 4)[..., SWAP, :][..., :, SWAP].reshape(*lead, 16)
    return np.concatenate([pairs, rows[..., 16:20][..., SWAP], rows[..., 20:]], -1)


def rule_bound(x64, x80):
    """The bound of the rule: 32 max|X64 - X80| + 1e-13 max(1, max|X80|)."""
    x80 = np.asarray(x80, dtype=np.longdouble)
    return float(32 * np.abs(np.asarray(x64).astype(np.longdouble) - x80).max() + 1e-13 * max(1.0, float(np.abs(x80).max())))


# ---- oracle -----------------------------------------------------------------------------------------------------------
def _floor(x, dtype):
    x = np.maximum(np.asarray(x).astype(dtype), dtype(np.float64(RMIN)))
    return x / x.sum(-1, keepdims=True)


def _model(theta, dtype):
    theta = np.asarray(theta, np.float64)
    assert theta.shape == (THETA,)
    return _floor(theta[:16].reshape(4, 4), dtype), _floor(theta[16:], dtype)


def _channel_evidence(p, prior, dtype):
    """l^c (N, F, 2) of float32 p, clamped at the doubles PMIN and 1 - PMIN, with the channel's prior divided out."""
    prior, one = dtype(np.float64(prior)), dtype(1)
    p = np.clip(np.asarray(p, dtype=np.float32).astype(dtype), dtype(np.float64(PMIN)), dtype(np.float64(1.0 - PMIN)))
    return np.stack([(one - p) / (one - prior), p / prior], -1)


def oracle_evidence(p_a, p_b, priors, dtype=np.float64):
    """l (N, F, 4): l(s) = l^a(s & 1) l^b(s >> 1)."""
    la, lb = _channel_evidence(p_a, priors[0], dtype), _channel_evidence(p_b, priors[1], dtype)
    return np.stack([la[..., s & 1] * lb[..., s >> 1] for s in range(4)], -1)


def oracle_estep(p_a, p_b, theta, priors=PRIORS, dtype=np.float64):
    """Sequential scaled forward-backward of every row: ``filt``, ``gamma`` (N, F, 4) and ``rows`` (N, 21) = the E n_ss'
    row-major, gamma_0, loglik; all in ``dtype``."""
    theta = np.asarray(theta, np.float64)
    if theta.ndim == 2:  # R chains on the same rows: every output gains a leading axis; each chain is computed on its own
        models = [_model(t, dtype) for t in theta]
        A, rho = np.stack([m[0] for m in models])[:, None], np.stack([m[1] for m in models])[:, None]  # (R, 1, 4, 4), (R, 1, 4)
    else:
        A, rho = _model(theta, dtype)
    ell = oracle_evidence(p_a, p_b, priors, dtype)
    N, F = ell.shape[:2]
    lead = theta.shape[:-1] + (N,)
    a = np.zeros(lead + (F, M), dtype)
    loglik = np.zeros(lead, dtype)
    for f in range(F):
        u = (np.broadcast_to(rho, lead + (M,)) if f == 0 else (a[..., f - 1, :, None] * A).sum(-2)) * ell[:, f]
        c = u.sum(-1)
        a[..., f, :] = u / c[..., None]
        loglik += np.log(c)
    gamma = np.zeros(lead + (F, M), dtype)
    beta = np.ones(lead + (M,), dtype)
    gamma[..., F - 1, :] = a[..., F - 1, :]
    counts = np.zeros(lead + (M, M), dtype)
    for f in range(F - 2, -1, -1):
        w = ell[:, f + 1] * beta
        xi = a[..., f, :, None] * A * w[..., None, :]
        counts += xi / xi.sum((-2, -1))[..., None, None]
        beta = (A * w[..., None, :]).sum(-1)
        beta /= beta.sum(-1)[..., None]
        g = a[..., f, :] * beta
        gamma[..., f, :] = g / g.sum(-1)[..., None]
    rows = np.concatenate([counts.reshape(lead + (M * M,)), gamma[..., 0, :], loglik[..., None]], -1)
    return {"filt": a, "gamma": gamma, "rows": rows}


def oracle_mstep_sums(s, n_rows, theta, structure, dtype=np.float64):
    """theta after the M-step of the summed columns ``s`` (21,) under ``structure``, from the formulas of the design: the
    factors P_a and P_b as quotients of margins of n, pooled over the partner's state where the structure says the channel
    does not see it, their product, the floor; a row with a zero denominator keeps its old values."""
    s = np.asarray(s).astype(dtype)
    n = s[:16].reshape(4, 4)
    new = np.asarray(theta, np.float64).astype(dtype)
    if structure == 4:
        for i in range(4):
            if n[i].sum() > 0:
                new[4 * i:4 * i + 4] = _floor(n[i] / n[i].sum(), dtype)
    else:
        n4 = n.reshape(2, 2, 2, 2)  # [z_b, z_a, z_b', z_a']
        for st in range(4):
            za, zb = st & 1, st >> 1
            # numerators over z_a' (resp. z_b'), denominators: per state or pooled over the partner's state
            num_a = n4[zb, za].sum(0) if structure in (2, 3) else n4[:, za].sum((0, 1))
            num_b = n4[zb, za].sum(1) if structure in (1, 3) else n4[zb, :].sum((0, 2))
            if num_a.sum() > 0 and num_b.sum() > 0:
                pa, pb = num_a / num_a.sum(), num_b / num_b.sum()
                new[4 * st:4 * st + 4] = _floor(np.array([pa[t & 1] * pb[t >> 1] for t in range(4)], dtype=dtype), dtype)
    new[16:] = _floor(s[16:20] / dtype(n_rows), dtype)
    return new, s[-1]


def oracle_mstep(rows, theta, structure, dtype=np.float64):
    return oracle_mstep_sums(np.asarray(rows, dtype=dtype).sum(0), len(rows), theta, structure, dtype)


def oracle_em(p_a, p_b, theta0, structure, num_iter, priors=PRIORS, dtype=np.float64):
    """``num_iter`` EM iterations from ``theta0``: thetas (num_iter + 1, 20) and trace (num_iter,), trace[i] the loglik at
    thetas[i].  theta is rounded to double between iterations, as the device's is."""
    thetas, trace = [np.array(theta0, dtype=np.float64)], []
    for _ in range(num_iter):
        new, ll = oracle_mstep(oracle_estep(p_a, p_b, thetas[-1], priors, dtype)["rows"], thetas[-1], structure, dtype)
        thetas.append(new.astype(np.float64))
        trace.append(ll)
    return np.array(thetas), np.array(trace, dtype=dtype)


def oracle_em_all(p_a, p_b, theta0, num_iter, structures=range(5), priors=PRIORS, dtype=np.float64):
    """``oracle_em`` of several structures from one start, their E-steps computed together: thetas (R, num_iter + 1, 20) and
    trace (R, num_iter)."""
    ids = list(structures)
    thetas, trace = [np.tile(np.asarray(theta0, np.float64), (len(ids), 1))], []
    for _ in range(num_iter):
        rows = oracle_estep(p_a, p_b, thetas[-1], priors, dtype)["rows"]
        steps = [oracle_mstep(rows[r], thetas[-1][r], k, dtype) for r, k in enumerate(ids)]
        thetas.append(np.array([s[0].astype(np.float64) for s in steps]))
        trace.append([s[1] for s in steps])
    return np.array(thetas).swapaxes(0, 1), np.array(trace, dtype=dtype).T


def oracle_loglik(p_a, p_b, theta, priors=PRIORS, dtype=np.float64):
    return oracle_estep(p_a, p_b, theta, priors, dtype)["rows"][:, -1].sum()


def bic(loglik, structure, N, F):
    return -2.0 * float(loglik) + N_PARAMS[structure] * np.log(N * F)


def oracle_viterbi(p_a, p_b, theta, priors=PRIORS, dtype=np.longdouble):
    """MAP path (N, F) uint8 of joint states in the log domain, a tie taking the lowest state, and the smallest gap
    between the best and the second best candidate of any decision taken."""
    A, rho = _model(theta, dtype)
    lell, lA = np.log(oracle_evidence(p_a, p_b, priors, dtype)), np.log(A)
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


def hand_rates(A):
    """The eight conditional rates and four ratios of one 4x4 matrix, written out entry by entry."""
    r = {"kon_a|b0": A[0][1] + A[0][3], "kon_a|b1": A[2][3] + A[2][1], "koff_a|b0": A[1][0] + A[1][2],
         "koff_a|b1": A[3][2] + A[3][0], "kon_b|a0": A[0][2] + A[0][3], "kon_b|a1": A[1][3] + A[1][2],
         "koff_b|a0": A[2][0] + A[2][1], "koff_b|a1": A[3][1] + A[3][0]}
    r["kon_a ratio"] = r["kon_a|b1"] / r["kon_a|b0"]
    r["koff_a ratio"] = r["koff_a|b1"] / r["koff_a|b0"]
    r["kon_b ratio"] = r["kon_b|a1"] / r["kon_b|a0"]
    r["koff_b ratio"] = r["koff_b|a1"] / r["koff_b|a0"]
    return r


def realised_matrix(states):
    """Pooled transition frequencies (4, 4) of a raster of joint states."""
    s = np.asarray(states).astype(np.int64)
    n = np.bincount((s[:, :-1] * 4 + s[:, 1:]).ravel(), minlength=16).reshape(4, 4).astype(np.float64)
    return n / n.sum(1, keepdims=True)


# ---- inputs -----------------------------------------------------------------------------------------------------------
def synthetic_joint(N, F, seed, A, priors=PRIORS):
    """A joint chain with calibrated evidence per channel.  One ``default_rng(seed)``, used in this order: z_a of frame 0
    is ``rng.random(N) < 1/3``, z_b likewise; ``u = rng.random((N, F))`` and the state of frame f is the number of
    cumulative entries of row A[s_{f-1}] that are <= u[:, f], capped at 3; then, per channel a then b, the log-likelihood
    ratio is ``rng.normal(+-2, 2)`` and p its posterior under the channel's prior.  Returns (p_a, p_b float32 (N, F),
    states uint8 (N, F))."""
    A = np.asarray(A, np.float64)
    rng = np.random.default_rng(seed)
    s = np.zeros((N, F), np.uint8)
    za0 = rng.random(N) < 1.0 / 3.0
    zb0 = rng.random(N) < 1.0 / 3.0
    s[:, 0] = za0 + 2 * zb0
    cum = np.cumsum(A, 1)
    u = rng.random((N, F))
    for f in range(1, F):
        s[:, f] = np.minimum((cum[s[:, f - 1]] <= u[:, f, None]).sum(-1), 3)
    out = []
    for z, prior in (((s & 1) == 1, priors[0]), ((s >> 1) == 1, priors[1])):
        llr = rng.normal(np.where(z, 2.0, -2.0), 2.0)
        out.append((1.0 / (1.0 + np.exp(-(llr + np.log(prior / (1.0 - prior)))))).astype(np.float32))
    return out[0], out[1], s


def estep_inputs(N, F, seed):
    """The E-step cases: channel a is ``with_special_rows`` of its p, channel b the same special rows rolled by one row, so
    every pairing of all-0 / all-1 / alternating / p = prior with a neighbour occurs."""
    pa, pb, _ = synthetic_joint(N, F, seed, A_DRIVEN)
    return with_special_rows(pa, PRIORS[0]), np.roll(with_special_rows(pb, PRIORS[1]), 1, axis=0)


# ---- shared cases, computed once and left unchanged --------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def em_case():
    """The driven chain, N = 40, F = 500, seed 0, from the default start: the oracle's EM of 25 iterations of every
    structure in both precisions."""
    pa, pb, s = synthetic_joint(40, 500, 0, A_DRIVEN)
    th64, tr64 = oracle_em_all(pa, pb, default_start(), 25)
    th80, tr80 = oracle_em_all(pa, pb, default_start(), 25, dtype=np.longdouble)
    return {"pa": pa, "pb": pb, "states": s, "th64": th64, "tr64": tr64, "th80": th80, "tr80": tr80}


@functools.lru_cache(maxsize=None)
def selection_case(kind, seed):
    """``kind`` in independent / driven / driven-swapped at N = 40, F = 500: the inputs and the float64 oracle's 60 EM
    iterations from the default start under every structure, with log evidence and BIC at the final theta."""
    A = A_INDEPENDENT if kind == "independent" else A_DRIVEN
    pa, pb, s = synthetic_joint(40, 500, seed, A)
    if kind == "driven-swapped":
        pa, pb, s = pb, pa, np.array(SWAP, np.uint8)[s]
    thetas = oracle_em_all(pa, pb, default_start(), 60)[0][:, -1]
    ll = [float(v) for v in oracle_estep(pa, pb, thetas)["rows"][:, :, -1].sum(1)]
    return {"pa": pa, "pb": pb, "states": s, "thetas": thetas, "logliks": ll, "bics": [bic(ll[k], k, 40, 500) for k in range(5)]}


# ---- g++ host check -----------------------------------------------------------------------------------------------------
def build_joint_check(out_dir):
    """Compile tests/hostcheck/joint_check.cpp into ``out_dir`` and bind it."""
    so = os.path.join(str(out_dir), "libtq_joint_check.so")
    build_host_check(SRC, so)
    lib = C.CDLL(so)
    vp, i, d = C.c_void_p, C.c_int, C.c_double
    lib.hk_joint_estep.argtypes = [vp, vp, i, i, vp, i, d, d, vp, vp, vp, vp]
    lib.hk_joint_estep.restype = None
    lib.hk_joint_mstep.argtypes = [vp, i, i, i, i, vp, vp, vp, vp]
    lib.hk_joint_mstep.restype = None
    lib.hk_joint_mstep_theta.argtypes = [vp, i, i, vp]
    lib.hk_joint_mstep_theta.restype = None
    lib.hk_joint_structure_ok.argtypes = [i]
    lib.hk_joint_structure_ok.restype = i
    lib.hk_joint_viterbi.argtypes = [vp, vp, i, i, vp, d, d, vp, vp]
    lib.hk_joint_viterbi.restype = None
    return lib


def _active_ptr(active):
    if active is None:
        return None, None
    a = np.ascontiguousarray(active, dtype=np.int32)
    return a, a.ctypes.data


def host_estep(lib, p_a, p_b, thetas, priors=PRIORS, active=None, gamma=True, out=None):
    """The g++ batched E-step: dict of ``rows`` (R, N, 21), ``filt`` and -- unless ``gamma=False`` -- ``gamma`` (R, N, F, 4),
    NaN where nothing is written; ``out`` is written into when given."""
    p_a, p_b = np.ascontiguousarray(p_a, dtype=np.float32), np.ascontiguousarray(p_b, dtype=np.float32)
    thetas = np.ascontiguousarray(thetas, dtype=np.float64)
    (N, F), R = p_a.shape, len(thetas)
    if out is None:
        out = {"rows": np.full((R, N, COLS), np.nan), "filt": np.full((R, N, F, M), np.nan)}
        if gamma:
            out["gamma"] = np.full((R, N, F, M), np.nan)
    keep, ptr = _active_ptr(active)
    lib.hk_joint_estep(p_a.ctypes.data, p_b.ctypes.data, N, F, thetas.ctypes.data, R, priors[0], priors[1], ptr,
                       out["filt"].ctypes.data, out["gamma"].ctypes.data if "gamma" in out else None, out["rows"].ctypes.data)
    return out


def host_mstep(lib, rows, thetas, trace, it, structures, active=None):
    """The g++ batched M-step, ``thetas`` (R, 20) and ``trace`` (R, T) float64 arrays updated in place."""
    rows = np.ascontiguousarray(rows, dtype=np.float64)
    R, N = rows.shape[:2]
    st = np.ascontiguousarray(structures, dtype=np.int32)
    assert st.shape == (R,)
    keep, ptr = _active_ptr(active)
    lib.hk_joint_mstep(rows.ctypes.data, N, R, trace.shape[1], it, st.ctypes.data, ptr, thetas.ctypes.data, trace.ctypes.data)
    return thetas


def host_viterbi(lib, p_a, p_b, theta, priors=PRIORS):
    p_a, p_b = np.ascontiguousarray(p_a, dtype=np.float32), np.ascontiguousarray(p_b, dtype=np.float32)
    theta = np.ascontiguousarray(theta, dtype=np.float64)
    N, F = p_a.shape
    back = np.zeros(((F + 3) // 4) * N, np.uint32)
    path = np.full((N, F), 255, np.uint8)
    lib.hk_joint_viterbi(p_a.ctypes.data, p_b.ctypes.data, N, F, theta.ctypes.data, priors[0], priors[1], back.ctypes.data,
                         path.ctypes.data)
    return path


def host_fit(lib, p_a, p_b, structures=range(5), start=None, num_iter=200, tol=1e-9, chunk=50, priors=PRIORS):
    """``joint_fit`` up to the choice of the best structure with the g++ build in place of the kernels: the chunks and
    the freezing are ``mle_analysis.multistart_em``'s, run on host tensors.  Returns thetas (R, 20), traces (R, num_iter)
    with NaN where nothing was written, iterations, converged, logliks, bics and best (a structure id)."""
    from tapqir_amd.utils.joint_analysis import joint_select
    from tapqir_amd.utils.mle_analysis import multistart_em

    ids = list(structures)
    thetas = np.tile(default_start() if start is None else np.asarray(start, np.float64), (len(ids), 1))
    R, (N, F) = len(ids), np.shape(p_a)
    out = {"rows": np.full((R, N, COLS), np.nan), "filt": np.full((R, N, F, M), np.nan)}
    trace = torch.full((R, num_iter), float("nan"), dtype=torch.float64)
    active = torch.ones(R, dtype=torch.int32)
    iterations, converged = multistart_em(
        lambda: host_estep(lib, p_a, p_b, thetas, priors, active.numpy(), False, out),
        lambda it: host_mstep(lib, out["rows"], thetas, trace.numpy(), it, ids, active.numpy()), trace, active, num_iter,
        tol, chunk)
    logliks = host_estep(lib, p_a, p_b, thetas, priors, None, False, out)["rows"][:, :, -1].sum(1)
    n_params, bics, best = joint_select(logliks.tolist(), ids, N, F)
    return {"thetas": thetas, "traces": trace.numpy(), "iterations": iterations, "converged": converged, "logliks": logliks,
            "n_params": n_params, "bics": bics, "best": best}
