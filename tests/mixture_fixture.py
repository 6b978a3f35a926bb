"""Test-side helpers of the mixture-of-chains tests: a numpy oracle that runs no code of the feature
(the E-step of hmm_fixture batched over chains, the responsibilities, the weighted M-step under a topology mask, the EM of
several mixtures of one (U, B) at once, the default start, the law of the population draw with a replay of the sampler's
draws, the per-population estimate; each in float64 or ``np.longdouble``), the generator of AOIs from two populations, the
shared cases with their oracle results computed once, and the build and binding of the g++ host check of tq_mixture.h with
a driver that runs ``mle_analysis.multistart_em`` on it.  The tolerance rule is smooth_fixture's."""

import ctypes as C
import functools
import os

import numpy as np
import torch

from helpers import build_host_check, load_hostcheck
from hmm_fixture import (PRIOR, RMIN, _evidence, _floor, cols, default_start, fixed_theta, oracle_sample, rule_excess,  # noqa: F401
                         sampler_laws, state_pair_counts, synthetic_hmm, with_special_rows)
from multistart_fixture import forbid, full  # noqa: F401 (re-exported)
from rates_fixture import build_rates_check, host_indices  # noqa: F401 (re-exported)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "hostcheck", "mixture_check.cpp")
POP_SITE = 0xA05  # TQ_MIXTURE_SITE
MAX_POP = 4
UB_LIST = [(1, 1), (1, 2), (2, 2)]
N_LIST = [1, 6, 300]
G_LIST = [1, 2, 3, 4]
SAMPLER_F = [1, 2, 63, 64, 65, 129]
SAMPLER_S = [1, 64, 65, 200]

# the populations of the generator: kon, koff per frame
POPS = {"X": (0.05, 0.10), "Y": (0.05, 0.01), "I": (0.001, 0.10)}
# BIC of the float64 oracle at the 150th EM iteration (the trace's last entry), tol 0, from the default starts: (1, 1), (1, 2),
# G = 2 and G = 3 of (1, 1)
TABLE = {("XY", 0): (-6111.80, -6218.63, -6276.75, -6243.60), ("XY", 1): (-5834.39, -5892.45, -5970.15, -5932.98),
         ("XI", 0): (-3524.06, -3482.98, -3659.42, -3626.30), ("XI", 1): (-3640.29, -3593.27, -3786.08, -3748.91),
         ("dynamic", 0): (-6713.26, -6738.03, -6693.40, -6669.76)}
MODELS = (("u1b1", 1, 1, 1), ("u1b2", 1, 2, 1), ("g2", 1, 1, 2), ("g3", 1, 1, 3))  # name, U, B, G: the table's columns


# ---- inputs -----------------------------------------------------------------------------------------------------------
def two_state(kon, koff):
    return np.array([[1.0 - kon, kon], [koff, 1.0 - koff]])


def static_data(kind, s, F=300):
    """24 AOIs of population X at seed s, then 16 of population ``kind[1]`` (Y or I) at seed 100 + s: p float32 (40, F) and
    the generating population (40,) of every AOI, 0 for X."""
    a = synthetic_hmm(24, F, s, A=two_state(*POPS[kind[0]]))[0]
    b = synthetic_hmm(16, F, 100 + s, A=two_state(*POPS[kind[1]]))[0]
    return np.concatenate([a, b]), np.repeat([0, 1], [24, 16])


def data(kind, s):
    return (synthetic_hmm(40, 300, s)[0], None) if kind == "dynamic" else static_data(kind, s)


def mixture_default_start(U, B, G, allow=None):
    """The documented default start: population g is ``hmm_fixture.default_start`` with the off-diagonal entries of A
    divided by 4^g and the diagonal 1 minus their sum; forbidden entries zeroed, their rows renormalised; rho and phi
    uniform.  Returns (thetas (G, M * M + M), phi (G,))."""
    M = U + B
    free = full(M) if allow is None else np.asarray(allow, bool)
    thetas = np.zeros((G, M * M + M))
    for g in range(G):
        A = default_start(U, B)[: M * M].reshape(M, M).copy()
        for i in range(M):
            A[i, i] = 0.0
            A[i] = A[i] / 4.0 ** g
            A[i, i] = 1.0 - A[i].sum()
            if not free[i].all():
                A[i] = A[i] * free[i] / (A[i] * free[i]).sum()
        thetas[g] = np.concatenate([A.ravel(), np.full(M, 1.0 / M)])
    return thetas, np.full(G, 1.0 / G)


def normalised(thetas, M):
    """(..., M * M + M) after the normalisation ``mixture_fit`` applies once to a start: the expressions of ``hmm_fit``."""
    x = torch.as_tensor(np.asarray(thetas), dtype=torch.float64).reshape(-1, M * M + M)
    A, rho = x[:, : M * M].reshape(-1, M, M), x[:, M * M:]
    out = torch.stack([torch.cat([(A[r] / A[r].sum(1, keepdim=True)).reshape(-1), rho[r] / rho[r].sum()]) for r in range(len(x))])
    return out.numpy().reshape(np.asarray(thetas).shape).copy()


# ---- oracle -----------------------------------------------------------------------------------------------------------
def oracle_estep(p, thetas, U, B, prior, dtype=np.float64):
    """``hmm_fixture.oracle_estep`` for R chains at once: rows (R, N, M^2 + M + 1), filt and gamma (R, N, F, M) in
    ``dtype``: sequential scaled forward-backward, every chain on the same rows of ``p`` (N, F), or chain r on p[r] of
    (R, N, F)."""
    M = U + B
    thetas = np.asarray(thetas, np.float64).reshape(-1, M * M + M)
    R = len(thetas)
    A = _floor(thetas[:, : M * M].reshape(R, M, M), dtype)
    rho = _floor(thetas[:, M * M:], dtype)
    pr, one = dtype(np.float64(prior)), dtype(1)
    ell = _evidence(p, np.array([one / (one - pr), one / pr], dtype=dtype), U, B, dtype)
    ell = ell if ell.ndim == 4 else ell[None]  # (R or 1, N, F, M)
    N, F = ell.shape[1:3]
    a = np.zeros((R, N, F, M), dtype)
    loglik = np.zeros((R, N), dtype)
    for f in range(F):
        u = (rho[:, None, :] if f == 0 else a[:, :, f - 1] @ A) * ell[:, :, f]
        c = u.sum(-1)
        a[:, :, f] = u / c[..., None]
        loglik += np.log(c)
    gamma = np.zeros((R, N, F, M), dtype)
    beta = np.ones((R, N, M), dtype)
    gamma[:, :, F - 1] = a[:, :, F - 1]
    counts = np.zeros((R, N, M, M), dtype)
    At = np.swapaxes(A, 1, 2)
    for f in range(F - 2, -1, -1):
        w = ell[:, :, f + 1] * beta
        xi = a[:, :, f, :, None] * A[:, None] * w[:, :, None, :]
        counts += xi / xi.sum((2, 3))[..., None, None]
        beta = w @ At
        beta /= beta.sum(-1)[..., None]
        g = a[:, :, f] * beta
        gamma[:, :, f] = g / g.sum(-1)[..., None]
    rows = np.concatenate([counts.reshape(R, N, M * M), gamma[:, :, 0], loglik[..., None]], 2)
    return {"filt": a, "gamma": gamma, "rows": rows}


def oracle_resp(L, phi, dtype=np.float64):
    """ev (N,) and w (G, N) of the logliks L (G, N) under the weights phi, floored at 1e-9 and renormalised: the log of the
    sum over g ascending, shifted by its largest term, and every term's share of that sum."""
    lphi = np.log(_floor(np.asarray(phi, np.float64), dtype))
    a = lphi[:, None] + np.asarray(L).astype(dtype)
    mx = a.max(0)
    e = np.exp(a - mx)
    s = np.zeros(a.shape[1], dtype)
    for g in range(len(a)):
        s = s + e[g]
    return mx + np.log(s), e / s


def oracle_mstep(rows, thetas, phi, U, B, allow=None, dtype=np.float64):
    """The weighted M-step of one start: rows (G, N, COLS), thetas (G, M * M + M), phi (G,).  Returns new thetas, new phi,
    the mixture log evidence, w (G, N) and ev (N,), in ``dtype``."""
    M = U + B
    free = full(M) if allow is None else np.asarray(allow, bool)
    rows = np.asarray(rows).astype(dtype)
    G, N = rows.shape[:2]
    ev, w = oracle_resp(rows[:, :, -1], phi, dtype)
    new = np.asarray(thetas, np.float64).astype(dtype)
    wsum = w.sum(1)
    for g in range(G):
        if not wsum[g] > 0:
            continue
        s = (w[g][:, None] * rows[g, :, : M * M + M]).sum(0)
        s[: M * M] = np.where(free.ravel(), s[: M * M], dtype(0))
        for i in range(M):
            r = s[i * M:(i + 1) * M]
            if r.sum() > 0:
                new[g, i * M:(i + 1) * M] = _floor(r / r.sum(), dtype)
        new[g, M * M:] = _floor(s[M * M:] / wsum[g], dtype)
    return new, _floor(wsum / dtype(N), dtype), ev.sum(), w, ev


def oracle_em(p, prior, models, U, B, num_iter, allow=None, dtype=np.float64):
    """``num_iter`` EM iterations of several mixtures of (U, B) chains at once (one batched E-step per iteration): models is
    a list of (thetas0 (G, .), phi0 (G,)), and ``p`` (N, F) is shared or a list with the rows of every model, all of one
    shape.  Returns per model {"thetas" (num_iter + 1, G, .), "phi" (num_iter + 1, G),
    "trace" (num_iter,) in ``dtype``}; theta and phi are rounded to double between iterations, as the device's are."""
    out = [{"thetas": [np.array(t, np.float64)], "phi": [np.array(f, np.float64)], "trace": []} for t, f in models]
    sizes = [len(t) for t, _ in models]
    if isinstance(p, (list, tuple)):
        p = np.concatenate([np.repeat(np.asarray(x, np.float32)[None], G, 0) for x, G in zip(p, sizes)])
    for _ in range(num_iter):
        rows = oracle_estep(p, np.concatenate([o["thetas"][-1] for o in out]), U, B, prior, dtype)["rows"]
        at = 0
        for o, G in zip(out, sizes):
            th, ph, ll, _, _ = oracle_mstep(rows[at:at + G], o["thetas"][-1], o["phi"][-1], U, B, allow, dtype)
            o["thetas"].append(th.astype(np.float64))
            o["phi"].append(ph.astype(np.float64))
            o["trace"].append(ll)
            at += G
    return [{"thetas": np.array(o["thetas"]), "phi": np.array(o["phi"]), "trace": np.array(o["trace"], dtype=dtype)} for o in out]


def oracle_final(p, prior, thetas, phi, U, B, dtype=np.float64):
    """The mixture at (thetas, phi): log evidence, w (G, N), ev (N,)."""
    rows = oracle_estep(p, thetas, U, B, prior, dtype)["rows"]
    _, _, ll, w, ev = oracle_mstep(rows, thetas, phi, U, B, None, dtype)
    return ll, w, ev


def n_params(M, G, allow=None):
    free = M * M if allow is None else int(np.asarray(allow, bool).sum())
    return G * (free - M + M - 1) + G - 1


def bic(loglik, k, N, F):
    return -2.0 * loglik + k * np.log(N * F)


CHOICE_SETS = (("XY", 0), ("XY", 1), ("XI", 0), ("XI", 1), ("dynamic", 0))  # the data sets the model-choice tests run


@functools.lru_cache(maxsize=None)
def choice_cases():
    """The data sets of the model-choice tests: the oracle's 150 EM iterations (tol 0) of the table's four models from their
    default starts, in both precisions, all data sets side by side -- per data set and model the final log evidence, the
    BIC, the trace, the final parameters and responsibilities.  Computed once and left unchanged."""
    sets = {key: data(*key) for key in CHOICE_SETS}
    out = {key: {"p": p, "labels": labels} for key, (p, labels) in sets.items()}
    for dtype, tag in ((np.float64, "64"), (np.longdouble, "80")):
        for U, B in ((1, 1), (1, 2)):
            jobs = [(key, name, G) for key in CHOICE_SETS for name, u, b, G in MODELS if (u, b) == (U, B)]
            fits = oracle_em([sets[key][0] for key, _, _ in jobs], PRIOR, [mixture_default_start(U, B, G) for _, _, G in jobs],
                             U, B, 150, None, dtype)
            for (key, name, G), fit in zip(jobs, fits):
                p = sets[key][0]
                ll, w, _ = oracle_final(p, PRIOR, fit["thetas"][-1], fit["phi"][-1], U, B, dtype)
                out[key][name + "_" + tag] = {"loglik": ll, "bic": bic(ll, n_params(U + B, G), *p.shape), "trace": fit["trace"],
                                              "bic_trace": bic(fit["trace"][-1], n_params(U + B, G), *p.shape), "w": w, "thetas": fit["thetas"][-1], "phi": fit["phi"][-1]}
    return out


def choice_case(kind, s):
    return choice_cases()[(kind, s)]


GOLDEN = os.path.join(ROOT, "tests", "golden", "mixture_golden.npz")
GOLDEN_COLS = ("bic64", "bic80_hi", "bic80_lo", "bic_trace64", "trace_bound", "bic_trace80_hi", "bic_trace80_lo")


def trace_drop_bound(tr64, tr80):
    """The rule's bound for a trace, 32 max|X64 - X80| + 1e-13 max(1, max|X80|): no entry may lie below the one before it by
    more than this."""
    tr80 = np.asarray(tr80, np.longdouble)
    return float(32 * np.abs(np.asarray(tr64).astype(np.longdouble) - tr80).max() + 1e-13 * max(1.0, float(np.abs(tr80).max())))


def choice_summary():
    """What the model-choice tests need of ``choice_cases()``, as the arrays tests/golden/mixture_golden.npz records (written
    by tests/golden/make_mixture_golden.py): per data set and model the float64 BIC, the longdouble BIC as two doubles, the
    float64 BIC of the trace's last entry, the rule's bound of the trace, and the longdouble BIC of the trace's last entry as
    two doubles."""
    out = {}
    for (kind, s), case in choice_cases().items():
        for name, _, _, _ in MODELS:
            o64, o80 = case[name + "_64"], case[name + "_80"]
            hi, thi = float(o80["bic"]), float(o80["bic_trace"])
            out[f"{kind}{s}_{name}"] = np.array([float(o64["bic"]), hi, float(o80["bic"] - np.longdouble(hi)),
                                                 float(o64["bic_trace"]), trace_drop_bound(o64["trace"], o80["trace"]), thi,
                                                 float(o80["bic_trace"] - np.longdouble(thi))])
    return out


@functools.lru_cache(maxsize=None)
def choice_reference(kind, s):
    """The recorded oracle results of one data set: {model: {"bic64", "bic80" (longdouble), "bic_trace64", "bic_trace80",
    "trace_bound"}}.  test_mixture_host.py checks the record against the oracle."""
    with np.load(GOLDEN) as z:
        rows = {name: z[f"{kind}{s}_{name}"] for name, _, _, _ in MODELS}
    return {name: {"bic64": r[0], "bic80": np.longdouble(r[1]) + np.longdouble(r[2]), "bic_trace64": r[3], "trace_bound": r[4],
                   "bic_trace80": np.longdouble(r[5]) + np.longdouble(r[6])}
            for name, r in rows.items()}


@functools.lru_cache(maxsize=None)
def em_case():
    """(1, 1), G = 2 on X + Y at s = 0: the oracle's first 15 EM iterations from the default start in both precisions."""
    p, _ = static_data("XY", 0)
    start = mixture_default_start(1, 1, 2)
    o64 = oracle_em(p, PRIOR, [start], 1, 1, 15)[0]
    o80 = oracle_em(p, PRIOR, [start], 1, 1, 15, None, np.longdouble)[0]
    return {"p": p, "start": start, "o64": o64, "o80": o80}


def mstep_case(U, B, N, G, seed=0):
    """The shared M-step case: p (N, 65) (special rows at N = 6), P = 2 starts of G chains at ``fixed_theta`` seeds, phi of
    a seeded Dirichlet draw, and the oracle's E-step rows of every chain in both precisions."""
    M = U + B
    p = synthetic_hmm(N, 65, seed=N + seed)[0]
    if N == 6:
        p = with_special_rows(p, PRIOR)
    thetas = np.array([[fixed_theta(U, B, seed=q * G + g) for g in range(G)] for q in range(2)])
    phi = np.random.default_rng(10 * N + G).dirichlet(np.ones(G), 2)
    return {"p": p, "thetas": thetas, "phi": phi, "M": M}


def check_mstep(got, rows, case, U, B, allow, who, starts=(0,)):
    """theta, phi, resp, evidence and trace of the starts given against the oracle at the E-step rows the build used (its
    own ``rows`` (P, G, N, COLS)), by the rule; prints every excess and returns the largest."""
    worst = 0.0
    for q in starts:
        o64 = oracle_mstep(rows[q], case["thetas"][q], case["phi"][q], U, B, allow)
        o80 = oracle_mstep(rows[q], case["thetas"][q], case["phi"][q], U, B, allow, np.longdouble)
        for k, name in enumerate(("theta", "phi", "trace", "resp", "evidence")):
            exc = rule_excess(np.atleast_1d(got[name][q]), np.atleast_1d(o64[k]), np.atleast_1d(o80[k]))
            print(f"{who} start {q} {name}: {exc:.3g} of the bound")
            assert exc <= 1.0, (who, q, name, exc)
            worst = max(worst, exc)
    return worst


# ---- sampler ----------------------------------------------------------------------------------------------------------
def pop_uniforms(seed, S, N):
    """u (S, N) float32: the first uniform of Philox stream (seed, step = s, site 0xA05, elem = n), mapped as tq_uniform
    maps a word."""
    hc = load_hostcheck()
    hc.hc_philox.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint64, C.POINTER(C.c_uint32), C.c_int]
    hc.hc_philox.restype = None
    words = np.zeros((S, N), np.uint32)
    buf = (C.c_uint32 * 4)()
    for s in range(S):
        for n in range(N):
            hc.hc_philox(seed, s, POP_SITE, n, buf, 4)
            words[s, n] = buf[0]
    return ((words >> 8).astype(np.float32) * np.float32(2.0 ** -24) + np.float32(2.0 ** -25)).astype(np.float32)


def pop_tails(resp):
    """tail[g] (G, N) = resp[G - 1] + ... + resp[g], summed from the top in float64 as the kernel sums."""
    resp = np.asarray(resp, np.float64)
    tail = np.zeros_like(resp)
    run = np.zeros(resp.shape[1])
    for g in range(len(resp) - 1, -1, -1):
        run = run + resp[g]
        tail[g] = run
    return tail


def oracle_pop(resp, S, seed):
    """The replay of the population draws: pop (S, N) uint8 = the number of tails g >= 1 above u, and the smallest
    |u - tail| (inf for one population)."""
    G, N = np.asarray(resp).shape
    u = pop_uniforms(seed, S, N).astype(np.float64)
    tail = pop_tails(resp)[1:]  # (G - 1, N)
    if G == 1:
        return np.zeros((S, N), np.uint8), np.inf
    return (u[:, None, :] < tail[None]).sum(1).astype(np.uint8), float(np.abs(u[:, None, :] - tail[None]).min())


def oracle_mixture_sample(filt, thetas, resp, U, B, S, seed):
    """pop (S, N), raster (S, N, F) and the two margins of the sampler's replay in numpy: the population draw, then
    ``hmm_fixture.oracle_sample`` of the drawn population's chain."""
    pop, m_pop = oracle_pop(resp, S, seed)
    rasters, m_state = [], np.inf
    for g in range(len(thetas)):
        r, m = oracle_sample(filt[g], thetas[g], U, B, S, seed)
        rasters.append(r)
        m_state = min(m_state, m)
    rasters = np.stack(rasters)  # (G, S, N, F)
    s_ix, n_ix = np.meshgrid(np.arange(S), np.arange(pop.shape[1]), indexing="ij")
    return pop, rasters[pop, s_ix, n_ix], m_pop, m_state


def class_counts(raster, U):
    """The class-level counts (..., 4) of a raster (..., F) of hidden states in the layout of tq_rates_count: pairs 0 -> 1,
    frames in 0 with a successor, pairs 1 -> 0, frames in 1 with a successor."""
    z = (np.asarray(raster) >= U).astype(np.int64)
    now, nxt = z[..., :-1], z[..., 1:]
    return np.stack([((1 - now) * nxt).sum(-1), (1 - now).sum(-1), (now * (1 - nxt)).sum(-1), now.sum(-1)], -1)


def chi2_bound(dof, alpha=1e-6):
    """The upper alpha quantile of chi-square with ``dof`` degrees of freedom (Wilson-Hilferty, with the normal quantile by
    bisection on erfc)."""
    from math import erfc, sqrt

    lo, hi = 0.0, 10.0
    for _ in range(80):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if 0.5 * erfc(mid / sqrt(2.0)) > alpha else (lo, mid)
    z = 0.5 * (lo + hi)
    return dof * (1.0 - 2.0 / (9.0 * dof) + z * sqrt(2.0 / (9.0 * dof))) ** 3


def pop_law_chi2(pop, resp):
    """chi-square of the drawn populations (S, N) against S resp (G, N), over the cells with at least 5 expected draws
    (the others pooled per AOI), and its degrees of freedom."""
    pop, resp = np.asarray(pop), np.asarray(resp, np.float64)
    S = pop.shape[0]
    chi2, dof = 0.0, 0
    for n in range(resp.shape[1]):
        obs = np.bincount(pop[:, n], minlength=len(resp)).astype(np.float64)
        exp = S * resp[:, n] / resp[:, n].sum()
        big = exp >= 5.0
        o, e = list(obs[big]), list(exp[big])
        if (~big).any() and exp[~big].sum() >= 5.0:
            o.append(obs[~big].sum())
            e.append(exp[~big].sum())
        if len(e) >= 2:
            chi2 += float(((np.array(o) - np.array(e)) ** 2 / np.array(e)).sum())
            dof += len(e) - 1
    return chi2, dof


def oracle_estimate(trans, pop, G, M, indices=None):
    """totals (S, G, M * M) int64, members (S, G) int64 and estimand (S, G, M * M): a numpy sum over the drawn AOIs of every
    population; ``indices`` (S, N) resamples the AOIs."""
    trans, pop = np.asarray(trans).astype(np.int64), np.asarray(pop).astype(np.int64)
    if indices is not None:
        trans = np.take_along_axis(trans, np.asarray(indices)[:, :, None], 1)
        pop = np.take_along_axis(pop, np.asarray(indices), 1)
    sel = pop[:, None, :] == np.arange(G)[None, :, None]  # (S, G, N)
    totals = (sel[..., None] * trans[:, None]).sum(2)
    t = totals.reshape(len(trans), G, M, M).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        est = t / t.sum(-1, keepdims=True)
    return totals, sel.sum(2), est.reshape(len(trans), G, M * M)


# ---- g++ host check -----------------------------------------------------------------------------------------------------
def build_mixture_check(out_dir):
    """Compile tests/hostcheck/mixture_check.cpp into ``out_dir`` and bind it."""
    so = os.path.join(str(out_dir), "libtq_mixture_check.so")
    build_host_check(SRC, so)
    lib = C.CDLL(so)
    vp, i = C.c_void_p, C.c_int
    lib.hk_mixture_estep.argtypes = [vp, i, i, vp, i, i, i, i, C.c_double, vp, vp, vp]
    lib.hk_mixture_estep.restype = None
    lib.hk_mixture_mstep.argtypes = [vp, i, i, i, i, i, i, i, C.c_uint32, vp, vp, vp, vp, vp, vp]
    lib.hk_mixture_mstep.restype = None
    lib.hk_mixture_count.argtypes = [vp, vp, vp, i, i, i, i, i, i, C.c_uint64, vp, vp, vp, vp, vp]
    lib.hk_mixture_count.restype = None
    lib.hk_mixture_estimate.argtypes = [vp, vp, i, i, i, i, i, i, C.c_uint64, vp, vp, vp]
    lib.hk_mixture_estimate.restype = None
    return lib


def _active_ptr(active):
    if active is None:
        return None, None
    a = np.ascontiguousarray(active, dtype=np.int32)
    return a, a.ctypes.data


def allow_bits(allow, M):
    from tapqir_amd import _lib_multistart

    return _lib_multistart.allow_bits(full(M) if allow is None else allow)


def host_estep(lib, p, thetas, U, B, prior, active=None, rows=None, filt=None):
    """The g++ batched E-step of the chains ``thetas`` (P, G, .): rows (P, G, N, COLS), NaN-filled unless ``rows`` is given;
    ``active`` (P,) skips whole starts; ``filt`` (P, G, N, F, M) receives the a_f when given."""
    M = U + B
    p = np.ascontiguousarray(p, dtype=np.float32)
    thetas = np.ascontiguousarray(thetas, dtype=np.float64)
    (N, F), (P, G) = p.shape, thetas.shape[:2]
    rows = np.full((P, G, N, cols(M)), np.nan) if rows is None else rows
    filt = np.empty((P, G, N, F, M)) if filt is None else filt
    assert filt.shape == (P, G, N, F, M) and filt.flags.c_contiguous and rows.flags.c_contiguous
    keep, ptr = _active_ptr(active)
    lib.hk_mixture_estep(p.ctypes.data, N, F, thetas.ctypes.data, P, G, U, B, prior, ptr, filt.ctypes.data, rows.ctypes.data)
    return rows


def host_mstep(lib, rows, thetas, phi, trace, it, U, B, allow=None, active=None, resp=None, evidence=None):
    """The g++ weighted M-step: ``thetas`` (P, G, .), ``phi`` (P, G) and ``trace`` (P, T) float64 arrays updated in place;
    ``resp`` (P, G, N) and ``evidence`` (P, N) filled when given."""
    rows = np.ascontiguousarray(rows, dtype=np.float64)
    P, G, N = rows.shape[:3]
    keep, ptr = _active_ptr(active)
    lib.hk_mixture_mstep(rows.ctypes.data, N, P, G, trace.shape[1], it, U, B, allow_bits(allow, U + B), ptr, thetas.ctypes.data,
                         phi.ctypes.data, trace.ctypes.data, None if resp is None else resp.ctypes.data,
                         None if evidence is None else evidence.ctypes.data)
    return thetas


def host_mstep_all(lib, rows, thetas, phi, U, B, allow=None, active=None, it=1, T=3):
    """One M-step on copies, with every output NaN-filled first: dict of theta, phi, trace (P,), resp, evidence, traces."""
    P, G, N = rows.shape[:3]
    th, ph = np.array(thetas, np.float64, order="C"), np.array(phi, np.float64, order="C")
    trace, resp, ev = np.full((P, T), np.nan), np.full((P, G, N), np.nan), np.full((P, N), np.nan)
    host_mstep(lib, rows, th, ph, trace, it, U, B, allow, active, resp, ev)
    return {"theta": th, "phi": ph, "trace": trace[:, it], "resp": resp, "evidence": ev, "traces": trace}


def host_fit(lib, p, prior, thetas0, phi0, U, B, allow=None, num_iter=200, tol=0.0, chunk=50):
    """``mixture_fit`` up to the choice of the best start with the g++ build in place of the kernels: the chunks and the
    freezing are ``mle_analysis.multistart_em``'s, run on host tensors.  Returns thetas (P, G, .), phi (P, G), traces
    (P, num_iter), iterations, converged, and logliks (P,), resp (P, G, N), evidence (P, N) of the closing E-step."""
    from tapqir_amd.utils.mle_analysis import multistart_em

    M = U + B
    p = np.ascontiguousarray(p, dtype=np.float32)
    thetas, phi = np.array(thetas0, dtype=np.float64, order="C"), np.array(phi0, dtype=np.float64, order="C")
    (P, G), N = thetas.shape[:2], len(p)
    rows = np.full((P, G, N, cols(M)), np.nan)
    trace = torch.full((P, num_iter), float("nan"), dtype=torch.float64)
    active = torch.ones(P, dtype=torch.int32)
    iterations, converged = multistart_em(
        lambda: host_estep(lib, p, thetas, U, B, prior, active.numpy(), rows),
        lambda it: host_mstep(lib, rows, thetas, phi, trace.numpy(), it, U, B, allow, active.numpy()), trace, active, num_iter,
        tol, chunk)
    host_estep(lib, p, thetas, U, B, prior, None, rows)
    closing = host_mstep_all(lib, rows, thetas, phi, U, B, allow, None, 0, 1)
    return {"thetas": thetas, "phi": phi, "traces": trace.numpy(), "iterations": iterations, "converged": converged,
            "logliks": closing["trace"], "resp": closing["resp"], "evidence": closing["evidence"]}


def host_count(lib, filt, thetas, resp, U, B, S, seed):
    """The g++ replay of tq_mixture_count: counts (S, N, 4), trans (S, N, M * M) int32, pop (S, N) and raster (S, N, F) uint8,
    and the margins (population draw, state draws)."""
    M = U + B
    filt = np.ascontiguousarray(filt, dtype=np.float64)
    thetas = np.ascontiguousarray(thetas, dtype=np.float64)
    resp = np.ascontiguousarray(resp, dtype=np.float64)
    G, N, F = filt.shape[:3]
    counts = np.full((S, N, 4), -1, np.int32)
    trans = np.full((S, N, M * M), -1, np.int32)
    pop = np.full((S, N), 255, np.uint8)
    raster = np.full((S, N, F), 255, np.uint8)
    margins = np.zeros(2)
    lib.hk_mixture_count(filt.ctypes.data, thetas.ctypes.data, resp.ctypes.data, U, B, G, S, N, F, seed, counts.ctypes.data,
                         trans.ctypes.data, pop.ctypes.data, raster.ctypes.data, margins.ctypes.data)
    return {"counts": counts, "trans": trans, "pop": pop, "raster": raster, "margins": margins}


def host_estimate(lib, trans, pop, G, U, B, resample, seed):
    """The g++ replay of tq_mixture_estimate: totals (S, G, M * M), members (S, G) int64 and estimand (S, G, M * M)."""
    M = U + B
    trans = np.ascontiguousarray(trans, dtype=np.int32)
    pop = np.ascontiguousarray(pop, dtype=np.uint8)
    S, N = trans.shape[:2]
    totals, members, est = np.zeros((S, G, M * M), np.int64), np.zeros((S, G), np.int64), np.zeros((S, G, M * M))
    lib.hk_mixture_estimate(trans.ctypes.data, pop.ctypes.data, S, N, G, U, B, int(resample), seed, totals.ctypes.data,
                            members.ctypes.data, est.ctypes.data)
    return totals, members, est


class HostBuild:
    """The g++ build behind the interface the shared cases drive: numpy in, numpy out."""

    name = "g++"

    def __init__(self, out_dir):
        from hmm_fixture import build_hmm_check
        from multistart_fixture import build_multistart_check

        self.lib = build_mixture_check(out_dir)
        self.multistart = build_multistart_check(out_dir)
        self.hmm = build_hmm_check(out_dir)

    def estep(self, p, thetas, U, B, active=None):
        return host_estep(self.lib, p, thetas, U, B, PRIOR, active)

    def filt(self, p, thetas, U, B):
        N, F = np.asarray(p).shape
        filt = np.empty((1, len(thetas), N, F, U + B))
        host_estep(self.lib, p, np.asarray(thetas)[None], U, B, PRIOR, None, None, filt)
        return filt[0]

    def mstep_all(self, rows, thetas, phi, U, B, allow=None, active=None, it=1, T=3):
        return host_mstep_all(self.lib, rows, thetas, phi, U, B, allow, active, it, T)

    def multistart_mstep(self, rows, thetas, U, B, allow=None):
        from multistart_fixture import host_mstep as single

        th, trace = np.array(thetas, np.float64), np.full((len(thetas), 3), np.nan)
        single(self.multistart, rows, th, trace, 1, U, B, allow)
        return th, trace[:, 1]

    def fit(self, p, thetas0, phi0, U, B, allow=None, num_iter=15, chunk=6):
        return host_fit(self.lib, p, PRIOR, thetas0, phi0, U, B, allow, num_iter, 0.0, chunk)

    def count(self, filt, thetas, resp, U, B, S, seed):
        return host_count(self.lib, filt, thetas, resp, U, B, S, seed)

    def hmm_count(self, filt, theta, U, B, S, seed):
        from hmm_fixture import host_count as single

        counts, trans, raster, _ = single(self.hmm, filt, theta, U, B, S, seed)
        return {"counts": counts, "trans": trans, "raster": raster}

    def estimate(self, trans, pop, G, U, B, resample, seed):
        return host_estimate(self.lib, trans, pop, G, U, B, resample, seed)

    def choice_fits(self, kind, s):
        """The four models of the table on one data set: 150 iterations, tol 0, one chunk."""
        p = data(kind, s)[0]
        out = {}
        for name, U, B, G in MODELS:
            th, ph = mixture_default_start(U, B, G)
            fit = self.fit(p, normalised(th, U + B)[None], ph[None], U, B, None, 150, 150)
            out[name] = {"loglik": fit["logliks"][0], "bic": bic(fit["logliks"][0], n_params(U + B, G), *p.shape),
                         "trace": fit["traces"][0], "resp": fit["resp"][0]}
        return out


# ---- the cases both builds run ------------------------------------------------------------------------------------------
def run_mstep_case(build, U, B, N, G):
    """P = 2 starts of G chains on N rows: both starts by the rule; resp sums to 1 within 4 ulp; start 1 inactive keeps its
    NaN-filled outputs; two runs give the same bits; at G = 1 theta and trace are bit-equal to the single-chain M-step."""
    M = U + B
    case = mstep_case(U, B, N, G)
    rows = build.estep(case["p"], case["thetas"], U, B)
    assert rows.shape == (2, G, N, cols(M)) and np.isfinite(rows).all()
    got = build.mstep_all(rows, case["thetas"], case["phi"], U, B)
    worst = check_mstep(got, rows, case, U, B, None, f"{build.name} ({U}, {B}) N = {N} G = {G}", (0, 1))
    assert np.abs(got["resp"].sum(1) - 1.0).max() <= 4 * np.spacing(1.0)
    assert np.isnan(got["traces"][:, [0, 2]]).all()
    A = got["theta"][..., : M * M].reshape(2, G, M, M)
    assert np.abs(A.sum(-1) - 1).max() <= 4 * np.spacing(1.0) and np.abs(got["phi"].sum(1) - 1).max() <= 4 * np.spacing(1.0)
    again = build.mstep_all(rows, case["thetas"], case["phi"], U, B)
    for key in ("theta", "phi", "trace", "resp", "evidence"):
        assert np.array_equal(again[key], got[key]), key
    frozen = build.mstep_all(rows, case["thetas"], case["phi"], U, B, None, np.array([1, 0], np.int32))
    assert np.array_equal(frozen["theta"][1], case["thetas"][1]) and np.array_equal(frozen["phi"][1], case["phi"][1])
    assert np.isnan(frozen["traces"][1]).all() and np.isnan(frozen["resp"][1]).all() and np.isnan(frozen["evidence"][1]).all()
    for key in ("theta", "phi", "trace", "resp", "evidence"):
        assert np.array_equal(frozen[key][0], got[key][0]), key
    if G == 1:
        th, tr = build.multistart_mstep(rows[:, 0], case["thetas"][:, 0], U, B)
        assert np.array_equal(th, got["theta"][:, 0]) and np.array_equal(tr, got["trace"])
        assert np.array_equal(got["resp"], np.ones((2, 1, N))) and np.array_equal(got["evidence"], rows[:, 0, :, -1])
        assert np.array_equal(got["phi"], np.ones((2, 1)))
    return worst


def run_mstep_masked_and_swapped(build, U=1, B=2, N=300, G=3):
    """The masked topology by the rule (forbidden entries at most 1e-9; bit-equal to the masked single-chain M-step at
    G = 1), and populations 0 and 2 swapped in the inputs: the outputs swapped, by the rule."""
    M = U + B
    allow = forbid(M, (M - 2, M - 1), (M - 1, M - 2))
    case = mstep_case(U, B, N, G)
    rows = build.estep(case["p"], case["thetas"], U, B)
    got = build.mstep_all(rows, case["thetas"], case["phi"], U, B, allow)
    check_mstep(got, rows, case, U, B, allow, f"{build.name} masked", (0, 1))
    A = got["theta"][..., : M * M].reshape(2, G, M, M)
    assert (A[..., ~allow] <= 1e-9).all() and (A[..., ~allow] > 0).all() and (A[..., allow] > 1e-4).all()
    one = mstep_case(U, B, N, 1)
    rows1 = build.estep(one["p"], one["thetas"], U, B)
    th, tr = build.multistart_mstep(rows1[:, 0], one["thetas"][:, 0], U, B, allow)
    got1 = build.mstep_all(rows1, one["thetas"], one["phi"], U, B, allow)
    assert np.array_equal(th, got1["theta"][:, 0]) and np.array_equal(tr, got1["trace"])

    perm = [2, 1, 0]
    swapped = {"thetas": case["thetas"][:, perm], "phi": case["phi"][:, perm]}
    got_s = build.mstep_all(np.ascontiguousarray(rows[:, perm]), swapped["thetas"], swapped["phi"], U, B)
    back = {"theta": got_s["theta"][:, perm], "phi": got_s["phi"][:, perm], "trace": got_s["trace"],
            "resp": got_s["resp"][:, perm], "evidence": got_s["evidence"]}
    check_mstep(back, rows, case, U, B, None, f"{build.name} swapped", (0, 1))


def run_hopeless_population(build, U=1, B=1, N=6, G=2):
    """A population with phi = 1e-9 whose chain explains nothing (it never leaves a state the rows leave all the time): its
    responsibilities are tiny but not zero in either precision (F = 65), its theta comes out of quotients of tiny sums, and
    every output is finite and within the rule."""
    case = mstep_case(U, B, N, G)
    case["thetas"][:, 1, :4] = [1.0 - 1e-9, 1e-9, 1e-9, 1.0 - 1e-9]
    case["thetas"][:, 1, 4:] = [1.0 - 1e-9, 1e-9]
    case["phi"][:] = [1.0 - 1e-9, 1e-9]
    rows = build.estep(case["p"], case["thetas"], U, B)
    got = build.mstep_all(rows, case["thetas"], case["phi"], U, B)
    for key in ("theta", "phi", "trace", "resp", "evidence"):
        assert np.isfinite(got[key]).all(), key
    print(f"{build.name}: largest responsibility of the hopeless population {got['resp'][:, 1].max():.3g}")
    assert 0 < got["resp"][:, 1, 2].max() < 1e-30  # the alternating row; the row that never binds leaves it 1e-6
    assert (got["theta"] > 0).all() and (got["phi"] > 0).all() and got["phi"][:, 1].max() < 1e-5
    check_mstep(got, rows, case, U, B, None, f"{build.name} hopeless", (0, 1))


def run_em_case(build):
    """(1, 1), G = 2 on X + Y at s = 0: 15 iterations in chunks of 6, 6 and 3 by the rule; the whole run in one chunk gives
    the same bits."""
    case = em_case()
    th0, ph0 = case["start"]
    fit = build.fit(case["p"], normalised(th0, 2)[None], ph0[None], 1, 1, None, 15, 6)
    assert fit["iterations"] == [15] and fit["converged"] == [False]
    exc = (rule_excess(fit["thetas"][0], case["o64"]["thetas"][15], case["o80"]["thetas"][15]),
           rule_excess(fit["phi"][0], case["o64"]["phi"][15], case["o80"]["phi"][15]),
           rule_excess(fit["traces"][0], case["o64"]["trace"], case["o80"]["trace"]))
    print(f"{build.name} EM after 15 iterations: theta {exc[0]:.3g}, phi {exc[1]:.3g}, trace {exc[2]:.3g} of the bound")
    assert max(exc) <= 1.0
    whole = build.fit(case["p"], normalised(th0, 2)[None], ph0[None], 1, 1, None, 15, 15)
    for key in ("thetas", "phi", "traces", "logliks", "resp", "evidence"):
        assert np.array_equal(whole[key], fit[key]), key
    return max(exc)


def run_choice_case(fits, kind, s, who):
    """``fits``: per model of the table {"bic", "trace", "resp"} of the build under test after 150 iterations.  The recorded
    float64 oracle reproduces the table to its last digit; the build's BIC of the trace's last entry -- the table's figure --
    and its BIC of the closing evidence both match the oracle's by the rule; on static data the two-population mixture at
    least 30 below both single chains, every AOI assigned to its generator with responsibility >= 0.9; on the dynamic chain
    (1, 2) at least 20 below the mixture; no trace entry lies below the one before it by more than the rule's bound."""
    ref = choice_reference(kind, s)
    worst = 0.0
    for k, (name, U, B, G) in enumerate(MODELS):
        o = ref[name]
        # the table's log evidence is the trace's last entry: at the parameters before the 150th M-step
        assert abs(o["bic_trace64"] - TABLE[(kind, s)][k]) <= 0.00501, (name, o["bic_trace64"])
        exc = rule_excess([fits[name]["bic"]], [o["bic64"]], [o["bic80"]])
        print(f"{who} {kind} s = {s} {name}: BIC {fits[name]['bic']:.6f}, {exc:.3g} of the bound")
        assert exc <= 1.0, (name, exc)
        worst = max(worst, exc)
        tr = np.asarray(fits[name]["trace"], np.float64)
        assert len(tr) == 150 and np.diff(tr).min() >= -o["trace_bound"], name
        N, F = data(kind, s)[0].shape
        table = bic(tr[-1], n_params(U + B, G), N, F)
        exc = rule_excess([table], [o["bic_trace64"]], [o["bic_trace80"]])
        print(f"{who} {kind} s = {s} {name}: the table's BIC {table:.6f}, {exc:.3g} of the bound, largest decrease of the "
              f"trace {max(0.0, -np.diff(tr).min()):.3g} against {o['trace_bound']:.3g}")
        assert exc <= 1.0 and abs(table - TABLE[(kind, s)][k]) <= 0.00501, (name, exc, table)
        worst = max(worst, exc)
    b = {name: fits[name]["bic"] for name, _, _, _ in MODELS}
    if kind == "dynamic":
        assert b["u1b2"] <= b["g2"] - 20.0
        return worst
    assert b["g2"] <= min(b["u1b1"], b["u1b2"]) - 30.0
    resp = np.asarray(fits["g2"]["resp"])
    pmap, labels = resp.argmax(0), data(kind, s)[1]
    assert np.array_equal(pmap, labels) or np.array_equal(pmap, 1 - labels)
    print(f"{who} {kind} s = {s}: smallest winning responsibility {resp.max(0).min():.4f}")
    assert resp.max(0).min() >= 0.9
    return worst


def sampler_inputs(build, U, B, G, F, N=6):
    """p (N, F) with the special rows, G chains at ``fixed_theta`` seeds, the build's own filt (G, N, F, M), and resp (G, N) of a
    seeded Dirichlet draw."""
    p = with_special_rows(synthetic_hmm(N, F, seed=F)[0], PRIOR)
    thetas = np.array([fixed_theta(U, B, seed=g) for g in range(G)])
    resp = np.ascontiguousarray(np.random.default_rng(100 * F + G).dirichlet(np.ones(G), N).T)
    return p, thetas, build.filt(p, thetas, U, B), resp


def check_sample(out, ref, U, M):
    """A sampler's outputs against a reference's pop and raster, bit for bit, and trans and counts against their own raster."""
    assert np.array_equal(out["pop"], ref["pop"]) and np.array_equal(out["raster"], ref["raster"])
    F = out["raster"].shape[-1]
    assert np.array_equal(out["trans"], state_pair_counts(out["raster"], M) if F > 1 else np.zeros_like(out["trans"]))
    assert np.array_equal(out["counts"], class_counts(out["raster"], U))
