"""Test-side helpers of the censored dwell-time tests: the g++ build of tq_censored.h, float64 restatements (the
log-likelihood of ``dwell_fixture.loglik64`` extended by the censored sum, the product-limit survival in numpy), the rows
and references of the one-step tests, and the simulated two-state chain that shows what the feature is for.

The one-step tests use the method and the rule of kinetics_boundary_fixture.py unchanged (a first step from zero moments
taken apart into gradient, loss and update; per row |g - g64| <= max(32 max_j |g32 - g64|, 1e-6 max_j |g64|))."""

import ctypes as C
import functools
import os

import numpy as np
import torch

import dwell_fixture
import kinetics_boundary_fixture as kb
from helpers import adam64, build_host_check

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "hostcheck", "censored_check.cpp")


def build_censored_check(out_dir):
    """Compile tests/hostcheck/censored_check.cpp into ``out_dir`` and bind it."""
    so = os.path.join(str(out_dir), "libtq_censored_check.so")
    build_host_check(SRC, so)
    lib = C.CDLL(so)
    vp = C.c_void_p
    lib.hk_censored_pair.argtypes = [vp, C.c_int, C.c_float, C.c_float, vp]
    lib.hk_censored_pair.restype = C.c_int
    lib.hk_survival.argtypes = [vp, vp, C.c_int, C.c_int, vp]
    lib.hk_survival.restype = None
    lib.hk_censored_fit_steps.argtypes = [C.c_int, vp, vp, vp, vp, vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_double,
                                          C.c_double, C.c_double, C.c_double]
    lib.hk_censored_fit_steps.restype = C.c_int
    return lib


# ---- float64 restatements ---------------------------------------------------------------------------------------------
def logsurv64(par, cdata, K):
    """Per-sample sum of log S(t) = log sum_j A_j exp(-k_j t) over the censored times: par (S, 2K) = (log k, softmax
    logits), cdata (S, Mc) padded with -1 (entries >= 0 count; t = 0 is a valid time with the term log 1)."""
    logk, a = par[:, :K], par[:, K:]
    logA = torch.log_softmax(a, dim=1)
    t = cdata.clamp(min=0).unsqueeze(-1)
    terms = torch.logsumexp(logA.unsqueeze(1) - logk.exp().unsqueeze(1) * t, dim=-1)
    return torch.where(cdata >= 0, terms, torch.zeros_like(terms)).sum(1)


def loglik64(par, data, cdata, K):
    """``dwell_fixture.loglik64`` of the complete dwell times ``data`` (S, M), padded with zeros, plus ``logsurv64`` of the
    censored times ``cdata`` (S, Mc), padded with -1."""
    return dwell_fixture.loglik64(par, data, K) + logsurv64(par, cdata, K)


def torch_fit64(data, cdata, K, n_steps=300, lr=5e-3):
    """The censored fit restated in float64 torch: autograd + torch.optim.Adam from the reference's initial values."""
    data, cdata = data.double().cpu(), cdata.double().cpu()
    p = adam64(dwell_fixture.init_par(data.shape[0], K), lambda par: loglik64(par, data, cdata, K), n_steps, lr)
    return {"k": p[:, :K].exp(), "A": torch.softmax(p[:, K:], dim=1), "par": p}


def censored_csr(cdata):
    """(values, weights, row_ptr) on the host of the -1-padded censored times ``cdata`` (S, Mc), each with weight 1."""
    keep = cdata >= 0
    row_ptr = torch.zeros(cdata.shape[0] + 1, dtype=torch.int64)
    row_ptr[1:] = torch.cumsum(keep.sum(1), 0)
    vals = cdata[keep].float().contiguous()
    if vals.numel() == 0:
        vals = torch.zeros(1)
    return vals, torch.ones_like(vals), row_ptr


def empty_csr(S):
    """A censored CSR of S empty rows (valid pointers, nothing in them)."""
    return torch.zeros(1), torch.zeros(1), torch.zeros(S + 1, dtype=torch.int64)


def survival_numpy(hist, cens):
    """Product-limit survival of (R, F) integer histograms in numpy float64: the definition, one factor after the other."""
    hist, cens = np.asarray(hist, np.int64), np.asarray(cens, np.int64)
    R, F = hist.shape
    surv = np.ones((R, F), np.float64)
    for r in range(R):
        prod = 1.0
        for u in range(1, F):
            Y = int(hist[r, u:].sum() + cens[r, u + 1:].sum())
            if Y > 0:
                prod = prod * (float(Y - int(hist[r, u])) / float(Y))
            surv[r, u] = prod
    return surv


# ---- one step taken apart: rows, states, reference -----------------------------------------------------------------------
# (complete, censored) pairs per row: around the 64-lane round and around TQ_DWELL_LDS_PAIRS = 2048 on the SUM
CENS_LENS = ((0, 0), (1, 0), (0, 1), (1, 1), (63, 1), (64, 64), (65, 63), (2000, 48), (2000, 49), (2048, 0), (0, 2049),
             (4097, 4097))
CENS_STATES = kb.DWELL_STATES


def _csr_of(parts):
    row_ptr = torch.zeros(len(parts) + 1, dtype=torch.int64)
    row_ptr[1:] = torch.cumsum(torch.tensor([len(t) for t, _ in parts]), 0)
    return torch.cat([t for t, _ in parts]).contiguous(), torch.cat([w for _, w in parts]).contiguous(), row_ptr


@functools.lru_cache(maxsize=None)
def censored_rows():
    """(csr, ccsr) of one row per entry of CENS_LENS.  Complete pairs as ``kb.dwell_rows``: rounded mixture draws >= 1, the
    last of two or more an outlier at t = 1e4.  Censored pairs: rounded draws >= 1; a list of two or more starts with a
    pair at t = 0 and ends with one at t = 1e4.  Even rows have unit weights, odd rows integer weights 1 .. 50 with one
    weight of 1e4 in each list."""
    gen = torch.Generator().manual_seed(20261020)
    full, cens = [], []
    for r, (n, nc) in enumerate(CENS_LENS):
        t = kb.dwell_draws(gen, 1, max(n, 1))[0, :n].round().clamp(min=1.0)
        tc = kb.dwell_draws(gen, 1, max(nc, 1))[0, :nc].round().clamp(min=1.0)
        w, wc = torch.ones(n), torch.ones(nc)
        if r % 2 == 1:
            if n:
                w = torch.randint(1, 51, (n,), generator=gen).float()
                w[0] = 1.0e4
            if nc:
                wc = torch.randint(1, 51, (nc,), generator=gen).float()
                wc[nc // 2] = 1.0e4
        if n >= 2:
            t[-1] = kb.OUTLIER
        if nc >= 2:
            tc[0] = 0.0
            tc[-1] = kb.OUTLIER
        full.append((t, w))
        cens.append((tc, wc))
    return _csr_of(full), _csr_of(cens)


def censored_par0(K, kind):
    return kb.dwell_par0(K, kind, S=len(CENS_LENS))


def _autograd(par0, csr, ccsr, K, dtype):
    (values, weights, row_ptr), (cvalues, cweights, crow_ptr) = csr, ccsr
    par = par0.to(dtype).clone().requires_grad_(True)
    lls = []
    for s in range(par.shape[0]):
        ll = par[s].sum() * 0.0
        a, b = int(row_ptr[s]), int(row_ptr[s + 1])
        if b > a:  # every pair as a sample of its own: the per-pair terms, weighted and summed here
            terms = dwell_fixture.loglik64(par[s].expand(b - a, 2 * K), values[a:b].to(dtype).unsqueeze(1), K)
            ll = ll + (weights[a:b].to(dtype) * terms).sum()
        a, b = int(crow_ptr[s]), int(crow_ptr[s + 1])
        if b > a:
            terms = logsurv64(par[s].expand(b - a, 2 * K), cvalues[a:b].to(dtype).unsqueeze(1), K)
            ll = ll + (cweights[a:b].to(dtype) * terms).sum()
        lls.append(ll)
    ll = torch.stack(lls)
    (-ll.sum()).backward()
    return par.grad.detach(), (-ll).detach()


def reference_at(par0, csr, ccsr, K):
    """Gradient (S, 2K) and loss (S,) of the LOSS at float32 parameters ``par0``: float64 and float32 autograd of the
    restated log-likelihood."""
    g64, loss64 = _autograd(par0, csr, ccsr, K, torch.float64)
    g32, loss32 = _autograd(par0, csr, ccsr, K, torch.float32)
    return {"g64": g64, "g32": g32, "loss64": loss64, "loss32": loss32}


@functools.lru_cache(maxsize=None)
def censored_reference(K, kind):
    return reference_at(censored_par0(K, kind), *censored_rows(), K)


def host_censored_steps(lib, state, csr, ccsr, K, step0=0, n_steps=1, lr=kb.LR):
    """One launch of the g++ replay from ``state`` (S, 6K): (state after, loss (S,))."""
    parts = [x.contiguous() if x.numel() else torch.zeros(1, dtype=x.dtype) for x in (*csr, *ccsr)]
    state = state.clone().contiguous()
    S = parts[2].shape[0] - 1
    loss = torch.full((S,), float("nan"))
    rc = lib.hk_censored_fit_steps(K, *(x.data_ptr() for x in parts), state.data_ptr(), loss.data_ptr(), S, step0, n_steps,
                                   lr, kb.BETA1, kb.BETA2, kb.ADAM_EPS)
    assert rc == 0, K
    return state, loss


# ---- trajectories ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def trajectory_data():
    """4 rows of 300 rounded mixture draws, 30 % of them censored at a random time before their end: (data (4, 300)
    zero-padded complete dwell times >= 1, cdata (4, 300) censored times >= 0 padded with -1)."""
    gen = torch.Generator().manual_seed(31)
    T = kb.dwell_draws(gen, 4, 300)
    cut = torch.rand(4, 300, generator=gen) < 0.3
    when = torch.rand(4, 300, generator=gen)
    data = torch.where(cut, torch.zeros_like(T), T.round().clamp(min=1.0))
    cdata = torch.where(cut, (T * when).floor(), -torch.ones_like(T))
    data[1, 250:] = 0.0  # padding in both lists
    cdata[1, 250:] = -1.0
    return data, cdata


@functools.lru_cache(maxsize=None)
def trajectory_reference(K, n_steps=300):
    return torch_fit64(*trajectory_data(), K, n_steps=n_steps)


# ---- what the feature is for --------------------------------------------------------------------------------------------
CHAIN = dict(N=200, F=300, kon=0.02, koff=0.01)
# chosen on the CPU (the first seed from 0 for which the generating raster alone satisfies the three conditions of the test)
CHAIN_SEED = 0


def two_state_raster(seed, N=CHAIN["N"], F=CHAIN["F"], kon=CHAIN["kon"], koff=CHAIN["koff"]):
    """(N, F) 0/1 raster of a stationary two-state chain with per-frame probabilities kon = P(0 -> 1), koff = P(1 -> 0)."""
    rng = np.random.default_rng(seed)
    z = np.zeros((N, F), np.uint8)
    z[:, 0] = rng.random(N) < kon / (kon + koff)
    u = rng.random((N, F))
    for f in range(1, F):
        z[:, f] = np.where(z[:, f - 1] == 1, u[:, f] >= koff, u[:, f] < kon)
    return z


def raster_histograms(z):
    """(hist_bound, cens_bound) (F,) int64 of a (N, F) raster by the definition: bound runs that open inside the record,
    by length; complete when they also close inside it, open when they reach the last frame."""
    N, F = z.shape
    hist, cens = np.zeros(F, np.int64), np.zeros(F, np.int64)
    for row in z:
        edges = np.flatnonzero(np.diff(row.astype(np.int8))) + 1  # first frames of the runs after the first
        starts = np.concatenate([[0], edges])
        stops = np.concatenate([edges, [F]])
        for a, b in zip(starts, stops):
            if row[a] == 1 and a > 0:
                (cens if b == F else hist)[b - a] += 1
    return hist, cens


def closed_form_rates(hist, cens):
    """(interior-only 1 / mean(d), censored n / (sum d + sum (d_open - 1)), n_complete) of one pair of histograms."""
    d = np.arange(len(hist), dtype=np.float64)
    n = float(hist.sum())
    return n / (hist * d).sum(), n / ((hist * d).sum() + (cens[2:] * (d[2:] - 1.0)).sum()), n


def chain_conditions(hist, cens, surv50, koff=CHAIN["koff"]):
    """The three conditions of the issue from the counts: the censored estimate within 3 k / sqrt(n) of koff, the
    interior-only one more than that above it, and the survival at t = 50 within 3 sigma of exp(-50 koff) with
    sigma = exp(-50 koff) 50 koff / sqrt(n) (the delta method from the rate's sigma).  Returns (ok, figures)."""
    k_int, k_cens, n = closed_form_rates(hist, cens)
    band = 3.0 * koff / np.sqrt(n)
    s_true = np.exp(-50.0 * koff)
    s_band = 3.0 * s_true * 50.0 * koff / np.sqrt(n)
    ok = abs(k_cens - koff) <= band and k_int - koff > band and abs(surv50 - s_true) <= s_band
    return ok, dict(k_int=k_int, k_cens=k_cens, n=n, band=band, surv50=surv50, s_true=s_true, s_band=s_band)
