"""
Dwell times with the open last run on the HIP device (``dwelltime --censored``).

``dwelltime`` fits the interior runs of the posterior rasters; a run that is still open at the last frame is dropped, which
keeps short dwells and discards long ones.  Here such a run, when it opened inside the record, enters as a right-censored
observation:

* ``dwell_censored_hist``: the histograms of the open last runs, counted from the device interval table that
  ``dwell_intervals`` and its kin return with ``device_table=True`` (``tq_dwell_censored_hist``);
* ``dwell_csr_from_censored_hist``: their (t, weight) pairs, t = seen frames - 1;
* ``dwell_censored_fit_steps`` / ``dwell_censored_fit``: the K-exponential fit of ``dwell_fit`` with the survival term
  ``log sum_j A_j exp(-k_j t)`` of every censored pair (``tq_dwell_censored_fit``);
* ``dwell_survival``: the product-limit (Kaplan-Meier) curve of every row of histograms (``tq_dwell_survival``);
* ``dwell_censored_rate`` / ``mixture_survival``: the closed-form K = 1 estimate and the fitted survival curve, host-side
  arithmetic on the results that runs anywhere.

First runs (``start_frame == 0``, a run that spans the record included) are used by neither part: their start was not
observed.  There is no CPU path: the entry points raise ``HipExtensionError`` off the device.
"""

import ctypes as C

import torch

from tapqir_amd import _lib, _lib_censored
from tapqir_amd.exceptions import HipExtensionError
from tapqir_amd.utils.mle_analysis import (ADAM_BETAS, ADAM_EPS, _check_K, _csr, _device_tensor, _run_chunks, _stream,
                                           dwell_init_state)


def _device_ints(x, what, dtype):
    if not isinstance(x, torch.Tensor) or x.device.type != "cuda":
        raise HipExtensionError(f"{what} runs on the HIP device only (no CPU fallback): pass a cuda tensor")
    return x.detach().to(dtype).contiguous()


def dwell_censored_hist(table, S, N, F, pop=None, populations=None):
    """Histograms of the open last runs of an interval table.

    ``table``: the (DWELL_COLS, total) int32 device table of ``dwell_intervals`` / ``smooth_dwell_intervals`` /
    ``hmm_dwell_intervals`` / ``mixture_dwell_intervals`` (``device_table=True``) for S samples of N AOIs and F frames.
    Every run with ``low_or_high`` 2 / 3 and ``start_frame > 0`` adds 1 at ``[s, dwell_time]`` of ``"cens_unbound"`` /
    ``"cens_bound"``, (S, F) int32 on the device.  With ``pop`` (S, N) uint8 -- ``mixture_dwell_sample``'s -- and
    ``populations`` = G the histograms are (S, G, F), kept apart by ``pop[s, aoi]``."""
    table = _device_ints(table, "dwell_censored_hist", torch.int32)
    if table.ndim != 2 or table.shape[0] != _lib.DWELL_COLS:
        raise ValueError(f"dwell_censored_hist: table must be ({_lib.DWELL_COLS}, total), got {tuple(table.shape)}")
    S, N, F = int(S), int(N), int(F)
    if (pop is None) != (populations is None):
        raise ValueError("dwell_censored_hist: pop and populations go together")
    G = 1 if populations is None else int(populations)
    if S < 1 or N < 1 or F < 1 or not 1 <= G <= _lib_censored.CENSORED_MAX_G:
        raise ValueError(f"dwell_censored_hist: S, N, F must be positive and populations in 1 .. "
                         f"{_lib_censored.CENSORED_MAX_G}, got {(S, N, F, G)}")
    if pop is not None:
        pop = _device_ints(pop, "dwell_censored_hist", torch.uint8)
        if pop.shape != (S, N):
            raise ValueError(f"dwell_censored_hist: pop must be ({S}, {N}), got {tuple(pop.shape)}")
    total = table.shape[1]
    shape = (S, F) if populations is None else (S, G, F)
    cb = torch.zeros(shape, dtype=torch.int32, device=table.device)
    cu = torch.zeros(shape, dtype=torch.int32, device=table.device)
    a = _lib_censored.DwellCensoredHistArgs(intervals=_lib.ptr(table) if total else None, pop=_lib.ptr(pop),
                                            cens_bound=_lib.ptr(cb), cens_unbound=_lib.ptr(cu), total=total, S=S, N=N, F=F,
                                            G=G)
    _lib.check(_lib_censored.lib().tq_dwell_censored_hist(C.byref(a), _stream(table.device)), "tq_dwell_censored_hist")
    return {"cens_bound": cb, "cens_unbound": cu}


def dwell_csr_from_censored_hist(cens):
    """(values, weights, row_ptr) of the censored pairs of per-sample histograms ``cens`` (S, F) of open last runs:
    value = bin - 1 (a run seen in d frames has made d - 1 stays), weight = its count.  Bins 0 and 1 are dropped: an open
    run of one frame (t = 0) carries no information."""
    h = cens.to(torch.float32)
    nz = h > 0
    nz[:, :2] = False
    t = torch.arange(h.shape[1], dtype=torch.float32, device=h.device).expand_as(h) - 1.0
    return _csr(t[nz], h[nz], nz.sum(1))


def _csr_on_device(csr, who):
    values, weights, row_ptr = csr
    values = _device_tensor(values, who)
    weights = _device_tensor(weights, who)
    if not isinstance(row_ptr, torch.Tensor) or row_ptr.device.type != "cuda":
        raise HipExtensionError(f"{who} runs on the HIP device only (no CPU fallback): pass cuda tensors")
    return values, weights, row_ptr.to(torch.int64).contiguous()


def dwell_censored_fit_steps(state, csr, ccsr, K, lr=5e-3, step0=0, n_steps=1, loss=None, stage_lds=True):
    """One launch of ``tq_dwell_censored_fit``: Adam steps ``step0 + 1 .. step0 + n_steps`` of every fit, in place on
    ``state`` (S, 6K).  ``csr`` = (values, weights, row_ptr) of the complete dwell times and ``ccsr`` of the censored
    times, for the same rows, on the device; ``loss`` (S,) receives the loss of the last step."""
    K = _check_K(K)
    values, weights, row_ptr = _csr_on_device(csr, "dwell_censored_fit")
    cvalues, cweights, crow_ptr = _csr_on_device(ccsr, "dwell_censored_fit")
    S = row_ptr.shape[0] - 1
    if crow_ptr.shape[0] != S + 1:
        raise ValueError(f"dwell_censored_fit: the censored CSR has {crow_ptr.shape[0] - 1} rows, the complete one {S}")
    if state.shape != (S, 6 * K) or state.dtype != torch.float32 or not state.is_contiguous():
        raise ValueError(f"dwell_censored_fit: state must be contiguous float32 ({S}, {6 * K}), got {tuple(state.shape)}")
    a = _lib_censored.DwellCensoredFitArgs(
        values=_lib.ptr(values), weights=_lib.ptr(weights), row_ptr=_lib.ptr(row_ptr), cvalues=_lib.ptr(cvalues),
        cweights=_lib.ptr(cweights), crow_ptr=_lib.ptr(crow_ptr), state=_lib.ptr(state), loss=_lib.ptr(loss), S=S, K=K,
        step0=int(step0), n_steps=int(n_steps), stage_lds=1 if stage_lds else 0, lr=float(lr), beta1=ADAM_BETAS[0],
        beta2=ADAM_BETAS[1], eps=ADAM_EPS)
    _lib.check(_lib_censored.lib().tq_dwell_censored_fit(C.byref(a), _stream(values.device)), "tq_dwell_censored_fit")
    return state


def dwell_censored_fit(csr, ccsr, K=3, lr=5e-3, n_steps=10000, chunk=1000, progress_bar=None, stage_lds=True):
    """Maximum-likelihood fit of a K-exponential mixture to every row's complete dwell times ``csr`` (such as
    ``dwell_csr_from_hist(hist)``) and right-censored times ``ccsr`` (``dwell_csr_from_censored_hist(cens)``): ``dwell_fit``
    with the loss ``-sum w log f(t) - sum wc log S(tc)``.  Returns ``{"k", "A"}``, each (S, K) float32 on the device, and
    ``"loss"`` (S,): the loss of the last step.  A row without data of either kind keeps its initial values; the result
    does not depend on ``chunk``."""
    K = _check_K(K)
    csr, ccsr = tuple(csr), tuple(ccsr)
    for part in (csr, ccsr):
        if not isinstance(part[2], torch.Tensor) or part[2].device.type != "cuda":
            raise HipExtensionError("dwell_censored_fit runs on the HIP device only (no CPU fallback): pass cuda tensors")
    S = csr[2].shape[0] - 1
    dev = csr[2].device
    state = dwell_init_state(S, K, dev)
    loss = torch.full((S,), float("nan"), dtype=torch.float32, device=dev)
    _run_chunks(lambda step0, n: dwell_censored_fit_steps(state, csr, ccsr, K, lr, step0, n, loss, stage_lds), n_steps,
                chunk, progress_bar)
    return {"k": state[:, :K].exp(), "A": torch.softmax(state[:, K:2 * K], dim=1), "loss": loss}


def dwell_survival(hist, cens):
    """The product-limit (Kaplan-Meier) survival curve of every row: ``hist`` and ``cens`` (R, F) (or (F,)) integer
    histograms of the complete runs and of the open last runs by number of frames, on the device.  Returns ``surv``
    (R, F) float64: ``surv[r, 0] = 1`` and ``surv[r, t] = prod_{u <= t} (Y_u - h_u) / Y_u`` with
    ``Y_u = sum_{d >= u} h_d + sum_{d >= u + 1} c_d`` runs at risk (a factor of 1 where none is)."""
    hist = _device_ints(hist, "dwell_survival", torch.int32)
    cens = _device_ints(cens, "dwell_survival", torch.int32)
    hist = hist[None] if hist.ndim == 1 else hist
    cens = cens[None] if cens.ndim == 1 else cens
    if hist.ndim != 2 or hist.shape != cens.shape or hist.shape[0] < 1 or not 1 <= hist.shape[1] <= _lib_censored.SURVIVAL_MAX_F:
        raise ValueError(f"dwell_survival: hist and cens must both be (R, F) with R >= 1 and 1 <= F <= "
                         f"{_lib_censored.SURVIVAL_MAX_F}, got {tuple(hist.shape)} and {tuple(cens.shape)}")
    R, F = hist.shape
    surv = torch.empty(R, F, dtype=torch.float64, device=hist.device)
    a = _lib_censored.DwellSurvivalArgs(hist=_lib.ptr(hist), cens=_lib.ptr(cens), surv=_lib.ptr(surv), R=R, F=F)
    _lib.check(_lib_censored.lib().tq_dwell_survival(C.byref(a), _stream(hist.device)), "tq_dwell_survival")
    return surv


def dwell_censored_rate(hist, cens=None):
    """The closed-form K = 1 maximiser per row, float64: ``n_complete / (sum d h_d + sum (d - 1) c_d)``, the
    maximum-likelihood estimate of the per-frame leaving probability of a geometric dwell; without ``cens`` it is the
    interior-only ``1 / mean(d)``.  NaN for a row without a complete run.  Plain torch on (R, F) numbers: runs anywhere."""
    h = hist.double()
    d = torch.arange(h.shape[-1], dtype=torch.float64, device=h.device)
    n = h[..., 1:].sum(-1)
    exposure = (h * d)[..., 1:].sum(-1)
    if cens is not None:
        exposure = exposure + (cens.double() * (d - 1.0))[..., 2:].sum(-1)
    return torch.where(n > 0, n / exposure.clamp(min=1.0), torch.full_like(n, float("nan")))


def mixture_survival(A, k, t):
    """``sum_j A_j exp(-k_j t)`` of one set of parameters (sequences of K numbers) at the times ``t`` (a tensor):
    the survival function of the fitted mixture.  Runs anywhere."""
    t = torch.as_tensor(t, dtype=torch.float64)
    A = torch.as_tensor(A, dtype=torch.float64).reshape(-1, 1)
    k = torch.as_tensor(k, dtype=torch.float64).reshape(-1, 1)
    return (A * torch.exp(-k * t.reshape(1, -1))).sum(0)
