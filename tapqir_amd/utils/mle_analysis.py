"""
Kinetics analysis on the HIP device (tapqir/utils/mle_analysis.py, the ``ttfb`` / ``dwelltime`` commands,
tapqir/main.py:926-1384, and the two-state rates of tapqir/utils/imscroll.py:199-317):

* ``ttfb_sample``: posterior samples of the first-binding frame of each AOI (``tq_ttfb_sample``);
* ``ttfb_fit``: one maximum-likelihood fit of the censored two-exponential model (Friedman & Gelles 2015) per sample,
  ``train(ttfb_model, ttfb_guide, lr, n_steps)`` of the reference (``tq_ttfb_fit``);
* ``fraction_bound`` / ``fraction_bound_fit``: the per-time statistics the command writes;
* ``dwell_sample`` / ``dwell_intervals``: interior dwell-time histograms and the interval table of posterior rasters
  drawn and walked on the device (``count_intervals(z_sample)`` of the ``dwelltime`` command, ``tq_dwell_sample``);
* ``dwell_fit``: one maximum-likelihood fit of the K-exponential mixture per sample, ``train(exp_model, exp_guide, lr,
  n_steps, data, K)`` of the reference (``tq_dwell_fit``);
* ``rates_sample`` / ``rates_estimate`` / ``rates_summary``: the transition counts of posterior rasters (the rasters of
  ``dwell_sample`` at the same seed), their pooled or AOI-resampled totals with kon = P(0 -> 1) and koff = P(1 -> 0) per
  frame, and mean and percentile interval of those -- ``posterior_estimate`` / ``sample_and_bootstrap`` of
  tapqir/utils/imscroll.py:278-317 with ``association_rate`` / ``dissociation_rate`` (``tq_rates_count``,
  ``tq_rates_estimate``);
* ``smooth_estep`` / ``smooth_fit`` / ``smooth_viterbi`` / ``smooth_sample``: a two-state hidden Markov chain over the
  frames with the fit's ``z_probs`` as evidence -- forward-backward marginals and expected transition counts, the EM fit
  of kon, koff and the initial probability, the MAP path, and posterior rasters by backward sampling, counted like those
  of ``rates_sample`` (``tq_smooth_estep``, ``tq_smooth_mstep``, ``tq_smooth_viterbi``, ``tq_smooth_count``);
* ``smooth_dwell_sample`` / ``smooth_dwell_intervals``: the outputs of ``dwell_sample`` / ``dwell_intervals`` and the
  first-binding frames of ``ttfb_sample`` for the rasters of ``smooth_sample``, walked as they are drawn
  (``tq_smooth_dwell``);
* ``hmm_estep`` / ``hmm_mstep`` / ``hmm_fit`` / ``hmm_viterbi`` / ``hmm_sample`` / ``hmm_estimate`` / ``hmm_summary``: the
  same chain with up to four hidden states, several of them sharing the evidence of z = 0 or of z = 1 -- state marginals,
  the EM fit of the whole transition matrix with its BIC, the MAP path in hidden states, posterior rasters with their
  class-level and state-level counts, and the transition matrix of every raster, pooled or resampled over AOIs
  (``tq_hmm_estep``, ``tq_hmm_mstep``, ``tq_hmm_viterbi``, ``tq_hmm_count``, ``tq_hmm_estimate``);
* ``hmm_dwell_sample`` / ``hmm_dwell_intervals``: the outputs of ``smooth_dwell_sample`` / ``smooth_dwell_intervals`` for
  the class rasters of ``hmm_sample``, walked as they are drawn (``tq_chain_dwell``);
* ``hmm_random_starts`` / ``hmm_fit_restarts``: the EM of ``hmm_fit`` from several starts fitted side by side, under an
  optional topology of forbidden transitions, and the best of them (``tq_multistart_estep``, ``tq_multistart_mstep``);
* ``refit_weights`` / ``refit_estep`` / ``refit_mstep`` / ``hmm_fit_refits``: the non-parametric bootstrap of that EM fit
  over the AOIs -- every resample a weight per AOI, the refits side by side from the fitted theta -- for the uncertainty
  of theta itself (``tq_refit_weights``, ``tq_refit_estep``, ``tq_refit_mstep``);
* ``mixture_default_start`` / ``mixture_random_starts`` / ``mixture_mstep`` / ``mixture_fit`` / ``mixture_sample`` /
  ``mixture_estimate`` / ``mixture_viterbi``: a mixture of G such chains over the AOIs -- static heterogeneity, every AOI
  belonging to one population -- fitted by EM from several starts side by side, with the responsibilities, the BIC,
  posterior rasters that draw a population each, and the transition matrix of every population
  (``tq_multistart_estep``, ``tq_mixture_mstep``, ``tq_mixture_count``, ``tq_mixture_estimate``);
* ``mixture_dwell_sample`` / ``mixture_dwell_intervals`` / ``population_first_binding``: the outputs of ``hmm_dwell_sample``
  / ``hmm_dwell_intervals`` for the class rasters of ``mixture_sample``, walked as they are drawn, with the histograms kept
  apart by the population every row drew, and the first-binding frames split by population (``tq_population_dwell``;
  ``population_first_binding`` is host-side torch on S x N numbers and runs anywhere);
* ``timed_gaps`` / ``timed_tables`` / ``timed_estep`` / ``timed_mstep`` / ``timed_fit``: the chain of ``hmm_fit`` in
  continuous time on the frames' time stamps -- a generator Q in the place of the per-frame matrix, the transition over a
  gap d its exponential exp(Q d), the expected jumps and holding times of a discretely observed Markov process in the
  E-step -- for records that are not equally spaced (``tq_timed_table``, ``tq_timed_estep``, ``tq_timed_mstep``;
  ``timed_gaps`` is host-side torch and runs anywhere).

Two colour channels smoothed together as one chain (``smooth --joint``), with the dwell times of one channel by the other's
state and the order of arrival (``dwelltime`` / ``ttfb --smooth --joint``), are in ``tapqir_amd/utils/joint_analysis.py``, the
open last run as a right-censored dwell (``dwelltime --censored``) in ``tapqir_amd/utils/censored_analysis.py``.

There is no CPU path: every entry point raises ``HipExtensionError`` off the device.
"""

import ctypes as C

import torch

from tapqir_amd import _lib, _lib_hmm, _lib_mixture, _lib_multistart, _lib_rates, _lib_refit, _lib_smooth, _lib_timed
from tapqir_amd.exceptions import HipExtensionError

ADAM_BETAS = (0.9, 0.999)
ADAM_EPS = 1e-8


def _device_tensor(x, what):
    if not isinstance(x, torch.Tensor) or x.device.type != "cuda":
        raise HipExtensionError(f"{what} runs on the HIP device only (no CPU fallback): pass a cuda tensor")
    return x.detach().to(torch.float32).contiguous()


def _stream(dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _sampler_inputs(who, p_bound, num_samples, seed):
    """What the samplers share: ``p_bound`` as a clamped (N, F) float32 device tensor, N, F, and the seed as the uint64
    of the argument block."""
    p = _device_tensor(p_bound, who)
    if p.ndim != 2 or p.shape[0] < 1 or p.shape[1] < 1 or num_samples < 1:
        raise ValueError(f"{who}: p_bound must be (N, F) with N, F >= 1 and num_samples >= 1, got {tuple(p.shape)}")
    return p.clamp(0.0, 1.0), p.shape[0], p.shape[1], int(seed) & (2**64 - 1)


def _run_chunks(fit_steps, n_steps, chunk, progress_bar):
    """``fit_steps(step0, n)`` for launches of ``max(1, int(chunk))`` steps (the last one shorter) up to ``n_steps``."""
    chunk = max(1, int(chunk))
    starts = range(0, n_steps, chunk)
    for step0 in (progress_bar(starts) if progress_bar is not None else starts):
        fit_steps(step0, min(chunk, n_steps - step0))


def ttfb_sample(p_bound, num_samples, seed=0):
    """``num_samples`` posterior draws of the first-binding frame of each AOI.

    ``p_bound`` (N, F): q(z = 1) of each AOI-frame (``z_probs[..., c, 1]`` of the params file).  Returns ``tau``
    (num_samples, N), float32 on the device: the first frame with z = 1 of each sampled raster, or F if there is none
    -- ``time_to_first_binding(z_sample(num_samples))`` of the reference, drawn from the exact law of that index."""
    p, N, F, seed = _sampler_inputs("ttfb_sample", p_bound, num_samples, seed)
    L = torch.empty(N, F, dtype=torch.float64, device=p.device)
    tau = torch.empty(num_samples, N, dtype=torch.float32, device=p.device)
    a = _lib.TtfbSampleArgs(p=_lib.ptr(p), log_surv=_lib.ptr(L), tau=_lib.ptr(tau), N=N, F=F, S=int(num_samples), seed=seed)
    _lib.check(_lib.load().tq_ttfb_sample(C.byref(a), _stream(p.device)), "tq_ttfb_sample")
    return tau


def ttfb_init_state(S, device):
    """Adam state of ``S`` fits at the reference's initial values (mle_analysis.py:50-64: ka = kns = 0.001, Af = 0.9,
    stored unconstrained by pyro as log / logit, float32), zero moments."""
    init = torch.tensor([0.001, 0.001, 0.9], dtype=torch.float32)
    unc = torch.stack([init[0].log(), init[1].log(), init[2].logit()])
    state = torch.zeros(S, _lib.TTFB_STATE, dtype=torch.float32)
    state[:, :3] = unc
    return state.to(device)


def ttfb_fit_steps(state, data, Tmax, control=None, lr=5e-3, step0=0, n_steps=1, loss=None, stage_lds=True):
    """One launch of ``tq_ttfb_fit``: Adam steps ``step0 + 1 .. step0 + n_steps`` of every fit, in place on ``state``
    (S, 9).  ``loss`` (S,) receives the loss of the last step (before its update) if given."""
    tau = _device_tensor(data, "ttfb_fit")
    S, N = tau.shape
    tauc = None if control is None else _device_tensor(control, "ttfb_fit")
    if tauc is not None and tauc.shape[0] != S:
        raise ValueError(f"ttfb_fit: control has {tauc.shape[0]} rows, data {S}")
    a = _lib.TtfbFitArgs(tau=_lib.ptr(tau), tauc=_lib.ptr(tauc), state=_lib.ptr(state), loss=_lib.ptr(loss), S=S, N=N,
                         Nc=0 if tauc is None else tauc.shape[1], step0=int(step0), n_steps=int(n_steps),
                         stage_lds=1 if stage_lds else 0, Tmax=float(Tmax), lr=float(lr), beta1=ADAM_BETAS[0],
                         beta2=ADAM_BETAS[1], eps=ADAM_EPS)
    _lib.check(_lib.load().tq_ttfb_fit(C.byref(a), _stream(tau.device)), "tq_ttfb_fit")
    return state


def ttfb_fit(data, Tmax, control=None, lr=5e-3, n_steps=15000, progress_bar=None, chunk=1000, stage_lds=True):
    """Maximum-likelihood fit of ka, kns, Af to every row of ``data`` (S, N) of first-binding times.

    ``control`` (S, Nc): first-binding times at control locations, or None.  Runs ``n_steps`` Adam steps (lr, betas
    (0.9, 0.999), eps 1e-8) in launches of ``chunk`` steps; the result does not depend on ``chunk``.  Returns
    ``{"ka", "kns", "Af"}``, each (S, 1) float32 on the device, and ``"loss"`` (S,): the loss of the last step."""
    tau = _device_tensor(data, "ttfb_fit")
    if tau.ndim != 2:
        raise ValueError(f"ttfb_fit: data must be (S, N), got {tuple(tau.shape)}")
    S = tau.shape[0]
    state = ttfb_init_state(S, tau.device)
    loss = torch.full((S,), float("nan"), dtype=torch.float32, device=tau.device)
    _run_chunks(lambda step0, n: ttfb_fit_steps(state, tau, Tmax, control, lr, step0, n, loss, stage_lds), n_steps, chunk,
                progress_bar)
    return {"ka": state[:, 0:1].exp(), "kns": state[:, 1:2].exp(), "Af": torch.sigmoid(state[:, 2:3]), "loss": loss}


def fraction_bound(data, Tmax):
    """``fraction_bound[s, t] = mean_n(data[s, n] < t)`` for t = 0 .. Tmax - 1 (main.py:1073), from per-sample counts
    and a cumulative sum instead of an S x N x T comparison."""
    tau = data.to(torch.int64).clamp(0, Tmax)
    S, N = tau.shape
    counts = torch.zeros(S, Tmax + 1, dtype=torch.float64, device=tau.device)
    counts.scatter_add_(1, tau, torch.ones_like(tau, dtype=torch.float64))
    below = torch.cumsum(counts, dim=1) - counts  # below[s, t] = #{n : tau < t}
    return (below[:, :Tmax] / N).to(torch.float32)


def hpdi_columns(x, prob):
    """Narrowest interval holding ``prob`` of the samples along dim 0, per column (pyro.ops.stats.hpdi(x, prob, dim=0))."""
    xs = torch.sort(x, dim=0)[0]
    n = xs.shape[0]
    k = int(prob * n)
    left, right = xs[: n - k], xs[k:]
    i = torch.argmin(right - left, dim=0, keepdim=True)
    return left.gather(0, i)[0], right.gather(0, i)[0]


def fraction_bound_fit(data, Tmax, ka, kns, Af):
    """Best-fit cumulative fraction bound at t = 0 .. Tmax - 1 (main.py:1079-1096): the share of AOIs bound at t = 0
    plus the fitted two-exponential curve over the rest, averaged over samples."""
    data = data.to(torch.float32)
    N = data.shape[1]
    nz = (data == 0).sum(1, keepdim=True).to(torch.float32)
    t = torch.arange(Tmax, dtype=torch.float32, device=data.device)
    curve = Af * (1 - torch.exp(-(ka + kns) * t)) + (1 - Af) * (1 - torch.exp(-kns * t))
    return (nz / N + (1 - nz / N) * curve).mean(0)


# ---- dwell times (`dwelltime`, tapqir/main.py:1150-1384) ---------------------------------------------------------------
def dwell_sample(p_bound, num_samples, seed=0):
    """Launch A of the interval sampler: ``num_samples`` posterior rasters of each AOI, drawn and walked on the device.

    ``p_bound`` (N, F): q(z = 1) of each AOI-frame.  Returns ``{"hist_bound", "hist_unbound"}``, (num_samples, F) int32:
    the number of interior bound / unbound runs of each dwell time per sample, and ``"counts"`` (num_samples, N) int32:
    the number of intervals (of any kind) of each sampled row.  Nothing of size S x N x F is stored."""
    p, N, F, seed = _sampler_inputs("dwell_sample", p_bound, num_samples, seed)
    S = int(num_samples)
    counts = torch.empty(S, N, dtype=torch.int32, device=p.device)
    hb = torch.zeros(S, F, dtype=torch.int32, device=p.device)
    hu = torch.zeros(S, F, dtype=torch.int32, device=p.device)
    a = _lib.DwellSampleArgs(p=_lib.ptr(p), counts=_lib.ptr(counts), hist_bound=_lib.ptr(hb), hist_unbound=_lib.ptr(hu),
                             N=N, F=F, S=S, mode=_lib.DWELL_COUNT, seed=seed)
    _lib.check(_lib.load().tq_dwell_sample(C.byref(a), _stream(p.device)), "tq_dwell_sample")
    return {"hist_bound": hb, "hist_unbound": hu, "counts": counts}


def dwell_intervals(p_bound, num_samples, seed=0, sample=None, device_table=False):
    """The interval table of ``num_samples`` posterior rasters (``count_intervals(z_sample)`` of the reference): launch A
    (or its result ``sample`` from ``dwell_sample`` with the same arguments), an exclusive scan of the row counts, and
    launch B, which draws the same bits again and writes every row's intervals at its offset.  Returns a DataFrame with
    the columns of ``tapqir_amd.utils.imscroll.INTERVAL_COLUMNS``, int64, in (sample, AOI, frame) order.  With
    ``device_table`` it returns ``(DataFrame, table)``, table the (DWELL_COLS, total) int32 device tensor launch B wrote
    (what ``censored_analysis.dwell_censored_hist`` reads)."""
    given = num_samples if sample is None else sample["counts"].shape[0]
    p, N, F, seed = _sampler_inputs("dwell_intervals", p_bound, given, seed)
    if sample is None:
        sample = dwell_sample(p, num_samples, seed)
    counts = sample["counts"]
    S = counts.shape[0]
    csum = torch.cumsum(counts.reshape(-1).to(torch.int64), 0)
    offsets = (csum - counts.reshape(-1)).contiguous()
    total = int(csum[-1].item())
    cols = torch.empty(_lib.DWELL_COLS, max(total, 1), dtype=torch.int32, device=p.device)
    a = _lib.DwellSampleArgs(p=_lib.ptr(p), offsets=_lib.ptr(offsets), intervals=_lib.ptr(cols), total=total, N=N, F=F,
                             S=S, mode=_lib.DWELL_EMIT, seed=seed)
    _lib.check(_lib.load().tq_dwell_sample(C.byref(a), _stream(p.device)), "tq_dwell_sample")
    return _interval_frame(cols, total, device_table)


def _interval_frame(cols, total, device_table=False):
    """The DataFrame of the first ``total`` columns of the device table ``cols`` (DWELL_COLS, max(total, 1)) int32; with
    ``device_table`` also that part of the table itself, still on the device."""
    import pandas as pd

    from tapqir_amd.utils.imscroll import INTERVAL_COLUMNS

    host = cols[:, :total].to(torch.int64).cpu().numpy()
    frame = pd.DataFrame({name: host[i] for i, name in enumerate(INTERVAL_COLUMNS)})
    return (frame, cols[:, :total]) if device_table else frame


def dwell_csr_from_hist(hist):
    """(values, weights, row_ptr) of the nonzero bins of per-sample histograms ``hist`` (S, F): value = dwell time (the
    bin index), weight = its count.  Bin 0 is ignored (a dwell time is at least one frame)."""
    h = hist.to(torch.float32)
    h = torch.cat([torch.zeros_like(h[:, :1]), h[:, 1:]], 1)
    nz = h > 0
    t = torch.arange(h.shape[1], dtype=torch.float32, device=h.device).expand_as(h)
    return _csr(t[nz], h[nz], nz.sum(1))


def dwell_csr_from_padded(data):
    """(values, weights, row_ptr) of zero-padded per-sample dwell times ``data`` (S, M), the reference's ``exp_model``
    input: the entries > 0, each with weight 1."""
    nz = data > 0
    vals = data[nz].to(torch.float32)
    return _csr(vals, torch.ones_like(vals), nz.sum(1))


def _csr(values, weights, row_len):
    row_ptr = torch.zeros(row_len.shape[0] + 1, dtype=torch.int64, device=values.device)
    row_ptr[1:] = torch.cumsum(row_len.to(torch.int64), 0)
    if values.numel() == 0:  # keep valid pointers for an all-empty data set
        values = torch.zeros(1, dtype=torch.float32, device=row_ptr.device)
        weights = torch.zeros(1, dtype=torch.float32, device=row_ptr.device)
    return values.contiguous(), weights.contiguous(), row_ptr


def dwell_init_state(S, K, device):
    """Adam state (S, 6K) of ``S`` fits at the reference's initial values (mle_analysis.py:108-116: k = logspace(-K + 1, 0,
    K), A = ones, stored unconstrained by pyro through transform_to: log k, and softmax logits log 1 = 0, i.e. A = 1 / K;
    float32), zero moments."""
    state = torch.zeros(S, 6 * K, dtype=torch.float32)
    state[:, :K] = torch.logspace(-K + 1, 0, K, dtype=torch.float32).log()
    return state.to(device)


def _check_K(K):
    if not 1 <= int(K) <= _lib.DWELL_KMAX:
        raise ValueError(f"dwell_fit: K must be in 1 .. {_lib.DWELL_KMAX}, got {K}")
    return int(K)


def dwell_fit_steps(state, csr, K, lr=5e-3, step0=0, n_steps=1, loss=None, stage_lds=True):
    """One launch of ``tq_dwell_fit``: Adam steps ``step0 + 1 .. step0 + n_steps`` of every fit, in place on ``state``
    (S, 6K).  ``csr`` = (values, weights, row_ptr) on the device; ``loss`` (S,) receives the loss of the last step."""
    K = _check_K(K)
    values, weights, row_ptr = csr
    values = _device_tensor(values, "dwell_fit")
    weights = _device_tensor(weights, "dwell_fit")
    if not isinstance(row_ptr, torch.Tensor) or row_ptr.device.type != "cuda":
        raise HipExtensionError("dwell_fit runs on the HIP device only (no CPU fallback): pass cuda tensors")
    row_ptr = row_ptr.to(torch.int64).contiguous()
    S = row_ptr.shape[0] - 1
    if state.shape != (S, 6 * K) or state.dtype != torch.float32 or not state.is_contiguous():
        raise ValueError(f"dwell_fit: state must be contiguous float32 ({S}, {6 * K}), got {tuple(state.shape)}")
    a = _lib.DwellFitArgs(values=_lib.ptr(values), weights=_lib.ptr(weights), row_ptr=_lib.ptr(row_ptr),
                          state=_lib.ptr(state), loss=_lib.ptr(loss), S=S, K=K, step0=int(step0), n_steps=int(n_steps),
                          stage_lds=1 if stage_lds else 0, lr=float(lr), beta1=ADAM_BETAS[0], beta2=ADAM_BETAS[1],
                          eps=ADAM_EPS)
    _lib.check(_lib.load().tq_dwell_fit(C.byref(a), _stream(values.device)), "tq_dwell_fit")
    return state


def dwell_fit(data, K=3, lr=5e-3, n_steps=10000, chunk=1000, progress_bar=None, stage_lds=True):
    """Maximum-likelihood fit of a K-exponential mixture to every posterior sample's dwell times (``train(exp_model,
    exp_guide, lr, n_steps, data, K)`` of the reference).

    ``data``: zero-padded dwell times (S, M) (entries > 0 count, as ``bound_dwell_times`` returns them), or a
    ``(values, weights, row_ptr)`` CSR triple such as ``dwell_csr_from_hist(hist)``; cuda tensors either way.  Runs
    ``n_steps`` Adam steps (lr, betas (0.9, 0.999), eps 1e-8) in launches of ``chunk`` steps; the result does not depend
    on ``chunk``.  Returns ``{"k", "A"}``, each (S, K) float32 on the device, and ``"loss"`` (S,): the loss of the last
    step.  A sample without data keeps its initial values."""
    K = _check_K(K)
    if isinstance(data, (tuple, list)):
        csr = tuple(data)
    else:
        d = _device_tensor(data, "dwell_fit")
        if d.ndim != 2:
            raise ValueError(f"dwell_fit: data must be (S, M), got {tuple(d.shape)}")
        csr = dwell_csr_from_padded(d)
    if not isinstance(csr[2], torch.Tensor) or csr[2].device.type != "cuda":
        raise HipExtensionError("dwell_fit runs on the HIP device only (no CPU fallback): pass cuda tensors")
    S = csr[2].shape[0] - 1
    dev = csr[2].device
    state = dwell_init_state(S, K, dev)
    loss = torch.full((S,), float("nan"), dtype=torch.float32, device=dev)
    _run_chunks(lambda step0, n: dwell_fit_steps(state, csr, K, lr, step0, n, loss, stage_lds), n_steps, chunk,
                progress_bar)
    return {"k": state[:, :K].exp(), "A": torch.softmax(state[:, K:2 * K], dim=1), "loss": loss}


# ---- two-state rates (`rates`, tapqir/utils/imscroll.py:199-317) -------------------------------------------------------
def rates_sample(p_bound, num_samples, seed=0):
    """Transition counts of ``num_samples`` posterior rasters of each AOI, drawn and counted on the device.

    ``p_bound`` (N, F): q(z = 1) of each AOI-frame.  Returns ``counts`` (num_samples, N, 4) int32 on the device: over
    the F - 1 frame pairs of row (s, n), the number of 0 -> 1 steps, of z_f = 0, of 1 -> 0 steps and of z_f = 1.  The
    rows are those of ``dwell_sample(p_bound, num_samples, seed)``; nothing of size S x N x F is stored."""
    p, N, F, seed = _sampler_inputs("rates_sample", p_bound, num_samples, seed)
    S = int(num_samples)
    counts = torch.empty(S, N, _lib_rates.RATES_COLS, dtype=torch.int32, device=p.device)
    a = _lib_rates.RatesCountArgs(p=_lib.ptr(p), counts=_lib.ptr(counts), N=N, F=F, S=S, seed=seed)
    _lib.check(_lib_rates.lib().tq_rates_count(C.byref(a), _stream(p.device)), "tq_rates_count")
    return counts


def rates_estimate(counts, bootstrap=False, seed=0):
    """kon and koff of every posterior sample from the row counts of ``rates_sample``.

    ``bootstrap=False`` pools every AOI once (``posterior_estimate(Bernoulli(p), association_rate)`` of the reference);
    ``bootstrap=True`` sums N rows drawn with replacement, a fresh draw per sample from ``seed`` (the 2-D analogue of
    ``sample_and_bootstrap``).  Returns ``{"kon", "koff"}``, (S,) float64, and ``"totals"`` (S, 4) int64, on the device.
    A zero denominator gives NaN or inf, which stay in the arrays (``rates_summary`` leaves them out)."""
    if not isinstance(counts, torch.Tensor) or counts.device.type != "cuda":
        raise HipExtensionError("rates_estimate runs on the HIP device only (no CPU fallback): pass a cuda tensor")
    if counts.ndim != 3 or counts.shape[2] != _lib_rates.RATES_COLS or counts.dtype != torch.int32 or 0 in counts.shape:
        raise ValueError(f"rates_estimate: counts must be int32 (S, N, {_lib_rates.RATES_COLS}) with S, N >= 1, got "
                         f"{counts.dtype} {tuple(counts.shape)}")
    counts = counts.contiguous()
    S, N = counts.shape[:2]
    totals = torch.empty(S, _lib_rates.RATES_COLS, dtype=torch.int64, device=counts.device)
    est = torch.empty(S, 2, dtype=torch.float64, device=counts.device)
    a = _lib_rates.RatesEstimateArgs(counts=_lib.ptr(counts), totals=_lib.ptr(totals), estimand=_lib.ptr(est), N=N, S=S,
                                     resample=1 if bootstrap else 0, seed=int(seed) & (2**64 - 1))
    _lib.check(_lib_rates.lib().tq_rates_estimate(C.byref(a), _stream(counts.device)), "tq_rates_estimate")
    return {"kon": est[:, 0], "koff": est[:, 1], "totals": totals}


def rates_summary(estimate, probs=0.68):
    """Mean and percentile interval (pyro's ``pi(estimand, probs)``: the linear-interpolation quantiles at
    (1 - probs) / 2 and (1 + probs) / 2) of each rate over its finite estimands.

    Returns ``{"kon": {...}, "koff": {...}}`` with the floats ``"mean"``, ``"ll"``, ``"ul"`` and the int ``"left_out"``:
    the number of non-finite estimands (zero denominators) that the three leave out.  A rate without a finite estimand
    has NaN for all three."""
    return {rate: estimand_summary(estimate[rate], probs) for rate in ("kon", "koff")}


def estimand_summary(estimand, probs):
    """``{"mean", "ll", "ul", "left_out"}`` of one estimand over the samples: what ``rates_summary`` returns per rate."""
    from tapqir_amd.utils.stats import quantile

    x = estimand.double()
    x = x[torch.isfinite(x)]
    left_out = estimand.numel() - x.numel()
    if x.numel() == 0:
        return {"mean": float("nan"), "ll": float("nan"), "ul": float("nan"), "left_out": left_out}
    return {"mean": x.mean().item(), "ll": quantile(x, (1 - probs) / 2).item(), "ul": quantile(x, (1 + probs) / 2).item(),
            "left_out": left_out}


# ---- two-state hidden Markov smoothing (`smooth`) --------------------------------------------------
def _smooth_inputs(who, p, theta, prior):
    """``p`` through ``_sampler_inputs``, ``theta`` as 3 doubles on p's device, the prior as a float in (0, 1)."""
    p, N, F, _ = _sampler_inputs(who, p, 1, 0)
    if F > _lib_smooth.SMOOTH_MAX_F:
        raise ValueError(f"{who}: at most {_lib_smooth.SMOOTH_MAX_F} frames, got {F}")
    if not isinstance(theta, torch.Tensor) or theta.device != p.device or theta.dtype != torch.float64 or theta.numel() != 3:
        raise ValueError(f"{who}: theta must be 3 float64 values (kon, koff, pi0) on the device of p")
    prior = float(prior)
    if not 0.0 < prior < 1.0:
        raise ValueError(f"{who}: prior must lie in (0, 1), got {prior}")
    return p, N, F, theta.contiguous(), prior


def _smooth_estep(p, N, F, theta, prior, out):
    a = _lib_smooth.SmoothEstepArgs(p=_lib.ptr(p), theta=_lib.ptr(theta), filt=_lib.ptr(out["filt"]),
                                    gamma=_lib.ptr(out["gamma"]), rows=_lib.ptr(out["rows"]), N=N, F=F, prior=prior)
    _lib.check(_lib_smooth.lib().tq_smooth_estep(C.byref(a), _stream(p.device)), "tq_smooth_estep")
    return out


def _smooth_buffers(N, F, device):
    return {"filt": torch.empty(N, F, dtype=torch.float64, device=device),
            "gamma": torch.empty(N, F, dtype=torch.float64, device=device),
            "rows": torch.empty(N, _lib_smooth.SMOOTH_COLS, dtype=torch.float64, device=device)}


def smooth_estep(p, theta, prior):
    """Forward-backward of every row of ``p`` (N, F), the fit's p(z = 1), under the chain ``theta`` = (kon, koff, pi0)
    (3 float64 on the device) with the fit's ``prior`` divided out of ``p``.

    Returns ``{"filt", "gamma"}``, (N, F) float64: the filtered and the smoothed p(z = 1), and ``"rows"`` (N, 6): the
    expected counts E n01, E n0, E n10, E n1 of the row's frame pairs (the columns of ``rates_sample``), its
    log-evidence and gamma_0(1)."""
    p, N, F, theta, prior = _smooth_inputs("smooth_estep", p, theta, prior)
    return _smooth_estep(p, N, F, theta, prior, _smooth_buffers(N, F, p.device))


def _mstep_inputs(who, rows, theta, trace, it, states=None):
    """What ``smooth_mstep``, ``hmm_mstep`` and ``timed_mstep`` ask of their arguments: ``rows`` a contiguous float64
    (N, cols) on the device, ``theta`` and ``trace`` float64 vectors there that hold theta and entry ``it``.  ``states`` =
    (unbound, bound) of a chain of M states, or None for the two-state chain of ``smooth``.  Returns (U, B, M)."""
    if not isinstance(rows, torch.Tensor) or rows.device.type != "cuda":
        raise HipExtensionError(f"{who} runs on the HIP device only (no CPU fallback): pass a cuda tensor")
    U, B, M = (None, None, None) if states is None else _hmm_states(who, *states)
    cols, n_theta = (_lib_smooth.SMOOTH_COLS, 3) if states is None else (_lib_hmm.hmm_cols(M), M * M + M)
    if rows.ndim != 2 or rows.shape[1] != cols or rows.shape[0] < 1 or rows.dtype != torch.float64 or not rows.is_contiguous():
        raise ValueError(f"{who}: rows must be contiguous float64 (N, {cols}), N >= 1")
    for name, x, n in (("theta", theta, n_theta), ("trace", trace, int(it) + 1)):
        if (not isinstance(x, torch.Tensor) or x.device != rows.device or x.dtype != torch.float64 or x.ndim != 1
                or x.numel() < n or not x.is_contiguous() or it < 0):
            raise ValueError(f"{who}: {name} must be a float64 vector of at least {n} values on the device of rows")
    return U, B, M


def smooth_mstep(rows, theta, trace, it=0):
    """One launch of ``tq_smooth_mstep``: ``theta`` (3 float64, in place) from the summed ``rows`` of an E-step, and the
    total log-evidence of those rows into ``trace[it]``.  Returns ``theta``."""
    _mstep_inputs("smooth_mstep", rows, theta, trace, it)
    a = _lib_smooth.SmoothMstepArgs(rows=_lib.ptr(rows), theta=_lib.ptr(theta), trace=_lib.ptr(trace), N=rows.shape[0],
                                    it=int(it))
    _lib.check(_lib_smooth.lib().tq_smooth_mstep(C.byref(a), _stream(rows.device)), "tq_smooth_mstep")
    return theta


def smooth_fit(p, prior, kon=0.5, koff=0.5, init=0.5, num_iter=200, tol=1e-9, chunk=50, progress_bar=None):
    """EM fit of the chain (kon, koff, pi0 from ``kon``, ``koff``, ``init``) to the rows of ``p`` (N, F).

    The iterations are launched in chunks of ``chunk`` pairs of E-step and M-step, with no host synchronisation inside
    a chunk; after each chunk the trace of the log-evidence is read, and the run stops once an iteration has gained
    at most ``tol * |loglik|`` over the one before.  One more E-step at the final theta gives the outputs.

    Returns ``theta`` (3,), ``gamma``, ``filt`` (N, F), ``rows`` (N, 6), ``trace`` (iterations,) -- trace[i] is the
    log-evidence at the theta after i iterations -- all float64 on the device, and the Python values ``iterations``
    (the number run: whole chunks) and ``converged``."""
    num_iter = int(num_iter)
    theta = torch.tensor([kon, koff, init], dtype=torch.float64)
    if num_iter < 1 or not bool(((theta > 0) & (theta < 1)).all()):
        raise ValueError("smooth_fit: num_iter must be positive and kon, koff, init lie in (0, 1)")
    if not isinstance(p, torch.Tensor) or p.device.type != "cuda":
        raise HipExtensionError("smooth_fit runs on the HIP device only (no CPU fallback): pass a cuda tensor")
    theta = theta.to(p.device)
    p, N, F, theta, prior = _smooth_inputs("smooth_fit", p, theta, prior)
    out = _smooth_buffers(N, F, p.device)
    trace = torch.full((num_iter,), float("nan"), dtype=torch.float64, device=p.device)

    def step(it):
        _smooth_estep(p, N, F, theta, prior, out)
        smooth_mstep(out["rows"], theta, trace, it)

    state = _chain_em(step, trace, num_iter, tol, chunk, progress_bar)
    _smooth_estep(p, N, F, theta, prior, out)
    return {"theta": theta, **out, "trace": trace[: state["iterations"]], **state}


def smooth_viterbi(p, theta, prior):
    """MAP path of every row of ``p`` (N, F) under the chain ``theta`` and the evidence of ``smooth_estep``: (N, F) uint8
    on the device.  A tie takes state 0."""
    p, N, F, theta, prior = _smooth_inputs("smooth_viterbi", p, theta, prior)
    back = torch.empty(((F + 15) // 16) * N, dtype=torch.int32, device=p.device)
    path = torch.empty(N, F, dtype=torch.uint8, device=p.device)
    a = _lib_smooth.SmoothViterbiArgs(p=_lib.ptr(p), theta=_lib.ptr(theta), back=_lib.ptr(back), path=_lib.ptr(path), N=N,
                                      F=F, prior=prior)
    _lib.check(_lib_smooth.lib().tq_smooth_viterbi(C.byref(a), _stream(p.device)), "tq_smooth_viterbi")
    return path


def _smooth_sample_inputs(who, filt, theta, num_samples):
    """What the backward samplers share: ``filt`` as contiguous float64 (N, F) on the device, ``theta`` as 3 doubles on
    the same device, S, N and F."""
    if not isinstance(filt, torch.Tensor) or filt.device.type != "cuda":
        raise HipExtensionError(f"{who} runs on the HIP device only (no CPU fallback): pass a cuda tensor")
    S = int(num_samples)
    if filt.ndim != 2 or 0 in filt.shape or filt.dtype != torch.float64 or S < 1 or filt.shape[1] > _lib_smooth.SMOOTH_MAX_F:
        raise ValueError(f"{who}: filt must be float64 (N, F) with N >= 1, 1 <= F <= {_lib_smooth.SMOOTH_MAX_F}, "
                         f"and num_samples >= 1, got {filt.dtype} {tuple(filt.shape)}")
    if not isinstance(theta, torch.Tensor) or theta.device != filt.device or theta.dtype != torch.float64 or theta.numel() != 3:
        raise ValueError(f"{who}: theta must be 3 float64 values (kon, koff, pi0) on the device of filt")
    return filt.contiguous(), theta.contiguous(), S, filt.shape[0], filt.shape[1]


def smooth_sample(filt, theta, num_samples, seed=0, raster=False):
    """Transition counts of ``num_samples`` posterior rasters of the chain, drawn by backward sampling from ``filt``
    (N, F) of ``smooth_estep`` at ``theta``.

    Returns ``counts`` (num_samples, N, 4) int32 in the layout of ``rates_sample`` (``rates_estimate`` takes them as they
    are); with ``raster=True`` returns ``(counts, z)`` with the rasters ``z`` (num_samples, N, F) uint8."""
    filt, theta, S, N, F = _smooth_sample_inputs("smooth_sample", filt, theta, num_samples)
    counts = torch.empty(S, N, _lib_rates.RATES_COLS, dtype=torch.int32, device=filt.device)
    z = torch.empty(S, N, F, dtype=torch.uint8, device=filt.device) if raster else None
    a = _lib_smooth.SmoothCountArgs(filt=_lib.ptr(filt), theta=_lib.ptr(theta), counts=_lib.ptr(counts), raster=_lib.ptr(z),
                                    N=N, F=F, S=S, seed=int(seed) & (2**64 - 1))
    _lib.check(_lib_smooth.lib().tq_smooth_count(C.byref(a), _stream(filt.device)), "tq_smooth_count")
    return (counts, z) if raster else counts


# ---- dwell times and first binding of the smoothed chain (`dwelltime --smooth`, `ttfb --smooth`) ----
def _walk_count(launch, S, N, F, dev, populations=None, partner=False):
    """Launch A of a sampler that walks its rasters as it draws them (``tq_smooth_dwell``, ``tq_chain_dwell``,
    ``tq_population_dwell``, ``tq_pair_dwell``): ``launch(**fields)`` fills the argument block's remaining fields and calls
    the entry point.  With ``populations`` = G the histograms are (S, G, F) and the launch also fills ``pop`` (S, N) uint8;
    with ``partner`` they are (S, 2, F) and it also fills ``tau_after`` (S, N) float32."""
    counts = torch.empty(S, N, dtype=torch.int32, device=dev)
    shape = (S, 2, F) if partner else (S, F) if populations is None else (S, populations, F)
    hb = torch.zeros(shape, dtype=torch.int32, device=dev)
    hu = torch.zeros(shape, dtype=torch.int32, device=dev)
    tau = torch.empty(S, N, dtype=torch.float32, device=dev)
    out = {"hist_bound": hb, "hist_unbound": hu, "counts": counts, "tau": tau}
    extra = {}
    if populations is not None:
        out["pop"] = torch.empty(S, N, dtype=torch.uint8, device=dev)
        extra["pop"] = _lib.ptr(out["pop"])
    if partner:
        out["tau_after"] = torch.empty(S, N, dtype=torch.float32, device=dev)
        extra["tau_after"] = _lib.ptr(out["tau_after"])
    launch(counts=_lib.ptr(counts), hist_bound=_lib.ptr(hb), hist_unbound=_lib.ptr(hu), tau=_lib.ptr(tau),
           mode=_lib.DWELL_COUNT, **extra)
    return out


def _walk_emit(who, launch, sample, S, N, dev, device_table=False, partner=False):
    """The exclusive scan of the row counts of launch A and launch B of the same sampler; the DataFrame of
    ``dwell_intervals`` (with ``device_table``, the pair it returns then).  With ``partner`` launch B also fills one uint8
    per interval, and the result is the pair of that and those ``total`` codes on the device."""
    counts = sample["counts"].contiguous()
    if counts.shape != (S, N) or counts.dtype != torch.int32 or counts.device != dev:
        raise ValueError(f"{who}: sample['counts'] must be int32 ({S}, {N}) on the device of filt")
    csum = torch.cumsum(counts.reshape(-1).to(torch.int64), 0)
    offsets = (csum - counts.reshape(-1)).contiguous()
    total = int(csum[-1].item())
    cols = torch.empty(_lib.DWELL_COLS, max(total, 1), dtype=torch.int32, device=dev)
    extra = {}
    if partner:
        codes = torch.empty(max(total, 1), dtype=torch.uint8, device=dev)
        extra["partner"] = _lib.ptr(codes)
    launch(counts=_lib.ptr(counts), offsets=_lib.ptr(offsets), intervals=_lib.ptr(cols), total=total, mode=_lib.DWELL_EMIT,
           **extra)
    frame = _interval_frame(cols, total, device_table)
    return (frame, codes[:total]) if partner else frame


def _smooth_dwell_launch(filt, theta, S, N, F, seed):
    def launch(**fields):
        a = _lib_smooth.SmoothDwellArgs(filt=_lib.ptr(filt), theta=_lib.ptr(theta), N=N, F=F, S=S,
                                        seed=int(seed) & (2**64 - 1), **fields)
        _lib.check(_lib_smooth.lib().tq_smooth_dwell(C.byref(a), _stream(filt.device)), "tq_smooth_dwell")

    return launch


def smooth_dwell_sample(filt, theta, num_samples, seed=0):
    """Launch A of the interval sampler on the rasters of ``smooth_sample(filt, theta, num_samples, seed)``: every row is
    walked into runs of equal labels as it is drawn backwards, and no raster is stored.

    Returns ``{"hist_bound", "hist_unbound", "counts"}`` with the shapes and meaning of ``dwell_sample``, and ``"tau"``
    (num_samples, N) float32 on the device: the first frame with z = 1 of each row, or F if there is none, as
    ``ttfb_sample`` returns it.  The histograms go to ``dwell_csr_from_hist`` / ``dwell_fit``, ``tau`` to ``ttfb_fit``."""
    filt, theta, S, N, F = _smooth_sample_inputs("smooth_dwell_sample", filt, theta, num_samples)
    return _walk_count(_smooth_dwell_launch(filt, theta, S, N, F, seed), S, N, F, filt.device)


def smooth_dwell_intervals(filt, theta, num_samples, seed=0, sample=None, device_table=False):
    """The interval table of the rasters of ``smooth_sample(filt, theta, num_samples, seed)``: launch A (or its result
    ``sample`` from ``smooth_dwell_sample`` with the same arguments), an exclusive scan of the row counts, and launch B,
    which draws the same bits again and writes every row's intervals, last run first, back from the end of the row's
    slice.  Returns the DataFrame of ``dwell_intervals``: the columns of ``tapqir_amd.utils.imscroll.INTERVAL_COLUMNS``,
    int64, in (sample, AOI, frame) order; with ``device_table`` the pair ``dwell_intervals`` returns then."""
    given = num_samples if sample is None else sample["counts"].shape[0]
    filt, theta, S, N, F = _smooth_sample_inputs("smooth_dwell_intervals", filt, theta, given)
    launch = _smooth_dwell_launch(filt, theta, S, N, F, seed)
    if sample is None:
        sample = _walk_count(launch, S, N, F, filt.device)
    return _walk_emit("smooth_dwell_intervals", launch, sample, S, N, filt.device, device_table)


# ---- hidden Markov smoothing with several states per class (`smooth --bound-states`) ---------------
def _hmm_states(who, unbound, bound):
    U, B = int(unbound), int(bound)
    if U < 1 or B < 1 or U + B > _lib_hmm.HMM_MAX_STATES:
        raise ValueError(f"{who}: unbound and bound must be at least 1 and sum to at most {_lib_hmm.HMM_MAX_STATES}, got "
                         f"{unbound} and {bound}")
    return U, B, U + B


def _hmm_theta(who, theta, M, device):
    if (not isinstance(theta, torch.Tensor) or theta.device != device or theta.dtype != torch.float64
            or theta.numel() != M * M + M):
        raise ValueError(f"{who}: theta must be {M * M + M} float64 values (A row-major, rho) on the device of the data")
    return theta.contiguous().reshape(-1)


def _hmm_inputs(who, p, theta, prior, unbound, bound):
    """``p`` through ``_sampler_inputs``, U, B, M, ``theta`` as M * M + M doubles on p's device, the prior in (0, 1)."""
    U, B, M = _hmm_states(who, unbound, bound)
    p, N, F, _ = _sampler_inputs(who, p, 1, 0)
    if F > _lib_smooth.SMOOTH_MAX_F:
        raise ValueError(f"{who}: at most {_lib_smooth.SMOOTH_MAX_F} frames, got {F}")
    prior = float(prior)
    if not 0.0 < prior < 1.0:
        raise ValueError(f"{who}: prior must lie in (0, 1), got {prior}")
    return p, N, F, _hmm_theta(who, theta, M, p.device), prior, U, B, M


def _hmm_buffers(N, F, M, device):
    return {"filt": torch.empty(N, F, M, dtype=torch.float64, device=device),
            "gamma": torch.empty(N, F, M, dtype=torch.float64, device=device),
            "rows": torch.empty(N, _lib_hmm.hmm_cols(M), dtype=torch.float64, device=device)}


def _hmm_estep(p, N, F, theta, prior, U, B, out):
    a = _lib_hmm.HmmEstepArgs(p=_lib.ptr(p), theta=_lib.ptr(theta), filt=_lib.ptr(out["filt"]), gamma=_lib.ptr(out["gamma"]),
                              rows=_lib.ptr(out["rows"]), N=N, F=F, U=U, B=B, prior=prior)
    _lib.check(_lib_hmm.lib().tq_hmm_estep(C.byref(a), _stream(p.device)), "tq_hmm_estep")
    return out


def hmm_estep(p, theta, prior, unbound=1, bound=1):
    """Forward-backward of every row of ``p`` (N, F), the fit's p(z = 1), under a chain of M = ``unbound`` + ``bound``
    hidden states: ``theta`` = (A row-major, rho), M * M + M float64 on the device; states 0 .. unbound - 1 emit the
    evidence of z = 0, the others that of z = 1, with the fit's ``prior`` divided out of ``p``.

    Returns ``{"filt", "gamma"}``, (N, F, M) float64: the filtered and the smoothed state probabilities, and ``"rows"``
    (N, M * M + M + 1): the expected number of frame pairs in states (i, j), row-major, gamma_0 and the log-evidence."""
    p, N, F, theta, prior, U, B, M = _hmm_inputs("hmm_estep", p, theta, prior, unbound, bound)
    return _hmm_estep(p, N, F, theta, prior, U, B, _hmm_buffers(N, F, M, p.device))


def hmm_mstep(rows, theta, trace, it=0, unbound=1, bound=1):
    """One launch of ``tq_hmm_mstep``: ``theta`` (M * M + M float64, in place) from the summed ``rows`` of an E-step, and
    the total log-evidence of those rows into ``trace[it]``.  Returns ``theta``."""
    U, B, M = _mstep_inputs("hmm_mstep", rows, theta, trace, it, (unbound, bound))
    a = _lib_hmm.HmmMstepArgs(rows=_lib.ptr(rows), theta=_lib.ptr(theta), trace=_lib.ptr(trace), N=rows.shape[0], it=int(it),
                              U=U, B=B)
    _lib.check(_lib_hmm.lib().tq_hmm_mstep(C.byref(a), _stream(rows.device)), "tq_hmm_mstep")
    return theta


def hmm_default_start(unbound, bound):
    """The deterministic default start of ``hmm_fit`` as (A (M, M), rho (M,)) float64: the r-th state of a class leaves
    with probability 0.3 / 4^r, spread evenly over the other M - 1 states, so no two states of a class start alike; rho is
    uniform."""
    U, B, M = _hmm_states("hmm_default_start", unbound, bound)
    A = torch.zeros(M, M, dtype=torch.float64)
    for i in range(M):
        leave = 0.3 / 4.0 ** (i if i < U else i - U)
        A[i] = leave / (M - 1)
        A[i, i] = 1.0 - leave
    return A, torch.full((M,), 1.0 / M, dtype=torch.float64)


def hmm_canonical_order(theta, unbound, bound):
    """The permutation (a list: new state k is old state order[k]) that puts the states of each class in descending
    A_ii; equal values keep their order."""
    U, B, M = _hmm_states("hmm_canonical_order", unbound, bound)
    stay = theta.detach().cpu().reshape(-1)[: M * M].reshape(M, M).diagonal().tolist()
    return sorted(range(U), key=lambda i: -stay[i]) + sorted(range(U, M), key=lambda i: -stay[i])


def hmm_permute(order, M, theta=None, filt=None, gamma=None, rows=None):
    """The given outputs of ``hmm_estep`` / ``hmm_fit`` with their states relabelled by ``order``, as a dict."""
    idx = torch.as_tensor(order, dtype=torch.int64)
    out = {}
    if theta is not None:
        t = theta.reshape(-1)
        ix = idx.to(t.device)
        out["theta"] = torch.cat([t[: M * M].reshape(M, M)[ix][:, ix].reshape(-1), t[M * M:][ix]])
    for name, x in (("filt", filt), ("gamma", gamma)):
        if x is not None:
            out[name] = x[..., idx.to(x.device)].contiguous()
    if rows is not None:
        ix = idx.to(rows.device)
        n = rows.shape[0]
        out["rows"] = torch.cat([rows[:, : M * M].reshape(n, M, M)[:, ix][:, :, ix].reshape(n, M * M),
                                 rows[:, M * M: M * M + M][:, ix], rows[:, M * M + M:]], 1)
    return out


def hmm_fit(p, prior, unbound=1, bound=1, A0=None, rho0=None, num_iter=200, tol=1e-9, chunk=50, progress_bar=None):
    """EM fit of a chain of ``unbound`` + ``bound`` hidden states to the rows of ``p`` (N, F), from (``A0``, ``rho0``) or
    from ``hmm_default_start``; the chunks, the stopping rule and the final E-step are those of ``smooth_fit``.

    After the fit the states of each class are put in descending A_ii (``hmm_canonical_order``), in ``theta`` and in
    every output alike.  Returns what ``smooth_fit`` returns -- ``theta`` (M * M + M,), ``gamma``, ``filt`` (N, F, M),
    ``rows`` (N, M * M + M + 1), ``trace``, ``iterations``, ``converged`` -- and ``loglik`` (the log-evidence at the final
    theta), ``n_params`` = M (M - 1) + (M - 1) and ``bic`` = -2 loglik + n_params log(N F): the lower, the better."""
    import math

    num_iter = int(num_iter)
    U, B, M = _hmm_states("hmm_fit", unbound, bound)
    A, rho = hmm_default_start(U, B)
    if A0 is not None:
        A = torch.as_tensor(A0, dtype=torch.float64).cpu()
    if rho0 is not None:
        rho = torch.as_tensor(rho0, dtype=torch.float64).cpu()
    if (num_iter < 1 or A.shape != (M, M) or rho.shape != (M,) or not bool((A >= 0).all()) or not bool((rho >= 0).all())
            or not bool((A.sum(1) > 0).all()) or not float(rho.sum()) > 0):
        raise ValueError(f"hmm_fit: num_iter must be positive, A0 ({M}, {M}) and rho0 ({M},) non-negative with positive sums")
    if not isinstance(p, torch.Tensor) or p.device.type != "cuda":
        raise HipExtensionError("hmm_fit runs on the HIP device only (no CPU fallback): pass a cuda tensor")
    theta = torch.cat([(A / A.sum(1, keepdim=True)).reshape(-1), rho / rho.sum()]).to(p.device)
    p, N, F, theta, prior, U, B, M = _hmm_inputs("hmm_fit", p, theta, prior, U, B)
    out = _hmm_buffers(N, F, M, p.device)
    trace = torch.full((num_iter,), float("nan"), dtype=torch.float64, device=p.device)

    def step(it):
        _hmm_estep(p, N, F, theta, prior, U, B, out)
        hmm_mstep(out["rows"], theta, trace, it, U, B)

    state = _chain_em(step, trace, num_iter, tol, chunk, progress_bar)
    _hmm_estep(p, N, F, theta, prior, U, B, out)
    order = hmm_canonical_order(theta, U, B)
    out = hmm_permute(order, M, theta=theta, **out)
    loglik = out["rows"][:, -1].sum().item()
    n_params = M * (M - 1) + (M - 1)
    return {**out, "trace": trace[: state["iterations"]], **state, "loglik": loglik, "n_params": n_params,
            "bic": -2.0 * loglik + n_params * math.log(N * F), "order": order}


def hmm_viterbi(p, theta, prior, unbound=1, bound=1):
    """MAP path in hidden states of every row of ``p`` (N, F) under the chain ``theta`` and the evidence of ``hmm_estep``:
    (N, F) uint8 on the device; ``path >= unbound`` is its class.  A tie takes the lowest state."""
    p, N, F, theta, prior, U, B, M = _hmm_inputs("hmm_viterbi", p, theta, prior, unbound, bound)
    back = torch.empty(((F + 3) // 4) * N, dtype=torch.int32, device=p.device)
    path = torch.empty(N, F, dtype=torch.uint8, device=p.device)
    a = _lib_hmm.HmmViterbiArgs(p=_lib.ptr(p), theta=_lib.ptr(theta), back=_lib.ptr(back), path=_lib.ptr(path), N=N, F=F,
                                U=U, B=B, prior=prior)
    _lib.check(_lib_hmm.lib().tq_hmm_viterbi(C.byref(a), _stream(p.device)), "tq_hmm_viterbi")
    return path


def _hmm_sample_inputs(who, filt, theta, unbound, bound, num_samples):
    """What the multi-state backward samplers share: ``filt`` as contiguous float64 (N, F, M) on the device, ``theta`` as
    M * M + M doubles on the same device, U, B, M, S, N and F."""
    if not isinstance(filt, torch.Tensor) or filt.device.type != "cuda":
        raise HipExtensionError(f"{who} runs on the HIP device only (no CPU fallback): pass a cuda tensor")
    U, B, M = _hmm_states(who, unbound, bound)
    S = int(num_samples)
    if (filt.ndim != 3 or 0 in filt.shape or filt.shape[2] != M or filt.dtype != torch.float64 or S < 1
            or filt.shape[1] > _lib_smooth.SMOOTH_MAX_F):
        raise ValueError(f"{who}: filt must be float64 (N, F, {M}) with N >= 1, 1 <= F <= {_lib_smooth.SMOOTH_MAX_F}, "
                         f"and num_samples >= 1, got {filt.dtype} {tuple(filt.shape)}")
    theta = _hmm_theta(who, theta, M, filt.device)
    return filt.contiguous(), theta, U, B, M, S, filt.shape[0], filt.shape[1]


def hmm_sample(filt, theta, unbound, bound, num_samples, seed=0, trans=False, raster=False):
    """``num_samples`` posterior rasters of the chain in hidden states, drawn by backward sampling from ``filt`` (N, F, M)
    of ``hmm_estep`` at ``theta``, and their counts.

    Returns a dict with ``"counts"`` (num_samples, N, 4) int32, the class-level counts in the layout of ``rates_sample``
    (``rates_estimate`` takes them as they are); with ``trans=True`` also ``"trans"`` (num_samples, N, M * M) int32, the
    number of frame pairs in states (i, j), for ``hmm_estimate``; with ``raster=True`` also ``"raster"`` (num_samples, N, F)
    uint8, the hidden states."""
    filt, theta, U, B, M, S, N, F = _hmm_sample_inputs("hmm_sample", filt, theta, unbound, bound, num_samples)
    out = {"counts": torch.empty(S, N, _lib_rates.RATES_COLS, dtype=torch.int32, device=filt.device)}
    if trans:
        out["trans"] = torch.empty(S, N, M * M, dtype=torch.int32, device=filt.device)
    if raster:
        out["raster"] = torch.empty(S, N, F, dtype=torch.uint8, device=filt.device)
    a = _lib_hmm.HmmCountArgs(filt=_lib.ptr(filt), theta=_lib.ptr(theta), counts=_lib.ptr(out["counts"]),
                              trans=_lib.ptr(out.get("trans")), raster=_lib.ptr(out.get("raster")), N=N, F=F, S=S, U=U, B=B,
                              seed=int(seed) & (2**64 - 1))
    _lib.check(_lib_hmm.lib().tq_hmm_count(C.byref(a), _stream(filt.device)), "tq_hmm_count")
    return out


# ---- dwell times and first binding of the multi-state chain ---------------------------------------
def _chain_dwell_launch(filt, theta, U, B, S, N, F, seed):
    def launch(**fields):
        a = _lib_hmm.ChainDwellArgs(filt=_lib.ptr(filt), theta=_lib.ptr(theta), N=N, F=F, S=S, U=U, B=B,
                                    seed=int(seed) & (2**64 - 1), **fields)
        _lib.check(_lib_hmm.lib().tq_chain_dwell(C.byref(a), _stream(filt.device)), "tq_chain_dwell")

    return launch


def hmm_dwell_sample(filt, theta, unbound, bound, num_samples, seed=0):
    """``smooth_dwell_sample`` for the chain in hidden states: launch A of the interval sampler on the class rasters
    ``hmm_sample(filt, theta, unbound, bound, num_samples, seed, raster=True)["raster"] >= unbound``, walked as they are
    drawn; neither the rasters nor the state pairs are stored.

    Returns ``{"hist_bound", "hist_unbound", "counts", "tau"}`` with the shapes and meaning of ``smooth_dwell_sample``:
    the histograms go to ``dwell_csr_from_hist`` / ``dwell_fit``, ``tau`` to ``ttfb_fit``."""
    filt, theta, U, B, M, S, N, F = _hmm_sample_inputs("hmm_dwell_sample", filt, theta, unbound, bound, num_samples)
    return _walk_count(_chain_dwell_launch(filt, theta, U, B, S, N, F, seed), S, N, F, filt.device)


def hmm_dwell_intervals(filt, theta, unbound, bound, num_samples, seed=0, sample=None, device_table=False):
    """``smooth_dwell_intervals`` for the chain in hidden states: launch A (or its result ``sample`` from
    ``hmm_dwell_sample`` with the same arguments), the exclusive scan of the row counts, and launch B.  Returns the
    DataFrame of ``dwell_intervals``; ``z`` is the class of a run, not its hidden state.  With ``device_table`` the pair
    ``dwell_intervals`` returns then."""
    given = num_samples if sample is None else sample["counts"].shape[0]
    filt, theta, U, B, M, S, N, F = _hmm_sample_inputs("hmm_dwell_intervals", filt, theta, unbound, bound, given)
    launch = _chain_dwell_launch(filt, theta, U, B, S, N, F, seed)
    if sample is None:
        sample = _walk_count(launch, S, N, F, filt.device)
    return _walk_emit("hmm_dwell_intervals", launch, sample, S, N, filt.device, device_table)


def hmm_estimate(trans, bootstrap=False, seed=0):
    """The transition matrix of every posterior sample from the state-pair counts ``trans`` (S, N, M * M) of
    ``hmm_sample``: pooled over the AOIs, or with ``bootstrap=True`` over N AOIs drawn with replacement -- the AOIs that
    ``rates_estimate`` draws for the same ``seed``.  Returns ``"A"`` (S, M, M) float64, rows of counts divided by their
    sums (NaN for a state never visited), and ``"totals"`` (S, M, M) int64, on the device."""
    import math

    if not isinstance(trans, torch.Tensor) or trans.device.type != "cuda":
        raise HipExtensionError("hmm_estimate runs on the HIP device only (no CPU fallback): pass a cuda tensor")
    M = math.isqrt(trans.shape[2]) if trans.ndim == 3 else 0
    if (trans.ndim != 3 or M * M != trans.shape[2] or not 2 <= M <= _lib_hmm.HMM_MAX_STATES or trans.dtype != torch.int32
            or 0 in trans.shape):
        raise ValueError(f"hmm_estimate: trans must be int32 (S, N, M * M) with S, N >= 1 and M in 2 .. "
                         f"{_lib_hmm.HMM_MAX_STATES}, got {trans.dtype} {tuple(trans.shape)}")
    trans = trans.contiguous()
    S, N = trans.shape[:2]
    totals = torch.empty(S, M, M, dtype=torch.int64, device=trans.device)
    est = torch.empty(S, M, M, dtype=torch.float64, device=trans.device)
    a = _lib_hmm.HmmEstimateArgs(trans=_lib.ptr(trans), totals=_lib.ptr(totals), estimand=_lib.ptr(est), N=N, S=S, U=1,
                                 B=M - 1, resample=1 if bootstrap else 0, seed=int(seed) & (2**64 - 1))
    _lib.check(_lib_hmm.lib().tq_hmm_estimate(C.byref(a), _stream(trans.device)), "tq_hmm_estimate")
    return {"A": est, "totals": totals}


def hmm_summary(estimate, probs=0.68):
    """``rates_summary`` per entry of A: ``{"A<i><j>": {"mean", "ll", "ul", "left_out"}}`` over the finite estimands of
    ``hmm_estimate``."""
    A = estimate["A"]
    M = A.shape[1]
    return {f"A{i}{j}": estimand_summary(A[:, i, j], probs) for i in range(M) for j in range(M)}


# ---- several EM starts side by side and constrained topologies (`smooth --restarts`) ---------------
MULTISTART_SCRATCH_BYTES = 8 * 2**30  # the largest scratch of a_f that hmm_fit_restarts allocates


def hmm_allow(allow, M, who="hmm_allow"):
    """The topology ``allow`` as an (M, M) bool tensor on the host: True where A_ij is free.  ``None`` is the fully
    connected chain.  Self-transitions are always free, so every row has a free entry."""
    if allow is None:
        return torch.ones(M, M, dtype=torch.bool)
    a = torch.as_tensor(allow).detach().cpu()
    if a.shape != (M, M) or not bool(((a == 0) | (a == 1)).all()):
        raise ValueError(f"{who}: allow must be ({M}, {M}) booleans, got {tuple(a.shape)}")
    a = a.bool()
    if not bool(a.diagonal().all()):
        raise ValueError(f"{who}: allow must leave every self-transition A_ii free")
    return a


def hmm_n_params(allow):
    """Free parameters of a chain with the topology ``allow`` (M, M): (free entries of A - M) + (M - 1)."""
    M = allow.shape[0]
    return int(allow.sum()) - M + (M - 1)


def _hmm_draw_start(rng, M, free):
    """One random start (M * M + M,) from ``rng``, in the order of draws that ``hmm_random_starts`` documents."""
    import numpy as np

    A = np.zeros((M, M))
    for i in range(M):
        leave = 10.0 ** rng.uniform(-2.5, -0.3)
        js = [j for j in range(M) if j != i and free[i, j]]
        if js:
            A[i, js] = leave * rng.dirichlet(np.ones(len(js)))
            A[i, i] = 1.0 - leave
        else:
            A[i, i] = 1.0
    return np.concatenate([A.ravel(), rng.dirichlet(np.ones(M))])


def hmm_random_starts(unbound, bound, restarts, seed=0, allow=None):
    """``restarts`` + 1 starts of the EM as (restarts + 1, M * M + M) float64 on the host, theta = (A row-major, rho).

    Row 0 is ``hmm_default_start``; with ``allow`` its forbidden entries are zeroed and its rows renormalised.  Rows 1 ...
    come from ``numpy.random.default_rng(seed)``, the draws of a start taken in this order: for state i = 0 .. M - 1,
    ``leave = 10 ** rng.uniform(-2.5, -0.3)`` and then ``w = rng.dirichlet(ones(k))`` over the k allowed off-diagonal
    entries of row i in ascending j, giving A_ij = leave * w and A_ii = 1 - leave; after the M rows,
    ``rho = rng.dirichlet(ones(M))``.  A row with k = 0 still takes its ``leave`` draw (so the draws of the other rows do
    not depend on the topology of this one) but no Dirichlet draw, and has A_ii = 1.  Forbidden entries are exact zeros
    here; the kernels read them at the floor of theta, 1e-9."""
    import numpy as np

    U, B, M = _hmm_states("hmm_random_starts", unbound, bound)
    restarts = int(restarts)
    if restarts < 0 or restarts + 1 > _lib_multistart.MULTISTART_MAX:
        raise ValueError(f"hmm_random_starts: restarts must lie in 0 .. {_lib_multistart.MULTISTART_MAX - 1}, got {restarts}")
    free = hmm_allow(allow, M, "hmm_random_starts").numpy()
    A, rho = hmm_default_start(U, B)
    A = A.numpy()
    for i in range(M):
        if not free[i].all():  # a row without forbidden entries keeps the bits of hmm_default_start
            A[i] = A[i] * free[i] / (A[i] * free[i]).sum()
    out = np.zeros((restarts + 1, M * M + M))
    out[0] = np.concatenate([A.ravel(), rho.numpy()])
    rng = np.random.default_rng(seed)
    for r in range(1, restarts + 1):
        out[r] = _hmm_draw_start(rng, M, free)
    return torch.from_numpy(out)


def _multistart_inputs(who, x, shape_tail, what):
    if not isinstance(x, torch.Tensor) or x.device.type != "cuda":
        raise HipExtensionError(f"{who} runs on the HIP device only (no CPU fallback): pass a cuda tensor")
    if (x.dtype != torch.float64 or not x.is_contiguous() or x.ndim != len(shape_tail) + 1
            or tuple(x.shape[1:]) != shape_tail or not 1 <= x.shape[0] <= _lib_multistart.MULTISTART_MAX):
        raise ValueError(f"{who}: {what} must be contiguous float64 (R, {', '.join(map(str, shape_tail))}) with 1 <= R <= "
                         f"{_lib_multistart.MULTISTART_MAX}, got {x.dtype} {tuple(x.shape)}")
    return x


def _multistart_active(who, active, R, device):
    if active is None:
        return None
    if (not isinstance(active, torch.Tensor) or active.device != device or active.dtype != torch.int32
            or active.shape != (R,) or not active.is_contiguous()):
        raise ValueError(f"{who}: active must be int32 ({R},) on the device of the data")
    return active


def multistart_estep(p, thetas, prior, unbound=1, bound=1, active=None, rows=None, scratch=None):
    """One launch of ``tq_multistart_estep``: the E-step of ``hmm_estep`` for the R chains ``thetas`` (R, M * M + M) on the
    shared rows of ``p`` (N, F).  Returns ``rows`` (R, N, M * M + M + 1); gamma is not computed.  ``active`` (R,) int32 on
    the device leaves the rows of a replica with a 0 as they are; ``rows`` and ``scratch`` (R, N, F, M) are reused when
    given."""
    if not isinstance(p, torch.Tensor) or p.device.type != "cuda":
        raise HipExtensionError("multistart_estep runs on the HIP device only (no CPU fallback): pass a cuda tensor")
    U, B, M = _hmm_states("multistart_estep", unbound, bound)
    thetas = _multistart_inputs("multistart_estep", thetas, (M * M + M,), "thetas")
    R = thetas.shape[0]
    p, N, F, _, prior, U, B, M = _hmm_inputs("multistart_estep", p, thetas[0], prior, U, B)
    active = _multistart_active("multistart_estep", active, R, p.device)
    if rows is None:
        rows = torch.empty(R, N, _lib_hmm.hmm_cols(M), dtype=torch.float64, device=p.device)
    if scratch is None:
        scratch = torch.empty(R, N, F, M, dtype=torch.float64, device=p.device)
    for name, x, shape in (("rows", rows, (R, N, _lib_hmm.hmm_cols(M))), ("scratch", scratch, (R, N, F, M))):
        if x.shape != shape or x.dtype != torch.float64 or x.device != p.device or not x.is_contiguous():
            raise ValueError(f"multistart_estep: {name} must be contiguous float64 {shape} on the device of p")
    a = _lib_multistart.MultistartEstepArgs(p=_lib.ptr(p), theta=_lib.ptr(thetas), filt=_lib.ptr(scratch), rows=_lib.ptr(rows),
                                            active=_lib.ptr(active), N=N, F=F, R=R, U=U, B=B, prior=prior)
    _lib.check(_lib_multistart.lib().tq_multistart_estep(C.byref(a), _stream(p.device)), "tq_multistart_estep")
    return rows


def multistart_mstep(rows, thetas, trace, it=0, unbound=1, bound=1, allow=None, active=None):
    """One launch of ``tq_multistart_mstep``: ``thetas`` (R, M * M + M, in place) from the summed ``rows`` (R, N, M * M + M
    + 1) of ``multistart_estep`` under the topology ``allow`` (M, M), and every replica's total log-evidence into
    ``trace[r, it]``, trace (R, T).  A forbidden A_ij is pinned at the floor of theta, 1e-9, not at an exact zero.  A
    replica with ``active[r] == 0`` keeps its theta and its trace.  Returns ``thetas``."""
    if not isinstance(rows, torch.Tensor) or rows.device.type != "cuda":
        raise HipExtensionError("multistart_mstep runs on the HIP device only (no CPU fallback): pass a cuda tensor")
    U, B, M = _hmm_states("multistart_mstep", unbound, bound)
    if rows.ndim != 3 or rows.shape[1] < 1:
        raise ValueError(f"multistart_mstep: rows must be (R, N, {_lib_hmm.hmm_cols(M)}) with N >= 1")
    rows = _multistart_inputs("multistart_mstep", rows, (rows.shape[1], _lib_hmm.hmm_cols(M)), "rows")
    R, N = rows.shape[:2]
    it = int(it)
    for name, x, ok in (("thetas", thetas, lambda x: x.shape == (R, M * M + M)),
                        ("trace", trace, lambda x: x.ndim == 2 and x.shape[0] == R and 0 <= it < x.shape[1])):
        if (not isinstance(x, torch.Tensor) or x.device != rows.device or x.dtype != torch.float64 or not x.is_contiguous()
                or not ok(x)):
            raise ValueError(f"multistart_mstep: {name} must be contiguous float64 on the device of rows, thetas "
                             f"({R}, {M * M + M}) and trace ({R}, T) with 0 <= it < T")
    active = _multistart_active("multistart_mstep", active, R, rows.device)
    bits = _lib_multistart.allow_bits(hmm_allow(allow, M, "multistart_mstep").tolist())
    a = _lib_multistart.MultistartMstepArgs(rows=_lib.ptr(rows), theta=_lib.ptr(thetas), trace=_lib.ptr(trace),
                                            active=_lib.ptr(active), N=N, it=it, T=trace.shape[1], R=R, U=U, B=B, allow=bits)
    _lib.check(_lib_multistart.lib().tq_multistart_mstep(C.byref(a), _stream(rows.device)), "tq_multistart_mstep")
    return thetas


def _chain_em(step, trace, num_iter, tol, chunk, progress_bar=None):
    """The chunks and the stopping rule of ``smooth_fit``, ``hmm_fit`` and ``timed_fit``.  ``step(it)`` launches iteration
    ``it`` -- E-step and M-step -- on buffers the caller owns, among them ``trace`` (num_iter,), NaN where nothing is
    written.  The iterations run in chunks of ``chunk`` with no host synchronisation inside a chunk; after each chunk the
    trace is read, and the run stops once some iteration has gained at most ``tol * |loglik|`` over the one before.
    Returns ``{"iterations", "converged"}``: the number run (whole chunks) and whether the rule stopped it."""
    state = {"iterations": 0, "converged": False}

    def em_steps(step0, n):
        if state["converged"]:
            return
        for it in range(step0, step0 + n):
            step(it)
        state["iterations"] = step0 + n
        ll = trace[: step0 + n].cpu()
        gain = ll[1:] - ll[:-1]
        state["converged"] = bool((gain <= tol * ll[1:].abs()).any())

    _run_chunks(em_steps, num_iter, chunk, progress_bar)
    return state


def multistart_em(estep, mstep, trace, active, num_iter, tol, chunk, progress_bar=None):
    """The chunks and the stopping rule of ``hmm_fit``, applied per replica.  ``estep()`` and ``mstep(it)`` launch one
    batched step on buffers the caller owns, among them ``trace`` (R, num_iter), NaN where nothing is written, and
    ``active`` (R,) int32, all ones.  After each chunk the trace is read, a replica some iteration of which has gained at
    most ``tol * |loglik|`` over the one before is marked inactive (one copy into ``active``), and the run stops when none
    is active: a replica ends after the whole chunks, and at the theta, that ``hmm_fit`` from its start would end with.
    Returns the lists ``iterations`` and ``converged`` (R,)."""
    R = trace.shape[0]
    iterations, converged = [0] * R, [False] * R

    def em_steps(step0, n):
        if all(converged):
            return
        for it in range(step0, step0 + n):
            estep()
            mstep(it)
        ll = trace[:, : step0 + n].cpu()
        for r in range(R):
            if not converged[r]:
                iterations[r] = step0 + n
                gain = ll[r, 1:] - ll[r, :-1]
                converged[r] = bool((gain <= tol * ll[r, 1:].abs()).any())
        active.copy_(torch.tensor([0 if c else 1 for c in converged], dtype=torch.int32))

    _run_chunks(em_steps, num_iter, chunk, progress_bar)
    return iterations, converged


def hmm_fit_restarts(p, prior, unbound, bound, restarts=8, seed=0, allow=None, starts=None, num_iter=200, tol=1e-9, chunk=50,
                     progress_bar=None):
    """``hmm_fit`` from R = ``restarts`` + 1 starts at once -- ``hmm_random_starts(unbound, bound, restarts, seed, allow)``,
    or the rows of ``starts`` (R, M * M + M), normalised as ``hmm_fit`` normalises A0 and rho0 -- under the topology
    ``allow`` (M, M; True where A_ij is free, None: fully connected), and the best of them.

    Every EM iteration is one batched E-step and one batched M-step for all replicas (``multistart_em``), so R fits cost
    the launches of one; a replica that meets the stopping rule of ``hmm_fit`` is frozen at the iteration count and the
    theta ``hmm_fit`` from the same start would return.  One more batched E-step gives every replica's final log-evidence;
    the best replica is the largest, a tie going to the lowest index.  For the best replica only, the closing E-step, the
    canonical order and the relabelling of ``hmm_fit`` follow; ``allow`` is relabelled with the states.

    Returns what ``hmm_fit`` returns for the winner -- ``theta``, ``gamma``, ``filt``, ``rows``, ``trace``, ``loglik``,
    ``order`` -- with ``n_params`` = (free entries of A - M) + (M - 1) and ``bic`` from that, and for all replicas
    ``best``, ``logliks`` (R,) float64 on the host, the lists ``iterations`` and ``converged`` (R,) (the winner's are
    ``iterations[best]`` and ``converged[best]``), ``thetas`` (R, M * M + M) in the order of the states the EM ran in,
    ``traces`` (R, T) with NaN after a replica's stop, ``starts`` (R, M * M + M) and ``allow`` (M, M) bool."""
    import math

    num_iter = int(num_iter)
    U, B, M = _hmm_states("hmm_fit_restarts", unbound, bound)
    free = hmm_allow(allow, M, "hmm_fit_restarts")
    if starts is None:
        starts = hmm_random_starts(U, B, restarts, seed, free)
    starts = torch.as_tensor(starts, dtype=torch.float64).detach().cpu()
    if (num_iter < 1 or starts.ndim != 2 or starts.shape[1] != M * M + M
            or not 1 <= starts.shape[0] <= _lib_multistart.MULTISTART_MAX or not bool((starts >= 0).all())):
        raise ValueError(f"hmm_fit_restarts: num_iter must be positive and starts (R, {M * M + M}) non-negative with 1 <= R "
                         f"<= {_lib_multistart.MULTISTART_MAX}")
    R = starts.shape[0]
    A, rho = starts[:, : M * M].reshape(R, M, M), starts[:, M * M:]
    if not bool((A.sum(2) > 0).all()) or not bool((rho.sum(1) > 0).all()):
        raise ValueError("hmm_fit_restarts: every row of A and every rho of starts must have a positive sum")
    if not isinstance(p, torch.Tensor) or p.device.type != "cuda":
        raise HipExtensionError("hmm_fit_restarts runs on the HIP device only (no CPU fallback): pass a cuda tensor")
    # row by row the expression of hmm_fit, so that a replica starts from the bits hmm_fit starts from
    thetas = torch.stack([torch.cat([(A[r] / A[r].sum(1, keepdim=True)).reshape(-1), rho[r] / rho[r].sum()])
                          for r in range(R)]).to(p.device)
    p, N, F, _, prior, U, B, M = _hmm_inputs("hmm_fit_restarts", p, thetas[0], prior, U, B)
    if R * N * F * M * 8 > MULTISTART_SCRATCH_BYTES:
        raise ValueError(f"hmm_fit_restarts: the scratch of R = {R} replicas, N = {N} rows, F = {F} frames and M = {M} states "
                         f"takes {R * N * F * M * 8} bytes, more than {MULTISTART_SCRATCH_BYTES}: use fewer restarts")
    dev = p.device
    rows = torch.empty(R, N, _lib_hmm.hmm_cols(M), dtype=torch.float64, device=dev)
    scratch = torch.empty(R, N, F, M, dtype=torch.float64, device=dev)
    trace = torch.full((R, num_iter), float("nan"), dtype=torch.float64, device=dev)
    active = torch.ones(R, dtype=torch.int32, device=dev)
    iterations, converged = multistart_em(
        lambda: multistart_estep(p, thetas, prior, U, B, active, rows, scratch),
        lambda it: multistart_mstep(rows, thetas, trace, it, U, B, free, active), trace, active, num_iter, tol, chunk,
        progress_bar)
    multistart_estep(p, thetas, prior, U, B, None, rows, scratch)
    logliks = rows[:, :, -1].sum(1).cpu()
    finite = torch.where(torch.isnan(logliks), torch.full_like(logliks, -math.inf), logliks)
    best = min(r for r in range(R) if finite[r] == finite.max())
    del scratch
    theta = thetas[best].clone()
    out = _hmm_estep(p, N, F, theta, prior, U, B, _hmm_buffers(N, F, M, dev))
    order = hmm_canonical_order(theta, U, B)
    out = hmm_permute(order, M, theta=theta, **out)
    idx = torch.as_tensor(order, dtype=torch.int64)
    loglik = out["rows"][:, -1].sum().item()
    n_params = hmm_n_params(free)
    return {**out, "trace": trace[best, : iterations[best]], "iterations": iterations, "converged": converged,
            "loglik": loglik, "n_params": n_params, "bic": -2.0 * loglik + n_params * math.log(N * F), "order": order,
            "best": best, "logliks": logliks, "thetas": thetas, "traces": trace[:, : max(iterations)], "starts": starts,
            "allow": free[idx][:, idx]}


# ---- bootstrap refits of the chain over AOIs (`smooth --refit`) -------------------------------------
def refit_weights(N, refits, seed=0, first=0, device="cuda"):
    """One launch of ``tq_refit_weights``: (``refits``, N) int32 on ``device``, row r the number of times each of the N
    AOIs is drawn by sample ``first`` + r of the bootstrap over AOIs of ``rates_estimate`` / ``hmm_estimate`` at the same
    ``seed``.  Every row sums to N; ``first`` batches the rows without changing any of them."""
    device = torch.device(device)
    if device.type != "cuda":
        raise HipExtensionError("refit_weights runs on the HIP device only (no CPU fallback): pass a cuda device")
    N, R, first = int(N), int(refits), int(first)
    if N < 1 or not 1 <= R <= _lib_multistart.MULTISTART_MAX or first < 0 or first + R > 2**31 - 1:
        raise ValueError(f"refit_weights: N must be positive, 1 <= refits <= {_lib_multistart.MULTISTART_MAX} and first "
                         f"non-negative, got N = {N}, refits = {R}, first = {first}")
    weights = torch.empty(R, N, dtype=torch.int32, device=device)
    a = _lib_refit.RefitWeightsArgs(weights=_lib.ptr(weights), N=N, R=R, first=first, seed=int(seed) & (2**64 - 1))
    _lib.check(_lib_refit.lib().tq_refit_weights(C.byref(a), _stream(weights.device)), "tq_refit_weights")
    return weights


def _refit_weights_arg(who, weights, R, N, device):
    if (not isinstance(weights, torch.Tensor) or weights.device != device or weights.dtype != torch.int32
            or weights.shape != (R, N) or not weights.is_contiguous()):
        raise ValueError(f"{who}: weights must be contiguous int32 ({R}, {N}) on the device of the data")
    return weights


def refit_estep(p, thetas, weights, prior, unbound=1, bound=1, active=None, rows=None, scratch=None):
    """One launch of ``tq_refit_estep``: ``multistart_estep`` that leaves out every pair (replica r, AOI n) with
    ``weights[r, n] == 0``, weights (R, N) int32 on the device.  The rows and the scratch of such a pair keep what they
    held (a fresh ``rows`` holds zeros there); where the weight is positive the rows are those of ``multistart_estep``
    bit for bit.  Returns ``rows`` (R, N, M * M + M + 1)."""
    if not isinstance(p, torch.Tensor) or p.device.type != "cuda":
        raise HipExtensionError("refit_estep runs on the HIP device only (no CPU fallback): pass a cuda tensor")
    U, B, M = _hmm_states("refit_estep", unbound, bound)
    thetas = _multistart_inputs("refit_estep", thetas, (M * M + M,), "thetas")
    R = thetas.shape[0]
    p, N, F, _, prior, U, B, M = _hmm_inputs("refit_estep", p, thetas[0], prior, U, B)
    active = _multistart_active("refit_estep", active, R, p.device)
    weights = _refit_weights_arg("refit_estep", weights, R, N, p.device)
    if rows is None:
        rows = torch.zeros(R, N, _lib_hmm.hmm_cols(M), dtype=torch.float64, device=p.device)
    if scratch is None:
        scratch = torch.empty(R, N, F, M, dtype=torch.float64, device=p.device)
    for name, x, shape in (("rows", rows, (R, N, _lib_hmm.hmm_cols(M))), ("scratch", scratch, (R, N, F, M))):
        if x.shape != shape or x.dtype != torch.float64 or x.device != p.device or not x.is_contiguous():
            raise ValueError(f"refit_estep: {name} must be contiguous float64 {shape} on the device of p")
    a = _lib_refit.RefitEstepArgs(p=_lib.ptr(p), theta=_lib.ptr(thetas), filt=_lib.ptr(scratch), rows=_lib.ptr(rows),
                                  active=_lib.ptr(active), weights=_lib.ptr(weights), N=N, F=F, R=R, U=U, B=B, prior=prior)
    _lib.check(_lib_refit.lib().tq_refit_estep(C.byref(a), _stream(p.device)), "tq_refit_estep")
    return rows


def refit_mstep(rows, thetas, weights, trace, it=0, unbound=1, bound=1, allow=None, active=None):
    """One launch of ``tq_refit_mstep``: ``multistart_mstep`` with row n of replica r counted ``weights[r, n]`` times and
    the sum of the weights in the place of N; ``trace[r, it]`` receives the weighted log evidence.  A row of weight 0 is
    never read.  With all weights 1 ``thetas`` and ``trace`` are those of ``multistart_mstep`` bit for bit.  Returns
    ``thetas``."""
    if not isinstance(rows, torch.Tensor) or rows.device.type != "cuda":
        raise HipExtensionError("refit_mstep runs on the HIP device only (no CPU fallback): pass a cuda tensor")
    U, B, M = _hmm_states("refit_mstep", unbound, bound)
    if rows.ndim != 3 or rows.shape[1] < 1:
        raise ValueError(f"refit_mstep: rows must be (R, N, {_lib_hmm.hmm_cols(M)}) with N >= 1")
    rows = _multistart_inputs("refit_mstep", rows, (rows.shape[1], _lib_hmm.hmm_cols(M)), "rows")
    R, N = rows.shape[:2]
    it = int(it)
    for name, x, ok in (("thetas", thetas, lambda x: x.shape == (R, M * M + M)),
                        ("trace", trace, lambda x: x.ndim == 2 and x.shape[0] == R and 0 <= it < x.shape[1])):
        if (not isinstance(x, torch.Tensor) or x.device != rows.device or x.dtype != torch.float64 or not x.is_contiguous()
                or not ok(x)):
            raise ValueError(f"refit_mstep: {name} must be contiguous float64 on the device of rows, thetas "
                             f"({R}, {M * M + M}) and trace ({R}, T) with 0 <= it < T")
    active = _multistart_active("refit_mstep", active, R, rows.device)
    weights = _refit_weights_arg("refit_mstep", weights, R, N, rows.device)
    bits = _lib_multistart.allow_bits(hmm_allow(allow, M, "refit_mstep").tolist())
    a = _lib_refit.RefitMstepArgs(rows=_lib.ptr(rows), theta=_lib.ptr(thetas), trace=_lib.ptr(trace), active=_lib.ptr(active),
                                  weights=_lib.ptr(weights), N=N, it=it, T=trace.shape[1], R=R, U=U, B=B, allow=bits)
    _lib.check(_lib_refit.lib().tq_refit_mstep(C.byref(a), _stream(rows.device)), "tq_refit_mstep")
    return thetas


REFIT_MAX = 4096  # the largest `refits` of hmm_fit_refits


def hmm_fit_refits(p, prior, theta_hat, unbound, bound, refits, seed=0, allow=None, num_iter=200, tol=1e-9, chunk=50,
                   progress_bar=None):
    """Non-parametric bootstrap of the EM fit over the AOIs: ``refits`` + 1 fits of the chain of ``hmm_fit`` to the rows
    of ``p`` (N, F), all warm-started at ``theta_hat`` (M * M + M,), under the topology ``allow``.

    Replica 0 has every weight 1: the data as they are, fitted by the same kernels, the like-for-like reference point of
    the others.  Replica r >= 1 is the resample of N AOIs with replacement that ``rates_estimate`` / ``hmm_estimate`` draw
    for sample r - 1 at the same ``seed`` (``refit_weights(N, ., seed, first=r - 1)``), as a weight per AOI.  The replicas
    are fitted in batches of at most 64 by ``multistart_em`` -- its freezing and its stopping rule, applied to the
    weighted log evidence -- on ``refit_estep`` / ``refit_mstep``; a replica's result does not depend on its batch.  Every
    refitted theta is put in the order of ``hmm_canonical_order``.

    Returns ``thetas`` (refits + 1, M * M + M) and ``logliks`` (refits + 1,) -- the weighted log evidence at the final
    theta -- and ``pairs`` (refits + 1, M, M) -- the weighted expected number of frame pairs in states (i, j) there, whose
    class blocks give kon and koff as `smooth` defines them -- float64 on the host, in the canonical order;
    ``traces`` (refits + 1, num_iter) in the order the EM ran in, with NaN after a replica's stop, ``orders`` (the
    permutation applied to every replica's theta), the lists ``iterations`` and ``converged``, ``seed`` and ``refits``."""
    num_iter, refits = int(num_iter), int(refits)
    U, B, M = _hmm_states("hmm_fit_refits", unbound, bound)
    free = hmm_allow(allow, M, "hmm_fit_refits")
    if num_iter < 1 or not 0 <= refits <= REFIT_MAX:
        raise ValueError(f"hmm_fit_refits: num_iter must be positive and refits lie in 0 .. {REFIT_MAX}, got {num_iter} "
                         f"and {refits}")
    if not isinstance(p, torch.Tensor) or p.device.type != "cuda":
        raise HipExtensionError("hmm_fit_refits runs on the HIP device only (no CPU fallback): pass a cuda tensor")
    start = torch.as_tensor(theta_hat, dtype=torch.float64).detach().reshape(-1).to(p.device)
    p, N, F, start, prior, U, B, M = _hmm_inputs("hmm_fit_refits", p, start, prior, U, B)
    dev, batch = p.device, _lib_multistart.MULTISTART_MAX
    if min(refits + 1, batch) * N * F * M * 8 > MULTISTART_SCRATCH_BYTES:
        raise ValueError(f"hmm_fit_refits: the scratch of a batch of {min(refits + 1, batch)} replicas, N = {N} rows, F = {F} "
                         f"frames and M = {M} states takes more than {MULTISTART_SCRATCH_BYTES} bytes")
    out_thetas, out_ll, pairs, traces, orders, iterations, converged = [], [], [], [], [], [], []
    for g0 in range(0, refits + 1, batch):  # replicas g0 .. g0 + R - 1
        R = min(batch, refits + 1 - g0)
        if g0 == 0:
            parts = [torch.ones(1, N, dtype=torch.int32, device=dev)]
            if R > 1:
                parts.append(refit_weights(N, R - 1, seed, 0, dev))
            weights = torch.cat(parts).contiguous()
        else:
            weights = refit_weights(N, R, seed, g0 - 1, dev)
        thetas = start.reshape(1, -1).repeat(R, 1).contiguous()
        rows = torch.zeros(R, N, _lib_hmm.hmm_cols(M), dtype=torch.float64, device=dev)
        scratch = torch.empty(R, N, F, M, dtype=torch.float64, device=dev)
        trace = torch.full((R, num_iter), float("nan"), dtype=torch.float64, device=dev)
        active = torch.ones(R, dtype=torch.int32, device=dev)
        its, conv = multistart_em(
            lambda: refit_estep(p, thetas, weights, prior, U, B, active, rows, scratch),
            lambda it: refit_mstep(rows, thetas, weights, trace, it, U, B, free, active), trace, active, num_iter, tol,
            chunk, progress_bar)
        refit_estep(p, thetas, weights, prior, U, B, None, rows, scratch)
        ll = rows[:, :, -1]
        out_ll.append(torch.where(weights > 0, weights.double() * ll, torch.zeros_like(ll)).sum(1).cpu())
        drawn = (weights > 0)[:, :, None]  # a row of weight 0 was never written: left out, not multiplied by 0
        pair = torch.where(drawn, weights.double()[:, :, None] * rows[:, :, : M * M], torch.zeros_like(rows[:, :, : M * M]))
        pair = pair.sum(1).reshape(R, M, M).cpu()
        host = thetas.cpu()
        orders += [hmm_canonical_order(host[r], U, B) for r in range(R)]
        for r, order in zip(range(R), orders[g0:]):
            out_thetas.append(hmm_permute(order, M, theta=host[r])["theta"])
            pairs.append(pair[r][order][:, order])
        traces.append(trace.cpu())
        iterations += its
        converged += conv
        del scratch
    return {"thetas": torch.stack(out_thetas), "logliks": torch.cat(out_ll), "pairs": torch.stack(pairs),
            "traces": torch.cat(traces), "orders": orders,
            "iterations": iterations, "converged": converged, "seed": int(seed), "refits": refits}


# ---- a mixture of chains over the AOIs (`smooth --populations`) ------------------------------------
def _mixture_pops(who, populations):
    G = int(populations)
    if not 1 <= G <= _lib_mixture.MIXTURE_MAX_POP:
        raise ValueError(f"{who}: populations must lie in 1 .. {_lib_mixture.MIXTURE_MAX_POP}, got {populations}")
    return G


def mixture_n_params(allow, populations):
    """Free parameters of a mixture of G chains of the topology ``allow``: G chains of ``hmm_n_params`` and G - 1 weights."""
    return populations * hmm_n_params(allow) + populations - 1


def mixture_default_start(unbound, bound, populations, allow=None):
    """The deterministic default start of ``mixture_fit`` as (thetas (G, M * M + M), phi (G,)) float64 on the host:
    population g is ``hmm_default_start`` with every off-diagonal entry of A divided by 4^g and the diagonal set to 1 minus
    the row's off-diagonal sum, so population g leaves its states 4^g times more slowly; rho and phi are uniform.  With
    ``allow`` the forbidden entries are zeroed and their rows renormalised, as ``hmm_random_starts`` does it."""
    import numpy as np

    U, B, M = _hmm_states("mixture_default_start", unbound, bound)
    G = _mixture_pops("mixture_default_start", populations)
    free = hmm_allow(allow, M, "mixture_default_start").numpy()
    A0, rho = hmm_default_start(U, B)
    thetas = np.zeros((G, M * M + M))
    for g in range(G):
        A = A0.numpy().copy()
        for i in range(M):
            A[i, i] = 0.0
            A[i] = A[i] / 4.0 ** g
            A[i, i] = 1.0 - A[i].sum()
            if not free[i].all():
                A[i] = A[i] * free[i] / (A[i] * free[i]).sum()
        thetas[g] = np.concatenate([A.ravel(), rho.numpy()])
    return torch.from_numpy(thetas), torch.full((G,), 1.0 / G, dtype=torch.float64)


def mixture_random_starts(unbound, bound, populations, restarts, seed=0, allow=None):
    """``restarts`` + 1 starts of the mixture EM as (thetas (P, G, M * M + M), phi (P, G)) float64 on the host.  Start 0 is
    ``mixture_default_start``.  Starts 1 ... come from ``numpy.random.default_rng(seed)``: for every population in turn
    the draws of a start of ``hmm_random_starts``, and after the G chains of a start ``phi = rng.dirichlet(ones(G))``.
    P * G is at most 64."""
    import numpy as np

    U, B, M = _hmm_states("mixture_random_starts", unbound, bound)
    G = _mixture_pops("mixture_random_starts", populations)
    restarts = int(restarts)
    if restarts < 0 or (restarts + 1) * G > _lib_multistart.MULTISTART_MAX:
        raise ValueError(f"mixture_random_starts: (restarts + 1) * populations must lie in 1 .. "
                         f"{_lib_multistart.MULTISTART_MAX}, got restarts = {restarts} and populations = {G}")
    free = hmm_allow(allow, M, "mixture_random_starts").numpy()
    thetas, phi = np.zeros((restarts + 1, G, M * M + M)), np.zeros((restarts + 1, G))
    t0, f0 = mixture_default_start(U, B, G, free)
    thetas[0], phi[0] = t0.numpy(), f0.numpy()
    rng = np.random.default_rng(seed)
    for p in range(1, restarts + 1):
        for g in range(G):
            thetas[p, g] = _hmm_draw_start(rng, M, free)
        phi[p] = rng.dirichlet(np.ones(G))
    return torch.from_numpy(thetas), torch.from_numpy(phi)


def mixture_mstep(rows, thetas, phi, trace, it=0, unbound=1, bound=1, allow=None, active=None, resp=None, evidence=None):
    """One launch of ``tq_mixture_mstep``: for each of P starts, the G chains ``thetas`` (P, G, M * M + M) and the weights
    ``phi`` (P, G), both in place, from ``rows`` (P, G, N, M * M + M + 1) -- ``multistart_estep`` of the P * G chains -- with
    every AOI weighted by its responsibility, under the topology ``allow``; the mixture log evidence goes into
    ``trace[p, it]``, trace (P, T).  ``resp`` (P, G, N) and ``evidence`` (P, N), when given, receive the responsibilities
    and the per-AOI log evidence at the thetas and phi the rows were computed with.  A start with ``active[p] == 0`` keeps
    everything.  Returns ``thetas``."""
    if not isinstance(rows, torch.Tensor) or rows.device.type != "cuda":
        raise HipExtensionError("mixture_mstep runs on the HIP device only (no CPU fallback): pass a cuda tensor")
    U, B, M = _hmm_states("mixture_mstep", unbound, bound)
    cols = _lib_hmm.hmm_cols(M)
    if (rows.ndim != 4 or rows.shape[3] != cols or 0 in rows.shape or rows.dtype != torch.float64 or not rows.is_contiguous()
            or rows.shape[1] > _lib_mixture.MIXTURE_MAX_POP or rows.shape[0] * rows.shape[1] > _lib_multistart.MULTISTART_MAX):
        raise ValueError(f"mixture_mstep: rows must be contiguous float64 (P, G, N, {cols}) with G <= "
                         f"{_lib_mixture.MIXTURE_MAX_POP} and P * G <= {_lib_multistart.MULTISTART_MAX}")
    P, G, N = rows.shape[:3]
    it = int(it)
    for name, x, ok in (("thetas", thetas, lambda x: x.shape == (P, G, M * M + M)), ("phi", phi, lambda x: x.shape == (P, G)),
                        ("trace", trace, lambda x: x.ndim == 2 and x.shape[0] == P and 0 <= it < x.shape[1]),
                        ("resp", resp, lambda x: x.shape == (P, G, N)), ("evidence", evidence, lambda x: x.shape == (P, N))):
        if x is None and name in ("resp", "evidence"):
            continue
        if (not isinstance(x, torch.Tensor) or x.device != rows.device or x.dtype != torch.float64 or not x.is_contiguous()
                or not ok(x)):
            raise ValueError(f"mixture_mstep: {name} must be contiguous float64 on the device of rows: thetas ({P}, {G}, "
                             f"{M * M + M}), phi ({P}, {G}), trace ({P}, T) with 0 <= it < T, resp ({P}, {G}, {N}), "
                             f"evidence ({P}, {N})")
    active = _multistart_active("mixture_mstep", active, P, rows.device)
    bits = _lib_multistart.allow_bits(hmm_allow(allow, M, "mixture_mstep").tolist())
    a = _lib_mixture.MixtureMstepArgs(rows=_lib.ptr(rows), theta=_lib.ptr(thetas), phi=_lib.ptr(phi), trace=_lib.ptr(trace),
                                      resp=_lib.ptr(resp), evidence=_lib.ptr(evidence), active=_lib.ptr(active), N=N, it=it,
                                      T=trace.shape[1], P=P, G=G, U=U, B=B, allow=bits)
    _lib.check(_lib_mixture.lib().tq_mixture_mstep(C.byref(a), _stream(rows.device)), "tq_mixture_mstep")
    return thetas


def mixture_fit(p, prior, unbound=1, bound=1, populations=2, restarts=0, seed=0, allow=None, num_iter=200, tol=1e-9,
                chunk=50, progress_bar=None, starts=None):
    """EM fit of a mixture of ``populations`` chains of ``unbound`` + ``bound`` hidden states to the rows of ``p`` (N, F):
    AOI n belongs to population g with weight phi_g and follows the chain theta_g throughout -- static heterogeneity,
    where ``hmm_fit`` with more bound states models a molecule that switches.  P = ``restarts`` + 1 starts
    (``mixture_random_starts``, or ``starts`` = (thetas (P, G, .), phi (P, G)), normalised as ``hmm_fit`` normalises its
    start) are fitted side by side: an iteration is one ``multistart_estep`` of the P * G chains and one
    ``mixture_mstep``, driven by ``multistart_em`` with the stopping rule of ``hmm_fit`` per start on the mixture log
    evidence.  A closing E-step gives every start's evidence; the best start is the largest, a tie going to the lowest
    index.  For the winner, ``hmm_estep`` per population gives ``filt`` and ``gamma``, the states of each population are
    put in ``hmm_canonical_order``, and the populations in descending phi (a tie: the lower index first).

    Returns ``thetas`` (G, M * M + M), ``phi`` (G,), ``resp`` (G, N), ``evidence`` (N,), ``loglik``, ``n_params`` =
    G (free entries of A - M + M - 1) + G - 1, ``bic`` = -2 loglik + n_params log(N F), ``trace``, ``logliks`` (P,) on the
    host, ``gamma`` (N, F, M) = sum_g resp gamma_g, ``gammas`` and ``filt`` (G, N, F, M), ``population_map`` (N,), ``best``,
    the lists ``iterations`` and ``converged`` (P,), ``traces`` (P, T), ``allows`` (G, M, M), ``orders``, and ``pair_sums``
    (G, M, M): the expected state pairs of every population, its AOIs weighted by their responsibilities."""
    import math

    num_iter = int(num_iter)
    U, B, M = _hmm_states("mixture_fit", unbound, bound)
    G = _mixture_pops("mixture_fit", populations)
    free = hmm_allow(allow, M, "mixture_fit")
    if starts is None:
        starts = mixture_random_starts(U, B, G, restarts, seed, free)
    th0 = torch.as_tensor(starts[0], dtype=torch.float64).detach().cpu()
    ph0 = torch.as_tensor(starts[1], dtype=torch.float64).detach().cpu()
    W = M * M + M
    if (num_iter < 1 or th0.ndim != 3 or th0.shape[1:] != (G, W) or ph0.shape != (th0.shape[0], G) or th0.shape[0] < 1
            or th0.shape[0] * G > _lib_multistart.MULTISTART_MAX or not bool((th0 >= 0).all()) or not bool((ph0 >= 0).all())):
        raise ValueError(f"mixture_fit: num_iter must be positive, starts non-negative (P, {G}, {W}) and (P, {G}) with "
                         f"1 <= P * {G} <= {_lib_multistart.MULTISTART_MAX}")
    P = th0.shape[0]
    A, rho = th0[..., : M * M].reshape(P * G, M, M), th0[..., M * M:].reshape(P * G, M)
    if not bool((A.sum(2) > 0).all()) or not bool((rho.sum(1) > 0).all()) or not bool((ph0.sum(1) > 0).all()):
        raise ValueError("mixture_fit: every row of A, every rho and every phi of starts must have a positive sum")
    if not isinstance(p, torch.Tensor) or p.device.type != "cuda":
        raise HipExtensionError("mixture_fit runs on the HIP device only (no CPU fallback): pass a cuda tensor")
    thetas = torch.stack([torch.cat([(A[r] / A[r].sum(1, keepdim=True)).reshape(-1), rho[r] / rho[r].sum()])
                          for r in range(P * G)]).to(p.device)  # (P * G, W): the replicas of multistart_estep
    phi = torch.stack([ph0[q] / ph0[q].sum() for q in range(P)]).to(p.device)
    p, N, F, _, prior, U, B, M = _hmm_inputs("mixture_fit", p, thetas[0], prior, U, B)
    R = P * G
    if R * N * F * M * 8 > MULTISTART_SCRATCH_BYTES:
        raise ValueError(f"mixture_fit: the scratch of R = {R} chains, N = {N} rows, F = {F} frames and M = {M} states takes "
                         f"{R * N * F * M * 8} bytes, more than {MULTISTART_SCRATCH_BYTES}: use fewer restarts")
    dev = p.device
    rows = torch.empty(R, N, _lib_hmm.hmm_cols(M), dtype=torch.float64, device=dev)
    scratch = torch.empty(R, N, F, M, dtype=torch.float64, device=dev)
    trace = torch.full((P, num_iter), float("nan"), dtype=torch.float64, device=dev)
    active = torch.ones(P, dtype=torch.int32, device=dev)
    active_r = torch.ones(R, dtype=torch.int32, device=dev)
    rows4, thetas3 = rows.view(P, G, N, -1), thetas.view(P, G, W)

    def estep():
        active_r.view(P, G).copy_(active[:, None])  # a population is a replica: active (P) expanded to (P * G)
        multistart_estep(p, thetas, prior, U, B, active_r, rows, scratch)

    iterations, converged = multistart_em(
        estep, lambda it: mixture_mstep(rows4, thetas3, phi, trace, it, U, B, free, active), trace, active, num_iter, tol,
        chunk, progress_bar)
    multistart_estep(p, thetas, prior, U, B, None, rows, scratch)
    del scratch
    closing = torch.full((P, 1), float("nan"), dtype=torch.float64, device=dev)
    resp = torch.empty(P, G, N, dtype=torch.float64, device=dev)
    evidence = torch.empty(P, N, dtype=torch.float64, device=dev)
    mixture_mstep(rows4, thetas3.clone(), phi.clone(), closing, 0, U, B, free, None, resp, evidence)
    logliks = closing[:, 0].cpu()
    finite = torch.where(torch.isnan(logliks), torch.full_like(logliks, -math.inf), logliks)
    best = min(q for q in range(P) if finite[q] == finite.max())

    weights = phi[best].cpu()
    pops = sorted(range(G), key=lambda g: -weights[g].item())  # stable: a tie keeps the lower index first
    out = {"thetas": [], "filt": [], "gammas": [], "allows": [], "orders": [], "pairs": []}
    for g in pops:
        theta = thetas3[best, g].clone()
        one = _hmm_estep(p, N, F, theta, prior, U, B, _hmm_buffers(N, F, M, dev))
        order = hmm_canonical_order(theta, U, B)
        one = hmm_permute(order, M, theta=theta, **one)
        idx = torch.as_tensor(order, dtype=torch.int64)
        out["pairs"].append((resp[best, g][:, None] * one["rows"][:, : M * M]).sum(0).reshape(M, M))
        out["thetas"].append(one["theta"])
        out["filt"].append(one["filt"])
        out["gammas"].append(one["gamma"])
        out["allows"].append(free[idx][:, idx])
        out["orders"].append(order)
    ix = torch.as_tensor(pops, dtype=torch.int64, device=dev)
    resp_best = resp[best][ix].contiguous()
    gammas = torch.stack(out["gammas"])
    loglik = logliks[best].item()
    n_params = mixture_n_params(free, G)
    return {"thetas": torch.stack(out["thetas"]), "phi": phi[best][ix].contiguous(), "resp": resp_best,
            "evidence": evidence[best].contiguous(), "loglik": loglik, "n_params": n_params,
            "bic": -2.0 * loglik + n_params * math.log(N * F), "trace": trace[best, : iterations[best]],
            "logliks": logliks, "gamma": (resp_best[:, :, None, None] * gammas).sum(0), "gammas": gammas,
            "filt": torch.stack(out["filt"]), "population_map": resp_best.argmax(0), "best": best,
            "iterations": iterations, "converged": converged, "traces": trace[:, : max(iterations)],
            "allows": torch.stack(out["allows"]), "orders": out["orders"], "populations": pops,
            "pair_sums": torch.stack(out["pairs"])}


def _mixture_chains(who, filt, thetas, resp, unbound, bound):
    """``filt`` (G, N, F, M), ``thetas`` (G, M * M + M) and ``resp`` (G, N) as contiguous float64 on one device."""
    if not isinstance(filt, torch.Tensor) or filt.device.type != "cuda":
        raise HipExtensionError(f"{who} runs on the HIP device only (no CPU fallback): pass a cuda tensor")
    U, B, M = _hmm_states(who, unbound, bound)
    if (filt.ndim != 4 or 0 in filt.shape or filt.shape[3] != M or filt.dtype != torch.float64
            or filt.shape[0] > _lib_mixture.MIXTURE_MAX_POP or filt.shape[2] > _lib_smooth.SMOOTH_MAX_F):
        raise ValueError(f"{who}: filt must be float64 (G, N, F, {M}) with 1 <= G <= {_lib_mixture.MIXTURE_MAX_POP}, N >= 1 "
                         f"and 1 <= F <= {_lib_smooth.SMOOTH_MAX_F}, got {filt.dtype} {tuple(filt.shape)}")
    G, N, F = filt.shape[:3]
    for name, x, shape in (("thetas", thetas, (G, M * M + M)), ("resp", resp, (G, N))):
        if (not isinstance(x, torch.Tensor) or x.device != filt.device or x.dtype != torch.float64 or x.shape != shape):
            raise ValueError(f"{who}: {name} must be float64 {shape} on the device of filt")
    return filt.contiguous(), thetas.contiguous(), resp.contiguous(), U, B, M, G, N, F


def mixture_sample(filt, thetas, resp, unbound, bound, num_samples, seed=0, trans=False, raster=False):
    """``num_samples`` posterior rasters of the mixture: every row (s, n) first draws its population from ``resp[:, n]``
    and is then the row ``hmm_sample`` draws from ``filt[g]`` under ``thetas[g]`` with the same seed.

    Returns ``"counts"`` (S, N, 4) int32 as ``hmm_sample`` does, ``"pop"`` (S, N) uint8, and with ``trans`` / ``raster``
    the state-pair counts (S, N, M * M) int32 and the hidden states (S, N, F) uint8.  With one population the outputs
    are those of ``hmm_sample``, bit for bit."""
    filt, thetas, resp, U, B, M, G, N, F = _mixture_chains("mixture_sample", filt, thetas, resp, unbound, bound)
    S = int(num_samples)
    if S < 1:
        raise ValueError(f"mixture_sample: num_samples must be at least 1, got {num_samples}")
    dev = filt.device
    out = {"counts": torch.empty(S, N, _lib_rates.RATES_COLS, dtype=torch.int32, device=dev),
           "pop": torch.empty(S, N, dtype=torch.uint8, device=dev)}
    if trans:
        out["trans"] = torch.empty(S, N, M * M, dtype=torch.int32, device=dev)
    if raster:
        out["raster"] = torch.empty(S, N, F, dtype=torch.uint8, device=dev)
    a = _lib_mixture.MixtureCountArgs(filt=_lib.ptr(filt), theta=_lib.ptr(thetas), resp=_lib.ptr(resp),
                                      counts=_lib.ptr(out["counts"]), trans=_lib.ptr(out.get("trans")),
                                      pop=_lib.ptr(out["pop"]), raster=_lib.ptr(out.get("raster")), N=N, F=F, S=S, G=G, U=U, B=B,
                                      seed=int(seed) & (2**64 - 1))
    _lib.check(_lib_mixture.lib().tq_mixture_count(C.byref(a), _stream(dev)), "tq_mixture_count")
    return out


# ---- dwell times and first binding of the mixture's rasters --------------------------------------
def _population_dwell_launch(filt, thetas, resp, U, B, G, S, N, F, seed):
    def launch(**fields):
        a = _lib_mixture.PopulationDwellArgs(filt=_lib.ptr(filt), theta=_lib.ptr(thetas), resp=_lib.ptr(resp), N=N, F=F, S=S,
                                             G=G, U=U, B=B, seed=int(seed) & (2**64 - 1), **fields)
        _lib.check(_lib_mixture.lib().tq_population_dwell(C.byref(a), _stream(filt.device)), "tq_population_dwell")

    return launch


def _mixture_dwell_inputs(who, filt, thetas, resp, unbound, bound, num_samples):
    filt, thetas, resp, U, B, M, G, N, F = _mixture_chains(who, filt, thetas, resp, unbound, bound)
    S = int(num_samples)
    if S < 1:
        raise ValueError(f"{who}: num_samples must be at least 1, got {num_samples}")
    return filt, thetas, resp, U, B, G, S, N, F


def mixture_dwell_sample(filt, thetas, resp, unbound, bound, num_samples, seed=0):
    """``hmm_dwell_sample`` for the mixture of chains: launch A of the interval sampler on the class rasters
    ``mixture_sample(filt, thetas, resp, unbound, bound, num_samples, seed, raster=True)["raster"] >= unbound``, walked as
    they are drawn with the population every row draws; neither the rasters nor the state pairs are stored.

    Returns ``"hist_bound"`` / ``"hist_unbound"`` (S, G, F) int32 -- the interior runs of the rows a sample drew into
    population g, by dwell time; ``hist[:, g]`` goes to ``dwell_csr_from_hist`` / ``dwell_fit`` --, ``"counts"`` (S, N)
    int32, ``"tau"`` (S, N) float32 and ``"pop"`` (S, N) uint8, the population of ``mixture_sample``.  With one population
    the outputs are those of ``hmm_dwell_sample``, bit for bit."""
    filt, thetas, resp, U, B, G, S, N, F = _mixture_dwell_inputs("mixture_dwell_sample", filt, thetas, resp, unbound, bound,
                                                                 num_samples)
    return _walk_count(_population_dwell_launch(filt, thetas, resp, U, B, G, S, N, F, seed), S, N, F, filt.device, G)


def mixture_dwell_intervals(filt, thetas, resp, unbound, bound, num_samples, seed=0, sample=None, device_table=False):
    """``hmm_dwell_intervals`` for the mixture of chains: launch A (or its result ``sample`` from ``mixture_dwell_sample``
    with the same arguments), the exclusive scan of the row counts, and launch B.  Returns the DataFrame of
    ``dwell_intervals`` and an int64 column ``population``: ``sample["pop"][posterior_sample, aoi]``.  With
    ``device_table`` the pair ``dwell_intervals`` returns then (the device table keeps its DWELL_COLS columns)."""
    given = num_samples if sample is None else sample["counts"].shape[0]
    filt, thetas, resp, U, B, G, S, N, F = _mixture_dwell_inputs("mixture_dwell_intervals", filt, thetas, resp, unbound,
                                                                 bound, given)
    launch = _population_dwell_launch(filt, thetas, resp, U, B, G, S, N, F, seed)
    if sample is None:
        sample = _walk_count(launch, S, N, F, filt.device, G)
    pop = sample.get("pop")
    if not isinstance(pop, torch.Tensor) or pop.shape != (S, N) or pop.dtype != torch.uint8 or pop.device != filt.device:
        raise ValueError(f"mixture_dwell_intervals: sample['pop'] must be uint8 ({S}, {N}) on the device of filt")
    table = _walk_emit("mixture_dwell_intervals", launch, sample, S, N, filt.device, device_table)
    frame = table[0] if device_table else table
    host = pop.cpu().numpy().astype("int64")
    frame["population"] = host[frame["posterior_sample"].to_numpy(), frame["aoi"].to_numpy()]
    return table


def population_first_binding(tau, pop, populations, Tmax):
    """The first-binding frames ``tau`` (S, N) of ``mixture_dwell_sample`` split by the drawn populations ``pop`` (S, N), per
    sample and population, float64 on the device of ``tau``: ``"share"`` (S, G), the share of AOIs drawn into g;
    ``"never_bound"`` (S, G), the share of those with tau = Tmax; ``"first_binding"`` (S, G), the mean tau of those that
    bound; ``"fraction_bound"`` (S, G, Tmax), ``fraction_bound`` over the AOIs of g.  NaN where a sample has no AOI in g (or
    none that bound)."""
    G = _mixture_pops("population_first_binding", populations)
    t = tau.to(torch.float64)
    S, N = t.shape
    member = (pop.to(torch.int64)[:, None, :] == torch.arange(G, device=pop.device)[None, :, None]).to(torch.float64)
    n_g = member.sum(2)  # (S, G)
    never = member * (t == Tmax).to(torch.float64)[:, None, :]
    bound = member - never
    nan = torch.full_like(n_g, float("nan"))
    first = torch.where(bound.sum(2) > 0, (bound * t[:, None, :]).sum(2) / bound.sum(2).clamp(min=1), nan)
    counts = torch.zeros(S, G, Tmax + 1, dtype=torch.float64, device=t.device)
    idx = tau.to(torch.int64).clamp(0, Tmax)[:, None, :].expand(S, G, N)
    counts.scatter_add_(2, idx, member)
    below = torch.cumsum(counts, 2) - counts
    fb = torch.where(n_g[..., None] > 0, below[..., :Tmax] / n_g.clamp(min=1)[..., None], nan[..., None])
    return {"share": n_g / N, "never_bound": torch.where(n_g > 0, never.sum(2) / n_g.clamp(min=1), nan),
            "first_binding": first, "fraction_bound": fb}


def mixture_estimate(trans, pop, populations, bootstrap=False, seed=0):
    """``hmm_estimate`` per population: from ``trans`` (S, N, M * M) and ``pop`` (S, N) of ``mixture_sample``, pooled over
    the AOIs a raster put into population g, or with ``bootstrap=True`` over the AOIs ``hmm_estimate`` draws for the same
    ``seed``.  Returns ``"A"`` (S, G, M, M) float64 (NaN rows for a state no member visited), ``"totals"`` (S, G, M, M) and
    ``"members"`` (S, G) int64, on the device."""
    import math

    if not isinstance(trans, torch.Tensor) or trans.device.type != "cuda":
        raise HipExtensionError("mixture_estimate runs on the HIP device only (no CPU fallback): pass a cuda tensor")
    G = _mixture_pops("mixture_estimate", populations)
    M = math.isqrt(trans.shape[2]) if trans.ndim == 3 else 0
    if (trans.ndim != 3 or M * M != trans.shape[2] or not 2 <= M <= _lib_hmm.HMM_MAX_STATES or trans.dtype != torch.int32
            or 0 in trans.shape or not isinstance(pop, torch.Tensor) or pop.device != trans.device
            or pop.dtype != torch.uint8 or pop.shape != trans.shape[:2]):
        raise ValueError(f"mixture_estimate: trans must be int32 (S, N, M * M) with S, N >= 1 and M in 2 .. "
                         f"{_lib_hmm.HMM_MAX_STATES}, and pop uint8 (S, N) on its device")
    trans, pop = trans.contiguous(), pop.contiguous()
    S, N = trans.shape[:2]
    totals = torch.empty(S, G, M, M, dtype=torch.int64, device=trans.device)
    members = torch.empty(S, G, dtype=torch.int64, device=trans.device)
    est = torch.empty(S, G, M, M, dtype=torch.float64, device=trans.device)
    a = _lib_mixture.MixtureEstimateArgs(trans=_lib.ptr(trans), pop=_lib.ptr(pop), totals=_lib.ptr(totals),
                                         members=_lib.ptr(members), estimand=_lib.ptr(est), N=N, S=S, G=G, U=1, B=M - 1,
                                         resample=1 if bootstrap else 0, seed=int(seed) & (2**64 - 1))
    _lib.check(_lib_mixture.lib().tq_mixture_estimate(C.byref(a), _stream(trans.device)), "tq_mixture_estimate")
    return {"A": est, "totals": totals, "members": members}


def mixture_viterbi(p, thetas, resp, prior, unbound=1, bound=1):
    """``hmm_viterbi`` under every population's chain; every AOI takes the path of its most probable population (the first
    of equal responsibilities).  Returns ``{"path"}`` (N, F) uint8 in hidden states and ``{"population_map"}`` (N,)."""
    if not isinstance(p, torch.Tensor) or p.device.type != "cuda":
        raise HipExtensionError("mixture_viterbi runs on the HIP device only (no CPU fallback): pass a cuda tensor")
    U, B, M = _hmm_states("mixture_viterbi", unbound, bound)
    if (not isinstance(thetas, torch.Tensor) or thetas.ndim != 2 or not 1 <= thetas.shape[0] <= _lib_mixture.MIXTURE_MAX_POP
            or not isinstance(resp, torch.Tensor) or resp.shape != (thetas.shape[0], p.shape[0])):
        raise ValueError("mixture_viterbi: thetas must be (G, M * M + M) and resp (G, N)")
    paths = torch.stack([hmm_viterbi(p, thetas[g], prior, U, B) for g in range(thetas.shape[0])])  # (G, N, F)
    pop = resp.argmax(0)
    return {"path": paths[pop, torch.arange(p.shape[0], device=p.device)], "population_map": pop}


# ---- the continuous-time chain on the frame timestamps (`smooth --timed`) ---------------------------
def timed_gaps(times):
    """The gap classes of the F time stamps ``times``: ``(d, cls, scale)`` with ``scale`` the median gap, ``d`` (D,) float64
    the distinct gaps over ``scale`` as ``torch.unique`` returns them, and ``cls`` (F - 1,) int32 the class of every gap,
    all on the host.  At equal spacing D = 1.  One frame has no gap: d = [1], no class, scale 1.  Raises ``ValueError``
    unless the stamps are finite and strictly increasing."""
    t = torch.as_tensor(times).detach().cpu().to(torch.float64).reshape(-1)
    if t.numel() < 1 or not bool(torch.isfinite(t).all()):
        raise ValueError("timed_gaps: times must be at least one finite time stamp")
    gaps = t[1:] - t[:-1]
    if not bool((gaps > 0).all()) or not bool(torch.isfinite(gaps).all()):
        raise ValueError("timed_gaps: the time stamps must be strictly increasing")
    if gaps.numel() == 0:
        return torch.ones(1, dtype=torch.float64), torch.zeros(0, dtype=torch.int32), 1.0
    scale = gaps.median().item()
    d, cls = torch.unique(gaps, return_inverse=True)
    return d / scale, cls.to(torch.int32), scale


def _timed_allow(who, allow, M):
    return _lib_multistart.allow_bits(hmm_allow(allow, M, who).tolist())


def _timed_classes(who, d, cls, F, device):
    """``d`` and ``cls`` of ``timed_gaps`` as (device d, host d, device cls, host cls, D), checked against F frames."""
    d_host = torch.as_tensor(d).detach().cpu().to(torch.float64).contiguous().reshape(-1)
    if d_host.numel() < 1 or not bool(torch.isfinite(d_host).all()) or not bool((d_host > 0).all()):
        raise ValueError(f"{who}: d must be at least one finite positive gap")
    if cls is None:
        return d_host.to(device), d_host, None, None, d_host.numel()
    cls_host = torch.as_tensor(cls).detach().cpu().to(torch.int32).contiguous().reshape(-1)
    if cls_host.numel() != F - 1 or (F > 1 and not (0 <= int(cls_host.min()) and int(cls_host.max()) < d_host.numel())):
        raise ValueError(f"{who}: cls must be {F - 1} class indices in [0, {d_host.numel()})")
    return d_host.to(device), d_host, cls_host.to(device), cls_host, d_host.numel()


def _timed_table(theta, d_dev, d_host, D, U, B, bits, P, K):
    a = _lib_timed.TimedTableArgs(theta=_lib.ptr(theta), d=_lib.ptr(d_dev), d_host=d_host.data_ptr(), P=_lib.ptr(P),
                                  K=_lib.ptr(K), D=D, U=U, B=B, allow=bits)
    _lib.check(_lib_timed.lib().tq_timed_table(C.byref(a), _stream(theta.device)), "tq_timed_table")


def timed_tables(theta, d, unbound=1, bound=1, allow=None):
    """One launch of ``tq_timed_table``: for the chain ``theta`` = (Q row-major, rho) (M * M + M float64 on the device, Q per
    unit of ``d``) and the D gaps ``d``, ``{"P"}`` (D, M, M) = exp(Q d) and ``{"K"}`` (D, M, M, M, M) with
    K[k, a, b, i, j] = the integral over the gap of P_ai(s) P_jb(d - s).  ``allow`` (M, M) is the topology of
    ``hmm_allow``: a forbidden rate is read as exactly 0."""
    if not isinstance(theta, torch.Tensor) or theta.device.type != "cuda":
        raise HipExtensionError("timed_tables runs on the HIP device only (no CPU fallback): pass a cuda tensor")
    U, B, M = _hmm_states("timed_tables", unbound, bound)
    theta = _hmm_theta("timed_tables", theta, M, theta.device)
    bits = _timed_allow("timed_tables", allow, M)
    d_dev, d_host, _, _, D = _timed_classes("timed_tables", d, None, 0, theta.device)
    out = {"P": torch.empty(D, M, M, dtype=torch.float64, device=theta.device),
           "K": torch.empty(D, M, M, M, M, dtype=torch.float64, device=theta.device)}
    _timed_table(theta, d_dev, d_host, D, U, B, bits, out["P"], out["K"])
    return out


def _timed_estep(p, N, F, theta, P, K, cls_dev, cls_host, D, prior, U, B, bits, out):
    gamma = out.get("gamma")
    a = _lib_timed.TimedEstepArgs(p=_lib.ptr(p), theta=_lib.ptr(theta), P=_lib.ptr(P), K=_lib.ptr(K),
                                  cls=_lib.ptr(cls_dev) if F > 1 else None, cls_host=cls_host.data_ptr() if F > 1 else None,
                                  filt=_lib.ptr(out["filt"]), gamma=None if gamma is None else _lib.ptr(gamma),
                                  rows=_lib.ptr(out["rows"]), N=N, F=F, D=D, U=U, B=B, allow=bits, prior=prior)
    _lib.check(_lib_timed.lib().tq_timed_estep(C.byref(a), _stream(p.device)), "tq_timed_estep")
    return out


def timed_estep(p, theta, tables, cls, prior, unbound=1, bound=1, allow=None, gamma=True):
    """One launch of ``tq_timed_estep``: ``hmm_estep`` with the transition from frame f to f + 1 read from
    ``tables["P"][cls[f]]`` (``timed_tables`` at the same ``theta``, ``cls`` of ``timed_gaps``).  Returns ``{"filt",
    "gamma"}`` (N, F, M) (no ``gamma`` with ``gamma=False``; the rows are the same bits) and ``"rows"`` (N, M * M + M + 1):
    off the diagonal the expected number of jumps from state i to state j, on it the expected time in state i in the unit
    of the gaps, then gamma_0 and the log evidence."""
    p, N, F, theta, prior, U, B, M = _hmm_inputs("timed_estep", p, theta, prior, unbound, bound)
    bits = _timed_allow("timed_estep", allow, M)
    P, K = tables["P"], tables["K"]
    for name, x, tail in (("P", P, (M, M)), ("K", K, (M, M, M, M))):
        if (not isinstance(x, torch.Tensor) or x.device != p.device or x.dtype != torch.float64 or not x.is_contiguous()
                or x.ndim != len(tail) + 1 or tuple(x.shape[1:]) != tail or x.shape[0] != P.shape[0] or x.shape[0] < 1):
            raise ValueError(f"timed_estep: tables[{name!r}] must be contiguous float64 (D, {', '.join(map(str, tail))}) on "
                             f"the device of p")
    D = P.shape[0]
    cls_host = torch.as_tensor(cls).detach().cpu().to(torch.int32).contiguous().reshape(-1)
    if cls_host.numel() != F - 1 or (F > 1 and not (0 <= int(cls_host.min()) and int(cls_host.max()) < D)):
        raise ValueError(f"timed_estep: cls must be {F - 1} class indices in [0, {D})")
    out = _hmm_buffers(N, F, M, p.device)
    if not gamma:
        del out["gamma"]
    return _timed_estep(p, N, F, theta, P, K, cls_host.to(p.device), cls_host, D, prior, U, B, bits, out)


def timed_mstep(rows, theta, trace, it=0, unbound=1, bound=1, allow=None):
    """One launch of ``tq_timed_mstep``: ``theta`` (M * M + M float64, in place) from the summed ``rows`` of
    ``timed_estep`` -- q_ij = sum E N_ij / sum E T_i, floored at 1e-9 where free and exactly 0 where ``allow`` forbids it,
    rho the mean gamma_0 -- and the total log evidence of those rows into ``trace[it]``.  Returns ``theta``."""
    U, B, M = _mstep_inputs("timed_mstep", rows, theta, trace, it, (unbound, bound))
    a = _lib_timed.TimedMstepArgs(rows=_lib.ptr(rows), theta=_lib.ptr(theta), trace=_lib.ptr(trace), N=rows.shape[0],
                                  it=int(it), T=trace.numel(), U=U, B=B, allow=_timed_allow("timed_mstep", allow, M))
    _lib.check(_lib_timed.lib().tq_timed_mstep(C.byref(a), _stream(rows.device)), "tq_timed_mstep")
    return theta


def timed_default_start(unbound, bound):
    """The deterministic default start of ``timed_fit`` as (Q (M, M), rho (M,)) float64: the off-diagonals of
    ``hmm_default_start``'s A as rates per median gap -- its first order -- and the diagonal minus the row's sum."""
    A, rho = hmm_default_start(unbound, bound)
    Q = A.clone()
    Q.fill_diagonal_(0.0)
    Q -= torch.diag(Q.sum(1))
    return Q, rho


def timed_canonical_order(theta, unbound, bound):
    """The permutation (a list: new state k is old state order[k]) that puts the states of each class in ascending exit
    rate -- the analogue of descending A_ii; equal values keep their order.  The stored diagonal is not read."""
    U, B, M = _hmm_states("timed_canonical_order", unbound, bound)
    Q = theta.detach().cpu().reshape(-1)[: M * M].reshape(M, M).clone()
    Q.fill_diagonal_(0.0)
    leave = Q.sum(1).tolist()
    return sorted(range(U), key=lambda i: leave[i]) + sorted(range(U, M), key=lambda i: leave[i])


def timed_fit(p, prior, times, unbound=1, bound=1, allow=None, Q0=None, rho0=None, num_iter=200, tol=1e-9, chunk=50,
              progress_bar=None):
    """EM fit of a continuous-time chain of ``unbound`` + ``bound`` hidden states to the rows of ``p`` (N, F) observed at the
    F time stamps ``times``, from (``Q0``, ``rho0``) -- Q0 in rates per unit of ``times`` -- or from
    ``timed_default_start``.  Every iteration is three launches (tables, E-step, M-step); the chunks, the stopping rule and
    the closing E-step are those of ``hmm_fit``.  ``allow`` (M, M) forbids transitions: their rates are exactly 0.

    After the fit the states of each class are put in ascending exit rate (``timed_canonical_order``), in every output
    alike.  Returns ``theta`` (M * M + M,) with Q in **rates per unit of ``times``**, ``gamma``, ``filt`` (N, F, M), ``rows``
    (N, M * M + M + 1; the expected times in the unit of ``times``), ``trace``, ``iterations``, ``converged``, ``loglik``,
    ``n_params`` (free off-diagonals + M - 1), ``bic``, ``order``, ``allow`` (in the order of the outputs) and ``scale``
    (the median gap, the kernels' unit of time)."""
    import math

    num_iter = int(num_iter)
    U, B, M = _hmm_states("timed_fit", unbound, bound)
    free = hmm_allow(allow, M, "timed_fit")
    d, cls_host, scale = timed_gaps(times)
    Q, rho = timed_default_start(U, B)
    if Q0 is not None:
        Q = torch.as_tensor(Q0, dtype=torch.float64).cpu() * scale
    if rho0 is not None:
        rho = torch.as_tensor(rho0, dtype=torch.float64).cpu()
    off = ~torch.eye(M, dtype=torch.bool)
    if (num_iter < 1 or Q.shape != (M, M) or rho.shape != (M,) or not bool((Q[off] >= 0).all()) or not bool((rho >= 0).all())
            or not bool(torch.isfinite(Q).all()) or not float(rho.sum()) > 0):
        raise ValueError(f"timed_fit: num_iter must be positive, Q0 ({M}, {M}) with finite non-negative off-diagonal rates and "
                         f"rho0 ({M},) non-negative with a positive sum")
    if not isinstance(p, torch.Tensor) or p.device.type != "cuda":
        raise HipExtensionError("timed_fit runs on the HIP device only (no CPU fallback): pass a cuda tensor")
    Q = torch.where(off & free, Q, torch.zeros_like(Q))
    Q = Q - torch.diag(Q.sum(1))
    theta = torch.cat([Q.reshape(-1), rho / rho.sum()]).to(p.device)
    p, N, F, theta, prior, U, B, M = _hmm_inputs("timed_fit", p, theta, prior, U, B)
    if cls_host.numel() != F - 1:
        raise ValueError(f"timed_fit: times must have one stamp per frame, got {cls_host.numel() + 1} for {F} frames")
    bits = _lib_multistart.allow_bits(free.tolist())
    d_dev, d_host, cls_dev, cls_host, D = _timed_classes("timed_fit", d, cls_host, F, p.device)
    P = torch.empty(D, M, M, dtype=torch.float64, device=p.device)
    K = torch.empty(D, M, M, M, M, dtype=torch.float64, device=p.device)
    out = _hmm_buffers(N, F, M, p.device)
    rows_only = {"filt": out["filt"], "rows": out["rows"]}
    trace = torch.full((num_iter,), float("nan"), dtype=torch.float64, device=p.device)

    def step(it):
        _timed_table(theta, d_dev, d_host, D, U, B, bits, P, K)
        _timed_estep(p, N, F, theta, P, K, cls_dev, cls_host, D, prior, U, B, bits, rows_only)
        timed_mstep(out["rows"], theta, trace, it, U, B, free)

    state = _chain_em(step, trace, num_iter, tol, chunk, progress_bar)
    _timed_table(theta, d_dev, d_host, D, U, B, bits, P, K)
    _timed_estep(p, N, F, theta, P, K, cls_dev, cls_host, D, prior, U, B, bits, out)
    order = timed_canonical_order(theta, U, B)
    out = hmm_permute(order, M, theta=theta, **out)
    ix = torch.as_tensor(order)
    # back to the unit of `times`: rates over the median gap, expected times times it
    unit = torch.ones(M * M + M, dtype=torch.float64, device=p.device)
    unit[: M * M] = 1.0 / scale
    out["theta"] = out["theta"] * unit
    rows = out["rows"]
    diag = torch.arange(M, device=p.device) * (M + 1)
    rows[:, diag] = rows[:, diag] * scale
    loglik = rows[:, -1].sum().item()
    n_params = int(free.sum()) - M + (M - 1)
    return {**out, "trace": trace[: state["iterations"]], **state, "loglik": loglik, "n_params": n_params,
            "bic": -2.0 * loglik + n_params * math.log(N * F), "order": order, "allow": free[ix][:, ix], "scale": scale}
