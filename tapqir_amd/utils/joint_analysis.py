"""
Two colour channels as one hidden Markov chain (``tapqir_amd smooth --joint A,B``).

Channels a and b of one cosmos fit are smoothed together: the hidden state is s = z_a + 2 z_b (0 neither bound, 1 only a,
2 only b, 3 both), theta = (A row-major (4, 4), rho (4)) is that of ``hmm_fit`` at four states, and a state emits the
product of the two channels' evidence.  Five structures of A state the scientific hypotheses -- ``independent``,
``a-drives-b``, ``b-drives-a``, ``coupled``, ``full`` -- and are fitted side by side, one replica each, by the EM loop of
``hmm_fit_restarts`` (``multistart_em``) on ``tq_joint_estep`` / ``tq_joint_mstep``; the BIC ranks them.  The backward
sampler and the estimate of A are ``hmm_sample`` / ``hmm_estimate`` at (2, 2) on the joint ``filt``.

``joint_dwell_sample`` / ``joint_dwell_intervals`` walk the rasters of that sampler, as they are drawn, into the runs of one
channel with the other channel's state at their ends (``tq_pair_dwell``), and ``joint_arrival_order``
turns the first-binding frames into the order of arrival (host-side torch on S x N numbers; it runs anywhere).

The states are identified by their emissions, so nothing is reordered after a fit.  Everything runs on the HIP device;
there is no CPU fallback.
"""

import ctypes as C
import math

import torch

from tapqir_amd import _lib, _lib_joint, _lib_smooth
from tapqir_amd._lib_multistart import MULTISTART_MAX
from tapqir_amd.exceptions import HipExtensionError
from tapqir_amd.utils.mle_analysis import (MULTISTART_SCRATCH_BYTES, _hmm_sample_inputs, _multistart_active,
                                           _multistart_inputs, _sampler_inputs, _stream, _walk_count, _walk_emit,
                                           multistart_em)

STRUCTURE_NAMES = tuple(name for name, _ in _lib_joint.STRUCTURES)
M, THETA, COLS = _lib_joint.JOINT_STATES, _lib_joint.JOINT_THETA, _lib_joint.JOINT_COLS
RATE_NAMES = ("kon_a|b0", "kon_a|b1", "koff_a|b0", "koff_a|b1", "kon_b|a0", "kon_b|a1", "koff_b|a0", "koff_b|a1")
RATIO_NAMES = ("kon_a ratio", "koff_a ratio", "kon_b ratio", "koff_b ratio")
PARTNER_COLUMNS = ("partner_start", "partner_before", "partner_stop", "partner_after")  # bits 0 .. 3 of the partner code
ORDER_NAMES = ("binds", "together", "later", "never", "mean_delay", "k_after", "k_base", "ratio")


def joint_structure_id(structure):
    """The id 0 .. 4 of a structure given by id or by name."""
    if isinstance(structure, str):
        if structure not in STRUCTURE_NAMES:
            raise ValueError(f"unknown structure {structure!r}: one of {', '.join(STRUCTURE_NAMES)}")
        return STRUCTURE_NAMES.index(structure)
    s = int(structure)
    if not 0 <= s < len(STRUCTURE_NAMES):
        raise ValueError(f"structure ids are 0 .. {len(STRUCTURE_NAMES) - 1}, got {structure}")
    return s


def joint_n_params(structure):
    """Free parameters of a structure: those of A and the 3 of rho."""
    return _lib_joint.STRUCTURES[joint_structure_id(structure)][1] + M - 1


def _two_state(theta):
    kon, koff, pi0 = (float(v) for v in torch.as_tensor(theta, dtype=torch.float64).detach().cpu().reshape(-1))
    return (torch.tensor([[1.0 - kon, kon], [koff, 1.0 - koff]], dtype=torch.float64),
            torch.tensor([1.0 - pi0, pi0], dtype=torch.float64))


def joint_start_from(theta_a, theta_b):
    """The chain of two independent channels as a joint theta (20,) float64 on the host: ``theta_a`` and ``theta_b`` are the
    two-state (kon, koff, pi0) of ``smooth_fit``; A = kron(A_b, A_a) and rho = kron(rho_b, rho_a), b being the slow index of
    s = z_a + 2 z_b."""
    (Aa, ra), (Ab, rb) = _two_state(theta_a), _two_state(theta_b)
    return torch.cat([torch.kron(Ab, Aa).reshape(-1), torch.kron(rb, ra)])


def joint_default_start():
    """The deterministic default start of ``joint_fit``: both channels switch at 0.1 per frame, rho uniform."""
    A0 = torch.tensor([[0.9, 0.1], [0.1, 0.9]], dtype=torch.float64)
    return torch.cat([torch.kron(A0, A0).reshape(-1), torch.full((M,), 1.0 / M, dtype=torch.float64)])


def joint_rates(A):
    """The eight conditional rates and their four ratios of a (..., 4, 4) tensor of joint transition matrices, as a dict
    of (...) tensors in the order ``RATE_NAMES + RATIO_NAMES``: ``kon_a|b0`` is the probability per frame that a binds while
    b is unbound, and a ratio is the rate with the partner bound over the rate with it unbound.  NaN entries propagate."""
    A = torch.as_tensor(A)
    if A.ndim < 2 or A.shape[-2:] != (M, M):
        raise ValueError(f"joint_rates: A must be (..., {M}, {M}), got {tuple(A.shape)}")
    a = lambda i, j: A[..., i, j]  # noqa: E731
    out = {"kon_a|b0": a(0, 1) + a(0, 3), "kon_a|b1": a(2, 3) + a(2, 1), "koff_a|b0": a(1, 0) + a(1, 2),
           "koff_a|b1": a(3, 2) + a(3, 0), "kon_b|a0": a(0, 2) + a(0, 3), "kon_b|a1": a(1, 3) + a(1, 2),
           "koff_b|a0": a(2, 0) + a(2, 1), "koff_b|a1": a(3, 1) + a(3, 0)}
    for name, hi, lo in (("kon_a ratio", "kon_a|b1", "kon_a|b0"), ("koff_a ratio", "koff_a|b1", "koff_a|b0"),
                         ("kon_b ratio", "kon_b|a1", "kon_b|a0"), ("koff_b ratio", "koff_b|a1", "koff_b|a0")):
        out[name] = out[hi] / out[lo]
    return out


def _joint_inputs(who, p_a, p_b, prior_a, prior_b):
    """Both channels through ``_sampler_inputs`` -- (N, F) float32 on one device -- N, F and the two priors in (0, 1)."""
    p_a, N, F, _ = _sampler_inputs(who, p_a, 1, 0)
    p_b, Nb, Fb, _ = _sampler_inputs(who, p_b, 1, 0)
    if (Nb, Fb) != (N, F) or p_b.device != p_a.device:
        raise ValueError(f"{who}: p_a and p_b must have one shape and one device, got {(N, F)} and {(Nb, Fb)}")
    if F > _lib_smooth.SMOOTH_MAX_F:
        raise ValueError(f"{who}: at most {_lib_smooth.SMOOTH_MAX_F} frames, got {F}")
    prior_a, prior_b = float(prior_a), float(prior_b)
    if not (0.0 < prior_a < 1.0 and 0.0 < prior_b < 1.0):
        raise ValueError(f"{who}: the priors must lie in (0, 1), got {prior_a} and {prior_b}")
    return p_a, p_b, N, F, prior_a, prior_b


def joint_estep(p_a, p_b, thetas, prior_a, prior_b, active=None, gamma=False, rows=None, filt=None):
    """One launch of ``tq_joint_estep``: forward-backward of the R chains ``thetas`` (R, 20) on the shared rows of ``p_a``
    and ``p_b`` (N, F), each channel's p(z = 1) with its own ``prior`` divided out.

    Returns ``{"rows" (R, N, 21), "filt" (R, N, F, 4)}`` float64 and, with ``gamma=True`` (or a tensor to write into),
    ``"gamma"`` (R, N, F, 4); without it no gamma is stored and ``rows`` has the same bits.  ``active`` (R,) int32 on the
    device leaves everything of a replica with a 0 as it is; ``rows`` and ``filt`` are reused when given."""
    if not isinstance(p_a, torch.Tensor) or p_a.device.type != "cuda":
        raise HipExtensionError("joint_estep runs on the HIP device only (no CPU fallback): pass a cuda tensor")
    thetas = _multistart_inputs("joint_estep", thetas, (THETA,), "thetas")
    R = thetas.shape[0]
    p_a, p_b, N, F, prior_a, prior_b = _joint_inputs("joint_estep", p_a, p_b, prior_a, prior_b)
    dev = p_a.device
    if thetas.device != dev:
        raise ValueError("joint_estep: thetas must be on the device of p_a")
    active = _multistart_active("joint_estep", active, R, dev)
    out = {"rows": torch.empty(R, N, COLS, dtype=torch.float64, device=dev) if rows is None else rows,
           "filt": torch.empty(R, N, F, M, dtype=torch.float64, device=dev) if filt is None else filt}
    if gamma is not False and gamma is not None:
        out["gamma"] = torch.empty(R, N, F, M, dtype=torch.float64, device=dev) if gamma is True else gamma
    for name, x in out.items():
        shape = (R, N, COLS) if name == "rows" else (R, N, F, M)
        if (not isinstance(x, torch.Tensor) or x.shape != shape or x.dtype != torch.float64 or x.device != dev
                or not x.is_contiguous()):
            raise ValueError(f"joint_estep: {name} must be contiguous float64 {shape} on the device of p_a")
    a = _lib_joint.JointEstepArgs(p_a=_lib.ptr(p_a), p_b=_lib.ptr(p_b), theta=_lib.ptr(thetas), filt=_lib.ptr(out["filt"]),
                                  gamma=_lib.ptr(out.get("gamma")), rows=_lib.ptr(out["rows"]), active=_lib.ptr(active),
                                  N=N, F=F, R=R, prior_a=prior_a, prior_b=prior_b)
    _lib.check(_lib_joint.lib().tq_joint_estep(C.byref(a), _stream(dev)), "tq_joint_estep")
    return out


def joint_mstep(rows, thetas, trace, it, structures, active=None):
    """One launch of ``tq_joint_mstep``: ``thetas`` (R, 20, in place) from the summed ``rows`` (R, N, 21) of
    ``joint_estep``, replica r under ``structures[r]`` (ids or names), and every replica's total log-evidence into
    ``trace[r, it]``, trace (R, T).  A replica with ``active[r] == 0`` keeps its theta and its trace.  Returns ``thetas``."""
    if not isinstance(rows, torch.Tensor) or rows.device.type != "cuda":
        raise HipExtensionError("joint_mstep runs on the HIP device only (no CPU fallback): pass a cuda tensor")
    if rows.ndim != 3 or rows.shape[1] < 1:
        raise ValueError(f"joint_mstep: rows must be (R, N, {COLS}) with N >= 1")
    rows = _multistart_inputs("joint_mstep", rows, (rows.shape[1], COLS), "rows")
    R, N = rows.shape[:2]
    it = int(it)
    for name, x, ok in (("thetas", thetas, lambda x: x.shape == (R, THETA)),
                        ("trace", trace, lambda x: x.ndim == 2 and x.shape[0] == R and 0 <= it < x.shape[1])):
        if (not isinstance(x, torch.Tensor) or x.device != rows.device or x.dtype != torch.float64 or not x.is_contiguous()
                or not ok(x)):
            raise ValueError(f"joint_mstep: {name} must be contiguous float64 on the device of rows, thetas ({R}, {THETA}) "
                             f"and trace ({R}, T) with 0 <= it < T")
    ids = [joint_structure_id(s) for s in structures]
    if len(ids) != R:
        raise ValueError(f"joint_mstep: {R} replicas need {R} structures, got {len(ids)}")
    active = _multistart_active("joint_mstep", active, R, rows.device)
    a = _lib_joint.JointMstepArgs(rows=_lib.ptr(rows), theta=_lib.ptr(thetas), trace=_lib.ptr(trace), active=_lib.ptr(active),
                                  N=N, it=it, T=trace.shape[1], R=R, structure=_lib_joint.structure_array(ids))
    _lib.check(_lib_joint.lib().tq_joint_mstep(C.byref(a), _stream(rows.device)), "tq_joint_mstep")
    return thetas


def _joint_theta(who, theta, device):
    if (not isinstance(theta, torch.Tensor) or theta.device != device or theta.dtype != torch.float64
            or theta.numel() != THETA):
        raise ValueError(f"{who}: theta must be {THETA} float64 values (A row-major, rho) on the device of the data")
    return theta.contiguous().reshape(-1)


def joint_viterbi(p_a, p_b, theta, prior_a, prior_b):
    """MAP path in joint states of every row under the chain ``theta`` (20,) and the evidence of ``joint_estep``: (N, F)
    uint8 on the device, ``path & 1`` is z_a and ``path >> 1`` is z_b.  A tie takes the lowest state."""
    if not isinstance(p_a, torch.Tensor) or p_a.device.type != "cuda":
        raise HipExtensionError("joint_viterbi runs on the HIP device only (no CPU fallback): pass a cuda tensor")
    p_a, p_b, N, F, prior_a, prior_b = _joint_inputs("joint_viterbi", p_a, p_b, prior_a, prior_b)
    theta = _joint_theta("joint_viterbi", theta, p_a.device)
    back = torch.empty(((F + 3) // 4) * N, dtype=torch.int32, device=p_a.device)
    path = torch.empty(N, F, dtype=torch.uint8, device=p_a.device)
    a = _lib_joint.JointViterbiArgs(p_a=_lib.ptr(p_a), p_b=_lib.ptr(p_b), theta=_lib.ptr(theta), back=_lib.ptr(back),
                                    path=_lib.ptr(path), N=N, F=F, prior_a=prior_a, prior_b=prior_b)
    _lib.check(_lib_joint.lib().tq_joint_viterbi(C.byref(a), _stream(p_a.device)), "tq_joint_viterbi")
    return path


def joint_select(logliks, structures, N, F):
    """n_params, BIC = -2 loglik + n_params log(N F) of every fitted structure, and the id of the lowest BIC; a tie goes to
    the lowest id."""
    n_params = [joint_n_params(s) for s in structures]
    bics = [-2.0 * float(ll) + k * math.log(N * F) for ll, k in zip(logliks, n_params)]
    finite = [b if math.isfinite(b) else math.inf for b in bics]
    best = min((s for s, b in zip(structures, finite) if b == min(finite)), default=structures[0])
    return n_params, bics, best


def joint_fit(p_a, p_b, prior_a, prior_b, structures=STRUCTURE_NAMES, start=None, num_iter=200, tol=1e-9, chunk=50,
              choose=None, progress_bar=None):
    """EM fit of the joint chain to the rows of ``p_a`` and ``p_b`` (N, F) under every structure of ``structures`` (ids or
    names, no repeats), one replica each, all from ``start`` (20,; default ``joint_default_start()``).

    Every EM iteration is one batched E-step and one batched M-step for all structures; the chunks, the stopping rule
    and the freezing of a converged replica are ``multistart_em``'s.  A closing batched E-step with gamma gives every
    structure's log-evidence at its final theta.  ``filt`` of all replicas takes R N F 32 bytes and the closing gamma as
    much again; more than ``MULTISTART_SCRATCH_BYTES`` in total is refused.

    Returns ``fits``: per structure, in the order given, ``{"structure", "name", "theta" (20,), "loglik", "n_params",
    "bic", "iterations", "converged", "trace"}``; ``best``: the id of the lowest BIC (a tie goes to the lowest id);
    ``chosen``: ``choose`` if given (it must be among ``structures``), else ``best``; and for the chosen structure ``theta``
    (20,), ``filt``, ``gamma`` (N, F, 4) and ``rows`` (N, 21) on the device.  No state is reordered."""
    num_iter = int(num_iter)
    ids = [joint_structure_id(s) for s in structures]
    if num_iter < 1 or not 1 <= len(ids) <= MULTISTART_MAX or len(set(ids)) != len(ids):
        raise ValueError("joint_fit: num_iter must be positive and structures a non-empty list without repeats")
    chosen = None if choose is None else joint_structure_id(choose)
    if chosen is not None and chosen not in ids:
        raise ValueError(f"joint_fit: the structure to choose, {STRUCTURE_NAMES[chosen]}, is not among those fitted")
    start = joint_default_start() if start is None else torch.as_tensor(start, dtype=torch.float64).detach().cpu().reshape(-1)
    if start.numel() != THETA or not bool((start >= 0).all()):
        raise ValueError(f"joint_fit: start must be {THETA} non-negative values (A row-major, rho)")
    A, rho = start[: M * M].reshape(M, M), start[M * M:]
    if not bool((A.sum(1) > 0).all()) or not float(rho.sum()) > 0:
        raise ValueError("joint_fit: every row of A and rho of start must have a positive sum")
    if not isinstance(p_a, torch.Tensor) or p_a.device.type != "cuda":
        raise HipExtensionError("joint_fit runs on the HIP device only (no CPU fallback): pass a cuda tensor")
    p_a, p_b, N, F, prior_a, prior_b = _joint_inputs("joint_fit", p_a, p_b, prior_a, prior_b)
    R, dev = len(ids), p_a.device
    if 2 * R * N * F * M * 8 > MULTISTART_SCRATCH_BYTES:
        raise ValueError(f"joint_fit: filt and gamma of R = {R} structures, N = {N} rows and F = {F} frames take "
                         f"{2 * R * N * F * M * 8} bytes, more than {MULTISTART_SCRATCH_BYTES}: fit fewer structures at once")
    theta0 = torch.cat([(A / A.sum(1, keepdim=True)).reshape(-1), rho / rho.sum()])
    thetas = theta0.repeat(R, 1).contiguous().to(dev)
    rows = torch.empty(R, N, COLS, dtype=torch.float64, device=dev)
    filt = torch.empty(R, N, F, M, dtype=torch.float64, device=dev)
    trace = torch.full((R, num_iter), float("nan"), dtype=torch.float64, device=dev)
    active = torch.ones(R, dtype=torch.int32, device=dev)
    iterations, converged = multistart_em(
        lambda: joint_estep(p_a, p_b, thetas, prior_a, prior_b, active, None, rows, filt),
        lambda it: joint_mstep(rows, thetas, trace, it, ids, active), trace, active, num_iter, tol, chunk, progress_bar)
    out = joint_estep(p_a, p_b, thetas, prior_a, prior_b, None, True, rows, filt)
    logliks = rows[:, :, -1].sum(1).cpu()
    n_params, bics, best = joint_select(logliks.tolist(), ids, N, F)
    chosen = best if chosen is None else chosen
    k = ids.index(chosen)
    host_thetas, host_trace = thetas.cpu(), trace.cpu()
    fits = [{"structure": s, "name": STRUCTURE_NAMES[s], "theta": host_thetas[r], "loglik": logliks[r].item(),
             "n_params": n_params[r], "bic": bics[r], "iterations": iterations[r], "converged": converged[r],
             "trace": host_trace[r, : iterations[r]]} for r, s in enumerate(ids)]
    return {"fits": fits, "best": best, "chosen": chosen, "theta": thetas[k].clone(), "filt": out["filt"][k].clone(),
            "gamma": out["gamma"][k].clone(), "rows": rows[k].clone()}


# ---- dwell times and first binding of one channel of the joint chain -----------------------------
def _pair_dwell_launch(filt, theta, which, S, N, F, seed):
    def launch(**fields):
        a = _lib_joint.PairDwellArgs(filt=_lib.ptr(filt), theta=_lib.ptr(theta), N=N, F=F, S=S, which=which,
                                     seed=int(seed) & (2**64 - 1), **fields)
        _lib.check(_lib_joint.lib().tq_pair_dwell(C.byref(a), _stream(filt.device)), "tq_pair_dwell")

    return launch


def _pair_dwell_inputs(who, filt, theta, which, num_samples):
    filt, theta, _, _, _, S, N, F = _hmm_sample_inputs(who, filt, theta, 2, 2, num_samples)
    if which not in (0, 1):
        raise ValueError(f"{who}: which must be 0 (the runs of channel a) or 1 (those of channel b), got {which!r}")
    return filt, theta, int(which), S, N, F


def joint_dwell_sample(filt, theta, which, num_samples, seed=0):
    """``hmm_dwell_sample`` for one channel of the joint chain: launch A of the interval sampler on the rasters
    ``hmm_sample(filt, theta, 2, 2, num_samples, seed, raster=True)["raster"]``, walked as they are drawn at the level of
    ``z = (state >> which) & 1`` -- channel a for ``which`` = 0, channel b for 1 -- with the partner
    ``q = (state >> (1 - which)) & 1`` beside it.  ``filt`` (N, F, 4) is that of ``joint_estep`` at one theta (20,).

    Returns ``"hist_bound"`` / ``"hist_unbound"`` (S, 2, F) int32 -- the interior runs by the partner's state q at the
    run's first frame and by dwell time; ``hist[:, q]`` goes to ``dwell_csr_from_hist`` / ``dwell_fit`` --, ``"counts"``
    (S, N) int32, ``"tau"`` (S, N) float32, the first frame with z = 1 or F, and ``"tau_after"`` (S, N) float32, the
    partner's first bound frame from ``tau`` on, or F (also where ``tau`` is F).  Both values of ``which`` at one seed
    describe the same rasters."""
    filt, theta, which, S, N, F = _pair_dwell_inputs("joint_dwell_sample", filt, theta, which, num_samples)
    return _walk_count(_pair_dwell_launch(filt, theta, which, S, N, F, seed), S, N, F, filt.device, partner=True)


def joint_dwell_intervals(filt, theta, which, num_samples, seed=0, sample=None, device_table=False):
    """``hmm_dwell_intervals`` for one channel of the joint chain: launch A (or its result ``sample`` from
    ``joint_dwell_sample`` with the same arguments), the exclusive scan of the row counts, and launch B.  Returns the
    DataFrame of ``dwell_intervals`` and four int64 columns, the partner's state at the run's first frame
    (``partner_start``), at the frame before it (``partner_before``), at its last frame (``partner_stop``) and at the frame
    after it (``partner_after``); -1 where that frame does not exist.  With ``device_table`` the pair ``dwell_intervals``
    returns then, the DataFrame with the four columns."""
    given = num_samples if sample is None else sample["counts"].shape[0]
    filt, theta, which, S, N, F = _pair_dwell_inputs("joint_dwell_intervals", filt, theta, which, given)
    launch = _pair_dwell_launch(filt, theta, which, S, N, F, seed)
    if sample is None:
        sample = _walk_count(launch, S, N, F, filt.device, partner=True)
    out, codes = _walk_emit("joint_dwell_intervals", launch, sample, S, N, filt.device, device_table, partner=True)
    table = out[0] if device_table else out
    code = codes.cpu().numpy().astype("int64")
    exists = (None, table["start_frame"].to_numpy() > 0, None, table["stop_frame"].to_numpy() < F - 1)
    for bit, name in enumerate(PARTNER_COLUMNS):
        value = (code >> bit) & 1
        table[name] = value if exists[bit] is None else value * exists[bit] - (~exists[bit])
    return out


def joint_arrival_order(tau_lead, tau_after, tau_partner, F):
    """The order of arrival of two channels from first-binding frames, per posterior sample: ``tau_lead`` and ``tau_after``
    (S, N) of ``joint_dwell_sample`` for the lead channel, ``tau_partner`` (S, N) the partner's own first-binding frame
    (``tau`` of the other ``which``), ``F`` the number of frames.  Plain torch on the device of ``tau_lead``; it runs on the
    host as well.  With d = tau_after - tau_lead, defined where the lead binds, returns a dict of (S,) float64 tensors:

    * ``binds``: the share of rows in which the lead binds (tau_lead < F);
    * ``together`` / ``later`` / ``never``: of those, the shares with d = 0, with d > 0 and the partner following
      (tau_after < F), and with the partner never following (tau_after = F); they sum to 1;
    * ``mean_delay``: the mean d over the rows of ``later``;
    * ``k_after`` = |E| / (sum_E d + sum_C (F - 1 - tau_lead)), E the rows of ``later`` and C those of ``never``;
    * ``k_base`` = |E0| / (sum_E0 tau_partner + |C0| (F - 1)), E0 = {0 < tau_partner < F}, C0 = {tau_partner = F};
    * ``ratio`` = k_after / k_base.

    The two k are the maximum-likelihood per-frame probabilities of a geometric waiting time with right censoring: events
    over frames at risk, for the partner's arrival after the lead has arrived and for its arrival from the start of the
    record.  A zero denominator gives NaN."""
    lead, after, own = (torch.as_tensor(x).to(torch.float64) for x in (tau_lead, tau_after, tau_partner))
    if lead.ndim != 2 or after.shape != lead.shape or own.shape != lead.shape:
        raise ValueError(f"joint_arrival_order: three (S, N) tensors of one shape, got {tuple(lead.shape)}, "
                         f"{tuple(after.shape)} and {tuple(own.shape)}")
    F = int(F)
    bound = lead < F
    d = after - lead
    events = bound & (d > 0) & (after < F)
    censored = bound & (after == F)
    n_bound = bound.sum(1).to(torch.float64)

    def quotient(num, den):
        return torch.where(den > 0, num / den.clamp(min=1e-300), torch.full_like(den, float("nan")))

    def total(x, where):
        return (x * where).sum(1)

    n_events = events.sum(1).to(torch.float64)
    k_after = quotient(n_events, total(d, events) + total(F - 1 - lead, censored))
    base_events, base_censored = (own > 0) & (own < F), own == F
    k_base = quotient(base_events.sum(1).to(torch.float64), total(own, base_events) + base_censored.sum(1).to(torch.float64) * (F - 1))
    return {"binds": n_bound / lead.shape[1], "together": quotient((bound & (d == 0)).sum(1).to(torch.float64), n_bound),
            "later": quotient(n_events, n_bound), "never": quotient(censored.sum(1).to(torch.float64), n_bound),
            "mean_delay": quotient(total(d, events), n_events), "k_after": k_after, "k_base": k_base,
            "ratio": quotient(k_after, k_base)}
