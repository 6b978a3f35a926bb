"""
Time to first binding of binary or probabilistic spot-presence rasters (tapqir/utils/imscroll.py:143-196), and the
interval table of binary rasters with its padded dwell-time arrays (imscroll.py:14-141).

For binary labels ``z`` (..., F) the result is the index of the first frame with ``z = 1``, or ``F`` if there is none:

    ttfb = sum_{f=1}^{F-1} f z_f prod_{f' < f} (1 - z_f') + F prod_{f'} (1 - z_f')

For probabilities ``q(z_f = 1)`` the same expression is the expectation of that index under independent frames.

Two-state rates of binary rasters and their resampling intervals (imscroll.py:199-317): ``association_rate`` and
``dissociation_rate`` are the per-frame transition frequencies kon = #(0 -> 1) / #(z_f = 0) and koff = #(1 -> 0) /
#(z_f = 1) over the frame pairs of the last axis, pooled over the axis before it; ``bootstrap``, ``posterior_estimate``
and ``sample_and_bootstrap`` are host loops over an arbitrary estimator that return the percentile interval of its
values.  For the two rate estimators on posterior rasters the device computes the same estimands without the rasters
(``tapqir_amd.utils.mle_analysis.rates_sample`` / ``rates_estimate``, the ``rates`` command).
"""

from functools import singledispatch

import numpy as np
import pandas as pd
import torch


@singledispatch
def time_to_first_binding(labels):
    r"""Time elapsed prior to the first binding (Friedman & Gelles 2015), over the last axis of ``labels``."""
    raise NotImplementedError


@time_to_first_binding.register(np.ndarray)
def _(labels):
    labels = labels.astype("float")
    F = labels.shape[-1]
    frames = np.arange(1, F + 1)
    q1 = np.ones_like(labels)
    q1[..., :-1] = labels[..., 1:]
    cumq0 = np.cumprod(1 - labels, axis=-1)
    return (frames * q1 * cumq0).sum(-1)


@time_to_first_binding.register(torch.Tensor)
def _(labels):
    labels = labels.float()
    F = labels.shape[-1]
    frames = torch.arange(1, F + 1, device=labels.device)
    q1 = torch.ones_like(labels)
    q1[..., :-1] = labels[..., 1:]
    cumq0 = torch.cumprod(1 - labels, dim=-1)
    return (frames * q1 * cumq0).sum(-1)


# ---- interval bookkeeping (tapqir/utils/imscroll.py:14-141) ------------------------------------------------------------
# Runs of equal labels along the last axis of a (S, N, F) raster, one row per run, in (sample, AOI, frame) order:
# low_or_high is -3 / -2 for the first run of a record (bound / unbound), 3 / 2 for the last one (a run that is both gets
# 3 / 2), and 1 / 0 for interior runs.  The device computes the same table (tapqir_amd.utils.mle_analysis.dwell_intervals).

INTERVAL_COLUMNS = ["posterior_sample", "aoi", "start_frame", "stop_frame", "dwell_time", "low_or_high", "z"]


def _interval_table(z, starts, stops, F):
    s, n, f0 = starts
    f1 = stops[2]
    label = (z[s, n, f0] != 0).astype(np.int64)
    start_type = np.where(f0 == 0, -label - 2, label)
    stop_type = np.where(f1 == F - 1, label + 2, label)
    low_or_high = np.where(np.abs(start_type) > np.abs(stop_type), start_type, stop_type)
    return pd.DataFrame({"posterior_sample": s, "aoi": n, "start_frame": f0, "stop_frame": f1, "dwell_time": f1 + 1 - f0,
                         "low_or_high": low_or_high, "z": z[s, n, f0]})


@singledispatch
def count_intervals(labels):
    r"""Binding and absent intervals of the (S, N, F) label raster ``labels`` (Friedman & Gelles 2015), as a DataFrame
    with the columns ``INTERVAL_COLUMNS``."""
    raise NotImplementedError


@count_intervals.register(np.ndarray)
def _(labels):
    b = labels.astype(bool)
    F = b.shape[-1]
    edge = b[..., 1:] != b[..., :-1]
    opens = np.concatenate([np.ones_like(b[..., :1]), edge], axis=-1)
    closes = np.concatenate([edge, np.ones_like(b[..., :1])], axis=-1)
    return _interval_table(labels, np.nonzero(opens), np.nonzero(closes), F)


@count_intervals.register(torch.Tensor)
def _(labels):
    return count_intervals(labels.detach().cpu().numpy())


def _dwell_times(intervals, code):
    """Zero-padded (n_values, max_count) float32 dwell times of the runs with ``low_or_high == code``: row i holds the
    runs of posterior sample i, for i < n_values = the number of samples that have any (imscroll.py:113-141).  No run at
    all gives a (0, 0) array."""
    assert isinstance(intervals, pd.DataFrame)
    sel = intervals.loc[intervals["low_or_high"] == code, ["posterior_sample", "dwell_time"]]
    s = sel["posterior_sample"].to_numpy().astype(np.int64)
    d = sel["dwell_time"].to_numpy()
    n_values = len(np.unique(s))
    if n_values == 0:
        return np.zeros((0, 0), dtype=np.float32)
    max_count = int(np.bincount(s).max())
    keep = s < n_values
    s, d = s[keep], d[keep]
    order = np.argsort(s, kind="stable")
    s, d = s[order], d[order]
    col = np.arange(len(s)) - np.searchsorted(s, s, side="left")
    data = np.zeros((n_values, max_count), dtype=np.float32)
    data[s, col] = d
    return data


def bound_dwell_times(intervals):
    """Interior bound dwell times (``low_or_high == 1``) per posterior sample, zero-padded."""
    return _dwell_times(intervals, 1)


def unbound_dwell_times(intervals):
    """Interior unbound dwell times (``low_or_high == 0``) per posterior sample, zero-padded."""
    return _dwell_times(intervals, 0)


# ---- two-state rates and resampling intervals (tapqir/utils/imscroll.py:199-317) --------------------------------------
def _pairs(labels):
    """(z_f, z_{f+1}) over the frame pairs of the last axis."""
    return labels[..., :-1], labels[..., 1:]


@singledispatch
def association_rate(labels):
    r"""On-rate of binary labels (..., N, F) under a two-state model: the share of unbound frames followed by a bound one,
    pooled over the last two axes."""
    raise NotImplementedError


@association_rate.register(np.ndarray)
def _(labels):
    now, nxt = _pairs(labels)
    return ((1 - now) * nxt).sum((-2, -1)) / (1 - now).sum((-2, -1))


@association_rate.register(torch.Tensor)
def _(labels):
    now, nxt = _pairs(labels.float())
    return ((1 - now) * nxt).sum((-2, -1)) / (1 - now).sum((-2, -1))


@singledispatch
def dissociation_rate(labels):
    r"""Off-rate of binary labels (..., N, F) under a two-state model: the share of bound frames followed by an unbound
    one, pooled over the last two axes."""
    raise NotImplementedError


@dissociation_rate.register(np.ndarray)
def _(labels):
    now, nxt = _pairs(labels)
    return (now * (1 - nxt)).sum((-2, -1)) / now.sum((-2, -1))


@dissociation_rate.register(torch.Tensor)
def _(labels):
    now, nxt = _pairs(labels.float())
    return (now * (1 - nxt)).sum((-2, -1)) / now.sum((-2, -1))


def _percentile_interval(estimand, probs):
    """pyro.ops.stats.pi: the linear-interpolation quantiles at (1 - probs) / 2 and (1 + probs) / 2."""
    from tapqir_amd.utils.stats import quantile

    estimand = torch.as_tensor(estimand)
    return quantile(estimand, (1 - probs) / 2), quantile(estimand, (1 + probs) / 2)


@singledispatch
def bootstrap(samples, estimator, repetitions=1000, probs=0.68):
    r"""Percentile interval of ``estimator`` over ``repetitions`` resamples of ``samples`` (along its first axis, with
    replacement, each as long as ``samples``)."""
    raise NotImplementedError


@bootstrap.register(np.ndarray)
def _(samples, estimator, repetitions=1000, probs=0.68):
    estimand = np.zeros((repetitions,))
    for i in range(repetitions):
        estimand[i] = estimator(samples[np.random.randint(0, len(samples), size=len(samples))])
    ll, ul = _percentile_interval(estimand, probs)
    return ll.item(), ul.item()


@bootstrap.register(torch.Tensor)
def _(samples, estimator, repetitions=1000, probs=0.68):
    estimand = torch.zeros(repetitions)
    for i in range(repetitions):
        estimand[i] = estimator(samples[torch.randint(0, len(samples), (len(samples),), device=samples.device)])
    return _percentile_interval(estimand, probs)


@singledispatch
def posterior_estimate(dist, estimator, repetitions=1000, probs=0.68):
    r"""Percentile interval of ``estimator`` over ``repetitions`` draws of ``dist``, each used whole.

    With ``dist = Bernoulli(p_bound)`` and ``association_rate`` / ``dissociation_rate`` the device computes the same
    estimands without the rasters: ``rates_estimate(rates_sample(p_bound, repetitions))`` of
    ``tapqir_amd.utils.mle_analysis``."""
    raise NotImplementedError


@posterior_estimate.register(torch.distributions.Distribution)
def _(dist, estimator, repetitions=1000, probs=0.68):
    samples = dist.sample((repetitions,))
    estimand = torch.zeros(repetitions)
    for i in range(repetitions):
        estimand[i] = estimator(samples[i])
    return _percentile_interval(estimand, probs)


@singledispatch
def sample_and_bootstrap(dist, estimator, preprocess=None, repetitions=1000, probs=0.68):
    r"""Percentile interval of ``estimator`` over ``repetitions`` rounds of: draw ``dist`` once, ``preprocess`` the draw
    if given, resample it along its first axis with replacement.

    With ``dist = Bernoulli(p_bound)`` and the two rate estimators, the device form is
    ``rates_estimate(rates_sample(p_bound, repetitions), bootstrap=True)`` of ``tapqir_amd.utils.mle_analysis``: the rows
    (AOIs) of every raster are resampled."""
    raise NotImplementedError


@sample_and_bootstrap.register(torch.distributions.Distribution)
def _(dist, estimator, preprocess=None, repetitions=1000, probs=0.68):
    estimand = torch.zeros(repetitions)
    for i in range(repetitions):
        samples = dist.sample()
        if preprocess is not None:
            samples = preprocess(samples)
        estimand[i] = estimator(samples[np.random.randint(0, len(samples), size=len(samples))])
    return _percentile_interval(estimand, probs)
