"""
Time to first binding of binary or probabilistic spot-presence rasters (tapqir/utils/imscroll.py:143-196), and the
interval table of binary rasters with its padded dwell-time arrays (imscroll.py:14-141).

For binary labels ``z`` (..., F) the result is the index of the first frame with ``z = 1``, or ``F`` if there is none:

    ttfb = sum_{f=1}^{F-1} f z_f prod_{f' < f} (1 - z_f') + F prod_{f'} (1 - z_f')

For probabilities ``q(z_f = 1)`` the same expression is the expectation of that index under independent frames.
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
