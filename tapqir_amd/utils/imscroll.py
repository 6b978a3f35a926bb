"""
Time to first binding of binary or probabilistic spot-presence rasters (tapqir/utils/imscroll.py:143-196).

For binary labels ``z`` (..., F) the result is the index of the first frame with ``z = 1``, or ``F`` if there is none:

    ttfb = sum_{f=1}^{F-1} f z_f prod_{f' < f} (1 - z_f') + F prod_{f'} (1 - z_f')

For probabilities ``q(z_f = 1)`` the same expression is the expectation of that index under independent frames.
"""

from functools import singledispatch

import numpy as np
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
