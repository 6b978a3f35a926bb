"""The credible-interval test grid (shared by tests/test_quantile.py and tests/test_gpu_quantile.py) and its oracle.

The grid covers what the model's constraints can produce; the oracle is the pair of scipy helpers of
``tapqir_amd.utils.stats`` that the device path replaces.  Tolerance: |got - scipy| <= 1e-8 (UL - LL)_scipy for LL and
for UL at every grid point: two decades above scipy's own self-consistency on this grid (9e-11 of the width for Beta,
9e-14 for Gamma, against 200-step bisection on its own CDF) and below the 6e-8 resolution of the fp32 parameters.
"""

import functools

import numpy as np
import torch

from tapqir_amd.utils.stats import affine_beta_interval, gamma_interval

TOL = 1e-8
CIS = (0.95, 0.999)
BOUNDS = ((-7.5, 7.5), (0.75, 2.25))
KIND_GAMMA, KIND_AFFINE_BETA = 0, 1


@functools.lru_cache(maxsize=None)
def gamma_grid():
    """(loc, beta) in fp32: concentration logspace(-2, 6, 33) x rate {1e-3, 1, 50}."""
    conc, rate = np.meshgrid(np.logspace(-2, 6, 33), np.array([1e-3, 1.0, 50.0]), indexing="ij")
    return torch.tensor((conc / rate).ravel(), dtype=torch.float32), torch.tensor(rate.ravel(), dtype=torch.float32)


@functools.lru_cache(maxsize=None)
def beta_grid(low, high):
    """(mean, size) in fp32: t {1e-3 .. 0.999} x size 2 + logspace(-2, 5, 15)."""
    t, size = np.meshgrid(np.array([1e-3, 1e-2, 0.1, 0.3, 0.5, 0.7, 0.9, 0.99, 0.999]), 2 + np.logspace(-2, 5, 15), indexing="ij")
    mean = low + (high - low) * t
    return torch.tensor(mean.ravel(), dtype=torch.float32), torch.tensor(size.ravel(), dtype=torch.float32)


@functools.lru_cache(maxsize=None)
def gamma_oracle(CI):
    ll, ul, _ = gamma_interval(*gamma_grid(), CI)
    return ll.numpy(), ul.numpy()


@functools.lru_cache(maxsize=None)
def beta_oracle(low, high, CI):
    ll, ul, _ = affine_beta_interval(*beta_grid(low, high), low, high, CI)
    return ll.numpy(), ul.numpy()


def worst_error(ll, ul, ref_ll, ref_ul):
    """max over the points of |got - ref| / (UL - LL)_ref, LL and UL together; the oracle must be a proper interval."""
    ll, ul = np.asarray(ll, dtype=np.float64), np.asarray(ul, dtype=np.float64)
    width = ref_ul - ref_ll
    assert np.isfinite(ref_ll).all() and np.isfinite(ref_ul).all() and (width > 0).all()
    assert np.isfinite(ll).all() and np.isfinite(ul).all()
    return float(max((np.abs(ll - ref_ll) / width).max(), (np.abs(ul - ref_ul) / width).max()))
