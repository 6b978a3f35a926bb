"""
The backward samplers share their draws, their staging and -- the dwell kernels -- their walk and interval sink
(DESIGN.md section 35), so what one launch returns ties to what another returns, bit for bit.  N = 6 with the special rows,
S = 70 (one full block of samples and a partly filled one), F at one frame, a full block, one more, and a third block.
"""

import functools

import numpy as np
import pandas as pd
import pytest
import torch

from hmm_fixture import PRIOR, fixed_theta, synthetic_hmm, with_special_rows
from smooth_dwell_fixture import n01_of_table
from tapqir_amd.utils.imscroll import INTERVAL_COLUMNS
from tapqir_amd.utils.joint_analysis import joint_dwell_intervals, joint_dwell_sample
from tapqir_amd.utils.mle_analysis import (hmm_dwell_intervals, hmm_dwell_sample, hmm_estep, hmm_sample, mixture_sample)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
S = 70
F_LIST = [1, 64, 65, 130]


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


@functools.lru_cache(maxsize=None)
def inputs(U, B, F):
    """The device's filt of the six rows and theta, computed once per case and left unchanged."""
    p = with_special_rows(synthetic_hmm(6, F, seed=F)[0], PRIOR)
    theta = dev(fixed_theta(U, B))
    return hmm_estep(dev(p), theta, PRIOR, U, B)["filt"], theta


@pytest.mark.parametrize("U,B", [(1, 1), (1, 2), (2, 2)])
@pytest.mark.parametrize("F", F_LIST)
def test_one_population_is_tq_hmm_count_bit_for_bit(U, B, F):
    filt, theta = inputs(U, B, F)
    seed = 2**40 + F
    resp = torch.ones(1, 6, dtype=torch.float64, device=DEV)
    got = mixture_sample(filt[None], theta[None], resp, U, B, S, seed=seed, trans=True, raster=True)
    want = hmm_sample(filt, theta, U, B, S, seed=seed, trans=True, raster=True)
    for key in ("counts", "trans", "raster"):
        assert torch.equal(got[key], want[key]), key
    assert not bool(got["pop"].any())


@pytest.mark.parametrize("F", F_LIST)
def test_channel_b_of_the_pair_walk_is_tq_chain_dwell_at_2_2(F):
    """Bit 1 of the joint state is the class ``state >= 2``: the same counts, first-binding frames and intervals, and the
    pair's histograms (S, 2, F) summed over the partner's state are the chain's (S, F)."""
    filt, theta = inputs(2, 2, F)
    seed = 2**40 + F
    pair = joint_dwell_sample(filt, theta, 1, S, seed=seed)
    chain = hmm_dwell_sample(filt, theta, 2, 2, S, seed=seed)
    for key in ("counts", "tau"):
        assert torch.equal(pair[key], chain[key]), key
    for key in ("hist_bound", "hist_unbound"):
        assert pair[key].shape == (S, 2, F) and chain[key].shape == (S, F)
        assert torch.equal(pair[key].sum(1, dtype=torch.int32), chain[key]), key
    table = joint_dwell_intervals(filt, theta, 1, S, seed=seed, sample=pair)
    want = hmm_dwell_intervals(filt, theta, 2, 2, S, seed=seed, sample=chain)
    assert len(INTERVAL_COLUMNS) == 7
    pd.testing.assert_frame_equal(table[INTERVAL_COLUMNS], want[INTERVAL_COLUMNS])


def test_class_counts_of_tq_hmm_count_are_the_run_starts_of_tq_chain_dwell():
    """The two walkers take the same draws: column 0 of the counts, the unbound -> bound transitions of a row, is the
    number of bound runs of the interval table that start after frame 0."""
    U, B, F = 1, 2, 65
    filt, theta = inputs(U, B, F)
    seed = 2**40 + F
    counts = hmm_sample(filt, theta, U, B, S, seed=seed)["counts"].cpu().numpy()
    table = hmm_dwell_intervals(filt, theta, U, B, S, seed=seed)
    assert np.array_equal(n01_of_table(table, S, 6), counts[..., 0])
