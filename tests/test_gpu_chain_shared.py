"""GPU tests of what the three hidden-Markov families share since their kernels call one E-step body (DESIGN.md section
28): ``multistart_estep`` with one replica returns the rows and the scratch of a_f of ``hmm_estep`` bit for bit, and
``joint_estep`` without gamma returns the rows and filt of ``joint_estep`` with gamma bit for bit.  F = 1, F around the 64
lanes (a lane without frames, the last lane with frames holding the identity suffix) and more than one frame per lane.  The
host twin is test_chain_shared_host.py."""

import numpy as np
import pytest
import torch

from hmm_fixture import PRIOR, fixed_theta, synthetic_hmm, with_special_rows
from joint_fixture import PRIORS, estep_inputs
from tapqir_amd.utils.joint_analysis import joint_estep, joint_start_from
from tapqir_amd.utils.mle_analysis import hmm_estep, multistart_estep

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N = 6
THETA_A, THETA_B = (0.05, 0.10, 0.3), (0.04, 0.08, 0.4)  # (kon, koff, pi0) of the two channels' two-state chains


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


@pytest.mark.parametrize("U,B", [(1, 1), (1, 2), (2, 2)])
@pytest.mark.parametrize("F", [1, 64, 65, 130])
def test_one_replica_of_the_batched_estep_is_the_hmm_estep(U, B, F):
    theta = dev(fixed_theta(U, B))
    p = dev(with_special_rows(synthetic_hmm(N, F, seed=F)[0], PRIOR))
    want = hmm_estep(p, theta, PRIOR, U, B)
    scratch = torch.full((1, N, F, U + B), float("nan"), dtype=torch.float64, device=DEV)
    rows = multistart_estep(p, theta[None], PRIOR, U, B, scratch=scratch)
    assert bool(torch.isfinite(want["rows"]).all()) and bool(torch.isfinite(want["filt"]).all())
    assert torch.equal(rows[0], want["rows"])
    assert torch.equal(scratch[0], want["filt"])


@pytest.mark.parametrize("F", [1, 65, 130])
def test_the_joint_estep_without_gamma_is_the_joint_estep_with_gamma(F):
    pa, pb = (dev(x) for x in estep_inputs(N, F, seed=F))
    theta = joint_start_from(torch.tensor(THETA_A, dtype=torch.float64), torch.tensor(THETA_B, dtype=torch.float64)).to(DEV)
    full = joint_estep(pa, pb, theta[None], *PRIORS, gamma=True)
    bare = joint_estep(pa, pb, theta[None], *PRIORS, gamma=False)
    assert "gamma" not in bare and bool(torch.isfinite(full["gamma"]).all()) and bool(torch.isfinite(full["rows"]).all())
    assert torch.equal(bare["rows"], full["rows"])
    assert torch.equal(bare["filt"], full["filt"])
