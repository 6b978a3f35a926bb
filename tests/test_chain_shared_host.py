"""CPU tests of what the three hidden-Markov families share since they run one set of sweeps, through
the ``hk_*`` entry points of the g++ build: the batched E-step with one replica is ``hk_hmm_estep`` bit for bit, scratch of
a_f included, and the joint E-step without gamma is the joint E-step with gamma bit for bit.  The GPU twin is
test_gpu_chain_shared.py."""

import numpy as np
import pytest

import hmm_fixture
import joint_fixture
import multistart_fixture

N = 6
THETA_A, THETA_B = (0.05, 0.10, 0.3), (0.04, 0.08, 0.4)  # (kon, koff, pi0) of the two channels' two-state chains


@pytest.fixture(scope="module")
def libs(tmp_path_factory):
    d = tmp_path_factory.mktemp("chain")
    return {"hmm": hmm_fixture.build_hmm_check(d), "multistart": multistart_fixture.build_multistart_check(d),
            "joint": joint_fixture.build_joint_check(d)}


@pytest.mark.parametrize("U,B", [(1, 1), (1, 2), (2, 2)])
@pytest.mark.parametrize("F", [1, 64, 65, 130])
def test_one_replica_of_the_batched_estep_is_the_hmm_estep(libs, U, B, F):
    theta = hmm_fixture.fixed_theta(U, B)
    p = hmm_fixture.with_special_rows(hmm_fixture.synthetic_hmm(N, F, seed=F)[0], hmm_fixture.PRIOR)
    want = hmm_fixture.host_estep(libs["hmm"], p, theta, U, B, hmm_fixture.PRIOR)
    filt = np.full((1, N, F, U + B), np.nan)
    rows = multistart_fixture.host_estep(libs["multistart"], p, theta[None], U, B, hmm_fixture.PRIOR, filt=filt)
    assert np.isfinite(want["rows"]).all() and np.isfinite(want["filt"]).all()
    assert np.array_equal(rows[0], want["rows"])
    assert np.array_equal(filt[0], want["filt"])


@pytest.mark.parametrize("F", [1, 65, 130])
def test_the_joint_estep_without_gamma_is_the_joint_estep_with_gamma(libs, F):
    pa, pb = joint_fixture.estep_inputs(N, F, seed=F)
    theta = joint_fixture.start_from(THETA_A, THETA_B)
    full = joint_fixture.host_estep(libs["joint"], pa, pb, theta[None], gamma=True)
    bare = joint_fixture.host_estep(libs["joint"], pa, pb, theta[None], gamma=False)
    assert "gamma" not in bare and np.isfinite(full["gamma"]).all() and np.isfinite(full["rows"]).all()
    assert np.array_equal(bare["rows"], full["rows"])
    assert np.array_equal(bare["filt"], full["filt"])
