"""The kinetics boundary cases (kinetics_boundary_fixture.py) on the g++ build: ``hk_dwell_fit_steps`` and
``hk_ttfb_fit_steps`` replay one launch of ``tq_dwell_fit`` / ``tq_ttfb_fit`` serially -- the kernel's lane-strided
partial sums, the pairwise tree of ``tq_group_sum<64>``, the shared inline bodies and ``TqFitAdam`` -- and go through the
same rule as the device.  So the cases, the reference and the bounds are proven without a GPU, and a device failure can
be placed: in the bodies if this file fails too, in the ``.hip`` wrapper or the hardware transcendentals if only the
device fails.

Measured with this build (worst error / bound over all rows of a case; at most 1 passes):
  dwell gradient, K = 1 .. 8, worst of the four states: 0.10, 0.17, 0.16, 0.08, 0.14, 0.14, 0.10, 0.15
  dwell loss <= 0.24, |g| from v <= 0.18, update (p, m, v against float64 Adam, 4 float32 eps) <= 0.45
  ttfb over the 25 (N, Nc) cases and both routes: gradient 0.47, loss 0.25, |g| from v 0.18, update 0.45
  step t = 10 000 from non-zero moments: dwell K = 8 0.38, ttfb 0.28
  300-step trajectories, K = 4 .. 8, relative to torch_fit64: k 3.2e-6, 1.4e-5, 9.9e-6, 9.6e-6, 1.9e-5; A <= 6.7e-6; loss
      <= 1.3e-7
"""

import pytest
import torch

import kinetics_boundary_fixture as kb
from dwell_fixture import build_dwell_check
from ttfb_fixture import build_kinetics_check


@pytest.fixture(scope="module")
def libs(tmp_path_factory):
    out = tmp_path_factory.mktemp("kinetics_boundaries")
    dwell, kinetics = build_dwell_check(out), build_kinetics_check(out)
    kb.bind_fit_steps(dwell, kinetics)
    return dwell, kinetics


def assert_within(report, where, names=None):
    for key, (excess, row) in kb.worst(report).items():
        label = row if names is None else names[row]
        print(f"{where} {key}: worst excess {excess:.3g} (row {label})")
        assert excess <= 1.0, (where, key, excess, label)


# ---- section 1: one step ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", kb.DWELL_STATES)
@pytest.mark.parametrize("K", range(1, 9))
def test_dwell_step(libs, K, kind):
    """Gradient, loss and update of one step of every K at every row length of DWELL_LENS, against float64."""
    csr, par0 = kb.dwell_rows(), kb.dwell_par0(K, kind)
    before = kb.dwell_state(par0)
    after, loss = kb.host_dwell_steps(libs[0], before, csr, K)
    assert_within(kb.step_report(before, after, loss, kb.dwell_reference(K, kind), 2 * K), f"dwell K={K} {kind}",
                  kb.DWELL_LENS)
    assert torch.equal(after[0], before[0]) and loss[0] == 0  # the empty row: zero gradient, untouched state
    if K == 1:  # no free weight: the logit gradient is exactly zero
        assert (after[:, 1] == par0[:, 1]).all() and (after[:, 3] == 0).all() and (after[:, 5] == 0).all()


@pytest.mark.parametrize("N,Nc", kb.TTFB_CASES)
def test_ttfb_step(libs, N, Nc):
    """Gradient, loss and update of one step at every composition and state of a row, both routes, against float64."""
    data, control, par0 = kb.ttfb_case(N, Nc)
    before, ref, names = kb.ttfb_state(par0), kb.ttfb_reference(N, Nc), kb.ttfb_row_names()
    out = {}
    for staged in (True, False):
        after, loss = out[staged] = kb.host_ttfb_steps(libs[1], before, data, control, staged)
        assert_within(kb.step_report(before, after, loss, ref, 3), f"ttfb N={N} Nc={Nc} staged={staged}", names)
    for r, name in enumerate(names):
        row = name.split("/")[0]
        if row == "all_zero" and not Nc:  # nothing but tau = 0: zero gradient, untouched state
            assert torch.equal(out[True][0][r], before[r]), name
        if row in kb.TTFB_SAME_LANES or N > 8192:
            assert kb.same_bits(out[True][0][r], out[False][0][r]) and kb.same_bits(out[True][1][r], out[False][1][r]), name


def test_late_step(libs):
    """Step t = 10 000 (step0 = 9999) from non-zero moments against float64 Adam: dwell at K = 8, and ttfb."""
    K = 8
    csr, par0 = kb.dwell_rows(), kb.dwell_par0(K, "perturbed")
    excess = kb.late_step_excess(lambda st, step0: kb.host_dwell_steps(libs[0], st, csr, K, step0)[0], par0, 2 * K, 11)
    print(f"dwell K=8 step 10000: worst excess {float(excess.max()):.3g}")
    assert excess.max() <= 1.0, excess
    data, control, par0 = kb.ttfb_case(129, 65)
    excess = kb.late_step_excess(lambda st, step0: kb.host_ttfb_steps(libs[1], st, data, control, True, step0)[0], par0, 3,
                                 12)
    print(f"ttfb step 10000: worst excess {float(excess.max()):.3g}")
    assert excess.max() <= 1.0, excess


# ---- section 2: short trajectories ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", kb.TRAJ_KS)
def test_dwell_trajectory(libs, K):
    """300 steps on the 4 x 300 data at K = 4 .. 8 against torch_fit64, 1e-4 relative on k and A; the reported loss is the
    float64 loss at the parameters the last step starts from."""
    data = kb.trajectory_data()
    want, loss64 = kb.trajectory_reference(K)
    state = kb.dwell_state(kb.dwell_par0(K, "initial", S=data.shape[0]))
    state, loss = kb.host_dwell_steps(libs[0], state, kb.padded_csr(data), K, 0, kb.TRAJ_STEPS)
    ek = kb.rel(state[:, :K].exp(), want["k"])
    eA = kb.rel(torch.softmax(state[:, K:2 * K], 1), want["A"])
    el = kb.rel(loss, loss64)
    print(f"dwell trajectory K={K}: rel k {ek:.3g} A {eA:.3g} loss {el:.3g}")
    assert ek <= kb.TRAJ_TOL and eA <= kb.TRAJ_TOL and el < kb.TRAJ_TOL, (K, ek, eA, el)
