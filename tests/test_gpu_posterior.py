"""
The posterior read-out on the MI355X: the checks of tests/test_posterior_host.py on tq_probs_globals_kernel and
tq_probs_kernel<K> -- every given-draw case against the float64 oracle per element (one and two workgroups of 256, a
partial last one, K = 1 .. 4, one particle, two channels, the crosstalk layout, the converged regime, draws on the clamp
values), the law of the global draws and their agreement with the host streams, and the outputs of draw = 1 against the
oracle on the draws the host build replays.  The same runners pass on the g++ build of the math, so a failure here points at
the device code.  Measured figures: DESIGN.md, "Posterior read-out: what is checked".
"""

import pytest
import torch

import posterior_fixture as pf
from posterior_fixture import DEVICE, HOST
from test_posterior_host import posterior_report

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("posterior_report")]
assert posterior_report  # (a fixture: imported for pytest to find it)


@pytest.mark.parametrize("name", pf.GIVEN_CASES)
def test_given_draws_match_the_oracle_per_element(name):
    pf.run_given(DEVICE, name)


def test_law_of_the_global_draws_and_the_host_streams():
    """tq_probs_globals_kernel at 2000 particles: the law of every site, distinct particles, and the base draws of the g++
    build of tq_globals_sample_site on the same keys to 1e-5 relative in at least 99 % of the entries (a rejection test within
    rounding of the fast intrinsics may flip a draw: the condition of test_rsample_kernel_has_the_law_and_matches_the_host_streams)."""
    dev, host = pf.run_global_law(DEVICE), pf.run_global_law(HOST)
    cols = [1, 2, 6, 7]  # proximity, lamda[0], pi[0]
    same = ((dev[:, cols] - host[:, cols]).abs() <= 1e-5 * host[:, cols].abs()).double().mean()
    pf.WORST[("global draws", "streams", "MI355X")] = "posterior global draws: share of entries equal to the host streams %.4f" % float(same)
    assert float(same) >= 0.99, float(same)


@pytest.mark.parametrize("name", pf.DRAWN_CASES)
def test_what_the_draws_give(name):
    """draw = 1 on the device against the oracle on the x / y draws the host build replays and the global base draws the
    device wrote.  The device's gamma sampler runs on the fast intrinsics, so a rejection test within rounding may flip and
    move a unit by up to 1 / S: at most 1 % of the on-target units may lie outside the allowance.  The other units see
    device x, y that differ from the replay by rounding only; their allowance is that of the given-draw cases, formed on
    these particles.  Measured on the MI355X (worst error over the units inside, allowance, share of units outside):
      partial_workgroup  absolute 7.63e-07 of 2e-05     relative 8.31e-06 of 1e-03  0 of 150 units outside
      K4                 absolute 5.06e-08 of 5.02e-06  relative 1.15e-05 of 1e-03  0 of 2
      crosstalk          absolute 4.55e-07 of 2e-05     relative 1.07e-05 of 1e-03  0 of 20
    The worst is 0.04 of the allowance, below the half from which a wider one (4 x measured, at most 2e-4) would have been
    due, so the allowance of the given-draw cases stands.  No unit was moved by a flipped rejection at these seeds."""
    (w_abs, w_rel, share), ref, (z, t) = pf.run_what_the_draws_give(DEVICE, name, flip_share=0.01)
    # two launches with the same seed are bitwise equal; another seed is not
    d, o = pf.drawn_case(name)[:2]
    eng = pf.engine_for(DEVICE, d, o)
    z2, t2, _ = pf.run_drawn(DEVICE, eng, pf.DRAWN_S, 3)
    assert torch.equal(z2, z) and torch.equal(t2, t)
    z3, t3, _ = pf.run_drawn(DEVICE, eng, pf.DRAWN_S, 4)
    assert not torch.equal(z3, z) and not torch.equal(t3, t)
