"""
The guide-site sampling kernels in the regime of a converged fit, on the MI355X.

Every sampling launch draws its AffineBeta sites through tq_site_beta_compact (tq_beta_compact.h): a workgroup of 256 draws
classifies each draw by the regime of torch's piecewise _dirichlet_grad, appends tasks to three LDS regions filled from both
ends (wave-aggregated LDS atomics, mbcnt prefix positions), evaluates the queues with class c starting on the wave after class
c - 1, and scatters the results back through L.res.  The code is device-only, and at the initial parameters -- where every
other GPU test starts -- every draw is in the saddle-point pair class and every workgroup skips the queue.  Here the
parameters are spread as a converged fit spreads them (site_fixture.converged_parameters) and whole workgroups are placed by
hand (site_fixture.HAND_PLACED); every stored site term goes against a plain float64 reference within
site_fixture.site_budget, and every test names the kernel it reaches and asserts the regime counts its inputs were built for.
The same runners pass on the g++ build of the math in test_site_regimes_host.py, so a failure here points at the device code.

Also reached here in their device builds only: tq_beta_grad_pair_rest and tq_body_site (tq_minibatch_kernel), the Gamma sites
at alpha < 1 and tq_sample_std_gamma at concentrations below 1.

Measured on the MI355X (worst error / allowance per stored row and launch family): DESIGN.md, "Guide sites in the converged
regime".
"""

import ctypes as C

import pytest
import torch

from helpers import gradient_report, replay_steps
from site_fixture import HAND_PLACED, WAVE, beta_site_regimes, check_sites, site_budget, site_inputs, site_reference, waves
from test_site_regimes_host import (HAND_DKW, REGIMES, assert_converged_mix, assert_hand_placed, clamp_masks, converged_step_case,
                                    drawn_sites, latents_of, law_of_the_draws, run_given_sites, site_report, stored_sites)

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("gradient_report", "site_report")]
assert gradient_report and site_report  # (fixtures: imported for pytest to find them)

DEV = "cuda:0"


# ---- (a) given draws, random converged parameters ------------------------------------------------------------------------------
def test_given_draws_two_workgroups_per_site():
    # tq_sample_locals_kernel, N = 10, F = 30, K = 2: 300 units = two workgroups per site; the second has 44 live lanes in one
    # wave and three waves with no live lane, which still take tasks and meet both barriers.
    eng, inp, _ = run_given_sites(dict(N=10, F=30), 2, "given N=10 F=30 K=2", device=DEV)
    assert_converged_mix(inp)
    for k in beta_site_regimes(inp).values():
        w = waves(k)
        assert [(r[0], r[1], r[2]) for r in w] == [(0, 0, 64), (0, 1, 64), (0, 2, 64), (0, 3, 64), (1, 0, 44)]


GIVEN = [
    # id, dataset, K, units
    ("75_units_K1", dict(N=5, F=15), 1, 75),             # one workgroup, a wave of 11 live lanes and two waves with none
    ("256_units_K2", dict(N=8, F=32), 2, 256),           # exactly one full workgroup
    ("K3_P9", dict(N=2, F=2, P=9), 3, 4),
    ("K4", dict(N=2, F=2), 4, 4),
    ("two_channels", dict(N=5, F=30, C=2), 2, 300),      # unit decode across channels
]


@pytest.mark.parametrize("name,dkw,K,units", GIVEN, ids=[c[0] for c in GIVEN])
def test_given_draws(name, dkw, K, units):
    # tq_sample_locals_kernel with draw_locals = 0: tq_site_beta_compact on the given draws of every AffineBeta site
    eng, inp, _ = run_given_sites(dkw, K, "given " + name, device=DEV)
    assert inp["a"].shape == (1 + 4 * K, units) and eng.K == K
    assert not bool(inp["clamped"].any())
    mixed = [r[4] for k in beta_site_regimes(inp).values() for r in waves(k)]
    assert any(mixed), "no wave of this case goes through the queue"


# ---- (b) hand-placed workgroups ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(HAND_PLACED))
def test_hand_placed_workgroup(case):
    # tq_sample_locals_kernel, N = 8, F = 32, K = 1, P = 15: one full workgroup per site, the x and y sites placed lane by lane
    eng, inp, tasks = run_given_sites(HAND_DKW, 1, "hand-placed " + case, device=DEV, hand=case)
    assert_hand_placed(inp, tasks, case)
    k = beta_site_regimes(inp)[3]  # the x site (the y site holds the same lanes)
    w = waves(k)
    tasks = tasks.tolist()
    if case == "all_series":              # R1 filled from the bottom, `qc += 256` taken twice
        assert tasks == [0, 512, 0, 0, 0]
    elif case == "all_rational":          # R1 filled from the top
        assert tasks == [0, 0, 0, 0, 512]
    elif case == "series_and_rational":   # the two ends of R1 meet with no free slot
        assert tasks == [0, 256, 0, 0, 256]
    elif case == "one_lane_outside_the_pair":
        # waves 0, 1, 3 evaluate in place; wave 2 goes through the queue with its 63 pair draws and the two rational tasks
        assert [r[4] for r in w] == [False, False, True, False] and tasks == [255, 0, 0, 0, 2]
        assert w[2][3].tolist() == [63, 0, 0, 0, 2]
    elif case == "one_pair_lane":
        assert all(r[4] for r in w) and tasks[0] == 1 and w[1][3][0] == 1
    elif case == "all_five_classes":      # wave0 advances through all five loops, both codes of class 3 present
        assert all(r[4] and bool((r[3] > 0).all()) for r in w)
        kinds = HAND_PLACED[case]
        assert "saddle_hi" in kinds and "saddle_lo" in kinds
    elif case == "clamp_values":          # rows 2 and 4 exactly 0, log q finite
        site, _ = stored_sites(eng)
        on = inp["clamped"][3:]
        assert int(on.sum()) == 2 * 128
        assert bool((site[2, 3:][on] == 0).all()) and bool((site[4, 3:][on] == 0).all())
        assert bool(torch.isfinite(site[0, 3:][on]).all())


# ---- (c) drawn on the device ---------------------------------------------------------------------------------------------------
def test_drawn_on_the_device():
    # tq_sample_locals_kernel with draw_locals = 1: tq_site_draw (tq_sample_std_gamma at concentrations from 0.03) feeds
    # tq_site_beta_compact; then tq_cosmos_sample_locals_range over the AffineBeta sites alone.
    K = 2
    o, eng, a, inp, site, lat = drawn_sites(dict(N=10, F=30), K, "device draws", device=DEV)
    for k in beta_site_regimes(inp).values():
        assert all(r[4] for r in waves(k))
    # the law of the draws
    p_beta, p_gamma, n_beta, n_gamma = law_of_the_draws(inp)
    REGIMES.append("device draws: KS p-value AffineBeta %.3g (%d draws)  Gamma %.3g (%d draws)" % (p_beta, n_beta, p_gamma, n_gamma))
    assert p_beta > 1e-4 and p_gamma > 1e-4, (p_beta, p_gamma)
    # the AffineBeta sites in a launch of their own: bitwise the rows of the full launch, nothing else written
    eng.site.fill_(float("nan"))
    eng.lat.fill_(float("nan"))
    assert eng.lib.tq_cosmos_sample_locals_range(C.byref(a), K + 1, 3 * K, None, eng._stream()) == 0
    torch.cuda.synchronize()
    site_r, lat_r = stored_sites(eng)
    assert torch.equal(lat_r[1 + K:], lat[1 + K:]) and torch.equal(site_r[:, 1 + K:], site[:, 1 + K:])
    assert bool(torch.isnan(lat_r[:1 + K]).all()) and bool(torch.isnan(site_r[:, :1 + K]).all())


# ---- (d) the other two launch families, at site level --------------------------------------------------------------------------
def first_step_sites(eng, o, nd, fd, where, **step_kw):
    """One first step of the engine, then its draws and stored site terms against the reference at the parameters before it."""
    eng.step(**step_kw)
    eng.join()
    torch.cuda.synchronize()
    site, _ = stored_sites(eng)
    inp = site_inputs(o, nd, fd, latents_of(eng, (len(nd), len(fd), eng.C)))
    ref = site_reference(inp)
    check_sites(site, inp, ref, site_budget(inp, ref), where)
    return inp


def test_full_batch_step_overlapped():
    # tq_sample_locals_tail_kernel (row 0 of its grid is the tail) inside tq_cosmos_step_overlapped: N = 10, F = 30, K = 2
    N, F = 10, 30
    d, o, eng = converged_step_case(dict(N=N, F=F), 2, device=DEV, small_full_max_units=0)
    assert eng._route(N, F, None) == "overlapped"
    inp = first_step_sites(eng, o, torch.arange(N), torch.arange(F), "overlapped first step")
    for k in beta_site_regimes(inp).values():
        assert all(r[4] for r in waves(k))


def test_minibatch_step_one_launch():
    # tq_minibatch_kernel: the device build of the uncompacted tq_body_site / tq_beta_grad_pair_rest; a contiguous minibatch
    # of 3 x 20 of N = 10, F = 30, batch rows decoded through ndx / fdx
    N, F = 10, 30
    d, o, eng = converged_step_case(dict(N=N, F=F), 2, device=DEV)
    nd, fd = torch.arange(2, 5), torch.arange(5, 25)
    assert len(fd) * eng.C >= 16 and eng._route(len(nd), len(fd), None) == "one_launch"
    inp = first_step_sites(eng, o, nd, fd, "one_launch first step", ndx=nd, fdx=fd)
    k = torch.stack([v.sum(1) for v in beta_site_regimes(inp).values()]).sum(0)
    assert bool((k[[0, 1, 2, 4]] > 0).all()), k.tolist()  # every regime of tq_beta_grad_pair_rest but the rare one


# ---- (e) whole steps -----------------------------------------------------------------------------------------------------------
def test_whole_steps_overlapped():
    # three steps of the overlapped route at the converged parameters, replayed by the oracle with the draws the kernel calls
    # clamped detached; the per-element budgets of helpers.assert_gradients_match unchanged
    N, F = 10, 30
    d, o, eng = converged_step_case(dict(N=N, F=F), 2, device=DEV, small_full_max_units=0)
    assert eng._route(N, F, None) == "overlapped"

    def step(eng, it):
        eng.step()
        return torch.arange(N), torch.arange(F)

    replay_steps(eng, o, step, steps=3, where="overlapped converged", clamped=clamp_masks)
    assert WAVE == 64
