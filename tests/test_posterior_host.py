"""
The posterior read-out on the CPU: the g++ build of tq_body_probs_globals / tq_body_probs_unit / tq_zt_responsibilities
(tests/hostcheck) against the float64 oracle per element, within the allowance posterior_fixture derives from the oracle's own
float32 pass; the law and the stream keys of the x / y draws (hc_probs_xy_draws replays them through the helpers the body
calls); the law of the global draws; and the outputs of draw = 1 against the oracle on those very draws.  The runners take
a backend: test_gpu_posterior.py runs them on the device.  Cases, allowance and measured figures: DESIGN.md, "Posterior
read-out: what is checked".
"""

import numpy as np
import pytest
import torch

import posterior_fixture as pf
from launch_fixture import copy_shard_params
from posterior_fixture import HOST


@pytest.fixture
def posterior_report(capsys):
    """Prints the worst error over the allowance of every check a test ran, per case and backend."""
    pf.WORST.clear()
    yield
    with capsys.disabled():
        for line in pf.WORST.values():
            print("\n" + line, end="")
    pf.WORST.clear()


pytestmark = pytest.mark.usefixtures("posterior_report")


# ---- 1. given draws -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", pf.GIVEN_CASES)
def test_given_draws_match_the_oracle_per_element(name):
    pf.run_given(HOST, name)


def test_cases_reach_what_they_are_built_for():
    """Units per case against the workgroup of 256, and on-target units on both sides of every workgroup boundary."""
    for name, c in pf.CASES.items():
        d = pf.case(name)[0]
        N, F, C = d.images.shape[:3]
        assert N * F * C == c["units"]
        assert bool(d.is_ontarget.any()) and bool((~d.is_ontarget).any())
        on = d.is_ontarget.repeat_interleave(F * C)
        if c["units"] > pf.WG:
            assert bool(on[:pf.WG].any()) and bool((~on[:pf.WG]).any()) and bool(on[pf.WG:].any())
    assert pf.CASES["partial_workgroup"]["units"] % pf.WG == 44 and pf.CASES["full_workgroup"]["units"] == pf.WG
    assert pf.CASES["two_channels"]["units"] > pf.WG and pf.CASES["crosstalk_two_workgroups"]["units"] > pf.WG
    assert pf.CASES["K4"]["K"] == 4 and pf.CASES["one_particle"]["S"] == 1


def test_crosstalk_globals_sit_where_the_read_out_looks():
    """tq_body_probs_globals reads the globals at params + NLOCAL U + 2 Nt C; the crosstalk layout appends alpha behind them."""
    d, o = pf.case("crosstalk")[:2]
    eng = pf.engine_for(HOST, d, o)
    lay = eng.layout
    assert lay.crosstalk and lay.slots()["gain_loc"][0] == (8 * eng.K + 2) * lay.U + 2 * eng.Nt * eng.C
    assert lay.slots()["alpha_mean"][0] == lay.slots()["pi_size"][0] + eng.C


# ---- 2. the draw path ---------------------------------------------------------------------------------------------------------
def test_law_of_the_replayed_draws():
    """S = 2000 on 24 units: per (k, axis), pooled over units, the draws through their own guide's cdf are uniform."""
    from scipy import stats

    d, o = pf.law_case()
    xy = pf.replay_xy(pf.engine_for(HOST, d, o), pf.LAW_S, seed=3)
    lo, hi = pf.xy_clamp_values(o)
    assert float(((xy == lo) | (xy == hi)).double().mean()) < 1e-3
    pit = pf.xy_pit(o, xy)
    ps = {}
    for j in range(2 * o.K):
        ps["%s[%d]" % ("xy"[j // o.K], j % o.K)] = stats.kstest(pit[:, j].reshape(-1), "uniform").pvalue
    pf.WORST[("xy draws", "law", "host")] = "posterior x / y draws [host]: KS p-values %s" % "  ".join("%s %.3g" % kv for kv in ps.items())
    assert min(ps.values()) > pf.KS_LEVEL, ps
    # streams that share a key give dependent draws: the transforms of neighbours along every axis of [S][2K][U] are uncorrelated
    n = pit[1:].size
    corr = lambda a, b: abs(float(np.corrcoef(a.reshape(-1), b.reshape(-1))[0, 1]))
    worst = max(corr(pit[1:], pit[:-1]), corr(pit[:, 1:], pit[:, :-1]), corr(pit[:, :, 1:], pit[:, :, :-1]),
                corr(pit[:, :o.K], pit[:, o.K:]))
    assert worst < 5.0 / np.sqrt(n / 2), worst


def test_streams_differ_across_particles_units_k_and_axis():
    """Every unit, spot and axis on ONE guide (same mean, same size): two draws are then equal exactly where two streams share
    their key.  A different seed changes every draw."""
    d, o = pf.law_case()
    o = pf.make_oracle(d, 2, perturb=0.0)
    eng = pf.engine_for(HOST, d, o)
    xy = pf.replay_xy(eng, pf.DRAWN_S, seed=3)
    lo, hi = pf.xy_clamp_values(o)
    assert not bool(((xy == lo) | (xy == hi)).any())
    assert len(np.unique(xy.numpy())) == xy.numel(), (len(np.unique(xy.numpy())), xy.numel())
    other = pf.replay_xy(eng, pf.DRAWN_S, seed=4)
    assert bool((other != xy).all())
    assert torch.equal(pf.replay_xy(eng, pf.DRAWN_S, seed=3), xy)


def test_a_shard_replays_the_draws_of_its_global_units():
    d, o = pf.law_case()
    full = pf.engine_for(HOST, d, o)
    N, F, C = d.images.shape[:3]
    eng = HOST.engine(pf.shard_of(d, 3), o.K, n_offset=3, Nt_global=N)
    copy_shard_params(full, eng, 3, N)
    xy_full, xy_shard = pf.replay_xy(full, pf.DRAWN_S, seed=3), pf.replay_xy(eng, pf.DRAWN_S, seed=3)
    assert xy_shard.shape[2] == (N - 3) * F * C and torch.equal(xy_shard, xy_full[:, :, 3 * F * C:])
    assert not torch.equal(xy_shard, xy_full[:, :, :(N - 3) * F * C])


def test_law_of_the_global_draws():
    pf.run_global_law(HOST)


@pytest.mark.parametrize("name", pf.DRAWN_CASES)
def test_what_the_draws_give(name):
    """draw = 1 of the host build against the oracle on the replayed x / y and the read-back global base draws: both sides
    run the same draws, so every unit meets the allowance of the given-draw cases."""
    pf.run_what_the_draws_give(HOST, name)
