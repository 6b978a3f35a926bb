"""Two-state rate kernels on the MI355X: the transition counts of posterior rasters against a numpy oracle on the g++ replay
of the dwell-time sampler's raster (which runs no code of the feature), the same counts derived from the interval table of
``dwell_intervals``, pooled and bootstrap totals, the estimands, edge shapes, the law of the counts, the summary's interval,
the MAP use of the count kernel and the ``rates`` command end to end."""

import numpy as np
import pandas as pd
import pytest
import torch
from typer.testing import CliRunner

from dwell_fixture import build_dwell_check, host_raster
from rates_fixture import build_rates_check, host_indices, oracle_counts, oracle_estimands
from tapqir_amd.main import app
from tapqir_amd.utils.dataset import save
from tapqir_amd.utils.mle_analysis import dwell_intervals, rates_estimate, rates_sample, rates_summary
from tapqir_amd.utils.simulate import TEST_PARAMS, simulate
from tapqir_amd.utils.stats import quantile

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ULP = 2.3e-16  # relative: one unit in the last place of a double


@pytest.fixture(scope="module")
def dwell_hk(tmp_path_factory):
    return build_dwell_check(tmp_path_factory.mktemp("rates_dwell"))


@pytest.fixture(scope="module")
def hk(tmp_path_factory):
    return build_rates_check(tmp_path_factory.mktemp("rates"))


@pytest.fixture(scope="module")
def replay(dwell_hk):
    """The input of test_sampler_replay_is_exact (S = 71, N = 37, F = 203, five special rows) with the oracle counts of
    its rasters; shared, and left unchanged, by the tests below."""
    S, seed = 71, 20261016
    gen = torch.Generator().manual_seed(0)
    p = torch.rand(37, 203, generator=gen) ** 3
    p[0] = 0.0
    p[1] = 1.0
    p[2, ::3] = 1.0
    p[3, 50:60] = 0.0
    p[4, 100:] = 1.0
    want = oracle_counts(host_raster(dwell_hk, p.numpy(), S, seed))
    want.setflags(write=False)
    return {"p": p, "S": S, "N": 37, "F": 203, "seed": seed, "counts": want}


def check_estimands(est, totals, who=""):
    """kon / koff of the device against the numpy quotients of the same integers: within 1 ulp, same non-finite values."""
    for got, want in zip((est["kon"], est["koff"]), oracle_estimands(totals)):
        got = got.cpu().numpy()
        assert got.dtype == np.float64 and got.shape == want.shape
        fin = np.isfinite(want)
        assert np.array_equal(np.isfinite(got), fin), who
        assert np.array_equal(got[~fin], want[~fin], equal_nan=True), who
        err = np.abs(got[fin] - want[fin]) / np.abs(np.where(want[fin] == 0, 1.0, want[fin]))
        print(f"{who} max relative error of the quotients: {err.max() if err.size else 0.0:.3g}")
        assert (err <= ULP).all(), (who, err.max())


def test_counts_replay_is_exact(replay):
    p, S, F = replay["p"].to(DEV), replay["S"], replay["F"]
    counts = rates_sample(p, S, seed=replay["seed"])
    assert counts.shape == (S, 37, 4) and counts.dtype == torch.int32 and counts.is_contiguous()
    got = counts.cpu().numpy()
    assert np.array_equal(got, replay["counts"])
    assert (got[..., 1] + got[..., 3] == F - 1).all()
    est = rates_estimate(counts)
    totals = est["totals"].cpu().numpy()
    assert totals.dtype == np.int64 and np.array_equal(totals, replay["counts"].sum(1))
    check_estimands(est, totals, "pooled")
    summary = rates_summary(est)
    assert summary["kon"]["left_out"] == 0 and summary["koff"]["left_out"] == 0


def test_counts_follow_from_the_dwelltime_table(replay):
    """The rasters are those of ``dwelltime``: from the interval table of the existing device code, n01 / n10 are the
    numbers of z = 1 / z = 0 runs that start after frame 0, and n0 / n1 the summed dwell times of the z = 0 / z = 1 runs
    less the frame F - 1 of the run that ends there."""
    p, S, N, F = replay["p"].to(DEV), replay["S"], replay["N"], replay["F"]
    table = dwell_intervals(p, S, seed=replay["seed"])
    s, n, z = (table[c].to_numpy() for c in ("posterior_sample", "aoi", "z"))
    opens_late = (table["start_frame"].to_numpy() > 0).astype(np.int64)
    frames = table["dwell_time"].to_numpy() - (table["stop_frame"].to_numpy() == F - 1)
    want = np.zeros((S, N, 4), np.int64)
    np.add.at(want, (s, n, np.where(z == 1, 0, 2)), opens_late)
    np.add.at(want, (s, n, np.where(z == 1, 3, 1)), frames)
    assert np.array_equal(want, replay["counts"])  # the identity itself, on the oracle
    assert np.array_equal(rates_sample(p, S, seed=replay["seed"]).cpu().numpy(), want)


def test_bootstrap_totals(replay, hk):
    p, S, N, F = replay["p"].to(DEV), replay["S"], replay["N"], replay["F"]
    counts = rates_sample(p, S, seed=replay["seed"])
    est = rates_estimate(counts, bootstrap=True, seed=99)
    idx = host_indices(hk, 99, S, N)
    assert idx.min() >= 0 and idx.max() < N
    want = replay["counts"][np.arange(S)[:, None], idx].sum(1)
    totals = est["totals"].cpu().numpy()
    assert np.array_equal(totals, want)
    assert (totals[:, 1] + totals[:, 3] == N * (F - 1)).all()
    check_estimands(est, totals, "bootstrap")
    assert not np.array_equal(totals, replay["counts"].sum(1))
    again = rates_estimate(counts, bootstrap=True, seed=99)
    assert torch.equal(again["totals"], est["totals"]) and torch.equal(again["kon"], est["kon"])
    other = rates_estimate(counts, bootstrap=True, seed=100)
    assert not torch.equal(other["totals"], est["totals"])
    assert np.array_equal(other["totals"].cpu().numpy(),
                          replay["counts"][np.arange(S)[:, None], host_indices(hk, 100, S, N)].sum(1))
    summary = rates_summary(est)
    assert summary["kon"]["left_out"] == 0 and summary["koff"]["left_out"] == 0


# S = 1; a second, partly filled block of samples; N = 1; F = 2; the 64-frame staging boundary; N beyond one wave's stride
EDGES = [(1, 5, 30), (65, 3, 20), (7, 1, 33), (4, 6, 2), (3, 4, 64), (3, 4, 65), (2, 131, 5)]


@pytest.mark.parametrize("S,N,F", EDGES)
def test_edge_shapes(dwell_hk, hk, S, N, F):
    gen = torch.Generator().manual_seed(S * 1000 + N * 100 + F)
    p = torch.rand(N, F, generator=gen)
    seed = 2**40 + F
    want = oracle_counts(host_raster(dwell_hk, p.numpy(), S, seed))
    counts = rates_sample(p.to(DEV), S, seed=seed)
    assert np.array_equal(counts.cpu().numpy(), want)
    pooled = rates_estimate(counts)
    assert np.array_equal(pooled["totals"].cpu().numpy(), want.sum(1))
    check_estimands(pooled, want.sum(1), "pooled")
    boot = rates_estimate(counts, bootstrap=True, seed=seed)
    want_boot = want[np.arange(S)[:, None], host_indices(hk, seed, S, N)].sum(1)
    assert np.array_equal(boot["totals"].cpu().numpy(), want_boot)
    check_estimands(boot, want_boot, "bootstrap")


def test_one_frame_has_no_transitions():
    S = 5
    counts = rates_sample(torch.rand(3, 1, generator=torch.Generator().manual_seed(1)).to(DEV), S, seed=3)
    assert counts.shape == (S, 3, 4) and not counts.any()
    for bootstrap in (False, True):
        est = rates_estimate(counts, bootstrap=bootstrap)
        assert not est["totals"].any()
        assert torch.isnan(est["kon"]).all() and torch.isnan(est["koff"]).all()
        summary = rates_summary(est)
        for rate in ("kon", "koff"):
            assert summary[rate]["left_out"] == S
            assert all(np.isnan(summary[rate][k]) for k in ("mean", "ll", "ul"))


@pytest.mark.parametrize("p", [0.2, 0.65])
def test_transition_law(p):
    """Constant p: E[sum n01] = E[sum n10] = S N (F - 1) (1 - p) p with p the float32 value the kernel compares against.
    Adjacent indicators (1 - z_f) z_{f+1} are never both 1, so their covariances are negative and the variance is below
    the mean: 5 sigma with sigma^2 taken as the expectation."""
    S, N, F = 4000, 16, 40
    est = rates_estimate(rates_sample(torch.full((N, F), p).to(DEV), S, seed=7))
    totals = est["totals"].sum(0).cpu().numpy().astype(np.float64)
    pf = float(np.float32(p))
    expect = S * N * (F - 1) * (1 - pf) * pf
    for name, got in (("n01", totals[0]), ("n10", totals[2])):
        z = abs(got - expect) / np.sqrt(expect)
        print(f"p = {p}: sum {name} = {got:.0f}, expected {expect:.1f}, {z:.2f} sigma")
        assert z < 5.0, (name, got, expect)
    assert totals[1] + totals[3] == S * N * (F - 1)


@pytest.mark.parametrize("p,starved", [(0.75, "kon"), (0.25, "koff")])
def test_summary_interval_is_the_quantile_of_the_finite_estimands(p, starved):
    """N = 2, F = 6 at p = 0.75: a sample has no unbound frame to bind from with probability (0.75^5)^2 = 5.6 %, so some
    kon estimands are not finite (p = 0.25: the same for koff); mean and limits are those of the rest."""
    S, probs = 400, 0.68
    est = rates_estimate(rates_sample(torch.full((2, 6), p).to(DEV), S, seed=11))
    summary = rates_summary(est, probs)
    for rate in ("kon", "koff"):
        x = est[rate].cpu()
        fin = x[torch.isfinite(x)]
        assert summary[rate]["left_out"] == S - fin.numel()
        if rate == starved:
            assert 0 < S - fin.numel() < S // 4
        want = (fin.mean().item(), quantile(fin, (1 - probs) / 2).item(), quantile(fin, (1 + probs) / 2).item())
        got = (summary[rate]["mean"], summary[rate]["ll"], summary[rate]["ul"])
        print(rate, got, want, summary[rate]["left_out"])
        assert got == pytest.approx(want, rel=1e-12)
        assert got[1] < got[2]


def test_binary_input_counts_the_given_raster():
    """The MAP column: p in {0, 1} is drawn as itself in every sample."""
    z = (torch.rand(6, 90, generator=torch.Generator().manual_seed(5)) < 0.3).float()
    z[0] = 0.0
    z[1] = 1.0
    counts = rates_sample(z.to(DEV), 3, seed=8).cpu().numpy()
    want = oracle_counts(z.numpy())
    for s in range(3):
        assert np.array_equal(counts[s], want)
    est = rates_estimate(rates_sample(z.to(DEV), 1, seed=0))
    check_estimands(est, want.sum(0)[None], "map")


# ---- command line -------------------------------------------------------------------------------------------------
def test_rates_command_end_to_end(tmp_path):
    from tapqir_amd.models import models

    runner = CliRunner()
    save(simulate(2, 8, 30, 1, 14, params=dict(TEST_PARAMS)), tmp_path)
    result = runner.invoke(app, ["--cd", str(tmp_path), "fit", "--model", "cosmos", "--nbatch-size", "8", "--fbatch-size",
                                 "30", "--num-iter", "2", "--cuda", "--no-input"])
    assert result.exit_code == 0, result.output
    m = models["cosmos"](device="cpu", dtype="float")
    m.load(tmp_path, data_only=False)
    mask = m.data.mask[: m.data.N].cpu().bool()
    p_bound = m.params["z_probs"][: m.data.N, :, 0, 1][mask].float().to(DEV)
    assert p_bound.shape == (4, 30)  # simulate: the first half of the AOIs are on target, all selected by the mask
    counts = rates_sample(p_bound, 50, seed=0)
    map_p = m.params["z_map"][: m.data.N, :, 0][mask].float().to(DEV)
    map_est = rates_estimate(rates_sample(map_p, 1, seed=0))

    for flag, bootstrap in (("--bootstrap", True), ("--no-bootstrap", False)):
        result = runner.invoke(app, ["--cd", str(tmp_path), "rates", "--num-samples", "50", flag, "--cuda", "--no-input"])
        assert result.exit_code == 0, result.output
        res = pd.read_csv(tmp_path / "cosmos_rates-channel0.csv", index_col=0)
        assert list(res.index) == ["kon", "koff"]
        assert list(res.columns) == ["Mean", "95% LL", "95% UL", "MAP"]
        summary = rates_summary(rates_estimate(counts, bootstrap=bootstrap, seed=0), 0.95)
        for rate in ("kon", "koff"):
            want = [summary[rate]["mean"], summary[rate]["ll"], summary[rate]["ul"], map_est[rate][0].item()]
            print(flag, rate, res.loc[rate].tolist(), want, summary[rate]["left_out"])
            assert np.allclose(res.loc[rate].to_numpy(dtype=float), want, rtol=1e-12, atol=0, equal_nan=True), (rate, flag)
