"""Hidden-Markov smoothing kernels on the MI355X: the E-step, the M-step and the EM against the numpy oracle of
smooth_fixture by the tolerance rule of DESIGN.md section 20, the Viterbi path exactly, the backward sampler bit-equal to
the g++ replay fed the device's own ``filt`` and ``theta`` (under a margin condition on its draws) and within 5 sigma of the
smoothed law, edge shapes, and ``fit`` then ``smooth`` end to end."""

import numpy as np
import pandas as pd
import pytest
import torch
from typer.testing import CliRunner

from rates_fixture import oracle_counts
from smooth_fixture import (F_LIST, build_smooth_check, host_count, oracle_em, oracle_estep, oracle_mstep, oracle_viterbi,
                            realised_rates, rule_excess, synthetic_chain, with_special_rows)
from tapqir_amd.main import app
from tapqir_amd.utils.dataset import save
from tapqir_amd.utils.mle_analysis import (rates_estimate, smooth_estep, smooth_fit, smooth_mstep, smooth_sample,
                                           smooth_viterbi)
from tapqir_amd.utils.safe_load import load_tpqr
from tapqir_amd.utils.simulate import TEST_PARAMS, simulate

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PRIOR = 1.0 / 3.0
THETA = (0.05, 0.10, 0.4)


@pytest.fixture(scope="module")
def hk(tmp_path_factory):
    return build_smooth_check(tmp_path_factory.mktemp("smooth"))


def dev_theta(theta):
    return torch.tensor(theta, dtype=torch.float64, device=DEV)


def to_numpy(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def check_rule(got, o64, o80, who):
    """filt, gamma and every column group of rows (expected counts, loglik, gamma_0) by the rule; prints each excess."""
    for key in ("filt", "gamma"):
        assert got[key].dtype == np.float64 and got[key].shape == o64[key].shape
        exc = rule_excess(got[key], o64[key], o80[key])
        print(f"{who} {key}: {exc:.3g} of the bound")
        assert exc <= 1.0, (who, key, exc)
    for name, cols in (("counts", slice(0, 4)), ("loglik", slice(4, 5)), ("gamma0", slice(5, 6))):
        exc = rule_excess(got["rows"][:, cols], o64["rows"][:, cols], o80["rows"][:, cols])
        print(f"{who} rows/{name}: {exc:.3g} of the bound")
        assert exc <= 1.0, (who, name, exc)


# ---- E-step -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,F", [(6, F) for F in F_LIST] + [(2, 5000)])
def test_estep_equals_the_oracle(N, F):
    """The inputs of the host test: rows of all 0, all 1, alternating 0 / 1 and p = prior first (as many as N allows)."""
    p = with_special_rows(synthetic_chain(N, F, seed=F)[0], PRIOR)
    o64, o80 = oracle_estep(p, THETA, PRIOR), oracle_estep(p, THETA, PRIOR, np.longdouble)
    out = smooth_estep(torch.from_numpy(p).to(DEV), dev_theta(THETA), PRIOR)
    got = to_numpy(out)
    check_rule(got, o64, o80, f"N = {N}, F = {F}")
    if F == 1:
        assert not got["rows"][:, :4].any()
    again = smooth_estep(torch.from_numpy(p).to(DEV), dev_theta(THETA), PRIOR)
    for key in out:
        assert torch.equal(out[key], again[key]), key  # bit-identical: no atomics, a fixed order of additions


# ---- M-step -----------------------------------------------------------------------------------------------------------
def test_mstep_totals():
    """300 rows, more than the workgroup's 256 threads: theta and the total loglik by the rule, twice the same bits."""
    p = synthetic_chain(300, 40, seed=11)[0]
    rows = smooth_estep(torch.from_numpy(p).to(DEV), dev_theta(THETA), PRIOR)["rows"]
    theta, trace = dev_theta(THETA), torch.full((3,), float("nan"), dtype=torch.float64, device=DEV)
    smooth_mstep(rows, theta, trace, 1)
    rows_host = rows.cpu().numpy()
    (t64, l64), (t80, l80) = oracle_mstep(rows_host, THETA), oracle_mstep(rows_host, THETA, np.longdouble)
    exc = rule_excess(theta.cpu().numpy(), t64, t80), rule_excess(trace[1:2].cpu().numpy(), [l64], [l80])
    print(f"theta {exc[0]:.3g}, loglik {exc[1]:.3g} of the bound")
    assert max(exc) <= 1.0
    assert torch.isnan(trace[0]) and torch.isnan(trace[2])
    theta2, trace2 = dev_theta(THETA), torch.zeros(3, dtype=torch.float64, device=DEV)
    smooth_mstep(rows, theta2, trace2, 1)
    assert torch.equal(theta2, theta) and torch.equal(trace2[1], trace[1])


# ---- EM ---------------------------------------------------------------------------------------------------------------
def test_fit_follows_the_oracle_and_converges():
    p_host, z = synthetic_chain(40, 500, seed=0)
    p = torch.from_numpy(p_host).to(DEV)
    th64, tr64 = oracle_em(p_host, PRIOR, (0.5, 0.5, 0.5), 25)
    th80, tr80 = oracle_em(p_host, PRIOR, (0.5, 0.5, 0.5), 25, np.longdouble)
    fit = smooth_fit(p, PRIOR, num_iter=25, tol=0.0, chunk=10)  # chunks of 10, 10 and 5
    assert fit["iterations"] == 25 and fit["trace"].shape == (25,) and not fit["converged"]
    exc = rule_excess(fit["theta"].cpu().numpy(), th64[25], th80[25]), rule_excess(fit["trace"].cpu().numpy(), tr64, tr80)
    print(f"theta after 25 iterations {exc[0]:.3g}, trace {exc[1]:.3g} of the bound")
    assert max(exc) <= 1.0
    check_rule(to_numpy({k: fit[k] for k in ("filt", "gamma", "rows")}), oracle_estep(p_host, th80[25], PRIOR),
               oracle_estep(p_host, th80[25], PRIOR, np.longdouble), "final E-step")
    whole = smooth_fit(p, PRIOR, num_iter=25, tol=0.0, chunk=25)
    assert torch.equal(whole["theta"], fit["theta"]) and torch.equal(whole["trace"], fit["trace"])

    fit = smooth_fit(p, PRIOR)
    assert fit["converged"] and fit["iterations"] <= 200 and fit["iterations"] % 50 == 0
    trace = fit["trace"].cpu().numpy()
    assert (np.diff(trace) >= -1e-9 * np.abs(trace[1:])).all()
    kon, koff = realised_rates(z)
    got = fit["theta"].tolist()
    print(f"EM kon {got[0]:.5f} koff {got[1]:.5f} after {fit['iterations']} iterations; realised {kon:.5f} {koff:.5f}")
    assert abs(got[0] / kon - 1) < 0.10 and abs(got[1] / koff - 1) < 0.10


# ---- Viterbi and the backward sampler ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def path_case():
    """N = 37, F = 203, generator seed 3, rows 0-2 special; kon 0.05, koff 0.1, pi0 = 1/3; with the device's E-step."""
    p = synthetic_chain(37, 203, seed=3)[0]
    p[:3] = with_special_rows(p[:3], PRIOR)
    theta = (0.05, 0.10, PRIOR)
    path, margin = oracle_viterbi(p, theta, PRIOR)
    estep = smooth_estep(torch.from_numpy(p).to(DEV), dev_theta(theta), PRIOR)
    return {"p": p, "theta": theta, "path": path, "margin": margin, "estep": estep}


def test_viterbi_path_is_the_oracles(path_case):
    assert path_case["margin"] > 1e-9
    path = smooth_viterbi(torch.from_numpy(path_case["p"]).to(DEV), dev_theta(path_case["theta"]), PRIOR)
    assert path.dtype == torch.uint8 and path.shape == (37, 203)
    assert np.array_equal(path.cpu().numpy(), path_case["path"])


def test_sampler_replay_is_exact(hk, path_case):
    S, F, theta = 71, 203, path_case["theta"]
    filt = path_case["estep"]["filt"]
    want, want_raster, margin = host_count(hk, filt.cpu().numpy(), theta, S, seed=0)
    print(f"smallest |u - q| of the replay: {margin:.3g}")
    assert margin > 1e-9
    counts, raster = smooth_sample(filt, dev_theta(theta), S, seed=0, raster=True)
    assert counts.shape == (S, 37, 4) and counts.dtype == torch.int32 and counts.is_contiguous()
    assert raster.shape == (S, 37, F) and raster.dtype == torch.uint8
    assert np.array_equal(counts.cpu().numpy(), want)
    assert np.array_equal(raster.cpu().numpy(), want_raster)
    assert np.array_equal(oracle_counts(raster.cpu().numpy()), want)
    assert torch.equal(smooth_sample(filt, dev_theta(theta), S, seed=0), counts)  # without the raster
    est = rates_estimate(counts)  # the rows are those of tq_rates_count: the estimate launch takes them unchanged
    assert np.array_equal(est["totals"].cpu().numpy(), want.astype(np.int64).sum(1))


def test_sampler_draws_the_smoothed_law():
    """S = 4096, N = 9, F = 65: raster means within 5 sigma of gamma (sigma^2 = gamma (1 - gamma) / S) and mean counts
    within 5 sigma of the E-step's expectations (sigma from the sample)."""
    S, N, F = 4096, 9, 65
    p = with_special_rows(synthetic_chain(N, F, seed=9)[0], PRIOR)
    e = smooth_estep(torch.from_numpy(p).to(DEV), dev_theta(THETA), PRIOR)
    counts, raster = smooth_sample(e["filt"], dev_theta(THETA), S, seed=5, raster=True)
    gamma = e["gamma"].cpu().numpy()
    sigma = np.sqrt(gamma * (1 - gamma) / S)
    dev = np.abs(raster.double().mean(0).cpu().numpy() - gamma) / np.maximum(sigma, 1e-4)
    print(f"largest deviation of the raster mean: {dev.max():.2f} sigma")
    assert dev.max() < 5.0
    counts = counts.double().cpu().numpy()
    dev = np.abs(counts.mean(0) - e["rows"][:, :4].cpu().numpy()) / np.maximum(counts.std(0) / np.sqrt(S), 1e-3)
    print(f"largest deviation of the mean counts: {dev.max():.2f} sigma")
    assert dev.max() < 5.0


# S = 1; a second, partly filled block of samples; N = 1; N beyond 64; F = 1, 2 and the 64-frame staging boundary
EDGES = [(1, 5, 1), (65, 3, 2), (7, 1, 64), (3, 4, 65), (2, 131, 5), (65, 131, 64), (1, 1, 65)]


@pytest.mark.parametrize("S,N,F", EDGES)
def test_edge_shapes(hk, S, N, F):
    p = synthetic_chain(N, F, seed=S * 1000 + N * 100 + F)[0]
    theta = dev_theta(THETA)
    e = smooth_estep(torch.from_numpy(p).to(DEV), theta, PRIOR)
    o64, o80 = oracle_estep(p, THETA, PRIOR), oracle_estep(p, THETA, PRIOR, np.longdouble)
    check_rule(to_numpy(e), o64, o80, f"N = {N}, F = {F}")
    path, margin = oracle_viterbi(p, THETA, PRIOR)
    assert margin > 1e-9
    assert np.array_equal(smooth_viterbi(torch.from_numpy(p).to(DEV), theta, PRIOR).cpu().numpy(), path)
    seed = 2**40 + F
    want, want_raster, margin = host_count(hk, e["filt"].cpu().numpy(), THETA, S, seed)
    assert margin > 1e-9
    counts, raster = smooth_sample(e["filt"], theta, S, seed=seed, raster=True)
    assert np.array_equal(counts.cpu().numpy(), want) and np.array_equal(raster.cpu().numpy(), want_raster)
    assert (want[..., 1] + want[..., 3] == F - 1).all()


# ---- command line -------------------------------------------------------------------------------------------------
def test_fit_then_smooth_end_to_end(tmp_path):
    runner = CliRunner()
    N, F = 8, 40
    params = {k: v for k, v in TEST_PARAMS.items() if k != "pi"}
    params.update(kon=0.1, koff=0.2)
    save(simulate(2, N, F, 1, 14, params=params), tmp_path)
    result = runner.invoke(app, ["--cd", str(tmp_path), "fit", "--model", "cosmos", "--nbatch-size", "8", "--fbatch-size",
                                 "40", "--num-iter", "2", "--cuda", "--no-input"])
    assert result.exit_code == 0, result.output
    payload = load_tpqr(tmp_path / "data.tpqr")
    payload["mask"][1] = False  # one on-target AOI outside the mask: it keeps its raw values
    torch.save(payload, tmp_path / "data.tpqr")
    result = runner.invoke(app, ["--cd", str(tmp_path), "smooth", "--num-samples", "50", "--num-iter", "30", "--cuda",
                                 "--no-input"])
    assert result.exit_code == 0, result.output
    res = pd.read_csv(tmp_path / "cosmos_smooth-channel0.csv", index_col=0)
    assert list(res.index) == ["kon", "koff"]
    assert list(res.columns) == ["EM", "Mean", "95% LL", "95% UL", "MAP"]
    assert ((res["EM"] > 0) & (res["EM"] < 1)).all()
    out = torch.load(tmp_path / "cosmos_smooth.tpqr")
    assert set(out) == {"z_probs", "z_map", "log_evidence", "theta", "prior", "loglik_trace", "mask"}
    Non = N // 2  # simulate: the first half of the AOIs are on target
    mask = out["mask"]
    assert mask.dtype == torch.bool and mask.tolist() == [True, False, True, True]
    assert out["z_probs"].shape == (Non, F, 1) and out["z_probs"].dtype == torch.float32
    assert out["z_map"].shape == (Non, F, 1) and out["z_map"].dtype == torch.bool
    assert out["log_evidence"].shape == (Non, 1) and out["log_evidence"].dtype == torch.float64
    assert out["theta"].shape == (1, 3) and out["theta"].dtype == torch.float64 and out["prior"].shape == (1,)
    assert bool(((out["z_probs"] >= 0) & (out["z_probs"] <= 1)).all())
    assert torch.isnan(out["log_evidence"][~mask]).all() and torch.isfinite(out["log_evidence"][mask]).all()
    raw = load_tpqr(tmp_path / "cosmos_params.tpqr")["z_probs"][:Non, :, :, 1].float()
    assert torch.equal(out["z_probs"][1], raw[1]) and torch.equal(out["z_map"][1], raw[1] > 0.5)
    assert not torch.equal(out["z_probs"][mask], raw[mask])
    assert np.allclose(res["EM"].to_numpy(), out["theta"][0, :2].numpy(), rtol=1e-12, atol=0)
    assert 0.0 < float(out["prior"][0]) < 1.0
    trace = out["loglik_trace"][0].numpy()
    assert len(out["loglik_trace"]) == 1 and 1 <= len(trace) <= 30
    assert (np.diff(trace) >= -1e-9 * np.abs(trace[1:])).all()
