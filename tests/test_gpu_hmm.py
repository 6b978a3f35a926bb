"""Multi-state hidden-Markov smoothing kernels on the MI355X: the E-step, the M-step and the EM
against the numpy oracle of hmm_fixture by the tolerance rule of section 20, the anchors against the device's own two-state
E-step and against the two-state oracle on lumpable chains, the Viterbi path exactly, the backward sampler bit-equal to the
g++ replay fed the device's own ``filt`` (under a margin condition on its draws) and within 5 sigma of the smoothed law,
the estimate against numpy, and ``fit``, ``smooth``, ``smooth --bound-states 2`` end to end."""

import re

import numpy as np
import pandas as pd
import pytest
import torch
from typer.testing import CliRunner

import smooth_fixture as two
from hmm_fixture import (F_LIST, PRIOR, UB_LIST, build_hmm_check, cols, default_start, fixed_theta, host_count,
                         oracle_em, oracle_estep, oracle_estimate, oracle_mstep, oracle_viterbi, pack, rule_excess,
                         state_pair_counts, synthetic_hmm, with_special_rows)
from rates_fixture import build_rates_check, host_indices, oracle_counts
from tapqir_amd.main import app
from tapqir_amd.utils.dataset import save
from tapqir_amd.utils.mle_analysis import (hmm_estep, hmm_estimate, hmm_fit, hmm_mstep, hmm_sample, hmm_summary, hmm_viterbi,
                                           rates_estimate, smooth_estep)
from tapqir_amd.utils.simulate import TEST_PARAMS, simulate
from test_hmm_host import (LUMPABLE, check_rule, compare_with_two_state, two_state_bounds, viterbi_case)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def hk(tmp_path_factory):
    return build_hmm_check(tmp_path_factory.mktemp("hmm"))


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def to_numpy(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


# ---- E-step -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("U,B", UB_LIST)
@pytest.mark.parametrize("N,F", [(6, F) for F in F_LIST] + [(2, 5000)])
def test_estep_equals_the_oracle(U, B, N, F):
    """The inputs of the host test: rows of all 0, all 1, alternating 0 / 1 and p = prior first (as many as N allows)."""
    M = U + B
    theta = fixed_theta(U, B)
    p = with_special_rows(synthetic_hmm(N, F, seed=F)[0], PRIOR)
    o64, o80 = oracle_estep(p, theta, U, B, PRIOR), oracle_estep(p, theta, U, B, PRIOR, np.longdouble)
    out = hmm_estep(dev(p), dev(theta), PRIOR, U, B)
    got = to_numpy(out)
    assert got["filt"].shape == (N, F, M) and got["gamma"].shape == (N, F, M) and got["rows"].shape == (N, cols(M))
    check_rule(got, o64, o80, M, f"({U}, {B}) N = {N}, F = {F}")
    assert np.allclose(got["rows"][:, : M * M].sum(1), F - 1, rtol=0, atol=1e-9 * F)
    assert np.abs(got["gamma"].sum(-1) - 1).max() < 1e-14
    if F == 1:
        assert not got["rows"][:, : M * M].any()
    again = hmm_estep(dev(p), dev(theta), PRIOR, U, B)
    for key in out:
        assert torch.equal(out[key], again[key]), key  # bit-identical: no atomics, a fixed order of additions


@pytest.mark.parametrize("F", [1, 65, 203])
def test_anchor_two_states_agree_with_the_two_state_kernel(F):
    """(a): tq_hmm_estep at (1, 1) against tq_smooth_estep on the same device."""
    kon, koff, pi0 = 0.05, 0.10, 0.4
    theta = pack([[1 - kon, kon], [koff, 1 - koff]], [1 - pi0, pi0])
    p = with_special_rows(two.synthetic_chain(6, F, seed=F)[0], PRIOR)
    got = to_numpy(hmm_estep(dev(p), dev(theta), PRIOR, 1, 1))
    ref = to_numpy(smooth_estep(dev(p), dev(np.array([kon, koff, pi0])), PRIOR))
    bounds, _ = two_state_bounds(p, (kon, koff, pi0), oracle_estep(p, theta, 1, 1, PRIOR),
                                 oracle_estep(p, theta, 1, 1, PRIOR, np.longdouble), 1, 1)
    compare_with_two_state(got, 1, 1, ref, bounds, f"(a) F = {F}")


@pytest.mark.parametrize("U,B", sorted(LUMPABLE))
def test_anchor_lumpable_chain_has_two_state_marginals(U, B):
    """(b): the class view of a lumpable three-state chain against the two-state oracle."""
    theta, theta2 = LUMPABLE[U, B]
    p = with_special_rows(two.synthetic_chain(6, 129, seed=5)[0], PRIOR)
    got = to_numpy(hmm_estep(dev(p), dev(theta), PRIOR, U, B))
    bounds, t80 = two_state_bounds(p, theta2, oracle_estep(p, theta, U, B, PRIOR),
                                   oracle_estep(p, theta, U, B, PRIOR, np.longdouble), U, B)
    compare_with_two_state(got, U, B, t80, bounds, f"(b) ({U}, {B})")


# ---- M-step -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("U,B", [(1, 1), (1, 2), (2, 2)])
def test_mstep_totals(U, B):
    """300 rows, more than the workgroup's 256 threads: theta and the total loglik by the rule, twice the same bits."""
    M = U + B
    theta0 = fixed_theta(U, B)
    p = synthetic_hmm(300, 40, seed=11)[0]
    rows = hmm_estep(dev(p), dev(theta0), PRIOR, U, B)["rows"]
    theta, trace = dev(theta0), torch.full((3,), float("nan"), dtype=torch.float64, device=DEV)
    hmm_mstep(rows, theta, trace, 1, U, B)
    rows_host = rows.cpu().numpy()
    (t64, l64), (t80, l80) = oracle_mstep(rows_host, theta0, U, B), oracle_mstep(rows_host, theta0, U, B, np.longdouble)
    exc = rule_excess(theta.cpu().numpy(), t64, t80), rule_excess(trace[1:2].cpu().numpy(), [l64], [l80])
    print(f"({U}, {B}) theta {exc[0]:.3g}, loglik {exc[1]:.3g} of the bound")
    assert max(exc) <= 1.0
    assert torch.isnan(trace[0]) and torch.isnan(trace[2])
    assert np.abs(theta.cpu().numpy()[: M * M].reshape(M, M).sum(1) - 1).max() <= 4 * np.spacing(1.0)
    theta2, trace2 = dev(theta0), torch.zeros(3, dtype=torch.float64, device=DEV)
    hmm_mstep(rows, theta2, trace2, 1, U, B)
    assert torch.equal(theta2, theta) and torch.equal(trace2[1], trace[1])


# ---- EM ---------------------------------------------------------------------------------------------------------------
def test_fit_follows_the_oracle():
    U, B, M = 1, 2, 3
    p_host = synthetic_hmm(40, 500, seed=0)[0]
    p = dev(p_host)
    th64, tr64 = oracle_em(p_host, PRIOR, default_start(U, B), U, B, 25)
    th80, tr80 = oracle_em(p_host, PRIOR, default_start(U, B), U, B, 25, np.longdouble)
    fit = hmm_fit(p, PRIOR, U, B, num_iter=25, tol=0.0, chunk=10)  # chunks of 10, 10 and 5
    assert fit["iterations"] == 25 and fit["trace"].shape == (25,) and not fit["converged"]
    order = fit["order"]
    assert sorted(order) == [0, 1, 2] and order[0] == 0

    def relabel(theta):
        return np.concatenate([theta[: M * M].reshape(M, M)[np.ix_(order, order)].ravel(), theta[M * M:][order]])

    exc = (rule_excess(fit["theta"].cpu().numpy(), relabel(th64[25]), relabel(th80[25])),
           rule_excess(fit["trace"].cpu().numpy(), tr64, tr80))
    print(f"theta after 25 iterations {exc[0]:.3g}, trace {exc[1]:.3g} of the bound")
    assert max(exc) <= 1.0
    stay = fit["theta"][: M * M].reshape(M, M).diagonal().cpu().numpy()
    assert stay[1] >= stay[2]  # the canonical order: the long-lived bound state first
    final = relabel(th80[25])
    check_rule(to_numpy({k: fit[k] for k in ("filt", "gamma", "rows")}), oracle_estep(p_host, final, U, B, PRIOR),
               oracle_estep(p_host, final, U, B, PRIOR, np.longdouble), M, "final E-step")
    ll = fit["rows"][:, -1].sum().item()
    assert fit["loglik"] == ll and fit["n_params"] == 8 and fit["bic"] == -2 * ll + 8 * np.log(40 * 500)
    whole = hmm_fit(p, PRIOR, U, B, num_iter=25, tol=0.0, chunk=25)
    assert torch.equal(whole["theta"], fit["theta"]) and torch.equal(whole["trace"], fit["trace"])
    assert torch.equal(whole["gamma"], fit["gamma"])
    trace = fit["trace"].cpu().numpy()
    assert (np.diff(trace) >= -1e-12 * np.abs(trace[1:])).all()


def test_bic_chooses_the_number_of_bound_states():
    """Seed 0 (the seed test_hmm_host finds for the oracle): (1, 2) on three-state data, (1, 1) on two-state data."""
    got = {}
    for name, p in (("three", synthetic_hmm(40, 500, seed=0)[0]), ("two", two.synthetic_chain(40, 500, seed=0)[0])):
        for B in (1, 2):
            got[name, B] = hmm_fit(dev(p), PRIOR, 1, B, num_iter=60, tol=0.0, chunk=60)["bic"]
    print(f"BIC: {got}")
    assert got["three", 2] < got["three", 1] and got["two", 1] < got["two", 2]


# ---- Viterbi ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("U,B", [(1, 2), (2, 2)])
def test_viterbi_path_is_the_oracles(U, B):
    case = viterbi_case(U, B)
    path = hmm_viterbi(dev(case["p"]), dev(case["theta"]), PRIOR, U, B)
    assert path.dtype == torch.uint8 and path.shape == (37, 203)
    assert np.array_equal(path.cpu().numpy(), case["path"])
    for F in (1, 4, 5, 8, 9):
        p = synthetic_hmm(5, F, seed=F)[0]
        want, margin = oracle_viterbi(p, case["theta"], U, B, PRIOR)
        assert margin > 1e-9
        assert np.array_equal(hmm_viterbi(dev(p), dev(case["theta"]), PRIOR, U, B).cpu().numpy(), want), F


# ---- backward sampler ---------------------------------------------------------------------------------------------------
def check_replay(hk, p, theta, U, B, S, seed):
    M = U + B
    N, F = p.shape
    filt = hmm_estep(dev(p), dev(theta), PRIOR, U, B)["filt"]
    want_counts, want_trans, want_raster, margin = host_count(hk, filt.cpu().numpy(), theta, U, B, S, seed)
    print(f"({U}, {B}) S = {S}, N = {N}, F = {F}, seed {seed}: smallest |u - t| of the replay {margin:.3g}")
    assert margin > 1e-9
    out = hmm_sample(filt, dev(theta), U, B, S, seed=seed, trans=True, raster=True)
    assert out["counts"].shape == (S, N, 4) and out["counts"].dtype == torch.int32
    assert out["trans"].shape == (S, N, M * M) and out["trans"].dtype == torch.int32
    assert out["raster"].shape == (S, N, F) and out["raster"].dtype == torch.uint8
    raster = out["raster"].cpu().numpy()
    assert np.array_equal(raster, want_raster)
    assert np.array_equal(out["counts"].cpu().numpy(), want_counts) and np.array_equal(out["trans"].cpu().numpy(), want_trans)
    assert np.array_equal(oracle_counts(raster >= U), want_counts) and np.array_equal(state_pair_counts(raster, M), want_trans)
    again = hmm_sample(filt, dev(theta), U, B, S, seed=seed, trans=True, raster=True)
    assert all(torch.equal(out[k], again[k]) for k in out)
    bare = hmm_sample(filt, dev(theta), U, B, S, seed=seed)  # without the optional outputs
    assert sorted(bare) == ["counts"] and torch.equal(bare["counts"], out["counts"])
    return out


@pytest.mark.parametrize("U,B", [(1, 2), (2, 2)])
@pytest.mark.parametrize("F", [1, 2, 63, 64, 65, 129])
def test_sampler_replay_is_exact(hk, U, B, F):
    """N = 6 with the special rows; S = 1, one full block of samples, one more, and a third, partly filled block."""
    p = with_special_rows(synthetic_hmm(6, F, seed=F)[0], PRIOR)
    for S in (1, 64, 65, 130):
        check_replay(hk, p, fixed_theta(U, B), U, B, S, seed=2**40 + F)


def test_sampler_replay_of_many_rows(hk):
    """N = 37, F = 203, S = 3 at (1, 3); the class counts go through tq_rates_estimate unchanged."""
    p = synthetic_hmm(37, 203, seed=3)[0]
    out = check_replay(hk, p, fixed_theta(1, 3), 1, 3, 3, seed=0)
    est = rates_estimate(out["counts"])
    assert np.array_equal(est["totals"].cpu().numpy(), out["counts"].cpu().numpy().astype(np.int64).sum(1))


def test_sampler_draws_the_smoothed_law():
    """S = 4096, N = 4, F = 129 at (1, 2), seed 0 (the seed of the host test): state frequencies within 5 sigma of gamma and
    mean pair counts within 5 sigma of the E-step's expectations."""
    S, N, F, U, B, M = 4096, 4, 129, 1, 2, 3
    theta = fixed_theta(U, B)
    p = with_special_rows(synthetic_hmm(N, F, seed=9)[0], PRIOR)
    e = hmm_estep(dev(p), dev(theta), PRIOR, U, B)
    out = hmm_sample(e["filt"], dev(theta), U, B, S, seed=0, trans=True, raster=True)
    gamma, raster = e["gamma"].cpu().numpy(), out["raster"].cpu().numpy()
    freq = np.stack([(raster == i).mean(0) for i in range(M)], -1)
    dev1 = np.abs(freq - gamma) / np.maximum(np.sqrt(gamma * (1 - gamma) / S), 1e-4)
    pairs = out["trans"].double().cpu().numpy()
    dev2 = np.abs(pairs.mean(0) - e["rows"][:, : M * M].cpu().numpy()) / np.maximum(pairs.std(0) / np.sqrt(S), 1e-3)
    print(f"state frequencies within {dev1.max():.2f} sigma, mean pair counts within {dev2.max():.2f} sigma")
    assert dev1.max() < 5.0 and dev2.max() < 5.0


# ---- estimate -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("U,B", [(1, 1), (1, 2), (2, 2)])
def test_estimate_sums_and_quotients(tmp_path_factory, U, B):
    M = U + B
    rng = np.random.default_rng(M)
    S, N = 5, 70  # more AOIs than lanes
    trans = rng.integers(0, 50, (S, N, M * M)).astype(np.int32)
    trans[2].reshape(N, M, M)[:, 1] = 0  # sample 2 never visits state 1
    est = hmm_estimate(dev(trans))
    want_totals, want = oracle_estimate(trans, M)
    assert est["A"].shape == (S, M, M) and est["totals"].dtype == torch.int64
    assert np.array_equal(est["totals"].cpu().numpy().reshape(S, -1), want_totals)
    assert np.array_equal(est["A"].cpu().numpy().reshape(S, -1), want, equal_nan=True)
    assert torch.isnan(est["A"][2, 1]).all()
    idx = host_indices(build_rates_check(tmp_path_factory.mktemp("rates")), 11, S, N)
    est = hmm_estimate(dev(trans), bootstrap=True, seed=11)
    want_totals, want = oracle_estimate(trans, M, idx)
    assert np.array_equal(est["totals"].cpu().numpy().reshape(S, -1), want_totals)
    assert np.array_equal(est["A"].cpu().numpy().reshape(S, -1), want, equal_nan=True)
    summary = hmm_summary(est, 0.68)
    assert len(summary) == M * M and summary["A11"]["left_out"] == 1


# ---- command line -------------------------------------------------------------------------------------------------
def test_fit_then_smooth_then_multistate_smooth(tmp_path):
    runner = CliRunner()
    N, F = 8, 40
    params = {k: v for k, v in TEST_PARAMS.items() if k != "pi"}
    params.update(kon=0.1, koff=0.2)
    save(simulate(2, N, F, 1, 14, params=params), tmp_path)
    result = runner.invoke(app, ["--cd", str(tmp_path), "fit", "--model", "cosmos", "--nbatch-size", "8", "--fbatch-size",
                                 "40", "--num-iter", "2", "--cuda", "--no-input"])
    assert result.exit_code == 0, result.output
    common = ["--num-samples", "50", "--num-iter", "30", "--cuda", "--no-input"]
    result = runner.invoke(app, ["--cd", str(tmp_path), "smooth", *common])
    assert result.exit_code == 0, result.output
    plain = {name: (tmp_path / name).read_bytes() for name in ("cosmos_smooth.tpqr", "cosmos_smooth-channel0.csv")}
    result = runner.invoke(app, ["--cd", str(tmp_path), "smooth", "--bound-states", "2", *common])
    assert result.exit_code == 0, result.output
    for name, content in plain.items():
        assert (tmp_path / name).read_bytes() == content, name
    again = runner.invoke(app, ["--cd", str(tmp_path), "smooth", *common])  # and the two-state run writes the same bits
    assert again.exit_code == 0 and all((tmp_path / name).read_bytes() == content for name, content in plain.items())

    Non, M = N // 2, 3
    out = torch.load(tmp_path / "cosmos_smooth-u1b2.tpqr")
    assert set(out) == {"z_probs", "state_probs", "z_map", "state_map", "log_evidence", "theta", "prior", "bic", "n_params",
                        "loglik_trace", "mask", "unbound", "bound"}
    assert out["z_probs"].shape == (Non, F, 1) and out["z_probs"].dtype == torch.float32
    assert out["state_probs"].shape == (Non, F, 1, M) and out["state_probs"].dtype == torch.float32
    assert out["z_map"].shape == (Non, F, 1) and out["z_map"].dtype == torch.bool
    assert out["state_map"].shape == (Non, F, 1) and out["state_map"].dtype == torch.uint8
    assert out["log_evidence"].shape == (Non, 1) and out["theta"].shape == (1, M * M + M) and out["prior"].shape == (1,)
    assert (out["unbound"], out["bound"], out["n_params"]) == (1, 2, 8)
    A = out["theta"][0, : M * M].reshape(M, M)
    assert torch.allclose(A.sum(1), torch.ones(M, dtype=torch.float64), rtol=0, atol=1e-15) and bool((A > 0).all())
    assert A[1, 1] >= A[2, 2]
    assert bool(((out["z_probs"] >= 0) & (out["z_probs"] <= 1)).all())
    assert torch.allclose(out["state_probs"][..., 1:].sum(-1), out["z_probs"], atol=1e-6)
    assert torch.equal(out["state_map"] >= 1, out["z_map"]) and int(out["state_map"].max()) < M
    assert out["bic"].shape == (1,) and bool(torch.isfinite(out["bic"]).all())
    logged = float(re.search(r"BIC = (\S+)", (tmp_path / ".tapqir" / "loginfo").read_text()).group(1))
    assert np.isfinite(logged) and abs(logged - out["bic"][0].item()) < 1e-5
    trace = out["loglik_trace"][0].numpy()
    assert (np.diff(trace) >= -1e-9 * np.abs(trace[1:])).all()
    res = pd.read_csv(tmp_path / "cosmos_smooth-u1b2-channel0.csv", index_col=0)
    assert list(res.index) == [f"A{i}{j}" for i in range(M) for j in range(M)] + ["dwell0", "dwell1", "dwell2", "kon", "koff"]
    assert list(res.columns) == ["EM", "Mean", "95% LL", "95% UL", "MAP"]
    assert np.allclose(res["EM"].to_numpy()[: M * M], A.numpy().ravel(), rtol=1e-12, atol=0)
    assert np.allclose(res.loc["dwell1", "EM"], 1 / (1 - A[1, 1].item()), rtol=1e-12)
    assert 0 < res.loc["kon", "EM"] < 1 and 0 < res.loc["koff", "EM"] < 1
