"""Two colour channels as one chain on the MI355X: ``tq_joint_estep``, ``tq_joint_mstep`` and
``tq_joint_viterbi`` against the numpy oracle of joint_fixture by the tolerance rule of section 20 on the inputs of the host
test, the Kronecker anchor against the two-state oracle and against ``smooth_estep`` of the same device, the channel swap,
the EM and the choice of a structure by BIC through ``joint_fit``, the unchanged sampler on the joint ``filt``, and ``fit``,
``smooth``, ``smooth --joint`` end to end."""

import re

import numpy as np
import pandas as pd
import pytest
import torch
from typer.testing import CliRunner

from helpers import make_dataset
from joint_fixture import (A_DRIVEN, COLS, F_LIST, M, N_PARAMS, NAMES, PRIORS, SWAP, default_start, em_case, estep_inputs,
                           fixed_theta, hand_rates, oracle_estep, oracle_mstep, oracle_viterbi, realised_matrix, rule_excess,
                           selection_case, start_from, swap_rows, swap_theta, synthetic_joint)
from tapqir_amd.main import app
from tapqir_amd.utils.dataset import save
from tapqir_amd.utils.joint_analysis import (RATE_NAMES, RATIO_NAMES, joint_default_start, joint_estep, joint_fit, joint_mstep,
                                             joint_rates, joint_start_from, joint_viterbi)
from tapqir_amd.utils.mle_analysis import hmm_mstep, hmm_sample, multistart_mstep, smooth_estep
from test_joint_host import (VITERBI_SEEDS, WANT, check_kronecker, check_ladder, check_rule, check_structure_identities,
                             mstep_case)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def estep(pa, pb, thetas, priors=PRIORS, **kw):
    return joint_estep(dev(pa), dev(pb), dev(np.atleast_2d(thetas)), priors[0], priors[1], **kw)


def replica(out, r):
    return {k: v[r].cpu().numpy() for k, v in out.items()}


# ---- E-step -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,F", [(6, F) for F in F_LIST] + [(2, 5000)])
def test_estep_equals_the_oracle(N, F):
    """The inputs of the host test."""
    theta = fixed_theta()
    pa, pb = estep_inputs(N, F, seed=F)
    o64, o80 = oracle_estep(pa, pb, theta), oracle_estep(pa, pb, theta, dtype=np.longdouble)
    out = estep(pa, pb, theta, gamma=True)
    got = replica(out, 0)
    check_rule(got, o64, o80, f"N = {N}, F = {F}")
    assert np.allclose(got["rows"][:, :16].sum(1), F - 1, rtol=0, atol=1e-9 * F)
    assert np.abs(got["gamma"].sum(-1) - 1).max() < 1e-14 and np.abs(got["filt"].sum(-1) - 1).max() < 1e-14
    if F == 1:
        assert not got["rows"][:, :16].any()
    again = estep(pa, pb, theta, gamma=True)  # no atomics, a fixed order of additions
    assert all(torch.equal(again[k], out[k]) for k in out)


@pytest.mark.parametrize("F", [1, 65, 203])
def test_estep_replicas_inactive_and_without_gamma(F):
    """R = 3 with the middle replica inactive: its outputs keep the NaN sentinel, the outer two have the bits of their own
    R = 1 runs; without gamma the rows have the same bits."""
    thetas = np.array([fixed_theta(seed=r) for r in range(3)])
    pa, pb = estep_inputs(6, F, seed=F)
    nan = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float64, device=DEV)  # noqa: E731
    active = torch.tensor([1, 0, 1], dtype=torch.int32, device=DEV)
    got = estep(pa, pb, thetas, active=active, gamma=nan(3, 6, F, M), rows=nan(3, 6, COLS), filt=nan(3, 6, F, M))
    assert set(got) == {"rows", "filt", "gamma"} and all(bool(torch.isnan(got[k][1]).all()) for k in got)
    for r in (0, 2):
        alone = estep(pa, pb, thetas[r], gamma=True)
        assert all(torch.equal(alone[k][0], got[k][r]) for k in got), r
    bare, full = estep(pa, pb, thetas), estep(pa, pb, thetas, gamma=True)
    assert "gamma" not in bare and torch.equal(bare["rows"], full["rows"]) and torch.equal(bare["filt"], full["filt"])


# ---- anchors ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [1, 65, 203])
def test_anchor_kronecker_start_is_two_independent_chains(F):
    """Against the two-state long-double oracles, and against ``smooth_estep`` of this device."""
    theta_a, theta_b, priors = (0.05, 0.10, 0.4), (0.03, 0.20, 0.25), (1.0 / 3.0, 0.2)
    pa, pb = estep_inputs(6, F, seed=F)
    theta = joint_start_from(theta_a, theta_b).numpy()
    assert np.allclose(theta, start_from(theta_a, theta_b), rtol=0, atol=1e-16)
    got = replica(estep(pa, pb, theta, priors, gamma=True), 0)
    check_kronecker(got, pa, pb, theta_a, theta_b, priors, f"F = {F}, oracle")
    refs = [{k: v.cpu().numpy() for k, v in smooth_estep(dev(p), dev(np.array(t)), pr).items()}
            for p, t, pr in ((pa, theta_a, priors[0]), (pb, theta_b, priors[1]))]
    check_kronecker(got, pa, pb, theta_a, theta_b, priors, f"F = {F}, smooth_estep", refs)


@pytest.mark.parametrize("F", [1, 65, 203])
def test_channel_swap_permutes_the_states(F):
    theta, priors = fixed_theta(seed=1), (1.0 / 3.0, 0.2)
    pa, pb = estep_inputs(6, F, seed=F)
    o64, o80 = oracle_estep(pa, pb, theta, priors), oracle_estep(pa, pb, theta, priors, np.longdouble)
    got = replica(estep(pb, pa, swap_theta(theta), priors[::-1], gamma=True), 0)
    back = {"filt": got["filt"][..., SWAP], "gamma": got["gamma"][..., SWAP], "rows": swap_rows(got["rows"])}
    check_rule(back, o64, o80, f"swapped, F = {F}")


# ---- M-step -----------------------------------------------------------------------------------------------------------
def test_mstep_of_the_five_structures():
    """N = 300, all five structures in one launch, R = 5."""
    rows, theta0 = mstep_case()
    d_rows = dev(rows)
    thetas, trace = dev(theta0), torch.full((5, 3), float("nan"), dtype=torch.float64, device=DEV)
    joint_mstep(d_rows, thetas, trace, 1, range(5))
    got, tr = thetas.cpu().numpy(), trace.cpu().numpy()
    for k in range(5):
        (t64, l64), (t80, l80) = oracle_mstep(rows[k], theta0[k], k), oracle_mstep(rows[k], theta0[k], k, np.longdouble)
        exc = rule_excess(got[k], t64, t80), rule_excess([tr[k, 1]], [l64], [l80])
        print(f"{NAMES[k]}: theta {exc[0]:.3g}, loglik {exc[1]:.3g} of the bound")
        assert max(exc) <= 1.0, k
    assert np.isnan(tr[:, [0, 2]]).all()
    check_structure_identities(got)
    # full: the bits of hmm_mstep and of multistart_mstep with every entry allowed, on the same rows
    one, t1 = dev(theta0[4]), torch.zeros(2, dtype=torch.float64, device=DEV)
    hmm_mstep(d_rows[4].contiguous(), one, t1, 1, 2, 2)
    many, t2 = dev(theta0[4:5]), torch.zeros(1, 2, dtype=torch.float64, device=DEV)
    multistart_mstep(d_rows[4:5].contiguous(), many, t2, 1, 2, 2)
    assert torch.equal(thetas[4], one) and torch.equal(thetas[4], many[0]) and trace[4, 1] == t1[1] == t2[0, 1]
    again, trace2 = dev(theta0), torch.zeros(5, 3, dtype=torch.float64, device=DEV)
    joint_mstep(d_rows, again, trace2, 1, range(5))
    assert torch.equal(again, thetas) and torch.equal(trace2[:, 1], trace[:, 1])
    frozen, trace3 = dev(theta0), torch.full((5, 3), float("nan"), dtype=torch.float64, device=DEV)
    joint_mstep(d_rows, frozen, trace3, 1, range(5), torch.tensor([1, 1, 0, 1, 1], dtype=torch.int32, device=DEV))
    assert torch.equal(frozen[2], dev(theta0[2])) and bool(torch.isnan(trace3[2]).all())
    assert torch.equal(frozen[[0, 1, 3, 4]], thetas[[0, 1, 3, 4]])


def test_mstep_keeps_a_row_without_occupancy():
    theta0 = np.array([fixed_theta()] * 5)
    pairs = np.arange(1.0, 17.0).reshape(4, 4)
    pairs[[1, 3]] = 0.0  # z_a = 1 never occupied: every structure keeps the rows of states 1 and 3
    row = np.concatenate([pairs.ravel(), [0.4, 0.3, 0.2, 0.1], [-7.0]])
    rows = dev(np.tile(row, (5, 1, 1)))
    thetas, trace = dev(theta0), torch.zeros(5, 1, dtype=torch.float64, device=DEV)
    joint_mstep(rows, thetas, trace, 0, range(5))
    A, old = thetas.cpu().numpy()[:, :16].reshape(5, 4, 4), theta0[0, :16].reshape(4, 4)
    for k in range(5):
        assert np.array_equal(A[k][[1, 3]], old[[1, 3]]) and not np.array_equal(A[k][0], old[0]), k
        want = oracle_mstep(row[None], theta0[0], k)[0]
        assert np.allclose(thetas[k].cpu().numpy(), want, rtol=1e-14, atol=0)


# ---- EM -----------------------------------------------------------------------------------------------------------------
def test_em_follows_the_oracle_under_every_structure():
    """The driven chain, N = 40, F = 500, seed 0, from the default start: 25 iterations in chunks of 10, 10 and 5."""
    case = em_case()
    pa, pb = dev(case["pa"]), dev(case["pb"])
    fit = joint_fit(pa, pb, *PRIORS, num_iter=25, tol=0.0, chunk=10)
    for k, f in enumerate(fit["fits"]):
        assert (f["structure"], f["name"], f["iterations"], f["n_params"]) == (k, NAMES[k], 25, N_PARAMS[k])
        theta, trace = f["theta"].numpy(), f["trace"].numpy()
        exc = rule_excess(theta, case["th64"][k][25], case["th80"][k][25]), rule_excess(trace, case["tr64"][k], case["tr80"][k])
        print(f"{NAMES[k]}: theta after 25 iterations {exc[0]:.3g}, trace {exc[1]:.3g} of the bound")
        assert max(exc) <= 1.0, k
        assert (np.diff(trace) >= -1e-12 * np.abs(trace[1:])).all(), k
    whole = joint_fit(pa, pb, *PRIORS, num_iter=25, tol=0.0, chunk=25)
    for f, g in zip(fit["fits"], whole["fits"]):
        assert torch.equal(f["theta"], g["theta"]) and torch.equal(f["trace"], g["trace"]) and f["loglik"] == g["loglik"]
    check_structure_identities(np.array([f["theta"].numpy() for f in fit["fits"]]))
    # the outputs of the chosen structure are an E-step at its theta
    k = fit["chosen"]
    assert k == fit["best"] and torch.equal(fit["theta"].cpu(), fit["fits"][k]["theta"])
    e = joint_estep(pa, pb, fit["theta"][None].contiguous(), *PRIORS, gamma=True)
    assert all(torch.equal(e[key][0], fit[key]) for key in ("filt", "gamma", "rows"))
    forced = joint_fit(pa, pb, *PRIORS, num_iter=3, tol=0.0, structures=["full", "independent"], choose="full")
    assert forced["chosen"] == 4 and [f["structure"] for f in forced["fits"]] == [4, 0]
    assert torch.equal(forced["theta"].cpu(), forced["fits"][0]["theta"])


# ---- selection ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("kind", sorted(WANT))
def test_bic_chooses_the_generating_structure(kind, seed):
    """60 iterations from the default start, N = 40, F = 500 (the host test asserts the oracle's margins)."""
    A = np.kron(np.array([[0.96, 0.04], [0.08, 0.92]]), np.array([[0.95, 0.05], [0.10, 0.90]])) if kind == "independent" else A_DRIVEN
    pa, pb, states = synthetic_joint(40, 500, seed, A)
    if kind == "driven-swapped":
        pa, pb = pb, pa
    fit = joint_fit(dev(pa), dev(pb), *PRIORS, start=joint_default_start(), num_iter=60, tol=0.0)
    bics = np.array([f["bic"] for f in fit["fits"]])
    order = np.argsort(bics)
    print(f"{kind} seed {seed}: {NAMES[fit['best']]} chosen, {NAMES[order[1]]} is {bics[order[1]] - bics[order[0]]:.2f} worse")
    assert fit["best"] == WANT[kind] == fit["chosen"]
    check_ladder([f["loglik"] for f in fit["fits"]], "device")
    if kind == "driven" and seed == 0:
        got = joint_rates(fit["theta"][:16].reshape(4, 4).cpu())
        real, true = hand_rates(realised_matrix(states)), hand_rates(A_DRIVEN)
        for name in ("kon_b|a0", "kon_b|a1", "kon_b ratio", "koff_b|a0", "koff_b|a1", "kon_a|b0", "koff_a|b0"):
            print(f"{name}: generating {true[name]:.4g}, realised {real[name]:.4g}, fitted {got[name].item():.4g}")
        assert got["kon_b ratio"].item() > 5.0


# ---- Viterbi ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", sorted(VITERBI_SEEDS))
def test_viterbi_equals_the_oracle(F):
    theta = fixed_theta()
    pa, pb, _ = synthetic_joint(37, F, VITERBI_SEEDS[F], A_DRIVEN)
    want, margin = oracle_viterbi(pa, pb, theta)
    assert margin > 1e-9
    got = joint_viterbi(dev(pa), dev(pb), dev(theta), *PRIORS)
    assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), want)


# ---- the unchanged sampler on the joint filt ------------------------------------------------------------------------------
def test_sampler_draws_the_joint_smoothed_law():
    """S = 4096, N = 4, F = 129: ``hmm_sample`` at (2, 2) on the joint filt has state frequencies within 5 sigma of the joint
    gamma and mean pair counts within 5 sigma of rows[:, :16]."""
    S, N, F = 4096, 4, 129
    theta = fixed_theta()
    pa, pb = estep_inputs(N, F, seed=9)
    e = estep(pa, pb, theta, gamma=True)
    out = hmm_sample(e["filt"][0], dev(theta), 2, 2, S, seed=0, trans=True, raster=True)
    gamma, raster = e["gamma"][0].cpu().numpy(), out["raster"].cpu().numpy()
    freq = np.stack([(raster == i).mean(0) for i in range(M)], -1)
    dev1 = np.abs(freq - gamma) / np.maximum(np.sqrt(gamma * (1 - gamma) / S), 1e-4)
    pairs = out["trans"].double().cpu().numpy()
    dev2 = np.abs(pairs.mean(0) - e["rows"][0, :, :16].cpu().numpy()) / np.maximum(pairs.std(0) / np.sqrt(S), 1e-3)
    print(f"state frequencies within {dev1.max():.2f} sigma, mean pair counts within {dev2.max():.2f} sigma")
    assert dev1.max() < 5.0 and dev2.max() < 5.0


# ---- command line -------------------------------------------------------------------------------------------------
def test_fit_then_smooth_then_joint_smooth(tmp_path):
    runner = CliRunner()
    N, F = 8, 40
    save(make_dataset(N=N, F=F, C=2), tmp_path)
    result = runner.invoke(app, ["--cd", str(tmp_path), "fit", "--model", "cosmos", "--nbatch-size", "8", "--fbatch-size",
                                 "40", "--num-iter", "2", "--cuda", "--no-input"])
    assert result.exit_code == 0, result.output
    common = ["--num-samples", "50", "--num-iter", "30", "--cuda", "--no-input"]
    result = runner.invoke(app, ["--cd", str(tmp_path), "smooth", *common])
    assert result.exit_code == 0, result.output
    names = ("cosmos_smooth.tpqr", "cosmos_smooth-channel0.csv", "cosmos_smooth-channel1.csv")
    plain = {name: (tmp_path / name).read_bytes() for name in names}
    before = {path.name for path in tmp_path.iterdir()}
    log = tmp_path / ".tapqir" / "loginfo"
    mark = len(log.read_text())
    result = runner.invoke(app, ["--cd", str(tmp_path), "smooth", "--joint", "0,1", *common])
    assert result.exit_code == 0, result.output
    for name, content in plain.items():
        assert (tmp_path / name).read_bytes() == content, name
    assert {path.name for path in tmp_path.iterdir()} - before == {"cosmos_smooth-joint01.tpqr", "cosmos_smooth-joint01.csv"}
    logged = log.read_text()[mark:]
    ladder = re.findall(r"structure (\S+): log evidence = (\S+), (\d+) parameters, BIC = (\S+) after", logged)
    assert [row[0] for row in ladder] == list(NAMES) and [int(row[2]) for row in ladder] == list(N_PARAMS)
    chosen = re.search(r"chosen structure: (\S+) \(the lowest BIC\)", logged).group(1)

    out = torch.load(tmp_path / "cosmos_smooth-joint01.tpqr")
    assert set(out) == {"state_probs", "z_probs", "state_map", "z_map", "log_evidence", "theta", "prior", "channels",
                        "structures", "logliks", "bics", "n_params", "chosen", "loglik_trace", "mask"}
    mask = out["mask"]
    Nd = len(mask)
    assert out["state_probs"].shape == (Nd, F, 4) and out["state_probs"].dtype == torch.float32
    assert out["z_probs"].shape == (Nd, F, 2) and out["z_probs"].dtype == torch.float32
    assert out["state_map"].shape == (Nd, F) and out["state_map"].dtype == torch.uint8
    assert out["z_map"].shape == (Nd, F, 2) and out["z_map"].dtype == torch.uint8
    assert out["log_evidence"].shape == (Nd,) and out["log_evidence"].dtype == torch.float64
    assert out["theta"].shape == (20,) and out["theta"].dtype == torch.float64
    assert out["prior"].shape == (2,) and out["channels"] == (0, 1)
    assert out["structures"] == list(NAMES) and out["chosen"] == chosen and chosen in NAMES
    assert out["logliks"].shape == (5,) and out["bics"].shape == (5,) and out["n_params"].tolist() == list(N_PARAMS)
    assert out["chosen"] == NAMES[int(torch.argmin(out["bics"]))]
    assert np.allclose([float(row[1]) for row in ladder], out["logliks"].numpy(), rtol=0, atol=1e-5)
    assert len(out["loglik_trace"]) == 5
    on, off = out["state_probs"][mask], out["state_probs"][~mask]
    assert bool(torch.isnan(off).all()) and bool(torch.isfinite(on).all())
    assert torch.allclose(on.sum(-1), torch.ones(on.shape[:-1]), atol=1e-6)
    marg = torch.stack([on[..., 1] + on[..., 3], on[..., 2] + on[..., 3]], -1)
    assert torch.allclose(out["z_probs"][mask], marg, atol=1e-6) and bool(torch.isnan(out["z_probs"][~mask]).all())
    sm = out["state_map"]
    assert bool((sm[~mask] == 255).all()) and bool((out["z_map"][~mask] == 255).all()) and int(sm[mask].max()) < 4
    assert torch.equal(out["z_map"][mask][..., 0], sm[mask] & 1) and torch.equal(out["z_map"][mask][..., 1], sm[mask] >> 1)
    assert bool(torch.isfinite(out["log_evidence"][mask]).all()) and bool(torch.isnan(out["log_evidence"][~mask]).all())
    assert abs(out["log_evidence"][mask].sum().item() - out["logliks"][NAMES.index(chosen)].item()) < 1e-8

    res = pd.read_csv(tmp_path / "cosmos_smooth-joint01.csv", index_col=0)
    assert list(res.index) == [f"A{i}{j}" for i in range(4) for j in range(4)] + list(RATE_NAMES) + list(RATIO_NAMES)
    assert list(res.columns) == ["EM", "Mean", "95% LL", "95% UL", "MAP"]
    A = out["theta"][:16].reshape(4, 4)
    assert np.allclose(res["EM"].to_numpy()[:16], A.numpy().ravel(), rtol=1e-12, atol=0)
    rates = joint_rates(A)
    assert np.allclose(res["EM"].to_numpy()[16:], [rates[n].item() for n in RATE_NAMES + RATIO_NAMES], rtol=1e-12, atol=0)

    result = runner.invoke(app, ["--cd", str(tmp_path), "smooth", "--joint", "0,1", "--structure", "full", *common])
    assert result.exit_code == 0, result.output
    forced = torch.load(tmp_path / "cosmos_smooth-joint01.tpqr")
    assert forced["chosen"] == "full" and torch.equal(forced["bics"], out["bics"])
    assert "chosen structure: full (forced by --structure)" in log.read_text()
    for name, content in plain.items():
        assert (tmp_path / name).read_bytes() == content, name
    result = runner.invoke(app, ["--cd", str(tmp_path), "smooth", "--joint", "0,2", *common])
    assert result.exit_code == 1 and "the data has 2 channels" in result.output
