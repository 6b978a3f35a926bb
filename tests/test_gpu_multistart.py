"""Several EM starts side by side on the MI355X: the batched E-step and M-step against the numpy
oracle by the tolerance rule of section 20, a replica alone against the same replica in a batch bit for bit, frozen replicas
untouched, ``hmm_fit_restarts`` against the oracle's EM from every start and against ``hmm_fit`` from every start, replicas
frozen where the stopping rule stops them, the best of eight starts where the default start is stuck, and ``fit``,
``smooth``, ``smooth --restarts`` end to end."""

import hashlib

import numpy as np
import pytest
import torch
from typer.testing import CliRunner

from hmm_fixture import fixed_theta, oracle_mstep, with_special_rows
from multistart_fixture import (F_LIST, FREEZE, PRIOR, UB_LIST, best_case, bic, cols, em_case, forbid, oracle_mstep_masked,
                                oracle_stop, rule_excess, synthetic_hmm, threshold_margin)
from tapqir_amd.main import app
from tapqir_amd.utils.dataset import save
from tapqir_amd.utils.mle_analysis import (hmm_fit, hmm_fit_restarts, hmm_permute, multistart_estep, multistart_mstep)
from tapqir_amd.utils.simulate import TEST_PARAMS, simulate
from test_hmm_host import rule_bound
from test_multistart_host import check_rows

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


# ---- batched E-step -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("U,B", UB_LIST)
@pytest.mark.parametrize("F", F_LIST)
def test_batched_estep_equals_the_oracle_and_the_single_replica(U, B, F):
    """The inputs of the host test: R = 3 chains on N = 6 shared rows."""
    M = U + B
    thetas = np.array([fixed_theta(U, B, seed=r) for r in range(3)])
    p = with_special_rows(synthetic_hmm(6, F, seed=F)[0], PRIOR)
    rows = multistart_estep(dev(p), dev(thetas), PRIOR, U, B)
    got = rows.cpu().numpy()
    assert got.shape == (3, 6, cols(M))
    for r in range(3):
        check_rows(got[r], p, thetas[r], U, B, f"({U}, {B}) F = {F} replica {r}")
        alone = multistart_estep(dev(p), dev(thetas[r:r + 1]), PRIOR, U, B)
        assert torch.equal(alone[0], rows[r]), r
    assert torch.equal(multistart_estep(dev(p), dev(thetas), PRIOR, U, B), rows)  # no atomics, a fixed order of additions

    active = torch.tensor([1, 0, 1], dtype=torch.int32, device=DEV)
    frozen = torch.full_like(rows, float("nan"))
    multistart_estep(dev(p), dev(thetas), PRIOR, U, B, active, frozen)
    assert bool(torch.isnan(frozen[1]).all()) and torch.equal(frozen[[0, 2]], rows[[0, 2]])
    new, trace = dev(thetas), torch.full((3, 4), float("nan"), dtype=torch.float64, device=DEV)
    multistart_mstep(rows, new, trace, 2, U, B, None, active)
    assert torch.equal(new[1], dev(thetas[1])) and bool(torch.isnan(trace[1]).all())
    assert bool(torch.isfinite(trace[[0, 2], 2]).all()) and bool(torch.isnan(trace[:, [0, 1, 3]]).all())
    assert not torch.equal(new[0], dev(thetas[0])) and not torch.equal(new[2], dev(thetas[2]))


# ---- batched M-step -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("U,B", [(1, 2), (2, 2)])
def test_batched_mstep_free_and_masked(U, B):
    """N = 300 rows (more than the workgroup's 256 threads), R = 3: the case of the host test."""
    M = U + B
    rng = np.random.default_rng(2)
    rows = rng.random((3, 300, cols(M)))
    rows[:, :, M * M: M * M + M] /= rows[:, :, M * M: M * M + M].sum(2, keepdims=True)
    theta0 = np.array([fixed_theta(U, B, seed=r) for r in range(3)])
    allow = forbid(M, (M - 2, M - 1), (M - 1, M - 2), (0, M - 1))
    for mask, name in ((None, "free"), (allow, "masked")):
        thetas, trace = dev(theta0), torch.full((3, 2), float("nan"), dtype=torch.float64, device=DEV)
        multistart_mstep(dev(rows), thetas, trace, 1, U, B, mask)
        got, ll = thetas.cpu().numpy(), trace.cpu().numpy()
        for r in range(3):
            if mask is None:
                (t64, l64), (t80, l80) = oracle_mstep(rows[r], theta0[r], U, B), oracle_mstep(rows[r], theta0[r], U, B, np.longdouble)
            else:
                t64, l64 = oracle_mstep_masked(rows[r], theta0[r], U, B, mask)
                t80, l80 = oracle_mstep_masked(rows[r], theta0[r], U, B, mask, np.longdouble)
            exc = rule_excess(got[r], t64, t80), rule_excess([ll[r, 1]], [l64], [l80])
            print(f"({U}, {B}) {name} replica {r}: theta {exc[0]:.3g}, loglik {exc[1]:.3g} of the bound")
            assert max(exc) <= 1.0
            A = got[r, : M * M].reshape(M, M)
            assert np.abs(A.sum(1) - 1).max() <= 4 * np.spacing(1.0)
            if mask is not None:
                assert (A[~mask] <= 1e-9).all() and (A[~mask] > 0).all() and (A[mask] > 1e-3).all()
        assert np.isnan(ll[:, 0]).all()
        again, trace2 = dev(theta0), torch.zeros(3, 2, dtype=torch.float64, device=DEV)
        multistart_mstep(dev(rows), again, trace2, 1, U, B, mask)
        assert torch.equal(again, thetas) and torch.equal(trace2[:, 1], trace[:, 1])


# ---- EM -----------------------------------------------------------------------------------------------------------------
def test_fit_restarts_follows_the_oracle_from_every_start():
    """(1, 2), N = 20, F = 300, the default start and 3 random ones, 15 iterations in chunks of 6, 6 and 3, tol = 0."""
    case = em_case()
    fit = hmm_fit_restarts(dev(case["p"]), PRIOR, 1, 2, starts=case["raw"], num_iter=15, tol=0.0, chunk=6)
    assert fit["iterations"] == [15] * 4 and fit["converged"] == [False] * 4 and fit["traces"].shape == (4, 15)
    assert np.array_equal(fit["starts"].numpy(), case["raw"])
    thetas, traces = fit["thetas"].cpu().numpy(), fit["traces"].cpu().numpy()
    for r in range(4):
        exc = (rule_excess(thetas[r], case["th64"][r][15], case["th80"][r][15]),
               rule_excess(traces[r], case["tr64"][r][:15], case["tr80"][r][:15]))
        print(f"start {r}: theta after 15 iterations {exc[0]:.3g}, trace {exc[1]:.3g} of the bound")
        assert max(exc) <= 1.0, r
    best = fit["best"]
    assert best == int(np.argmax(fit["logliks"].numpy())) and fit["trace"].shape == (15,)
    assert torch.equal(fit["trace"], fit["traces"][best])
    assert fit["n_params"] == 8 and fit["bic"] == -2 * fit["loglik"] + 8 * np.log(20 * 300)
    assert abs(fit["loglik"] - fit["logliks"][best].item()) <= 1e-10 * abs(fit["loglik"])
    assert torch.equal(fit["theta"], hmm_permute(fit["order"], 3, theta=fit["thetas"][best])["theta"])


def test_fit_restarts_ends_where_hmm_fit_ends_from_every_start():
    """Every replica against ``hmm_fit`` from its start: the same number of iterations, theta within the sum of the two
    rule bounds.  Whether the bits are equal is printed, not asserted: two kernels may contract differently."""
    case = em_case()
    p = dev(case["p"])
    fit = hmm_fit_restarts(p, PRIOR, 1, 2, starts=case["raw"], num_iter=15, tol=0.0, chunk=6)
    for r in range(4):
        one = hmm_fit(p, PRIOR, 1, 2, A0=case["raw"][r, :9].reshape(3, 3), rho0=case["raw"][r, 9:], num_iter=15, tol=0.0, chunk=6)
        assert one["iterations"] == fit["iterations"][r]
        mine = hmm_permute(one["order"], 3, theta=fit["thetas"][r])["theta"]
        bound = 2 * rule_bound(case["th64"][r][15], case["th80"][r][15])
        err = float((mine - one["theta"]).abs().max())
        print(f"start {r}: |theta - hmm_fit's| = {err:.3g}, bound {bound:.3g}, equal bits: {torch.equal(mine, one['theta'])}, "
              f"traces equal bits: {torch.equal(fit['traces'][r], one['trace'])}")
        assert err <= bound, r


def test_replicas_freeze_where_the_rule_stops_them():
    """The freezing case of the host test: stops after 16, 24, 32 and 40 iterations in the float64 oracle."""
    case = em_case()
    p = dev(case["p"])
    tol, num_iter, chunk = FREEZE["tol"], FREEZE["num_iter"], FREEZE["chunk"]
    want = [oracle_stop(case["tr64"][r], tol, num_iter, chunk) for r in range(4)]
    assert min(threshold_margin(case["tr64"][r], tol) for r in range(4)) > 1e-3 and len({w[0] for w in want}) >= 2
    fit = hmm_fit_restarts(p, PRIOR, 1, 2, starts=case["raw"], num_iter=num_iter, tol=tol, chunk=chunk)
    assert fit["iterations"] == [w[0] for w in want] and fit["converged"] == [w[1] for w in want]
    for r in range(4):
        stop = fit["iterations"][r]
        short = hmm_fit_restarts(p, PRIOR, 1, 2, starts=case["raw"], num_iter=stop, tol=0.0, chunk=chunk)
        assert torch.equal(short["thetas"][r], fit["thetas"][r]), r
        assert torch.equal(short["traces"][r], fit["traces"][r, :stop]) and bool(torch.isnan(fit["traces"][r, stop:]).all())
        assert short["logliks"][r] == fit["logliks"][r]


def test_the_best_start_beats_the_default_start():
    """(2, 2) on N = 30, F = 400, restarts = 7, seed = 7, 120 iterations, tol = 0, through ``hmm_fit_restarts``."""
    case = best_case()
    fit = hmm_fit_restarts(dev(case["p"]), PRIOR, 2, 2, restarts=7, seed=7, num_iter=120, tol=0.0)
    ll = fit["logliks"].numpy()
    print("log evidence by start:", np.array2string(ll, precision=3), "best", fit["best"])
    assert np.array_equal(fit["starts"].numpy(), case["raw"]) and ll.shape == (8,)
    assert fit["best"] != 0 and fit["best"] == int(np.argmax(ll)) and ll[fit["best"]] - ll[0] >= 2.0
    exc = rule_excess([ll[0]], [case["ll64"]], [case["ll80"]])
    print(f"default start's log evidence {ll[0]:.6f}: {exc:.3g} of the bound")
    assert exc <= 1.0
    assert fit["n_params"] == 15 and fit["bic"] == -2 * fit["loglik"] + 15 * np.log(30 * 400)
    assert fit["bic"] < bic(ll[0], 15, 30, 400) and bool(fit["allow"].all())
    stay = fit["theta"][:16].reshape(4, 4).diagonal().cpu().numpy()
    assert stay[0] >= stay[1] and stay[2] >= stay[3]  # the canonical order


# ---- command line -----------------------------------------------------------------------------------------------------
def test_fit_then_smooth_then_smooth_with_restarts(tmp_path):
    runner = CliRunner()
    N, F = 8, 40
    params = {k: v for k, v in TEST_PARAMS.items() if k != "pi"}
    params.update(kon=0.1, koff=0.2)
    save(simulate(2, N, F, 1, 14, params=params), tmp_path)

    def hashes(*names):
        return {name: hashlib.sha256((tmp_path / name).read_bytes()).hexdigest() for name in names}

    def run(*flags):
        result = runner.invoke(app, ["--cd", str(tmp_path), *flags, "--cuda", "--no-input"])
        assert result.exit_code == 0, result.output

    smooth = ["--num-samples", "50", "--num-iter", "30"]
    two_names = ("cosmos_smooth.tpqr", "cosmos_smooth-channel0.csv")
    run("fit", "--model", "cosmos", "--nbatch-size", "8", "--fbatch-size", "40", "--num-iter", "2")
    run("smooth", *smooth)  # the two-state files, which no later step may touch
    two = hashes(*two_names)
    run("smooth", "--bound-states", "2", *smooth)
    three = hashes("cosmos_smooth-u1b2.tpqr", "cosmos_smooth-u1b2-channel0.csv")
    assert hashes(*two_names) == two
    run("smooth", "--unbound-states", "2", "--bound-states", "2", *smooth)
    before = torch.load(tmp_path / "cosmos_smooth-u2b2.tpqr")
    assert "restart_logliks" not in before and before["n_params"] == 15 and hashes(*two_names) == two
    run("smooth", "--unbound-states", "2", "--bound-states", "2", "--restarts", "3", *smooth)
    after = torch.load(tmp_path / "cosmos_smooth-u2b2.tpqr")
    assert set(after) >= set(before) | {"restart_logliks", "restart_best", "topology"}
    assert after["restart_logliks"].shape == (1, 4) and after["restart_best"].shape == (1,)
    assert after["topology"].shape == (4, 4) and after["topology"].dtype == torch.bool and bool(after["topology"].all())
    assert after["n_params"] == 15
    best = int(after["restart_best"][0])
    assert after["restart_logliks"][0, best] == after["restart_logliks"][0].max()
    assert after["bic"][0] <= before["bic"][0] + 1e-9 * abs(before["bic"][0])
    log = (tmp_path / ".tapqir" / "loginfo").read_text()
    assert "EM from 4 starts" in log and f"start #{best}" in log
    assert hashes(*two_names) == two and hashes(*three) == three
    run("smooth", "--bound-states", "2", *smooth)
    assert hashes(*three) == three and hashes(*two_names) == two
