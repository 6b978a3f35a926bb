"""Bootstrap refits of the chain over AOIs on the MI355X: the checks of tests/test_refit_host.py on
the kernels -- the weights against the oracle's bincount and against the resample of ``tq_hmm_estimate``, the weighted
M-step against ``tq_multistart_mstep`` bit for bit at weights 1 and against the long-double oracle, the E-step against
``tq_multistart_estep`` bit for bit where the weight is positive and untouched where it is 0, ``hmm_fit_refits`` against the
oracle's weighted EM -- then the statistical condition at R = 200 and ``fit``, ``smooth``, ``smooth --refit`` end to end."""

import hashlib

import numpy as np
import pandas as pd
import pytest
import torch
from typer.testing import CliRunner

from refit_fixture import PRIOR, START, fit_data
from smooth_fixture import synthetic_chain
from tapqir_amd.main import app
from tapqir_amd.utils.dataset import save
from tapqir_amd.utils.mle_analysis import (hmm_estimate, hmm_fit_refits, hmm_fit_restarts, hmm_permute, multistart_estep,
                                           multistart_mstep, refit_estep, refit_mstep, refit_weights)
from tapqir_amd.utils.safe_load import load_tpqr
from tapqir_amd.utils.simulate import TEST_PARAMS, simulate
from test_refit_host import (check_batches, check_estep, check_fit, check_mstep, check_weights,
                             check_weights_against_the_estimate)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


class DeviceBackend:
    """The kernels behind the interface of the checks of test_refit_host: numpy in, numpy out."""

    def weights(self, seed, first, R, N):
        return refit_weights(N, R, seed, first, DEV).cpu().numpy()

    def estimate_totals(self, trans, U, B, seed):
        return hmm_estimate(dev(trans), bootstrap=True, seed=seed)["totals"].cpu().numpy()

    def ms_estep(self, p, thetas, U, B):
        return multistart_estep(dev(p), dev(thetas), PRIOR, U, B).cpu().numpy()

    def ms_mstep(self, rows, thetas, T, it, U, B, allow=None):
        thetas, trace = dev(thetas), torch.full((len(thetas), T), float("nan"), dtype=torch.float64, device=DEV)
        multistart_mstep(dev(rows), thetas, trace, it, U, B, allow)
        return thetas.cpu().numpy(), trace.cpu().numpy()

    def estep(self, p, thetas, w, U, B, active, rows, filt):
        rows, filt = dev(rows), dev(filt)
        refit_estep(dev(p), dev(thetas), dev(w), PRIOR, U, B, None if active is None else dev(active), rows, filt)
        return rows.cpu().numpy(), filt.cpu().numpy()

    def mstep(self, rows, w, thetas, T, it, U, B, allow=None, active=None):
        thetas, trace = dev(thetas), torch.full((len(thetas), T), float("nan"), dtype=torch.float64, device=DEV)
        refit_mstep(dev(rows), thetas, dev(w), trace, it, U, B, allow, None if active is None else dev(active))
        return thetas.cpu().numpy(), trace.cpu().numpy()

    def fit_refits(self, p, theta_hat, U, B, refits, seed, num_iter, tol, chunk):
        fit = hmm_fit_refits(dev(p), PRIOR, theta_hat, U, B, refits, seed=seed, num_iter=num_iter, tol=tol, chunk=chunk)
        assert fit["thetas"].shape == (refits + 1, (U + B) ** 2 + U + B) and fit["logliks"].shape == (refits + 1,)
        return {"thetas": fit["thetas"].numpy(), "traces": fit["traces"].numpy(), "iterations": fit["iterations"],
                "converged": fit["converged"]}

    def ms_fit(self, p, start, U, B, num_iter, tol, chunk):
        fit = hmm_fit_restarts(dev(p), PRIOR, U, B, starts=start[None], num_iter=num_iter, tol=tol, chunk=chunk)
        theta = hmm_permute(fit["order"], U + B, theta=fit["thetas"][0])["theta"]
        return theta.cpu().numpy(), fit["traces"][0].cpu().numpy()


BE = DeviceBackend()


@pytest.mark.parametrize("first", [0, 5])
@pytest.mark.parametrize("R", [1, 3, 64])
@pytest.mark.parametrize("N", [1, 2, 63, 400])
def test_weights_are_the_bincount_of_the_resample(N, R, first):
    check_weights(BE, N, R, first)


@pytest.mark.parametrize("N", [2, 63, 400])
def test_weights_are_the_resample_of_the_estimate(N):
    check_weights_against_the_estimate(BE, N)


@pytest.mark.parametrize("R", [1, 2, 64])
@pytest.mark.parametrize("M", [2, 3, 4])
@pytest.mark.parametrize("N", [1, 2, 255, 256, 257, 300])
def test_weighted_mstep(N, M, R):
    check_mstep(BE, N, M, R)


@pytest.mark.parametrize("U,B", [(1, 1), (1, 2), (2, 2)])
@pytest.mark.parametrize("F", [1, 2, 65, 203])
def test_estep_skips_the_pairs_of_weight_zero(F, U, B):
    check_estep(BE, F, U, B)


@pytest.mark.parametrize("U,B", [(1, 1), (1, 2)])
def test_refits_follow_the_oracles_weighted_em(U, B):
    check_fit(BE, U, B)


def test_a_replica_does_not_depend_on_its_batch():
    check_batches(BE)


# ---- statistical condition ------------------------------------------------------------------------------------------------
STAT_SEED = 1


def test_the_interval_of_the_refits_covers_the_em_value():
    """N = 40, F = 500 of the synthetic chain (kon 0.05, koff 0.10), R = 200 refits of at most 200 iterations at the default
    --tol: no replica is left out as unconverged, and the 95 % percentile interval over the refits has the EM value of
    replica 0 strictly inside, for kon and for koff.  The seed was fixed after the float64 oracle's weighted EM alone met
    both conditions for it (DESIGN.md section 33 has its figures)."""
    fit = hmm_fit_refits(dev(fit_data()), PRIOR, START[(1, 1)], 1, 1, 200, seed=STAT_SEED, num_iter=200, tol=1e-9)
    left_out = 200 - sum(fit["converged"][1:])
    print(f"unconverged refits: {left_out}; iterations {min(fit['iterations'])} .. {max(fit['iterations'])}")
    assert left_out <= 0 and fit["converged"][0]
    pairs = fit["pairs"]
    for name, x in (("kon", pairs[:, 0, 1] / pairs[:, 0].sum(1)), ("koff", pairs[:, 1, 0] / pairs[:, 1].sum(1))):
        x = x.numpy()
        ll, ul = np.quantile(x[1:], [0.025, 0.975])
        print(f"{name}: EM {x[0]:.6f}, mean {x[1:].mean():.6f}, SE {x[1:].std(ddof=1):.6f}, 95% [{ll:.6f}, {ul:.6f}]")
        assert ll < x[0] < ul, name


# ---- command line -----------------------------------------------------------------------------------------------------
def test_fit_then_smooth_then_smooth_with_refit(tmp_path):
    runner = CliRunner()
    N, F, R = 8, 40, 32
    params = {k: v for k, v in TEST_PARAMS.items() if k != "pi"}
    params.update(kon=0.1, koff=0.2)
    save(simulate(2, N, F, 1, 14, params=params), tmp_path)

    def hashes(*names):
        return {name: hashlib.sha256((tmp_path / name).read_bytes()).hexdigest() for name in names}

    def run(*flags):
        result = runner.invoke(app, ["--cd", str(tmp_path), *flags, "--cuda", "--no-input"])
        assert result.exit_code == 0, result.output

    smooth = ["--num-samples", "50", "--num-iter", "60"]
    run("fit", "--model", "cosmos", "--nbatch-size", "8", "--fbatch-size", "40", "--num-iter", "2")
    for states, suffix, M, U in (([], "", 2, 1), (["--bound-states", "2"], "-u1b2", 3, 1)):
        plain = (f"cosmos_smooth{suffix}.tpqr", f"cosmos_smooth{suffix}-channel0.csv")
        new = (f"cosmos_smooth{suffix}-refit.tpqr", f"cosmos_smooth{suffix}-refit-channel0.csv")
        run("smooth", *states, *smooth)
        before = hashes(*plain)
        assert not any((tmp_path / name).exists() for name in new)
        run("smooth", *states, *smooth, "--refit", str(R), "--refit-seed", "2")
        assert hashes(*plain) == before  # what `smooth` wrote without --refit, byte for byte
        table = pd.read_csv(tmp_path / new[1], index_col=0)
        labels = [f"A{i}{j}" for i in range(M) for j in range(M)] + [f"dwell{i}" for i in range(M)] + ["kon", "koff"]
        assert list(table.columns) == ["EM", "Mean", "SE", "95% LL", "95% UL"] and list(table.index) == labels
        assert set(pd.read_csv(tmp_path / plain[1], index_col=0).index) <= set(labels)  # every row label of the channel CSV
        saved = torch.load(tmp_path / new[0])
        assert saved["refits"] == R and saved["seed"] == 2 and (saved["unbound"], saved["bound"]) == (U, M - U)
        assert saved["thetas"].shape == (1, R + 1, M * M + M) and saved["logliks"].shape == (1, R + 1)
        assert saved["converged"].shape == (1, R + 1) and saved["converged"].dtype == torch.bool
        keep = saved["converged"][0, 1:]
        assert int(keep.sum()) >= 2
        assert f"{R} refits" in (tmp_path / ".tapqir" / "loginfo").read_text()
        A = saved["thetas"][0, :, : M * M].reshape(R + 1, M, M)
        pairs = saved["pairs"][0]
        value = {f"A{i}{j}": A[:, i, j] for i in range(M) for j in range(M)}
        value.update({f"dwell{i}": 1 / (1 - A[:, i, i]) for i in range(M)})
        value["kon"] = pairs[:, :U, U:].sum((1, 2)) / pairs[:, :U].sum((1, 2))
        value["koff"] = pairs[:, U:, :U].sum((1, 2)) / pairs[:, U:].sum((1, 2))
        for name in labels:
            row, x = table.loc[name], value[name].numpy()
            assert row["EM"] == pytest.approx(x[0], rel=1e-12), name  # the CSV's digits of replica 0
            kept = x[1:][keep.numpy()]
            assert row["Mean"] == pytest.approx(kept.mean(), rel=1e-12) and row["SE"] == pytest.approx(kept.std(ddof=1), rel=1e-9)
            assert row["95% LL"] <= row["95% UL"] and row["SE"] >= 0, name
        run("smooth", *states, *smooth)
        assert hashes(*plain) == before
    # The posterior of a two-iteration fit is all bound (the EM ends at kon = 1, koff = 1e-9), so every refit sits at the same
    # floor of theta and the spread above is 0 -- the right answer there.  SE > 0 is checked where the evidence can move the
    # chain: the same files with the fit's p(z = 1) replaced by that of the fixture's chain (kon 0.05, koff 0.10) on 8 x 40.
    params = load_tpqr(tmp_path / "cosmos_params.tpqr")
    p = torch.from_numpy(synthetic_chain(N, F, seed=0)[0])
    params["z_probs"][:N, :, 0, 1] = p.to(params["z_probs"].dtype)
    params["z_probs"][:N, :, 0, 0] = (1 - p).to(params["z_probs"].dtype)
    torch.save(params, tmp_path / "cosmos_params.tpqr")
    run("smooth", "--num-samples", "50", "--num-iter", "200", "--refit", str(R), "--refit-seed", "2")
    table = pd.read_csv(tmp_path / "cosmos_smooth-refit-channel0.csv", index_col=0)
    saved = torch.load(tmp_path / "cosmos_smooth-refit.tpqr")
    print(table.to_string(), "\nconverged:", int(saved["converged"][0, 1:].sum()), "of", R)
    assert int(saved["converged"][0, 1:].sum()) >= 2
    for name in table.index:
        row = table.loc[name]
        assert row["SE"] > 0 and row["95% LL"] <= row["95% UL"], name
    assert table.loc["kon", "EM"] == pytest.approx((saved["pairs"][0, 0, 0, 1] / saved["pairs"][0, 0, 0].sum()).item(), rel=1e-12)
