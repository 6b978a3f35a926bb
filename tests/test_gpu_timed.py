"""The continuous-time hidden Markov chain on the frame timestamps on the MI355X: the checks of
tests/test_timed_host.py on the kernels -- the tables against the Van Loan oracle and their identities, the E-step against
the oracle's forward-backward at every length boundary and gap pattern, the M-step, the EM on the two-speed record -- then
the statistical condition through ``timed_fit`` and ``hmm_fit``, and ``fit``, ``smooth``, ``smooth --timed`` end to end."""

import hashlib

import numpy as np
import pandas as pd
import pytest
import torch
from typer.testing import CliRunner

import timed_fixture as tf
from tapqir_amd.main import app
from tapqir_amd.utils.dataset import save
from tapqir_amd.utils.mle_analysis import hmm_estep, hmm_fit, timed_estep, timed_fit, timed_mstep, timed_tables
from tapqir_amd.utils.safe_load import load_tpqr
from tapqir_amd.utils.simulate import TEST_PARAMS, simulate
from test_timed_host import (check_equal_spacing_is_the_per_frame_chain, check_estep, check_fit,
                             check_forbidden_k_plays_no_part, check_mstep, check_statistical_condition, check_tables)
from timed_fixture import PRIOR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def topology(bits, M):
    return torch.from_numpy(tf.allow_matrix(M, bits))


class DeviceBackend:
    """The kernels behind the interface of the checks of test_timed_host: numpy in, numpy out."""

    name = "MI355X"

    def tables(self, theta, d, U, B, allow):
        out = timed_tables(dev(theta), d, U, B, topology(allow, U + B))
        return out["P"].cpu().numpy(), out["K"].cpu().numpy()

    def estep(self, p, theta, P, K, cls, U, B, allow, gamma=True):
        out = timed_estep(dev(p), dev(theta), {"P": dev(P), "K": dev(K)}, cls, PRIOR, U, B, topology(allow, U + B), gamma)
        return {k: out[k].cpu().numpy() if k in out else None for k in ("filt", "gamma", "rows")}

    def mstep(self, rows, theta, U, B, allow):
        theta, trace = dev(theta), torch.full((1,), float("nan"), dtype=torch.float64, device=DEV)
        timed_mstep(dev(rows), theta, trace, 0, U, B, topology(allow, U + B))
        return theta.cpu().numpy(), trace.item()

    def em(self, p, theta0, d, cls, U, B, allow, num_iter):
        """One table launch, one E-step and one M-step per iteration on device buffers; theta is read back after each."""
        p, theta, top = dev(p), dev(theta0), topology(allow, U + B)
        trace = torch.full((num_iter,), float("nan"), dtype=torch.float64, device=DEV)
        thetas = [np.array(theta0, dtype=np.float64)]
        for it in range(num_iter):
            rows = timed_estep(p, theta, timed_tables(theta, d, U, B, top), cls, PRIOR, U, B, top, gamma=False)["rows"]
            timed_mstep(rows, theta, trace, it, U, B, top)
            thetas.append(theta.cpu().numpy().copy())
        return np.array(thetas), trace.cpu().numpy()

    def hmm_estep(self, p, theta, U, B):
        return {k: v.cpu().numpy() for k, v in hmm_estep(dev(p), dev(theta), PRIOR, U, B).items()}

    def fits(self, p, times, U, B, num_iter):
        fit = timed_fit(dev(p), PRIOR, times, U, B, num_iter=num_iter)
        frame = hmm_fit(dev(p), PRIOR, U, B, num_iter=num_iter)
        print(f"timed EM: {fit['iterations']} iterations, converged {fit['converged']}; per frame: {frame['iterations']}")
        theta = fit["theta"].cpu().numpy()
        return theta[1], theta[2], fit["loglik"], frame["loglik"]


BE = DeviceBackend()


@pytest.mark.parametrize("name", ["m2", "m3", "m4", "ref"])
def test_tables(name):
    check_tables(BE, name)


@pytest.mark.parametrize("pattern", tf.PATTERNS)
@pytest.mark.parametrize("U,B", tf.UB_LIST)
@pytest.mark.parametrize("F", tf.F_LIST)
def test_estep(F, U, B, pattern):
    check_estep(BE, F, U, B, pattern)


def test_estep_long_rows():
    check_estep(BE, 5000, 2, 2, "two-speed", N=2)


def test_forbidden_k_plays_no_part():
    check_forbidden_k_plays_no_part(BE)


@pytest.mark.parametrize("U,B", tf.UB_LIST)
@pytest.mark.parametrize("F", [2, 65, 203])
def test_equal_spacing_is_the_per_frame_chain(F, U, B):
    check_equal_spacing_is_the_per_frame_chain(BE, F, U, B)


@pytest.mark.parametrize("M", [2, 3, 4])
@pytest.mark.parametrize("N", [1, 2, 255, 256, 257])
def test_mstep(N, M):
    check_mstep(BE, N, M)


@pytest.mark.parametrize("U,B", [(1, 1), (1, 2)])
def test_fit_follows_the_oracles_em(U, B):
    check_fit(BE, U, B)


def test_statistical_condition():
    check_statistical_condition(BE)


def test_timed_fit_outputs():
    """``timed_fit`` on the two-speed record at (1, 2) with one transition forbidden: shapes, units, the canonical order, the
    forbidden rate exactly 0 in the order of the outputs, and a trace that is the log evidence of every iteration."""
    p, times = tf.record()
    allow = torch.ones(3, 3, dtype=torch.bool)
    allow[1, 2] = False
    fit = timed_fit(dev(p[:8, :120]), PRIOR, times[:120], 1, 2, allow=allow, num_iter=30, tol=-1.0, chunk=7)
    M, N, F = 3, 8, 120
    assert fit["theta"].shape == (M * M + M,) and fit["gamma"].shape == (N, F, M) and fit["filt"].shape == (N, F, M)
    assert fit["rows"].shape == (N, M * M + M + 1) and fit["trace"].shape == (30,) and fit["iterations"] == 30
    assert fit["n_params"] == 5 + 2 and fit["bic"] == pytest.approx(-2 * fit["loglik"] + 7 * np.log(N * F))
    Q = fit["theta"][: M * M].reshape(M, M).cpu().numpy()
    top = fit["allow"].numpy()
    off = ~np.eye(M, dtype=bool)
    assert (Q[off & ~top] == 0).all() and (~top).sum() == 1 and (Q[off & top] > 0).all()
    assert np.abs(Q.sum(1)).max() <= 1e-15 * np.abs(Q).max() * 8
    assert -Q[1, 1] <= -Q[2, 2]  # ascending exit rate within the bound class
    rows = fit["rows"].cpu().numpy()
    assert np.allclose(rows[:, [0, 4, 8]].sum(1), times[119] - times[0], rtol=1e-12)  # seconds
    assert fit["loglik"] == pytest.approx(rows[:, -1].sum()) and fit["loglik"] >= fit["trace"][-1].item() - 1e-9
    assert fit["scale"] == tf.gap_classes(times[:120])[2]
    assert np.allclose(fit["gamma"].sum(-1).cpu().numpy(), 1.0, atol=1e-12)


# ---- command line -----------------------------------------------------------------------------------------------------
def test_fit_then_smooth_then_smooth_timed(tmp_path):
    runner = CliRunner()
    N, F = 8, 40
    params = {k: v for k, v in TEST_PARAMS.items() if k != "pi"}
    params.update(kon=0.1, koff=0.2)
    data = simulate(2, N, F, 1, 14, params=params)
    save(data, tmp_path)
    Nt = data.N  # the on-target AOIs

    def hashes(*names):
        return {name: hashlib.sha256((tmp_path / name).read_bytes()).hexdigest() for name in names}

    def run(*flags, code=0):
        result = runner.invoke(app, ["--cd", str(tmp_path), *flags, "--cuda", "--no-input"])
        assert result.exit_code == code, result.output
        return result.output

    smooth = ["--num-samples", "50", "--num-iter", "60"]
    run("fit", "--model", "cosmos", "--nbatch-size", "8", "--fbatch-size", "40", "--num-iter", "2")
    plain = ("cosmos_smooth.tpqr", "cosmos_smooth-channel0.csv")
    run("smooth", *smooth)
    before = hashes(*plain)
    # no time stamps in data.tpqr and none given: exit 1 with a text, nothing written
    assert "--frame-time" in run("smooth", "--timed", *smooth, code=1)
    assert not list(tmp_path.glob("cosmos_smooth-timed*"))
    # the two-speed stamps in Glimpse's milliseconds: 20 frames 1 s apart, a pause of 60 s, 20 frames 5 s apart
    gaps = np.concatenate([np.ones(19), [60.0], np.full(19, 5.0)])
    stamps = torch.from_numpy(np.concatenate([[0.0], np.cumsum(gaps)]) * 1000.0 + 12345.0)
    data.ttb = stamps[:, None].clone()
    save(data, tmp_path)
    # The posterior of a two-iteration fit is all bound; the chain has something to fit where the fit's p(z = 1) is that of
    # the fixture's two-state chain (kon 0.05, koff 0.10 per frame) on 8 x 40.
    from smooth_fixture import synthetic_chain

    fitted = load_tpqr(tmp_path / "cosmos_params.tpqr")
    p = torch.from_numpy(synthetic_chain(N, F, seed=0)[0])
    fitted["z_probs"][:N, :, 0, 1] = p.to(fitted["z_probs"].dtype)
    fitted["z_probs"][:N, :, 0, 0] = (1 - p).to(fitted["z_probs"].dtype)
    torch.save(fitted, tmp_path / "cosmos_params.tpqr")
    run("smooth", *smooth)
    before = hashes(*plain)
    for flags, suffix, M, U, forbidden in (
            ([], "", 2, 1, []),
            (["--bound-states", "2", "--forbid", "1-2", "--forbid", "2-1"], "-u1b2", 3, 1, [(1, 2), (2, 1)])):
        new = (f"cosmos_smooth-timed{suffix}.tpqr", f"cosmos_smooth-timed{suffix}-channel0.csv")
        run("smooth", "--timed", *flags, *smooth)
        assert hashes(*plain) == before  # what `smooth` wrote without --timed, byte for byte
        table = pd.read_csv(tmp_path / new[1], index_col=0)
        labels = ([f"q{i}{j}" for i in range(M) for j in range(M) if i != j] + [f"dwell{i}" for i in range(M)]
                  + ["kon", "koff"])
        assert list(table.columns) == ["EM"] and list(table.index) == labels
        saved = torch.load(tmp_path / new[0])
        assert (saved["unbound"], saved["bound"]) == (U, M - U) and saved["theta"].shape == (1, M * M + M)
        assert saved["z_probs"].shape == (Nt, F, 1) and saved["state_probs"].shape == (Nt, F, 1, M)
        assert torch.equal(saved["z_map"], saved["z_probs"] > 0.5) and saved["mask"].shape == (Nt,)
        assert torch.equal(saved["times"][:, 0], (stamps * 0.001).to(torch.float64))
        assert saved["log_evidence"].shape == (Nt, 1) and saved["bic"].shape == (1,) and len(saved["loglik_trace"]) == 1
        assert saved["log_evidence_per_frame"].shape == (1,)
        assert saved["n_params"] == M * (M - 1) - len(forbidden) + M - 1
        Q = saved["theta"][0, : M * M].reshape(M, M)
        top = saved["topology_by_channel"][0]
        off = ~torch.eye(M, dtype=torch.bool)
        assert bool((Q[off] >= 0).all()) and bool((Q[off & ~top] == 0).all()) and int((~top).sum()) == len(forbidden)
        assert bool((Q[off & top] >= 1e-9 / 5.0 * 0.99).all())  # the floor, per median gap of 5 s
        for i in range(M):
            for j in range(M):
                if i != j:
                    assert table.loc[f"q{i}{j}", "EM"] == pytest.approx(Q[i, j].item(), rel=1e-12, abs=0)
            assert table.loc[f"dwell{i}", "EM"] == pytest.approx(-1.0 / Q[i, i].item(), rel=1e-12)
        assert table.loc["kon", "EM"] > 0 and table.loc["koff", "EM"] > 0
        log = (tmp_path / ".tapqir" / "loginfo").read_text()
        assert "the time stamps gain" in log
    # --frame-time in the place of the stamps; a time scale that leaves them as they are
    run("smooth", "--timed", "--frame-time", "0.5", *smooth)
    saved = torch.load(tmp_path / "cosmos_smooth-timed.tpqr")
    assert torch.equal(saved["times"][:, 0], torch.arange(F, dtype=torch.float64) * 0.5)
    # stamps that do not increase: exit 1
    data.ttb = stamps[:, None].clone()
    data.ttb[7] = data.ttb[6]
    save(data, tmp_path)
    assert "strictly increasing" in run("smooth", "--timed", *smooth, code=1)
    run("smooth", *smooth)
    assert hashes(*plain) == before
