"""Dwell-time kernels on the MI355X: the interval sampler (exact replay, histograms, 0/1 rows, law of the interior runs),
the batched K-exponential mixture MLE (float64 torch restatement, input forms, chunking, LDS and L2 paths, empty rows,
recovery of known rates) and the ``dwelltime`` command end to end."""

import math

import numpy as np
import pandas as pd
import pytest
import torch
from typer.testing import CliRunner

from dwell_fixture import COLUMNS, build_dwell_check, host_sample, loglik64, torch_fit64
from tapqir_amd.main import app
from tapqir_amd.utils.dataset import save
from tapqir_amd.utils.imscroll import bound_dwell_times, unbound_dwell_times
from tapqir_amd.utils.mle_analysis import (dwell_csr_from_hist, dwell_csr_from_padded, dwell_fit, dwell_fit_steps,
                                           dwell_init_state, dwell_intervals, dwell_sample)
from tapqir_amd.utils.simulate import TEST_PARAMS, simulate

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def hk(tmp_path_factory):
    return build_dwell_check(tmp_path_factory.mktemp("dwell"))


def mixture_draws(gen, S, M, k=(0.1, 0.01), A=(0.6, 0.4)):
    """S x M continuous dwell times of the mixture sum_j A_j k_j exp(-k_j t)."""
    u = torch.rand(S, M, generator=gen, dtype=torch.float64)
    comp = torch.searchsorted(torch.cumsum(torch.tensor(A, dtype=torch.float64), 0), u.reshape(-1)).reshape(S, M)
    rate = torch.tensor(k, dtype=torch.float64)[comp.clamp(max=len(k) - 1)]
    return (-torch.log(torch.rand(S, M, generator=gen, dtype=torch.float64)) / rate).float()


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float(((a - b).abs() / b.abs()).max())


def test_sampler_replay_is_exact(hk):
    """S = 71, N = 37, F = 203 with exact 0s and 1s: row counts, histograms and the table equal the g++ replay."""
    S, seed = 71, 20261016
    gen = torch.Generator().manual_seed(0)
    p = torch.rand(37, 203, generator=gen) ** 3
    p[0] = 0.0
    p[1] = 1.0
    p[2, ::3] = 1.0
    p[3, 50:60] = 0.0
    p[4, 100:] = 1.0
    sample = dwell_sample(p.to(DEV), S, seed=seed)
    table = dwell_intervals(p.to(DEV), S, seed=seed, sample=sample)
    want_table, counts, hb, hu = host_sample(hk, p.numpy(), S, seed)
    assert np.array_equal(sample["counts"].cpu().numpy(), counts)
    assert np.array_equal(sample["hist_bound"].cpu().numpy(), hb)
    assert np.array_equal(sample["hist_unbound"].cpu().numpy(), hu)
    assert list(table.columns) == COLUMNS and all(table[c].dtype == np.int64 for c in COLUMNS)
    pd.testing.assert_frame_equal(table, want_table)
    # launch B without a given launch A draws the same table
    pd.testing.assert_frame_equal(dwell_intervals(p.to(DEV), S, seed=seed), want_table)


def test_histograms_are_the_bincount_of_the_interior_rows():
    gen = torch.Generator().manual_seed(1)
    p = torch.rand(19, 150, generator=gen)
    S, F = 130, 150
    sample = dwell_sample(p.to(DEV), S, seed=5)
    table = dwell_intervals(p.to(DEV), S, seed=5, sample=sample)
    for code, key in ((1, "hist_bound"), (0, "hist_unbound")):
        sel = table[table["low_or_high"] == code]
        want = np.zeros((S, F), np.int64)
        np.add.at(want, (sel["posterior_sample"].to_numpy(), sel["dwell_time"].to_numpy()), 1)
        assert np.array_equal(sample[key].cpu().numpy(), want), key
    assert np.array_equal(sample["counts"].cpu().numpy().sum(1), np.bincount(table["posterior_sample"], minlength=S))


def test_deterministic_rows_give_the_same_intervals_in_every_sample():
    F, S = 12, 90
    p = torch.zeros(3, F)
    p[1] = 1.0
    p[2, 3:7] = 1.0  # 0 0 0 1 1 1 1 0 0 0 0 0
    table = dwell_intervals(p.to(DEV), S, seed=11)
    want = {0: [(0, F - 1, 2, 0)], 1: [(0, F - 1, 3, 1)], 2: [(0, 2, -2, 0), (3, 6, 1, 1), (7, F - 1, 2, 0)]}
    for s in range(S):
        rows = table[table["posterior_sample"] == s]
        for n, runs in want.items():
            got = rows[rows["aoi"] == n][["start_frame", "stop_frame", "low_or_high", "z"]]
            assert [tuple(r) for r in got.to_numpy()] == runs, (s, n)
    sample = dwell_sample(p.to(DEV), S, seed=11)
    assert (sample["hist_bound"][:, 4] == 1).all() and sample["hist_bound"].sum() == S
    assert sample["hist_unbound"].sum() == 0


@pytest.mark.parametrize("p", [0.2, 0.65])
def test_interior_run_law(p):
    """Rows of F frames with constant p: a bound run of length L is interior when it starts at some f in 1 .. F - L - 1
    after an unbound frame and ends before an unbound one, so E[count] = (F - L - 1) (1 - p)^2 p^L per row (p <-> 1 - p
    for unbound runs); every bin within 5 sigma (sigma^2 ~ the expectation, clamped at 1)."""
    S, N, F = 4000, 16, 40
    sample = dwell_sample(torch.full((N, F), p).to(DEV), S, seed=7)
    L = torch.arange(F, dtype=torch.float64)
    for key, q in (("hist_bound", p), ("hist_unbound", 1 - p)):
        pf = torch.tensor(np.float32(q), dtype=torch.float64)  # the kernel compares against the float32 value
        expect = S * N * (F - L - 1).clamp(min=0) * (1 - pf) ** 2 * pf ** L
        expect[0] = 0.0
        got = sample[key].sum(0).double().cpu()
        z = (got - expect).abs() / expect.sqrt().clamp(min=1.0)
        assert z.max() < 5.0, (key, z.max(), got[:6], expect[:6])


# ---- fit ----------------------------------------------------------------------------------------------------------
TOL_10K = {1: 1e-4, 2: 1e-3, 3: 3e-3}  # relative, after 10 000 float32 Adam steps


@pytest.mark.parametrize("K", [1, 2, 3])
def test_fit_matches_float64_torch(K):
    gen = torch.Generator().manual_seed(3)
    data = mixture_draws(gen, 4, 300).round().clamp(min=1.0)
    data[1, 250:] = 0.0  # padding
    for steps, tol in ((300, 1e-4), (10000, TOL_10K[K])):
        got = dwell_fit(data.to(DEV), K, n_steps=steps)
        want = torch_fit64(data, K, n_steps=steps)
        assert rel(got["k"], want["k"]) <= tol, (K, steps, got["k"].cpu(), want["k"])
        assert rel(got["A"], want["A"]) <= tol, (K, steps, got["A"].cpu(), want["A"])
        # the reported loss is the float64 loss at the parameters the last step starts from
        loss64 = -loglik64(torch_fit64(data, K, n_steps=steps - 1)["par"], data.double(), K)
        assert rel(got["loss"], loss64) < 1e-4, (got["loss"].cpu(), loss64)


def test_histogram_and_padded_inputs_agree():
    gen = torch.Generator().manual_seed(4)
    p = (torch.rand(40, 300, generator=gen) < 0.5).float() * 0.8 + 0.1
    S = 16
    sample = dwell_sample(p.to(DEV), S, seed=2)
    table = dwell_intervals(p.to(DEV), S, seed=2, sample=sample)
    for key, padded_fn in (("hist_bound", bound_dwell_times), ("hist_unbound", unbound_dwell_times)):
        assert (sample[key].sum(1) > 0).all()  # every sample has runs: the padded rows are not shifted
        padded = torch.from_numpy(padded_fn(table))
        a = dwell_fit(dwell_csr_from_hist(sample[key]), 2, n_steps=1000)
        b = dwell_fit(padded.to(DEV), 2, n_steps=1000)
        for name in ("k", "A", "loss"):
            assert rel(a[name], b[name]) < 1e-4, (key, name)


def test_chunked_equals_single_launch():
    gen = torch.Generator().manual_seed(5)
    data = mixture_draws(gen, 64, 200).round().clamp(min=1.0).to(DEV)
    one = dwell_fit(data, 3, n_steps=3000, chunk=3000)
    chunked = dwell_fit(data, 3, n_steps=3000, chunk=700)
    for name in ("k", "A", "loss"):
        assert torch.equal(one[name], chunked[name]), name


def test_lds_and_l2_paths_agree():
    gen = torch.Generator().manual_seed(6)
    data = mixture_draws(gen, 8, 1500).round().clamp(min=1.0).to(DEV)
    staged = dwell_fit(data, 2, n_steps=1000, stage_lds=True)
    l2 = dwell_fit(data, 2, n_steps=1000, stage_lds=False)
    for name in ("k", "A", "loss"):
        assert rel(l2[name], staged[name]) < 1e-5, name
    # rows longer than the LDS budget (TQ_DWELL_LDS_PAIRS = 2048) take the L2 path on their own
    big = mixture_draws(gen, 3, 5000)
    got = dwell_fit(big.to(DEV), 2, n_steps=300)
    want = torch_fit64(big, 2, n_steps=300)
    assert rel(got["k"], want["k"]) <= 1e-4 and rel(got["A"], want["A"]) <= 1e-4


@pytest.mark.parametrize("K", [1, 3])
def test_empty_row_keeps_its_initial_parameters(K):
    data = torch.zeros(3, 50)
    data[1, :10] = torch.arange(1, 11).float()
    data[2, :3] = 5.0
    values, weights, row_ptr = dwell_csr_from_padded(data.to(DEV))
    state = dwell_init_state(3, K, DEV)
    init = state.clone()
    dwell_fit_steps(state, (values, weights, row_ptr), K, n_steps=500)
    assert torch.equal(state[0], init[0])
    assert torch.isfinite(state).all()
    if K == 1:  # one component: the logit gradient is exactly zero, so the logit and its moments stay put
        assert (state[:, 1] == 0).all() and (state[:, 3] == 0).all() and (state[:, 5] == 0).all()


def test_recovery_of_known_rates():
    """2000 continuous dwell times per data set from k = (0.1, 0.01), A = (0.6, 0.4), 8 data sets.  Tolerance: the
    asymptotic standard error of the MLE from the float64 Fisher information at the truth, in (log k0, log k1, logit A0);
    every fit within 5 standard errors, their mean within 5 / sqrt(8)."""
    gen = torch.Generator().manual_seed(7)
    data = mixture_draws(gen, 8, 2000)
    fit = dwell_fit(data.to(DEV), 2, n_steps=10000)
    k, A = fit["k"].double().cpu(), fit["A"].double().cpu()
    order = torch.argsort(k, dim=1, descending=True)  # components are exchangeable: fast one first
    k, A = k.gather(1, order), A.gather(1, order)
    est = torch.stack([k[:, 0].log(), k[:, 1].log(), torch.logit(A[:, 0])], 1)
    truth = torch.tensor([math.log(0.1), math.log(0.01), math.log(0.6 / 0.4)], dtype=torch.float64)

    def ll(q):
        par = torch.stack([q[0], q[1], q[2], torch.zeros((), dtype=q.dtype)]).reshape(1, 4)
        return loglik64(par, data[:1].double(), 2).sum()

    info = -torch.autograd.functional.hessian(ll, truth)
    se = torch.sqrt(torch.diagonal(torch.linalg.inv(info)))
    zs = (est - truth) / se
    assert zs.abs().max() < 5.0, zs
    assert (zs.mean(0).abs() < 5.0 / math.sqrt(8)).all(), zs.mean(0)
    print(f"fitted means k={k.mean(0).tolist()} A={A.mean(0).tolist()}; max |z| = {zs.abs().max().item():.2f}")


# ---- command line -------------------------------------------------------------------------------------------------
def test_dwelltime_command_end_to_end(tmp_path):
    runner = CliRunner()
    save(simulate(2, 8, 30, 1, 14, params=dict(TEST_PARAMS)), tmp_path)
    result = runner.invoke(app, ["--cd", str(tmp_path), "fit", "--model", "cosmos", "--nbatch-size", "8", "--fbatch-size",
                                 "30", "--num-iter", "2", "--cuda", "--no-input"])
    assert result.exit_code == 0, result.output
    result = runner.invoke(app, ["--cd", str(tmp_path), "dwelltime", "-K", "2", "--num-samples", "50", "--num-iter", "200",
                                 "--cuda", "--no-input"])
    assert result.exit_code == 0, result.output
    n_on = 4  # simulate: the first half of the AOIs are on target, all selected by the mask
    table = pd.read_pickle(tmp_path / "cosmos_dwelltime-intervals-channel0.pkl")
    assert list(table.columns) == COLUMNS and all(table[c].dtype == np.int64 for c in COLUMNS)
    assert set(table["posterior_sample"]) == set(range(50)) and set(table["aoi"]) == set(range(n_on))
    assert (table["dwell_time"] == table["stop_frame"] + 1 - table["start_frame"]).all()
    assert table.groupby(["posterior_sample", "aoi"])["dwell_time"].sum().eq(30).all()
    for rate in ("koff", "kon"):
        res = pd.read_csv(tmp_path / f"cosmos_dwelltime-{rate}-channel0.csv", index_col=0)
        assert list(res.index) == ["A0", f"{rate}0", "A1", f"{rate}1"], list(res.index)
        assert list(res.columns) == ["Mean", "95% LL", "95% UL"]
        assert np.isfinite(res.values).all()
    try:
        import scipy.io
    except ImportError:
        scipy = None
    if scipy is not None:
        mat = scipy.io.loadmat(tmp_path / "cosmos_dwelltime-intervals-channel0.mat")
        assert np.array_equal(mat["dwell_time"].ravel(), table["dwell_time"].to_numpy())
    try:
        import matplotlib  # noqa: F401
    except ImportError:
        return
    for kind in ("bound", "unbound"):
        assert (tmp_path / f"cosmos_dwelltime-{kind}-histogram-channel0.png").is_file(), kind
