"""``tq_smooth_dwell`` on the MI355X: counts, interior histograms, first-binding frames and the interval table exactly equal
to the host functions of ``tapqir_amd.utils.imscroll`` on the raster that the existing ``smooth_sample(..., raster=True)``
writes for the same ``filt``, ``theta`` and seed; the guards of the EMIT launch; the law of the first binding; the size of
the correction over independent draws; and ``fit``, ``smooth``, ``dwelltime --smooth``, ``ttfb --smooth`` end to end."""

import ctypes as C

import numpy as np
import pandas as pd
import pytest
import torch
from typer.testing import CliRunner

from smooth_dwell_fixture import (F_LIST, assert_equals_oracle, interior_means, n01_of_table, oracle_of_raster,
                                  oracle_survival, survival_deviation)
from smooth_fixture import synthetic_chain, with_special_rows
from tapqir_amd import _lib, _lib_smooth
from tapqir_amd.main import app
from tapqir_amd.utils.dataset import save
from tapqir_amd.utils.imscroll import INTERVAL_COLUMNS
from tapqir_amd.utils.mle_analysis import (dwell_csr_from_hist, dwell_fit, dwell_sample, smooth_dwell_intervals,
                                           smooth_dwell_sample, smooth_estep, smooth_fit, smooth_sample, ttfb_fit,
                                           ttfb_sample)
from tapqir_amd.utils.safe_load import load_tpqr
from tapqir_amd.utils.simulate import TEST_PARAMS, simulate

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PRIOR = 1.0 / 3.0
THETA = (0.05, 0.10, 0.4)


def dev_theta(theta):
    return torch.tensor(theta, dtype=torch.float64, device=DEV)


def to_numpy(sample, table):
    return {**{k: v.cpu().numpy() for k, v in sample.items()}, "table": table}


def replay(p, S, seed):
    """The device's filt, the raster of the existing sampler with its counts, and both launches of the new one."""
    theta = dev_theta(THETA)
    filt = smooth_estep(torch.from_numpy(p).to(DEV), theta, PRIOR)["filt"]
    counts4, raster = smooth_sample(filt, theta, S, seed=seed, raster=True)
    sample = smooth_dwell_sample(filt, theta, S, seed=seed)
    table = smooth_dwell_intervals(filt, theta, S, seed=seed, sample=sample)
    return filt, theta, counts4.cpu().numpy(), raster.cpu().numpy(), sample, table


def check_replay(p, S, seed):
    N, F = p.shape
    filt, theta, counts4, raster, sample, table = replay(p, S, seed)
    assert sample["counts"].shape == (S, N) and sample["counts"].dtype == torch.int32
    assert sample["tau"].shape == (S, N) and sample["tau"].dtype == torch.float32
    for key in ("hist_bound", "hist_unbound"):
        assert sample[key].shape == (S, F) and sample[key].dtype == torch.int32
    assert all(table[c].dtype == np.int64 for c in INTERVAL_COLUMNS)
    want = oracle_of_raster(raster)
    assert_equals_oracle(to_numpy(sample, table), want, f"S = {S}, N = {N}, F = {F}")
    assert np.array_equal(n01_of_table(table, S, N), counts4[..., 0])
    # twice the same bits, with and without a given launch A
    again = smooth_dwell_sample(filt, theta, S, seed=seed)
    for key in sample:
        assert torch.equal(sample[key], again[key]), key
    pd.testing.assert_frame_equal(smooth_dwell_intervals(filt, theta, S, seed=seed), table)
    return want


# ---- exact replay -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 64, 65, 130])
@pytest.mark.parametrize("F", F_LIST)
def test_replay_equals_the_host_functions_on_the_raster_of_smooth(F, S):
    """N = 6: rows of all 0, all 1, alternating 0 / 1 and p = prior, and two rows of the synthetic chain."""
    want = check_replay(with_special_rows(synthetic_chain(6, F, 0)[0], PRIOR), S, seed=0)
    assert (want["tau"][:, 0] == F).all() and (want["tau"][:, 1] == 0).all()  # never and always bound


def test_many_rows_few_samples():
    check_replay(synthetic_chain(37, 203, seed=3)[0], 3, seed=2**40 + 203)


# ---- guards -----------------------------------------------------------------------------------------------------------
def emit(filt, theta, counts, offsets, buffer, total, S, seed):
    """One EMIT launch into ``buffer`` (rows of ``total`` int32) through the entry point itself."""
    N, F = filt.shape
    a = _lib_smooth.SmoothDwellArgs(filt=_lib.ptr(filt), theta=_lib.ptr(theta), counts=_lib.ptr(counts),
                                    offsets=_lib.ptr(offsets), intervals=_lib.ptr(buffer), total=total, N=N, F=F, S=S,
                                    mode=_lib.DWELL_EMIT, seed=seed)
    rc = _lib_smooth.lib().tq_smooth_dwell(C.byref(a), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("F", [2, 65])
def test_short_table_holds_the_first_rows_and_nothing_else(F):
    S, seed = 70, 0
    p = with_special_rows(synthetic_chain(6, F, 0)[0], PRIOR)
    filt, theta, _, raster, sample, table = replay(p, S, seed)
    counts = sample["counts"]
    csum = torch.cumsum(counts.reshape(-1).to(torch.int64), 0)
    offsets = (csum - counts.reshape(-1)).contiguous()
    total = len(table) - 1
    buffer = torch.full((_lib.DWELL_COLS + 1, total), -7, dtype=torch.int32, device=DEV)  # the last row is the canary
    assert emit(filt, theta, counts, offsets, buffer, total, S, seed) == 0
    host = buffer.cpu().numpy()
    assert (host[_lib.DWELL_COLS] == -7).all()
    for i, col in enumerate(INTERVAL_COLUMNS):
        assert np.array_equal(host[i], table[col].to_numpy()[:total]), col
    # an empty table launches nothing
    buffer.fill_(-7)
    assert emit(filt, theta, counts, offsets, buffer, 0, S, seed) == 0
    assert bool((buffer == -7).all())


# ---- the law of the first binding ---------------------------------------------------------------------------------------
def test_first_binding_follows_the_exact_survival_law():
    """S = 4096, N = 4, F = 129 (generator seed 4: 136 points, see the host test): the empirical P(tau > f) within 5
    binomial sigma of the exact survival of the smoothed chain wherever that lies in [0.02, 0.98]."""
    S, N, F = 4096, 4, 129
    p = synthetic_chain(N, F, seed=4)[0]
    theta = dev_theta(THETA)
    filt = smooth_estep(torch.from_numpy(p).to(DEV), theta, PRIOR)["filt"]
    tau = smooth_dwell_sample(filt, theta, S, seed=7)["tau"].cpu().numpy()
    assert tau.min() >= 0 and tau.max() <= F and np.array_equal(tau, np.rint(tau))
    points, dev = survival_deviation(tau, oracle_survival(p, THETA, PRIOR))
    print(f"{points} points, largest deviation {dev:.2f} sigma")
    assert points >= 100
    assert dev <= 5.0


# ---- it fixes what it is for ------------------------------------------------------------------------------------------
def test_markov_rasters_mend_the_dwell_times_and_the_first_binding():
    """N = 40, F = 500, seed 0, 50 EM iterations, S = 64: for the interior bound and unbound dwell times and for tau,
    |Markov - hidden| <= 0.25 |independent - hidden| (means over samples of per-sample means); independent =
    ``dwell_sample`` / ``ttfb_sample`` on the same p, hidden = the fixture's true raster."""
    S = 64
    p_host, z = synthetic_chain(40, 500, seed=0)
    p = torch.from_numpy(p_host).to(DEV)
    fit = smooth_fit(p, PRIOR, num_iter=50, tol=0.0)
    assert fit["iterations"] == 50
    markov = smooth_dwell_sample(fit["filt"], fit["theta"], S, seed=0)
    independent = dwell_sample(p, S, seed=0)
    hidden = oracle_of_raster(z[None])
    for key in ("hist_bound", "hist_unbound"):
        h, i, m = (interior_means(x) for x in (hidden[key], independent[key].cpu().numpy(), markov[key].cpu().numpy()))
        print(f"{key}: hidden {h:.3f}, independent {i:.3f}, Markov {m:.3f}, ratio {abs(m - h) / abs(i - h):.3f}")
        assert abs(m - h) <= 0.25 * abs(i - h)
    h, i, m = hidden["tau"].mean(), ttfb_sample(p, S, seed=0).mean().item(), markov["tau"].mean().item()
    print(f"tau: hidden {h:.3f}, independent {i:.3f}, Markov {m:.3f}, ratio {abs(m - h) / abs(i - h):.3f}")
    assert abs(m - h) <= 0.25 * abs(i - h)
    # the outputs plug into the fits unchanged
    k = dwell_fit(dwell_csr_from_hist(markov["hist_bound"]), 1, n_steps=200)["k"]
    ka = ttfb_fit(markov["tau"], 500, n_steps=200)["ka"]
    assert k.shape == (S, 1) and ka.shape == (S, 1) and bool(torch.isfinite(k).all() and torch.isfinite(ka).all())


# ---- command line -------------------------------------------------------------------------------------------------
def test_fit_smooth_dwelltime_ttfb_end_to_end(tmp_path):
    runner = CliRunner()
    N, F = 8, 40
    params = {k: v for k, v in TEST_PARAMS.items() if k != "pi"}
    params.update(kon=0.1, koff=0.2)
    save(simulate(2, N, F, 1, 14, params=params), tmp_path)

    def run(*args):
        return runner.invoke(app, ["--cd", str(tmp_path), *args, "--cuda", "--no-input"])

    result = run("fit", "--model", "cosmos", "--nbatch-size", "8", "--fbatch-size", "40", "--num-iter", "2")
    assert result.exit_code == 0, result.output
    dwell_args = ("dwelltime", "-K", "1", "--num-samples", "8", "--num-iter", "50")
    result = run(*dwell_args, "--smooth")
    assert result.exit_code == 1 and "run `smooth` first" in result.output, result.output
    result = run("smooth", "--num-samples", "50", "--num-iter", "30")
    assert result.exit_code == 0, result.output
    result = run(*dwell_args)
    assert result.exit_code == 0, result.output
    plain = {f.name: f.read_bytes() for f in tmp_path.iterdir() if "_dwelltime-" in f.name}
    assert "cosmos_dwelltime-intervals-channel0.pkl" in plain and not any("-smooth" in name for name in plain)

    result = run(*dwell_args, "--smooth")
    assert result.exit_code == 0, result.output
    result = run("ttfb", "--smooth", "--num-samples", "8", "--num-iter", "50")
    assert result.exit_code == 0, result.output
    for name, content in plain.items():
        assert (tmp_path / name).read_bytes() == content, name
    assert not any(f.name.startswith("cosmos_ttfb-") and "-smooth" not in f.name for f in tmp_path.iterdir())

    n_on = N // 2  # simulate: the first half of the AOIs are on target, all selected by the mask
    table = pd.read_pickle(tmp_path / "cosmos_dwelltime-smooth-intervals-channel0.pkl")
    assert list(table.columns) == INTERVAL_COLUMNS and all(table[c].dtype == np.int64 for c in INTERVAL_COLUMNS)
    assert set(table["posterior_sample"]) == set(range(8)) and set(table["aoi"]) == set(range(n_on))
    assert table.groupby(["posterior_sample", "aoi"])["dwell_time"].sum().eq(F).all()
    tau = pd.read_csv(tmp_path / "cosmos_ttfb-smooth-data-points-channel0.csv", index_col=0).to_numpy()
    assert tau.shape == (8, n_on) and tau.min() >= 0 and tau.max() <= F
    res = pd.read_csv(tmp_path / "cosmos_ttfb-smooth-params-channel0.csv", index_col=0)
    assert list(res.index) == ["ka", "kns", "Af"] and np.isfinite(res.values).all()
    assert (tmp_path / "cosmos_ttfb-smooth-fraction-bound-channel0.csv").is_file()
    # the rasters are those of `smooth`: the table's first-binding frames are ttfb --smooth's data points
    first = table[table["z"] == 1].groupby(["posterior_sample", "aoi"])["start_frame"].min()
    want = np.full((8, n_on), float(F))
    want[first.index.get_level_values(0), first.index.get_level_values(1)] = first.to_numpy()
    assert np.array_equal(tau, want)

    payload = load_tpqr(tmp_path / "data.tpqr")
    payload["mask"][1] = False  # another selection of AOIs than `smooth` saw
    torch.save(payload, tmp_path / "data.tpqr")
    result = run("ttfb", "--smooth", "--num-samples", "8", "--num-iter", "50")
    assert result.exit_code == 1 and "mask" in result.output, result.output
