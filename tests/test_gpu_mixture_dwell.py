"""``tq_population_dwell`` on the MI355X: counts, first-binding frames, populations and the interval
table exactly equal to the host functions of ``tapqir_amd.utils.imscroll`` on the class view of the raster that the existing
``mixture_sample(..., raster=True)`` writes for the same inputs and seed, the histograms of every population equal to those
of that raster with the other populations' rows blanked, and everything bit-equal to the g++ replay fed the device's ``filt``
and ``resp``; one population bit-equal to ``tq_chain_dwell``; the guards of the EMIT launch; the law of the first binding
under the mixture; the conditions of the section; and ``fit``, ``smooth``, ``smooth --populations 2``,
``dwelltime --smooth --populations 2``, ``ttfb --smooth --populations 2`` end to end."""

import ctypes as C
import importlib.util

import numpy as np
import pandas as pd
import pytest
import torch
from typer.testing import CliRunner

import mixture_dwell_fixture as mdf
import mixture_fixture as mf
from smooth_dwell_fixture import survival_deviation
from tapqir_amd import _lib, _lib_mixture
from tapqir_amd.main import app
from tapqir_amd.utils.dataset import save
from tapqir_amd.utils.imscroll import INTERVAL_COLUMNS
from tapqir_amd.utils.mle_analysis import (hmm_dwell_intervals, hmm_dwell_sample, hmm_estep, hmm_fit, mixture_dwell_intervals,
                                           mixture_dwell_sample, mixture_fit, mixture_sample)
from tapqir_amd.utils.safe_load import load_tpqr
from tapqir_amd.utils.simulate import TEST_PARAMS, simulate

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
UB_LIST = [(1, 1), (1, 2), (2, 2)]


@pytest.fixture(scope="module")
def hk(tmp_path_factory):
    return mdf.build_population_dwell_check(tmp_path_factory.mktemp("population_dwell"))


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def to_numpy(sample, table):
    return {**{k: v.cpu().numpy() for k, v in sample.items()}, "table": table}


def device_filt(p, thetas, U, B):
    return torch.stack([hmm_estep(dev(p), dev(thetas[g]), mf.PRIOR, U, B)["filt"] for g in range(len(thetas))])


def inputs(U, B, G, F, N=6):
    """``mixture_fixture.sampler_inputs`` with the device's own filt."""
    p = mf.synthetic_hmm(N, F, seed=F)[0]
    if N == 6:
        p = mf.with_special_rows(p, mf.PRIOR)
    thetas = np.array([mf.fixed_theta(U, B, seed=g) for g in range(G)])
    resp = np.ascontiguousarray(np.random.default_rng(100 * F + G).dirichlet(np.ones(G), N).T)
    return device_filt(p, thetas, U, B), dev(thetas), dev(resp), thetas, resp


def check_replay(hk, filt, dthetas, dresp, thetas, resp, U, B, S, seed):
    G, N, F = filt.shape[:3]
    who = f"({U}, {B}) G = {G}, S = {S}, N = {N}, F = {F}"
    existing = mixture_sample(filt, dthetas, dresp, U, B, S, seed=seed, raster=True)
    sample = mixture_dwell_sample(filt, dthetas, dresp, U, B, S, seed=seed)
    table = mixture_dwell_intervals(filt, dthetas, dresp, U, B, S, seed=seed, sample=sample)
    assert sample["counts"].shape == (S, N) and sample["counts"].dtype == torch.int32
    assert sample["tau"].shape == (S, N) and sample["tau"].dtype == torch.float32
    assert sample["pop"].shape == (S, N) and sample["pop"].dtype == torch.uint8
    for key in ("hist_bound", "hist_unbound"):
        assert sample[key].shape == (S, G, F) and sample[key].dtype == torch.int32
    assert list(table.columns) == INTERVAL_COLUMNS + ["population"] and all(table[c].dtype == np.int64 for c in table.columns)
    pop = existing["pop"].cpu().numpy()
    got, want = to_numpy(sample, table[INTERVAL_COLUMNS]), mdf.oracle_of_populations(existing["raster"].cpu().numpy() >= U, pop, G)
    mdf.assert_equals_population_oracle(got, want, who)
    assert np.array_equal(table["population"].to_numpy(), pop[table["posterior_sample"], table["aoi"]].astype(np.int64))
    # twice the same bits, with and without a given launch A
    again = mixture_dwell_sample(filt, dthetas, dresp, U, B, S, seed=seed)
    for key in sample:
        assert torch.equal(sample[key], again[key]), key
    pd.testing.assert_frame_equal(mixture_dwell_intervals(filt, dthetas, dresp, U, B, S, seed=seed), table)
    # bit-equal to the g++ replay fed the device's filt and resp, where both margins of that replay exceed 1e-9
    host = mdf.host_sample(hk, filt.cpu().numpy(), thetas, resp, U, B, S, seed)
    print(f"{who}, seed {seed}: margins of the replay (population, state) {host['margins']}")
    assert host["margins"].min() > mdf.MARGIN
    for key in ("counts", "hist_bound", "hist_unbound", "tau", "pop"):
        assert np.array_equal(got[key], host[key]), (who, key)
    pd.testing.assert_frame_equal(table[INTERVAL_COLUMNS], host["table"])
    return sample, table, want


# ---- exact replay -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("U,B", UB_LIST)
@pytest.mark.parametrize("G", mdf.G_LIST)
@pytest.mark.parametrize("F", [1, 2, 63, 64, 65, 129])
def test_replay_equals_the_host_functions_on_the_class_raster_of_mixture_sample(hk, U, B, G, F):
    """N = 6 with the special rows; S = 1, one full block of samples, one more, and a third, partly filled block."""
    filt, dthetas, dresp, thetas, resp = inputs(U, B, G, F)
    for S in (1, 64, 65, 130):
        _, _, want = check_replay(hk, filt, dthetas, dresp, thetas, resp, U, B, S, seed=2**40 + F)
        assert (want["tau"][:, 0] == F).all() and (want["tau"][:, 1] == 0).all()  # never and always bound


@pytest.mark.parametrize("U,B", UB_LIST)
def test_many_rows_few_samples_three_populations(hk, U, B):
    check_replay(hk, *inputs(U, B, 3, 203, N=37), U, B, 3, seed=0)


@pytest.mark.parametrize("U,B", UB_LIST)
@pytest.mark.parametrize("F", [1, 2, 63, 64, 65, 129])
def test_one_population_is_tq_chain_dwell_bit_for_bit(U, B, F):
    filt, dthetas, dresp, _, _ = inputs(U, B, 1, F)
    for S in (1, 64, 65, 130):
        seed = 2**40 + F
        got = mixture_dwell_sample(filt, dthetas, dresp, U, B, S, seed=seed)
        want = hmm_dwell_sample(filt[0], dthetas[0], U, B, S, seed=seed)
        for key in ("counts", "tau"):
            assert torch.equal(got[key], want[key]), key
        for key in ("hist_bound", "hist_unbound"):
            assert got[key].shape == (S, 1, F) and torch.equal(got[key][:, 0], want[key]), key
        assert not bool(got["pop"].any())
        table = mixture_dwell_intervals(filt, dthetas, dresp, U, B, S, seed=seed, sample=got)
        pd.testing.assert_frame_equal(table[INTERVAL_COLUMNS], hmm_dwell_intervals(filt[0], dthetas[0], U, B, S, seed=seed))
        assert not table["population"].any()


# ---- guards -----------------------------------------------------------------------------------------------------------
def emit(filt, thetas, resp, U, B, counts, offsets, buffer, total, S, seed):
    """One EMIT launch into ``buffer`` (rows of ``total`` int32) through the entry point itself."""
    G, N, F = filt.shape[:3]
    a = _lib_mixture.PopulationDwellArgs(filt=_lib.ptr(filt), theta=_lib.ptr(thetas), resp=_lib.ptr(resp), counts=_lib.ptr(counts),
                                         offsets=_lib.ptr(offsets), intervals=_lib.ptr(buffer), total=total, N=N, F=F, S=S,
                                         G=G, U=U, B=B, mode=_lib.DWELL_EMIT, seed=seed)
    rc = _lib_mixture.lib().tq_population_dwell(C.byref(a), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("U,B", [(1, 2), (2, 2)])
@pytest.mark.parametrize("F", [2, 65])
def test_short_table_holds_the_first_rows_and_nothing_else(U, B, F):
    S, seed = 70, 0
    filt, dthetas, dresp, _, _ = inputs(U, B, 2, F)
    sample = mixture_dwell_sample(filt, dthetas, dresp, U, B, S, seed=seed)
    table = mixture_dwell_intervals(filt, dthetas, dresp, U, B, S, seed=seed, sample=sample)
    counts = sample["counts"]
    csum = torch.cumsum(counts.reshape(-1).to(torch.int64), 0)
    offsets = (csum - counts.reshape(-1)).contiguous()
    total = len(table) - 1
    buffer = torch.full((_lib.DWELL_COLS + 1, total), -7, dtype=torch.int32, device=DEV)  # the last row is the canary
    assert emit(filt, dthetas, dresp, U, B, counts, offsets, buffer, total, S, seed) == 0
    host = buffer.cpu().numpy()
    assert (host[_lib.DWELL_COLS] == -7).all()
    for i, col in enumerate(INTERVAL_COLUMNS):
        assert np.array_equal(host[i], table[col].to_numpy()[:total]), col
    # an empty table launches nothing
    buffer.fill_(-7)
    assert emit(filt, dthetas, dresp, U, B, counts, offsets, buffer, 0, S, seed) == 0
    assert bool((buffer == -7).all())


# ---- the law of tau ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("U,B", [(1, 2), (2, 2)])
@pytest.mark.parametrize("G", [2, 4])
def test_first_binding_follows_the_exact_survival_law_of_the_mixture(U, B, G):
    """S = 4096, N = 4, F = 129, generator seed 2, theta_g = fixed_theta(U, B, seed=g), phi uniform, resp of the oracle,
    sampler seed 0 (the host test's): within 5 binomial sigma of sum_g resp[g, n] S_g(n, f) wherever that lies in
    [0.02, 0.98]; at least 50 such points."""
    S, N, F = 4096, 4, 129
    p = mf.synthetic_hmm(N, F, 2)[0]
    thetas = np.array([mf.fixed_theta(U, B, seed=g) for g in range(G)])
    resp = np.asarray(mf.oracle_final(p, mf.PRIOR, thetas, np.full(G, 1.0 / G), U, B)[1], np.float64)
    got = mixture_dwell_sample(device_filt(p, thetas, U, B), dev(thetas), dev(resp), U, B, S, seed=0)
    tau = got["tau"].cpu().numpy()
    assert tau.min() >= 0 and tau.max() <= F and np.array_equal(tau, np.rint(tau))
    points, deviation = survival_deviation(tau, mdf.mixture_survival(p, thetas, resp, U, B, mf.PRIOR))
    print(f"({U}, {B}) G = {G}: {points} points, largest deviation {deviation:.2f} sigma, winning responsibilities "
          f"{resp.max(0).round(3)}")
    assert points >= 50
    assert deviation <= 5.0


# ---- the conditions -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,s", [("XY", 0), ("XY", 1), ("XI", 0), ("XI", 1)])
def test_population_rasters_mend_what_the_single_chain_pools(kind, s):
    """The conditions of section 30 on the device: 150 EM iterations (tol 0) from the default start, S = 64, sampler seed 0;
    the (1, 1) single chain's rasters pooled through ``tq_chain_dwell``."""
    S = 64
    p = dev(mf.static_data(kind, s)[0])
    mix = mixture_fit(p, mf.PRIOR, 1, 1, populations=2, num_iter=150, tol=0.0, chunk=150)
    one = hmm_fit(p, mf.PRIOR, 1, 1, num_iter=150, tol=0.0, chunk=150)
    assert mix["iterations"][mix["best"]] == 150 and one["iterations"] == 150
    mixture = mixture_dwell_sample(mix["filt"], mix["thetas"], mix["resp"], 1, 1, S, seed=0)
    single = hmm_dwell_sample(one["filt"], one["theta"], 1, 1, S, seed=0)
    figures = mdf.condition_figures(kind, s, {k: v.cpu().numpy() for k, v in mixture.items()},
                                    {k: v.cpu().numpy() for k, v in single.items()}, mix["resp"].cpu().numpy())
    mdf.check_conditions(kind, s, figures, "device")


# ---- command line -------------------------------------------------------------------------------------------------
def test_fit_smooth_and_the_population_kinetics_end_to_end(tmp_path):
    runner = CliRunner()
    N, F, S, G = 8, 40, 8, 2
    params = {k: v for k, v in TEST_PARAMS.items() if k != "pi"}
    params.update(kon=0.1, koff=0.2)
    save(simulate(2, N, F, 1, 14, params=params), tmp_path)

    def run(*args):
        return runner.invoke(app, ["--cd", str(tmp_path), *args, "--cuda", "--no-input"])

    def files():
        """Every file of the directory but the .mat tables, whose header carries the time of writing."""
        return {f.name: f.read_bytes() for f in tmp_path.iterdir() if f.is_file() and f.suffix != ".mat"}

    result = run("fit", "--model", "cosmos", "--nbatch-size", "8", "--fbatch-size", "40", "--num-iter", "2")
    assert result.exit_code == 0, result.output
    # two iterations leave a posterior without a single interior interval: the on-target p(z = 1) of the fit's file is
    # replaced by that of two fast and two slow AOIs of the fixture's generator, so that both kinds of fit have data
    n_on = N // 2  # simulate: the first half of the AOIs are on target, all selected by the mask
    fitted = load_tpqr(tmp_path / "cosmos_params.tpqr")
    p = np.concatenate([mf.synthetic_hmm(2, F, 0, A=mf.two_state(0.3, 0.4))[0], mf.synthetic_hmm(2, F, 100, A=mf.two_state(0.1, 0.1))[0]])
    fitted["z_probs"][:n_on, :, 0, 1] = torch.from_numpy(p).to(fitted["z_probs"].dtype)
    fitted["z_probs"][:n_on, :, 0, 0] = 1.0 - fitted["z_probs"][:n_on, :, 0, 1]
    torch.save(fitted, tmp_path / "cosmos_params.tpqr")
    result = run("smooth", "--num-samples", "50", "--num-iter", "30")
    assert result.exit_code == 0, result.output
    dwell_args = ("dwelltime", "-K", "1", "--num-samples", str(S), "--num-iter", "50")
    ttfb_args = ("ttfb", "--num-samples", str(S), "--num-iter", "50")
    pops = ("--smooth", "--populations", "2")
    # the mixture has to be fitted first
    for args in (dwell_args, ttfb_args):
        result = run(*args, *pops)
        assert result.exit_code == 1 and "run `smooth --populations 2` first" in result.output, result.output
        result = run(*args, *pops, "--bound-states", "2")
        assert result.exit_code == 1, result.output
        assert "run `smooth --unbound-states 1 --bound-states 2 --populations 2` first" in result.output, result.output
    result = run("smooth", "--populations", "2", "--num-samples", "50", "--num-iter", "30")
    assert result.exit_code == 0, result.output
    # the option at one population is today's code path: the same bytes as without it
    for args in (dwell_args, ttfb_args):
        result = run(*args, "--smooth")
        assert result.exit_code == 0, result.output
    plain = files()
    for args in (dwell_args, ttfb_args):
        result = run(*args, "--smooth", "--populations", "1")
        assert result.exit_code == 0, result.output
    again = files()
    assert sorted(again) == sorted(plain)
    for name, content in plain.items():
        assert again[name] == content, name

    before = files()
    assert "cosmos_smooth-u1b1g2.tpqr" in before and "cosmos_dwelltime-smooth-intervals-channel0.pkl" in before
    result = run(*dwell_args, *pops)
    assert result.exit_code == 0, result.output
    result = run(*ttfb_args, *pops)
    assert result.exit_code == 0, result.output
    after = files()
    for name, content in before.items():
        assert after[name] == content, name
    new = sorted(set(after) - set(before))
    assert new and all(name.startswith(("cosmos_dwelltime-smooth-u1b1g2-", "cosmos_ttfb-smooth-u1b1g2-")) for name in new), new

    table = pd.read_pickle(tmp_path / "cosmos_dwelltime-smooth-u1b1g2-intervals-channel0.pkl")
    assert list(table.columns) == INTERVAL_COLUMNS + ["population"] and all(table[c].dtype == np.int64 for c in table.columns)
    assert set(table["posterior_sample"]) == set(range(S)) and set(table["aoi"]) == set(range(n_on))
    assert table.groupby(["posterior_sample", "aoi"])["dwell_time"].sum().eq(F).all()
    assert set(table["z"]) <= {0, 1} and set(table["population"]) <= set(range(G))
    assert table.groupby(["posterior_sample", "aoi"])["population"].nunique().eq(1).all()  # one population per row
    drawn = set(table["population"])
    for rate, z in (("koff", 1), ("kon", 0)):
        res = pd.read_csv(tmp_path / f"cosmos_dwelltime-smooth-u1b1g2-{rate}-channel0.csv", index_col=0)
        assert list(res.columns) == ["Mean", "95% LL", "95% UL"] and np.isfinite(res.values).all()
        # a population has its two rows exactly when some sample has an interior interval of the kind in it
        interior = table[(table["z"] == z) & (table["start_frame"] > 0) & (table["stop_frame"] < F - 1)]
        assert interior["low_or_high"].isin([0, 1]).all()
        fitted_pops = sorted(set(interior["population"]))
        assert fitted_pops and set(fitted_pops) <= drawn
        assert list(res.index) == [f"g{g}_{key}0" for g in fitted_pops for key in ("A", rate)]
        if importlib.util.find_spec("matplotlib") is not None:
            kind = "bound" if z else "unbound"
            for g in fitted_pops:
                assert (tmp_path / f"cosmos_dwelltime-smooth-u1b1g2-g{g}-{kind}-histogram-channel0.png").is_file()
    tau = pd.read_csv(tmp_path / "cosmos_ttfb-smooth-u1b1g2-data-points-channel0.csv", index_col=0).to_numpy()
    assert tau.shape == (S, n_on) and tau.min() >= 0 and tau.max() <= F
    res = pd.read_csv(tmp_path / "cosmos_ttfb-smooth-u1b1g2-params-channel0.csv", index_col=0)
    assert list(res.index) == ["ka", "kns", "Af"] and np.isfinite(res.values).all()
    assert (tmp_path / "cosmos_ttfb-smooth-u1b1g2-fraction-bound-channel0.csv").is_file()
    # both commands walk the same rasters: the table's first-binding frames are ttfb's data points
    first = table[table["z"] == 1].groupby(["posterior_sample", "aoi"])["start_frame"].min()
    want = np.full((S, n_on), float(F))
    want[first.index.get_level_values(0), first.index.get_level_values(1)] = first.to_numpy()
    assert np.array_equal(tau, want)
    # the populations file against the table's population column and the data points
    split = pd.read_csv(tmp_path / "cosmos_ttfb-smooth-u1b1g2-populations-channel0.csv", index_col=0)
    assert list(split.columns) == ["Mean", "95% LL", "95% UL"]
    labels = [f"g{g}_{key}" for g in range(G) for key in ("share", "never_bound", "first_binding")]
    assert list(split.index) == labels + [f"g{g}_fraction_bound_{t}" for g in range(G) for t in range(F)]
    pop = np.zeros((S, n_on), np.int64)
    rows = table.drop_duplicates(["posterior_sample", "aoi"])
    pop[rows["posterior_sample"], rows["aoi"]] = rows["population"]
    share = np.stack([(pop == g).mean(1) for g in range(G)], 1)  # (S, G)
    assert np.allclose(split.loc[[f"g{g}_share" for g in range(G)], "Mean"].to_numpy(), share.mean(0), atol=1e-12)
    assert abs(split.loc[[f"g{g}_share" for g in range(G)], "Mean"].sum() - 1.0) < 1e-12
    for g in range(G):
        members = (pop == g).sum(1)
        never = ((pop == g) & (tau == F)).sum(1)[members > 0] / members[members > 0]
        if len(never):
            assert abs(split.loc[f"g{g}_never_bound", "Mean"] - never.mean()) < 1e-12
            fb = np.array([(((pop == g) & (tau < t)).sum(1)[members > 0] / members[members > 0]).mean() for t in range(F)])
            assert np.allclose(split.loc[[f"g{g}_fraction_bound_{t}" for t in range(F)], "Mean"].to_numpy(), fb, atol=1e-6)
    # the sampled share of every population follows the stored responsibilities
    sm = load_tpqr(tmp_path / "cosmos_smooth-u1b1g2.tpqr")
    resp = sm["population_probs"][:n_on, :, 0].numpy()  # (N_on, G)
    sigma = np.sqrt((resp * (1 - resp)).sum(0) / S) / n_on + 1e-12
    assert (np.abs(share.mean(0) - resp.mean(0)) <= 6 * sigma).all(), (share.mean(0), resp.mean(0), sigma)

    # (1, 2) with two populations, after its `smooth`
    result = run("smooth", "--bound-states", "2", "--populations", "2", "--num-samples", "50", "--num-iter", "30")
    assert result.exit_code == 0, result.output
    before = files()
    result = run(*dwell_args, *pops, "--bound-states", "2")
    assert result.exit_code == 0, result.output
    after = files()
    for name, content in before.items():
        assert after[name] == content, name
    new = sorted(set(after) - set(before))
    assert new and all(name.startswith("cosmos_dwelltime-smooth-u1b2g2-") for name in new), new
    table = pd.read_pickle(tmp_path / "cosmos_dwelltime-smooth-u1b2g2-intervals-channel0.pkl")
    assert list(table.columns) == INTERVAL_COLUMNS + ["population"] and set(table["z"]) <= {0, 1}

    payload = load_tpqr(tmp_path / "data.tpqr")
    payload["mask"][1] = False  # another selection of AOIs than `smooth` saw
    torch.save(payload, tmp_path / "data.tpqr")
    result = run(*ttfb_args, *pops)
    assert result.exit_code == 1 and "mask" in result.output, result.output
