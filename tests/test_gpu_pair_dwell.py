"""``tq_pair_dwell`` on the MI355X: counts, first-binding frames, the partner's first bound frame from
there on, the interval table with the partner's state at the ends of every run and the histograms by the partner's state at
a run's start, exactly equal to the oracle of pair_dwell_fixture on the raster of joint states that the existing
``hmm_sample(..., 2, 2, raster=True)`` writes for the same inputs and seed, and bit-equal to the g++ replay fed the device's
``filt``; channel b bit-equal to ``tq_chain_dwell`` at (2, 2); the guards of the EMIT launch; the condition of the section;
and ``fit``, ``smooth``, ``smooth --joint 0,1``, ``dwelltime --smooth --joint 0,1``, ``ttfb --smooth --joint 0,1`` end to
end."""

import ctypes as C

import numpy as np
import pandas as pd
import pytest
import torch
from typer.testing import CliRunner

import joint_fixture as jf
import pair_dwell_fixture as pdf
from helpers import make_dataset
from tapqir_amd import _lib, _lib_joint
from tapqir_amd.main import app
from tapqir_amd.utils.dataset import save
from tapqir_amd.utils.imscroll import INTERVAL_COLUMNS
from tapqir_amd.utils.joint_analysis import (ORDER_NAMES, joint_arrival_order, joint_dwell_intervals, joint_dwell_sample,
                                             joint_estep, joint_fit, joint_start_from)
from tapqir_amd.utils.mle_analysis import hmm_dwell_intervals, hmm_dwell_sample, hmm_sample, smooth_fit
from tapqir_amd.utils.safe_load import load_tpqr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
COLUMNS = INTERVAL_COLUMNS + pdf.PARTNER_COLUMNS


@pytest.fixture(scope="module")
def hk(tmp_path_factory):
    return pdf.build_pair_dwell_check(tmp_path_factory.mktemp("pair_dwell"))


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def inputs(F, N=6):
    """The inputs of the host test with the device's own filt: N = 6 with the special rows of both channels, or N rows of
    the driven chain; theta = ``fixed_theta()``."""
    pa, pb = jf.estep_inputs(N, F, seed=F) if N == 6 else jf.synthetic_joint(N, F, F, jf.A_DRIVEN)[:2]
    theta = jf.fixed_theta()
    filt = joint_estep(dev(pa), dev(pb), dev(theta[None]), *jf.PRIORS)["filt"][0].contiguous()
    return filt, dev(theta), theta


def to_numpy(sample, table):
    """The device's outputs as the oracle's keys: the partner code is put together again from the four columns."""
    code = sum(np.maximum(table[name].to_numpy(), 0) << bit for bit, name in enumerate(pdf.PARTNER_COLUMNS))
    return {**{k: v.cpu().numpy() for k, v in sample.items()}, "table": table[INTERVAL_COLUMNS], "partner": code.astype(np.uint8)}


def check_replay(hk, filt, dtheta, theta, which, S, seed):
    N, F = filt.shape[:2]
    who = f"which = {which}, S = {S}, N = {N}, F = {F}"
    raster = hmm_sample(filt, dtheta, 2, 2, S, seed=seed, raster=True)["raster"].cpu().numpy()
    sample = joint_dwell_sample(filt, dtheta, which, S, seed=seed)
    table = joint_dwell_intervals(filt, dtheta, which, S, seed=seed, sample=sample)
    assert set(sample) == {"hist_bound", "hist_unbound", "counts", "tau", "tau_after"}
    assert sample["counts"].shape == (S, N) and sample["counts"].dtype == torch.int32
    for key in ("tau", "tau_after"):
        assert sample[key].shape == (S, N) and sample[key].dtype == torch.float32
    for key in ("hist_bound", "hist_unbound"):
        assert sample[key].shape == (S, 2, F) and sample[key].dtype == torch.int32
    assert list(table.columns) == COLUMNS and all(table[c].dtype == np.int64 for c in table.columns)
    got, want = to_numpy(sample, table), pdf.oracle_of_states(raster, which)
    pdf.assert_equals_pair_oracle(got, want, who)
    for name in pdf.PARTNER_COLUMNS:  # -1 where the record has no such frame
        assert np.array_equal(table[name].to_numpy(), want[name]), (who, name)
    # twice the same bits, with and without a given launch A
    again = joint_dwell_sample(filt, dtheta, which, S, seed=seed)
    for key in sample:
        assert torch.equal(sample[key], again[key]), key
    pd.testing.assert_frame_equal(joint_dwell_intervals(filt, dtheta, which, S, seed=seed), table)
    # channel b is the class of tq_chain_dwell at (2, 2): the same bits
    if which == 1:
        chain = hmm_dwell_sample(filt, dtheta, 2, 2, S, seed=seed)
        for key in ("counts", "tau"):
            assert torch.equal(sample[key], chain[key]), (who, key)
        for key in ("hist_bound", "hist_unbound"):
            assert torch.equal(sample[key].sum(1, dtype=torch.int32), chain[key]), (who, key)
        pd.testing.assert_frame_equal(table[INTERVAL_COLUMNS], hmm_dwell_intervals(filt, dtheta, 2, 2, S, seed=seed))
    # bit-equal to the g++ replay fed the device's filt, where the smallest |u - t| of that replay exceeds 1e-9
    host = pdf.host_sample(hk, filt.cpu().numpy(), theta, which, S, seed)
    print(f"{who}, seed {seed}: smallest |u - t| of the replay {host['margin']:.3g}")
    assert host["margin"] > pdf.MARGIN
    for key in ("counts", "hist_bound", "hist_unbound", "tau", "tau_after", "partner"):
        assert np.array_equal(got[key], host[key]), (who, key)
    pd.testing.assert_frame_equal(table[INTERVAL_COLUMNS], host["table"])
    return sample, table, want


# ---- exact replay -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("F", [1, 2, 63, 64, 65, 129])
def test_replay_equals_the_oracle_on_the_raster_of_hmm_sample(hk, which, F):
    """N = 6 with the special rows; S = 1, one full block of samples, one more, and a third, partly filled block."""
    filt, dtheta, theta = inputs(F)
    for S in (1, 64, 65, 130):
        check_replay(hk, filt, dtheta, theta, which, S, seed=2**40 + F)


@pytest.mark.parametrize("which", [0, 1])
def test_many_rows_few_samples(hk, which):
    check_replay(hk, *inputs(203, N=37), which, 3, seed=0)


# ---- guards -----------------------------------------------------------------------------------------------------------
def emit(filt, theta, which, counts, offsets, table, codes, total, S, seed):
    """One EMIT launch into ``table`` (rows of ``total`` int32) and ``codes`` through the entry point itself."""
    N, F = filt.shape[:2]
    a = _lib_joint.PairDwellArgs(filt=_lib.ptr(filt), theta=_lib.ptr(theta), counts=_lib.ptr(counts), offsets=_lib.ptr(offsets),
                                 intervals=_lib.ptr(table), partner=_lib.ptr(codes), total=total, N=N, F=F, S=S, which=which,
                                 mode=_lib.DWELL_EMIT, seed=seed)
    rc = _lib_joint.lib().tq_pair_dwell(C.byref(a), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("F", [2, 65])
def test_short_table_holds_the_first_rows_and_nothing_else(which, F):
    S, seed = 70, 0
    filt, dtheta, _ = inputs(F)
    sample = joint_dwell_sample(filt, dtheta, which, S, seed=seed)
    full = joint_dwell_intervals(filt, dtheta, which, S, seed=seed, sample=sample)
    counts = sample["counts"]
    csum = torch.cumsum(counts.reshape(-1).to(torch.int64), 0)
    offsets = (csum - counts.reshape(-1)).contiguous()
    total = len(full) - 1
    table = torch.full((_lib.DWELL_COLS + 1, total), -7, dtype=torch.int32, device=DEV)  # the last row is the canary
    codes = torch.full((total + 8,), 0xEE, dtype=torch.uint8, device=DEV)  # and the last eight entries
    assert emit(filt, dtheta, which, counts, offsets, table, codes, total, S, seed) == 0
    host, host_codes = table.cpu().numpy(), codes.cpu().numpy().astype(np.int64)
    assert (host[_lib.DWELL_COLS] == -7).all() and (host_codes[total:] == 0xEE).all()
    for i, col in enumerate(INTERVAL_COLUMNS):
        assert np.array_equal(host[i], full[col].to_numpy()[:total]), col
    for bit, name in enumerate(pdf.PARTNER_COLUMNS):
        assert np.array_equal((host_codes[:total] >> bit) & 1, np.maximum(full[name].to_numpy()[:total], 0)), name
    # an empty table launches nothing
    table.fill_(-7)
    codes.fill_(0xEE)
    assert emit(filt, dtheta, which, counts, offsets, table, codes, 0, S, seed) == 0
    assert bool((table == -7).all()) and bool((codes == 0xEE).all())


# ---- the condition ------------------------------------------------------------------------------------------------------
def test_partner_split_recovers_what_the_pooled_histogram_hides():
    """The condition of section 32 on the device: the driven chain N = 40, F = 500, seed 0; two-state fits of 50 EM
    iterations per channel from (0.5, 0.5, 0.5), then 50 EM iterations (tol 0) of ``a-drives-b`` from their Kronecker
    product; S = 64, sampler seed 0, channel b; the pooled figure through ``tq_chain_dwell`` at (2, 2) on the same filt.
    The g++ build measures q = 0 38.931 (ratio 0.084), q = 1 21.527 (ratio 0.086), pooled 30.690."""
    S = 64
    pa, pb, _ = pdf.driven_case()
    pa, pb = dev(pa), dev(pb)
    two = [smooth_fit(p, prior, num_iter=50, tol=0.0)["theta"] for p, prior in zip((pa, pb), jf.PRIORS)]
    fit = joint_fit(pa, pb, *jf.PRIORS, structures=["a-drives-b"], start=joint_start_from(*two), num_iter=50, tol=0.0)
    assert fit["fits"][0]["iterations"] == 50 and fit["chosen"] == 1
    filt, theta = fit["filt"], fit["theta"]
    b = joint_dwell_sample(filt, theta, 1, S, seed=0)
    a = joint_dwell_sample(filt, theta, 0, S, seed=0)
    pooled = hmm_dwell_sample(filt, theta, 2, 2, S, seed=0)
    pdf.check_condition(b["hist_unbound"].cpu().numpy(), pooled["hist_unbound"].cpu().numpy(), "device")
    order = joint_arrival_order(a["tau"], a["tau_after"], b["tau"], 500)
    events = (order["later"] * order["binds"] * 40).mean().item()
    hb = b["hist_bound"].cpu().numpy()
    print(f"device: k_after / k_base = {order['ratio'].mean().item():.3f} from {events:.1f} events a sample (hidden raster: "
          f"1.4 from 29); bound dwells of b by q: {pdf.interior_means(hb[:, 0]):.3f} / {pdf.interior_means(hb[:, 1]):.3f} "
          f"(hidden 12.38 / 12.19)")
    assert bool(torch.isfinite(order["ratio"]).all())


# ---- command line -------------------------------------------------------------------------------------------------
def test_fit_smooth_and_the_joint_kinetics_end_to_end(tmp_path):
    runner = CliRunner()
    N, F, S = 8, 40, 8
    save(make_dataset(N=N, F=F, C=2), tmp_path)

    def run(*args):
        return runner.invoke(app, ["--cd", str(tmp_path), *args, "--cuda", "--no-input"])

    def files():
        """Every file of the directory but the .mat tables, whose header carries the time of writing."""
        return {f.name: f.read_bytes() for f in tmp_path.iterdir() if f.is_file() and f.suffix != ".mat"}

    result = run("fit", "--model", "cosmos", "--nbatch-size", "8", "--fbatch-size", "40", "--num-iter", "2")
    assert result.exit_code == 0, result.output
    # two iterations leave a posterior without a single interior interval: the on-target p(z = 1) of the fit's file is
    # replaced, in both channels, by that of the driven chain of the fixture's generator
    n_on = N // 2  # simulate: the first half of the AOIs are on target, all selected by the mask
    fitted = load_tpqr(tmp_path / "cosmos_params.tpqr")
    for c, p in enumerate(jf.synthetic_joint(n_on, F, 0, jf.driven_chain(0.02, 0.3, 0.2))[:2]):
        fitted["z_probs"][:n_on, :, c, 1] = torch.from_numpy(p).to(fitted["z_probs"].dtype)
        fitted["z_probs"][:n_on, :, c, 0] = 1.0 - fitted["z_probs"][:n_on, :, c, 1]
    torch.save(fitted, tmp_path / "cosmos_params.tpqr")
    result = run("smooth", "--num-samples", "50", "--num-iter", "30")
    assert result.exit_code == 0, result.output
    dwell_args = ("dwelltime", "-K", "1", "--num-samples", str(S), "--num-iter", "50")
    ttfb_args = ("ttfb", "--num-samples", str(S), "--num-iter", "50")
    pair = ("--smooth", "--joint", "0,1")
    # the joint chain has to be fitted first
    for args in (dwell_args, ttfb_args):
        result = run(*args, *pair)
        assert result.exit_code == 1 and "run `smooth --joint 0,1` first" in result.output, result.output
    result = run("smooth", "--joint", "0,1", "--num-samples", "50", "--num-iter", "30")
    assert result.exit_code == 0, result.output
    result = run(*dwell_args, "--smooth")
    assert result.exit_code == 0, result.output

    before = files()
    assert "cosmos_smooth-joint01.tpqr" in before and "cosmos_dwelltime-smooth-intervals-channel0.pkl" in before
    result = run(*dwell_args, *pair)
    assert result.exit_code == 0, result.output
    result = run(*ttfb_args, *pair)
    assert result.exit_code == 0, result.output
    after = files()
    for name, content in before.items():
        assert after[name] == content, name
    stem = "cosmos_dwelltime-smooth-joint01-"
    new = set(after) - set(before)
    assert {f"{stem}intervals-channel{c}.pkl" for c in (0, 1)} | {"cosmos_ttfb-smooth-joint01-order.csv"} <= new
    assert all(name.startswith(stem) or name == "cosmos_ttfb-smooth-joint01-order.csv" for name in new), new
    assert not any(name.endswith(".png") for name in new)  # no plots

    tables = {}
    for c in (0, 1):
        table = tables[c] = pd.read_pickle(tmp_path / f"{stem}intervals-channel{c}.pkl")
        assert list(table.columns) == COLUMNS and all(table[col].dtype == np.int64 for col in table.columns)
        assert set(table["posterior_sample"]) == set(range(S)) and set(table["aoi"]) == set(range(n_on))
        assert table.groupby(["posterior_sample", "aoi"])["dwell_time"].sum().eq(F).all()
        assert set(table["z"]) <= {0, 1}
        assert ((table["partner_before"] == -1) == (table["start_frame"] == 0)).all()
        assert ((table["partner_after"] == -1) == (table["stop_frame"] == F - 1)).all()
        assert set(table["partner_start"]) <= {0, 1} and set(table["partner_stop"]) <= {0, 1}
        for rate, z in (("koff", 1), ("kon", 0)):
            # a partner state has its two rows exactly when some sample has an interior interval of the kind that starts in it
            interior = table[(table["z"] == z) & (table["start_frame"] > 0) & (table["stop_frame"] < F - 1)]
            fitted_q = sorted(set(interior["partner_start"]))
            path = tmp_path / f"{stem}{rate}-channel{c}.csv"
            assert path.is_file() == bool(fitted_q)
            if fitted_q:
                res = pd.read_csv(path, index_col=0)
                assert list(res.columns) == ["Mean", "95% LL", "95% UL"] and np.isfinite(res.values).all()
                assert list(res.index) == [f"q{q}_{key}0" for q in fitted_q for key in ("A", rate)]
    assert any((tmp_path / f"{stem}{rate}-channel{c}.csv").is_file() for rate in ("koff", "kon") for c in (0, 1))

    # the two tables describe the same rasters: where a run of channel 0 starts, the table of channel 1 has a run over that
    # frame whose label is the partner state the first table gives
    other = tables[1].set_index(["posterior_sample", "aoi"]).sort_index()
    for _, row in tables[0].head(200).iterrows():
        runs = other.loc[(row["posterior_sample"], row["aoi"])]
        runs = runs if isinstance(runs, pd.DataFrame) else runs.to_frame().T
        over = runs[(runs["start_frame"] <= row["start_frame"]) & (runs["stop_frame"] >= row["start_frame"])]
        assert len(over) == 1 and int(over["z"].iloc[0]) == row["partner_start"]

    order = pd.read_csv(tmp_path / "cosmos_ttfb-smooth-joint01-order.csv", index_col=0)
    assert list(order.columns) == ["Mean", "95% LL", "95% UL"]
    assert list(order.index) == [f"{lead}_{key}" for lead in ("a", "b") for key in ORDER_NAMES]
    # the lead's share of binding rows against the tables' first bound runs
    for lead, c in (("a", 0), ("b", 1)):
        bound = tables[c][tables[c]["z"] == 1].groupby(["posterior_sample", "aoi"]).ngroups
        assert abs(order.loc[f"{lead}_binds", "Mean"] - bound / (S * n_on)) < 1e-12
        shares = order.loc[[f"{lead}_{key}" for key in ("together", "later", "never")], "Mean"]
        assert shares.notna().all() and 0 <= shares.min() and shares.max() <= 1

    payload = load_tpqr(tmp_path / "data.tpqr")
    payload["mask"][1] = False  # another selection of AOIs than `smooth --joint` saw
    torch.save(payload, tmp_path / "data.tpqr")
    for args in (dwell_args, ttfb_args):
        result = run(*args, *pair)
        assert result.exit_code == 1 and "mask" in result.output, result.output
    (tmp_path / "cosmos_smooth-joint01.tpqr").unlink()
    for args in (dwell_args, ttfb_args):
        result = run(*args, *pair)
        assert result.exit_code == 1 and "run `smooth --joint 0,1` first" in result.output, result.output
