"""``tq_chain_dwell`` on the MI355X: counts, interior histograms, first-binding frames and the
interval table exactly equal to the host functions of ``tapqir_amd.utils.imscroll`` on the class view of the raster that
the existing ``hmm_sample(..., raster=True)`` writes for the same ``filt``, ``theta``, U, B and seed, and bit-equal to the
g++ replay fed the device's ``filt``; the guards of the EMIT launch; the three conditions of the section; and ``fit``,
``smooth``, ``smooth --bound-states 2``, ``dwelltime --smooth [--bound-states 2]``, ``ttfb --smooth --bound-states 2`` end to
end."""

import ctypes as C

import numpy as np
import pandas as pd
import pytest
import torch
from typer.testing import CliRunner

from hmm_dwell_fixture import (MARGIN, PRIOR, UB_LIST, build_hmm_dwell_check, check_what_it_is_for, host_sample,
                               oracle_survival)
from hmm_fixture import fixed_theta, synthetic_hmm, with_special_rows
from smooth_dwell_fixture import assert_equals_oracle, n01_of_table, oracle_of_raster, survival_deviation
from tapqir_amd import _lib, _lib_hmm
from tapqir_amd.main import app
from tapqir_amd.utils.dataset import save
from tapqir_amd.utils.imscroll import INTERVAL_COLUMNS
from tapqir_amd.utils.mle_analysis import (dwell_csr_from_hist, dwell_fit, dwell_sample, hmm_dwell_intervals,
                                           hmm_dwell_sample, hmm_estep, hmm_fit, hmm_sample, ttfb_fit, ttfb_sample)
from tapqir_amd.utils.safe_load import load_tpqr
from tapqir_amd.utils.simulate import TEST_PARAMS, simulate

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def hk(tmp_path_factory):
    return build_hmm_dwell_check(tmp_path_factory.mktemp("hmm_dwell"))


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def to_numpy(sample, table):
    return {**{k: v.cpu().numpy() for k, v in sample.items()}, "table": table}


def replay(p, theta, U, B, S, seed):
    """The device's filt, the raster of the existing sampler with its counts, and both launches of the new one."""
    theta = dev(theta)
    filt = hmm_estep(dev(p), theta, PRIOR, U, B)["filt"]
    existing = hmm_sample(filt, theta, U, B, S, seed=seed, raster=True)
    sample = hmm_dwell_sample(filt, theta, U, B, S, seed=seed)
    table = hmm_dwell_intervals(filt, theta, U, B, S, seed=seed, sample=sample)
    return filt, theta, existing["counts"].cpu().numpy(), existing["raster"].cpu().numpy(), sample, table


def check_replay(hk, p, theta, U, B, S, seed):
    N, F = p.shape
    who = f"({U}, {B}) S = {S}, N = {N}, F = {F}"
    filt, dtheta, counts4, raster, sample, table = replay(p, theta, U, B, S, seed)
    assert sample["counts"].shape == (S, N) and sample["counts"].dtype == torch.int32
    assert sample["tau"].shape == (S, N) and sample["tau"].dtype == torch.float32
    for key in ("hist_bound", "hist_unbound"):
        assert sample[key].shape == (S, F) and sample[key].dtype == torch.int32
    assert all(table[c].dtype == np.int64 for c in INTERVAL_COLUMNS)
    got, want = to_numpy(sample, table), oracle_of_raster(raster >= U)
    assert_equals_oracle(got, want, who)
    assert np.array_equal(n01_of_table(table, S, N), counts4[..., 0])
    # twice the same bits, with and without a given launch A
    again = hmm_dwell_sample(filt, dtheta, U, B, S, seed=seed)
    for key in sample:
        assert torch.equal(sample[key], again[key]), key
    pd.testing.assert_frame_equal(hmm_dwell_intervals(filt, dtheta, U, B, S, seed=seed), table)
    # bit-equal to the g++ replay fed the device's filt, where no uniform of that replay lies within 1e-9 of a threshold
    host = host_sample(hk, filt.cpu().numpy(), theta, U, B, S, seed)
    print(f"{who}, seed {seed}: smallest |u - t| of the replay {host['margin']:.3g}")
    assert host["margin"] > MARGIN
    for key in ("counts", "hist_bound", "hist_unbound", "tau"):
        assert np.array_equal(got[key], host[key]), (who, key)
    pd.testing.assert_frame_equal(table, host["table"])
    return want


# ---- exact replay -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("U,B", UB_LIST)
@pytest.mark.parametrize("F", [1, 2, 63, 64, 65, 129])
def test_replay_equals_the_host_functions_on_the_class_raster_of_hmm_sample(hk, U, B, F):
    """N = 6 with the special rows; S = 1, one full block of samples, one more, and a third, partly filled block."""
    p = with_special_rows(synthetic_hmm(6, F, seed=F)[0], PRIOR)
    for S in (1, 64, 65, 130):
        want = check_replay(hk, p, fixed_theta(U, B), U, B, S, seed=2**40 + F)
        assert (want["tau"][:, 0] == F).all() and (want["tau"][:, 1] == 0).all()  # never and always bound


@pytest.mark.parametrize("U,B", UB_LIST)
def test_many_rows_few_samples(hk, U, B):
    check_replay(hk, synthetic_hmm(37, 203, seed=3)[0], fixed_theta(U, B), U, B, 3, seed=0)


# ---- guards -----------------------------------------------------------------------------------------------------------
def emit(filt, theta, U, B, counts, offsets, buffer, total, S, seed):
    """One EMIT launch into ``buffer`` (rows of ``total`` int32) through the entry point itself."""
    N, F = filt.shape[:2]
    a = _lib_hmm.ChainDwellArgs(filt=_lib.ptr(filt), theta=_lib.ptr(theta), counts=_lib.ptr(counts),
                                offsets=_lib.ptr(offsets), intervals=_lib.ptr(buffer), total=total, N=N, F=F, S=S, U=U, B=B,
                                mode=_lib.DWELL_EMIT, seed=seed)
    rc = _lib_hmm.lib().tq_chain_dwell(C.byref(a), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("U,B", [(1, 2), (2, 2)])
@pytest.mark.parametrize("F", [2, 65])
def test_short_table_holds_the_first_rows_and_nothing_else(U, B, F):
    S, seed = 70, 0
    p = with_special_rows(synthetic_hmm(6, F, seed=F)[0], PRIOR)
    filt, theta, _, raster, sample, table = replay(p, fixed_theta(U, B), U, B, S, seed)
    counts = sample["counts"]
    csum = torch.cumsum(counts.reshape(-1).to(torch.int64), 0)
    offsets = (csum - counts.reshape(-1)).contiguous()
    total = len(table) - 1
    buffer = torch.full((_lib.DWELL_COLS + 1, total), -7, dtype=torch.int32, device=DEV)  # the last row is the canary
    assert emit(filt, theta, U, B, counts, offsets, buffer, total, S, seed) == 0
    host = buffer.cpu().numpy()
    assert (host[_lib.DWELL_COLS] == -7).all()
    for i, col in enumerate(INTERVAL_COLUMNS):
        assert np.array_equal(host[i], table[col].to_numpy()[:total]), col
    # an empty table launches nothing
    buffer.fill_(-7)
    assert emit(filt, theta, U, B, counts, offsets, buffer, 0, S, seed) == 0
    assert bool((buffer == -7).all())


# ---- the conditions -----------------------------------------------------------------------------------------------------
def test_multi_state_rasters_mend_what_two_states_leave():
    """Conditions 1 and 2 of section 25 (see the host test), with the device's EM and independent draws from
    ``dwell_sample`` / ``ttfb_sample``; hidden = the fixture's true raster."""
    S = 64
    p_host, states = synthetic_hmm(40, 500, seed=0)
    p = dev(p_host)
    chains = {}
    for U, B in ((1, 1), (1, 2)):
        fit = hmm_fit(p, PRIOR, U, B, num_iter=50, tol=0.0)
        assert fit["iterations"] == 50
        chains[U, B] = hmm_dwell_sample(fit["filt"], fit["theta"], U, B, S, seed=0)
        print(f"({U}, {B}): {int(chains[U, B]['counts'].sum()) / S:.0f} intervals per raster")
    independent = {**dwell_sample(p, S, seed=0), "tau": ttfb_sample(p, S, seed=0)}
    as_numpy = [{k: x[k].cpu().numpy() for k in ("hist_bound", "hist_unbound", "tau")}
                for x in (independent, chains[1, 1], chains[1, 2])]
    check_what_it_is_for(oracle_of_raster((states >= 1)[None]), *as_numpy)
    # the outputs plug into the fits unchanged
    k = dwell_fit(dwell_csr_from_hist(chains[1, 2]["hist_bound"]), 2, n_steps=200)["k"]
    ka = ttfb_fit(chains[1, 2]["tau"], 500, n_steps=200)["ka"]
    assert k.shape == (S, 2) and ka.shape == (S, 1) and bool(torch.isfinite(k).all() and torch.isfinite(ka).all())


@pytest.mark.parametrize("U,B", [(1, 2), (2, 2)])
def test_first_binding_follows_the_exact_survival_law(U, B):
    """Condition 3: S = 4096, N = 4, F = 129, generator seed 2, theta = fixed_theta(U, B), sampler seed 0 (the host test's):
    within 5 binomial sigma of the exact survival wherever that lies in [0.02, 0.98]; at least 50 such points."""
    S, N, F = 4096, 4, 129
    theta = fixed_theta(U, B)
    p = synthetic_hmm(N, F, seed=2)[0]
    filt = hmm_estep(dev(p), dev(theta), PRIOR, U, B)["filt"]
    tau = hmm_dwell_sample(filt, dev(theta), U, B, S, seed=0)["tau"].cpu().numpy()
    assert tau.min() >= 0 and tau.max() <= F and np.array_equal(tau, np.rint(tau))
    points, deviation = survival_deviation(tau, oracle_survival(p, theta, U, B, PRIOR))
    print(f"({U}, {B}): {points} points, largest deviation {deviation:.2f} sigma")
    assert points >= 50
    assert deviation <= 5.0


# ---- command line -------------------------------------------------------------------------------------------------
def test_fit_smooth_and_the_multi_state_kinetics_end_to_end(tmp_path):
    runner = CliRunner()
    N, F = 8, 40
    params = {k: v for k, v in TEST_PARAMS.items() if k != "pi"}
    params.update(kon=0.1, koff=0.2)
    save(simulate(2, N, F, 1, 14, params=params), tmp_path)

    def run(*args):
        return runner.invoke(app, ["--cd", str(tmp_path), *args, "--cuda", "--no-input"])

    def files():
        return {f.name: f.read_bytes() for f in tmp_path.iterdir() if f.is_file()}

    result = run("fit", "--model", "cosmos", "--nbatch-size", "8", "--fbatch-size", "40", "--num-iter", "2")
    assert result.exit_code == 0, result.output
    result = run("smooth", "--num-samples", "50", "--num-iter", "30")
    assert result.exit_code == 0, result.output
    dwell_args = ("dwelltime", "-K", "1", "--num-samples", "8", "--num-iter", "50")
    ttfb_args = ("ttfb", "--num-samples", "8", "--num-iter", "50")
    multi = ("--smooth", "--bound-states", "2")
    # the chain has to be fitted first, and the flags choose a chain of `smooth`
    result = run(*dwell_args, *multi)
    assert result.exit_code == 1 and "smooth --unbound-states 1 --bound-states 2" in result.output, result.output
    for args in (dwell_args, ttfb_args):
        result = run(*args, "--bound-states", "2")
        assert result.exit_code == 1 and "need --smooth" in result.output, result.output
    result = run("smooth", "--bound-states", "2", "--num-samples", "50", "--num-iter", "30")
    assert result.exit_code == 0, result.output
    result = run(*dwell_args, "--smooth")
    assert result.exit_code == 0, result.output

    before = files()
    assert "cosmos_dwelltime-smooth-intervals-channel0.pkl" in before and "cosmos_smooth-u1b2.tpqr" in before
    result = run(*dwell_args, *multi)
    assert result.exit_code == 0, result.output
    result = run(*ttfb_args, *multi)
    assert result.exit_code == 0, result.output
    after = files()
    for name, content in before.items():
        assert after[name] == content, name
    new = sorted(set(after) - set(before))
    assert new and all(name.startswith(("cosmos_dwelltime-smooth-u1b2-", "cosmos_ttfb-smooth-u1b2-")) for name in new), new

    n_on = N // 2  # simulate: the first half of the AOIs are on target, all selected by the mask
    table = pd.read_pickle(tmp_path / "cosmos_dwelltime-smooth-u1b2-intervals-channel0.pkl")
    assert list(table.columns) == INTERVAL_COLUMNS and all(table[c].dtype == np.int64 for c in INTERVAL_COLUMNS)
    assert set(table["posterior_sample"]) == set(range(8)) and set(table["aoi"]) == set(range(n_on))
    assert table.groupby(["posterior_sample", "aoi"])["dwell_time"].sum().eq(F).all()
    assert set(table["z"]) <= {0, 1}
    tau = pd.read_csv(tmp_path / "cosmos_ttfb-smooth-u1b2-data-points-channel0.csv", index_col=0).to_numpy()
    assert tau.shape == (8, n_on) and tau.min() >= 0 and tau.max() <= F
    res = pd.read_csv(tmp_path / "cosmos_ttfb-smooth-u1b2-params-channel0.csv", index_col=0)
    assert list(res.index) == ["ka", "kns", "Af"] and np.isfinite(res.values).all()
    assert (tmp_path / "cosmos_ttfb-smooth-u1b2-fraction-bound-channel0.csv").is_file()
    # both commands walk the same rasters: the table's first-binding frames are ttfb's data points
    first = table[table["z"] == 1].groupby(["posterior_sample", "aoi"])["start_frame"].min()
    want = np.full((8, n_on), float(F))
    want[first.index.get_level_values(0), first.index.get_level_values(1)] = first.to_numpy()
    assert np.array_equal(tau, want)

    payload = load_tpqr(tmp_path / "data.tpqr")
    payload["mask"][1] = False  # another selection of AOIs than `smooth` saw
    torch.save(payload, tmp_path / "data.tpqr")
    result = run(*ttfb_args, *multi)
    assert result.exit_code == 1 and "mask" in result.output, result.output
