"""`dwelltime --censored` on the MI355X (cases, references and bounds in censored_fixture.py; the same bodies on the g++
build in test_censored.py).

1. ``tq_dwell_censored_hist`` on the device tables of all four samplers, bit for bit against the bincount of the host
   DataFrame's open last runs, at the workgroup boundaries of the table and with an empty table.
2. One Adam step of ``tq_dwell_censored_fit`` (K = 1 .. 8) taken apart under the rule of kinetics_boundary_fixture.py, at
   (complete, censored) pair counts that straddle the 64-lane round and the staging limit on their sum; the LDS and L2
   routes have the same bits.
3. Trajectories against the float64 restatement, chunking, empty rows, censored-only rows, and bit equality with
   ``tq_dwell_fit`` when every censored row is empty.
4. ``tq_dwell_survival`` against numpy float64.
5. What the feature is for: a simulated two-state chain whose interior-only rate is biased and whose censored rate is not.
6. The command end to end.

Measured on an MI355X: see DESIGN.md section 31.
"""

import ctypes as C

import numpy as np
import pandas as pd
import pytest
import torch
from typer.testing import CliRunner

import censored_fixture as cf
import kinetics_boundary_fixture as kb
from hmm_fixture import PRIOR, fixed_theta
from smooth_fixture import synthetic_chain
from tapqir_amd import _lib, _lib_censored
from tapqir_amd.main import app
from tapqir_amd.utils.censored_analysis import (dwell_censored_fit, dwell_censored_fit_steps, dwell_censored_hist,
                                                dwell_censored_rate, dwell_csr_from_censored_hist, dwell_survival)
from tapqir_amd.utils.dataset import save
from tapqir_amd.utils.mle_analysis import (dwell_csr_from_hist, dwell_csr_from_padded, dwell_fit_steps, dwell_init_state,
                                           dwell_intervals, dwell_sample, hmm_dwell_intervals, hmm_dwell_sample, hmm_estep,
                                           mixture_dwell_intervals, mixture_dwell_sample, smooth_dwell_intervals,
                                           smooth_dwell_sample, smooth_estep)
from tapqir_amd.utils.safe_load import load_tpqr
from tapqir_amd.utils.simulate import TEST_PARAMS, simulate

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZES = [(1, 5, 1), (65, 3, 2), (3, 4, 65), (70, 7, 129)]  # (S, N, F)


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def on_dev(csr):
    return tuple(x.to(DEV) for x in csr)


def evidence(N, F, seed):
    """(N, F) float32 p: rows of all 0, all 1, alternating 0 / 1, p = 1 on the last frame only, then a synthetic chain."""
    p = np.array(synthetic_chain(N, F, seed)[0], dtype=np.float32)
    last = np.zeros(F)
    last[F - 1] = 1.0
    for n, row in enumerate([np.zeros(F), np.ones(F), np.arange(F) % 2, last][:N]):
        p[n] = row
    return p


def open_run_bincount(frame, S, F, G=None):
    """{"cens_bound", "cens_unbound"} from the host DataFrame: rows with low_or_high == z + 2 and start_frame > 0."""
    out = {}
    for z, key in ((1, "cens_bound"), (0, "cens_unbound")):
        sel = frame[(frame["low_or_high"] == z + 2) & (frame["start_frame"] > 0)]
        assert (sel["z"] == z).all()
        want = np.zeros((S, F) if G is None else (S, G, F), np.int32)
        index = (sel["posterior_sample"].to_numpy(),) + (() if G is None else (sel["population"].to_numpy(),))
        np.add.at(want, index + (sel["dwell_time"].to_numpy(),), 1)
        out[key] = want
    return out


def assert_hist_equals(got, want, where):
    for key in ("cens_bound", "cens_unbound"):
        assert got[key].dtype == torch.int32 and tuple(got[key].shape) == want[key].shape, (where, key)
        assert np.array_equal(got[key].cpu().numpy(), want[key]), (where, key)


# ---- 1. tq_dwell_censored_hist --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,N,F", SIZES)
def test_censored_hist_of_the_independent_sampler(S, N, F):
    p = dev(evidence(N, F, seed=F))
    sample = dwell_sample(p, S, seed=3)
    frame, table = dwell_intervals(p, S, seed=3, sample=sample, device_table=True)
    pd.testing.assert_frame_equal(frame, dwell_intervals(p, S, seed=3, sample=sample))  # the DataFrame it returns now
    assert table.dtype == torch.int32 and tuple(table.shape) == (_lib.DWELL_COLS, len(frame)) and table.is_cuda
    got = dwell_censored_hist(table, S, N, F)
    assert_hist_equals(got, open_run_bincount(frame, S, F), ("dwell_sample", S, N, F))
    # the deterministic rows: whole-record runs count nowhere; p = 1 on the last frame only is an open run of d = 1
    if F > 2 and N >= 4:
        assert int(got["cens_bound"][:, 1].min()) >= 1
    if F == 1:
        assert int(got["cens_bound"].sum()) == 0 and int(got["cens_unbound"].sum()) == 0
    again = dwell_censored_hist(table, S, N, F)
    assert all(torch.equal(got[k], again[k]) for k in got)


@pytest.mark.parametrize("S,N,F", SIZES)
def test_censored_hist_of_the_markov_samplers(S, N, F):
    p = dev(evidence(N, F, seed=100 + F))
    theta = torch.tensor((0.05, 0.10, 0.4), dtype=torch.float64, device=DEV)
    filt = smooth_estep(p, theta, PRIOR)["filt"]
    sample = smooth_dwell_sample(filt, theta, S, seed=5)
    frame, table = smooth_dwell_intervals(filt, theta, S, seed=5, sample=sample, device_table=True)
    assert_hist_equals(dwell_censored_hist(table, S, N, F), open_run_bincount(frame, S, F), ("tq_smooth_dwell", S, N, F))

    U, B = 1, 2
    theta = dev(fixed_theta(U, B))
    filt = hmm_estep(p, theta, PRIOR, U, B)["filt"]
    sample = hmm_dwell_sample(filt, theta, U, B, S, seed=6)
    frame, table = hmm_dwell_intervals(filt, theta, U, B, S, seed=6, sample=sample, device_table=True)
    assert_hist_equals(dwell_censored_hist(table, S, N, F), open_run_bincount(frame, S, F), ("tq_chain_dwell", S, N, F))

    G = 3
    thetas = np.array([fixed_theta(U, B, seed=g) for g in range(G)])
    filt = torch.stack([hmm_estep(p, dev(thetas[g]), PRIOR, U, B)["filt"] for g in range(G)])
    resp = dev(np.ascontiguousarray(np.random.default_rng(100 * F + G).dirichlet(np.ones(G), N).T))
    sample = mixture_dwell_sample(filt, dev(thetas), resp, U, B, S, seed=7)
    frame, table = mixture_dwell_intervals(filt, dev(thetas), resp, U, B, S, seed=7, sample=sample, device_table=True)
    assert tuple(table.shape) == (_lib.DWELL_COLS, len(frame)) and "population" in frame.columns
    got = dwell_censored_hist(table, S, N, F, pop=sample["pop"], populations=G)
    assert_hist_equals(got, open_run_bincount(frame, S, F, G), ("tq_population_dwell", S, N, F))
    pooled = dwell_censored_hist(table, S, N, F)
    assert torch.equal(pooled["cens_bound"], got["cens_bound"].sum(1)) and torch.equal(pooled["cens_unbound"],
                                                                                        got["cens_unbound"].sum(1))


@pytest.mark.parametrize("total", [0, 1, 63, 64, 65, 255, 256, 257])
def test_censored_hist_of_a_table_of_a_few_rows(total):
    """A hand-made table of ``total`` rows, every one of them an open last run that opened inside the record, between two
    canaries: each is counted once, nothing else is written."""
    S, N, F = 4, 3, 9
    i = np.arange(total)
    cols = np.zeros((_lib.DWELL_COLS, total), np.int32)
    cols[0], cols[1] = i % S, i % N
    cols[4] = 1 + i % (F - 1)
    cols[3] = F - 1
    cols[2] = F - cols[4]
    cols[6] = i % 2
    cols[5] = cols[6] + 2
    table = dev(cols) if total else torch.zeros(_lib.DWELL_COLS, 0, dtype=torch.int32, device=DEV)
    got = dwell_censored_hist(table, S, N, F)
    want = {k: np.zeros((S, F), np.int32) for k in ("cens_bound", "cens_unbound")}
    for key, z in (("cens_bound", 1), ("cens_unbound", 0)):
        np.add.at(want[key], (cols[0][cols[6] == z], cols[4][cols[6] == z]), 1)
    assert_hist_equals(got, want, total)
    assert int(got["cens_bound"].sum() + got["cens_unbound"].sum()) == total
    # the entry point itself, with canaries around both histograms
    buf = torch.full((2, S * F + 2), -7, dtype=torch.int32, device=DEV)
    buf[:, 1:-1] = 0
    a = _lib_censored.DwellCensoredHistArgs(intervals=_lib.ptr(table) if total else None, cens_bound=buf[0, 1:].data_ptr(),
                                            cens_unbound=buf[1, 1:].data_ptr(), total=total, S=S, N=N, F=F, G=1)
    assert _lib_censored.lib().tq_dwell_censored_hist(C.byref(a), C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    assert (host[:, 0] == -7).all() and (host[:, -1] == -7).all()
    assert np.array_equal(host[0, 1:-1].reshape(S, F), want["cens_bound"])
    assert np.array_equal(host[1, 1:-1].reshape(S, F), want["cens_unbound"])


# ---- 2. the fit, one step taken apart --------------------------------------------------------------------------------------
def dev_censored_steps(state, csr, ccsr, K, step0=0, stage_lds=True, n_steps=1):
    state = state.to(DEV)
    loss = torch.full((state.shape[0],), float("nan"), device=DEV)
    dwell_censored_fit_steps(state, on_dev(csr), on_dev(ccsr), K, step0=step0, n_steps=n_steps, loss=loss,
                             stage_lds=stage_lds)
    return state.cpu(), loss.cpu()


@pytest.fixture(scope="module")
def hk(tmp_path_factory):
    return cf.build_censored_check(tmp_path_factory.mktemp("censored"))


@pytest.mark.parametrize("kind", cf.CENS_STATES)
@pytest.mark.parametrize("K", range(1, 9))
def test_censored_step(hk, K, kind):
    """Gradient, loss and update of one step of tq_dwell_censored_fit_kernel<K> at every row of CENS_LENS in one launch per
    route, against float64; the routes have the same bits."""
    csr, ccsr = cf.censored_rows()
    par0 = cf.censored_par0(K, kind)
    before, ref = kb.dwell_state(par0), cf.censored_reference(K, kind)
    out = {}
    for staged in (True, False):
        after, loss = out[staged] = dev_censored_steps(before, csr, ccsr, K, stage_lds=staged)
        for key, (excess, row) in kb.worst(kb.step_report(before, after, loss, ref, 2 * K)).items():
            print(f"censored K={K} {kind} staged={staged} {key}: worst excess {excess:.3g} (row {cf.CENS_LENS[row]})")
            assert excess <= 1.0, (K, kind, staged, key, excess, cf.CENS_LENS[row])
        assert torch.equal(after[0], before[0]) and loss[0] == 0  # the empty row: zero gradient, untouched state
    assert kb.same_bits(out[True][0], out[False][0]) and kb.same_bits(out[True][1], out[False][1])
    if K == 1:  # no free weight: the logit gradient is exactly zero
        after = out[True][0]
        assert (after[:, 1] == par0[:, 1]).all() and (after[:, 3] == 0).all() and (after[:, 5] == 0).all()
    host = cf.host_censored_steps(hk, before, csr, ccsr, K)[0]
    gd, gh = kb.recover_gradient(out[True][0], 2 * K)[0], kb.recover_gradient(host, 2 * K)[0]
    gap = float(((gd - gh).abs().amax(1) / gh.abs().amax(1).clamp(min=1e-30)).max())
    print(f"censored K={K} {kind}: device - host gradient {gap:.3g} of the row's largest")


# ---- 3. the fit, trajectories ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 2, 3])
def test_censored_fit_matches_float64_torch(K):
    data, cdata = cf.trajectory_data()
    want = cf.trajectory_reference(K)
    csr, ccsr = dwell_csr_from_padded(data.to(DEV)), on_dev(cf.censored_csr(cdata))
    got = dwell_censored_fit(csr, ccsr, K, n_steps=300)
    rk, rA = kb.rel(got["k"], want["k"]), kb.rel(got["A"], want["A"])
    print(f"censored trajectory K={K}: relative error of k {rk:.3g}, of A {rA:.3g}")
    assert rk <= 1e-4 and rA <= 1e-4, (K, got["k"].cpu(), want["k"])
    loss64 = -cf.loglik64(cf.trajectory_reference(K, 299)["par"], data.double(), cdata.double(), K)
    assert kb.rel(got["loss"], loss64) < 1e-4
    chunked = dwell_censored_fit(csr, ccsr, K, n_steps=300, chunk=70)
    for name in ("k", "A", "loss"):
        assert torch.equal(got[name], chunked[name]), name


@pytest.mark.parametrize("K", [1, 3])
def test_empty_and_censored_only_rows(K):
    """Row 0 has nothing and keeps its initial parameters exactly; row 1 has censored pairs only: nothing ever left, so
    every step lowers its rates, and it stays finite; row 2 has both."""
    data = torch.zeros(3, 50)
    data[2, :10] = torch.arange(1, 11).float()
    cdata = -torch.ones(3, 50)
    cdata[1, :20] = torch.arange(20).float() * 3.0
    cdata[2, :3] = 40.0
    csr, ccsr = dwell_csr_from_padded(data.to(DEV)), on_dev(cf.censored_csr(cdata))
    state = dwell_init_state(3, K, DEV)
    init = state.clone()
    loss = torch.full((3,), float("nan"), device=DEV)
    dwell_censored_fit_steps(state, csr, ccsr, K, n_steps=500, loss=loss)
    assert torch.equal(state[0], init[0]) and loss[0] == 0
    assert torch.isfinite(state).all() and torch.isfinite(loss).all()
    assert (state[1, :K] < init[1, :K]).all()
    if K == 1:
        assert (state[:, 1] == 0).all() and (state[:, 3] == 0).all() and (state[:, 5] == 0).all()


@pytest.mark.parametrize("K", [1, 3, 8])
def test_empty_censored_rows_give_the_bits_of_tq_dwell_fit(K):
    csr = on_dev(kb.dwell_rows())
    S = len(kb.DWELL_LENS)
    ccsr = on_dev(cf.empty_csr(S))
    for steps in (1, 300):
        for staged in (True, False):
            a, b = dwell_init_state(S, K, DEV), dwell_init_state(S, K, DEV)
            la, lb = torch.full((S,), float("nan"), device=DEV), torch.full((S,), float("nan"), device=DEV)
            dwell_censored_fit_steps(a, csr, ccsr, K, n_steps=steps, loss=la, stage_lds=staged)
            dwell_fit_steps(b, csr, K, n_steps=steps, loss=lb, stage_lds=staged)
            assert kb.same_bits(a, b) and kb.same_bits(la, lb), (K, steps, staged)


# ---- 4. tq_dwell_survival --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [1, 5])
@pytest.mark.parametrize("F", [1, 2, 63, 64, 65, 129, 300])
def test_survival_matches_numpy(R, F):
    """Rows (cyclically): random, all-zero, events only in the last bin, censored only, no censoring (Y = h at the last
    event: the curve ends at exactly 0)."""
    rng = np.random.default_rng(1000 * R + F)
    hist = (rng.integers(0, 50, (R, F)) * (rng.random((R, F)) < 0.4)).astype(np.int32)
    cens = (rng.integers(0, 30, (R, F)) * (rng.random((R, F)) < 0.3)).astype(np.int32)
    for r in range(R):
        if r % 5 == 1:
            hist[r], cens[r] = 0, 0
        elif r % 5 == 2:
            hist[r], cens[r] = 0, 0
            hist[r, F - 1] = 11
        elif r % 5 == 3:
            hist[r] = 0
        elif r % 5 == 4:
            cens[r] = 0
    if R == 1:
        cens[0, F // 2:] = 0  # Y = h somewhere in the upper half, when that half has an event
    surv = dwell_survival(dev(hist), dev(cens))
    assert surv.dtype == torch.float64 and tuple(surv.shape) == (R, F)
    got, want = surv.cpu().numpy(), cf.survival_numpy(hist, cens)
    assert np.all(got[:, 0] == 1.0)
    assert np.array_equal(got == 1.0, want == 1.0) and np.array_equal(got == 0.0, want == 0.0)
    rel = np.abs(got - want) / np.where(want > 0, want, 1.0)
    print(f"survival R={R} F={F}: worst relative error {rel.max():.3g} (bound {2 * F * 2.0 ** -52:.3g})")
    assert rel.max() <= 2 * F * 2.0 ** -52
    for r in range(R):
        if r % 5 in (1, 3):
            assert np.all(got[r] == 1.0)
        elif r % 5 == 2 and F > 1:
            assert np.all(got[r, : F - 1] == 1.0) and got[r, F - 1] == 0.0
        elif r % 5 == 4 and hist[r, 1:].any():
            assert got[r, np.flatnonzero(hist[r, 1:])[-1] + 1] == 0.0
    assert torch.equal(dwell_survival(dev(hist)[0], dev(cens)[0]), surv[:1])  # one row as a vector


# ---- 5. what the feature is for ----------------------------------------------------------------------------------------------
def test_open_runs_remove_the_bias_of_slow_complexes():
    """200 AOIs x 300 frames of a two-state chain with kon 0.02, koff 0.01 as an exact 0/1 ``p``: every sample walks the
    same runs.  From the device histograms, the closed-form K = 1 estimates: the censored one within 3 k / sqrt(n) of
    0.01, the interior-only one more than that above it; the K = 1 censored fit against its float64 restatement; and the
    survival at t = 50 within the same 3-sigma band (delta method) of exp(-0.5)."""
    z = cf.two_state_raster(cf.CHAIN_SEED)
    N, F = z.shape
    S, koff = 3, cf.CHAIN["koff"]
    p = dev(z.astype(np.float32))
    sample = dwell_sample(p, S, seed=0)
    frame, table = dwell_intervals(p, S, seed=0, sample=sample, device_table=True)
    cens = dwell_censored_hist(table, S, N, F)
    h_want, c_want = cf.raster_histograms(z)
    for s in range(S):  # the device histograms are those of the raster
        assert np.array_equal(sample["hist_bound"][s].cpu().numpy(), h_want)
        assert np.array_equal(cens["cens_bound"][s].cpu().numpy(), c_want)
    hist, open_runs = sample["hist_bound"], cens["cens_bound"]
    k_int, k_cens = dwell_censored_rate(hist)[0].item(), dwell_censored_rate(hist, open_runs)[0].item()
    n = float(hist[0].sum())
    band = 3.0 * koff / np.sqrt(n)
    print(f"n_complete {n:.0f}, open {int(open_runs[0, 2:].sum())}: interior-only koff {k_int:.5f}, censored {k_cens:.5f}, "
          f"band {band:.5f}")
    assert abs(k_cens - koff) <= band
    assert k_int - koff > band

    steps, lr = 1500, 0.05  # from k = 1 the default lr of 5e-3 needs more than 4000 steps to arrive; 0.05 is there by 1500
    fit = dwell_censored_fit(dwell_csr_from_hist(hist), dwell_csr_from_censored_hist(open_runs), 1, lr=lr, n_steps=steps)
    d = torch.arange(F, dtype=torch.float64)
    data = torch.repeat_interleave(d, torch.from_numpy(h_want))[None]
    cdata = torch.repeat_interleave(d[2:] - 1.0, torch.from_numpy(c_want[2:]))[None]
    want = cf.torch_fit64(data, cdata, 1, n_steps=steps, lr=lr)
    assert abs(want["k"].item() - k_cens) <= 1e-3 * k_cens  # the fit's maximiser is the closed form
    print(f"K = 1 censored fit after {steps} steps: {fit['k'][0, 0].item():.6f}, float64 {want['k'][0, 0].item():.6f}, "
          f"closed form {k_cens:.6f}")
    assert kb.rel(fit["k"], want["k"].expand(S, 1)) <= 1e-4
    assert torch.equal(fit["k"][0], fit["k"][1]) and torch.equal(fit["k"][0], fit["k"][2])

    surv50 = dwell_survival(hist, open_runs)[0, 50].item()
    s_true = np.exp(-50.0 * koff)
    s_band = 3.0 * s_true * 50.0 * koff / np.sqrt(n)
    print(f"survival at t = 50: {surv50:.4f}, exp(-0.5) = {s_true:.4f}, band {s_band:.4f}")
    assert abs(surv50 - s_true) <= s_band


# ---- 6. command line -------------------------------------------------------------------------------------------------------
def test_dwelltime_censored_command_end_to_end(tmp_path):
    runner = CliRunner()
    N, F = 8, 60
    params = {k: v for k, v in TEST_PARAMS.items() if k != "pi"}
    params.update(kon=0.1, koff=0.2)
    save(simulate(2, N, F, 1, 14, params=params), tmp_path)

    def run(*args):
        return runner.invoke(app, ["--cd", str(tmp_path), *args, "--cuda", "--no-input"])

    def snapshot():
        return {f.name: f.read_bytes() for f in tmp_path.iterdir() if f.is_file()}

    try:
        import matplotlib  # noqa: F401

        plots = True
    except ImportError:
        plots = False

    result = run("fit", "--model", "cosmos", "--nbatch-size", "8", "--fbatch-size", "60", "--num-iter", "2")
    assert result.exit_code == 0, result.output
    # a fit of two iterations knows nothing of z yet, and the chain `smooth` fits to it never leaves a state.  The
    # calibrated posterior of a simulated chain stands in for what a converged fit leaves in the parameter file.
    payload = load_tpqr(tmp_path / "cosmos_params.tpqr")
    p = torch.from_numpy(synthetic_chain(payload["z_probs"].shape[0], F, seed=1)[0])
    payload["z_probs"][:, :, 0, 1] = p
    payload["z_probs"][:, :, 0, 0] = 1.0 - p
    payload["p_specific"][:, :, 0] = p
    payload["z_map"][:, :, 0] = p > 0.5
    torch.save(payload, tmp_path / "cosmos_params.tpqr")
    result = run("smooth", "--num-samples", "50", "--num-iter", "30")
    assert result.exit_code == 0, result.output
    dwell_args = ("dwelltime", "-K", "1", "--num-samples", "8", "--num-iter", "50")
    for form, stem in (((), "cosmos_dwelltime"), (("--smooth",), "cosmos_dwelltime-smooth")):
        result = run(*dwell_args, *form)
        assert result.exit_code == 0, result.output
        before = snapshot()
        assert f"{stem}-intervals-channel0.pkl" in before and not any(name.startswith(f"{stem}-censored-") for name in before)
        table = pd.read_pickle(tmp_path / f"{stem}-intervals-channel0.pkl")

        result = run(*dwell_args, *form, "--censored")
        assert result.exit_code == 0, result.output
        assert "open" in result.output
        after = snapshot()
        pd.testing.assert_frame_equal(pd.read_pickle(tmp_path / f"{stem}-intervals-channel0.pkl"), table)
        for name, content in before.items():
            # the .mat file is written again with the same table; its header carries the time of writing
            if not name.endswith(".mat") and not name.endswith(".log"):
                assert after[name] == content, name
        new = sorted(set(after) - set(before))
        assert new and all(name.startswith(f"{stem}-censored-") for name in new), new
        for rate, kind in (("koff", "bound"), ("kon", "unbound")):
            res = pd.read_csv(tmp_path / f"{stem}-censored-{rate}-channel0.csv", index_col=0)
            assert list(res.index) == ["A0", f"{rate}0"] and list(res.columns) == ["Mean", "95% LL", "95% UL"]
            assert np.isfinite(res.values).all()
            curve = pd.read_csv(tmp_path / f"{stem}-censored-{kind}-survival-channel0.csv", index_col=0)
            assert list(curve.columns) == ["time", "best fit", "survival mean", "survival 95% ll", "survival 95% ul"]
            assert np.isfinite(curve.values).all() and curve["survival mean"][0] == 1.0 and curve["best fit"][0] == 1.0
            assert (curve["survival 95% ll"] <= curve["survival mean"] + 1e-12).all()
            assert (curve["survival mean"] <= curve["survival 95% ul"] + 1e-12).all()
            assert (tmp_path / f"{stem}-censored-{kind}-survival-channel0.png").is_file() == plots

    # per population: the same switch after `smooth --populations 2` (which populations have data is up to the mixture)
    result = run("smooth", "--populations", "2", "--num-samples", "50", "--num-iter", "30")
    assert result.exit_code == 0, result.output
    pops, stem = ("--smooth", "--populations", "2"), "cosmos_dwelltime-smooth-u1b1g2"
    result = run(*dwell_args, *pops)
    assert result.exit_code == 0, result.output
    before = snapshot()
    result = run(*dwell_args, *pops, "--censored")
    assert result.exit_code == 0, result.output
    after = snapshot()
    for name, content in before.items():
        if not name.endswith(".mat"):
            assert after[name] == content, name
    new = sorted(set(after) - set(before))
    assert new and all(name.startswith(f"{stem}-") and "-censored-" in name for name in new), new
    tables = [name for name in new if name.endswith(("-censored-koff-channel0.csv", "-censored-kon-channel0.csv"))]
    assert tables, new
    for name in tables:
        res = pd.read_csv(tmp_path / name, index_col=0)
        assert all(row.startswith(("g0_", "g1_")) for row in res.index) and np.isfinite(res.values).all(), name
    curves = [name for name in new if "-survival-" in name and name.endswith(".csv")]
    assert curves and all(name.startswith((f"{stem}-g0-censored-", f"{stem}-g1-censored-")) for name in curves), new
    for name in curves:
        assert np.isfinite(pd.read_csv(tmp_path / name, index_col=0).values).all(), name
