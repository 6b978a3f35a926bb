"""A mixture of hidden Markov chains over the AOIs on the MI355X: the cases of test_mixture_host.py on
the device build -- ``tq_mixture_mstep`` against the numpy oracle by the tolerance rule of section 20 and bit-equal to
``tq_multistart_mstep`` at G = 1, the EM in chunks and whole, the model-choice table through ``mixture_fit`` and ``hmm_fit``,
``tq_mixture_count`` bit-equal to the g++ replay fed the device's own ``filt`` and ``resp`` and to ``hmm_sample`` at G = 1,
the law of the population draw, ``tq_mixture_estimate`` against numpy -- and ``fit``, ``smooth``, ``smooth --populations``
end to end."""

import hashlib

import numpy as np
import pytest
import torch
from typer.testing import CliRunner

import mixture_fixture as mf
from mixture_fixture import (G_LIST, MODELS, N_LIST, PRIOR, SAMPLER_F, SAMPLER_S, UB_LIST, HostBuild, bic, check_sample,
                             chi2_bound, n_params, oracle_estimate, pop_law_chi2, run_choice_case, run_em_case,
                             run_hopeless_population, run_mstep_case, run_mstep_masked_and_swapped, sampler_inputs)
from tapqir_amd.main import app
from tapqir_amd.utils import mle_analysis as ma
from tapqir_amd.utils.dataset import save
from tapqir_amd.utils.simulate import TEST_PARAMS, simulate

pytestmark = pytest.mark.gpu


def dev(x, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(x))
    return (t if dtype is None else t.to(dtype)).cuda()


class DeviceBuild:
    """The HIP build behind the interface of ``mixture_fixture.HostBuild``: numpy in, numpy out."""

    name = "HIP"

    def estep(self, p, thetas, U, B, active=None):
        P, G = thetas.shape[:2]
        N, M = len(p), U + B
        rows = torch.full((P * G, N, mf.cols(M)), float("nan"), dtype=torch.float64, device="cuda")
        act = None if active is None else dev(np.repeat(active, G), torch.int32)
        ma.multistart_estep(dev(p), dev(thetas.reshape(P * G, -1)), PRIOR, U, B, act, rows)
        return rows.cpu().numpy().reshape(P, G, N, -1)

    def filt(self, p, thetas, U, B):
        return np.stack([ma.hmm_estep(dev(p), dev(t), PRIOR, U, B)["filt"].cpu().numpy() for t in thetas])

    def mstep_all(self, rows, thetas, phi, U, B, allow=None, active=None, it=1, T=3):
        P, G, N = rows.shape[:3]
        th, ph = dev(thetas), dev(phi)
        nan = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float64, device="cuda")  # noqa: E731
        trace, resp, ev = nan(P, T), nan(P, G, N), nan(P, N)
        ma.mixture_mstep(dev(rows), th, ph, trace, it, U, B, allow, None if active is None else dev(active, torch.int32), resp, ev)
        return {"theta": th.cpu().numpy(), "phi": ph.cpu().numpy(), "trace": trace[:, it].cpu().numpy(),
                "resp": resp.cpu().numpy(), "evidence": ev.cpu().numpy(), "traces": trace.cpu().numpy()}

    def multistart_mstep(self, rows, thetas, U, B, allow=None):
        th = dev(thetas)
        trace = torch.full((len(thetas), 3), float("nan"), dtype=torch.float64, device="cuda")
        ma.multistart_mstep(dev(rows), th, trace, 1, U, B, allow)
        return th.cpu().numpy(), trace[:, 1].cpu().numpy()

    def fit(self, p, thetas0, phi0, U, B, allow=None, num_iter=15, chunk=6):
        """The loop of ``mixture_fit`` -- ``multistart_em`` on the two device steps -- and its closing E-step."""
        P, G = thetas0.shape[:2]
        p, N, M = dev(p), len(p), U + B
        thetas, phi = dev(thetas0.reshape(P * G, -1)), dev(phi0)
        rows = torch.empty(P * G, N, mf.cols(M), dtype=torch.float64, device="cuda")
        trace = torch.full((P, num_iter), float("nan"), dtype=torch.float64, device="cuda")
        active = torch.ones(P, dtype=torch.int32, device="cuda")
        rows4, thetas3 = rows.view(P, G, N, -1), thetas.view(P, G, -1)
        iterations, converged = ma.multistart_em(
            lambda: ma.multistart_estep(p, thetas, PRIOR, U, B, active.repeat_interleave(G), rows),
            lambda it: ma.mixture_mstep(rows4, thetas3, phi, trace, it, U, B, allow, active), trace, active, num_iter, 0.0, chunk)
        ma.multistart_estep(p, thetas, PRIOR, U, B, None, rows)
        closing = self.mstep_all(rows4.cpu().numpy(), thetas3.cpu().numpy(), phi.cpu().numpy(), U, B, allow, None, 0, 1)
        return {"thetas": thetas3.cpu().numpy(), "phi": phi.cpu().numpy(), "traces": trace.cpu().numpy(),
                "iterations": iterations, "converged": converged, "logliks": closing["trace"], "resp": closing["resp"],
                "evidence": closing["evidence"]}

    def count(self, filt, thetas, resp, U, B, S, seed):
        out = ma.mixture_sample(dev(filt), dev(thetas), dev(resp), U, B, S, seed=seed, trans=True, raster=True)
        return {k: v.cpu().numpy() for k, v in out.items()}

    def hmm_count(self, filt, theta, U, B, S, seed):
        out = ma.hmm_sample(dev(filt), dev(theta), U, B, S, seed=seed, trans=True, raster=True)
        return {k: v.cpu().numpy() for k, v in out.items()}

    def estimate(self, trans, pop, G, U, B, resample, seed):
        out = ma.mixture_estimate(dev(trans), dev(pop), G, bootstrap=bool(resample), seed=seed)
        S = len(trans)
        return (out["totals"].cpu().numpy().reshape(S, G, -1), out["members"].cpu().numpy(),
                out["A"].cpu().numpy().reshape(S, G, -1))


@pytest.fixture(scope="module")
def build():
    return DeviceBuild()


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return HostBuild(tmp_path_factory.mktemp("mixture"))


# ---- M-step -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("U,B", UB_LIST)
@pytest.mark.parametrize("N", N_LIST)
@pytest.mark.parametrize("G", G_LIST)
def test_weighted_mstep_equals_the_oracle(build, U, B, N, G):
    run_mstep_case(build, U, B, N, G)


def test_masked_topology_and_swapped_populations(build):
    run_mstep_masked_and_swapped(build)


def test_a_hopeless_population_keeps_a_finite_theta(build):
    run_hopeless_population(build)


# ---- EM and model choice ------------------------------------------------------------------------------------------------
def test_em_follows_the_oracle_in_chunks_and_whole(build):
    run_em_case(build)


@pytest.mark.parametrize("kind,s", mf.CHOICE_SETS)
def test_model_choice_reproduces_the_table(kind, s):
    """``hmm_fit`` for the single chains and ``mixture_fit`` for the mixtures, 150 iterations in one chunk, tol 0; the
    responsibilities, the per-AOI evidence and the population map of ``mixture_fit`` are those of its populations in
    descending phi."""
    p = dev(mf.data(kind, s)[0])
    N, F = p.shape
    fits = {}
    for name, U, B, G in MODELS:
        if G == 1:
            fit = ma.hmm_fit(p, PRIOR, U, B, num_iter=150, tol=0.0, chunk=150)
        else:
            fit = ma.mixture_fit(p, PRIOR, U, B, populations=G, num_iter=150, tol=0.0, chunk=150)
            assert fit["n_params"] == n_params(U + B, G) and fit["best"] == 0 and fit["logliks"].shape == (1,)
            phi = fit["phi"].cpu().numpy()
            assert (np.diff(phi) <= 0).all() and abs(phi.sum() - 1) <= 4 * np.spacing(1.0)
            assert fit["thetas"].shape == (G, 6) and fit["filt"].shape == (G, N, F, 2) and fit["gamma"].shape == (N, F, 2)
            assert torch.equal(fit["population_map"], fit["resp"].argmax(0))
            assert abs(fit["evidence"].sum().item() - fit["loglik"]) <= 1e-9 * abs(fit["loglik"])
            assert float((fit["gamma"].sum(-1) - 1).abs().max()) <= 1e-12
        assert fit["bic"] == bic(fit["loglik"], fit["n_params"], N, F)
        fits[name] = {"bic": fit["bic"], "trace": fit["trace"].cpu().numpy(),
                      "resp": fit["resp"].cpu().numpy() if G > 1 else None}
    run_choice_case(fits, kind, s, "HIP")


# ---- sampler ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("U,B", UB_LIST)
@pytest.mark.parametrize("G", [1, 2, 4])
@pytest.mark.parametrize("F", SAMPLER_F)
def test_sampler_equals_the_replay(build, host, G, F, U, B):
    """``tq_mixture_count`` against the g++ replay fed the device's own filt and resp, bit for bit, after the margins of the
    population draws and of the state draws; at G = 1 bit-equal to ``hmm_sample``."""
    p, thetas, filt, resp = sampler_inputs(build, U, B, G, F)
    for S in SAMPLER_S:
        ref = host.count(filt, thetas, resp, U, B, S, F)
        print(f"G = {G} F = {F} S = {S}: smallest |u - threshold| {ref['margins'][0]:.3g} (population), "
              f"{ref['margins'][1]:.3g} (states)")
        assert ref["margins"][1] > 1e-9 and (G == 1 or ref["margins"][0] > 1e-9)
        out = build.count(filt, thetas, resp, U, B, S, F)
        check_sample(out, ref, U, U + B)
        assert np.array_equal(out["counts"], ref["counts"]) and np.array_equal(out["trans"], ref["trans"])
        if G == 1:
            single = build.hmm_count(filt[0], thetas[0], U, B, S, F)
            assert (out["pop"] == 0).all()
            for key in ("counts", "trans", "raster"):
                assert np.array_equal(out[key], single[key]), key


def test_population_draws_follow_the_responsibilities(build):
    p, thetas, filt, resp = sampler_inputs(build, 1, 1, 4, 2)
    out = build.count(filt, thetas, resp, 1, 1, 4096, 11)
    chi2, dof = pop_law_chi2(out["pop"], resp)
    print(f"chi2 = {chi2:.2f} with {dof} degrees of freedom, bound {chi2_bound(dof):.2f}")
    assert dof >= 6 and chi2 <= chi2_bound(dof)


# ---- estimate -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("resample", [0, 1])
def test_estimate_equals_numpy(build, resample, tmp_path):
    U, B, G, S, N = 1, 2, 3, 70, 6
    rng = np.random.default_rng(5)
    trans = rng.integers(0, 40, (S, N, 9)).astype(np.int32)
    pop = rng.integers(0, 2, (S, N)).astype(np.uint8)  # population 2 has no member
    pop[0] = 0
    idx = mf.host_indices(mf.build_rates_check(tmp_path), 9, S, N) if resample else None
    totals, members, est = build.estimate(trans, pop, G, U, B, resample, 9)
    t, m, e = oracle_estimate(trans, pop, G, U + B, idx)
    assert np.array_equal(totals, t) and np.array_equal(members, m) and np.array_equal(est, e, equal_nan=True)
    assert (members[:, 2] == 0).all() and np.isnan(est[:, 2]).all() and np.isnan(est[0, 1]).all()


def test_viterbi_takes_the_path_of_the_map_population(build):
    U, B, G, F = 1, 2, 3, 65
    p, thetas, filt, resp = sampler_inputs(build, U, B, G, F)
    out = ma.mixture_viterbi(dev(p), dev(thetas), dev(resp), PRIOR, U, B)
    pmap = out["population_map"].cpu().numpy()
    assert np.array_equal(pmap, resp.argmax(0))
    for n in range(len(p)):
        want = ma.hmm_viterbi(dev(p[n:n + 1]), dev(thetas[pmap[n]]), PRIOR, U, B)[0]
        assert torch.equal(out["path"][n], want), n


# ---- command line -----------------------------------------------------------------------------------------------------
def test_fit_then_smooth_then_smooth_with_populations(tmp_path):
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

    def files():
        return sorted(f.name for f in tmp_path.iterdir() if f.is_file())

    smooth = ["--num-samples", "50", "--num-iter", "30"]
    two_names = ("cosmos_smooth.tpqr", "cosmos_smooth-channel0.csv")
    run("fit", "--model", "cosmos", "--nbatch-size", "8", "--fbatch-size", "40", "--num-iter", "2")
    run("smooth", *smooth)
    before = files()
    old = hashes(*before)
    run("smooth", "--populations", "2", *smooth)
    g2 = ("cosmos_smooth-u1b1g2.tpqr", "cosmos_smooth-u1b1g2-channel0.csv")
    assert files() == sorted([*before, *g2]) and hashes(*before) == old
    out = torch.load(tmp_path / g2[0])
    N, n = out["mask"].numel(), int(out["mask"].sum())  # the AOIs of the data set and the on-target ones among them
    shapes = {"z_probs": (N, F, 1), "z_map": (N, F, 1), "state_probs": (N, F, 1, 2), "population_probs": (N, 2, 1),
              "population_map": (N, 1), "theta": (1, 2, 6), "phi": (1, 2), "log_evidence": (N, 1), "bic": (1,),
              "restart_logliks": (1, 1), "topology": (2, 2), "mask": (N,)}
    for key, shape in shapes.items():
        assert tuple(out[key].shape) == shape, key
    assert out["n_params"] == 7 and len(out["loglik_trace"]) == 1 and out["populations"] == 2
    probs = out["population_probs"][out["mask"]][:, :, 0]
    assert float((probs.sum(1) - 1).abs().max()) <= 1e-12 and torch.equal(out["population_map"][out["mask"]][:, 0].long(), probs.argmax(1))
    assert out["phi"][0, 0] >= out["phi"][0, 1] and abs(out["phi"].sum().item() - 1) <= 1e-12
    assert out["bic"][0] == -2 * out["restart_logliks"][0, 0] + 7 * np.log(n * F)
    assert abs(out["log_evidence"][out["mask"]][:, 0].sum().item() - out["restart_logliks"][0, 0].item()) <= 1e-9 * n * F
    import pandas as pd

    table = pd.read_csv(tmp_path / g2[1], index_col=0)
    rows = [f"g{g}_{name}" for g in range(2) for name in ("phi", "A00", "A01", "A10", "A11", "dwell0", "dwell1", "kon", "koff")]
    assert list(table.index) == rows and list(table.columns) == ["EM", "Mean", "95% LL", "95% UL"]
    assert np.isfinite(table["EM"].to_numpy()).all()
    log = (tmp_path / ".tapqir" / "loginfo").read_text()
    assert "mixture BIC" in log and "--bound-states" in log

    run("smooth", "--bound-states", "2", "--populations", "2", "--restarts", "2", *smooth)
    g22 = ("cosmos_smooth-u1b2g2.tpqr", "cosmos_smooth-u1b2g2-channel0.csv")
    assert files() == sorted([*before, *g2, *g22]) and hashes(*before) == old
    mid = hashes(*g2)
    out = torch.load(tmp_path / g22[0])
    assert out["theta"].shape == (1, 2, 12) and out["restart_logliks"].shape == (1, 3) and out["n_params"] == 17
    assert out["bic"][0] == -2 * out["restart_logliks"][0].max() + 17 * np.log(n * F)
    assert out["bic"][0] <= -2 * out["restart_logliks"][0, 0] + 17 * np.log(n * F)  # no higher than from the default start alone
    run("smooth", *smooth)
    assert hashes(*before) == old and hashes(*g2) == mid
