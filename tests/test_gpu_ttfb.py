"""Time-to-first-binding kernels on the MI355X: the first-binding sampler (exact replay, binary rows, law), the batched
censored-mixture MLE (float64 torch restatement, edge cases, chunking, LDS and L2 paths, recovery of known rates) and
the ``ttfb`` command end to end."""

import math

import numpy as np
import pandas as pd
import pytest
import torch
from typer.testing import CliRunner

from tapqir_amd.main import app
from tapqir_amd.utils.dataset import save
from tapqir_amd.utils.imscroll import time_to_first_binding
from tapqir_amd.utils.mle_analysis import ttfb_fit, ttfb_fit_steps, ttfb_init_state, ttfb_sample
from tapqir_amd.utils.simulate import TEST_PARAMS, simulate
from ttfb_fixture import build_kinetics_check, host_sample, loglik64, torch_fit64

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T = 1000.0


@pytest.fixture(scope="module")
def hk(tmp_path_factory):
    return build_kinetics_check(tmp_path_factory.mktemp("kinetics"))


def mixture_draws(gen, S, N, ka=0.02, kns=0.002, Af=0.7, Tmax=T, zeros=0.0):
    """S x N first-binding times of the model (continuous, censored at Tmax; a fraction `zeros` bound at t = 0)."""
    active = torch.rand(S, N, generator=gen, dtype=torch.float64) < Af
    rate = torch.where(active, torch.tensor(ka + kns, dtype=torch.float64), torch.tensor(kns, dtype=torch.float64))
    t = -torch.log(torch.rand(S, N, generator=gen, dtype=torch.float64)) / rate
    t = t.clamp(max=Tmax)
    t = torch.where(torch.rand(S, N, generator=gen, dtype=torch.float64) < zeros, torch.zeros_like(t), t)
    return t.float()


def rel(a, b):
    return float(((a.double().cpu() - b.double().cpu()).abs() / b.double().cpu().abs()).max())


# ---- sampler ------------------------------------------------------------------------------------------------------
def test_sampler_on_binary_rows_gives_the_first_binding():
    gen = torch.Generator().manual_seed(0)
    z = (torch.rand(70, 300, generator=gen) < 0.01).float()
    z[0] = 0.0
    z[1, 0] = 1.0
    tau = ttfb_sample(z.to(DEV), 25, seed=3).cpu()
    want = time_to_first_binding(z)
    assert torch.equal(tau, want.expand(25, -1))


def test_sampler_host_replay_is_exact(hk):
    gen = torch.Generator().manual_seed(1)
    p = torch.rand(37, 500, generator=gen) ** 6  # mostly small p, long survival
    p[3, 100] = 1.0
    p[4] = 0.0
    p[5, :10] = 0.0
    tau = ttfb_sample(p.to(DEV), 129, seed=12345).cpu()
    assert torch.equal(tau, host_sample(hk, p, 129, 12345))
    assert (tau[:, 3] <= 100).all() and (tau[:, 4] == 500).all()


def test_sampler_law_matches_the_exact_pmf():
    S, F = 100000, 24
    gen = torch.Generator().manual_seed(2)
    p = torch.rand(3, F, generator=gen, dtype=torch.float64) * torch.tensor([0.05, 0.2, 0.6], dtype=torch.float64)[:, None]
    tau = ttfb_sample(p.float().to(DEV), S, seed=9).cpu().long()
    surv = torch.cumprod(1 - p.float().double(), dim=1)
    prev = torch.cat([torch.ones(3, 1, dtype=torch.float64), surv[:, :-1]], 1)
    pmf = torch.cat([prev * p.float().double(), surv[:, -1:]], 1)  # P(tau = f), f < F, and P(tau = F)
    for n in range(3):
        counts = torch.bincount(tau[:, n], minlength=F + 1).double()
        sd = torch.sqrt(S * pmf[n] * (1 - pmf[n])).clamp(min=1.0)
        z = (counts - S * pmf[n]).abs() / sd
        assert z.max() < 5.0, (n, z.max())


# ---- fit ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_control", [False, True])
def test_fit_matches_float64_torch(with_control):
    gen = torch.Generator().manual_seed(3)
    data = mixture_draws(gen, 4, 200, zeros=0.05).round()
    data[0, :5] = T  # some censored points besides the natural ones
    control = mixture_draws(gen, 4, 150, ka=0.0, Af=0.0).round() if with_control else None
    dd = data.to(DEV)
    dc = None if control is None else control.to(DEV)
    for steps, tol in ((300, 1e-4), (15000, 1e-3)):
        got = ttfb_fit(dd, T, dc, n_steps=steps)
        want = torch_fit64(data, T, control, n_steps=steps)
        for name in ("ka", "kns", "Af"):
            assert rel(got[name], want[name]) <= tol, (steps, name, got[name].cpu(), want[name])
        assert torch.isfinite(got["loss"]).all()
    # the reported loss is the float64 loss at the parameters of the last step
    par = torch.cat([want["ka"].log(), want["kns"].log(), torch.logit(want["Af"])], 1)
    assert rel(got["loss"], -loglik64(par, data.double(), T, None if control is None else control.double())) < 1e-3


def test_fit_edge_rows():
    data = torch.zeros(3, 100)
    data[1] = T          # all censored
    data[2, :50] = T     # half censored, half at t = 0
    got_state = ttfb_init_state(3, DEV)
    init = got_state.clone()
    ttfb_fit_steps(got_state, data.to(DEV), T, n_steps=2000)
    assert torch.equal(got_state[0], init[0])  # only tau = 0: zero gradient, parameters untouched
    assert torch.isfinite(got_state).all()
    fit = ttfb_fit(data.to(DEV), T, n_steps=15000)
    for name in ("ka", "kns", "Af", "loss"):
        assert torch.isfinite(fit[name]).all(), name


def test_chunked_equals_single_launch():
    gen = torch.Generator().manual_seed(4)
    data = mixture_draws(gen, 64, 300).round().to(DEV)
    control = mixture_draws(gen, 64, 40, ka=0.0, Af=0.0).round().to(DEV)
    one = ttfb_fit(data, T, control, n_steps=3000, chunk=3000)
    chunked = ttfb_fit(data, T, control, n_steps=3000, chunk=700)
    for name in ("ka", "kns", "Af", "loss"):
        assert torch.equal(one[name], chunked[name]), name


def test_lds_and_l2_paths_agree():
    gen = torch.Generator().manual_seed(5)
    data = mixture_draws(gen, 8, 1000, zeros=0.1).round().to(DEV)
    staged = ttfb_fit(data, T, n_steps=1000, stage_lds=True)
    l2 = ttfb_fit(data, T, n_steps=1000, stage_lds=False)
    for name in ("ka", "kns", "Af"):
        assert rel(l2[name], staged[name]) < 1e-5, name
    # rows longer than the LDS budget (TQ_TTFB_LDS_POINTS = 8192) take the L2 path on their own
    big = mixture_draws(gen, 3, 10000, zeros=0.1).round()
    got = ttfb_fit(big.to(DEV), T, n_steps=300)
    want = torch_fit64(big, T, n_steps=300)
    for name in ("ka", "kns", "Af"):
        assert rel(got[name], want[name]) <= 1e-4, name


def test_recovery_of_known_rates():
    """2000 first-binding times per data set from ka = 0.02, kns = 0.002, Af = 0.7, T = 1000, 8 data sets.  Tolerance:
    the asymptotic standard error of the MLE, from the float64 Fisher information (Hessian of the log-likelihood at the
    truth) in the unconstrained parameters; every fit lies within 5 standard errors, their mean within 5 / sqrt(8)."""
    truth = torch.tensor([[math.log(0.02), math.log(0.002), math.log(0.7 / 0.3)]], dtype=torch.float64)
    gen = torch.Generator().manual_seed(6)
    data = mixture_draws(gen, 8, 2000)
    fit = ttfb_fit(data.to(DEV), T, n_steps=15000)
    est = torch.cat([fit["ka"].log(), fit["kns"].log(), torch.logit(fit["Af"])], 1).double().cpu()
    info = -torch.autograd.functional.hessian(lambda p: loglik64(p, data[:1].double(), T).sum(), truth)
    se = torch.sqrt(torch.diagonal(torch.linalg.inv(info.reshape(3, 3))))
    zs = (est - truth) / se
    assert zs.abs().max() < 5.0, zs
    assert (zs.mean(0).abs() < 5.0 / math.sqrt(8)).all(), zs.mean(0)
    kns_ratio = fit["kns"].mean().item() / 0.002
    print(f"fitted means ka={fit['ka'].mean().item():.4g} kns={fit['kns'].mean().item():.4g} "
          f"Af={fit['Af'].mean().item():.4g} (kns ratio {kns_ratio:.3f}); z = {zs.abs().max().item():.2f}")


# ---- command line -------------------------------------------------------------------------------------------------
def test_ttfb_command_end_to_end(tmp_path):
    runner = CliRunner()
    save(simulate(2, 8, 30, 1, 14, params=dict(TEST_PARAMS)), tmp_path)
    result = runner.invoke(app, ["--cd", str(tmp_path), "fit", "--model", "cosmos", "--nbatch-size", "8", "--fbatch-size",
                                 "30", "--num-iter", "2", "--cuda", "--no-input"])
    assert result.exit_code == 0, result.output
    result = runner.invoke(app, ["--cd", str(tmp_path), "ttfb", "--num-samples", "50", "--num-iter", "200", "--cuda",
                                 "--no-input"])
    assert result.exit_code == 0, result.output
    n_on = 4  # simulate: the first half of the AOIs are on target, all selected by the mask
    pts = pd.read_csv(tmp_path / "cosmos_ttfb-data-points-channel0.csv", index_col=0)
    assert pts.shape == (50, n_on) and list(pts.index) == list(range(50))
    assert np.isfinite(pts.values).all() and ((pts.values >= 0) & (pts.values <= 30)).all()
    par = pd.read_csv(tmp_path / "cosmos_ttfb-params-channel0.csv", index_col=0)
    assert list(par.index) == ["ka", "kns", "Af"] and list(par.columns) == ["Mean", "95% LL", "95% UL"]
    v = par.values
    assert np.isfinite(v).all()
    slack = 1e-6 * np.abs(v[:, 0])  # a constant column: the float32 mean may differ from its value in the last bit
    assert (v[:, 1] <= v[:, 0] + slack).all() and (v[:, 0] <= v[:, 2] + slack).all()
    fb = pd.read_csv(tmp_path / "cosmos_ttfb-fraction-bound-channel0.csv", index_col=0)
    assert list(fb.columns) == ["time", "best fit", "fraction bound mean", "fraction bound 95% ll", "fraction bound 95% ul"]
    assert fb.shape == (30, 5) and list(fb["time"]) == list(range(30))
    assert np.isfinite(fb.values).all()
    assert (fb["fraction bound 95% ll"] <= fb["fraction bound 95% ul"]).all()
    try:
        import matplotlib  # noqa: F401
    except ImportError:
        return
    for f in ("cosmos_ttfb-rastergram-channel0.png", "cosmos_ttfb-plot-channel0.png"):
        assert (tmp_path / f).is_file(), f
