"""
The local guide sites in the regime of a converged fit, on the CPU: the stored site terms of the g++ build of the kernels'
inline math (tests/hostcheck: tq_body_site, i.e. tq_gamma_site_terms and tq_affine_beta_site_terms with
tq_beta_grad_pair_mid / tq_beta_grad_pair_rest) against the plain float64 reference of site_fixture.py, element by element
within site_fixture.site_budget, at parameters spread as a converged fit spreads them (site_fixture.converged_parameters:
Beta concentrations from 0.03 to 3000, Gamma concentrations from 0.1 to 3000) -- every other test of the suite starts from the
initial parameters, where every AffineBeta draw is in the saddle-point pair regime of torch's piecewise _dirichlet_grad.

The host build has no workgroup, no LDS queue and no wave: tq_site_beta_compact (tq_beta_compact.h) is device-only and runs in
test_gpu_site_regimes.py, which takes the runner and the cases from here.  This file says that the MATH holds in these regimes
and that the reference, the allowance and the inputs (regime counts per site row and per wave) are what the GPU tests need.

Two traps of the harness ("Guide sites in the converged regime"), both removed by site_fixture.interior:
a float64-clamped oracle draw can sit on the support bound once rounded to float32 (log q = +inf), and a draw exactly on the
float32 clamp value gets no pathwise gradient from the kernel while the float64 oracle differentiates through it.

Not pinned here: the restated regime rule (site_fixture.grad_regime) against torch itself.  torch offers no way to evaluate
one branch of _dirichlet_grad by itself, so "the branch the rule names agrees with torch" cannot be formed without
restating every branch's series in Python; the rule is restated from the text of torch's _dirichlet_grad_one, and the
hand-placed cases put draws well inside each branch.
"""

import pytest
import torch

from helpers import (GIVEN_STAGES, CosmosEngine, fp32_latents, load_hostcheck, make_dataset, make_oracle, oracle_grads,
                     oracle_to_engine, put_latents)
from site_fixture import (CLASSES, HAND_PLACED, WORST, beta_site_regimes, bounds, check_sites, converged_parameters, hand_placed,
                          interior, kernel_clamped, regime_report, report_lines, site_budget, site_inputs, site_reference,
                          waves)
from test_offset_histograms_host import check

HAND_DKW = dict(N=8, F=32, P=15)  # one full workgroup per site; H = 8, sc = 16: t = (y + 8) / 16 is exact in float32


@pytest.fixture
def site_report(capsys, request):
    """Prints the regime counts of the inputs and the worst error / allowance per stored row of the checks a test ran."""
    WORST.clear()
    REGIMES.clear()
    yield
    with capsys.disabled():
        for line in REGIMES + report_lines(request.node.name):
            print("\n" + line, end="")
    WORST.clear()
    REGIMES.clear()


REGIMES = []
pytestmark = pytest.mark.usefixtures("site_report")


def clamp_masks(o, lat32):
    """{site kind: mask of the draws the kernel calls clamped}: those get no pathwise gradient (torch's clamp passes none)."""
    return {name: kernel_clamped(lat32[name], lo, hi, o.eps) for name, (lo, hi) in bounds(o).items()}


def converged_case(dkw, K, device="cpu", hand=None, prepare=None):
    """Data set, oracle at the converged parameters, engine (host build on "cpu") and the oracle's float32 guide draws moved
    into the interior; ``hand``: a case of site_fixture.HAND_PLACED written over the x / y sites.  Returns
    (oracle, engine, AOI indices, frame indices, latents, base draws, expected tasks per class or None)."""
    gpu = device != "cpu"
    d = make_dataset(K=K, **dkw)
    o = converged_parameters(make_oracle(d, K, perturb=0.3), seed=5)
    eng = CosmosEngine(d, K=K, device=device, lib=None if gpu else load_hostcheck())
    if prepare is not None:
        prepare(eng)
    nd, fd = torch.arange(d.images.shape[0]), torch.arange(d.images.shape[1])
    lat32, _ = fp32_latents(o, nd, fd)
    lat32 = interior(lat32, o)
    tasks = hand_placed(hand, o, lat32) if hand is not None else None
    oracle_to_engine(o, eng)
    with torch.no_grad():
        base = o.base_draws(lat32, o._guide_dists(o.constrained(o.params), nd, fd))
    return o, eng, nd, fd, lat32, base, tasks


def stored_sites(eng):
    """(site rows (5, 1 + 4K, B), draws (1 + 4K, B)) of the engine's workspace, float64 on the host."""
    S = 1 + 4 * eng.K
    return eng.site.detach().cpu().double().view(5, S, -1), eng.lat.detach().cpu().double().view(S, -1)


def run_given_sites(dkw, K, where, device="cpu", hand=None, prepare=None, whole_step=True):
    """Given draws through the staged calls: every stored row against the reference within the allowance, then ELBO and
    gradients against the oracle (test_offset_histograms_host.check; the oracle detaches the draws the kernel calls
    clamped).  Returns (engine, inputs of the reference, expected tasks per class)."""
    o, eng, nd, fd, lat32, base, tasks = converged_case(dkw, K, device, hand, prepare)
    elbo_o, g_o = oracle_grads(o, nd, fd, base, detach=clamp_masks(o, lat32))
    a = eng.make_args(None, None, draw_globals=False)
    put_latents(eng, lat32, base)
    for stage in GIVEN_STAGES if whole_step else GIVEN_STAGES[:2]:
        eng.call(stage, a)
    if device != "cpu":
        torch.cuda.synchronize()
    inp = site_inputs(o, nd, fd, lat32)
    REGIMES.extend("%s %s" % (where, line) for line in regime_report(inp))
    site, lat = stored_sites(eng)
    assert torch.equal(lat, torch.cat([lat32["background"].reshape(1, -1)] + [lat32[n].reshape(K, -1) for n in
                                                                              ("height", "width", "x", "y")]))
    ref = site_reference(inp)
    check_sites(site, inp, ref, site_budget(inp, ref), where)
    if whole_step:
        check(o, eng, elbo_o, g_o)
    return eng, inp, tasks


def assert_converged_mix(inp, at_least=30):
    """What the 300-unit case is built for: per AffineBeta site row at least ``at_least`` evaluations in each of the pair,
    x-small, (1-x)-small and rational classes, every wave mixed, no draw on a clamp value."""
    assert not bool(inp["clamped"].any())
    for s, k in beta_site_regimes(inp).items():
        n = k.sum(1)
        for c in (0, 1, 2, 4):
            assert int(n[c]) >= at_least, (s, CLASSES[c], n.tolist())
        assert all(w[4] for w in waves(k)), (s, [(w[0], w[1], w[4]) for w in waves(k)])


def assert_hand_placed(inp, tasks, case):
    """The x and y site rows of a hand-placed case hold the tasks the lanes were chosen for, and the clamped draws are where
    they were put."""
    K = inp["K"]
    kinds = HAND_PLACED[case]
    want_clamped = torch.tensor([k.startswith("clamp") for k in kinds])
    for s, k in beta_site_regimes(inp).items():
        if s >= 1 + 2 * K:
            assert k.sum(1).tolist() == tasks.tolist(), (case, s, k.sum(1).tolist(), tasks.tolist())
            assert torch.equal(inp["clamped"][s], want_clamped)


# ---- random converged parameters --------------------------------------------------------------------------------------------
def test_300_units_converged_mix():
    """N = 10, F = 30, K = 2: the case the regime counts are asserted on (two workgroups per site on the device)."""
    eng, inp, _ = run_given_sites(dict(N=10, F=30), 2, "N=10 F=30 K=2")
    assert_converged_mix(inp)


@pytest.mark.parametrize("P", [14, 15])
@pytest.mark.parametrize("C", [1, 2])
@pytest.mark.parametrize("K", [1, 2, 3])
def test_converged_parameters(K, C, P):
    eng, inp, _ = run_given_sites(dict(N=3, F=16, C=C, P=P), K, "K=%d C=%d P=%d" % (K, C, P))
    assert not bool(inp["clamped"].any())
    assert (eng.K, eng.C, eng.P) == (K, C, P)


# ---- hand-placed workgroups -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(HAND_PLACED))
def test_hand_placed(case):
    eng, inp, tasks = run_given_sites(HAND_DKW, 1, case, hand=case)
    assert_hand_placed(inp, tasks, case)
    if case == "clamp_values":
        site, _ = stored_sites(eng)
        on = inp["clamped"][3:]
        assert int(on.sum()) == 2 * 128
        assert bool((site[2, 3:][on] == 0).all()) and bool((site[4, 3:][on] == 0).all())
        assert bool(torch.isfinite(site[0, 3:][on]).all())


# ---- the box of the allowance -----------------------------------------------------------------------------------------------
def test_inputs_of_the_build_lie_in_the_box():
    """The float32 t, c1, c0 (v, alpha, beta) the host build evaluates its site terms at (hc_cosmos_site_inputs) against the
    reference's inputs: inside the box site_budget spreads the reference over, and the implicit gradients and the
    derivatives of log q at the build's OWN inputs are inside the floor alone -- what is left of them is arithmetic."""
    # (log q itself is not held to the floor alone: t T - c1 of the Binet form is rounded at the magnitude of c1 by g++,
    # where the device contracts it into one fused multiply-add)
    import ctypes as C

    o, eng, nd, fd, lat32, base, _ = converged_case(dict(N=10, F=30), 2)
    a = eng.make_args(None, None, draw_globals=False)
    put_latents(eng, lat32, base)
    for stage in GIVEN_STAGES[:2]:
        eng.call(stage, a)
    inp = site_inputs(o, nd, fd, lat32)
    S, B = inp["a"].shape
    buf = torch.zeros(3, S, B, dtype=torch.float32)
    eng.lib.hc_cosmos_site_inputs(C.byref(a), C.c_void_p(buf.data_ptr()))
    own = dict(inp)
    for j, (name, d) in enumerate((("a", "da"), ("b", "db"), ("c", "dc"))):
        own[name] = buf[j].double()
        off = (own[name] - inp[name]).abs()
        assert bool((off <= inp[d]).all()), (name, float((off / inp[d].clamp(min=1e-300)).max()))
    ref = site_reference(own)
    floor = site_budget(own, ref, box=0.0)
    site, _ = stored_sites(eng)
    # (the upper half of the support is left out: there the build takes 1 - t from the draw, not from its rounded t)
    err = torch.where((own["a"] < 0.5) | (own["sc"] == 0)[:, None], (site - ref).abs(), torch.zeros_like(ref))
    for r in (1, 2, 3, 4):
        rows = slice(0, S) if r <= 2 else slice(1 + inp["K"], S)
        assert bool((err[r, rows] <= floor[r, rows]).all()), (r, float((err[r, rows] / floor[r, rows].clamp(min=1e-300)).max()))


# ---- draws of the build itself ----------------------------------------------------------------------------------------------
def latents_of(eng, shape):
    """The local draws of the engine's workspace as an oracle-style dict (float64 holding float32), batch shape ``shape``."""
    K = eng.K
    _, lat = stored_sites(eng)
    out = {"background": lat[0].reshape(shape)}
    for j, n in enumerate(("height", "width", "x", "y")):
        out[n] = lat[1 + j * K:1 + (j + 1) * K].reshape(K, *shape)
    return out


def drawn_sites(dkw, K, where, device="cpu"):
    """One sampling launch that draws its local sites (draw_locals) at the converged parameters: every stored row against the
    reference AT THE READ-BACK DRAWS (draws on a clamp value stay in, classified by kernel_clamped), and a second identical
    launch bitwise equal in draws and site terms.  Returns (oracle, engine, argument block, reference inputs, site rows, draws)."""
    o, eng, nd, fd, _, _, _ = converged_case(dkw, K, device)
    a = eng.make_args(None, None, draw_globals=False, draw_locals=True)
    eng.site.fill_(float("nan"))
    eng.call("cosmos_sample_locals", a)
    if device != "cpu":
        torch.cuda.synchronize()
    site, lat = stored_sites(eng)
    site, lat = site.clone(), lat.clone()
    inp = site_inputs(o, nd, fd, latents_of(eng, (len(nd), len(fd), eng.C)))
    REGIMES.extend("%s %s" % (where, line) for line in regime_report(inp))
    ref = site_reference(inp)
    check_sites(site.nan_to_num(nan=0.0), inp, ref, site_budget(inp, ref), where)
    assert bool(torch.isnan(site[3:, :1 + K]).all()), "a Gamma site wrote rows it does not have"
    assert bool(torch.isfinite(site[:3]).all()) and bool(torch.isfinite(site[3:, 1 + K:]).all())
    on = inp["clamped"]
    assert bool((site[2][on] == 0).all()) and bool((site[4][on] == 0).all())
    eng.call("cosmos_sample_locals", a)
    if device != "cpu":
        torch.cuda.synchronize()
    site2, lat2 = stored_sites(eng)
    assert torch.equal(lat2, lat) and torch.equal(site2[:3], site[:3]) and torch.equal(site2[3:, 1 + K:], site[3:, 1 + K:])
    return o, eng, a, inp, site, lat


def law_of_the_draws(inp):
    """Kolmogorov-Smirnov p-values of the pooled probability-integral transforms (float64 cdfs from scipy) of the AffineBeta
    draws and of the Gamma draws against the uniform law; draws on a clamp value are left out, and are fewer than 3 %."""
    from scipy import stats

    K = inp["K"]
    a, b, c = (inp[n].numpy() for n in ("a", "b", "c"))
    keep = ~inp["clamped"][1 + K:].numpy()
    assert (~keep).mean() < 0.03, (~keep).mean()
    u_beta = stats.beta.cdf(a[1 + K:], b[1 + K:], c[1 + K:])[keep]
    tiny = float(torch.finfo(torch.float32).tiny)
    keep_g = a[:1 + K] > tiny
    assert (~keep_g).mean() < 0.03, (~keep_g).mean()
    u_gamma = stats.gamma.cdf(a[:1 + K] * c[:1 + K], b[:1 + K])[keep_g]
    return stats.kstest(u_beta, "uniform").pvalue, stats.kstest(u_gamma, "uniform").pvalue, u_beta.size, u_gamma.size


def test_draws_of_the_host_build():
    """tq_site_draw / tq_sample_std_gamma of the g++ build at concentrations from 0.03 to 3000: site terms at its own draws,
    a repeat bit for bit, and the law of the draws (p > 1e-4, the bar of test_math.py)."""
    o, eng, a, inp, site, lat = drawn_sites(dict(N=10, F=30), 2, "host draws")
    p_beta, p_gamma, n_beta, n_gamma = law_of_the_draws(inp)
    REGIMES.append("host draws: KS p-value AffineBeta %.3g (%d draws)  Gamma %.3g (%d draws)" % (p_beta, n_beta, p_gamma, n_gamma))
    assert p_beta > 1e-4 and p_gamma > 1e-4, (p_beta, p_gamma)


# ---- whole steps ------------------------------------------------------------------------------------------------------------
def converged_step_case(dkw, K, device="cpu", seed=11, **attrs):
    """Oracle with optimiser and engine at the converged parameters, for helpers.replay_steps."""
    d = make_dataset(K=K, **dkw)
    o = converged_parameters(make_oracle(d, K, perturb=0.3), seed=5)
    o.make_optim(lr=0.005)
    eng = CosmosEngine(d, K=K, device=device, seed=seed, lib=None if device != "cpu" else load_hostcheck())
    for n, v in attrs.items():
        setattr(eng, n, v)
    oracle_to_engine(o, eng)
    return d, o, eng


def test_whole_steps_of_the_host_build():
    """Three steps of the g++ build at the converged parameters, replayed by the oracle with the draws the kernel calls
    clamped detached (helpers.replay_steps, ``clamped``): the per-element gradient budgets of assert_gradients_match."""
    from helpers import gradient_report  # noqa: F401  (the figures are printed by the modules that use the fixture)
    from helpers import replay_steps

    N, F = 4, 16
    d, o, eng = converged_step_case(dict(N=N, F=F), 2)

    def step(eng, it):
        eng.step()
        return torch.arange(N), torch.arange(F)

    replay_steps(eng, o, step, steps=3, where="host converged", clamped=clamp_masks)
