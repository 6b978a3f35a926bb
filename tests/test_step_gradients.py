"""
Per-element gradient checks of whole steps (helpers: oracle_grads32, recover_step_gradient, assert_gradients_match,
check_step, lr0_sequence), run here without a GPU:

  * on the host build of the kernels' math (HostCheckEngine), dense and lazy Adam: every replayed step asserts the recovered
    gradient of EVERY parameter against the oracle per element, the second moments and the update;
  * on the oracle alone: the checks accept the reference's own float32 evaluation and reject the errors the parameter
    checks of the replays cannot see -- and three Adam steps in float64 show why those cannot.

Why parameters cannot show a gradient error: Adam's update is invariant to a persistent per-element factor on the gradient,
and its first step is lr sign(g) (tapqir/models/model.py:169-183 runs pyro.optim.Adam, betas (0.9, 0.999)).
"""

import pytest
import torch

from helpers import (ADAM_B1, EPS32, PARAM_ATOL, LOCAL_NAMES, HostCheckEngine, assert_gradients_match, fp32_latents,
                     gradient_report, lr0_sequence, make_dataset, make_oracle, oracle_grads, oracle_grads32, oracle_to_engine,
                     recover_step_gradient, rel_err, replay_steps)

pytestmark = pytest.mark.usefixtures("gradient_report")
assert gradient_report  # (a fixture: imported for pytest to find it)

HOST_CASES = [
    # id, K, dataset kwargs, nb, fb
    ("K2_full_batch", 2, dict(N=4, F=6), None, None),
    ("K2_minibatch_3x17", 2, dict(N=5, F=24), 3, 17),
    ("K3_hist_masked_aoi_3x16", 3, dict(N=4, F=20, offsets="hist", mask=torch.tensor([True, False, True, True])), 3, 16),
]


def host_engine(K, dkw, lazy, perturb=0.3):
    d = make_dataset(K=K, **dkw)
    o = make_oracle(d, K, perturb=perturb)
    o.make_optim(lr=0.005)
    eng = HostCheckEngine(d, K=K, device="cpu", seed=11)
    eng.lazy_adam = lazy
    oracle_to_engine(o, eng)
    return d, o, eng


def subsampler(N, F, nb, fb, seed=5):
    g = torch.Generator().manual_seed(seed)

    def draw():
        if nb is None:
            return None, None
        return torch.randperm(N, generator=g)[:nb], torch.randperm(F, generator=g)[:fb]
    return draw


@pytest.mark.parametrize("lazy", [False, True], ids=["dense", "lazy"])
@pytest.mark.parametrize("name,K,dkw,nb,fb", HOST_CASES, ids=[c[0] for c in HOST_CASES])
def test_host_build_steps_gradients_moments_and_updates(name, K, dkw, nb, fb, lazy):
    """Three steps of the g++ build of the kernels' math, each replayed by the oracle: replay_steps asserts the recovered
    gradient of all 20 parameter families per element, exp_avg_sq and the update from the engine's own moments.
    Measured: worst excess over the relative term 0.51 E32 (budget 16), parameters from own moments within 4e-7."""
    N, F = dkw["N"], dkw["F"]
    d, o, eng = host_engine(K, dkw, lazy)
    draw = subsampler(N, F, nb, fb)

    def step(eng, it):
        nd, fd = draw()
        eng.step(nd, fd)
        return (torch.arange(N), torch.arange(F)) if nd is None else (nd, fd)

    replay_steps(eng, o, step, where="host %s %s" % (name, "lazy" if lazy else "dense"))
    assert eng.adam_step == 3


@pytest.mark.parametrize("lazy", [False, True], ids=["dense", "lazy"])
def test_minibatch_after_a_full_batch_step_gives_other_aois_no_gradient(lazy):
    """A full-batch step leaves its gradients in the buffer (only the Adam of minibatch steps clears what it read); the
    minibatch step after it writes the per-AOI gradients of its own AOIs only.  background_mean_loc / background_std_loc of
    the AOIs outside that minibatch must take a zero-gradient update, not the full-batch gradient once more
    (CosmosEngine._open_step clears the buffer at the transition; without that this test fails at step 1)."""
    N, F = 5, 24
    d, o, eng = host_engine(2, dict(N=N, F=F), lazy)
    draw = subsampler(N, F, 3, 17)

    def step(eng, it):
        nd, fd = (None, None) if it == 0 else draw()
        eng.step(nd, fd)
        return (torch.arange(N), torch.arange(F)) if nd is None else (nd, fd)

    replay_steps(eng, o, step, where="host full then minibatch %s" % ("lazy" if lazy else "dense"))


def test_host_build_lazy_clock_without_joins():
    """lr0_sequence on the host build with the lazy clock: six steps, minibatches and one full batch, no join() in between,
    so that units sit out several steps and their moments decay by b1**k at their next visit: the decay count comes from the
    test's own table of last updates."""
    N, F = 5, 24
    d, o, eng = host_engine(2, dict(N=N, F=F), lazy=True)
    draw = subsampler(N, F, 3, 17)
    plan = [dict(zip(("nd", "fd"), draw())) for _ in range(3)] + [dict(nd=None, fd=None)] + \
           [dict(zip(("nd", "fd"), draw())) for _ in range(2)]
    stale = []
    for e in plan:
        e["post"] = lambda eng: stale.append(eng._stale)
    lr0_sequence(eng, o, plan, "host lazy lr0")
    assert stale == [True, True, True, False, True, True] and not eng._stale


# ---- the checks have teeth: the oracle alone, no code under test -------------------------------------------------------------
@pytest.fixture(scope="module")
def k2_minibatch():
    """Oracle gradients (float64 and plain float32) of the K = 2 minibatch case: 3 x 17 of N = 5, F = 24."""
    N, F = 5, 24
    d = make_dataset(N=N, F=F, K=2)
    o = make_oracle(d, 2, perturb=0.3)
    g = torch.Generator().manual_seed(5)
    nd, fd = torch.randperm(N, generator=g)[:3], torch.randperm(F, generator=g)[:17]
    lat32, base = fp32_latents(o, nd, fd)
    _, g64 = oracle_grads(o, nd, fd, base)
    g32 = oracle_grads32(o, nd, fd, base)
    return {"o": o, "nd": nd, "fd": fd, "g64": g64, "g32": g32, "scale": (3 / N, 17 / F)}


def _zeros(g):
    return {n: torch.zeros_like(v) for n, v in g.items()}


def _old_check(g_dev, g64):
    """The norm-wise check of the staged tests by itself."""
    return all(rel_err(g_dev[n], g64[n]) < 1e-4 for n in g64 if float(g64[n].abs().max()) > 0)


def test_fp32_oracle_is_accepted_and_measures_the_budget(k2_minibatch):
    """(a) the reference's own float32 gradients pass as device gradients (excess <= 1 E32 by construction), and for the
    local and per-AOI families E32 is ~1e-6 of the family's largest gradient: the element-wise check is far tighter than
    1e-4 max|g| for small elements.  The ten GLOBAL families are sums over every unit of the batch, which plain fp32 torch
    gets to 3e-5 .. 1.8e-4 of the gradient depending on the draws (proximity_loc / _size worst; six draw seeds measured):
    there the norm-wise check, which the fp32 oracle itself can miss, is the one that binds, and the element-wise one adds
    nothing -- the kernels accumulate those sums in double."""
    c = k2_minibatch
    per_unit = [n for n in c["g64"] if n in LOCAL_NAMES or n.startswith("background_")]
    assert len(per_unit) == 12 and len(c["g64"]) == 20
    sub = lambda g: {n: g[n] for n in per_unit}
    worst = assert_gradients_match(sub(c["g32"]), sub(c["g64"]), c["g32"], _zeros(c["g64"]), "fp32 oracle")
    assert max(worst.values()) <= 1.0
    for n in per_unit:
        ref = c["g64"][n]
        e32 = float((c["g32"][n] - ref).abs().max())
        assert 0 < e32 <= 2e-5 * float(ref.abs().max()), (n, e32, float(ref.abs().max()))


def test_one_small_element_off_by_one_percent_is_rejected(k2_minibatch):
    """(b) one element whose gradient is small next to its family's largest, multiplied by 1.01: the norm-wise check alone
    accepts it, the element-wise check names it."""
    c = k2_minibatch
    ref = c["g64"]["h_loc"]
    flat = ref.abs().reshape(-1)
    small = (flat > 0) & (0.01 * flat < 0.9e-4 * flat.max())  # 1 % of it is inside the norm-wise tolerance
    e32 = float((c["g32"]["h_loc"] - ref).abs().max())
    small &= 0.01 * flat > 1e-4 * flat + 20 * e32  # ... and beyond the whole element-wise budget
    assert bool(small.any())
    at = int(torch.nonzero(small)[0])
    bad = {n: v.clone() for n, v in c["g64"].items()}
    bad["h_loc"].view(-1)[at] *= 1.01
    assert _old_check(bad, c["g64"])
    with pytest.raises(AssertionError, match=r"element-wise.* of h_loc\[%d\]" % at):
        assert_gradients_match(bad, c["g64"], c["g32"], _zeros(c["g64"]), "one element x 1.01")


@pytest.mark.parametrize("kind", ["doubled", "plate_scale_forgotten_on_the_aoi_axis"])
def test_scaled_local_gradients_are_rejected(k2_minibatch, kind):
    """(c) every local family multiplied by 2; (d) multiplied by nb / Nt, the plate scale Nt/nb F/fb forgotten on one axis."""
    c = k2_minibatch
    factor = 2.0 if kind == "doubled" else c["scale"][0]
    bad = {n: v * factor if n in LOCAL_NAMES else v.clone() for n, v in c["g64"].items()}
    with pytest.raises(AssertionError, match="element-wise"):
        assert_gradients_match(bad, c["g64"], c["g32"], _zeros(c["g64"]), kind)


def test_gradient_on_a_unit_outside_the_minibatch_is_rejected(k2_minibatch):
    """A unit the oracle gives no gradient must have none: 8 E32, inside the absolute allowance of the element-wise check,
    is rejected by the zero-gradient check alone."""
    c = k2_minibatch
    ref = c["g64"]["w_mean"]
    e32 = float((c["g32"]["w_mean"] - ref).abs().max())
    outside = torch.nonzero(ref.reshape(-1) == 0)
    assert len(outside) > 0
    bad = {n: v.clone() for n, v in c["g64"].items()}
    bad["w_mean"].view(-1)[int(outside[0])] = 8 * e32
    with pytest.raises(AssertionError, match="gradient where the oracle has none"):
        assert_gradients_match(bad, c["g64"], c["g32"], _zeros(c["g64"]), "leak")


def test_recovery_rounding_is_what_R_allows(k2_minibatch):
    """recover_step_gradient on moments formed as the kernel forms them (fp32: m = b1 m + (1 - b1) (-g)) from a moment 100
    times the gradient: the recovered gradient is off by the fp32 roundings of the two moments, which R covers and nothing
    else in the budget does; and k steps of decay are undone by b1**k, not by b1."""
    c = k2_minibatch
    f32 = torch.float32
    b1 = torch.tensor(ADAM_B1, dtype=f32)
    g_dev, R, R0 = {}, {}, {}
    for n, ref in c["g64"].items():
        g = ref.to(f32)
        m0 = -100.0 * ref.abs().max().to(f32) * torch.ones_like(g)
        m1 = b1 * m0 + (1.0 - b1) * -g
        g_dev[n], R[n] = recover_step_gradient(m0.double(), m1.double())
        R0[n] = torch.zeros_like(R[n])
        nz = ref != 0  # (the fp32 cast of the gradient itself: one rounding, inside the relative term)
        assert bool(((g_dev[n] - ref).abs()[nz] <= R[n][nz] + EPS32 * ref.abs()[nz]).all())
    assert_gradients_match(g_dev, c["g64"], c["g32"], R, "kernel-formed moments")
    with pytest.raises(AssertionError):
        assert_gradients_match(g_dev, c["g64"], c["g32"], R0, "kernel-formed moments, R dropped")
    # three steps of decay before the update
    ref = c["g64"]["h_loc"]
    m0 = (3.0 * ref + 1.0).to(f32)
    m1 = b1 * (b1 * (b1 * m0)) + (1.0 - b1) * -ref.to(f32)
    g3, R3 = recover_step_gradient(m0.double(), m1.double(), torch.full(ref.shape, 3))
    assert bool(((g3 - ref).abs() <= R3 + EPS32 * ref.abs()).all())
    g1, _ = recover_step_gradient(m0.double(), m1.double())
    assert float((g1 - ref).abs().max()) > 0.1


def test_three_adam_steps_cannot_see_doubled_gradients(k2_minibatch):
    """Why the parameter check of the replays could not see (c): three Adam steps in float64 (lr 0.005, re-synchronised
    parameters as in replay_steps, so the same gradients on both sides) with every gradient doubled end within PARAM_ATOL
    of the true trajectory."""
    c = k2_minibatch
    worst = 0.0
    for n, ref in c["g64"].items():
        p_true, p_twin = (torch.zeros_like(ref).requires_grad_(True) for _ in range(2))
        opts = [torch.optim.Adam([p], lr=0.005, betas=(0.9, 0.999)) for p in (p_true, p_twin)]
        gen = torch.Generator().manual_seed(0)
        for it in range(3):
            g = -ref * (1.0 + 0.3 * torch.randn(ref.shape, generator=gen, dtype=torch.float64))  # a step's gradient of the loss
            p_true.grad, p_twin.grad = g, 2.0 * g
            for opt in opts:
                opt.step()
            worst = max(worst, float((p_true - p_twin).detach().abs().max()))
            p_twin.data.copy_(p_true.data)
    assert worst < PARAM_ATOL, worst
    assert worst > 0  # (not bit-identical: eps = 1e-8 in the denominator is where the factor shows)
