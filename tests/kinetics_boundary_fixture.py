"""Cases, references and bounds of the kinetics boundary tests (test_gpu_kinetics_boundaries.py on the device,
test_kinetics_boundaries_host.py on the g++ replays): one Adam step of ``tq_dwell_fit`` / ``tq_ttfb_fit`` taken apart into
its gradient, loss and update, at every K and at the row lengths where the kernels change what they do.

How a step is taken apart.  A launch with ``n_steps = 1``, ``step0 = 0`` from zero moments leaves m = w1 g and
v = w2 g^2 in the state (w1 = float32(1 - beta1), w2 = float32(1 - beta2)), so g = m / w1 to one rounding and
|g| = sqrt(v / w2); ``loss`` is the loss at the parameters the step starts from.  g and the loss are compared with float64
autograd of the fixtures' log-likelihoods at the same float32 parameters; p after the step is compared with
``torch.optim.Adam`` in float64 applied to the recovered g.

The rule.  Per row, |g - g64| <= max(32 max_j |g32 - g64|, 1e-6 max_j |g64|), g32 the same torch log-likelihood in
float32: the bound is the float32 noise of the reference itself, relative to the row's largest component (components as
small as 1e-5 of it occur).  The loss follows the same rule with |loss64|.  Nothing in the bound comes from the code
under test."""

import ctypes as C
import functools

import numpy as np
import torch

import dwell_fixture
import ttfb_fixture

EPS32 = float(torch.finfo(torch.float32).eps)
LR, BETA1, BETA2, ADAM_EPS = 5e-3, 0.9, 0.999, 1e-8
W1 = float(np.float32(1.0 - BETA1))
W2 = float(np.float32(1.0 - BETA2))
UPDATE_ULPS = 4  # bound of the update checks: this many float32 eps of the magnitudes that enter the quantity


# ---- the rule ---------------------------------------------------------------------------------------------------------
def rule_bound(x32, x64):
    """Per row: max(32 max_j |x32 - x64|, 1e-6 max_j |x64|); x (S, J) or (S,)."""
    x32, x64 = x32.double().reshape(x64.shape[0], -1), x64.double().reshape(x64.shape[0], -1)
    return torch.maximum(32.0 * (x32 - x64).abs().amax(1), 1e-6 * x64.abs().amax(1))


def rule_excess(x, x32, x64):
    """Per row: max_j |x - x64| over the rule's bound: at most 1 when x is within the rule (0 / 0 counts as 0)."""
    err = (x.double().reshape(x64.shape[0], -1) - x64.double().reshape(x64.shape[0], -1)).abs().amax(1)
    bound = rule_bound(x32, x64)
    return torch.where(err == 0, torch.zeros_like(err), err / bound)


def recover_gradient(after, P):
    """(g, |g| from v) of a first step from zero moments: ``after`` (S, 3P) float32 state of the launch."""
    m, v = after[:, P:2 * P].double(), after[:, 2 * P:3 * P].double()
    return m / W1, (v / W2).sqrt()


def adam_step64(p, m, v, g, t, lr=LR):
    """Optimiser step ``t`` (1-based) of torch.optim.Adam in float64 from parameters p, moments m, v and gradient g:
    (p, m, v) after it."""
    par = p.double().clone().requires_grad_(True)
    opt = torch.optim.Adam([par], lr=lr, betas=(BETA1, BETA2), eps=ADAM_EPS)
    par.grad = g.double().clone()
    opt.state[par] = {"step": torch.tensor(float(t - 1)), "exp_avg": m.double().clone(), "exp_avg_sq": v.double().clone()}
    opt.step()
    return par.detach(), opt.state[par]["exp_avg"], opt.state[par]["exp_avg_sq"]


def update_excess(before, after, g, t, P):
    """Worst error of (p, m, v) after step ``t`` over its bound, against ``adam_step64`` from ``before`` (S, 3P) with
    gradient g.  Bounds, UPDATE_ULPS float32 eps of what enters each quantity: |p'| + |update| for p (the update goes
    through six roundings, the subtraction through one), |m| + w1 |g - m| for m, v' for v (plus the smallest normal
    float32: a flushed denormal is no error)."""
    b, a = before.double(), after.double()
    p0, m0, v0 = b[:, :P], b[:, P:2 * P], b[:, 2 * P:]
    p1, m1, v1 = adam_step64(p0, m0, v0, g, t)
    ulp = UPDATE_ULPS * EPS32
    bound = torch.cat([ulp * (p1.abs() + (p1 - p0).abs()), ulp * (m0.abs() + W1 * (g - m0).abs()) + 1.2e-38,
                       ulp * v1 + 1.2e-38], 1)
    err = (a - torch.cat([p1, m1, v1], 1)).abs()
    return torch.where(err == 0, torch.zeros_like(err), err / bound).amax(1)


def step_report(before, after, loss, ref, P):
    """Everything section 1 measures of one first-step launch, per row: {"grad", "loss", "v", "update"} excesses (each at
    most 1 when the launch is within its bound).  "v": |sqrt(v / w2) - |g|| over 4 eps32 |g| + 1e-17 (v = w2 g^2 has two
    roundings; below 1e-17 it is a float32 denormal)."""
    g, gabs = recover_gradient(after, P)
    return {"grad": rule_excess(g, ref["g32"], ref["g64"]),
            "loss": rule_excess(loss, ref["loss32"], ref["loss64"]),
            "v": ((gabs - g.abs()).abs() / (4.0 * EPS32 * g.abs() + 1e-17)).amax(1),
            "update": update_excess(before, after, g, 1, P)}


def worst(report):
    """{name: (worst excess, its row)} of a ``step_report``."""
    return {k: (float(v.max()), int(v.argmax())) for k, v in report.items()}


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ---- dwell: rows, states, reference -------------------------------------------------------------------------------------
DWELL_LENS = (0, 1, 2, 63, 64, 65, 127, 128, 129, 2047, 2048, 2049, 4097)  # around the wave and TQ_DWELL_LDS_PAIRS = 2048
DWELL_STATES = ("initial", "perturbed", "vertex", "far_vertex")
OUTLIER = 1.0e4


def dwell_draws(gen, S, M, k=(0.1, 0.01), A=(0.6, 0.4)):
    """S x M continuous dwell times of the mixture sum_j A_j k_j exp(-k_j t) (``mixture_draws`` of test_gpu_dwelltime)."""
    u = torch.rand(S, M, generator=gen, dtype=torch.float64)
    comp = torch.searchsorted(torch.cumsum(torch.tensor(A, dtype=torch.float64), 0), u.reshape(-1)).reshape(S, M)
    rate = torch.tensor(k, dtype=torch.float64)[comp.clamp(max=len(k) - 1)]
    return (-torch.log(torch.rand(S, M, generator=gen, dtype=torch.float64)) / rate).float()


@functools.lru_cache(maxsize=None)
def dwell_rows():
    """The CSR (values, weights, row_ptr) of one row per length of DWELL_LENS: rounded mixture draws >= 1; even rows have
    unit weights, odd rows integer weights 1 .. 50 with one weight of 1e4; the last pair of a row of two or more is an
    outlier at t = 1e4, so a dropped tail element moves every sum."""
    gen = torch.Generator().manual_seed(20261020)
    vals, wts = [], []
    for r, n in enumerate(DWELL_LENS):
        t = dwell_draws(gen, 1, max(n, 1))[0, :n].round().clamp(min=1.0)
        w = torch.ones(n)
        if r % 2 == 1 and n:
            w = torch.randint(1, 51, (n,), generator=gen).float()
            w[0] = 1.0e4
        if n >= 2:
            t[-1] = OUTLIER
        vals.append(t)
        wts.append(w)
    row_ptr = torch.zeros(len(DWELL_LENS) + 1, dtype=torch.int64)
    row_ptr[1:] = torch.cumsum(torch.tensor(DWELL_LENS), 0)
    return torch.cat(vals).contiguous(), torch.cat(wts).contiguous(), row_ptr


def dwell_par0(K, kind, S=len(DWELL_LENS)):
    """(S, 2K) float32 parameters: the reference's initial state; that plus N(0, 0.5^2) in every coordinate; or the vertex
    state: rates spread over 1e-5 .. 10, one softmax logit at +12 (column row % K) and the others at -12.  "far_vertex" is
    the vertex state with logits of +-50: their spread of 100 is past ln(FLT_MAX) = 88.7, the only regime in which the
    max-shift of the softmax in ``tq_dwell_consts`` changes the result (at +-12 an unshifted e^24 is still a float32)."""
    init = dwell_fixture.init_par(S, K).float()
    if kind == "initial":
        return init
    if kind == "perturbed":
        return init + 0.5 * torch.randn(S, 2 * K, generator=torch.Generator().manual_seed(1000 + K))
    logit = {"vertex": 12.0, "far_vertex": 50.0}[kind]
    par = torch.full((S, 2 * K), -logit)
    par[:, :K] = torch.logspace(-5, 1, K, dtype=torch.float32).log()
    par[torch.arange(S), K + torch.arange(S) % K] = logit
    return par


def dwell_state(par0):
    """(S, 6K) float32 Adam state at ``par0`` with zero moments."""
    return torch.cat([par0, torch.zeros(par0.shape[0], 2 * par0.shape[1])], 1).contiguous()


def _dwell_autograd(par0, csr, K, dtype):
    values, weights, row_ptr = csr
    par = par0.to(dtype).clone().requires_grad_(True)
    lls = []
    for s in range(par.shape[0]):
        a, b = int(row_ptr[s]), int(row_ptr[s + 1])
        if a == b:
            lls.append(par[s].sum() * 0.0)
            continue
        # every pair as a sample of its own: loglik64 returns the per-pair terms, weighted and summed here
        terms = dwell_fixture.loglik64(par[s].expand(b - a, 2 * K), values[a:b].to(dtype).unsqueeze(1), K)
        lls.append((weights[a:b].to(dtype) * terms).sum())
    ll = torch.stack(lls)
    (-ll.sum()).backward()
    return par.grad.detach(), (-ll).detach()


def dwell_reference_at(par0, csr, K):
    """Gradient (S, 2K) and loss (S,) of the LOSS at float32 parameters ``par0``: float64 and float32 autograd of
    ``dwell_fixture.loglik64``."""
    g64, loss64 = _dwell_autograd(par0, csr, K, torch.float64)
    g32, loss32 = _dwell_autograd(par0, csr, K, torch.float32)
    return {"g64": g64, "g32": g32, "loss64": loss64, "loss32": loss32}


@functools.lru_cache(maxsize=None)
def dwell_reference(K, kind):
    return dwell_reference_at(dwell_par0(K, kind), dwell_rows(), K)


# ---- ttfb: rows, states, reference ---------------------------------------------------------------------------------------
TTFB_T = 1000.0
TTFB_NS = (1, 2, 63, 64, 65, 127, 128, 129, 8191, 8192, 8193)  # around the wave and TQ_TTFB_LDS_POINTS = 8192
TTFB_CASES = tuple([(N, 0) for N in TTFB_NS] + [(N, 65) for N in TTFB_NS] + [(65, Nc) for Nc in (1, 63, 64)])
TTFB_ROWS = ("draws", "all_zero", "all_T", "one_interior_last", "upper_lanes", "all_interior")
TTFB_STATES = ("initial", "perturbed", "extreme+", "extreme-")
# rows whose two routes add the same numbers in the same lanes: no point, one point, or nothing for the compaction to move
TTFB_SAME_LANES = ("all_zero", "all_T", "one_interior_last", "all_interior")


def ttfb_draws(gen, S, N, ka=0.02, kns=0.002, Af=0.7, Tmax=TTFB_T, zeros=0.0):
    """S x N first-binding times of the model (``mixture_draws`` of test_gpu_ttfb): continuous, censored at Tmax."""
    active = torch.rand(S, N, generator=gen, dtype=torch.float64) < Af
    rate = torch.where(active, torch.tensor(ka + kns, dtype=torch.float64), torch.tensor(kns, dtype=torch.float64))
    t = (-torch.log(torch.rand(S, N, generator=gen, dtype=torch.float64)) / rate).clamp(max=Tmax)
    t = torch.where(torch.rand(S, N, generator=gen, dtype=torch.float64) < zeros, torch.zeros_like(t), t)
    return t.float()


def ttfb_row_names():
    return [f"{row}/{state}" for row in TTFB_ROWS for state in TTFB_STATES]


@functools.lru_cache(maxsize=None)
def ttfb_case(N, Nc):
    """(data (S, N), control (S, Nc) or None, par0 (S, 3)) with S = len(TTFB_ROWS) x len(TTFB_STATES): every composition
    of a row at every state.  Compositions: rounded draws of the model (with zeros and censored points); all 0; all T;
    0 / T alternating with one interior point at index N - 1; 0 / T alternating with interior points only in lanes >= 32
    of the last round of 64 (of the round before it when the last one has no such lane; none when N < 33); interior
    points only."""
    gen = torch.Generator().manual_seed(7000 + 10 * N + Nc)
    T = TTFB_T
    draws = ttfb_draws(gen, 1, N, zeros=0.05)[0].round()
    inner = ttfb_draws(gen, 1, N)[0].round().clamp(1.0, T - 1.0)
    alt = torch.where(torch.arange(N) % 2 == 0, torch.zeros(N), torch.full((N,), T))
    one = alt.clone()
    one[N - 1] = 37.0
    upper = alt.clone()
    r0 = 64 * ((N - 1) // 64)
    idx = [i for i in range(r0, N) if i % 64 >= 32]
    if not idx and r0 >= 64:
        idx = list(range(r0 - 32, r0))
    if idx:
        upper[idx] = inner[idx]
    rows = {"draws": draws, "all_zero": torch.zeros(N), "all_T": torch.full((N,), T), "one_interior_last": one,
            "upper_lanes": upper, "all_interior": inner}
    data = torch.stack([rows[r] for r in TTFB_ROWS for _ in TTFB_STATES]).contiguous()
    S = data.shape[0]
    control = ttfb_draws(gen, S, Nc, ka=0.0, Af=0.0).round().contiguous() if Nc else None
    init = torch.tensor([0.001, 0.001, 0.9], dtype=torch.float32)
    init = torch.stack([init[0].log(), init[1].log(), init[2].logit()])
    extreme = torch.tensor([10.0, 0.002], dtype=torch.float32).log()  # ka T = 1e4
    states = {"initial": lambda: init.clone(), "perturbed": lambda: init + torch.randn(3, generator=gen),
              "extreme+": lambda: torch.cat([extreme, torch.tensor([12.0])]),
              "extreme-": lambda: torch.cat([extreme, torch.tensor([-12.0])])}
    par0 = torch.stack([states[s]() for _ in TTFB_ROWS for s in TTFB_STATES]).float().contiguous()
    return data, control, par0


def ttfb_state(par0):
    return torch.cat([par0, torch.zeros(par0.shape[0], 6)], 1).contiguous()


def _ttfb_autograd(par0, data, control, dtype):
    par = par0.to(dtype).clone().requires_grad_(True)
    ll = ttfb_fixture.loglik64(par, data.to(dtype), TTFB_T, None if control is None else control.to(dtype))
    (-ll.sum()).backward()
    return par.grad.detach(), (-ll).detach()


def ttfb_reference_at(par0, data, control):
    g64, loss64 = _ttfb_autograd(par0, data, control, torch.float64)
    g32, loss32 = _ttfb_autograd(par0, data, control, torch.float32)
    return {"g64": g64, "g32": g32, "loss64": loss64, "loss32": loss32}


@functools.lru_cache(maxsize=None)
def ttfb_reference(N, Nc):
    data, control, par0 = ttfb_case(N, Nc)
    return ttfb_reference_at(par0, data, control)


# ---- step t = 10 000 from non-zero moments ---------------------------------------------------------------------------
def late_state(par0, seed):
    """Adam state at ``par0`` with seeded non-zero moments: m ~ N(0, 1), v = m^2 (1 + U(0, 1)) > 0."""
    gen = torch.Generator().manual_seed(seed)
    m = torch.randn(par0.shape, generator=gen)
    v = m * m * (1.0 + torch.rand(par0.shape, generator=gen)) + 1e-6
    return torch.cat([par0, m, v], 1).contiguous()


def late_step_excess(run, par0, P, seed):
    """``run(state, step0) -> state after one step``: the step at step0 = 9999 from ``late_state`` against step
    t = 10 000 of ``adam_step64``, with the gradient recovered from a first step at the same parameters (the gradient
    depends on neither the moments nor t).  Per row, error over the ``update_excess`` bound."""
    g, _ = recover_gradient(run(torch.cat([par0, torch.zeros(par0.shape[0], 2 * P)], 1).contiguous(), 0), P)
    before = late_state(par0, seed)
    after = run(before.clone(), 9999)
    return update_excess(before, after, g, 10000, P)


# ---- short trajectories at K = 4 .. 8 -------------------------------------------------------------------------------------
TRAJ_KS = (4, 5, 6, 7, 8)
TRAJ_STEPS = 300
TRAJ_TOL = 1e-4  # the project's 300-step bar, relative on k and A


@functools.lru_cache(maxsize=None)
def trajectory_data():
    """The 4 x 300 data of test_gpu_dwelltime.test_fit_matches_float64_torch."""
    gen = torch.Generator().manual_seed(3)
    data = dwell_draws(gen, 4, 300).round().clamp(min=1.0)
    data[1, 250:] = 0.0  # padding
    return data


@functools.lru_cache(maxsize=None)
def trajectory_reference(K):
    """``torch_fit64`` after TRAJ_STEPS steps, and the float64 loss at the parameters the last step starts from."""
    data = trajectory_data()
    want = dwell_fixture.torch_fit64(data, K, n_steps=TRAJ_STEPS)
    before_last = dwell_fixture.torch_fit64(data, K, n_steps=TRAJ_STEPS - 1)["par"]
    return want, -dwell_fixture.loglik64(before_last, data.double(), K)


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float(((a - b).abs() / b.abs()).max())


def padded_csr(data):
    """(values, weights, row_ptr) of zero-padded (S, M) dwell times on the host (``dwell_csr_from_padded``)."""
    nz = data > 0
    row_ptr = torch.zeros(data.shape[0] + 1, dtype=torch.int64)
    row_ptr[1:] = torch.cumsum(nz.sum(1), 0)
    vals = data[nz].float().contiguous()
    return vals, torch.ones_like(vals), row_ptr


# ---- the g++ replays of one launch -------------------------------------------------------------------------------------
def bind_fit_steps(dwell_lib=None, kinetics_lib=None):
    """ctypes signatures of hk_dwell_fit_steps / hk_ttfb_fit_steps on the libraries of build_dwell_check /
    build_kinetics_check."""
    vp = C.c_void_p
    if dwell_lib is not None:
        dwell_lib.hk_dwell_fit_steps.argtypes = [C.c_int, vp, vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_double,
                                                 C.c_double, C.c_double, C.c_double]
        dwell_lib.hk_dwell_fit_steps.restype = C.c_int
    if kinetics_lib is not None:
        kinetics_lib.hk_ttfb_fit_steps.argtypes = [vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                                   C.c_float, C.c_double, C.c_double, C.c_double, C.c_double]
        kinetics_lib.hk_ttfb_fit_steps.restype = None


def host_dwell_steps(lib, state, csr, K, step0=0, n_steps=1, lr=LR):
    """One launch of the g++ replay from ``state`` (S, 6K): (state after, loss (S,))."""
    values, weights, row_ptr = (x.contiguous() for x in csr)
    state = state.clone().contiguous()
    S = row_ptr.shape[0] - 1
    loss = torch.full((S,), float("nan"))
    keep = (values if values.numel() else torch.zeros(1), weights if weights.numel() else torch.zeros(1))
    rc = lib.hk_dwell_fit_steps(K, keep[0].data_ptr(), keep[1].data_ptr(), row_ptr.data_ptr(), state.data_ptr(),
                                loss.data_ptr(), S, step0, n_steps, lr, BETA1, BETA2, ADAM_EPS)
    assert rc == 0, K
    return state, loss


def host_ttfb_steps(lib, state, data, control, staged, step0=0, n_steps=1, lr=LR):
    """One launch of the g++ replay from ``state`` (S, 9), LDS route when ``staged`` (and N <= 8192): (state after,
    loss)."""
    state = state.clone().contiguous()
    data = data.contiguous()
    S, N = data.shape
    loss = torch.full((S,), float("nan"))
    lib.hk_ttfb_fit_steps(data.data_ptr(), None if control is None else control.data_ptr(), state.data_ptr(),
                          loss.data_ptr(), S, N, 0 if control is None else control.shape[1], step0, n_steps,
                          1 if staged and N <= 8192 else 0, TTFB_T, lr, BETA1, BETA2, ADAM_EPS)
    return state, loss
