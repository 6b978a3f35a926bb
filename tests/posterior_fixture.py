"""
The posterior read-out (tq_cosmos_probs: tq_body_probs_globals, tq_body_probs_unit, tq_zt_responsibilities) against the
float64 oracle: the cases, the particles, the reference with its allowance, and the runners.  Every runner takes a backend
-- the g++ build of the kernels' inline math (HOST) or the device (DEVICE) -- so every check exists on both
(test_posterior_host.py, test_gpu_posterior.py) and a failure on the GPU alone points at device code.

Given draws (draw = 0): the oracle's own float32-rounded guide draws, x and y clamped onto the kernel's float32 clamp values
first (an oracle draw can round to +-H exactly, where compute_probs is inf - inf), go to both sides.
Allowance, from the reference alone: the oracle runs a second time in plain float32 on the same particles,
  e_abs = max |o32 - o64|;   e_rel = max |o32 - o64| / o64 over the entries of z_probs[..., 1] and theta_probs with o64 >= 1e-6
  absolute rule  max |got - o64| <= min(2e-5, max(8 e_abs, 2^-22))           every entry, z_probs[..., 0] included
  relative rule  |got - o64| / o64 <= min(1e-3, max(8 e_rel, 2^-17))         the same entries >= 1e-6
(8: the kernel's order of sums and its sigmoid differ from torch's; the floors keep an accidentally exact float32 pass from
making the bound unreachable; the ceilings are the assertion test_posterior.py had.)

Drawn on the backend (draw = 1): hc_probs_xy_draws replays the x / y draws of the host build through the helpers the body
itself calls (tq_probs_spot_guide, tq_probs_draw_coord, tq_probs_elem); the global base draws are read back from gbase_p.
"""

import ctypes as C
import functools
import math

import numpy as np
import torch

from helpers import CosmosEngine, load_hostcheck, make_dataset, make_oracle, oracle_to_engine
from oracle.cosmos import OracleData, working_dtype
from site_fixture import clamp_values, converged_parameters, f32
from tapqir_amd.models.posterior import probs_args, run_probs
from tapqir_amd.utils.dataset import CosmosDataset

EPS32 = float(torch.finfo(torch.float32).eps)
WG = 256  # units per workgroup of tq_probs_kernel
REL_FROM = 1e-6
ABS_CEIL, ABS_FLOOR, REL_CEIL, REL_FLOOR, FACTOR = 2e-5, 2.0 ** -22, 1e-3, 2.0 ** -17, 8.0
KS_LEVEL = 1e-4  # the level of test_math.py and test_gpu_site_regimes.py


class Backend:
    def __init__(self, name, device):
        self.name, self.device = name, device

    @property
    def lib(self):
        return load_hostcheck() if self.device == "cpu" else None

    def engine(self, d, K, crosstalk=False, **kw):
        return CosmosEngine(d, K=K, device=self.device, lib=self.lib, crosstalk=crosstalk, **kw)

    def sync(self):
        if self.device != "cpu":
            torch.cuda.synchronize()


HOST, DEVICE = Backend("host", "cpu"), Backend("MI355X", "cuda:0")

# ---- the cases ----------------------------------------------------------------------------------------------------------------
# name -> dataset, K, particles, crosstalk, regime ("perturbed": make_oracle(perturb=0.4); "converged": converged_readout),
# clamp (a quarter of the given x, y on the kernel's clamp values), units (all AOIs; every other one is off-target, the
# last one on-target: ``interleaved``)
CASES = {
    # two workgroups, the second with 44 live lanes: 14 of an off-target AOI, then the 30 of the last, on-target one
    "partial_workgroup": dict(dkw=dict(N=10, F=30), K=2, S=6, units=300),
    "full_workgroup": dict(dkw=dict(N=8, F=32), K=2, S=6, units=256),       # exactly one full workgroup
    "K4": dict(dkw=dict(N=2, F=2), K=4, S=6, units=4),                      # the 16-combination loop (TQ_MAXK)
    "K3": dict(dkw=dict(N=2, F=2, P=9), K=3, S=6, units=4),
    "K1": dict(dkw=dict(N=2, F=4), K=1, S=6, units=8),                      # the ln_c = 0 branch
    # c = u % C, n = u / (F C) across a workgroup boundary (the last AOI, on-target, holds units 240 .. 299)
    "two_channels": dict(dkw=dict(N=5, F=30, C=2), K=2, S=6, units=300),
    "one_particle": dict(dkw=dict(N=10, F=30), K=2, S=1, units=300),
    "crosstalk": dict(dkw=dict(N=4, F=5, C=2), K=2, S=5, units=40, crosstalk=True),
    "crosstalk_two_workgroups": dict(dkw=dict(N=10, F=15, C=2), K=2, S=5, units=300, crosstalk=True),
    "converged_partial_workgroup": dict(dkw=dict(N=10, F=30), K=2, S=6, units=300, regime="converged"),
    "converged_K4": dict(dkw=dict(N=2, F=2), K=4, S=6, units=4, regime="converged"),
    "clamp_values": dict(dkw=dict(N=10, F=30), K=2, S=6, units=300, clamp=True),
}
GIVEN_CASES = list(CASES)
DRAWN_CASES = ["partial_workgroup", "K4", "crosstalk"]  # draw = 1 at DRAWN_S particles
DRAWN_S, LAW_S = 8, 2000
LAW_DKW = dict(N=4, F=6)  # 24 units


def interleaved(d):
    """``d`` with on- and off-target AOIs in turn, the last AOI on-target (the simulated sets put the on-target AOIs first:
    the second workgroup of a 300-unit case would then hold off-target units alone, which are written as zeros)."""
    N = d.images.shape[0]
    on = torch.arange(N) % 2 == (N - 1) % 2
    return CosmosDataset(d.images, d.xy, on, offset_samples=d.offset.samples, offset_weights=d.offset.weights)


# ---- parameters ---------------------------------------------------------------------------------------------------------------
# targets of the converged regime; assert_converged_readout holds the built parameters to them
LOGIT_MAX, SIZE_MAX, MEAN_EDGE, PI1_MIN, LAMDA_MIN = 8.0, 1e3, 0.99, 1e-4, 1e-2


def converged_readout(o, seed=5):
    """The rows the read-out reads, spread as a converged fit spreads them.  site_fixture.converged_parameters gives m_probs
    logits uniform in [-8, 8] and sizes log-uniform to 3000, but means only to 0.97 of the support and no globals; here the
    means go uniform in logit [-6, 6] (sigmoid 0.0025 .. 0.9975: 0.5 % from +-H), the extremes are written into the first two
    units of the first on-target AOI so that a case of four units has them too, and the globals get
    pi[1] = 1e-4 (size 1e5: concentration 10 on the small side), lamda = 1e-2 (beta 1e3) and a proximity of 0.3."""
    converged_parameters(o, seed=seed)
    g = torch.Generator().manual_seed(seed + 1)
    p = o.params
    for n in ("x_mean", "y_mean"):
        p[n].data = f32(-6.0 + 12.0 * torch.rand(p[n].shape, generator=g, dtype=torch.float64))
    K = o.K
    flat = lambda n: p[n].data.reshape(K, -1)
    big = float(f32(math.log(1.001 * SIZE_MAX - 2.0)))
    u0 = int(torch.nonzero(o.data.is_ontarget)[0]) * o.data.F * o.data.C
    u1 = u0 + 1
    # unit u0: a confident spot at one corner of the support in slot 0 and an excluded one at the opposite corner in slot K - 1
    flat("m_probs")[0, u0], flat("size")[0, u0], flat("x_mean")[0, u0], flat("y_mean")[0, u0] = LOGIT_MAX, big, 6.0, -6.0
    flat("m_probs")[K - 1, u0], flat("x_mean")[K - 1, u0], flat("y_mean")[K - 1, u0] = -LOGIT_MAX, -6.0, 6.0
    # unit u1: a confident, sharply placed spot at the target in slot 0 (the read-out is of order 1 there whatever pi is)
    flat("m_probs")[0, u1], flat("size")[0, u1], flat("x_mean")[0, u1], flat("y_mean")[0, u1] = LOGIT_MAX, big, 0.0, 0.0
    Q = o.Q
    p["pi_mean"].data = f32(torch.tensor([[0.0, math.log(PI1_MIN / (1.0 - PI1_MIN))]] * Q))
    p["pi_size"].data = f32(torch.full((Q, 1), math.log(1e5)))
    p["lamda_loc"].data = f32(torch.full((Q,), math.log(LAMDA_MIN)))
    p["lamda_beta"].data = f32(torch.full((Q,), math.log(1e3)))
    Hs = (o.data.P + 1) / math.sqrt(12.0)
    t = 0.3 / (Hs - o.eps)
    p["proximity_loc"].data = f32(torch.tensor(math.log(t) - math.log1p(-t)))
    return o


def assert_converged_readout(o, lats, ref):
    """The spread that was built, on the on-target units (a silently mild input fails here), and a reference that is neither
    all zero nor all one under it."""
    on = o.data.is_ontarget
    with torch.no_grad():
        cp = o.constrained(o.params)
    u = o.params["m_probs"].detach()[:, on]
    assert float(u.max()) >= LOGIT_MAX and float(u.min()) <= -LOGIT_MAX, (float(u.min()), float(u.max()))
    assert float(cp["size"][:, on].max()) >= SIZE_MAX, float(cp["size"][:, on].max())
    for n in ("x_mean", "y_mean"):
        m = cp[n][:, on] / o.H
        assert float(m.max()) >= MEAN_EDGE and float(m.min()) <= -MEAN_EDGE, (n, float(m.min()), float(m.max()))
    pi1 = cp["pi_mean"][:, 1]
    assert float(pi1.max()) <= 1.001 * PI1_MIN and float(cp["lamda_loc"].max()) <= 1.001 * LAMDA_MIN
    drawn_pi = torch.stack([lat["pi"][..., 1] for lat in lats])
    drawn_lam = torch.stack([lat["lamda"] for lat in lats])
    assert float(drawn_pi.min()) <= 1.5 * PI1_MIN and float(drawn_lam.min()) <= 1.5 * LAMDA_MIN, (
        float(drawn_pi.min()), float(drawn_lam.min()))
    z1 = ref["z"][on][..., 1]
    assert float(z1.max()) >= 0.1 and float(z1.min()) <= 1e-3 and ref["n_rel"] >= 2, (float(z1.min()), float(z1.max()), ref["n_rel"])


# ---- particles ----------------------------------------------------------------------------------------------------------------
def xy_clamp_values(o):
    """The kernel's clamp of an x / y draw, fl32(-H + 2 H eps) and fl32(H - 2 H eps) (tq_probs_draw_coord)."""
    return clamp_values(-o.H, o.H, o.eps)


def particles(o, S, seed=0, on_clamp=False):
    """``S`` joint guide draws of the oracle, every value rounded through float32 and x, y clamped as the kernel clamps its
    own draws; ``on_clamp``: every fourth x and y is put exactly on a clamp value, the lower and the upper in turn."""
    nd, fd = torch.arange(o.data.Nt), torch.arange(o.data.F)
    lo, hi = xy_clamp_values(o)
    torch.manual_seed(seed)
    lats = []
    with torch.no_grad():
        for s in range(S):
            lat = {k: v.float().double() for k, v in o.sample_guide(o.params, nd, fd).items()}
            lat["pi"] = torch.stack([1 - lat["pi"][..., 1], lat["pi"][..., 1]], -1)
            for j, n in enumerate(("x", "y")):
                v = lat[n].clamp(lo, hi)
                if on_clamp:
                    i = torch.arange(v.numel()).reshape(v.shape) + s + j
                    v = torch.where(i % 4 == 0, torch.where((i // 4) % 2 == 0, torch.full_like(v, lo), torch.full_like(v, hi)), v)
                lat[n] = v
            lats.append(lat)
    return nd, fd, lats


def given_inputs(o, eng, lats, nd, fd):
    """gbase_p [S][sizeof(TqGlobalBase) / 8] doubles and xy_given [S][2K][U] floats of tq_cosmos_probs(draw = 0).
    TqGlobalBase { double gain_g; double prox_t; double lamda_g[4]; double pi_x[4][2]; (alpha_x) }."""
    S, K, Q = len(lats), o.K, o.Q
    U = o.data.Nt * o.data.F * o.data.C
    with torch.no_grad():
        dists = o._guide_dists(o.constrained(o.params), nd, fd)
        gb = torch.zeros(S, eng.struct_sizes()[1] // 8, dtype=torch.float64)
        xy = torch.zeros(S, 2 * K, U, dtype=torch.float32)
        for s, lat in enumerate(lats):
            base = type(o).base_draws(lat, dists)
            gb[s, 0] = 1.0
            gb[s, 1] = base["proximity_t"]
            gb[s, 2:2 + Q] = base["lamda_g"]
            gb[s, 6:6 + 2 * Q] = base["pi_x"].reshape(-1)
            xy[s, :K] = lat["x"].reshape(K, U).float()
            xy[s, K:] = lat["y"].reshape(K, U).float()
    return gb.reshape(-1).to(eng.device), xy.reshape(-1).to(eng.device)


# ---- the reference and its allowance ------------------------------------------------------------------------------------------
def oracle32(o):
    """The same oracle in plain float32 (to be used inside working_dtype(torch.float32))."""
    d = o.data
    od = OracleData(d.images, d.xy, d.is_ontarget, d.offset_samples, d.offset_weights, mask=d.mask)
    t = type(o)(od, K=o.K, priors=o.priors, eps=o.eps)
    t.params = {n: u.detach().float() for n, u in o.params.items()}
    return t


def reference(o, nd, fd, lats):
    """{z, t: the float64 oracle on ``lats``; abs, rel: the allowances; e_abs, e_rel: the float32 oracle's own error}.
    Finite everywhere, off-target rows included."""
    z64, t64 = o.compute_probs(nd, fd, lats)
    assert bool(torch.isfinite(z64).all()) and bool(torch.isfinite(t64).all()), "the float64 reference is not finite"
    with working_dtype(torch.float32):
        z32, t32 = oracle32(o).compute_probs(nd, fd, [{k: v.float() for k, v in lat.items()} for lat in lats])
    assert z32.dtype == torch.float32 and t32.dtype == torch.float32
    on = o.data.is_ontarget
    dz, dt = (z32.double() - z64).abs()[on], (t32.double() - t64).abs()[:, on]
    e_abs = max(float(dz.max()), float(dt.max()))
    rz, rt = z64[on][..., 1], t64[:, on]
    rel = torch.cat([(dz[..., 1] / rz)[rz >= REL_FROM], (dt / rt)[rt >= REL_FROM]])
    e_rel = float(rel.max()) if rel.numel() else 0.0
    return {"z": z64, "t": t64, "e_abs": e_abs, "e_rel": e_rel, "n_rel": int(rel.numel()),
            "abs": min(ABS_CEIL, max(FACTOR * e_abs, ABS_FLOOR)), "rel": min(REL_CEIL, max(FACTOR * e_rel, REL_FLOOR))}


def unit_errors(z, t, ref, on):
    """Per on-target unit (n, f, c): the worst absolute error of its entries (both columns of z, every theta) and the worst
    relative error of its entries of z[..., 1] and theta with reference >= 1e-6."""
    ez, et = (z - ref["z"]).abs()[on], (t - ref["t"]).abs()[:, on]
    e_abs = torch.maximum(ez.amax(-1), et.amax(0))
    rz, rt = ref["z"][on][..., 1], ref["t"][:, on]
    zero = torch.zeros_like(rz)
    e_rel = torch.maximum(torch.where(rz >= REL_FROM, ez[..., 1] / rz, zero),
                          torch.where(rt >= REL_FROM, et / rt, torch.zeros_like(rt)).amax(0))
    return e_abs, e_rel


WORST = {}  # (check, case, backend) -> line of the report


def record(check, case, backend, e_abs, e_rel, ref, extra=""):
    WORST[(check, case, backend.name)] = (
        "posterior %s [%s, %s]: worst error / allowance  absolute %.3g (%.3g / %.3g)  relative %.3g (%.3g / %.3g)%s" % (
            check, case, backend.name, e_abs / ref["abs"], e_abs, ref["abs"], e_rel / ref["rel"], e_rel, ref["rel"], extra))


def check_outputs(z, t, ref, o, check, case, backend, flip_share=0.0):
    """The outputs of one call against ``ref``: off-target rows exactly 0, z0 + z1 = 1 to one ulp, and every on-target unit
    within both rules -- but for a share ``flip_share`` of them (draw = 1 on the device).  Returns (worst absolute, worst
    relative error over the units inside the allowance, share outside)."""
    on = o.data.is_ontarget
    z, t = z.detach().cpu().double(), t.detach().cpu().double()
    assert bool(torch.isfinite(z).all()) and bool(torch.isfinite(t).all()), (case, backend.name, "non-finite output")
    assert float(z[~on].abs().max()) == 0.0 and float(t[:, ~on].abs().max()) == 0.0, (case, "off-target rows")  # cosmos.py:615-623
    assert float((z[on].sum(-1) - 1.0).abs().max()) <= EPS32, (case, float((z[on].sum(-1) - 1.0).abs().max()))
    a_abs, a_rel = ref["abs"], ref["rel"]
    e_abs, e_rel = unit_errors(z, t, ref, on)
    out = (e_abs > a_abs) | (e_rel > a_rel)
    share = float(out.double().mean())
    inside = ~out if flip_share > 0 else torch.ones_like(out)
    w_abs, w_rel = (float(e_abs[inside].max()), float(e_rel[inside].max())) if bool(inside.any()) else (math.inf, math.inf)
    record(check, case, backend, w_abs, w_rel, ref, "  units outside %.2f %%" % (100 * share) if flip_share > 0 else "")
    assert share <= flip_share, "%s %s on %s: %d of %d on-target units outside the allowance (abs %.3g, rel %.3g): worst " \
        "absolute %.3g relative %.3g" % (check, case, backend.name, int(out.sum()), out.numel(), a_abs, a_rel,
                                        float(e_abs.max()), float(e_rel.max()))
    return w_abs, w_rel, share


# ---- cases, built once --------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case(name):
    """(dataset, oracle, AOI indices, frame indices, particles, reference) of a given-draw case: built once, shared by the
    host and the device tests, never written to."""
    c = CASES[name]
    K, xt = c["K"], c.get("crosstalk", False)
    d = interleaved(make_dataset(K=K, **c["dkw"]))
    o = make_oracle(d, K, perturb=0.4, crosstalk=xt)
    if c.get("regime") == "converged":
        converged_readout(o)
    assert d.images.shape[0] * d.images.shape[1] * d.images.shape[2] == c["units"]
    nd, fd, lats = particles(o, c["S"], on_clamp=c.get("clamp", False))
    if c.get("clamp"):
        lo, hi = xy_clamp_values(o)
        v = torch.stack([torch.stack([lat["x"], lat["y"]]) for lat in lats])
        assert abs(float(((v == lo) | (v == hi)).double().mean()) - 0.25) < 0.01 and bool((v == lo).any()) and bool((v == hi).any())
    ref = reference(o, nd, fd, lats)
    if c.get("regime") == "converged":
        assert_converged_readout(o, lats, ref)
    return d, o, nd, fd, lats, ref


def engine_for(backend, d, o, **kw):
    eng = backend.engine(d, o.K, crosstalk=type(o).__name__ == "CrosstalkOracle", **kw)
    oracle_to_engine(o, eng)
    return eng


def run_given(backend, name):
    """draw = 0 on the case's particles through ``backend``, every on-target unit against the oracle."""
    d, o, nd, fd, lats, ref = case(name)
    eng = engine_for(backend, d, o)
    gb, xy = given_inputs(o, eng, lats, nd, fd)
    a, ws = probs_args(eng, len(lats), seed=1, draw=False, gbase_p=gb, xy_given=xy)
    run_probs(eng, a)
    backend.sync()
    return check_outputs(ws["z_probs"], ws["theta_probs"], ref, o, "given draws", name, backend)


# ---- the draws of the build ---------------------------------------------------------------------------------------------------
def replay_xy(eng_host, S, seed):
    """[S][2K][U] float32: the x / y draws of tq_body_probs_unit(draw = 1) of the host build, for every unit."""
    a, _ = probs_args(eng_host, S, seed=seed)
    U = eng_host.Nt * eng_host.F * eng_host.C
    out = torch.zeros(S, 2 * eng_host.K, U, dtype=torch.float32)
    load_hostcheck().hc_probs_xy_draws(C.byref(a), C.c_void_p(out.data_ptr()))
    return out


def run_drawn(backend, eng, S, seed):
    """draw = 1: (z_probs, theta_probs, gbase_p [S][.]) as ``backend`` wrote them, on the host."""
    a, ws = probs_args(eng, S, seed=seed)
    run_probs(eng, a)
    backend.sync()
    return ws["z_probs"].cpu().clone(), ws["theta_probs"].cpu().clone(), ws["gbase_p"].cpu().clone().reshape(S, -1)


def latents_of_draws(o, nd, fd, xy, gbase):
    """The oracle's latents behind base draws ``gbase`` [S][.] and x / y draws ``xy`` [S][2K][U]: the globals as
    latents_from_base derives them (lamda = g / beta, pi = x, proximity = the clamped affine map of t), lamda and pi rounded
    to float32 as TqGlobals holds them."""
    K, Q, d = o.K, o.Q, o.data
    with torch.no_grad():
        dists = o._guide_dists(o.constrained(o.params), nd, fd)
    lats = []
    for s in range(xy.shape[0]):
        v = xy[s].double().reshape(2, K, d.Nt, d.F, d.C)
        pi1 = f32(gbase[s, 6:6 + 2 * Q].reshape(Q, 2)[:, 1])
        lats.append({"x": v[0], "y": v[1], "pi": torch.stack([1 - pi1, pi1], -1),
                     "lamda": f32(gbase[s, 2:2 + Q] / dists["lamda"].rate),
                     "proximity": dists["proximity"].from_base(gbase[s, 1])})
    return lats


@functools.lru_cache(maxsize=None)
def drawn_case(name, seed=3):
    """(dataset, oracle, indices, replayed x / y draws [DRAWN_S][2K][U]) of a draw = 1 case."""
    c = CASES[name]
    d, o, nd, fd, _, _ = case(name)
    xy = replay_xy(engine_for(HOST, d, o), DRAWN_S, seed)
    return d, o, nd, fd, xy


def run_what_the_draws_give(backend, name, seed=3, flip_share=0.0):
    """draw = 1 through ``backend``; the oracle on the replayed x / y and the global base draws the backend wrote."""
    d, o, nd, fd, xy = drawn_case(name, seed)
    eng = engine_for(backend, d, o)
    z, t, gbase = run_drawn(backend, eng, DRAWN_S, seed)
    ref = reference(o, nd, fd, latents_of_draws(o, nd, fd, xy, gbase))
    return check_outputs(z, t, ref, o, "own draws", name, backend, flip_share), ref, (z, t)


# ---- laws ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def law_case():
    d = interleaved(make_dataset(K=2, **LAW_DKW))
    return d, make_oracle(d, 2, perturb=0.4)


def xy_pit(o, xy):
    """The replayed draws through their own guide's cdf (scipy, float64 concentrations from the oracle), [S][2K][U]."""
    from scipy import stats

    K, H = o.K, o.H
    with torch.no_grad():
        cp = o.constrained(o.params)
    size = cp["size"].reshape(K, -1)
    mean = torch.cat([cp["x_mean"].reshape(K, -1), cp["y_mean"].reshape(K, -1)])
    c1 = torch.cat([size, size]) * (mean + H) / (2 * H)
    c0 = torch.cat([size, size]) - c1
    return stats.beta.cdf((xy.double().numpy() + H) / (2 * H), c1.numpy()[None], c0.numpy()[None])


def global_laws(o, gbase):
    """{site: KS p-value} of the global base draws [S][.] against the guide's law from the oracle's constrained parameters."""
    from scipy import stats

    Q = o.Q
    with torch.no_grad():
        dists = o._guide_dists(o.constrained(o.params), torch.arange(1), torch.arange(1))
    g = gbase.numpy()
    prox = dists["proximity"]
    out = {"proximity": stats.kstest(g[:, 1], stats.beta(float(prox.c1), float(prox.c0)).cdf).pvalue}
    for q in range(Q):
        out["lamda[%d]" % q] = stats.kstest(g[:, 2 + q], stats.gamma(float(dists["lamda"].concentration[q])).cdf).pvalue
        c = dists["pi"].concentration[q]
        out["pi[%d]" % q] = stats.kstest(g[:, 6 + 2 * q + 1], stats.beta(float(c[1]), float(c[0])).cdf).pvalue
        assert np.allclose(g[:, 6 + 2 * q] + g[:, 6 + 2 * q + 1], 1.0, atol=1e-15)
    return out


def run_global_law(backend, seed=3):
    """draw = 1 at LAW_S particles on 24 units: the law of every global site and pairwise distinct particles.  Returns gbase_p."""
    d, o = law_case()
    _, _, gbase = run_drawn(backend, engine_for(backend, d, o), LAW_S, seed)
    p = global_laws(o, gbase)
    WORST[("global draws", "law", backend.name)] = "posterior global draws [%s]: KS p-values %s" % (
        backend.name, "  ".join("%s %.3g" % kv for kv in p.items()))
    assert min(p.values()) > KS_LEVEL, p
    used = gbase[:, [1, 2, 7]].numpy()  # proximity, lamda[0], pi[0][1]: no two particles share all of them, nor one of the
    # double-valued ones (lamda's base draw is a float32 Gamma(50) variate: a few of 2000 coincide by chance)
    assert len(np.unique(used, axis=0)) == LAW_S and all(len(np.unique(used[:, j])) == LAW_S for j in (0, 2))
    assert len(np.unique(used[:, 1])) > 0.99 * LAW_S
    return gbase


def shard_of(d, lo):
    """AOIs ``lo``.. of ``d`` as a data set of their own."""
    return CosmosDataset(d.images[lo:], d.xy[lo:], d.is_ontarget[lo:], offset_samples=d.offset.samples,
                         offset_weights=d.offset.weights)
