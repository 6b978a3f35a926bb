"""
The local guide sites in the regime of a converged fit: parameters, draws, a plain float64 reference of the stored site
terms (tq_site_store), torch's regime rule restated, and the per-element allowance.  Plain Python on the CPU; the host
build and the device are compared with it in test_site_regimes_host.py and test_gpu_site_regimes.py.

Stored rows of one site row (tq_site.h, TQ_NSITE_STORED):
  Gamma(alpha = loc beta, beta), draw v:         0 log q   1 d lq/d alpha   2 d v/d alpha
  AffineBeta(mean, size, lo, hi), draw y, t = (y - lo) / sc:
                                                 0 log q   1 d lq/d c1      2 d y/d c1      3 d lq/d c0   4 d y/d c0
Site order: background, height[k], width[k], x[k], y[k]; a site row holds the B units of the batch.
"""

import math

import numpy as np
import torch

EPS32 = float(torch.finfo(torch.float32).eps)
WG, WAVE = 256, 64  # TQ_BC_NT draws of one site per workgroup, 64 lanes per wave
CLASSES = ("pair", "x-small", "(1-x)-small", "saddle-1", "rational")  # the task classes of tq_site_beta_compact, 0..4
ROWS = ("log q", "d lq/d c1", "d y/d c1", "d lq/d c0", "d y/d c0")


def f32(x):
    """Rounded through float32, held in float64."""
    return torch.as_tensor(x, dtype=torch.float64).float().double()


def ulp32(x):
    """Spacing of float32 at ``x`` (float64 tensor)."""
    return torch.from_numpy(np.spacing(np.abs(x.numpy()).astype(np.float32)).astype(np.float64)).reshape(x.shape)


# ---- parameters and draws ---------------------------------------------------------------------------------------------------
def converged_parameters(o, seed=5):
    """Overwrites unconstrained leaves of the oracle with the spread of a converged fit, every value rounded through float32:
    size and w_size = 2 + s, s + 2 log-uniform in [3, 3000]; x_mean, y_mean, w_mean uniform in [-3.5, 3.5] (sigmoid 0.03 ..
    0.97 of the support); m_probs uniform in [-8, 8]; h_beta log-uniform in [1e-4, 1] (height concentrations 0.1 .. 3000)."""
    g = torch.Generator().manual_seed(seed)
    uni = lambda shape, a, b: a + (b - a) * torch.rand(shape, generator=g, dtype=torch.float64)
    p = o.params
    for n in ("size", "w_size"):
        s = torch.exp(uni(p[n].shape, math.log(3.0), math.log(3000.0)))
        p[n].data = f32(torch.log(s - 2.0))
    for n in ("x_mean", "y_mean", "w_mean"):
        p[n].data = f32(uni(p[n].shape, -3.5, 3.5))
    p["m_probs"].data = f32(uni(p["m_probs"].shape, -8.0, 8.0))
    p["h_beta"].data = f32(uni(p["h_beta"].shape, math.log(1e-4), 0.0))
    return o


def bounds(o):
    """{site kind: (lo, hi)} of the AffineBeta sites."""
    return {"width": (o.priors["width_min"], o.priors["width_max"]), "x": (-o.H, o.H), "y": (-o.H, o.H)}


def interior(lat32, o, margin=1e-4):
    """Moves the width, x and y draws into [lo + margin sc, hi - margin sc] (float32 values); the caller recovers the base
    draws again.  A draw the float64 oracle clamps with its own eps can sit ON the bound after rounding to float32 (log q
    = +inf in the kernel), or exactly on the float32 clamp value, where the kernel passes no pathwise gradient and the
    float64 oracle does: neither can be compared."""
    for name, (lo, hi) in bounds(o).items():
        sc = hi - lo
        lat32[name] = f32(lat32[name].clamp(lo + margin * sc, hi - margin * sc))
    return lat32


def kernel_clamped(y32, lo, hi, eps=EPS32):
    """The kernel's decision (tq_site_beta_compact, tq_affine_beta_site_terms), restated in float32:
    y <= fl32(lo + eps sc) or y >= fl32(hi - eps sc).  (eps sc is exact in float32 for every support here, so a fused
    multiply-add gives the same bound.)"""
    y = torch.as_tensor(y32).float()
    lo_, hi_, e = torch.tensor(lo, dtype=torch.float32), torch.tensor(hi, dtype=torch.float32), torch.tensor(eps, dtype=torch.float32)
    sc = hi_ - lo_
    return (y <= lo_ + e * sc) | (y >= hi_ - e * sc)


def clamp_values(lo, hi, eps=EPS32):
    """(fl32(lo + eps sc), fl32(hi - eps sc)) as python floats."""
    lo_, hi_, e = torch.tensor(lo, dtype=torch.float32), torch.tensor(hi, dtype=torch.float32), torch.tensor(eps, dtype=torch.float32)
    sc = hi_ - lo_
    return float(lo_ + e * sc), float(hi_ - e * sc)


# ---- the inputs of the site terms -------------------------------------------------------------------------------------------
def site_inputs(o, nd, fd, lat32, params=None):
    """Per site row (site order above) the inputs of the reference, as float64 tensors of shape (1 + 4K, B):
    Gamma rows: a = v, b = alpha = fl32(loc) fl32(beta), c = fl32(beta); AffineBeta rows: a = t, b = c1, c = c0 from the
    constrained parameters rounded to float32 and the float32 draws; ``sc`` (0 for Gamma rows), ``clamped``, and ``da``,
    ``db``, ``dc``: how far the kernel's own float32 value of each input may lie from this one (see site_budget)."""
    K = o.K
    P = o.params if params is None else params
    with torch.no_grad():
        cp = o.constrained(P)
    n_, f_ = nd[:, None], fd[None, :]
    per_k = lambda src, name: src[name].detach()[:, n_, f_, :].reshape(K, -1)
    con = lambda name: f32(per_k(cp, name))
    B = len(nd) * len(fd) * o.Q
    S = 1 + 4 * K
    a, b, c, db, dc = (torch.zeros(S, B, dtype=torch.float64) for _ in range(5))
    sc_row = torch.zeros(S, dtype=torch.float64)
    clamped = torch.zeros(S, B, dtype=torch.bool)
    half = 0.5 * EPS32

    def gamma(rows, v, loc, beta, ul, ub):
        a[rows], b[rows], c[rows] = v, loc * beta, beta
        db[rows] = ULPS * ulp32(loc * beta) + loc * beta * (ul.abs() + ub.abs()) * half
        dc[rows] = beta * (EPS32 + ub.abs() * half)

    flat = lambda src, name: src[name].detach()[n_, f_, :].reshape(-1)
    gamma(0, lat32["background"].reshape(-1), f32(flat(cp, "b_loc")), f32(flat(cp, "b_beta")), flat(P, "b_loc"), flat(P, "b_beta"))
    gamma(slice(1, 1 + K), lat32["height"].reshape(K, -1), con("h_loc"), con("h_beta"), per_k(P, "h_loc"), per_k(P, "h_beta"))
    bd = bounds(o)
    for j, (name, mean_n, size_n) in enumerate((("width", "w_mean", "w_size"), ("x", "x_mean", "size"), ("y", "y_mean", "size"))):
        lo, hi = bd[name]
        sc = hi - lo
        rows = slice(1 + (1 + j) * K, 1 + (2 + j) * K)
        y, mean, size, us = lat32[name].reshape(K, -1), con(mean_n), con(size_n), per_k(P, size_n)
        a[rows], b[rows], c[rows] = (y - lo) / sc, size * (mean - lo) / sc, size * (hi - mean) / sc
        d_mean = (size / sc) * MEAN_ULPS * float(np.spacing(np.float32(max(abs(lo), abs(hi)))))
        db[rows] = ULPS * ulp32(b[rows]) + b[rows] * us.abs() * half + d_mean
        dc[rows] = ULPS * ulp32(c[rows]) + c[rows] * us.abs() * half + d_mean
        sc_row[rows] = sc
        clamped[rows] = kernel_clamped(y, lo, hi, o.eps)
    return {"a": a, "b": b, "c": c, "da": ULPS * ulp32(a), "db": db, "dc": dc, "sc": sc_row, "clamped": clamped, "K": K}


# ---- the reference ----------------------------------------------------------------------------------------------------------
def gamma_rows(v, alpha, beta):
    """(3, n): log q, d lq/d alpha (autograd of torch.distributions.Gamma), d v/d alpha = _standard_gamma_grad(alpha, v beta) / beta."""
    al = alpha.clone().requires_grad_(True)
    lq = torch.distributions.Gamma(al, beta).log_prob(v)
    (d_al,) = torch.autograd.grad(lq.sum(), al)
    dv = torch._standard_gamma_grad(alpha, v * beta) / beta
    return torch.stack([lq.detach(), d_al, dv])


def beta_rows(t, c1, c0, sc, clamped):
    """(5, n): log q - ln sc, d lq/d c1, sc _dirichlet_grad(t, c1, size) (1 - t), d lq/d c0, -sc _dirichlet_grad(1 - t, c0, size) t
    with size = c1 + c0; both implicit gradients exactly 0 where ``clamped``."""
    a1, a0 = c1.clone().requires_grad_(True), c0.clone().requires_grad_(True)
    lq = torch.distributions.Beta(a1, a0).log_prob(t)
    d1, d0 = torch.autograd.grad(lq.sum(), (a1, a0))
    total = c1 + c0
    zero = torch.zeros_like(t)
    g1 = torch.where(clamped, zero, sc * torch._dirichlet_grad(t, c1, total) * (1.0 - t))
    g0 = torch.where(clamped, zero, -sc * torch._dirichlet_grad(1.0 - t, c0, total) * t)
    return torch.stack([lq.detach() - math.log(sc), d1, g1, d0, g0])


def site_reference(inp):
    """The five stored rows of every site and unit, (5, 1 + 4K, B) float64, from ``site_inputs`` (rows 3 and 4 of the Gamma
    sites, which the kernels do not write, are 0)."""
    K = inp["K"]
    S, B = inp["a"].shape
    out = torch.zeros(5, S, B, dtype=torch.float64)
    for s in range(S):
        if s <= K:
            out[:3, s] = gamma_rows(inp["a"][s], inp["b"][s], inp["c"][s])
        else:
            out[:, s] = beta_rows(inp["a"][s], inp["b"][s], inp["c"][s], float(inp["sc"][s]), inp["clamped"][s])
    return out


# ---- torch's regime rule, restated ------------------------------------------------------------------------------------------
def grad_regime(x, alpha, total):
    """The branch of torch._dirichlet_grad (aten/src/ATen/native/Distributions.h, _dirichlet_grad_one) for one direction:
    0 x-small series, 1 (1-x)-small series, 2 saddle point, 3 rational."""
    beta = total - alpha
    boundary = total * x * (1.0 - x)
    r = torch.full(x.shape, 3, dtype=torch.int64)
    r = torch.where((alpha > 6.0) & (beta > 6.0), torch.full_like(r, 2), r)
    r = torch.where((x >= 0.5) & (boundary < 0.75), torch.full_like(r, 1), r)
    r = torch.where((x <= 0.5) & (boundary < 2.5), torch.full_like(r, 0), r)
    return r


def regimes(t, c1, c0, size, clamped=None):
    """The tasks of tq_site_beta_compact per draw, (5, n) int64: 0 pair (both directions in the saddle-point regime with
    boundary >= 2.5, one task), 1 x-small series, 2 (1-x)-small series, 3 saddle point of one direction (one task, either
    or both), 4 rational; a clamped draw has none."""
    clamped = torch.zeros_like(t, dtype=torch.bool) if clamped is None else clamped
    pair = (size * t * (1.0 - t) >= 2.5) & (c1 > 6.0) & (size - c1 > 6.0) & ~clamped
    off = pair | clamped
    r0 = torch.where(off, torch.full(t.shape, -1, dtype=torch.int64), grad_regime(t, c1, size))
    r1 = torch.where(off, torch.full(t.shape, -1, dtype=torch.int64), grad_regime(1.0 - t, c0, size))
    cnt = lambda r: (r0 == r).long() + (r1 == r).long()
    return torch.stack([pair.long(), cnt(0), cnt(1), ((r0 == 2) | (r1 == 2)).long(), cnt(3)])


def waves(k):
    """``k`` = regimes(...) of one site row in launch order (256 consecutive units per workgroup, 64 per wave).  Returns one
    record per wave with a live lane: (workgroup, wave, live lanes, tasks per class (5,), mixed), mixed = the wave has a
    draw outside the pair class that is not clamped, and so goes through the queue."""
    n = k.shape[1]
    out = []
    for w0 in range(0, n, WAVE):
        kw = k[:, w0:w0 + WAVE]
        out.append((w0 // WG, (w0 % WG) // WAVE, kw.shape[1], kw.sum(1), bool(kw[1:].sum() > 0)))
    return out


def beta_site_regimes(inp):
    """{site row: regimes(...)} of the AffineBeta rows of ``site_inputs``."""
    K = inp["K"]
    return {s: regimes(inp["a"][s], inp["b"][s], inp["c"][s], inp["b"][s] + inp["c"][s], inp["clamped"][s])
            for s in range(1 + K, 1 + 4 * K)}


def regime_report(inp):
    """Per AffineBeta site row: tasks per class, and how many of its waves are mixed.  One line each."""
    lines = []
    for s, k in beta_site_regimes(inp).items():
        w = waves(k)
        lines.append("site %d: %s  clamped %d  mixed waves %d / %d" % (
            s, "  ".join("%s %d" % (n, int(v)) for n, v in zip(CLASSES, k.sum(1))), int(inp["clamped"][s].sum()),
            sum(1 for r in w if r[4]), len(w)))
    return lines


# ---- the allowance ----------------------------------------------------------------------------------------------------------
# |kernel - reference| <= 2 spread + tol floor, per element.
#   spread: the largest change of the reference when its inputs move inside the box the kernel's own float32 inputs lie in, in
#           every sign combination -- t, c1, c0 (Gamma: v, alpha, beta).  The factor 2 is margin for the second-order terms.
#           A perturbed t stays inside (0, 1).  The box (site_inputs: da, db, dc), ulp = float32 spacing at the value:
#             t, v        2 ulp: (y - lo) / sc is two roundings and one approximate reciprocal.
#             c1, c0      2 ulp for the same reason, and two terms that are rounding of the kernel's INPUTS, found on the host
#                         build with the reference evaluated at the build's own t, c1, c0 (hc_cosmos_site_inputs): there the
#                         excess vanished, the arithmetic was inside the floor.
#                           * the mean is formed as (lo + eps) + (sc - 2 eps) sigmoid(u), a sum of magnitude H = max(|lo|,
#                             |hi|): lo + eps rounds to lo (eps = ulp(H) / 4 at H = 7.5), the sum rounds (ulp(H) / 2), and the
#                             sigmoid through exp2 and a reciprocal carries (|u| / 2 + 2) eps (1 - sigmoid) relatively, at
#                             most 0.9e-6 = 1.9 ulp(H) on the mean at sc = 15: 3 ulp(H) absolutely.  mean - lo (or hi - mean)
#                             keeps that absolute error however small it is: size / sc * 3 ulp(H) on both concentrations,
#                             with opposite signs.  (c0 = 26.5 at size 673 was 68 ulp from the reference's; the host build
#                             reached 2.4 ulp(H).)
#                           * size = 2 + exp(u) through exp2(u log2 e): the product is rounded at its own magnitude, which
#                             puts |u| eps / 2 of relative error on exp(u).
#             alpha, beta the same exponentials: alpha = exp(u_loc) exp(u_beta) carries (|u_loc| + |u_beta|) eps / 2 next to
#                         its 2 ulp, beta |u_beta| eps / 2 and one ulp of the hardware exponential (the reference holds beta
#                         fixed otherwise: log q moves by (loc - v) d beta, some sqrt(alpha) relative changes of beta).
#   floor:  the tolerances of tests/test_math.py on the routines themselves: lgamma / digamma 6e-6 max(1, |ref|) (rows 0, 1, 3);
#           _dirichlet_grad 5e-5 |ref| plus the two float32 products of the stored term: 1e-4 |ref| (Beta rows 2, 4);
#           _standard_gamma_grad 2e-5 plus the reciprocal and product: 4e-5 |ref| (Gamma row 2).
TOL_LQ, TOL_BETA_GRAD, TOL_GAMMA_GRAD = 6e-6, 1e-4, 4e-5
ULPS, MEAN_ULPS = 2.0, 3.0
T_MIN, T_MAX = 2.0 ** -40, 1.0 - 2.0 ** -25


def site_budget(inp, ref, box=1.0):
    """The allowance of every element of ``ref`` = site_reference(inp), same shape (``box`` scales the box of the spread:
    0 leaves the floor alone)."""
    K = inp["K"]
    S, B = inp["a"].shape
    spread = torch.zeros_like(ref)
    signs = [(sa, sb, sc_) for sa in (-1.0, 1.0) for sb in (-1.0, 1.0) for sc_ in (-1.0, 1.0)] if box else []
    for s in range(S):
        a, b, c = inp["a"][s], inp["b"][s], inp["c"][s]
        da, db, dc = box * inp["da"][s], box * inp["db"][s], box * inp["dc"][s]
        for sa, sb, sc_ in signs:
            if s <= K:
                r = gamma_rows((a + sa * da).clamp(min=1e-45), b + sb * db, c + sc_ * dc)
                spread[:3, s] = torch.maximum(spread[:3, s], (r - ref[:3, s]).abs())
            else:
                r = beta_rows((a + sa * da).clamp(T_MIN, T_MAX), b + sb * db, c + sc_ * dc, float(inp["sc"][s]), inp["clamped"][s])
                spread[:, s] = torch.maximum(spread[:, s], (r - ref[:, s]).abs())
    floor = TOL_LQ * ref.abs().clamp(min=1.0)
    floor[2, :1 + K] = TOL_GAMMA_GRAD * ref[2, :1 + K].abs()
    floor[2, 1 + K:] = TOL_BETA_GRAD * ref[2, 1 + K:].abs()
    floor[4, 1 + K:] = TOL_BETA_GRAD * ref[4, 1 + K:].abs()
    floor[3:, :1 + K] = 0.0
    return 2.0 * spread + floor


WORST = {}  # where -> {row name: (worst error / allowance, site row, unit)}: printed by the test modules


def check_sites(got, inp, ref, allow, where, skip=None):
    """Every stored row of every site within its allowance (``got``: (5, 1 + 4K, B), the workspace ``site`` of an engine);
    records the worst error / allowance per row under ``where``.  ``skip``: (1 + 4K, B) mask of elements not compared."""
    K = inp["K"]
    got = got.detach().cpu().double().reshape(ref.shape)
    assert bool(torch.isfinite(got).all()), (where, "non-finite site term", torch.nonzero(~torch.isfinite(got))[:4].tolist())
    err = (got - ref).abs()
    live = torch.ones(ref.shape, dtype=torch.bool)
    live[3:, :1 + K] = False  # rows the Gamma sites do not have
    if skip is not None:
        live &= ~skip[None]
    ratio = torch.where(live, torch.where(err > 0, err / allow.clamp(min=1e-300), torch.zeros_like(err)), torch.zeros_like(err))
    rec = WORST.setdefault(where, {})
    for kind, rows in (("Gamma", slice(0, 1 + K)), ("Beta", slice(1 + K, None))):
        for r in range(3 if kind == "Gamma" else 5):
            sub = ratio[r, rows]
            at = int(sub.reshape(-1).argmax())
            rec["%s %s" % (kind, ROWS[r] if kind == "Beta" else ("log q", "d lq/d alpha", "d v/d alpha")[r])] = (
                float(sub.reshape(-1)[at]), at // sub.shape[1] + rows.start, at % sub.shape[1])
    bad = ratio > 1.0
    if bool(bad.any()):
        at = int(ratio.reshape(-1).argmax())
        r, s, i = np.unravel_index(at, tuple(ratio.shape))
        raise AssertionError("%s: stored row %d of site %d unit %d: got %.9g reference %.9g, error %.3g > allowance %.3g; inputs "
                             "a %.9g b %.9g c %.9g (%d elements over)" % (
                                 where, r, s, i, float(got[r, s, i]), float(ref[r, s, i]), float(err[r, s, i]),
                                 float(allow[r, s, i]), float(inp["a"][s, i]), float(inp["b"][s, i]), float(inp["c"][s, i]),
                                 int(bad.sum())))
    return rec


def report_lines(name):
    out = []
    for where, rec in WORST.items():
        out.append("site terms %s [%s]: worst error / allowance  %s" % (
            name, where, "  ".join("%s %.2f" % (k, v[0]) for k, v in rec.items())))
    return out


# ---- hand-placed workgroups -------------------------------------------------------------------------------------------------
# P = 15: H = 8, sc = 16, t = (y + 8) / 16 exact in float32.  One workgroup (256 units) per site; every lane gets (t, size,
# mean fraction m = (mean - lo) / sc) for its x and y sites alike.  Lane kinds, with the classes torch's rule gives them:
LANE = {
    "series": (0.5, 8.0, 0.5),      # boundary 2 < 2.5 at x = 1/2: both directions x-small -> two tasks of class 1
    "rational": (0.5, 11.0, 0.5),   # boundary 2.75, c1 = c0 = 5.5 <= 6: both directions rational -> two tasks of class 4
    "pair": (0.375, 200.0, 0.5),    # boundary 46.9, c1 = c0 = 100: the saddle-point pair, 0.125 from the mean (3.5 sd)
    "saddle_hi": (0.015, 100.0, 0.08),   # c1 = 8, c0 = 92, boundary 1.48: t x-small, 1 - t saddle point (code 2)
    "saddle_lo": (0.985, 100.0, 0.08),   # the mirror: t saddle point (code 1), 1 - t x-small
    "one_minus": (0.9375, 8.0, 0.5),     # boundary 0.47 < 0.75 at x >= 1/2: (1-x)-small, the other direction x-small
    "clamp_lo": (None, 40.0, 0.5),       # y = fl32(lo + eps sc)
    "clamp_hi": (None, 40.0, 0.3),       # y = fl32(hi - eps sc)
}
# expected tasks per class (pair, x-small, (1-x)-small, saddle-1, rational) of one lane of each kind
LANE_TASKS = {"series": (0, 2, 0, 0, 0), "rational": (0, 0, 0, 0, 2), "pair": (1, 0, 0, 0, 0), "saddle_hi": (0, 1, 0, 1, 0),
              "saddle_lo": (0, 1, 0, 1, 0), "one_minus": (0, 1, 1, 0, 0), "clamp_lo": (0, 0, 0, 0, 0), "clamp_hi": (0, 0, 0, 0, 0)}
ALL_FIVE = ("series", "rational", "pair", "saddle_hi", "saddle_lo", "one_minus")


def _lanes(f):
    return [f(i) for i in range(WG)]


HAND_PLACED = {
    # 512 tasks of class 1: R1 filled from the bottom, the `qc += 256` loop taken twice
    "all_series": _lanes(lambda i: "series"),
    # 512 tasks of class 4: R1 filled from the top
    "all_rational": _lanes(lambda i: "rational"),
    # 256 + 256: the two ends of R1 meet with no free slot
    "series_and_rational": _lanes(lambda i: "series" if i % 2 == 0 else "rational"),
    # waves 0, 1, 3 evaluate in place, wave 2 is mixed through one lane
    "one_lane_outside_the_pair": _lanes(lambda i: "rational" if i == 2 * WAVE + 37 else "pair"),
    # every wave mixed, one pair task in the queue
    "one_pair_lane": _lanes(lambda i: "pair" if i == WAVE + 5 else ALL_FIVE[i % 6 if i % 6 != 2 else 0]),
    # all five classes in every wave: wave0 advances through all five loops
    "all_five_classes": _lanes(lambda i: ALL_FIVE[(i + i // WAVE) % 6]),
    # draws on both float32 clamp values among lanes of the other classes
    "clamp_values": _lanes(lambda i: ("clamp_lo", "clamp_hi", ALL_FIVE[(i // 4) % 6], ALL_FIVE[(i // 4 + 3) % 6])[i % 4]),
}


def hand_placed(case, o, lat32):
    """Writes the lanes of HAND_PLACED[case] into the oracle's x_mean, y_mean and size and into the x and y draws of
    ``lat32`` (every k; N F C = 256 units, P = 15).  Returns the expected tasks per class of one site row, (5,)."""
    kinds = HAND_PLACED[case]
    assert o.H == 8.0 and lat32["x"][0].numel() == WG
    lo_v, hi_v = clamp_values(-8.0, 8.0, o.eps)
    t = [LANE[k][0] for k in kinds]
    y = torch.tensor([lo_v if k == "clamp_lo" else hi_v if k == "clamp_hi" else 16.0 * t_ - 8.0 for k, t_ in zip(kinds, t)],
                     dtype=torch.float64)
    size = torch.tensor([LANE[k][1] for k in kinds], dtype=torch.float64)
    m = torch.tensor([LANE[k][2] for k in kinds], dtype=torch.float64)
    shape = o.params["size"].shape  # (K, N, F, C)
    full = lambda v: f32(v).reshape(1, *shape[1:]).expand(shape).clone()
    o.params["size"].data = full(torch.log(size - 2.0))
    for n in ("x_mean", "y_mean"):
        o.params[n].data = full(torch.log(m) - torch.log1p(-m))
    for n in ("x", "y"):
        lat32[n] = f32(y).reshape(1, *lat32[n].shape[1:]).expand(lat32[n].shape).clone()
    return torch.tensor([LANE_TASKS[k] for k in kinds]).sum(0)
