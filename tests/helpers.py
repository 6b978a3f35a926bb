"""Shared test utilities: problem construction, oracle <-> engine plumbing, host-check loader."""

import ctypes as C
import math
import os
import subprocess

import pytest
import torch

from oracle.cosmos import CosmosOracle, OracleData
from oracle.crosstalk import CrosstalkOracle
from tapqir_amd import _lib
from tapqir_amd.models.engine import CosmosEngine as HipEngine
from tapqir_amd.utils.dataset import CosmosDataset
from tapqir_amd.utils.simulate import TEST_PARAMS, simulate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HC_DIR = os.path.join(ROOT, "tests", "hostcheck")
EPS32 = float(torch.finfo(torch.float32).eps)

_hc = None

# stages of a step whose latent draws are supplied by the test (make_args(draw_globals=False)):
# tables from the given global base draws, site terms of the given local draws, ELBO + gradients
GIVEN_STAGES = ("cosmos_sample_globals", "cosmos_sample_locals", "cosmos_elbo_grads", "cosmos_globals_grad")


def build_host_check(src, so_path):
    """g++ build of one tests/hostcheck source (the kernels' host+device headers on host memory) into ``so_path``."""
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-o", so_path, src])


def adam64(par0, loglik, n_steps, lr):
    """``n_steps`` of torch.optim.Adam (betas (0.9, 0.999), eps 1e-8) on ``-loglik(par).sum()`` from ``par0`` (float64):
    the optimiser of the reference's fits.  Returns the final parameters, detached."""
    par = par0.clone().requires_grad_(True)
    opt = torch.optim.Adam([par], lr=lr, betas=(0.9, 0.999), eps=1e-8)
    for _ in range(n_steps):
        opt.zero_grad()
        loss = -loglik(par).sum()
        loss.backward()
        opt.step()
    return par.detach()


def load_hostcheck():
    """g++ build of the kernels' inline math, driven on host memory (tests only)."""
    global _hc
    if _hc is not None:
        return _hc
    so = os.path.join(HC_DIR, "libtq_hostcheck.so")
    src = os.path.join(HC_DIR, "hostcheck.cpp")
    hdrs = [os.path.join(ROOT, "tapqir_amd", "csrc", f) for f in os.listdir(os.path.join(ROOT, "tapqir_amd", "csrc"))
            if f.endswith(".h")] + [os.path.join(ROOT, "include", "tapqir_hip.h"), src]
    if not os.path.exists(so) or any(os.path.getmtime(h) > os.path.getmtime(so) for h in hdrs):
        build_host_check(src, so)
    lib = C.CDLL(so)
    lib.hc_globals_size.restype = C.c_int64
    lib.hc_gbase_size.restype = C.c_int64
    lib.hc_ksmogn_log_prob.argtypes = [C.POINTER(_lib.KsmognArgs)]
    lib.hc_ksmogn_crosstalk_log_prob.argtypes = [C.POINTER(_lib.XtalkArgs)]
    lib.hc_image_stats.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32]
    lib.hc_image_stats.restype = None
    lib.hc_snr_chi2.argtypes = [C.POINTER(_lib.SnrArgs)]
    lib.hc_snr_chi2.restype = None
    lib.hc_ksmogn_rsample.argtypes = [C.POINTER(_lib.RsampleArgs)]
    lib.hc_ksmogn_rsample.restype = None
    lib.hc_cosmos_probs.argtypes = [C.POINTER(_lib.ProbsArgs)]
    lib.hc_cosmos_probs.restype = None
    lib.hc_probs_xy_draws.argtypes = [C.POINTER(_lib.ProbsArgs), C.c_void_p]
    lib.hc_probs_xy_draws.restype = None
    for n in ("hc_cosmos_sample_globals", "hc_cosmos_sample_locals", "hc_cosmos_elbo_grads",
              "hc_cosmos_globals_grad", "hc_cosmos_adam"):
        getattr(lib, n).argtypes = [C.POINTER(_lib.CosmosArgs)]
        getattr(lib, n).restype = None
    lib.hc_cosmos_adam_catchup.argtypes = [C.POINTER(_lib.CosmosArgs), C.c_int32]
    lib.hc_cosmos_adam_catchup.restype = None
    lib.hc_cosmos_tail_reduced.argtypes = [C.POINTER(_lib.CosmosArgs), C.POINTER(_lib.CosmosArgs)]
    lib.hc_cosmos_tail_reduced.restype = None
    _hc = lib
    return lib


class HostCheckEngine(HipEngine):
    """The engine's host logic (workspace, argument blocks, lazy-Adam clock, sharded step sequence) driving the g++ build
    of the kernels' inline math on host memory instead of libtapqir_hip.so.  Test-side only: it lets the CPU suite run the
    parity comparisons and the world-size-2 gloo test without a GPU.  The product class has no such path."""

    pipelined_tail = False     # the host build has the plain stage functions only
    split_sampling = False
    lazy_adam_default = False

    def _open_library(self):
        return load_hostcheck()

    def struct_sizes(self):
        return int(self.lib.hc_globals_size()), int(self.lib.hc_gbase_size())

    def _interleaved_images(self):
        return None  # the interleaved layout belongs to the GPU kernels

    def _image_stats(self, U):
        self.lib.hc_image_stats(_lib.ptr(self.images), _lib.ptr(self.offset_samples), _lib.ptr(self.pixstats),
                                C.c_int64(U), C.c_int32(self.P))

    def _stream(self):
        return None

    def _blk_floats(self, B):
        return ((B + 255) // 256) * self.n_gsum

    def call(self, name, args):
        getattr(self.lib, "hc_" + name)(C.byref(args))

    def _adam_catchup(self, a, all_units):
        self.lib.hc_cosmos_adam_catchup(C.byref(a), all_units)

    def _tail_reduced(self, a, next_args):
        self.lib.hc_cosmos_tail_reduced(C.byref(a), None if next_args is None else C.byref(next_args))

    def run_probs(self, a):
        self.lib.hc_cosmos_probs(C.byref(a))

    def _run_snr_chi2(self, a):
        self.lib.hc_snr_chi2(C.byref(a))


def CosmosEngine(data, lib=None, **kw):
    """Engine factory of the tests: the HIP engine, or (``lib`` = the loaded host build) its host-check subclass."""
    return HostCheckEngine(data, **kw) if lib is not None else HipEngine(data, **kw)


def make_dataset(N=4, F=6, C=1, P=14, K=2, seed=0, offsets="sim", mask=None):
    """Synthetic data with the reference test-suite parameters (test/test_tapqir.py:20-50)."""
    if C == 1:
        d = simulate(K, N, F, C, P, seed, TEST_PARAMS)
    else:  # independent channels: stack single-channel simulations
        parts = [simulate(K, N, F, 1, P, seed + c, TEST_PARAMS) for c in range(C)]
        d = CosmosDataset(torch.cat([p.images for p in parts], 2), torch.cat([p.xy for p in parts], 2),
                          parts[0].is_ontarget, offset_samples=parts[0].offset.samples,
                          offset_weights=parts[0].offset.weights)
    if offsets == "hist":  # a wide offset histogram like real data (glimpse_reader.py:414-421)
        s = torch.arange(70.0, 110.0)
        w = torch.exp(-0.5 * ((s - 90.0) / 6.0) ** 2)
        d = CosmosDataset(d.images, d.xy, d.is_ontarget, labels=d.labels, offset_samples=s,
                          offset_weights=(w / w.sum()).float())
    if offsets == "peaked":  # weights spanning > 2^40: the packed histogram kernel keeps log-weights inside the exponent
        s = torch.arange(70.0, 110.0)
        w = torch.exp(-0.5 * ((s - 90.0) / 2.0) ** 2).double()
        d = CosmosDataset(d.images, d.xy, d.is_ontarget, labels=d.labels, offset_samples=s, offset_weights=w / w.sum())
    if offsets == "wide":  # offsets reaching above the dimmest pixels: some offsets are masked per pixel (ksmogn.py:226)
        s = torch.arange(70.0, 330.0, 4.0)
        w = torch.exp(-0.5 * ((s - 90.0) / 60.0) ** 2)
        d = CosmosDataset(d.images, d.xy, d.is_ontarget, labels=d.labels, offset_samples=s,
                          offset_weights=(w / w.sum()).float())
    if offsets == "hist8":  # a histogram narrow enough for the dense oracle at the default 10 x 512 minibatch (5120 units)
        s = torch.arange(82.0, 98.0, 2.0)
        w = torch.exp(-0.5 * ((s - 90.0) / 4.0) ** 2)
        d = CosmosDataset(d.images, d.xy, d.is_ontarget, labels=d.labels, offset_samples=s,
                          offset_weights=(w / w.sum()).float())
    if isinstance(offsets, tuple):  # ("grid", O, lo, hi, sigma): a histogram of any length, see offset_grid
        s, w = offset_grid(*offsets[1:])
        d = CosmosDataset(d.images, d.xy, d.is_ontarget, labels=d.labels, offset_samples=s, offset_weights=w)
    if mask is not None:
        d.mask = mask
    return d


def offset_grid(O, lo=70.0, hi=110.0, sigma=6.0):
    """An offset histogram of exactly ``O`` DISTINCT samples torch.linspace(lo, hi, O) (fractional spacing, like a bin size
    below 1; merge_offsets keeps every one) with Gaussian weights of width ``sigma`` about 90, normalised, float64.
    The simulated pixels are >= 141 at the suite's shapes, so [70, 110] keeps every offset below every pixel (the unmasked branch of the packed
    kernel) at any length; hi = 330 reaches above the dimmest pixels (the masked branch, as "wide"); sigma = 2 spreads the
    weights over more than 2^40 (merge_offsets clamps them at 2^-52: the non-factored form of the packed kernel, as "peaked")."""
    s = torch.linspace(lo, hi, O, dtype=torch.float32)
    assert O == 1 or bool((s[1:] > s[:-1]).all()), "offset samples must stay distinct in float32"
    w = torch.exp(-0.5 * ((s.double() - 90.0) / sigma) ** 2)
    return s, w / w.sum()


def grid(O, lo=70.0, hi=110.0, sigma=6.0):
    """``offsets=`` of make_dataset for offset_grid(O, lo, hi, sigma)."""
    return ("grid", O, lo, hi, sigma)


# ---- the LDS a launch of the 16-lane tile routine asks for ------------------------------------------------------------------
# The request of tq_tile16_lds_floats (tapqir_amd/csrc/tq_ksmogn_dev.h), restated once: per unit slot the staged tile (npix
# floats rounded up to 16 mod 32) and the separable factors (2 K rows of TQ_MAX_P), then, for 1 < O <= TQ_OFFTAB_MAX (and at O = 1 in the histogram form), the
# offset table (4 extrema + 4 floats per offset).  16 slots for the 16-lane kernel and the single-launch minibatch step, 4 for
# the wave-per-unit kernel of gathered histogram batches.  The minibatch kernel adds its static LDS (9264 B in the code
# object: s_bias 8 KB, s_part, flags) and asks for at least TQ_SUBSAMPLE_LDS where it also draws the next subsample.
LDS_MAX_P, LDS_OFFTAB_MAX, LDS_SLOTS, LDS_SLOTS_WAVE = 32, 2048, 16, 4
MB_STATIC_LDS, SUBSAMPLE_LDS = 9264, 4 * (2048 + 8)


def tile_stride(npix):
    return ((npix + 15) // 32) * 32 + 16


def lds_request_bytes(P, K, O=1, slots=LDS_SLOTS, minibatch=False, draws=False, no_pixstats=False):
    """Bytes of LDS per workgroup of a launch: the dynamic request, plus (``minibatch``) the static LDS of
    tq_minibatch_kernel; ``draws``: the launch also draws the next step's subsample; ``no_pixstats``: a caller that passes
    O = 1 without pixel statistics gets the histogram form, which builds its (one-entry) table at O = 1 too."""
    table = 4 + 4 * O if (1 < O or no_pixstats) and O <= LDS_OFFTAB_MAX else 0
    dyn = 4 * (slots * (tile_stride(P * P) + 2 * K * LDS_MAX_P) + table)
    if not minibatch:
        return dyn
    return max(dyn, SUBSAMPLE_LDS if draws else 0) + MB_STATIC_LDS


def device_lds_limit(device=0):
    """LDS a workgroup may ask for on this device, as the runtime reports it (hipDeviceAttributeMaxSharedMemoryPerBlock)."""
    return int(torch.cuda.get_device_properties(device).shared_memory_per_block)


def make_oracle(d, K, perturb=0.3, seed=1, eps=EPS32, crosstalk=False):
    od = OracleData(d.images, d.xy, d.is_ontarget, d.offset.samples, d.offset.weights, mask=d.mask)
    o = (CrosstalkOracle if crosstalk else CosmosOracle)(od, K=K, eps=eps)
    p = o.init_parameters()
    g = torch.Generator().manual_seed(seed)
    for u in p.values():
        if perturb:
            u.data += perturb * torch.randn(u.shape, generator=g, dtype=torch.float64)
        u.data = u.data.float().double()  # identical parameter values on both sides
    return o


def oracle_to_engine(o, eng):
    """Copy the oracle's unconstrained leaves into the engine's flat buffer."""
    views = eng.layout.views(eng.params)
    for n, u in o.params.items():
        views[n].copy_(u.detach().to(eng.params.dtype).reshape(views[n].shape))


def fp32_latents(o, ndx, fdx, seed=3):
    """Native guide draws, rounded to float32 so oracle and kernels consume identical values.
    Returns (lat32 dict of float64 tensors holding fp32 values, base draws consistent with them)."""
    torch.manual_seed(seed)
    with torch.no_grad():
        lat = o.sample_guide(o.params, ndx, fdx)
    lat32 = {k: v.float().double() for k, v in lat.items()}
    lat32["pi"] = torch.stack([1 - lat32["pi"][..., 1], lat32["pi"][..., 1]], -1)
    if "alpha" in lat32:  # the kernels carry both components in fp32; keep them summing to one as drawn
        lat32["alpha"] = torch.stack([lat32["alpha"][..., 0], lat32["alpha"][..., 1]], -1)
    with torch.no_grad():
        dists = o._guide_dists(o.constrained(o.params), ndx, fdx)
        base = o.base_draws(lat32, dists)
    return lat32, base


def put_latents(eng, lat32, base):
    """Write latent draws into the engine's workspace and the global base draws into gbase."""
    K = eng.K
    B = lat32["background"].numel()
    rows = [lat32["background"].reshape(1, B)]
    for name in ("height", "width", "x", "y"):
        rows.append(lat32[name].reshape(K, B))
    eng.lat.copy_(torch.cat(rows, 0).reshape(-1).to(eng.lat.dtype))
    # TqGlobalBase { double gain_g; double prox_t; double lamda_g[4]; double pi_x[4][2]; }
    gb = torch.zeros_like(eng.gbase)
    gb[0] = base["gain_g"]
    gb[1] = base["proximity_t"]
    Q = eng.C
    gb[2:2 + Q] = base["lamda_g"]
    gb[6:6 + 2 * Q] = base["pi_x"].reshape(-1)
    if "alpha_x" in base:  # double alpha_x[2][2] follows pi_x[4][2]
        gb[14:18] = base["alpha_x"].reshape(-1)
    eng.gbase.copy_(gb)


def oracle_grads(o, ndx, fdx, base, detach=None):
    """``detach``: {latent name: mask} of draws that carry no pathwise gradient (the kernels' float32 clamp of an AffineBeta
    draw, which the float64 oracle does not reach at the same value: torch's clamp passes no gradient for a clamped draw)."""
    for u in o.params.values():
        u.grad = None
    lat = o.latents_from_base(o.params, ndx, fdx, base)
    for n, mask in (detach or {}).items():
        lat[n] = torch.where(mask.reshape(lat[n].shape), lat[n].detach(), lat[n])
    elbo = o.elbo(o.params, ndx, fdx, lat)
    elbo.backward()
    return float(elbo.detach()), {n: (u.grad.clone() if u.grad is not None else torch.zeros_like(u)) for n, u in o.params.items()}


def rel_err(a, b):
    """max |a-b| / max|b| (norm-wise relative error)."""
    a, b = a.double().reshape(-1), b.double().reshape(-1)
    return float((a - b).abs().max() / b.abs().max().clamp(min=1e-300))


def read_engine_latents(eng, nb, fb):
    """Latent draws of the last step as an oracle-style dict (float64 tensors holding fp32 values)."""
    K, C = eng.K, eng.C
    B = nb * fb * C
    lat = eng.lat.detach().cpu().double().view(1 + 4 * K, B)
    g = eng.globals.detach().cpu().double()
    out = {
        "background": lat[0].view(nb, fb, C),
        "height": lat[1:1 + K].view(K, nb, fb, C),
        "width": lat[1 + K:1 + 2 * K].view(K, nb, fb, C),
        "x": lat[1 + 2 * K:1 + 3 * K].view(K, nb, fb, C),
        "y": lat[1 + 3 * K:1 + 4 * K].view(K, nb, fb, C),
        "gain": g[0].clone(), "proximity": g[1].clone(),
        "lamda": g[5:5 + C].clone(),
        "pi": torch.stack([1 - g[9:9 + C], g[9:9 + C]], -1),
    }
    if getattr(eng, "crosstalk", False):  # float alpha[2][2] follows c[4]
        out["alpha"] = g[21:25].clone().view(2, 2)
    return out


# ---- gradients of whole device steps, per element ---------------------------------------------------------------------------
# A whole step writes no gradient: it leaves Adam moments.  exp_avg across one update is b1 m + (1 - b1) g, so the gradient
# the step took comes back from the two moments, for every element of every parameter, and is compared with the oracle's
# element by element.  (Parameters after the update cannot show a gradient error: Adam's update is invariant to a persistent
# factor on a gradient element, and its first step is lr sign(g).)
def _f32(v):
    return float(torch.tensor(v, dtype=torch.float32))


ADAM_B1, ADAM_B2 = _f32(0.9), _f32(0.999)  # the kernels' fp32 constants (CosmosEngine.betas); 1 - b is exact in fp32
FLT_MIN = float(torch.finfo(torch.float32).tiny)
GRAD_RTOL = 1e-4   # the project's gradient tolerance
FP32_FACTOR = 16   # allowance over the plain-fp32 oracle's own error: 2 (hardware exp2 / log2 / rcp against libm) x 4 (wave-order
#                    sums of 196-400 pixel terms against torch's pairwise sums) x 2 (fp32 series of the implicit gradients)


def oracle_grads32(o, nd, fd, base, detach=None):
    """The gradients of ``oracle_grads`` from the reference's plain float32 evaluation: a second oracle built inside
    ``oracle.cosmos.working_dtype(torch.float32)`` on the same data with the same parameter values, the base draws cast to
    float32.  Returns float64 tensors.  |oracle_grads32 - oracle_grads| is the error fp32 torch makes on the same formula."""
    from oracle.cosmos import working_dtype

    with working_dtype(torch.float32):
        d = o.data
        od = OracleData(d.images, d.xy, d.is_ontarget, d.offset_samples, d.offset_weights, mask=d.mask)
        t = type(o)(od, K=o.K, priors=o.priors, eps=o.eps)
        t.params = {n: u.detach().float().requires_grad_(True) for n, u in o.params.items()}
        _, g = oracle_grads(t, nd, fd, {k: v.float() for k, v in base.items()}, detach=detach)
    return {n: v.double() for n, v in g.items()}


def recover_step_gradient(m_before, m_after, decay_steps=1):
    """d ELBO / d param of one Adam update from exp_avg before and after it (float64 tensors holding the fp32 moments):
    m_after = b1**k m_before + (1 - b1) (-g), ``decay_steps`` = k = steps since the element's last Adam update, this one
    included (a tensor per element under the lazy clock; 1 everywhere after a ``join()``).  Returns (g, R):
    R = 4 eps32 (|m_before| + |m_after|) / (1 - b1), two fp32 roundings of the moment before and after, amplified by the
    division, times two -- what the recovery itself cannot resolve."""
    m_before, m_after = m_before.double(), m_after.double()
    k = torch.as_tensor(decay_steps, dtype=torch.float64)
    g = -(m_after - ADAM_B1 ** k * m_before) / (1.0 - ADAM_B1)
    R = 4.0 * EPS32 * (m_before.abs() + m_after.abs()) / (1.0 - ADAM_B1)
    return g, R


def _unit_of(name, shape, flat):
    """'(k, n, f, c)' of flat index ``flat`` of a parameter of shape ``shape`` ('-' for the axes it does not have)."""
    idx = [int(i) for i in torch.unravel_index(torch.tensor(flat), shape)] if len(shape) else []
    k, n, f, c = "-", "-", "-", "-"
    if len(shape) == 4:
        k, n, f, c = idx
    elif len(shape) == 3:
        n, f, c = idx
        if shape[1] == 1:
            f = "-"
    elif len(shape):
        c = tuple(idx) if len(idx) > 1 else idx[0]
    return "(k=%s, n=%s, f=%s, c=%s)" % (k, n, f, c)


def assert_gradients_match(g_dev, g64, g32, R, where, norm_only=()):
    """Recovered device gradients against the oracle's, per element, for every parameter family n (dicts of tensors of the
    oracle's shapes; ``R`` the recovery rounding of ``recover_step_gradient``):

      * finite everywhere;
      * element-wise  |g_dev - g64| <= 1e-4 |g64| + 16 E32_n + R,  E32_n = max |g32_n - g64_n|: the project's gradient
        tolerance relative to the ELEMENT, plus a fixed multiple of the error plain fp32 torch makes on the same formula;
      * norm-wise, as the staged tests have it:  max(|g_dev - g64| - R) <= 1e-4 max |g64|;
      * where the oracle's gradient is exactly zero (units outside the minibatch, per-AOI parameters of AOIs outside it,
        masked AOIs)  |g_dev| <= R.

    ``norm_only``: families held to the norm-wise check only (a test lists them with the mechanism).  Returns
    {family: worst (|g_dev - g64| - 1e-4 |g64| - R) / E32_n}: what of the factor 16 the family used (<= 0: none)."""
    worst = {}
    for n, ref in g64.items():
        ref = ref.detach().double()
        shape = tuple(ref.shape)
        got, r = g_dev[n].double().reshape(shape), R[n].double().reshape(shape)
        e32 = float((g32[n].double().reshape(shape) - ref).abs().max())
        err = (got - ref).abs()

        def fail(what, mask_or_excess):
            at = int(mask_or_excess.reshape(-1).argmax())
            return "%s: %s of %s[%d] unit %s: device %.9g oracle %.9g (fp32 oracle %.9g) R %.3g E32 %.3g" % (
                where, what, n, at, _unit_of(n, shape, at), float(got.reshape(-1)[at]), float(ref.reshape(-1)[at]),
                float(g32[n].double().reshape(-1)[at]), float(r.reshape(-1)[at]), e32)

        assert bool(torch.isfinite(got).all()), fail("non-finite gradient", (~torch.isfinite(got)).double())
        zero = ref == 0
        over = torch.where(zero, got.abs() - r, torch.full_like(err, -1.0))
        assert not bool((over > 0).any()), fail("gradient where the oracle has none", over)
        excess = err - GRAD_RTOL * ref.abs() - r
        top = float(excess.max()) if excess.numel() else 0.0
        worst[n] = top / e32 if e32 > 0 else (0.0 if top <= 0 else math.inf)
        if n not in norm_only:
            assert top <= FP32_FACTOR * e32, fail("element-wise, excess %.3g E32" % worst[n], excess)
        normwise = err - r
        assert float(normwise.max()) <= GRAD_RTOL * float(ref.abs().max()), fail("norm-wise", normwise)
    return worst


WORST_RATIOS = {}  # where -> {family: worst excess / E32_n} of the checks run so far (tests print and clear it)


def engine_state(eng):
    """(params, exp_avg, exp_avg_sq) as float64 host copies, every unit at the current Adam step (the reads join())."""
    return tuple(getattr(eng, n).detach().cpu().double().clone() for n in ("params", "exp_avg", "exp_avg_sq"))


def check_step(eng, before, after, g64, g32, where, norm_only=()):
    """One Adam update of every element between two ``engine_state`` snapshots (every unit current in both, so one decay
    step everywhere): the recovered gradient against the oracle (assert_gradients_match), the second moment against that
    gradient, and the parameters against the Adam update evaluated in float64 from the device's own moments at step count
    ``eng.adam_step``.  Returns the worst excess / E32 per family."""
    (p0, m0, v0), (p1, m1, v1) = before, after
    g, R = recover_step_gradient(m0, m1)
    lay = eng.layout
    worst = assert_gradients_match(lay.views(g), g64, g32, lay.views(R), where, norm_only)
    resid = (v1 - ADAM_B2 * v0 - (1.0 - ADAM_B2) * g ** 2).abs()
    bound = 1e-5 * v1 + 4.0 * EPS32 * (v0 + v1) + FLT_MIN
    at = int((resid - bound).argmax())
    assert bool((resid <= bound).all()), "%s: exp_avg_sq[%d] %.9g after %.9g with gradient %.9g: residual %.3g > %.3g" % (
        where, at, float(v1[at]), float(v0[at]), float(g[at]), float(resid[at]), float(bound[at]))
    t = eng.adam_step
    m_hat, v_hat = m1 / (1.0 - eng.betas[0] ** t), v1 / (1.0 - eng.betas[1] ** t)
    want = p0 - eng.lr * m_hat / (v_hat.sqrt() + eng.adam_eps)
    ok = torch.isclose(p1, want, rtol=1e-5, atol=1e-6)
    at = int((p1 - want).abs().argmax())
    assert bool(ok.all()), "%s: params[%d] %.9g, Adam step %d of the device's own moments gives %.9g" % (
        where, at, float(p1[at]), t, float(want[at]))
    rec = WORST_RATIOS.setdefault(where.split(" step ")[0], {})
    for n, w in worst.items():
        rec[n] = max(rec.get(n, -math.inf), w)
    return worst


@pytest.fixture
def gradient_report(capsys, request):
    """Prints the worst excess / E32_n per family of the gradient checks a test ran (import it into the test module and
    mark the module's tests with ``pytest.mark.usefixtures("gradient_report")``)."""
    WORST_RATIOS.clear()
    yield
    with capsys.disabled():
        for where, rec in WORST_RATIOS.items():
            fam = max(rec, key=rec.get)
            print("\ngradient check %s [%s]: worst excess / E32 %.3g (%s)  %s" % (
                request.node.name, where, rec[fam], fam, {n: round(w, 2) for n, w in rec.items() if w > 0}))
    WORST_RATIOS.clear()


# ---- whole device steps against the oracle ---------------------------------------------------------------------------------
# -ELBO relative, every parameter after the update absolute (2 % of one Adam step of lr = 0.005)
ELBO_RTOL, PARAM_ATOL = 2e-5, 1e-4


def replay_steps(eng, o, step, steps=3, where="replay", norm_only=(), clamped=None):
    """``step(eng, it)`` runs step ``it`` on the engine and returns the AOI and frame indices it ran on (host int64 tensors).
    The oracle replays each step from the device's draws: -ELBO to ELBO_RTOL, every parameter after the update to
    PARAM_ATOL; and -- what the parameters cannot show -- the gradient of every parameter recovered from the moments,
    the second moments and the update itself (check_step).  Then the oracle's parameters go back into the engine.
    ``clamped(o, lat32)``: a hook that returns, per step, {latent name: mask} of the read-back draws the kernel treated as
    clamped; the oracle detaches those before the ELBO (oracle_grads).  Without it nothing changes."""
    cuda = eng.device.type == "cuda"
    for it in range(steps):
        before = engine_state(eng)  # (joins: every unit current)
        nd, fd = step(eng, it)
        eng.join()
        if cuda:
            torch.cuda.synchronize()
        after = engine_state(eng)
        lat32 = read_engine_latents(eng, len(nd), len(fd))
        with torch.no_grad():
            base = o.base_draws(lat32, o._guide_dists(o.constrained(o.params), nd, fd))
        det = None if clamped is None else clamped(o, lat32)
        elbo_o, g64 = oracle_grads(o, nd, fd, base, detach=det)  # at the pre-step parameters: the gradients the oracle's own step takes
        g32 = oracle_grads32(o, nd, fd, base, detach=det)
        for n, u in o.params.items():  # CosmosOracle.step on those gradients (the loss is -ELBO)
            u.grad = -g64[n]
            o.optim[n].step()
        loss_o = -elbo_o
        loss_k = -float(eng.elbo_out[0])
        assert abs(loss_k - loss_o) <= ELBO_RTOL * abs(loss_o), (it, loss_k, loss_o)
        views = eng.named("params")
        for n, u in o.params.items():
            got = views[n].cpu().double().reshape(u.shape)
            err = float((got - u.detach()).abs().max())
            assert err < PARAM_ATOL, (it, n, err)
        check_step(eng, before, after, g64, g32, "%s step %d" % (where, it), norm_only)
        oracle_to_engine(o, eng)  # identical parameters on both sides for the next step


LOCAL_NAMES = ("m_probs", "h_loc", "h_beta", "w_mean", "w_size", "x_mean", "y_mean", "size", "b_loc", "b_beta")


def lr0_sequence(eng, o, plan, where, norm_only=()):
    """Steps with ``eng.lr = 0`` and NO join() between them, so that every tail runs where a fit runs it: inside the next
    launch.  The parameters never move -- the oracle holds them exactly at every step with nothing read back -- while the
    moments still accumulate b1 m + (1 - b1) g, and every step's gradient comes back from exp_avg read raw after each launch:

      * local parameters of step t from the local block across launch t; the decay count of every unit comes from a table of
        last updates kept HERE (a unit of the batch: every step since its last update, the catch-up of the lazy clock
        included).  Units outside the batch are either bit-unchanged, or -- where the launch brought every unit to the
        current step first -- decayed with no gradient;
      * per-AOI and global parameters of step t from the rest of the buffer across the launch that ran tail t: launch t + 1
        where the step left its tail pending (and then the block is bit-unchanged across launch t), launch t itself otherwise;
      * -ELBO of step t where free_run reads it.
    The last tail, and the decay of every unit a lazy step left behind, come after the final join().

    ``plan``: one dict per step with ``nd`` / ``fd`` (host index tensors, None = whole axis) and optionally ``pre(eng)``,
    ``post(eng)`` (called before / right after the launch) and ``kw`` (keyword arguments of ``step``).  Returns, per step,
    whether its tail was left pending."""
    eng.lr = 0.0
    eng.__dict__.pop("_tmpl_key", None)  # (argument templates carry the learning rate)
    lay, cuda = eng.layout, eng.device.type == "cuda"
    nl, Nt, F, C = lay.n_local, eng.Nt, eng.F, eng.C
    rows = nl // lay.U
    rest_names = [n for n in o.params if n not in LOCAL_NAMES]

    def raw():
        if cuda:
            torch.cuda.synchronize()
        return eng._exp_avg.detach().cpu().double().clone()

    def rest_views(flat_rest):
        full = torch.cat([torch.zeros(nl, dtype=torch.float64), flat_rest])
        return {n: v for n, v in lay.views(full).items() if n in rest_names}

    def local_views(flat_local):
        full = torch.cat([flat_local.reshape(-1), torch.zeros(lay.total - nl, dtype=torch.float64)])
        return {n: v for n, v in lay.views(full).items() if n in LOCAL_NAMES}

    def record(worst):
        rec = WORST_RATIOS.setdefault(where, {})
        for n, w in worst.items():
            rec[n] = max(rec.get(n, -math.inf), w)

    def check_rest(m0, m1, tails, tag):
        """``tails``: (g64, g32) of the tails the launch ran, oldest first: m1 = b1^k m0 + (1 - b1) sum b1^(k-1-i) (-g_i)."""
        k = len(tails)
        g, R = recover_step_gradient(m0[nl:], m1[nl:], k)
        mix = lambda which: {n: sum(ADAM_B1 ** (k - 1 - i) * tl[which][n].detach().double() for i, tl in enumerate(tails))
                             for n in rest_names}
        record(assert_gradients_match(rest_views(g), mix(0), mix(1), rest_views(R), "%s %s" % (where, tag), norm_only))

    def check_elbo(it, loss_o):
        loss_k = -float(eng.elbo_out[0])
        assert abs(loss_k - loss_o) <= ELBO_RTOL * abs(loss_o), (where, it, loss_k, loss_o)

    eng.join()
    p0 = eng._params.detach().cpu().clone()
    m_prev = raw()
    clock = torch.zeros(Nt, F, dtype=torch.int64) + eng.adam_step  # Adam steps every unit has taken
    t0 = eng.adam_step
    owed, pendings = None, []
    for it, e in enumerate(plan):
        t = t0 + it
        if e.get("pre") is not None:
            e["pre"](eng)
        nd, fd = e.get("nd"), e.get("fd")
        eng.step(nd, fd, **e.get("kw", {}))
        if e.get("post") is not None:
            e["post"](eng)
        m_now = raw()
        pending = eng._tail_args is not None or eng._pending is not None
        pendings.append(pending)
        nd_ = torch.arange(Nt) if nd is None else nd
        fd_ = torch.arange(F) if fd is None else fd
        lat32 = read_engine_latents(eng, len(nd_), len(fd_))
        with torch.no_grad():
            base = o.base_draws(lat32, o._guide_dists(o.constrained(o.params), nd_, fd_))
        elbo_o, g64 = oracle_grads(o, nd_, fd_, base)
        g32 = oracle_grads32(o, nd_, fd_, base)
        # ---- local block across this launch
        inb = torch.zeros(Nt, F, dtype=torch.bool)
        inb[nd_[:, None], fd_[None, :]] = True
        l0, l1 = m_prev[:nl].view(rows, Nt, F, C), m_now[:nl].view(rows, Nt, F, C)
        out = (~inb)[None, :, :, None].expand_as(l0)
        caught_up = not torch.equal(l0[out], l1[out])  # the launch brought the units outside the batch to step t first
        k = torch.where(inb, t + 1 - clock, (t - clock) if caught_up else torch.zeros_like(clock))
        clock = torch.where(inb, torch.full_like(clock, t + 1), torch.full_like(clock, t) if caught_up else clock)
        g, R = recover_step_gradient(l0, l1, k[None, :, :, None].expand_as(l0))
        loc64 = {n: v for n, v in g64.items() if n in LOCAL_NAMES}
        record(assert_gradients_match(local_views(g), loc64, g32, local_views(R), "%s step %d" % (where, it), norm_only))
        # ---- the rest of the buffer: the tails this launch ran
        tails = ([owed[1:]] if owed is not None else []) + ([] if pending else [(g64, g32)])
        if tails:
            check_rest(m_prev, m_now, tails, "tail run by launch %d" % it)
        else:
            assert torch.equal(m_prev[nl:], m_now[nl:]), (where, it, "a launch that left its tail pending moved per-AOI / global moments")
        if pending:
            if owed is not None:
                check_elbo(it - 1, owed[0])
            owed = (-elbo_o, g64, g32)
        else:
            check_elbo(it, -elbo_o)
            owed = None
        m_prev = m_now
    T = t0 + len(plan)
    eng.join()
    m_fin = raw()
    assert eng.adam_step == T
    if owed is not None:
        check_elbo(len(plan) - 1, owed[0])
        check_rest(m_prev, m_fin, [owed[1:]], "tail after the last join")
    else:
        assert torch.equal(m_prev[nl:], m_fin[nl:])
    l0, l1 = m_prev[:nl].view(rows, Nt, F, C), m_fin[:nl].view(rows, Nt, F, C)
    g, R = recover_step_gradient(l0, l1, (T - clock)[None, :, :, None].expand_as(l0))
    zeros = {n: torch.zeros_like(u.detach()) for n, u in o.params.items() if n in LOCAL_NAMES}
    assert_gradients_match(local_views(g), zeros, zeros, local_views(R), "%s catch-up of the last join" % where)
    assert torch.equal(eng._params.detach().cpu(), p0), (where, "lr = 0 moved a parameter")
    return pendings


# ---- free-running trajectories: nothing is copied back into the engine -------------------------------------------------------
def oracle_twin(o):
    """A second oracle on the same data with the same parameter values and a fresh Adam state (``o`` has not stepped yet)."""
    t = type(o)(o.data, K=o.K, priors=o.priors, eps=o.eps)
    t.params = {n: u.detach().clone().requires_grad_(True) for n, u in o.params.items()}
    t.make_optim(lr=next(iter(o.optim.values())).param_groups[0]["lr"])
    return t


def oracle_step_from_latents(o, nd, fd, lat32, grad_eps=0.0, generator=None, round32=False):
    """One oracle step on latent VALUES ``lat32`` (the base draws behind them are recovered with the oracle's own parameters,
    as replay() does).  ``grad_eps``: every gradient element is multiplied by 1 + grad_eps randn before Adam;
    ``round32``: the parameters are rounded to float32 after the update.  Returns the loss (-ELBO)."""
    with torch.no_grad():
        base = o.base_draws(lat32, o._guide_dists(o.constrained(o.params), nd, fd))
    for u in o.params.values():
        u.grad = None
    loss = -o.elbo(o.params, nd, fd, o.latents_from_base(o.params, nd, fd, base))
    loss.backward()
    for n, u in o.params.items():
        if u.grad is None:
            u.grad = torch.zeros_like(u)
        if grad_eps:
            u.grad.mul_(1.0 + grad_eps * torch.randn(u.shape, generator=generator, dtype=u.dtype))
        o.optim[n].step()
        if round32:
            u.data = u.data.float().double()
    return float(loss.detach())


def _max_diff(a, b):
    """{family: max |a - b|} of two oracles' parameters."""
    return {n: float((a.params[n].detach() - u.detach()).abs().max()) for n, u in b.params.items()}


def free_run(eng, o, N, F, steps, nb=None, fb=None, seed=5, expect=None, extra_eps=(), check_at=(10, 25)):
    """``steps`` steps of the engine and of the oracle side by side, each with its OWN parameters and Adam state from a common
    start: every step the engine's latent draws go to the oracle (read_engine_latents + base_draws, as in replay()), and
    nothing ever goes back.  A gradient error the step-by-step replays wipe out accumulates here, and so does an error in how
    the Adam moments or the lazy-Adam clock carry from step to step.  The engine runs as a fit runs it: the tail of a step
    stays pending and runs inside the next launch (its ELBO is compared then), ``join()`` -- which also brings every unit of a
    lazy-Adam fit to the current step -- is called only where the parameters are read: after steps ``check_at`` and the last.

    The bound comes from the reference alone.  Two more copies of the oracle take the same latents:
      * the tolerated-error twin multiplies every gradient element by 1 + 1e-4 randn (fixed generator) before Adam: 1e-4 is
        the gradient tolerance the suite grants the kernels;
      * the storage twin rounds its parameters to float32 after every step.
    drift(twin) = max over all parameters of |twin - oracle|.  At every check, for every parameter family,
        max |engine - oracle| <= 3 drift(tolerated twin) + drift(storage twin)
    (3: the twin's noise is random and adds in quadrature, a kernel's error of that size may be systematic); -ELBO agrees to
    ELBO_RTOL at every step.  ``extra_eps``: further gradient-noise twins, recorded only.  ``eng`` = None: no engine, the
    latents are the oracle's own float32-rounded guide draws (the twins and the bound by themselves).

    Returns one record per check: step, bound, drift of each twin ("tolerated", "storage", every extra eps) and "engine" =
    {family: (max |engine - oracle|, flat index of that element)}."""
    twins = {"tolerated": (oracle_twin(o), 1e-4, False), "storage": (oracle_twin(o), 0.0, True)}
    for e in extra_eps:
        twins[e] = (oracle_twin(o), e, False)
    noise = {k: torch.Generator().manual_seed(100 + i) for i, k in enumerate(twins)}
    g = torch.Generator().manual_seed(seed)
    mini = nb is not None
    cuda = eng is not None and eng.device.type == "cuda"
    owed = None  # (step, oracle loss) of a step whose device ELBO is still in its pending tail
    records = []

    def settle(owed):
        it, loss_o = owed
        loss_k = -float(eng.elbo_out[0])
        assert abs(loss_k - loss_o) <= ELBO_RTOL * abs(loss_o), (it, loss_k, loss_o)

    for it in range(steps):
        nd = torch.randperm(N, generator=g)[:nb] if mini else torch.arange(N)
        fd = torch.randperm(F, generator=g)[:fb] if mini else torch.arange(F)
        if eng is None:
            lat32, _ = fp32_latents(o, nd, fd, seed=seed + it)
        else:
            eng.step(nd if mini else None, fd if mini else None)
            if expect is not None:
                expect(eng)
            if cuda:
                torch.cuda.synchronize()
            if owed is not None:  # the launch just run carried the tail of the step before
                settle(owed)
            lat32 = read_engine_latents(eng, len(nd), len(fd))
        loss_o = oracle_step_from_latents(o, nd, fd, lat32)
        for k, (t, e, r32) in twins.items():
            oracle_step_from_latents(t, nd, fd, lat32, grad_eps=e, generator=noise[k], round32=r32)
        if eng is not None:
            owed = (it, loss_o)
            if eng._tail_args is None and eng._pending is None:  # nothing deferred: the ELBO of this step is out
                settle(owed)
                owed = None
        if it + 1 in check_at or it + 1 == steps:
            rec = {"step": it + 1}
            for k, (t, _, _) in twins.items():
                rec[k] = max(_max_diff(t, o).values())
            rec["bound"] = 3.0 * rec["tolerated"] + rec["storage"]
            if eng is not None:
                views = eng.named("params")  # join(): the pending tail, and every unit at the current Adam step
                if cuda:
                    torch.cuda.synchronize()
                if owed is not None:
                    settle(owed)
                    owed = None
                rec["engine"] = {}
                for n, u in o.params.items():
                    diff = (views[n].cpu().double().reshape(u.shape) - u.detach()).abs().reshape(-1)
                    rec["engine"][n] = (float(diff.max()), int(diff.argmax()))
                    assert math.isfinite(rec["engine"][n][0]) and rec["engine"][n][0] <= rec["bound"], (n, rec)
            records.append(rec)
    return records
