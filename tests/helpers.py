"""Shared test utilities: problem construction, oracle <-> engine plumbing, host-check loader."""

import ctypes as C
import math
import os
import subprocess

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
    if mask is not None:
        d.mask = mask
    return d


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


def oracle_grads(o, ndx, fdx, base):
    for u in o.params.values():
        u.grad = None
    lat = o.latents_from_base(o.params, ndx, fdx, base)
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


# ---- whole device steps against the oracle ---------------------------------------------------------------------------------
# the tolerances of test_gpu_production_kernels.replay: -ELBO relative, every parameter after the update absolute (2 % of one
# Adam step of lr = 0.005)
ELBO_RTOL, PARAM_ATOL = 2e-5, 1e-4


def replay_steps(eng, o, step, steps=3):
    """test_gpu_production_kernels.replay with the device step left to the caller: ``step(eng, it)`` runs step ``it`` on the
    engine and returns the AOI and frame indices it ran on (host int64 tensors).  The oracle replays each step from the
    device's draws, the same assertions are made, and the oracle's parameters go back into the engine."""
    for it in range(steps):
        nd, fd = step(eng, it)
        eng.join()
        torch.cuda.synchronize()
        lat32 = read_engine_latents(eng, len(nd), len(fd))
        with torch.no_grad():
            base = o.base_draws(lat32, o._guide_dists(o.constrained(o.params), nd, fd))
        loss_o = o.step(nd, fd, base=base)
        loss_k = -float(eng.elbo_out[0])
        assert abs(loss_k - loss_o) <= ELBO_RTOL * abs(loss_o), (it, loss_k, loss_o)
        views = eng.named("params")
        for n, u in o.params.items():
            got = views[n].cpu().double().reshape(u.shape)
            err = float((got - u.detach()).abs().max())
            assert err < PARAM_ATOL, (it, n, err)
        oracle_to_engine(o, eng)


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
