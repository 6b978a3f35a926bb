"""Test-side helpers of the time-to-first-binding tests: the g++ build of tq_kinetics.h and a float64 torch restatement
of the reference's censored-mixture MLE (tapqir/utils/mle_analysis.py:49-101 with torch.optim.Adam)."""

import ctypes as C
import os

import torch

from helpers import adam64, build_host_check

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "hostcheck", "kinetics_check.cpp")


def build_kinetics_check(out_dir):
    """Compile tests/hostcheck/kinetics_check.cpp into ``out_dir`` and bind it."""
    so = os.path.join(str(out_dir), "libtq_kinetics_check.so")
    build_host_check(SRC, so)
    lib = C.CDLL(so)
    fp, dp = C.POINTER(C.c_float), C.POINTER(C.c_double)
    lib.hk_ttfb_point.argtypes = [fp, C.c_float, C.c_float, C.c_int, fp]
    lib.hk_ttfb_point.restype = None
    lib.hk_ttfb_prefix.argtypes = [fp, dp, C.c_int, C.c_int]
    lib.hk_ttfb_prefix.restype = None
    lib.hk_ttfb_search.argtypes = [dp, C.c_int, C.c_double]
    lib.hk_ttfb_search.restype = C.c_int
    lib.hk_ttfb_sample.argtypes = [dp, fp, C.c_int, C.c_int, C.c_int, C.c_uint64]
    lib.hk_ttfb_sample.restype = None
    lib.hk_log1p_det.argtypes = [C.c_double]
    lib.hk_log1p_det.restype = C.c_double
    return lib


def fptr(t):
    return C.cast(t.data_ptr(), C.POINTER(C.c_float))


def dptr(t):
    return C.cast(t.data_ptr(), C.POINTER(C.c_double))


def host_prefix(lib, p):
    p = p.detach().cpu().float().contiguous()
    N, F = p.shape
    L = torch.empty(N, F, dtype=torch.float64)
    lib.hk_ttfb_prefix(fptr(p), dptr(L), N, F)
    return L


def host_sample(lib, p, S, seed):
    L = host_prefix(lib, p)
    N, F = L.shape
    tau = torch.empty(S, N, dtype=torch.float32)
    lib.hk_ttfb_sample(dptr(L), fptr(tau), N, F, S, seed)
    return tau


def loglik64(par, data, Tmax, control=None):
    """Per-sample log-likelihood of mle_analysis.py:49-101 in float64: par (S, 3) unconstrained (log ka, log kns,
    logit Af), data (S, N), control (S, Nc) or None."""
    ka, kns, Af = par[:, 0:1].exp(), par[:, 1:2].exp(), torch.sigmoid(par[:, 2:3])
    k0, k1 = kns, ka + kns
    la, lb = torch.log(Af), torch.log1p(-Af)
    inner = (data > 0) & (data < Tmax)
    tau = data.masked_fill(~inner, 1.0)
    t_in = torch.logaddexp(la + k1.log() - k1 * tau, lb + k0.log() - k0 * tau)
    t_cens = torch.logaddexp(la - k1 * Tmax, lb - k0 * Tmax)
    ll = torch.where(inner, t_in, torch.zeros_like(t_in)).sum(1) + torch.where(data == Tmax, t_cens,
                                                                               torch.zeros_like(t_in)).sum(1)
    if control is not None:
        ci = (control > 0) & (control < Tmax)
        tc = control.masked_fill(~ci, 1.0)
        ll = ll + torch.where(ci, kns.log() - kns * tc, torch.zeros_like(tc)).sum(1)
        ll = ll + torch.where(control == Tmax, -kns * Tmax, torch.zeros_like(tc)).sum(1)
    return ll


def torch_fit64(data, Tmax, control=None, n_steps=300, lr=5e-3):
    """The reference's fit restated in float64 torch: autograd + torch.optim.Adam from the same initial values."""
    data = data.double().cpu()
    control = None if control is None else control.double().cpu()
    S = data.shape[0]
    init = torch.tensor([0.001, 0.001, 0.9], dtype=torch.float32)
    par0 = torch.stack([init[0].log(), init[1].log(), init[2].logit()]).double()
    p = adam64(par0.expand(S, 3), lambda par: loglik64(par, data, Tmax, control), n_steps, lr)
    return {"ka": p[:, 0:1].exp(), "kns": p[:, 1:2].exp(), "Af": torch.sigmoid(p[:, 2:3])}
