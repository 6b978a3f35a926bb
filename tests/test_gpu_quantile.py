"""``tq_credible_intervals`` on the device against scipy: the raw entry point on the test grid, the two helpers of
``tapqir_amd.utils.stats``, ``compute_params`` of a real model, and the argument checks of the C ABI."""

import ctypes as C
import math

import numpy as np
import pytest
import torch

from helpers import make_dataset, make_oracle, oracle_to_engine
from quantile_fixture import BOUNDS, CIS, KIND_AFFINE_BETA, KIND_GAMMA, TOL, beta_grid, beta_oracle, gamma_grid, gamma_oracle, worst_error
from tapqir_amd import _lib
from tapqir_amd.utils import stats

TILED = 70001  # 273 full workgroups and a ragged last one


def launch(kind, p0, p1, low, high, ci, n=None):
    """One ``tq_credible_intervals`` call on device copies of p0 / p1; (rc, LL, UL) with the outputs as numpy arrays."""
    dev = torch.device("cuda:0")
    a0, a1 = p0.to(dev).contiguous(), p1.to(dev).contiguous()
    ll = torch.full((a0.numel(),), -1.0, dtype=torch.float64, device=dev)
    ul = torch.full((a0.numel(),), -1.0, dtype=torch.float64, device=dev)
    a = _lib.IntervalArgs()
    a.kind, a.p0, a.p1, a.ll, a.ul = kind, _lib.ptr(a0), _lib.ptr(a1), _lib.ptr(ll), _lib.ptr(ul)
    a.n, a.ci, a.low, a.high = (a0.numel() if n is None else n), ci, low, high
    rc = _lib.load().tq_credible_intervals(C.byref(a), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    torch.cuda.synchronize()
    return rc, ll.cpu().numpy(), ul.cpu().numpy()


def tiled(t, n):
    return t.repeat(-(-n // t.numel()))[:n]


@pytest.mark.gpu
@pytest.mark.parametrize("CI", CIS)
def test_gamma_kernel_matches_scipy(CI):
    loc, beta = gamma_grid()
    ref_ll, ref_ul = gamma_oracle(CI)
    rc, ll, ul = launch(KIND_GAMMA, loc, beta, 0.0, 0.0, CI)
    assert rc == 0
    err = worst_error(ll, ul, ref_ll, ref_ul)
    print(f"gamma device CI={CI}: worst error / width = {err:.3e}")
    assert err <= TOL
    rc, ll, ul = launch(KIND_GAMMA, tiled(loc, TILED), tiled(beta, TILED), 0.0, 0.0, CI)
    assert rc == 0
    reps = -(-TILED // loc.numel())
    assert worst_error(ll, ul, np.tile(ref_ll, reps)[:TILED], np.tile(ref_ul, reps)[:TILED]) <= TOL


@pytest.mark.gpu
@pytest.mark.parametrize("CI", CIS)
@pytest.mark.parametrize("bounds", BOUNDS)
def test_beta_kernel_matches_scipy(bounds, CI):
    mean, size = beta_grid(*bounds)
    ref_ll, ref_ul = beta_oracle(*bounds, CI)
    rc, ll, ul = launch(KIND_AFFINE_BETA, mean, size, bounds[0], bounds[1], CI)
    assert rc == 0
    err = worst_error(ll, ul, ref_ll, ref_ul)
    print(f"beta device {bounds} CI={CI}: worst error / width = {err:.3e}")
    assert err <= TOL
    rc, ll, ul = launch(KIND_AFFINE_BETA, tiled(mean, TILED), tiled(size, TILED), bounds[0], bounds[1], CI)
    assert rc == 0
    reps = -(-TILED // mean.numel())
    assert worst_error(ll, ul, np.tile(ref_ll, reps)[:TILED], np.tile(ref_ul, reps)[:TILED]) <= TOL


@pytest.mark.gpu
def test_kernel_writes_only_its_n_elements():
    """n below the buffers' length: the elements behind n keep their fill value."""
    loc, beta = gamma_grid()
    rc, ll, ul = launch(KIND_GAMMA, loc, beta, 0.0, 0.0, 0.95, n=37)
    assert rc == 0
    assert (ll[37:] == -1.0).all() and (ul[37:] == -1.0).all() and (ll[:37] >= 0.0).all() and (ul[:37] > 0.0).all()


@pytest.mark.gpu
def test_device_helpers_keep_shape_dtype_and_mean():
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(5)
    shape = (2, 3, 4, 1)
    loc = (torch.rand(shape, generator=g) * 300 + 0.5).to(dev)
    beta = (torch.rand(shape, generator=g) * 3 + 0.1).to(dev)
    mean = (torch.rand(shape, generator=g) * 1.4 + 0.8).to(dev)
    size = (torch.rand(shape, generator=g) * 500 + 2.0).to(dev)
    for got, ref in ((stats.gamma_interval_device(loc, beta, 0.95), stats.gamma_interval(loc, beta, 0.95)),
                     (stats.affine_beta_interval_device(mean, size, 0.75, 2.25, 0.95),
                      stats.affine_beta_interval(mean, size, 0.75, 2.25, 0.95))):
        for t in got:
            assert t.shape == shape and t.dtype == torch.float64 and t.device.type == "cpu"
        assert torch.equal(got[2], ref[2])
        assert worst_error(got[0].numpy(), got[1].numpy(), ref[0].numpy(), ref[1].numpy()) <= TOL


@pytest.mark.gpu
def test_device_helpers_refuse_cpu_tensors():
    from tapqir_amd.exceptions import HipExtensionError

    with pytest.raises(HipExtensionError):
        stats.gamma_interval_device(torch.ones(3), torch.ones(3), 0.95)
    with pytest.raises(HipExtensionError):
        stats.affine_beta_interval_device(torch.ones(3), torch.full((3,), 4.0), 0.0, 2.0, 0.95)


LOCAL = ("background", "height", "width", "x", "y")
GLOBAL = ("gain", "pi", "lamda", "proximity")


@pytest.mark.gpu
@pytest.mark.parametrize("K,dkw", [(2, dict(N=3, F=4)), (3, dict(N=2, F=2, P=20))])
def test_compute_params_matches_the_scipy_helpers(K, dkw):
    from tapqir_amd.models.cosmos import cosmos

    m = cosmos(K=K, device="cuda")
    m.data = make_dataset(K=K, **dkw)
    eng = m._make_engine()
    oracle_to_engine(make_oracle(m.data, K, perturb=0.3), eng)
    out = m.compute_params(0.95)
    assert set(out) == set(LOCAL) | set(GLOBAL) | {"m_probs", "z_probs", "theta_probs", "z_map", "p_specific"}

    cp = {n: v.detach() for n, v in eng.layout.constrained(eng.params).items()}
    P, pr = m.data.P, m.priors
    H = (P + 1) / 2
    ref = {
        "gain": stats.gamma_interval(cp["gain_loc"], cp["gain_beta"], 0.95),
        "pi": stats.dirichlet_interval(cp["pi_mean"] * cp["pi_size"], 0.95),
        "lamda": stats.gamma_interval(cp["lamda_loc"], cp["lamda_beta"], 0.95),
        "proximity": stats.affine_beta_interval(cp["proximity_loc"], cp["proximity_size"], 0.0, (P + 1) / math.sqrt(12), 0.95),
        "background": stats.gamma_interval(cp["b_loc"], cp["b_beta"], 0.95),
        "height": stats.gamma_interval(cp["h_loc"], cp["h_beta"], 0.95),
        "width": stats.affine_beta_interval(cp["w_mean"], cp["w_size"], pr["width_min"], pr["width_max"], 0.95),
        "x": stats.affine_beta_interval(cp["x_mean"], cp["size"], -H, H, 0.95),
        "y": stats.affine_beta_interval(cp["y_mean"], cp["size"], -H, H, 0.95),
    }
    for name, (ll, ul, mean) in ref.items():
        got = out[name]
        assert set(got) == {"LL", "UL", "Mean"}
        for key, r in (("LL", ll), ("UL", ul), ("Mean", mean)):
            assert got[key].shape == r.shape and got[key].dtype == r.dtype == torch.float64, (name, key)
            assert got[key].device.type == "cpu"
        assert torch.equal(got["Mean"], mean), name
        if name in GLOBAL:
            assert torch.equal(got["LL"], ll) and torch.equal(got["UL"], ul), name
        else:
            assert worst_error(got["LL"].numpy().ravel(), got["UL"].numpy().ravel(), ll.numpy().ravel(), ul.numpy().ravel()) <= TOL, name
        assert bool((got["LL"] < got["Mean"]).all()) and bool((got["Mean"] < got["UL"]).all()), name
    Nt, F, Q = m.data.Nt, m.data.F, m.data.C
    assert out["background"]["LL"].shape == (Nt, F, Q) and out["x"]["UL"].shape == (K, Nt, F, Q)
    for name, shape, dtype in (("m_probs", (K, Nt, F, Q), torch.float32), ("z_probs", (Nt, F, Q, 2), torch.float32),
                               ("theta_probs", (K, Nt, F, Q), torch.float32), ("z_map", (Nt, F, Q), torch.int64),
                               ("p_specific", (Nt, F, Q), torch.float32)):
        assert out[name].shape == shape and out[name].dtype == dtype and out[name].device.type == "cpu", name


@pytest.mark.gpu
def test_argument_checks_return_err_arg_and_launch_nothing():
    lib = _lib.load()
    dev = torch.device("cuda:0")
    p0 = torch.ones(8, device=dev)
    p1 = torch.ones(8, device=dev)
    ll = torch.full((8,), -1.0, dtype=torch.float64, device=dev)
    ul = torch.full((8,), -1.0, dtype=torch.float64, device=dev)

    def args(**kw):
        a = _lib.IntervalArgs()
        a.kind, a.p0, a.p1, a.ll, a.ul = _lib.INTERVAL_GAMMA, _lib.ptr(p0), _lib.ptr(p1), _lib.ptr(ll), _lib.ptr(ul)
        a.n, a.ci, a.low, a.high = 8, 0.95, 0.0, 1.0
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    bad = [args(p0=None), args(p1=None), args(ll=None), args(ul=None), args(n=0), args(ci=1.0), args(ci=0.0),
           args(ci=float("nan")), args(kind=2), args(kind=-1), args(kind=_lib.INTERVAL_AFFINE_BETA, low=1.0, high=1.0)]
    for a in bad:
        assert lib.tq_credible_intervals(C.byref(a), stream) == 1  # TQ_ERR_ARG
        assert len(lib.tq_last_error()) > 0
    assert lib.tq_credible_intervals(None, stream) == 1
    torch.cuda.synchronize()
    assert bool((ll == -1.0).all()) and bool((ul == -1.0).all())  # nothing was launched
    assert lib.tq_credible_intervals(C.byref(args()), stream) == 0
    torch.cuda.synchronize()
    assert bool((ll > 0.0).all()) and bool((ul > ll).all())
