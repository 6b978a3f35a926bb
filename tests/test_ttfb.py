"""Time-to-first-binding analysis without a GPU: time_to_first_binding against brute force and exact enumeration,
the g++ build of tq_kinetics.h against float64 autograd, the C layout of the new argument structs, and the exits of
the ``ttfb`` command."""

import ctypes
import itertools
import os
import subprocess
import tempfile

import numpy as np
import pytest
import torch
from typer.testing import CliRunner

from tapqir_amd import _lib
from tapqir_amd.main import app
from tapqir_amd.utils.dataset import save
from tapqir_amd.utils.imscroll import time_to_first_binding
from tapqir_amd.utils.simulate import TEST_PARAMS, simulate
from ttfb_fixture import build_kinetics_check, dptr, host_prefix, loglik64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
runner = CliRunner()


@pytest.fixture(scope="module")
def hk(tmp_path_factory):
    return build_kinetics_check(tmp_path_factory.mktemp("kinetics"))


def first_one(row):
    for f, v in enumerate(row):
        if v:
            return f
    return len(row)


def test_time_to_first_binding_binary():
    rng = np.random.default_rng(0)
    for F in (1, 2, 7, 40):
        z = rng.random((50, F)) < rng.choice([0.02, 0.2, 0.7], size=(50, 1))
        want = np.array([first_one(r) for r in z], dtype=float)
        np.testing.assert_array_equal(time_to_first_binding(z), want)
        np.testing.assert_array_equal(time_to_first_binding(torch.from_numpy(z)).numpy(), want)


def test_time_to_first_binding_expectation_is_exact():
    """For probabilities the result is E[first success index] under independent frames: enumerate every sequence."""
    rng = np.random.default_rng(1)
    for F in (1, 3, 6, 10):
        p = rng.random((4, F))
        p[0, 2 % F] = 1.0  # certain binding
        p[1] = 0.0         # never binds
        want = np.zeros(4)
        for z in itertools.product((0, 1), repeat=F):
            z = np.array(z)
            prob = np.prod(np.where(z == 1, p, 1 - p), axis=-1)
            want += prob * first_one(z)
        np.testing.assert_allclose(time_to_first_binding(p), want, rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(time_to_first_binding(torch.from_numpy(p)).double().numpy(), want, rtol=1e-5)


def test_point_terms_and_gradients_match_float64_autograd(hk):
    """Per data point: log-likelihood term and its gradient in (log ka, log kns, logit Af), extreme values included
    (k tau up to 1e4, far beyond exp's range of 88; Af within 1e-6 of 0 and 1)."""
    T = 1000.0
    ks = [1e-6, 1e-3, 0.05, 10.0]
    afs = [1e-6, 0.3, 0.9, 1 - 1e-6]
    taus = [1.0, 7.0, 500.0, T - 1, T]
    worst = 0.0
    for ka, kns, af, tau, control in itertools.product(ks, ks, afs, taus, (0, 1)):
        par32 = torch.tensor([np.log(ka), np.log(kns), np.log(af / (1 - af))], dtype=torch.float32)
        out = (ctypes.c_float * 4)()
        hk.hk_ttfb_point(ctypes.cast(par32.data_ptr(), ctypes.POINTER(ctypes.c_float)), tau, T, control, out)
        got = np.array(out[:])
        par = par32.double().reshape(1, 3).requires_grad_(True)
        x = torch.tensor([[tau]], dtype=torch.float64)
        ll = loglik64(par, torch.zeros(1, 1, dtype=torch.float64), T, x) if control else loglik64(par, x, T)
        (g,) = torch.autograd.grad(ll.sum(), par)
        want = np.concatenate([[ll.item()], g[0].numpy()])
        # relative error, floored at 1 (a gradient of 1e-7 next to terms of order one is float32's absolute noise)
        err = np.abs(got - want) / np.maximum(np.abs(want), 1.0)
        assert np.all(np.isfinite(got)), (ka, kns, af, tau, control, got)
        assert err.max() < 1e-5, (ka, kns, af, tau, control, got, want)
        worst = max(worst, err.max())
    print(f"worst relative error {worst:.2e}")


def test_point_at_zero_contributes_nothing(hk):
    out = (ctypes.c_float * 4)()
    par = torch.tensor([-3.0, -5.0, 1.0], dtype=torch.float32)
    for control in (0, 1):
        hk.hk_ttfb_point(ctypes.cast(par.data_ptr(), ctypes.POINTER(ctypes.c_float)), 0.0, 100.0, control, out)
        assert list(out) == [0.0, 0.0, 0.0, 0.0]


def test_log1p_is_accurate(hk):
    xs = np.concatenate([-np.logspace(-300, -1e-9, 200), np.logspace(-300, 3, 200), [-0.5, 0.5, -0.999999, 1.0]])
    got = np.array([hk.hk_log1p_det(float(x)) for x in xs])
    np.testing.assert_allclose(got, np.log1p(xs), rtol=4e-16, atol=0)
    assert hk.hk_log1p_det(-1.0) == -np.inf


def test_search_gives_the_first_success_on_binary_rows(hk):
    rng = np.random.default_rng(2)
    z = (rng.random((64, 37)) < 0.08).astype(np.float32)
    z[0] = 0.0
    z[1] = 1.0
    L = host_prefix(hk, torch.from_numpy(z))
    for n in range(z.shape[0]):
        row = L[n].contiguous()
        for lu in (-1e-12, -0.7, -30.0, np.log(2.0 ** -24)):
            assert hk.hk_ttfb_search(dptr(row), z.shape[1], lu) == first_one(z[n])


def test_search_inverts_the_survival_function(hk):
    p = torch.tensor([[0.1, 0.5, 0.0, 0.25, 1.0, 0.3]])
    L = host_prefix(hk, p)[0].contiguous()
    surv = torch.cumprod(1 - p[0].double(), 0)
    for f in range(6):
        for lu in (torch.log(surv[f]) + 1e-9, torch.log(surv[f]) - 1e-9):
            want = next((j for j in range(6) if surv[j] < torch.exp(lu)), 6)
            assert hk.hk_ttfb_search(dptr(L), 6, float(lu)) == want


def test_ttfb_struct_layout_matches_the_c_header():
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "tapqir_hip.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %d %d\n", sizeof(tq_ttfb_sample_args), offsetof(tq_ttfb_sample_args, N),
         offsetof(tq_ttfb_sample_args, seed), sizeof(tq_ttfb_fit_args), offsetof(tq_ttfb_fit_args, S),
         offsetof(tq_ttfb_fit_args, Tmax), offsetof(tq_ttfb_fit_args, lr), offsetof(tq_ttfb_fit_args, eps),
         TQ_TTFB_LDS_POINTS, TQ_TTFB_STATE);
  return 0;
}'''
    with tempfile.TemporaryDirectory() as td:
        c = os.path.join(td, "s.c")
        open(c, "w").write(src)
        exe = os.path.join(td, "s")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        got = [int(v) for v in subprocess.check_output([exe]).split()]
    Sa, Fa = _lib.TtfbSampleArgs, _lib.TtfbFitArgs
    want = [ctypes.sizeof(Sa), Sa.N.offset, Sa.seed.offset, ctypes.sizeof(Fa), Fa.S.offset, Fa.Tmax.offset,
            Fa.lr.offset, Fa.eps.offset, _lib.TTFB_LDS_POINTS, _lib.TTFB_STATE]
    assert got == want


def test_ttfb_entry_points_validate_without_a_gpu():
    from tapqir_amd.build import build

    build(verbose=False)
    lib = _lib.load()
    a = _lib.TtfbSampleArgs()
    assert lib.tq_ttfb_sample(ctypes.byref(a), None) == 1  # TQ_ERR_ARG
    assert b"NULL" in lib.tq_last_error()
    f = _lib.TtfbFitArgs()
    assert lib.tq_ttfb_fit(ctypes.byref(f), None) == 1
    buf = (ctypes.c_float * 9)()
    f = _lib.TtfbFitArgs(tau=ctypes.addressof(buf), state=ctypes.addressof(buf), S=1, N=1, n_steps=0, Tmax=10.0,
                         lr=5e-3, beta1=0.9, beta2=0.999, eps=1e-8)
    assert lib.tq_ttfb_fit(ctypes.byref(f), None) == 1  # n_steps < 1
    assert b"n_steps" in lib.tq_last_error()


def test_mle_entry_points_refuse_cpu_tensors():
    from tapqir_amd.exceptions import HipExtensionError
    from tapqir_amd.utils.mle_analysis import ttfb_fit, ttfb_sample

    with pytest.raises(HipExtensionError):
        ttfb_sample(torch.rand(3, 5), 10)
    with pytest.raises(HipExtensionError):
        ttfb_fit(torch.rand(3, 5), 5)


def test_fit_launches_chunks_of_max_1_int_chunk(monkeypatch):
    """The fits run their steps in launches of ``max(1, int(chunk))`` steps: ``chunk = 0`` and a float ``chunk`` behave as
    that integer.  The launches are recorded by a fake ``ttfb_fit_steps``; the fake ``dwell_fit_steps`` is driven through the
    chunk loop ``dwell_fit`` shares with ``ttfb_fit``."""
    from tapqir_amd.utils import mle_analysis as mle

    calls = []
    monkeypatch.setattr(mle, "_device_tensor", lambda x, what: x)
    monkeypatch.setattr(mle, "ttfb_fit_steps", lambda state, tau, Tmax, control, lr, step0, n_steps, loss, stage_lds:
                        calls.append((step0, n_steps)))
    for chunk, want in ((0, [(0, 1), (1, 1), (2, 1)]), (2.9, [(0, 2), (2, 1)]), (0.5, [(0, 1), (1, 1), (2, 1)]),
                        (3, [(0, 3)]), (10, [(0, 3)])):
        calls.clear()
        mle.ttfb_fit(torch.rand(2, 5), 5, n_steps=3, chunk=chunk)
        assert calls == want, (chunk, calls)
        assert all(type(n) is int for _, n in calls)

    def dwell_fit_steps(step0, n_steps):
        calls.append((step0, n_steps))

    for chunk, want in ((0, [(0, 1), (1, 1)]), (1.5, [(0, 1), (1, 1)]), (2.0, [(0, 2)])):
        calls.clear()
        mle._run_chunks(dwell_fit_steps, 2, chunk, None)
        assert calls == want, (chunk, calls)


def test_fraction_bound_counts():
    from tapqir_amd.utils.mle_analysis import fraction_bound, hpdi_columns

    data = torch.tensor([[0.0, 3.0, 5.0, 5.0], [1.0, 1.0, 2.0, 4.0]])
    fb = fraction_bound(data, 5)
    want = (data.unsqueeze(-1) < torch.arange(5)).float().mean(1)  # main.py:1073
    assert torch.equal(fb, want)
    x = torch.rand(200, 7, dtype=torch.float64)
    ll, ul = hpdi_columns(x, 0.95)
    from tapqir_amd.utils.stats import hpdi

    for j in range(7):
        a, b = hpdi(x[:, j], 0.95)
        assert ll[j] == a and ul[j] == b


@pytest.fixture
def fitted_path(tmp_path):
    save(simulate(2, 2, 5, 1, 14, params=dict(TEST_PARAMS)), tmp_path)
    return tmp_path


def ttfb_cmd(path, model="cosmos", device="--cuda"):
    return ["--cd", str(path), "ttfb", "--model", model, device, "--num-samples", "10", "--num-iter", "5", "--no-input"]


def test_ttfb_cpu_is_refused(fitted_path):
    result = runner.invoke(app, ttfb_cmd(fitted_path, device="--cpu"))
    assert result.exit_code == 1
    assert "GPU" in result.output


def test_ttfb_missing_files(tmp_path, fitted_path):
    result = runner.invoke(app, ttfb_cmd(tmp_path))  # no data.tpqr
    assert result.exit_code == 1
    result = runner.invoke(app, ttfb_cmd(fitted_path))  # data but no cosmos_params.tpqr
    assert result.exit_code == 1
    assert "parameter" in result.output


@pytest.mark.parametrize("model", ["crosstalk", "cosmos+hmm"])
def test_ttfb_unavailable_models(fitted_path, model):
    result = runner.invoke(app, ttfb_cmd(fitted_path, model=model))
    assert result.exit_code == 1
    assert "cosmos only" in result.output
