"""`dwelltime --censored` without a GPU: the g++ build of tq_censored.h (the censored pair's term and gradient against
float64 autograd, the cancellation at the K = 1 closed form, the replay of one launch against the one-step rule, the
product-limit survival against numpy), the C layout of the three argument structs, argument validation of the entry
points, the host-side helpers, and the exits of the command."""

import ctypes
import itertools
import os
import subprocess
import tempfile

import numpy as np
import pytest
import torch
from typer.testing import CliRunner

import censored_fixture as cf
import kinetics_boundary_fixture as kb
from tapqir_amd import _lib, _lib_censored
from tapqir_amd.main import app
from tapqir_amd.utils.dataset import save
from tapqir_amd.utils.simulate import TEST_PARAMS, simulate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
runner = CliRunner()


@pytest.fixture(scope="module")
def hk(tmp_path_factory):
    return cf.build_censored_check(tmp_path_factory.mktemp("censored"))


# ---- g++ build of tq_censored.h -------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 2, 3, 4])
def test_censored_pair_terms_and_gradients_match_float64_autograd(hk, K):
    """Per censored pair (t, w): the term w log sum_j A_j exp(-k_j t) and its gradient in (log k, a), for k from 1e-5 to
    10, t from 0 to 1e4 and A within 1e-6 of a simplex vertex; the tolerance of
    test_dwelltime.test_pair_terms_and_gradients_match_float64_autograd."""
    ks = [1e-5, 1e-3, 0.1, 10.0]
    ts = [0.0, 1.0, 3.0, 70.0, 1e4]
    A_sets = [np.full(K, 1.0 / K)]
    if K > 1:
        vertex = np.full(K, 1e-6 / (K - 1))
        vertex[0] = 1 - 1e-6
        A_sets += [vertex, np.roll(vertex, K - 1)]
    worst = 0.0
    out = (ctypes.c_float * (1 + 2 * K))()
    for kk, A, t, w in itertools.product(itertools.product(ks, repeat=min(K, 2)), A_sets, ts, (1.0, 7.0)):
        k = np.resize(np.array(kk), K) * np.linspace(1.0, 1.5, K)
        par32 = torch.tensor(np.concatenate([np.log(k), np.log(A)]), dtype=torch.float32)
        assert hk.hk_censored_pair(par32.data_ptr(), K, t, w, out) == 0
        got = np.array(out[:])
        par = par32.double().reshape(1, 2 * K).requires_grad_(True)
        ll = w * cf.logsurv64(par, torch.tensor([[t]], dtype=torch.float64), K)
        (g,) = torch.autograd.grad(ll.sum(), par)
        want = np.concatenate([[ll.item()], g[0].numpy()])
        err = np.abs(got - want) / np.maximum(np.abs(want), w)  # relative, floored at the pair's weight
        assert np.all(np.isfinite(got)), (k, A, t, got)
        assert err.max() < 2e-5, (k, A, t, w, got, want)
        if K == 1:
            assert got[2] == 0.0
        worst = max(worst, err.max())
    print(f"K={K}: worst relative error {worst:.2e}")
    assert hk.hk_censored_pair(par32.data_ptr(), 9, 1.0, 1.0, out) == 1


def test_gradient_cancels_at_the_closed_form_of_one_exponential(hk):
    """K = 1 at log k = log(n / (sum w t + sum wc tc)): the two terms of d / d log k, n and k (RT + RTc), cancel, and what
    the replay of a launch leaves is within the one-step rule of its float64 value (itself only the rounding of log k)."""
    csr, ccsr = cf.censored_rows()
    S = len(cf.CENS_LENS)
    par0 = torch.zeros(S, 2)
    for s in range(S):
        (a, b), (ca, cb) = (int(csr[2][s]), int(csr[2][s + 1])), (int(ccsr[2][s]), int(ccsr[2][s + 1]))
        n = csr[1][a:b].double().sum()
        exposure = (csr[1][a:b].double() * csr[0][a:b].double()).sum() + (ccsr[1][ca:cb].double() * ccsr[0][ca:cb].double()).sum()
        if n > 0:
            par0[s, 0] = torch.log(n / exposure).float()
    before, ref = kb.dwell_state(par0), cf.reference_at(par0, csr, ccsr, 1)
    after, loss = cf.host_censored_steps(hk, before, csr, ccsr, 1)
    g, _ = kb.recover_gradient(after, 2)
    n_rows = torch.tensor([float(csr[1][int(csr[2][s]):int(csr[2][s + 1])].sum()) for s in range(S)], dtype=torch.float64)
    full = n_rows > 0
    # the closed form is the maximiser: the float64 gradient there is the rounding of log k times n, far below n
    assert (ref["g64"][full, 0].abs() <= 1e-6 * n_rows[full]).all(), ref["g64"][:, 0]
    excess = kb.rule_excess(g, ref["g32"], ref["g64"])
    print("closed form, K = 1: gradient error / bound per row", [f"{float(x):.3g}" for x in excess])
    assert (excess <= 1.0).all(), excess
    assert (kb.rule_excess(loss, ref["loss32"], ref["loss64"]) <= 1.0).all()
    assert (g[:, 1] == 0).all()


@pytest.mark.parametrize("kind", cf.CENS_STATES)
@pytest.mark.parametrize("K", range(1, 9))
def test_replay_of_one_step_is_within_the_rule(hk, K, kind):
    """The g++ replay of one launch on the rows of the device test: gradient, loss and update under the same rule."""
    csr, ccsr = cf.censored_rows()
    par0 = cf.censored_par0(K, kind)
    before, ref = kb.dwell_state(par0), cf.censored_reference(K, kind)
    after, loss = cf.host_censored_steps(hk, before, csr, ccsr, K)
    for key, (excess, row) in kb.worst(kb.step_report(before, after, loss, ref, 2 * K)).items():
        print(f"host censored K={K} {kind} {key}: worst excess {excess:.3g} (row {cf.CENS_LENS[row]})")
        assert excess <= 1.0, (key, excess, cf.CENS_LENS[row])
    assert torch.equal(after[0], before[0]) and loss[0] == 0  # the empty row


def test_replay_with_empty_censored_rows_is_the_replay_of_tq_dwell_fit(hk, tmp_path):
    import dwell_fixture

    dwell = dwell_fixture.build_dwell_check(tmp_path)
    kb.bind_fit_steps(dwell)
    csr = kb.dwell_rows()
    S = len(kb.DWELL_LENS)
    for K in (1, 3, 8):
        before = kb.dwell_state(kb.dwell_par0(K, "perturbed"))
        a, la = cf.host_censored_steps(hk, before, csr, cf.empty_csr(S), K, n_steps=5)
        b, lb = kb.host_dwell_steps(dwell, before, csr, K, n_steps=5)
        assert kb.same_bits(a, b) and kb.same_bits(la, lb), K


def test_survival_body_against_numpy(hk):
    rng = np.random.default_rng(5)
    R, F = 9, 131
    hist = rng.integers(0, 6, (R, F)).astype(np.int32) * (rng.random((R, F)) < 0.3)
    cens = rng.integers(0, 4, (R, F)).astype(np.int32) * (rng.random((R, F)) < 0.2)
    hist[0], cens[0] = 0, 0  # nothing: all ones
    cens[1] = 0  # Y = h at the last event: the curve drops to exactly 0
    hist[2] = 0  # censored only: all ones
    hist[3], cens[3] = 0, 0
    hist[3, F - 1] = 7  # events only in the last bin
    hist, cens = np.ascontiguousarray(hist, np.int32), np.ascontiguousarray(cens, np.int32)
    surv = np.full((R, F), np.nan)
    hk.hk_survival(hist.ctypes.data, cens.ctypes.data, R, F, surv.ctypes.data)
    want = cf.survival_numpy(hist, cens)
    assert np.all(surv[:, 0] == 1.0)
    assert np.all(surv[0] == 1.0) and np.all(surv[2] == 1.0)
    last = np.flatnonzero(hist[1, 1:])[-1] + 1
    assert np.all(surv[1, last:] == 0.0) and np.all(surv[1, :last] > 0.0)
    assert np.all(surv[3, : F - 1] == 1.0) and surv[3, F - 1] == 0.0
    assert np.all((want == 0.0) == (surv == 0.0)) and np.all((want == 1.0) == (surv == 1.0))
    rel = np.abs(surv - want) / np.where(want > 0, want, 1.0)
    print(f"survival body: worst relative error {rel.max():.3g} (bound {2 * F * 2.0 ** -52:.3g})")
    assert rel.max() <= 2 * F * 2.0 ** -52
    assert np.all(np.diff(surv, axis=1) <= 0)


# ---- C ABI ----------------------------------------------------------------------------------------------------------
def test_censored_struct_layout_matches_the_c_header():
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "tapqir_hip.h"
#define H tq_dwell_censored_hist_args
#define T tq_dwell_censored_fit_args
#define V tq_dwell_survival_args
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu ", sizeof(H), offsetof(H, intervals), offsetof(H, pop), offsetof(H, cens_bound),
         offsetof(H, cens_unbound), offsetof(H, total), offsetof(H, S));
  printf("%zu %zu %zu ", offsetof(H, N), offsetof(H, F), offsetof(H, G));
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu ", sizeof(T), offsetof(T, values), offsetof(T, weights), offsetof(T, row_ptr),
         offsetof(T, cvalues), offsetof(T, cweights), offsetof(T, crow_ptr), offsetof(T, state), offsetof(T, loss));
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu ", offsetof(T, S), offsetof(T, K), offsetof(T, step0), offsetof(T, n_steps),
         offsetof(T, stage_lds), offsetof(T, lr), offsetof(T, beta1), offsetof(T, beta2), offsetof(T, eps));
  printf("%zu %zu %zu %zu %zu %zu %d\n", sizeof(V), offsetof(V, hist), offsetof(V, cens), offsetof(V, surv), offsetof(V, R),
         offsetof(V, F), TQ_SMOOTH_MAX_F);
  return 0;
}'''
    with tempfile.TemporaryDirectory() as td:
        c = os.path.join(td, "s.c")
        open(c, "w").write(src)
        exe = os.path.join(td, "s")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        got = [int(v) for v in subprocess.check_output([exe]).split()]
    H, T, V = _lib_censored.DwellCensoredHistArgs, _lib_censored.DwellCensoredFitArgs, _lib_censored.DwellSurvivalArgs
    want = [ctypes.sizeof(H)] + [getattr(H, f).offset for f, _ in H._fields_]
    want += [ctypes.sizeof(T)] + [getattr(T, f).offset for f, _ in T._fields_]
    want += [ctypes.sizeof(V)] + [getattr(V, f).offset for f, _ in V._fields_] + [_lib_censored.SURVIVAL_MAX_F]
    assert got == want
    assert [f for f, _ in H._fields_] == ["intervals", "pop", "cens_bound", "cens_unbound", "total", "S", "N", "F", "G"]
    assert [f for f, _ in V._fields_] == ["hist", "cens", "surv", "R", "F"]


def test_censored_entry_points_validate_without_a_gpu():
    from tapqir_amd.build import build

    build(verbose=False)
    lib = _lib_censored.lib()
    buf = (ctypes.c_int64 * 64)()
    addr = ctypes.addressof(buf)
    H, T, V = _lib_censored.DwellCensoredHistArgs, _lib_censored.DwellCensoredFitArgs, _lib_censored.DwellSurvivalArgs

    assert lib.tq_dwell_censored_hist(ctypes.byref(H()), None) == 1  # TQ_ERR_ARG
    assert b"NULL" in lib.tq_last_error()
    ok = dict(intervals=addr, cens_bound=addr, cens_unbound=addr, total=5, S=2, N=3, F=4, G=1)
    for bad, word in ((dict(intervals=None), b"NULL"), (dict(cens_bound=None), b"NULL"), (dict(cens_unbound=None), b"NULL"),
                      (dict(S=0), b"S"), (dict(N=0), b"N"), (dict(F=-1), b"F"), (dict(total=-1), b"total"),
                      (dict(G=0), b"G"), (dict(G=5, pop=addr), b"G"), (dict(G=2), b"pop")):
        assert lib.tq_dwell_censored_hist(ctypes.byref(H(**{**ok, **bad})), None) == 1, bad
        assert word in lib.tq_last_error(), bad
    # an empty table is done before anything touches the device, with or without a table pointer
    assert lib.tq_dwell_censored_hist(ctypes.byref(H(**{**ok, "total": 0})), None) == 0
    assert lib.tq_dwell_censored_hist(ctypes.byref(H(**{**ok, "total": 0, "intervals": None})), None) == 0

    assert lib.tq_dwell_censored_fit(ctypes.byref(T()), None) == 1
    assert b"NULL" in lib.tq_last_error()
    ok = dict(values=addr, weights=addr, row_ptr=addr, cvalues=addr, cweights=addr, crow_ptr=addr, state=addr, S=1, K=2,
              n_steps=1, lr=5e-3, beta1=0.9, beta2=0.999, eps=1e-8)
    for bad, word in ((dict(K=0), b"K"), (dict(K=9), b"K"), (dict(n_steps=0), b"n_steps"), (dict(S=0), b"S"),
                      (dict(values=None), b"NULL"), (dict(cvalues=None), b"NULL"), (dict(cweights=None), b"NULL"),
                      (dict(crow_ptr=None), b"NULL"), (dict(state=None), b"NULL"), (dict(step0=-1), b"step0"),
                      (dict(lr=0.0), b"Adam"), (dict(beta2=1.0), b"Adam")):
        assert lib.tq_dwell_censored_fit(ctypes.byref(T(**{**ok, **bad})), None) == 1, bad
        assert word in lib.tq_last_error(), bad

    assert lib.tq_dwell_survival(ctypes.byref(V()), None) == 1
    assert b"NULL" in lib.tq_last_error()
    ok = dict(hist=addr, cens=addr, surv=addr, R=1, F=8)
    for bad, word in ((dict(hist=None), b"NULL"), (dict(cens=None), b"NULL"), (dict(surv=None), b"NULL"), (dict(R=0), b"R"),
                      (dict(F=0), b"F"), (dict(F=_lib_censored.SURVIVAL_MAX_F + 1), b"F")):
        assert lib.tq_dwell_survival(ctypes.byref(V(**{**ok, **bad})), None) == 1, bad
        assert word in lib.tq_last_error(), bad


def test_the_three_symbols_are_exported():
    assert {"tq_dwell_censored_hist", "tq_dwell_censored_fit", "tq_dwell_survival"} <= set(_lib.EXPORTS)
    lib = _lib_censored.lib()
    for name in ("tq_dwell_censored_hist", "tq_dwell_censored_fit", "tq_dwell_survival"):
        assert getattr(lib, name).restype is ctypes.c_int


# ---- host functions -----------------------------------------------------------------------------------------------------
def test_censored_api_refuses_cpu_tensors():
    from tapqir_amd.exceptions import HipExtensionError
    from tapqir_amd.utils.censored_analysis import (dwell_censored_fit, dwell_censored_fit_steps, dwell_censored_hist,
                                                    dwell_survival)

    csr = (torch.ones(4), torch.ones(4), torch.tensor([0, 2, 4]))
    with pytest.raises(HipExtensionError):
        dwell_censored_hist(torch.zeros(7, 5, dtype=torch.int32), 2, 3, 4)
    with pytest.raises(HipExtensionError):
        dwell_censored_fit(csr, csr, 2)
    with pytest.raises(HipExtensionError):
        dwell_censored_fit_steps(torch.zeros(2, 12), csr, csr, 2)
    with pytest.raises(HipExtensionError):
        dwell_survival(torch.zeros(2, 5, dtype=torch.int32), torch.zeros(2, 5, dtype=torch.int32))
    with pytest.raises(ValueError):
        dwell_censored_fit(csr, csr, 9)


def test_csr_from_censored_hist_drops_bin_one_and_shifts_by_one():
    from tapqir_amd.utils.censored_analysis import dwell_csr_from_censored_hist

    cens = torch.tensor([[9, 4, 0, 2, 0, 1], [0, 7, 0, 0, 0, 0], [0, 0, 3, 0, 0, 0]], dtype=torch.int32)
    values, weights, row_ptr = dwell_csr_from_censored_hist(cens)
    assert row_ptr.tolist() == [0, 2, 2, 3] and row_ptr.dtype == torch.int64
    assert values.tolist() == [2.0, 4.0, 1.0] and values.dtype == torch.float32  # bins 3, 5 and 2
    assert weights.tolist() == [2.0, 1.0, 3.0]
    # nothing at all: valid pointers, empty rows
    values, weights, row_ptr = dwell_csr_from_censored_hist(torch.zeros(2, 4, dtype=torch.int32))
    assert row_ptr.tolist() == [0, 0, 0] and values.numel() == 1 and weights.numel() == 1


def test_closed_form_rate_and_fitted_survival():
    from tapqir_amd.utils.censored_analysis import dwell_censored_rate, mixture_survival

    hist = torch.tensor([[0, 2, 0, 1, 0], [0, 0, 0, 0, 0]])  # d = 1, 1, 3
    cens = torch.tensor([[0, 5, 1, 0, 2], [0, 0, 4, 0, 0]])  # open runs of 2 and 4, 4 frames (bin 1 carries nothing)
    k_int, k_cens = dwell_censored_rate(hist), dwell_censored_rate(hist, cens)
    assert k_int[0].item() == pytest.approx(3 / 5) and k_cens[0].item() == pytest.approx(3 / (5 + 1 + 3 + 3))
    assert torch.isnan(k_int[1]) and torch.isnan(k_cens[1])
    z = cf.two_state_raster(1, N=40)
    h, c = cf.raster_histograms(z)
    want = cf.closed_form_rates(h, c)
    assert dwell_censored_rate(torch.from_numpy(h)).item() == pytest.approx(want[0], rel=1e-12)
    assert dwell_censored_rate(torch.from_numpy(h), torch.from_numpy(c)).item() == pytest.approx(want[1], rel=1e-12)
    s = mixture_survival([0.25, 0.75], [0.1, 0.01], torch.arange(3))
    assert s.tolist() == pytest.approx([1.0, 0.25 * np.exp(-0.1) + 0.75 * np.exp(-0.01), 0.25 * np.exp(-0.2) + 0.75 * np.exp(-0.02)])


def test_chain_seed_satisfies_the_conditions_on_the_generating_raster():
    """The seed of the device test was chosen here: the raster alone, by the definitions in numpy, lies inside the bands."""
    h, c = cf.raster_histograms(cf.two_state_raster(cf.CHAIN_SEED))
    ok, fig = cf.chain_conditions(h, c, cf.survival_numpy(h[None], c[None])[0, 50])
    print(fig)
    assert ok, fig


# ---- command line -------------------------------------------------------------------------------------------------
@pytest.fixture
def fitted_path(tmp_path):
    save(simulate(2, 2, 5, 1, 14, params=dict(TEST_PARAMS)), tmp_path)
    return tmp_path


def dwell_cmd(path, *more, model="cosmos", device="--cuda"):
    return ["--cd", str(path), "dwelltime", "--model", model, "-K", "1", device, "--num-samples", "10", "--num-iter", "5",
            "--censored", "--no-input", *more]


def test_dwelltime_censored_cpu_is_refused(fitted_path):
    result = runner.invoke(app, dwell_cmd(fitted_path, device="--cpu"))
    assert result.exit_code == 1
    assert "GPU" in result.output


@pytest.mark.parametrize("model", ["crosstalk", "cosmos+hmm"])
def test_dwelltime_censored_unavailable_models(fitted_path, model):
    result = runner.invoke(app, dwell_cmd(fitted_path, model=model))
    assert result.exit_code == 1
    assert "cosmos only" in result.output


def test_dwelltime_help_names_the_switch(tmp_path):
    result = runner.invoke(app, ["--cd", str(tmp_path), "dwelltime", "--help"])
    assert result.exit_code == 0 and "--censored" in result.output
