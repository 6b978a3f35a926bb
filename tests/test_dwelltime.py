"""Dwell-time analysis without a GPU: the host interval helpers against the reference's golden outputs, the g++ build of
tq_dwell.h (interval walker, sampler replay, per-pair terms and gradients against float64 autograd), the C layout of the
new argument structs, argument validation of the entry points, and the exits of the ``dwelltime`` command."""

import ctypes
import itertools
import os
import subprocess
import tempfile

import numpy as np
import pandas as pd
import pytest
import torch
from typer.testing import CliRunner

from dwell_fixture import COLUMNS, build_dwell_check, host_raster, host_sample, host_walk, loglik64
from tapqir_amd import _lib
from tapqir_amd.main import app
from tapqir_amd.utils.dataset import save
from tapqir_amd.utils.imscroll import INTERVAL_COLUMNS, bound_dwell_times, count_intervals, unbound_dwell_times
from tapqir_amd.utils.simulate import TEST_PARAMS, simulate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = np.load(os.path.join(ROOT, "tests", "golden", "dwell_golden.npz"))
CASES = sorted({k[: -len("_raster")] for k in GOLDEN.files if k.endswith("_raster")})
runner = CliRunner()


@pytest.fixture(scope="module")
def hk(tmp_path_factory):
    return build_dwell_check(tmp_path_factory.mktemp("dwell"))


def assert_table(table, name):
    assert list(table.columns) == COLUMNS == INTERVAL_COLUMNS
    for col in COLUMNS:
        got = table[col].to_numpy()
        assert got.dtype == np.int64, (name, col, got.dtype)
        np.testing.assert_array_equal(got, GOLDEN[f"{name}_{col}"], err_msg=f"{name} {col}")


# ---- host interval helpers against the reference -----------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("as_torch", [False, True])
def test_count_intervals_matches_the_reference(name, as_torch):
    z = GOLDEN[f"{name}_raster"]
    table = count_intervals(torch.from_numpy(z) if as_torch else z)
    assert_table(table, name)
    for kind, fn in (("bound", bound_dwell_times), ("unbound", unbound_dwell_times)):
        key = f"{name}_{kind}"
        got = fn(table)
        if key in GOLDEN.files:
            assert got.dtype == np.float32
            np.testing.assert_array_equal(got, GOLDEN[key])
        else:  # the reference fails on an empty selection; the port returns an empty array
            assert got.shape == (0, 0)


def test_golden_covers_the_edge_rows():
    z = GOLDEN["rand_raster"]
    assert (z[:, 0] == 0).all() and (z[:, 1] == 1).all()
    assert GOLDEN["f1_raster"].shape[-1] == 1 and GOLDEN["f2_raster"].shape[-1] == 2
    # the reference pads by sample index, so a sample without bound runs shifts the rows: the port keeps that
    assert GOLDEN["gap_bound"].shape[0] < GOLDEN["gap_raster"].shape[0]


# ---- g++ build of tq_dwell.h -------------------------------------------------------------------------------------
def test_low_or_high_codes(hk):
    for z, first, last in itertools.product((0, 1), (0, 1), (0, 1)):
        want = z + 2 if last else (-z - 2 if first else z)
        assert hk.hk_dwell_code(z, first, last) == want


@pytest.mark.parametrize("name", CASES)
def test_walker_gives_the_reference_table(hk, name):
    z = GOLDEN[f"{name}_raster"]
    table, counts, hb, hu = host_walk(hk, z)
    assert_table(table, name)
    S = z.shape[0]
    np.testing.assert_array_equal(counts.sum(1), np.bincount(GOLDEN[f"{name}_posterior_sample"], minlength=S))
    interior = table[table["low_or_high"].isin([0, 1])]
    for code, h in ((1, hb), (0, hu)):
        sel = interior[interior["low_or_high"] == code]
        want = np.zeros_like(h)
        np.add.at(want, (sel["posterior_sample"].to_numpy(), sel["dwell_time"].to_numpy()), 1)
        np.testing.assert_array_equal(h, want)


def test_sampler_replay_is_count_intervals_of_its_raster(hk):
    rng = np.random.default_rng(3)
    p = rng.random((11, 57)).astype(np.float32) ** 2
    p[0] = 0.0
    p[1] = 1.0
    p[2, ::2] = 1.0
    p[2, 1::2] = 0.0
    S, seed = 23, 987654321
    table, counts, hb, hu = host_sample(hk, p, S, seed)
    z = host_raster(hk, p, S, seed)
    want = count_intervals(z)
    pd.testing.assert_frame_equal(table, want.astype(np.int64))
    _, counts2, hb2, hu2 = host_walk(hk, z)
    np.testing.assert_array_equal(counts, counts2)
    np.testing.assert_array_equal(hb, hb2)
    np.testing.assert_array_equal(hu, hu2)
    assert (z[:, 0] == 0).all() and (z[:, 1] == 1).all() and (z[:, 2] == (np.arange(57) % 2 == 0)).all()
    assert 0.2 < z[:, 3:].mean() < 0.5  # the draws are not degenerate


@pytest.mark.parametrize("K", [1, 2, 3, 4])
def test_pair_terms_and_gradients_match_float64_autograd(hk, K):
    """Per pair (t, w): log-likelihood term and its gradient in (log k, a), for k from 1e-5 to 10, t up to 1e4 and A
    within 1e-6 of a simplex vertex."""
    ks = [1e-5, 1e-3, 0.1, 10.0]
    ts = [1.0, 3.0, 70.0, 1e4]
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
        assert hk.hk_dwell_pair(par32.data_ptr(), K, t, w, out) == 0
        got = np.array(out[:])
        par = par32.double().reshape(1, 2 * K).requires_grad_(True)
        ll = w * loglik64(par, torch.tensor([[t]], dtype=torch.float64), K)
        (g,) = torch.autograd.grad(ll.sum(), par)
        want = np.concatenate([[ll.item()], g[0].numpy()])
        err = np.abs(got - want) / np.maximum(np.abs(want), w)  # relative, floored at the pair's weight
        assert np.all(np.isfinite(got)), (k, A, t, got)
        assert err.max() < 2e-5, (k, A, t, w, got, want)
        if K == 1:
            assert got[2] == 0.0
        worst = max(worst, err.max())
    print(f"K={K}: worst relative error {worst:.2e}")


# ---- C ABI ----------------------------------------------------------------------------------------------------------
def test_dwell_struct_layout_matches_the_c_header():
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "tapqir_hip.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %d %d %d %d %d\n", sizeof(tq_dwell_sample_args),
         offsetof(tq_dwell_sample_args, total), offsetof(tq_dwell_sample_args, N), offsetof(tq_dwell_sample_args, mode),
         offsetof(tq_dwell_sample_args, seed), sizeof(tq_dwell_fit_args), offsetof(tq_dwell_fit_args, S),
         offsetof(tq_dwell_fit_args, stage_lds), offsetof(tq_dwell_fit_args, lr), offsetof(tq_dwell_fit_args, eps),
         TQ_DWELL_COUNT, TQ_DWELL_EMIT, TQ_DWELL_COLS, TQ_DWELL_KMAX, TQ_DWELL_LDS_PAIRS);
  return 0;
}'''
    with tempfile.TemporaryDirectory() as td:
        c = os.path.join(td, "s.c")
        open(c, "w").write(src)
        exe = os.path.join(td, "s")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        got = [int(v) for v in subprocess.check_output([exe]).split()]
    Sa, Fa = _lib.DwellSampleArgs, _lib.DwellFitArgs
    want = [ctypes.sizeof(Sa), Sa.total.offset, Sa.N.offset, Sa.mode.offset, Sa.seed.offset, ctypes.sizeof(Fa),
            Fa.S.offset, Fa.stage_lds.offset, Fa.lr.offset, Fa.eps.offset, _lib.DWELL_COUNT, _lib.DWELL_EMIT,
            _lib.DWELL_COLS, _lib.DWELL_KMAX, _lib.DWELL_LDS_PAIRS]
    assert got == want


def test_dwell_entry_points_validate_without_a_gpu():
    from tapqir_amd.build import build

    build(verbose=False)
    lib = _lib.load()
    buf = (ctypes.c_int64 * 64)()
    addr = ctypes.addressof(buf)
    assert lib.tq_dwell_sample(ctypes.byref(_lib.DwellSampleArgs()), None) == 1  # TQ_ERR_ARG
    assert b"NULL" in lib.tq_last_error()
    ok = dict(p=addr, counts=addr, hist_bound=addr, hist_unbound=addr, N=2, F=3, S=4, mode=_lib.DWELL_COUNT)
    for bad in (dict(counts=None), dict(hist_bound=None), dict(N=0), dict(F=0), dict(S=0), dict(mode=7),
                dict(mode=_lib.DWELL_EMIT), dict(mode=_lib.DWELL_EMIT, offsets=addr, total=-1)):
        a = _lib.DwellSampleArgs(**{**ok, **bad})
        assert lib.tq_dwell_sample(ctypes.byref(a), None) == 1, bad
    assert lib.tq_dwell_fit(ctypes.byref(_lib.DwellFitArgs()), None) == 1
    assert b"NULL" in lib.tq_last_error()
    ok = dict(values=addr, weights=addr, row_ptr=addr, state=addr, S=1, K=2, n_steps=1, lr=5e-3, beta1=0.9, beta2=0.999,
              eps=1e-8)
    for bad, word in ((dict(K=0), b"K"), (dict(K=9), b"K"), (dict(n_steps=0), b"n_steps"), (dict(S=0), b"S"),
                      (dict(values=None), b"NULL"), (dict(row_ptr=None), b"NULL"), (dict(step0=-1), b"step0")):
        a = _lib.DwellFitArgs(**{**ok, **bad})
        assert lib.tq_dwell_fit(ctypes.byref(a), None) == 1, bad
        assert word in lib.tq_last_error(), bad


def test_dwell_api_refuses_cpu_tensors():
    from tapqir_amd.exceptions import HipExtensionError
    from tapqir_amd.utils.mle_analysis import dwell_fit, dwell_intervals, dwell_sample

    with pytest.raises(HipExtensionError):
        dwell_sample(torch.rand(3, 5), 10)
    with pytest.raises(HipExtensionError):
        dwell_intervals(torch.rand(3, 5), 10)
    with pytest.raises(HipExtensionError):
        dwell_fit(torch.rand(3, 5) * 10, 2)
    with pytest.raises(HipExtensionError):
        dwell_fit((torch.ones(4), torch.ones(4), torch.tensor([0, 2, 4])), 2)
    with pytest.raises(ValueError):
        dwell_fit(torch.rand(3, 5), 9)


def test_dwell_init_state_is_the_reference_init():
    from tapqir_amd.utils.mle_analysis import dwell_init_state

    st = dwell_init_state(2, 3, "cpu")
    assert st.shape == (2, 18)
    torch.testing.assert_close(st[:, :3].exp(), torch.tensor([[0.01, 0.1, 1.0]] * 2))
    assert (st[:, 3:] == 0).all()  # softmax logits 0 (A = 1/3) and zero moments


# ---- command line -------------------------------------------------------------------------------------------------
@pytest.fixture
def fitted_path(tmp_path):
    save(simulate(2, 2, 5, 1, 14, params=dict(TEST_PARAMS)), tmp_path)
    return tmp_path


def dwell_cmd(path, model="cosmos", device="--cuda", K="2"):
    return ["--cd", str(path), "dwelltime", "--model", model, "-K", K, device, "--num-samples", "10", "--num-iter", "5",
            "--no-input"]


def test_dwelltime_cpu_is_refused(fitted_path):
    result = runner.invoke(app, dwell_cmd(fitted_path, device="--cpu"))
    assert result.exit_code == 1
    assert "GPU" in result.output


def test_dwelltime_missing_files(tmp_path, fitted_path):
    result = runner.invoke(app, dwell_cmd(tmp_path))  # no data.tpqr
    assert result.exit_code == 1
    result = runner.invoke(app, dwell_cmd(fitted_path))  # data but no cosmos_params.tpqr
    assert result.exit_code == 1
    assert "parameter" in result.output


@pytest.mark.parametrize("model", ["crosstalk", "cosmos+hmm"])
def test_dwelltime_unavailable_models(fitted_path, model):
    result = runner.invoke(app, dwell_cmd(fitted_path, model=model))
    assert result.exit_code == 1
    assert "cosmos only" in result.output


@pytest.mark.parametrize("K", ["0", "9", "-1"])
def test_dwelltime_K_out_of_range(fitted_path, K):
    result = runner.invoke(app, dwell_cmd(fitted_path, K=K))
    assert result.exit_code == 1
    assert "-K" in result.output
