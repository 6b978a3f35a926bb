"""Two-state rates without a GPU: the g++ build of tq_rates.h (row counter, index draw) against a numpy oracle on the
rasters of the dwell-time fixture, the ``imscroll`` rate and resampling functions, the C layout of the two new argument
structs, argument validation of the entry points, and the exit of ``rates --cpu``."""

import ctypes
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest
import torch
from typer.testing import CliRunner

from dwell_fixture import build_dwell_check, host_raster
from rates_fixture import (build_rates_check, host_count, host_indices, host_sample, oracle_counts, oracle_estimands)
from tapqir_amd import _lib, _lib_rates
from tapqir_amd.main import app
from tapqir_amd.utils import imscroll
from tapqir_amd.utils.dataset import save
from tapqir_amd.utils.simulate import TEST_PARAMS, simulate
from tapqir_amd.utils.stats import quantile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def hk(tmp_path_factory):
    return build_rates_check(tmp_path_factory.mktemp("rates"))


@pytest.fixture(scope="module")
def dwell_hk(tmp_path_factory):
    return build_dwell_check(tmp_path_factory.mktemp("rates_dwell"))


# ---- g++ counter ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [1, 2, 3, 64, 65, 130])
def test_row_counter_equals_the_numpy_oracle(hk, dwell_hk, F):
    """S = 5, N = 9 with a row of exact 0s, one of exact 1s and an alternating 0/1 row: bit-exact integers, for the counter
    on the given raster and for its replay of the sampler's draws."""
    S, N, seed = 5, 9, 77 + F
    gen = torch.Generator().manual_seed(F)
    p = torch.rand(N, F, generator=gen).numpy()
    p[0] = 0.0
    p[1] = 1.0
    p[2] = np.arange(F) % 2
    z = host_raster(dwell_hk, p, S, seed)
    assert (z[:, 0] == 0).all() and (z[:, 1] == 1).all() and (z[:, 2] == np.arange(F) % 2).all()
    want = oracle_counts(z)
    assert want.shape == (S, N, 4)
    assert np.array_equal(host_count(hk, z), want)
    assert np.array_equal(host_sample(hk, p, S, seed), want)
    assert (want[..., 1] + want[..., 3] == F - 1).all()
    if F == 1:
        assert not want.any()


def test_quotients_are_double_divisions(hk):
    totals = np.array([[3, 7, 2, 9], [0, 0, 5, 0], [1, 3, 0, 4]], np.int64)
    kon, koff = oracle_estimands(totals)
    for row, a, b in zip(totals, kon, koff):
        out = np.zeros(2)
        hk.hk_rates_quotients(np.ascontiguousarray(row).ctypes.data, out.ctypes.data)
        assert np.array_equal(out, [a, b], equal_nan=True)
    assert np.isnan(kon[1]) and np.isinf(koff[1])


# ---- index draw -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 2, 37, 65535])
def test_index_is_below_N(hk, N):
    idx = host_indices(hk, 5, 3, N)
    assert idx.min() >= 0 and idx.max() < N
    assert hk.hk_rates_index(5, 2, N - 1, N) == idx[2, N - 1]
    if N > 1:
        assert len(np.unique(idx)) > 1


def test_index_histogram_is_uniform(hk):
    """10^5 draws at N = 8: chi^2 against the uniform law below 40, the 1 - 10^-6 quantile of chi^2 with 7 degrees."""
    idx = host_indices(hk, 2026, 12500, 8).reshape(-1)
    obs = np.bincount(idx, minlength=8)
    assert obs.sum() == 100000 and len(obs) == 8
    chi2 = ((obs - 12500.0) ** 2 / 12500.0).sum()
    print(f"chi2 = {chi2:.2f}")
    assert chi2 < 40.0, (chi2, obs)


def test_index_streams_differ_by_seed_and_sample(hk):
    a, b = host_indices(hk, 1, 2, 50), host_indices(hk, 2, 2, 50)
    assert not np.array_equal(a, b) and not np.array_equal(a[0], a[1])
    assert np.array_equal(a, host_indices(hk, 1, 2, 50))


# ---- imscroll: rates --------------------------------------------------------------------------------------------------
def loop_rates(z):
    """kon, koff of every leading index of a (B, N, F) raster by the explicit double loop, in float64."""
    kon, koff = [], []
    for zb in z:
        n01 = n0 = n10 = n1 = 0
        for row in zb:
            for f in range(len(row) - 1):
                n0 += row[f] == 0
                n1 += row[f] == 1
                n01 += row[f] == 0 and row[f + 1] == 1
                n10 += row[f] == 1 and row[f + 1] == 0
        kon.append(n01 / n0)
        koff.append(n10 / n1)
    return np.array(kon), np.array(koff)


def test_rates_equal_the_double_loop():
    z = (np.random.default_rng(3).random((3, 4, 17)) < 0.4).astype(np.int64)
    kon, koff = loop_rates(z)
    assert np.array_equal(imscroll.association_rate(z), kon)
    assert np.array_equal(imscroll.dissociation_rate(z), koff)
    assert imscroll.association_rate(z[0]) == kon[0] and imscroll.dissociation_rate(z[0]) == koff[0]
    # torch divides in float32, as the reference does
    t_kon, t_koff = imscroll.association_rate(torch.from_numpy(z)), imscroll.dissociation_rate(torch.from_numpy(z))
    assert t_kon.dtype == torch.float32 and t_kon.shape == (3,)
    assert np.abs(t_kon.double().numpy() - kon).max() < 1e-6
    assert np.abs(t_koff.double().numpy() - koff).max() < 1e-6
    with pytest.raises(NotImplementedError):
        imscroll.association_rate([0, 1])
    with pytest.raises(NotImplementedError):
        imscroll.dissociation_rate([0, 1])


# ---- imscroll: resampling ---------------------------------------------------------------------------------------------
class Recorder:
    """An estimator that records what it is given and returns its mean."""

    def __init__(self):
        self.seen = []

    def __call__(self, values):
        values = torch.as_tensor(values).double()
        self.seen.append(values)
        return values.mean()


def pair_of(rec, probs):
    est = torch.stack([v.mean() for v in rec.seen]).float()  # the estimands are kept in float32, as the reference does
    return float(quantile(est, (1 - probs) / 2)), float(quantile(est, (1 + probs) / 2))


@pytest.mark.parametrize("kind", ["numpy", "torch"])
def test_bootstrap_returns_the_quantile_pair(kind):
    values = np.arange(1.0, 12.0)
    samples = values if kind == "numpy" else torch.from_numpy(values)
    rec = Recorder()
    np.random.seed(0)
    torch.manual_seed(0)
    ll, ul = imscroll.bootstrap(samples, rec, repetitions=37, probs=0.8)
    assert len(rec.seen) == 37
    assert all(len(v) == len(values) and np.isin(v.numpy(), values).all() for v in rec.seen)
    assert len({tuple(v.tolist()) for v in rec.seen}) > 1
    if kind == "numpy":  # float64 estimands
        est = torch.stack([v.mean() for v in rec.seen])
        want = float(quantile(est, 0.1)), float(quantile(est, 0.9))
    else:
        want = pair_of(rec, 0.8)
    assert (float(ll), float(ul)) == pytest.approx(want, rel=1e-12)
    # a constant input: a zero-width interval at that constant
    const = np.full(9, 2.5) if kind == "numpy" else torch.full((9,), 2.5)
    ll, ul = imscroll.bootstrap(const, Recorder(), repetitions=11)
    assert float(ll) == 2.5 and float(ul) == 2.5
    with pytest.raises(NotImplementedError):
        imscroll.bootstrap([1.0, 2.0], Recorder())


def test_posterior_estimate_returns_the_quantile_pair():
    torch.manual_seed(1)
    dist = torch.distributions.Bernoulli(torch.full((6, 20), 0.3))
    rec = Recorder()
    ll, ul = imscroll.posterior_estimate(dist, rec, repetitions=23, probs=0.68)
    assert len(rec.seen) == 23
    assert all(v.shape == (6, 20) and np.isin(v.numpy(), [0.0, 1.0]).all() for v in rec.seen)
    est = torch.stack([v.mean() for v in rec.seen]).float()
    assert (float(ll), float(ul)) == pytest.approx((float(quantile(est, 0.16)), float(quantile(est, 0.84))), rel=1e-12)
    # with a rate estimator: the interval brackets the frame-to-frame binding probability of independent frames, p
    ll, ul = imscroll.posterior_estimate(torch.distributions.Bernoulli(torch.full((40, 200), 0.3)),
                                         imscroll.association_rate, repetitions=30, probs=0.999)
    assert ll < 0.3 < ul
    const = torch.distributions.Bernoulli(torch.ones(5))
    ll, ul = imscroll.posterior_estimate(const, Recorder(), repetitions=7)
    assert float(ll) == 1.0 and float(ul) == 1.0
    with pytest.raises(NotImplementedError):
        imscroll.posterior_estimate(torch.ones(3), Recorder())


def test_sample_and_bootstrap_returns_the_quantile_pair():
    torch.manual_seed(2)
    np.random.seed(2)
    dist = torch.distributions.Normal(torch.arange(8.0), 1.0)
    rec, pre = Recorder(), []

    def preprocess(x):
        pre.append(x.clone())
        return x * 2

    ll, ul = imscroll.sample_and_bootstrap(dist, rec, preprocess=preprocess, repetitions=19, probs=0.5)
    assert len(rec.seen) == 19 and len(pre) == 19
    for drawn, given in zip(pre, rec.seen):  # every resample is drawn from that round's (preprocessed) draw
        assert given.shape == (8,) and np.isin(given.numpy(), (drawn * 2).double().numpy()).all()
    est = torch.stack([v.mean() for v in rec.seen]).float()
    assert (float(ll), float(ul)) == pytest.approx((float(quantile(est, 0.25)), float(quantile(est, 0.75))), rel=1e-12)
    const = torch.distributions.Bernoulli(torch.zeros(5))
    ll, ul = imscroll.sample_and_bootstrap(const, Recorder(), repetitions=7)
    assert float(ll) == 0.0 and float(ul) == 0.0
    with pytest.raises(NotImplementedError):
        imscroll.sample_and_bootstrap(torch.ones(3), Recorder())


# ---- ABI ------------------------------------------------------------------------------------------------------------
def header_fields(name):
    """Field names of ``typedef struct { ... } name;`` in include/tapqir_hip.h, in order."""
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tapqir_hip.h")).read(), flags=re.S)
    body = re.search(r"typedef struct \{([^{}]*)\}\s*%s;" % name, text).group(1)
    out = []
    for decl in body.split(";"):
        if decl.strip():  # "const float* p" | "int32_t N, F, S": the declarators' identifiers
            out += [re.search(r"(\w+)\s*$", d.strip()).group(1) for d in decl.split(",")]
    return out


MIRRORS = {"tq_rates_count_args": _lib_rates.RatesCountArgs, "tq_rates_estimate_args": _lib_rates.RatesEstimateArgs}


def test_struct_layouts_match_the_c_header():
    """sizeof and every offsetof of the two mirrors equal the C compiler's, and the mirrors name the header's fields in
    order (the method of test_abi.py: gcc on a generated program)."""
    lines, want = [], []
    for cname, cls in sorted(MIRRORS.items()):
        assert cname in cls.__doc__
        names = [f[0] for f in cls._fields_]
        assert names == header_fields(cname), cname
        lines.append('  printf("%%zu\\n", sizeof(%s));' % cname)
        want.append((cname, "sizeof", ctypes.sizeof(cls)))
        for f in names:
            lines.append('  printf("%%zu\\n", offsetof(%s, %s));' % (cname, f))
            want.append((cname, f, getattr(cls, f).offset))
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "tapqir_hip.h"\nint main(void) {\n' + "\n".join(lines)
           + '\n  printf("%d\\n", TQ_RATES_COLS);\n  return 0;\n}\n')
    with tempfile.TemporaryDirectory() as td:
        c = os.path.join(td, "s.c")
        open(c, "w").write(src)
        exe = os.path.join(td, "s")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        got = [int(v) for v in subprocess.check_output([exe]).split()]
    assert got.pop() == _lib_rates.RATES_COLS == 4
    assert len(got) == len(want)
    assert [(n, f, g) for (n, f, _), g in zip(want, got)] == want


def test_the_binding_keeps_its_mirrors_out_of_lib():
    assert {"tq_rates_count", "tq_rates_estimate"} <= set(_lib.EXPORTS)
    assert not any(isinstance(v, type) and issubclass(v, ctypes.Structure) and v.__module__ == _lib_rates.__name__
                   for v in vars(_lib).values())


def test_argument_validation_returns_error_codes_without_a_gpu():
    lib = _lib_rates.lib()
    a = _lib_rates.RatesCountArgs()
    assert lib.tq_rates_count(ctypes.byref(a), None) == 1  # TQ_ERR_ARG
    assert b"tq_rates_count" in lib.tq_last_error() and b"NULL" in lib.tq_last_error()
    e = _lib_rates.RatesEstimateArgs()
    assert lib.tq_rates_estimate(ctypes.byref(e), None) == 1
    assert b"tq_rates_estimate" in lib.tq_last_error() and b"NULL" in lib.tq_last_error()
    assert lib.tq_rates_count(None, None) == 1 and lib.tq_rates_estimate(None, None) == 1
    # pointers given, sizes zero or out of range: still refused before any launch
    buf = (ctypes.c_int64 * 8)()
    addr = ctypes.addressof(buf) & ~15
    a = _lib_rates.RatesCountArgs(p=addr, counts=addr, N=3, F=0, S=2)
    assert lib.tq_rates_count(ctypes.byref(a), None) == 1 and b"positive" in lib.tq_last_error()
    a = _lib_rates.RatesCountArgs(p=addr, counts=addr + 4, N=3, F=5, S=2)
    assert lib.tq_rates_count(ctypes.byref(a), None) == 1 and b"aligned" in lib.tq_last_error()
    a = _lib_rates.RatesCountArgs(p=addr, counts=addr, N=3, F=5, S=65535 * 64 + 1)
    assert lib.tq_rates_count(ctypes.byref(a), None) == 1 and b"S too large" in lib.tq_last_error()
    e = _lib_rates.RatesEstimateArgs(counts=addr, totals=addr, estimand=addr, N=3, S=2, resample=2)
    assert lib.tq_rates_estimate(ctypes.byref(e), None) == 1 and b"resample" in lib.tq_last_error()


def test_device_entry_points_refuse_host_tensors():
    from tapqir_amd.exceptions import HipExtensionError
    from tapqir_amd.utils.mle_analysis import rates_estimate, rates_sample, rates_summary

    with pytest.raises(HipExtensionError):
        rates_sample(torch.rand(3, 5), 4)
    with pytest.raises(HipExtensionError):
        rates_estimate(torch.zeros(4, 3, 4, dtype=torch.int32))
    # the summary is host arithmetic on whatever device the estimands are on: finite-only mean and interval
    est = {"kon": torch.tensor([0.1, float("nan"), 0.3, float("inf")], dtype=torch.float64),
           "koff": torch.full((4,), float("nan"), dtype=torch.float64)}
    got = rates_summary(est, 0.5)
    assert got["kon"]["left_out"] == 2 and got["kon"]["mean"] == pytest.approx(0.2)
    assert (got["kon"]["ll"], got["kon"]["ul"]) == pytest.approx((0.15, 0.25))
    assert got["koff"]["left_out"] == 4 and all(np.isnan(got["koff"][k]) for k in ("mean", "ll", "ul"))


# ---- command line -----------------------------------------------------------------------------------------------------
def test_rates_cpu_is_refused(tmp_path):
    save(simulate(2, 2, 5, 1, 14, params=dict(TEST_PARAMS)), tmp_path)
    result = CliRunner().invoke(app, ["--cd", str(tmp_path), "rates", "--cpu", "--num-samples", "10", "--no-input"])
    assert result.exit_code == 1, result.output  # 2 = no such command
    assert "GPU" in result.output
