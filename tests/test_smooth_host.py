"""Hidden-Markov smoothing without a GPU: the g++ build of tq_smooth.h (the E-step with the device's lane ownership and
scan order, the M-step, the EM, Viterbi, the backward sampler) against the numpy oracle of smooth_fixture by the
tolerance rule of DESIGN.md section 20, the C layout of the four argument structs, argument validation of the entry
points, and the exits of ``smooth --cpu`` and ``smooth --model crosstalk``."""

import ctypes
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest
import torch
from typer.testing import CliRunner

from rates_fixture import oracle_counts
from smooth_fixture import (F_LIST, RMIN, build_smooth_check, host_count, host_em, host_estep, host_mstep, host_viterbi,
                            oracle_em, oracle_estep, oracle_mstep, oracle_viterbi, path_logprob, realised_rates, rule_excess,
                            synthetic_chain, with_special_rows)
from tapqir_amd import _lib, _lib_smooth
from tapqir_amd.main import app
from tapqir_amd.utils.dataset import save
from tapqir_amd.utils.simulate import TEST_PARAMS, simulate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRIOR = 1.0 / 3.0
THETA = (0.05, 0.10, 0.4)


@pytest.fixture(scope="module")
def hk(tmp_path_factory):
    return build_smooth_check(tmp_path_factory.mktemp("smooth"))


def check_rule(got, o64, o80, who):
    """filt, gamma and every column group of rows (expected counts, loglik, gamma_0) by the rule; prints each excess."""
    for key in ("filt", "gamma"):
        exc = rule_excess(got[key], o64[key], o80[key])
        print(f"{who} {key}: {exc:.3g} of the bound")
        assert exc <= 1.0, (who, key, exc)
    for name, cols in (("counts", slice(0, 4)), ("loglik", slice(4, 5)), ("gamma0", slice(5, 6))):
        exc = rule_excess(got["rows"][:, cols], o64["rows"][:, cols], o80["rows"][:, cols])
        print(f"{who} rows/{name}: {exc:.3g} of the bound")
        assert exc <= 1.0, (who, name, exc)


# ---- E-step -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", F_LIST + [5000])
def test_estep_equals_the_oracle(hk, F):
    """N = 6: rows of all 0, all 1, alternating 0 / 1 and p = prior, and two rows of the synthetic chain."""
    p = with_special_rows(synthetic_chain(6, F, seed=F)[0], PRIOR)
    o64, o80 = oracle_estep(p, THETA, PRIOR), oracle_estep(p, THETA, PRIOR, np.longdouble)
    got = host_estep(hk, p, THETA, PRIOR)
    check_rule(got, o64, o80, f"F = {F}")
    rows = got["rows"]
    assert np.allclose(rows[:, 1] + rows[:, 3], F - 1, rtol=0, atol=1e-9 * F)
    assert (rows[:, 0] <= rows[:, 1] + 1e-12).all() and (rows[:, 2] <= rows[:, 3] + 1e-12).all()
    if F == 1:
        assert not rows[:, :4].any()
        assert np.abs(got["filt"] - got["gamma"]).max() < 4e-16  # a_0 renormalised once more


@pytest.mark.parametrize("F", [1, 65, 5000])
def test_uninformative_row_has_closed_forms(hk, F):
    """p = prior (as the float32 the kernel reads): l = (1, 1), so loglik = 0 and gamma_f = filt_f = (rho A^f)(1)."""
    prior = float(np.float32(PRIOR))
    p = np.full((1, F), prior, np.float32)
    got = host_estep(hk, p, THETA, prior)
    kon, koff, pi0 = (np.longdouble(v) for v in THETA)
    stationary = kon / (kon + koff)  # (rho A^f)(1) = stationary + (pi0 - stationary) (1 - kon - koff)^f
    want = stationary + (pi0 - stationary) * (1 - kon - koff) ** np.arange(F, dtype=np.longdouble)
    o64, o80 = oracle_estep(p, THETA, prior), oracle_estep(p, THETA, prior, np.longdouble)
    assert np.abs(o80["gamma"][0] - want).max() < 1e-15
    for key in ("gamma", "filt"):
        exc = rule_excess(got[key][0], o64[key][0], want)
        print(f"F = {F} {key} against the closed form: {exc:.3g} of the bound")
        assert exc <= 1.0
    exc = rule_excess(got["rows"][:, 4], o64["rows"][:, 4], np.zeros(1, np.longdouble))
    print(f"F = {F} loglik = {got['rows'][0, 4]:.3g}: {exc:.3g} of the bound")
    assert exc <= 1.0


# ---- M-step -----------------------------------------------------------------------------------------------------------
def test_mstep_quotients_clamps_and_zero_over_zero(hk):
    rng = np.random.default_rng(1)
    rows = rng.random((300, 6))  # more rows than the 256 threads of the device's workgroup
    rows[:, 1] += rows[:, 0]
    rows[:, 3] += rows[:, 2]
    theta, ll, sums = host_mstep(hk, rows, THETA)
    want, want_ll = oracle_mstep(rows, THETA, np.longdouble)
    for got, o64, o80 in ((theta, oracle_mstep(rows, THETA)[0], want), ([ll], [oracle_mstep(rows, THETA)[1]], [want_ll]),
                          (sums, rows.sum(0), rows.astype(np.longdouble).sum(0))):
        assert rule_excess(got, o64, o80) <= 1.0
    assert np.array_equal(host_mstep(hk, rows, THETA)[0], theta)

    def from_sums(sums, N=10, old=(0.3, 0.6, 0.2)):
        theta = np.array(old, np.float64)
        hk.hk_smooth_mstep_theta(np.array(sums, np.float64).ctypes.data, N, theta.ctypes.data)
        return theta

    assert np.array_equal(from_sums([1, 4, 3, 6, -7.0, 5]), [0.25, 0.5, 0.5])
    assert np.array_equal(from_sums([0, 0, 3, 6, 0, 5]), [0.3, 0.5, 0.5])  # 0 / 0 keeps kon
    assert np.array_equal(from_sums([1, 4, 0, 0, 0, 5]), [0.25, 0.6, 0.5])  # ... and koff
    assert np.array_equal(from_sums([0, 4, 6, 6, 0, 0]), [RMIN, 1 - RMIN, RMIN])
    assert np.array_equal(from_sums([4, 4, 0, 6, 0, 10]), [1 - RMIN, RMIN, 1 - RMIN])


# ---- EM ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def em_case():
    """N = 40, F = 500, seed 0, with the oracle's EM of 25 iterations in both precisions; shared and left unchanged."""
    p, z = synthetic_chain(40, 500, seed=0)
    start = (0.5, 0.5, 0.5)
    th64, tr64 = oracle_em(p, PRIOR, start, 25)
    th80, tr80 = oracle_em(p, PRIOR, start, 25, np.longdouble)
    return {"p": p, "z": z, "start": start, "th64": th64, "tr64": tr64, "th80": th80, "tr80": tr80}


def test_em_follows_the_oracle_and_recovers_the_rates(hk, em_case):
    p, z = em_case["p"], em_case["z"]
    thetas, trace = host_em(hk, p, PRIOR, em_case["start"], 25)
    for it in (1, 2, 25):
        exc = rule_excess(thetas[it], em_case["th64"][it], em_case["th80"][it])
        print(f"theta after {it} iterations {thetas[it]}: {exc:.3g} of the bound")
        assert exc <= 1.0, it
    exc = rule_excess(trace, em_case["tr64"], em_case["tr80"])
    print(f"trace: {exc:.3g} of the bound")
    assert exc <= 1.0
    thetas, trace = host_em(hk, p, PRIOR, thetas[-1], 175)
    gain = np.diff(trace)
    assert (gain >= -1e-9 * np.abs(trace[1:])).all(), gain.min()
    assert (gain <= 1e-9 * np.abs(trace[1:])).any()  # converged within 200 iterations
    kon, koff = realised_rates(z)
    print(f"EM kon {thetas[-1][0]:.5f} koff {thetas[-1][1]:.5f}; realised {kon:.5f} {koff:.5f}")
    assert abs(thetas[-1][0] / kon - 1) < 0.10 and abs(thetas[-1][1] / koff - 1) < 0.10
    # the input is one the smoothing matters for: the thresholded raster's rates are off by more than a factor of 2
    raw_kon, raw_koff = realised_rates(p > 0.5)
    print(f"thresholded kon {raw_kon:.5f} koff {raw_koff:.5f}")
    assert raw_kon > 2 * kon and raw_koff > 2 * koff


def test_em_trace_is_monotone_from_the_start(hk, em_case):
    _, trace = host_em(hk, em_case["p"], PRIOR, em_case["start"], 25)
    assert (np.diff(trace) >= -1e-9 * np.abs(trace[1:])).all()
    assert trace[-1] > trace[0]


# ---- Viterbi ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def path_case():
    """N = 37, F = 203, generator seed 3, rows 0-2 special (all 0, all 1, alternating); kon 0.05, koff 0.1, pi0 = 1/3."""
    p, z = synthetic_chain(37, 203, seed=3)
    p[:3] = with_special_rows(p[:3], PRIOR)
    theta = (0.05, 0.10, PRIOR)
    path, margin = oracle_viterbi(p, theta, PRIOR)
    return {"p": p, "z": z, "theta": theta, "path": path, "margin": margin}


def test_viterbi_path_is_the_oracles(hk, path_case):
    p, theta = path_case["p"], path_case["theta"]
    print(f"smallest decision margin of the oracle: {path_case['margin']:.3g}")
    assert path_case["margin"] > 1e-9
    path = host_viterbi(hk, p, theta, PRIOR)
    assert path.dtype == np.uint8 and np.array_equal(path, path_case["path"])
    assert not path[0].any() and path[1].all()
    best = path_logprob(path, p, theta, PRIOR)
    gamma = host_estep(hk, p, theta, PRIOR)["gamma"]
    for other in (gamma > 0.5, p > 0.5):
        assert (best >= path_logprob(other, p, theta, PRIOR) - 1e-9).all()
    err_raw, err_path = ((p[3:] > 0.5) != path_case["z"][3:]).mean(), (path[3:] != path_case["z"][3:]).mean()
    err_gamma = ((gamma[3:] > 0.5) != path_case["z"][3:]).mean()
    print(f"label error: raw {err_raw:.4f}, smoothed {err_gamma:.4f}, Viterbi {err_path:.4f}")
    assert err_gamma < err_raw


@pytest.mark.parametrize("F", [1, 2, 15, 16, 17, 33])
def test_viterbi_word_boundaries(hk, F):
    """Back-pointers are packed 16 frames to a word."""
    p = synthetic_chain(5, F, seed=F)[0]
    path, margin = oracle_viterbi(p, THETA, PRIOR)
    assert margin > 1e-9
    assert np.array_equal(host_viterbi(hk, p, THETA, PRIOR), path)


# ---- backward sampler ---------------------------------------------------------------------------------------------------
def test_sampler_counts_are_those_of_its_raster(hk, path_case):
    filt = host_estep(hk, path_case["p"], path_case["theta"], PRIOR)["filt"]
    F = filt.shape[1]
    counts, raster, margin = host_count(hk, filt, path_case["theta"], 71, seed=0)
    print(f"smallest |u - q| at seed 0: {margin:.3g}")
    assert margin > 1e-9  # the seed of the GPU test: a last-bit difference of q changes no label
    assert raster.max() <= 1 and np.array_equal(counts, oracle_counts(raster))
    assert (counts[..., 1] + counts[..., 3] == F - 1).all()
    assert not raster[:, 0].any() and raster[:, 1].all()
    again = host_count(hk, filt, path_case["theta"], 71, seed=0)
    assert np.array_equal(again[0], counts) and not np.array_equal(host_count(hk, filt, path_case["theta"], 71, 1)[0], counts)
    one = host_count(hk, filt[:, :1], path_case["theta"], 3, seed=0)
    assert not one[0].any()


def test_sampler_draws_the_smoothed_law(hk):
    """S = 4096, N = 9, F = 65: the mean of the rasters within 5 sigma of gamma, sigma^2 = gamma (1 - gamma) / S, and the
    mean counts within 5 sigma of the E-step's expectations (a count is at most F - 1, so sigma <= (F - 1) / 2 / sqrt(S))."""
    S, N, F = 4096, 9, 65
    p = with_special_rows(synthetic_chain(N, F, seed=9)[0], PRIOR)
    e = host_estep(hk, p, THETA, PRIOR)
    counts, raster, _ = host_count(hk, e["filt"], THETA, S, seed=5)
    gamma = e["gamma"]
    sigma = np.sqrt(gamma * (1 - gamma) / S)
    dev = np.abs(raster.mean(0) - gamma) / np.maximum(sigma, 1e-4)
    print(f"largest deviation of the raster mean: {dev.max():.2f} sigma")
    assert dev.max() < 5.0
    sd = counts.std(0) / np.sqrt(S)
    dev = np.abs(counts.mean(0) - e["rows"][:, :4]) / np.maximum(sd, 1e-3)
    print(f"largest deviation of the mean counts: {dev.max():.2f} sigma")
    assert dev.max() < 5.0


# ---- ABI ------------------------------------------------------------------------------------------------------------
def header_fields(name):
    """Field names of ``typedef struct { ... } name;`` in include/tapqir_hip.h, in order."""
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tapqir_hip.h")).read(), flags=re.S)
    body = re.search(r"typedef struct \{([^{}]*)\}\s*%s;" % name, text).group(1)
    out = []
    for decl in body.split(";"):
        if decl.strip():
            out += [re.search(r"(\w+)\s*$", d.strip()).group(1) for d in decl.split(",")]
    return out


MIRRORS = {"tq_smooth_estep_args": _lib_smooth.SmoothEstepArgs, "tq_smooth_mstep_args": _lib_smooth.SmoothMstepArgs,
           "tq_smooth_viterbi_args": _lib_smooth.SmoothViterbiArgs, "tq_smooth_count_args": _lib_smooth.SmoothCountArgs}


def test_struct_layouts_match_the_c_header():
    """sizeof and every offsetof of the four mirrors equal the C compiler's, and the mirrors name the header's fields in
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
           + '\n  printf("%d\\n%d\\n", TQ_SMOOTH_MAX_F, TQ_SMOOTH_COLS);\n'
           + '  printf("%d\\n", TQ_SMOOTH_PMIN == 1e-6 && TQ_SMOOTH_RMIN == 1e-9);\n  return 0;\n}\n')
    with tempfile.TemporaryDirectory() as td:
        c = os.path.join(td, "s.c")
        open(c, "w").write(src)
        exe = os.path.join(td, "s")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        got = [int(v) for v in subprocess.check_output([exe]).split()]
    assert got.pop() == 1
    assert got.pop() == _lib_smooth.SMOOTH_COLS == 6
    assert got.pop() == _lib_smooth.SMOOTH_MAX_F == 65536
    assert len(got) == len(want)
    assert [(n, f, g) for (n, f, _), g in zip(want, got)] == want


def test_the_binding_keeps_its_mirrors_out_of_lib():
    names = {"tq_smooth_estep", "tq_smooth_mstep", "tq_smooth_viterbi", "tq_smooth_count"}
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tapqir_hip.h")).read(), flags=re.S)
    declared_symbols = set(re.findall(r"\b(tq_[a-z_0-9]+)\s*\(", text))
    assert names <= set(_lib.EXPORTS) and names <= declared_symbols
    assert not any(isinstance(v, type) and issubclass(v, ctypes.Structure) and v.__module__ == _lib_smooth.__name__
                   for v in vars(_lib).values())


def test_argument_validation_returns_error_codes_without_a_gpu():
    lib = _lib_smooth.lib()
    buf = (ctypes.c_int64 * 8)()
    addr = ctypes.addressof(buf) & ~15
    calls = {"estep": (lib.tq_smooth_estep, _lib_smooth.SmoothEstepArgs,
                       dict(p=addr, theta=addr, filt=addr, gamma=addr, rows=addr, N=3, F=5, prior=0.3)),
             "mstep": (lib.tq_smooth_mstep, _lib_smooth.SmoothMstepArgs, dict(rows=addr, theta=addr, trace=addr, N=3, it=0)),
             "viterbi": (lib.tq_smooth_viterbi, _lib_smooth.SmoothViterbiArgs,
                         dict(p=addr, theta=addr, back=addr, path=addr, N=3, F=5, prior=0.3)),
             "count": (lib.tq_smooth_count, _lib_smooth.SmoothCountArgs,
                       dict(filt=addr, theta=addr, counts=addr, N=3, F=5, S=2))}

    def refused(name, text, **change):
        fn, cls, good = calls[name]
        assert fn(ctypes.byref(cls(**{**good, **change})), None) == 1, (name, change)  # TQ_ERR_ARG
        err = lib.tq_last_error()
        assert ("tq_smooth_" + name).encode() in err and text in err, err

    for name, (fn, cls, good) in calls.items():
        assert fn(None, None) == 1
        assert fn(ctypes.byref(cls()), None) == 1 and b"NULL" in lib.tq_last_error()
        for key, value in good.items():
            if value == addr:
                refused(name, b"NULL", **{key: None})
        refused(name, b"positive", N=0)
    for name in ("estep", "viterbi", "count"):
        refused(name, b"positive", F=0)
        refused(name, b"65536", F=65537)
    for name in ("estep", "viterbi"):
        for prior in (0.0, 1.0, -0.5, float("nan")):
            refused(name, b"prior", prior=prior)
    refused("mstep", b"non-negative", it=-1)
    refused("count", b"positive", S=0)
    refused("count", b"S too large", S=65535 * 64 + 1)
    refused("count", b"aligned", counts=addr + 4)


def test_device_entry_points_refuse_host_tensors():
    from tapqir_amd.exceptions import HipExtensionError
    from tapqir_amd.utils.mle_analysis import smooth_estep, smooth_fit, smooth_mstep, smooth_sample, smooth_viterbi

    theta = torch.tensor(THETA, dtype=torch.float64)
    with pytest.raises(HipExtensionError):
        smooth_estep(torch.rand(3, 5), theta, PRIOR)
    with pytest.raises(HipExtensionError):
        smooth_fit(torch.rand(3, 5), PRIOR)
    with pytest.raises(HipExtensionError):
        smooth_viterbi(torch.rand(3, 5), theta, PRIOR)
    with pytest.raises(HipExtensionError):
        smooth_sample(torch.rand(3, 5, dtype=torch.float64), theta, 4)
    with pytest.raises(HipExtensionError):
        smooth_mstep(torch.rand(3, 6, dtype=torch.float64), theta, torch.zeros(1, dtype=torch.float64))
    with pytest.raises(ValueError):
        smooth_fit(torch.rand(3, 5), PRIOR, kon=0.0)


# ---- command line -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [["--cpu"], ["--model", "crosstalk"]])
def test_smooth_off_the_device_or_off_cosmos_is_refused(tmp_path, flags):
    save(simulate(2, 2, 5, 1, 14, params=dict(TEST_PARAMS)), tmp_path)
    result = CliRunner().invoke(app, ["--cd", str(tmp_path), "smooth", *flags, "--num-samples", "10", "--no-input"])
    assert result.exit_code == 1, result.output  # 2 = no such command
    assert ("GPU" if flags == ["--cpu"] else "cosmos only") in result.output
