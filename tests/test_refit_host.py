"""Bootstrap refits of the chain over AOIs without a GPU: the g++ build of tq_refit.h (the weights
of the resamples, the E-step that leaves out the pairs of weight 0, the weighted M-step with the device's strided sums and
tree) against the numpy oracle of refit_fixture by the tolerance rule of section 20 and against the g++ build of
tq_multistart.h bit for bit where the issue says so, the batches of ``hmm_fit_refits`` driven on that build, the C layout
of the three argument structs, the exports, argument validation of the entry points, and the exits and the help text of
``smooth --refit / --refit-seed``.  The ``check_*`` functions take a backend, so that tests/test_gpu_refit.py runs them on
the kernels."""

import ctypes
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest
import torch
from typer.testing import CliRunner

import multistart_fixture as msf
from hmm_fixture import build_hmm_check, fixed_theta, host_estimate
from refit_fixture import (FIT, PRIOR, START, build_refit_check, canonical, cols, fit_case, host_estep, host_fit_refits,
                           host_mstep, host_weights, oracle_mstep_weighted, oracle_weights, rule_excess)
from smooth_fixture import synthetic_chain, with_special_rows
from tapqir_amd import _lib, _lib_multistart, _lib_refit
from tapqir_amd.main import app
from tapqir_amd.utils.dataset import save
from tapqir_amd.utils.simulate import TEST_PARAMS, simulate
from test_hmm_host import rule_bound

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UB_OF_M = {2: (1, 1), 3: (1, 2), 4: (2, 2)}


class HostBackend:
    """The g++ builds behind the interface the checks use: numpy in, numpy out."""

    def __init__(self, refit, multistart, hmm):
        self.refit, self.multistart, self.hmm = refit, multistart, hmm

    def weights(self, seed, first, R, N):
        return host_weights(self.refit, seed, first, R, N)

    def estimate_totals(self, trans, U, B, seed):
        return host_estimate(self.hmm, trans, U, B, 1, seed)[0]

    def ms_estep(self, p, thetas, U, B):
        return msf.host_estep(self.multistart, p, thetas, U, B, PRIOR)

    def ms_mstep(self, rows, thetas, T, it, U, B, allow=None):
        thetas, trace = np.array(thetas, dtype=np.float64), np.full((len(thetas), T), np.nan)
        msf.host_mstep(self.multistart, rows, thetas, trace, it, U, B, allow)
        return thetas, trace

    def estep(self, p, thetas, w, U, B, active, rows, filt):
        rows, filt = rows.copy(), filt.copy()
        host_estep(self.refit, p, thetas, w, U, B, PRIOR, active, rows, filt)
        return rows, filt

    def mstep(self, rows, w, thetas, T, it, U, B, allow=None, active=None):
        thetas, trace = np.array(thetas, dtype=np.float64), np.full((len(thetas), T), np.nan)
        host_mstep(self.refit, rows, w, thetas, trace, it, U, B, allow, active)
        return thetas, trace

    def fit_refits(self, p, theta_hat, U, B, refits, seed, num_iter, tol, chunk):
        fit = host_fit_refits(self.refit, p, PRIOR, theta_hat, U, B, refits, seed, None, num_iter, tol, chunk)
        fit["thetas"] = np.array([canonical(t, U, B)[0] for t in fit["thetas"]])
        return fit

    def ms_fit(self, p, start, U, B, num_iter, tol, chunk):
        fit = msf.host_fit(self.multistart, p, PRIOR, start[None], U, B, None, num_iter, tol, chunk)
        return canonical(fit["thetas"][0], U, B)[0], fit["traces"][0]


@pytest.fixture(scope="module")
def be(tmp_path_factory):
    d = tmp_path_factory.mktemp("refit")
    return HostBackend(build_refit_check(d), msf.build_multistart_check(d), build_hmm_check(d))


# ---- weights ------------------------------------------------------------------------------------------------------------
def check_weights(be, N, R, first):
    """The bincount of the oracle's indices; every row sums to N; one call equals two batches joined at any row."""
    seed = 11
    want = oracle_weights(seed, first, R, N)
    got = be.weights(seed, first, R, N)
    assert got.dtype == np.int32 and got.shape == (R, N)
    assert np.array_equal(got, want)
    assert (got.sum(1) == N).all() and (got >= 0).all()
    if N == 1:
        assert (got == 1).all()
    if R > 1:
        k = R // 2
        joined = np.concatenate([be.weights(seed, first, k, N), be.weights(seed, first + k, R - k, N)])
        assert np.array_equal(joined, got)
    assert np.array_equal(be.weights(seed, first, R, N), got)
    if N >= 63:
        assert not np.array_equal(be.weights(seed + 1, first, R, N), got)


@pytest.mark.parametrize("first", [0, 5])
@pytest.mark.parametrize("R", [1, 3, 64])
@pytest.mark.parametrize("N", [1, 2, 63, 400])
def test_weights_are_the_bincount_of_the_resample(be, N, R, first):
    check_weights(be, N, R, first)


def check_weights_against_the_estimate(be, N):
    """``tq_hmm_estimate`` with resample = 1 on a `trans` whose entries are known per-AOI integers: its totals of sample s
    are sum_n weights[s, n] trans[n] -- the same AOIs are resampled there and here."""
    S, seed, M = 5, 4, 2
    rng = np.random.default_rng(N)
    per_aoi = rng.integers(0, 1000, (N, M * M)).astype(np.int32)
    trans = np.broadcast_to(per_aoi, (S, N, M * M)).copy()
    totals = be.estimate_totals(trans, 1, 1, seed)
    w = be.weights(seed, 0, S, N).astype(np.int64)
    assert np.array_equal(totals.reshape(S, M * M), w @ per_aoi.astype(np.int64))


@pytest.mark.parametrize("N", [2, 63, 400])
def test_weights_are_the_resample_of_the_estimate(be, N):
    check_weights_against_the_estimate(be, N)


# ---- M-step -------------------------------------------------------------------------------------------------------------
def mstep_case(N, M, R):
    U, B = UB_OF_M[M]
    rng = np.random.default_rng(1000 * N + 10 * M + R)
    rows = rng.random((R, N, cols(M)))
    rows[:, :, M * M: M * M + M] /= rows[:, :, M * M: M * M + M].sum(2, keepdims=True)
    rows[:, :, -1] = -50.0 * rng.random((R, N)) - 1.0
    w = rng.integers(0, 4, (R, N)).astype(np.int32)
    w[np.arange(R), rng.integers(0, N, R)] = 2  # at least one AOI drawn
    theta0 = np.array([fixed_theta(U, B, seed=r % 5) for r in range(R)])
    return U, B, rows, w, theta0


def check_mstep(be, N, M, R):
    U, B, rows, w, theta0 = mstep_case(N, M, R)
    T, it = 3, 1
    # all weights 1: tq_multistart_mstep bit for bit
    ones = np.ones((R, N), np.int32)
    got1, tr1 = be.mstep(rows, ones, theta0, T, it, U, B)
    want1, wtr1 = be.ms_mstep(rows, theta0, T, it, U, B)
    assert np.array_equal(got1, want1) and np.array_equal(tr1[:, it], wtr1[:, it]) and np.isnan(tr1[:, [0, 2]]).all()
    # integer weights: the long-double oracle, and the unweighted M-step on rows repeated w times
    got, tr = be.mstep(rows, w, theta0, T, it, U, B)
    worst = 0.0
    for r in range(R):
        t64, l64 = oracle_mstep_weighted(rows[r], w[r], theta0[r], U, B)
        t80, l80 = oracle_mstep_weighted(rows[r], w[r], theta0[r], U, B, dtype=np.longdouble)
        exc = rule_excess(got[r], t64, t80), rule_excess([tr[r, it]], [l64], [l80])
        assert max(exc) <= 1.0, (r, exc)
        worst = max(worst, *exc)
        if r < 3:
            rep, rtr = be.ms_mstep(np.repeat(rows[r], w[r], axis=0)[None], theta0[r:r + 1], T, it, U, B)
            assert np.abs(rep[0] - got[r]).max() <= 2 * rule_bound(t64, t80), r
            assert abs(rtr[0, it] - tr[r, it]) <= 2 * rule_bound([l64], [l80]), r
    print(f"N = {N} M = {M} R = {R}: weighted M-step {worst:.3g} of the bound")
    assert np.abs(got[:, : M * M].reshape(R, M, M).sum(2) - 1).max() <= 4 * np.spacing(1.0)
    # a row of weight 0 is never read
    poisoned = rows.copy()
    poisoned[w == 0] = np.nan
    got_nan, tr_nan = be.mstep(poisoned, w, theta0, T, it, U, B)
    assert np.isfinite(got_nan).all() and np.isfinite(tr_nan[:, it]).all()
    assert np.array_equal(got_nan, got) and np.array_equal(tr_nan[:, it], tr[:, it])
    # a cleared allow bit stays at the floor
    allow = msf.forbid(M, (0, M - 1))
    masked, _ = be.mstep(rows, w, theta0, T, it, U, B, allow)
    A = masked[:, : M * M].reshape(R, M, M)
    assert (A[:, 0, M - 1] <= 1e-9).all() and (A[:, 0, M - 1] > 0).all() and (A[:, allow] > 1e-6).all()
    # an inactive replica keeps theta and writes no trace entry
    if R > 1:
        active = np.ones(R, np.int32)
        active[1] = 0
        frozen, ftr = be.mstep(rows, w, theta0, T, it, U, B, None, active)
        assert np.array_equal(frozen[1], theta0[1]) and np.isnan(ftr[1]).all()
        keep = active == 1
        assert np.array_equal(frozen[keep], got[keep]) and np.array_equal(ftr[keep, it], tr[keep, it])
    # two runs give the same bits
    again, tr2 = be.mstep(rows, w, theta0, T, it, U, B)
    assert np.array_equal(again, got) and np.array_equal(tr2[:, it], tr[:, it])
    return worst


@pytest.mark.parametrize("R", [1, 2, 64])
@pytest.mark.parametrize("M", [2, 3, 4])
@pytest.mark.parametrize("N", [1, 2, 255, 256, 257, 300])
def test_weighted_mstep(be, N, M, R):
    check_mstep(be, N, M, R)


# ---- E-step -------------------------------------------------------------------------------------------------------------
def check_estep(be, F, U, B):
    """N = 6 shared rows, R = 3 chains, weights with zeros in every replica: where w > 0 the bits of tq_multistart_estep,
    where w = 0 the sentinel in rows and scratch; an inactive replica untouched."""
    M, N, R, sentinel = U + B, 6, 3, -123.25
    thetas = np.array([fixed_theta(U, B, seed=r) for r in range(R)])
    p = with_special_rows(synthetic_chain(N, F, seed=F)[0], PRIOR)
    w = np.array([[1, 0, 2, 0, 1, 3], [0, 0, 0, 0, 0, 6], [1, 1, 1, 1, 1, 1]], np.int32)
    want = be.ms_estep(p, thetas, U, B)
    rows0, filt0 = np.full((R, N, cols(M)), sentinel), np.full((R, N, F, M), sentinel)
    rows, filt = be.estep(p, thetas, w, U, B, None, rows0, filt0)
    assert np.array_equal(rows[w > 0], want[w > 0])
    assert (rows[w == 0] == sentinel).all() and (filt[w == 0] == sentinel).all()
    assert (filt[w > 0] != sentinel).all()
    active = np.array([1, 1, 0], np.int32)
    rows_a, filt_a = be.estep(p, thetas, w, U, B, active, rows0, filt0)
    assert (rows_a[2] == sentinel).all() and (filt_a[2] == sentinel).all() and np.array_equal(rows_a[:2], rows[:2])
    again, _ = be.estep(p, thetas, w, U, B, None, rows0, filt0)
    assert np.array_equal(again, rows)


@pytest.mark.parametrize("U,B", [(1, 1), (1, 2), (2, 2)])
@pytest.mark.parametrize("F", [1, 2, 65, 203])
def test_estep_skips_the_pairs_of_weight_zero(be, F, U, B):
    check_estep(be, F, U, B)


# ---- fit ----------------------------------------------------------------------------------------------------------------
def check_fit(be, U, B):
    """R = 8 refits for 25 iterations on N = 40, F = 500: every replica's theta and trace against the oracle's weighted EM;
    replica 0 against the unweighted batched EM from the same start."""
    case = fit_case(U, B)
    T = FIT["num_iter"]
    fit = be.fit_refits(case["p"], case["start"], U, B, FIT["refits"], FIT["seed"], T, -1.0, 10)  # tol < 0: no early stop
    assert fit["iterations"] == [T] * 9
    worst = 0.0
    for r in range(9):
        t64, t80 = canonical(case["th64"][r][T], U, B)[0], canonical(case["th80"][r][T], U, B)[0]
        exc = rule_excess(fit["thetas"][r], t64, t80), rule_excess(fit["traces"][r], case["tr64"][r], case["tr80"][r])
        print(f"({U}, {B}) replica {r}: theta after {T} iterations {exc[0]:.3g}, trace {exc[1]:.3g} of the bound")
        assert max(exc) <= 1.0, r
        worst = max(worst, *exc)
    theta0, trace0 = be.ms_fit(case["p"], case["start"], U, B, T, -1.0, 10)
    t64, t80 = canonical(case["th64"][0][T], U, B)[0], canonical(case["th80"][0][T], U, B)[0]
    assert np.abs(theta0 - fit["thetas"][0]).max() <= 2 * rule_bound(t64, t80)
    assert np.abs(trace0 - fit["traces"][0]).max() <= 2 * rule_bound(case["tr64"][0], case["tr80"][0])
    return worst


@pytest.mark.parametrize("U,B", [(1, 1), (1, 2)])
def test_refits_follow_the_oracles_weighted_em(be, U, B):
    check_fit(be, U, B)


def check_batches(be):
    """R = 70 takes two batches (64 + 7 replicas), R = 64 two as well (64 + 1): replicas 0 .. 64 have the same bits."""
    p = synthetic_chain(5, 40, seed=2)[0]
    start = START[(1, 1)]
    a = be.fit_refits(p, start, 1, 1, 70, 9, 4, -1.0, 3)
    b = be.fit_refits(p, start, 1, 1, 64, 9, 4, -1.0, 3)
    assert a["thetas"].shape == (71, 6) and b["thetas"].shape == (65, 6)
    assert np.array_equal(a["thetas"][:65], b["thetas"]) and np.array_equal(a["traces"][:65], b["traces"])
    assert a["iterations"][:65] == b["iterations"] and len({tuple(t) for t in a["thetas"]}) > 20


def test_a_replica_does_not_depend_on_its_batch(be):
    check_batches(be)


# ---- ABI ------------------------------------------------------------------------------------------------------------
def header_text():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tapqir_hip.h")).read(), flags=re.S)


def header_fields(name):
    """Field names of ``typedef struct { ... } name;`` in include/tapqir_hip.h, in order."""
    body = re.search(r"typedef struct \{([^{}]*)\}\s*%s;" % name, header_text()).group(1)
    out = []
    for decl in body.split(";"):
        if decl.strip():
            out += [re.search(r"(\w+)\s*$", d.strip()).group(1) for d in decl.split(",")]
    return out


MIRRORS = {"tq_refit_weights_args": _lib_refit.RefitWeightsArgs, "tq_refit_estep_args": _lib_refit.RefitEstepArgs,
           "tq_refit_mstep_args": _lib_refit.RefitMstepArgs}


def test_struct_layouts_match_the_c_header():
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
           + "\n  return 0;\n}\n")
    with tempfile.TemporaryDirectory() as td:
        c = os.path.join(td, "s.c")
        open(c, "w").write(src)
        exe = os.path.join(td, "s")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        got = [int(v) for v in subprocess.check_output([exe]).split()]
    assert len(got) == len(want)
    assert [(n, f, g) for (n, f, _), g in zip(want, got)] == want


def test_exports_are_the_headers_declarations():
    names = {"tq_refit_weights", "tq_refit_estep", "tq_refit_mstep"}
    declared = set(re.findall(r"\b(tq_[a-z_0-9]+)\s*\(", header_text()))
    assert {n for n in declared if n.startswith("tq_refit_")} == names
    assert names == {n for n in _lib.EXPORTS if n.startswith("tq_refit_")}
    lib = _lib_refit.lib()
    assert all(hasattr(lib, n) for n in names)


def test_argument_validation_returns_error_codes_without_a_gpu():
    lib = _lib_refit.lib()
    buf = (ctypes.c_int64 * 8)()
    addr = ctypes.addressof(buf)
    A = _lib_refit
    calls = {"weights": (lib.tq_refit_weights, A.RefitWeightsArgs, dict(weights=addr, N=3, R=2, first=0, seed=1)),
             "estep": (lib.tq_refit_estep, A.RefitEstepArgs,
                       dict(p=addr, theta=addr, filt=addr, rows=addr, weights=addr, N=3, F=5, R=2, U=1, B=2, prior=0.3)),
             "mstep": (lib.tq_refit_mstep, A.RefitMstepArgs,
                       dict(rows=addr, theta=addr, trace=addr, weights=addr, N=3, it=0, T=1, R=2, U=1, B=2, allow=0x1FF))}

    def refused(name, text, **change):
        fn, cls, good = calls[name]
        assert fn(ctypes.byref(cls(**{**good, **change})), None) == 1, (name, change)  # TQ_ERR_ARG
        err = lib.tq_last_error()
        assert ("tq_refit_" + name).encode() in err and text in err, err

    for name, (fn, cls, good) in calls.items():
        assert fn(None, None) == 1
        assert fn(ctypes.byref(cls()), None) == 1 and b"NULL" in lib.tq_last_error()
        for key, value in good.items():
            if value == addr:
                refused(name, b"NULL", **{key: None})
        refused(name, b"positive", N=0)
        for R in (0, -1, 65):
            refused(name, b"at most 64", R=R)
    for name in ("estep", "mstep"):
        for U, B in ((0, 2), (2, 0), (-1, 3), (1, 4), (3, 2), (4, 1)):
            refused(name, b"U + B at most 4", U=U, B=B)
    refused("weights", b"first", first=-1)
    refused("weights", b"first", first=2**31 - 2)
    refused("estep", b"positive", F=0)
    refused("estep", b"65536", F=65537)
    for prior in (0.0, 1.0, -0.5, float("nan")):
        refused("estep", b"prior", prior=prior)
    refused("mstep", b"non-negative", it=-1)
    refused("mstep", b"T must exceed it", it=1, T=1)
    refused("mstep", b"T must exceed it", it=0, T=0)
    refused("mstep", b"allow", allow=0x3FF)      # a bit beyond M * M = 9
    refused("mstep", b"allow", allow=0x1FF & ~0b111000)  # row 1 has no free entry
    refused("mstep", b"allow", allow=0)


def test_device_entry_points_refuse_host_tensors_and_bad_arguments():
    from tapqir_amd.exceptions import HipExtensionError
    from tapqir_amd.utils import mle_analysis as ma

    p, thetas = torch.rand(3, 5), torch.from_numpy(np.array([fixed_theta(1, 2, seed=r) for r in range(2)]))
    w = torch.ones(2, 3, dtype=torch.int32)
    with pytest.raises(HipExtensionError):
        ma.hmm_fit_refits(p, PRIOR, thetas[0], 1, 2, 4)
    with pytest.raises(HipExtensionError):
        ma.refit_weights(3, 2, device="cpu")
    with pytest.raises(HipExtensionError):
        ma.refit_estep(p, thetas, w, PRIOR, 1, 2)
    with pytest.raises(HipExtensionError):
        ma.refit_mstep(torch.rand(2, 3, 13, dtype=torch.float64), thetas, w, torch.zeros(2, 1, dtype=torch.float64), 0, 1, 2)
    for U, B in ((0, 1), (1, 0), (3, 2), (1, 4)):
        with pytest.raises(ValueError):
            ma.hmm_fit_refits(p, PRIOR, thetas[0], U, B, 4)
    for bad in (dict(refits=-1), dict(refits=4097), dict(refits=2, num_iter=0), dict(refits=2, allow=torch.ones(2, 2))):
        with pytest.raises(ValueError):
            ma.hmm_fit_refits(p, PRIOR, thetas[0], 1, 2, **bad)
    assert ma.REFIT_MAX == 4096 and _lib_multistart.MULTISTART_MAX == 64


# ---- command line -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags,text", [
    (["--refit", "4", "--joint", "0,1"], "--refit does not go with --joint or --populations"),
    (["--refit", "4", "--structure", "full"], "--refit does not go with --joint or --populations"),
    (["--refit", "4", "--populations", "2"], "--refit does not go with --joint or --populations"),
    (["--refit", "4", "--bound-states", "2", "--populations", "2", "--cpu"], "--refit does not go with --joint or --populations"),
    (["--refit", "4", "--cpu"], "GPU"),
    (["--refit", "4", "--refit-seed", "3", "--bound-states", "2", "--cpu"], "GPU"),
    (["--refit", "4", "--model", "crosstalk"], "cosmos only"),
])
def test_smooth_refusals(tmp_path, flags, text):
    save(simulate(2, 2, 5, 1, 14, params=dict(TEST_PARAMS)), tmp_path)
    result = CliRunner().invoke(app, ["--cd", str(tmp_path), "smooth", *flags, "--num-samples", "10", "--no-input"])
    assert result.exit_code == 1, result.output  # 2 = no such command or option
    assert text in result.output


@pytest.mark.parametrize("value", ["-1", "4097"])
def test_smooth_refit_out_of_range_is_a_usage_error(tmp_path, value):
    result = CliRunner().invoke(app, ["--cd", str(tmp_path), "smooth", "--refit", value, "--cpu"])
    assert result.exit_code == 2 and "4096" in result.output


def test_smooth_help_shows_the_new_options(tmp_path):
    result = CliRunner().invoke(app, ["--cd", str(tmp_path), "smooth", "--help"])
    assert result.exit_code == 0
    for option in ("--refit", "--refit-seed"):
        assert option in result.output
