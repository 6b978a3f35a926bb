"""Several EM starts side by side without a GPU: the g++ build of tq_multistart.h (the batched
E-step with the device's lane ownership, scan order and replica layout, the batched M-step under a topology mask) against
the numpy oracle of hmm_fixture by the tolerance rule of section 20, the chunk and freezing logic of ``hmm_fit_restarts``
(``multistart_em``) driven on that build, the best of eight starts on data where the default start is stuck, a constrained
topology, the generator of the starts, the C layout of the two argument structs, the exports, argument validation of the
entry points, and the exits and the help text of ``smooth --restarts / --restart-seed / --forbid``."""

import ctypes
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest
import torch
from typer.testing import CliRunner

from hmm_fixture import default_start, fixed_theta, oracle_mstep, with_special_rows
from multistart_fixture import (F_LIST, FREEZE, PRIOR, UB_LIST, best_case, bic, build_multistart_check, cols, em_case, forbid,
                                full, host_estep, host_fit, host_model, host_mstep, normalised, oracle_em_masked, oracle_estep,
                                oracle_loglik, oracle_mstep_masked, oracle_stop, rule_excess, synthetic_hmm,
                                threshold_margin)
from tapqir_amd import _lib, _lib_multistart
from tapqir_amd.main import app
from tapqir_amd.utils.dataset import save
from tapqir_amd.utils.simulate import TEST_PARAMS, simulate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def hk(tmp_path_factory):
    return build_multistart_check(tmp_path_factory.mktemp("multistart"))


def groups(M):
    """The column groups of ``rows``: expected pair counts, gamma_0, loglik."""
    return (("pairs", slice(0, M * M)), ("gamma0", slice(M * M, M * M + M)), ("loglik", slice(M * M + M, M * M + M + 1)))


def check_rows(got, p, theta, U, B, who):
    """One replica's rows (N, COLS) against the oracle at its theta, by the rule; prints each excess, returns the largest."""
    M = U + B
    o64, o80 = oracle_estep(p, theta, U, B, PRIOR)["rows"], oracle_estep(p, theta, U, B, PRIOR, np.longdouble)["rows"]
    worst = 0.0
    for name, sl in groups(M):
        exc = rule_excess(got[:, sl], o64[:, sl], o80[:, sl])
        print(f"{who} rows/{name}: {exc:.3g} of the bound")
        assert exc <= 1.0, (who, name, exc)
        worst = max(worst, exc)
    return worst


# ---- batched E-step -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("U,B", UB_LIST)
@pytest.mark.parametrize("F", F_LIST)
def test_batched_estep_equals_the_oracle_and_the_single_replica(hk, U, B, F):
    """R = 3 chains on N = 6 shared rows (all 0, all 1, alternating, p = prior, two of the reference chain): every replica
    by the rule, with the bits of a run of that replica alone, and an inactive replica untouched by both steps."""
    M = U + B
    thetas = np.array([fixed_theta(U, B, seed=r) for r in range(3)])
    p = with_special_rows(synthetic_hmm(6, F, seed=F)[0], PRIOR)
    rows = host_estep(hk, p, thetas, U, B, PRIOR)
    assert rows.shape == (3, 6, cols(M)) and np.isfinite(rows).all()
    for r in range(3):
        check_rows(rows[r], p, thetas[r], U, B, f"({U}, {B}) F = {F} replica {r}")
        alone = host_estep(hk, p, thetas[r:r + 1], U, B, PRIOR)
        assert np.array_equal(alone[0], rows[r]), r
    assert np.allclose(rows[:, :, : M * M].sum(2), F - 1, rtol=0, atol=1e-9 * F)

    active = np.array([1, 0, 1], np.int32)
    frozen = host_estep(hk, p, thetas, U, B, PRIOR, active)
    assert np.isnan(frozen[1]).all() and np.array_equal(frozen[[0, 2]], rows[[0, 2]])
    new, trace = thetas.copy(), np.full((3, 4), np.nan)
    host_mstep(hk, rows, new, trace, 2, U, B, None, active)
    assert np.array_equal(new[1], thetas[1]) and np.isnan(trace[1]).all()
    assert np.isfinite(trace[[0, 2], 2]).all() and np.isnan(trace[:, [0, 1, 3]]).all()
    assert not np.array_equal(new[0], thetas[0]) and not np.array_equal(new[2], thetas[2])


# ---- batched M-step -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("U,B", [(1, 2), (2, 2)])
def test_batched_mstep_free_and_masked(hk, U, B):
    """N = 300 rows (more than the 256 threads of the device's workgroup), R = 3.  A forbidden entry is stored at most at
    1e-9, and is read by tq_hmm_model as 1e-9 to within 4 ulp (measured: 1e-9 (1 + 2.2e-16) at the most)."""
    M = U + B
    rng = np.random.default_rng(2)
    rows = rng.random((3, 300, cols(M)))
    rows[:, :, M * M: M * M + M] /= rows[:, :, M * M: M * M + M].sum(2, keepdims=True)
    theta0 = np.array([fixed_theta(U, B, seed=r) for r in range(3)])
    allow = forbid(M, (M - 2, M - 1), (M - 1, M - 2), (0, M - 1))
    ulp = np.spacing(1.0)
    for mask, name in ((None, "free"), (allow, "masked")):
        thetas, trace = theta0.copy(), np.full((3, 2), np.nan)
        host_mstep(hk, rows, thetas, trace, 1, U, B, mask)
        for r in range(3):
            if mask is None:
                (t64, l64), (t80, l80) = oracle_mstep(rows[r], theta0[r], U, B), oracle_mstep(rows[r], theta0[r], U, B, np.longdouble)
            else:
                t64, l64 = oracle_mstep_masked(rows[r], theta0[r], U, B, mask)
                t80, l80 = oracle_mstep_masked(rows[r], theta0[r], U, B, mask, np.longdouble)
            exc = rule_excess(thetas[r], t64, t80), rule_excess([trace[r, 1]], [l64], [l80])
            print(f"({U}, {B}) {name} replica {r}: theta {exc[0]:.3g}, loglik {exc[1]:.3g} of the bound")
            assert max(exc) <= 1.0
            A = thetas[r, : M * M].reshape(M, M)
            assert np.abs(A.sum(1) - 1).max() <= 4 * ulp and abs(thetas[r, M * M:].sum() - 1) <= 4 * ulp
            if mask is not None:
                # stored: 1e-9 over a row sum above 1.  Read back through tq_hmm_model: 1e-9 over the sum of the floored row,
                # which is 1 + k 1e-18 before rounding, so at most 1e-9 up to the rounding of an M-term sum and a quotient
                read = host_model(hk, thetas[r], U, B)[: M * M].reshape(M, M)
                assert (A[~mask] <= 1e-9).all() and (A[~mask] > 0).all()
                assert (read[~mask] <= 1e-9 * (1 + 4 * ulp)).all() and (read[~mask] > 0).all()
                assert (A[mask] > 1e-3).all()
        assert np.isnan(trace[:, 0]).all()
        again, trace2 = theta0.copy(), np.zeros((3, 2))
        host_mstep(hk, rows, again, trace2, 1, U, B, mask)
        assert np.array_equal(again, thetas) and np.array_equal(trace2[:, 1], trace[:, 1])


def test_allow_check(hk):
    lib = hk
    for M in (2, 3, 4):
        assert lib.hk_multistart_allow_ok(_lib_multistart.allow_bits(full(M)), M) == 1
        assert lib.hk_multistart_allow_ok(_lib_multistart.allow_bits(np.eye(M, dtype=bool)), M) == 1
        assert lib.hk_multistart_allow_ok(1 << (M * M), M) == 0  # a bit beyond M * M
        for i in range(M):
            assert lib.hk_multistart_allow_ok(_lib_multistart.allow_bits(full(M)) & ~(((1 << M) - 1) << (i * M)), M) == 0
    assert _lib_multistart.allow_bits([[True, False], [True, True]]) == 0b1101


# ---- EM -----------------------------------------------------------------------------------------------------------------
def test_em_follows_the_oracle_from_every_start(hk):
    """(1, 2), N = 20, F = 300, the default start and 3 random ones, 15 iterations in chunks of 6, 6 and 3, tol = 0."""
    case = em_case()
    fit = host_fit(hk, case["p"], PRIOR, case["starts"], 1, 2, None, num_iter=15, tol=0.0, chunk=6)
    assert fit["iterations"] == [15] * 4 and fit["converged"] == [False] * 4
    for r in range(4):
        exc = (rule_excess(fit["thetas"][r], case["th64"][r][15], case["th80"][r][15]),
               rule_excess(fit["traces"][r], case["tr64"][r][:15], case["tr80"][r][:15]))
        print(f"start {r}: theta after 15 iterations {exc[0]:.3g}, trace {exc[1]:.3g} of the bound")
        assert max(exc) <= 1.0, r
    whole = host_fit(hk, case["p"], PRIOR, case["starts"], 1, 2, None, num_iter=15, tol=0.0, chunk=15)
    assert np.array_equal(whole["thetas"], fit["thetas"]) and np.array_equal(whole["traces"], fit["traces"])


def test_replicas_freeze_where_the_rule_stops_them(hk):
    """tol = 2e-5, 40 iterations in chunks of 8: the float64 oracle stops the four replicas after 16, 24, 32 and 40
    iterations.  A frozen replica keeps the theta of its stop, bit for bit, while the others go on."""
    case = em_case()
    tol, num_iter, chunk = FREEZE["tol"], FREEZE["num_iter"], FREEZE["chunk"]
    want = [oracle_stop(case["tr64"][r], tol, num_iter, chunk) for r in range(4)]
    margin = min(threshold_margin(case["tr64"][r], tol) for r in range(4))
    print(f"oracle stops {want}, smallest relative distance of a gain from the threshold {margin:.3g}")
    assert margin > 1e-3 and len({w[0] for w in want}) >= 2
    fit = host_fit(hk, case["p"], PRIOR, case["starts"], 1, 2, None, num_iter=num_iter, tol=tol, chunk=chunk)
    assert fit["iterations"] == [w[0] for w in want] and fit["converged"] == [w[1] for w in want]
    for r in range(4):
        stop = fit["iterations"][r]
        short = host_fit(hk, case["p"], PRIOR, case["starts"], 1, 2, None, num_iter=stop, tol=0.0, chunk=chunk)
        assert np.array_equal(short["thetas"][r], fit["thetas"][r]), r
        assert np.array_equal(short["traces"][r], fit["traces"][r, :stop]) and np.isnan(fit["traces"][r, stop:]).all()
        assert fit["logliks"][r] == short["logliks"][r]


# ---- the best of several starts ---------------------------------------------------------------------------------------------
def test_the_best_start_beats_the_default_start(hk):
    """(2, 2) on N = 30, F = 400 of the three-state reference chain, the default start and 7 random ones of seed 7, 120
    iterations, tol = 0: the default start is stuck 5.05 log-evidence units below the best one (float64 oracle)."""
    from tapqir_amd.utils.mle_analysis import hmm_allow, hmm_n_params

    case = best_case()
    fit = host_fit(hk, case["p"], PRIOR, case["starts"], 2, 2, None, num_iter=120, tol=0.0, chunk=50)
    ll = fit["logliks"]
    print("log evidence by start:", np.array2string(ll, precision=3), "best", fit["best"])
    assert fit["best"] != 0 and fit["best"] == int(np.argmax(ll))
    assert ll[fit["best"]] - ll[0] >= 2.0
    exc = rule_excess([ll[0]], [case["ll64"]], [case["ll80"]])
    print(f"default start's log evidence {ll[0]:.6f}: {exc:.3g} of the bound")
    assert exc <= 1.0
    n_params = hmm_n_params(hmm_allow(None, 4))
    assert n_params == 15
    assert bic(ll[fit["best"]], n_params, 30, 400) < bic(ll[0], n_params, 30, 400)


def test_a_forbidden_pair_costs_no_evidence_and_two_parameters(hk):
    """(1, 2) on N = 20, F = 300 of the reference chain, whose bound states do not exchange: without A_12 and A_21 the fit
    has the log evidence of the fully connected one to 1e-6 relative, 6 parameters instead of 8 and so the lower BIC --
    first in the oracle, then in the build under test."""
    from tapqir_amd.utils.mle_analysis import hmm_allow, hmm_n_params, hmm_random_starts

    U, B, N, F, iters = 1, 2, 20, 300, 60
    p = em_case()["p"]
    allow = forbid(3, (1, 2), (2, 1))
    free0 = normalised(hmm_random_starts(U, B, 0).numpy(), 3)
    mask0 = normalised(hmm_random_starts(U, B, 0, allow=allow).numpy(), 3)
    assert np.array_equal(free0[0], default_start(U, B)) and mask0[0, 5] == 0 and mask0[0, 7] == 0
    n_free, n_mask = hmm_n_params(hmm_allow(None, 3)), hmm_n_params(hmm_allow(allow, 3))
    assert (n_free, n_mask) == (8, 6)

    def check(ll_free, ll_mask, who):
        print(f"{who}: log evidence {ll_free:.6f} fully connected, {ll_mask:.6f} without 1-2 and 2-1")
        assert abs(ll_free - ll_mask) <= 1e-6 * abs(ll_free)
        assert bic(ll_mask, n_mask, N, F) < bic(ll_free, n_free, N, F)

    th_free = oracle_em_masked(p, PRIOR, free0[0], U, B, iters)[0][-1]
    th_mask = oracle_em_masked(p, PRIOR, mask0[0], U, B, iters, allow)[0][-1]
    check(oracle_loglik(p, PRIOR, th_free, U, B), oracle_loglik(p, PRIOR, th_mask, U, B), "oracle")
    got_free = host_fit(hk, p, PRIOR, free0, U, B, None, num_iter=iters, tol=0.0, chunk=25)
    got_mask = host_fit(hk, p, PRIOR, mask0, U, B, allow, num_iter=iters, tol=0.0, chunk=25)
    check(got_free["logliks"][0], got_mask["logliks"][0], "build under test")
    A = got_mask["thetas"][0, :9].reshape(3, 3)
    assert A[1, 2] <= 1e-9 and A[2, 1] <= 1e-9 and A[1, 0] > 1e-3 and A[2, 0] > 1e-3
    assert rule_excess(got_mask["thetas"][0], th_mask, oracle_em_masked(p, PRIOR, mask0[0], U, B, iters, allow, np.longdouble)[0][-1]) <= 1.0


# ---- the starts -------------------------------------------------------------------------------------------------------------
def test_random_starts_are_reproducible_normalised_and_respect_the_topology():
    from tapqir_amd.utils.mle_analysis import hmm_random_starts

    for U, B in ((1, 2), (2, 2), (1, 3)):
        M = U + B
        s = hmm_random_starts(U, B, 5, seed=3)
        assert s.shape == (6, M * M + M) and s.dtype == torch.float64 and s.device.type == "cpu"
        assert torch.equal(s, hmm_random_starts(U, B, 5, seed=3)) and not torch.equal(s[1:], hmm_random_starts(U, B, 5, seed=4)[1:])
        assert torch.equal(s[:3], hmm_random_starts(U, B, 2, seed=3))  # fewer restarts: a prefix
        assert np.array_equal(s[0].numpy(), default_start(U, B))
        A, rho = s[:, : M * M].reshape(6, M, M).numpy(), s[:, M * M:].numpy()
        assert np.abs(A.sum(2) - 1).max() < 1e-15 and np.abs(rho.sum(1) - 1).max() < 1e-15 and (A > 0).all() and (rho > 0).all()
        leave = 1 - np.diagonal(A[1:], axis1=1, axis2=2)
        assert (leave >= 10 ** -2.5 - 1e-12).all() and (leave <= 10 ** -0.3 + 1e-12).all()
        allow = forbid(M, (M - 1, 0), (0, M - 1))
        t = hmm_random_starts(U, B, 5, seed=3, allow=allow).reshape(6, -1)
        At = t[:, : M * M].reshape(6, M, M).numpy()
        assert (At[:, ~allow] == 0).all() and (At[:, allow] > 0).all() and np.abs(At.sum(2) - 1).max() < 1e-15
    # the generator, spelled out: the first random start of seed 11 at (1, 2)
    rng = np.random.default_rng(11)
    A = np.zeros((3, 3))
    for i in range(3):
        leave = 10 ** rng.uniform(-2.5, -0.3)
        A[i, [j for j in range(3) if j != i]] = leave * rng.dirichlet(np.ones(2))
        A[i, i] = 1 - leave
    want = np.concatenate([A.ravel(), rng.dirichlet(np.ones(3))])
    assert np.array_equal(hmm_random_starts(1, 2, 1, seed=11)[1].numpy(), want)
    # a state with no way out still takes its `leave` draw, so the other rows are those of the free topology
    only = np.array([[True, True, True], [False, True, False], [True, True, True]])
    shut = hmm_random_starts(1, 2, 1, seed=11, allow=only)[1].numpy()
    assert np.array_equal(shut[3:6], [0, 1, 0]) and np.array_equal(shut[:3], want[:3])
    for bad in (dict(restarts=-1), dict(restarts=64), dict(restarts=1, allow=np.ones((2, 2), bool)),
                dict(restarts=1, allow=~np.eye(3, dtype=bool))):
        with pytest.raises(ValueError):
            hmm_random_starts(1, 2, **bad)


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


MIRRORS = {"tq_multistart_estep_args": _lib_multistart.MultistartEstepArgs,
           "tq_multistart_mstep_args": _lib_multistart.MultistartMstepArgs}


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
           + '\n  printf("%d\\n", TQ_MULTISTART_MAX);\n  return 0;\n}\n')
    with tempfile.TemporaryDirectory() as td:
        c = os.path.join(td, "s.c")
        open(c, "w").write(src)
        exe = os.path.join(td, "s")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        got = [int(v) for v in subprocess.check_output([exe]).split()]
    assert got.pop() == _lib_multistart.MULTISTART_MAX == 64
    assert len(got) == len(want)
    assert [(n, f, g) for (n, f, _), g in zip(want, got)] == want


def test_exports_are_the_headers_declarations():
    names = {"tq_multistart_estep", "tq_multistart_mstep"}
    declared = set(re.findall(r"\b(tq_[a-z_0-9]+)\s*\(", header_text()))
    assert {n for n in declared if n.startswith("tq_multistart_")} == names
    assert names == {n for n in _lib.EXPORTS if n.startswith("tq_multistart_")}
    lib = _lib_multistart.lib()
    assert all(hasattr(lib, n) for n in names)


def test_argument_validation_returns_error_codes_without_a_gpu():
    lib = _lib_multistart.lib()
    buf = (ctypes.c_int64 * 8)()
    addr = ctypes.addressof(buf)
    A = _lib_multistart
    calls = {"estep": (lib.tq_multistart_estep, A.MultistartEstepArgs,
                       dict(p=addr, theta=addr, filt=addr, rows=addr, N=3, F=5, R=2, U=1, B=2, prior=0.3)),
             "mstep": (lib.tq_multistart_mstep, A.MultistartMstepArgs,
                       dict(rows=addr, theta=addr, trace=addr, N=3, it=0, T=1, R=2, U=1, B=2, allow=0x1FF))}

    def refused(name, text, **change):
        fn, cls, good = calls[name]
        assert fn(ctypes.byref(cls(**{**good, **change})), None) == 1, (name, change)  # TQ_ERR_ARG
        err = lib.tq_last_error()
        assert ("tq_multistart_" + name).encode() in err and text in err, err

    for name, (fn, cls, good) in calls.items():
        assert fn(None, None) == 1
        assert fn(ctypes.byref(cls()), None) == 1 and b"NULL" in lib.tq_last_error()
        for key, value in good.items():
            if value == addr:
                refused(name, b"NULL", **{key: None})
        refused(name, b"positive", N=0)
        for U, B in ((0, 2), (2, 0), (-1, 3), (1, 4), (3, 2), (4, 1)):
            refused(name, b"U + B at most 4", U=U, B=B)
        for R in (0, -1, 65):
            refused(name, b"at most 64", R=R)
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
    with pytest.raises(HipExtensionError):
        ma.hmm_fit_restarts(p, PRIOR, 1, 2, restarts=2)
    with pytest.raises(HipExtensionError):
        ma.multistart_estep(p, thetas, PRIOR, 1, 2)
    with pytest.raises(HipExtensionError):
        ma.multistart_mstep(torch.rand(2, 3, 13, dtype=torch.float64), thetas, torch.zeros(2, 1, dtype=torch.float64), 0, 1, 2)
    for U, B in ((0, 1), (1, 0), (3, 2), (1, 4)):
        with pytest.raises(ValueError):
            ma.hmm_fit_restarts(p, PRIOR, U, B)
    for bad in (dict(num_iter=0), dict(restarts=64), dict(restarts=-1), dict(starts=torch.ones(2, 11)),
                dict(starts=-torch.ones(2, 12)), dict(starts=torch.zeros(2, 12)), dict(starts=torch.ones(65, 12)),
                dict(allow=torch.ones(2, 2)), dict(allow=1 - torch.eye(3))):
        with pytest.raises(ValueError):
            ma.hmm_fit_restarts(p, PRIOR, 1, 2, **bad)
    assert ma.MULTISTART_SCRATCH_BYTES == 8 * 2**30


# ---- command line -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags,text", [
    (["--restarts", "3", "--cpu"], "more than two states"),
    (["--forbid", "0-1", "--cpu"], "more than two states"),
    (["--restart-seed", "5", "--cpu"], "more than two states"),
    (["--bound-states", "2", "--forbid", "1-1", "--cpu"], "--forbid takes i-j"),
    (["--bound-states", "2", "--forbid", "1-3", "--cpu"], "--forbid takes i-j"),
    (["--bound-states", "2", "--forbid", "12", "--cpu"], "--forbid takes i-j"),
    (["--bound-states", "2", "--forbid", "a-b", "--cpu"], "--forbid takes i-j"),
    (["--bound-states", "2", "--forbid", "1-2", "--forbid", "2-1-0", "--cpu"], "--forbid takes i-j"),
    (["--bound-states", "2", "--restarts", "3", "--forbid", "1-2", "--cpu"], "GPU"),
    (["--bound-states", "2", "--restarts", "3", "--model", "crosstalk"], "cosmos only"),
])
def test_smooth_refusals(tmp_path, flags, text):
    save(simulate(2, 2, 5, 1, 14, params=dict(TEST_PARAMS)), tmp_path)
    result = CliRunner().invoke(app, ["--cd", str(tmp_path), "smooth", *flags, "--num-samples", "10", "--no-input"])
    assert result.exit_code == 1, result.output  # 2 = no such command or option
    assert text in result.output


def test_smooth_restarts_above_63_is_a_usage_error(tmp_path):
    result = CliRunner().invoke(app, ["--cd", str(tmp_path), "smooth", "--bound-states", "2", "--restarts", "64", "--cpu"])
    assert result.exit_code == 2 and "63" in result.output


def test_smooth_help_shows_the_new_options(tmp_path):
    result = CliRunner().invoke(app, ["--cd", str(tmp_path), "smooth", "--help"])
    assert result.exit_code == 0
    for option in ("--restarts", "--restart-seed", "--forbid"):
        assert option in result.output
