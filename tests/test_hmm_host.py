"""Multi-state hidden-Markov smoothing without a GPU: the g++ build of tq_hmm.h (the E-step with
the device's lane ownership and scan order, the M-step, the EM, Viterbi, the backward sampler, the estimate) against the
numpy oracle of hmm_fixture by the tolerance rule of section 20, three anchors that do not share the oracle's code path
(the two-state host check, lumpable chains against the two-state oracle, the closed form of an uninformative row), the
choice of the number of states by BIC, the C layout of the five argument structs, argument validation of the entry points,
and the exits and the help text of ``smooth --unbound-states / --bound-states``."""

import ctypes
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest
import torch
from typer.testing import CliRunner

import smooth_fixture as two
from hmm_fixture import (F_LIST, PRIOR, UB_LIST, bic, build_hmm_check, class_view, cols, default_start, fixed_theta,
                         host_count, host_em, host_estep, host_estimate, host_mstep, host_viterbi, oracle_em, oracle_estep,
                         oracle_estimate, oracle_mstep, oracle_sample, oracle_viterbi, pack, rule_excess, state_pair_counts,
                         synthetic_hmm, with_special_rows)
from rates_fixture import build_rates_check, host_indices, oracle_counts
from tapqir_amd import _lib, _lib_hmm
from tapqir_amd.main import app
from tapqir_amd.utils.dataset import save
from tapqir_amd.utils.simulate import TEST_PARAMS, simulate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RMIN = two.RMIN


@pytest.fixture(scope="module")
def hk(tmp_path_factory):
    return build_hmm_check(tmp_path_factory.mktemp("hmm"))


@pytest.fixture(scope="module")
def hk2(tmp_path_factory):
    return two.build_smooth_check(tmp_path_factory.mktemp("smooth"))


def groups(M):
    """The column groups of ``rows``: expected pair counts, gamma_0, loglik."""
    return (("pairs", slice(0, M * M)), ("gamma0", slice(M * M, M * M + M)), ("loglik", slice(M * M + M, M * M + M + 1)))


def check_rule(got, o64, o80, M, who):
    """filt, gamma and every column group of rows by the rule; prints each excess."""
    for key in ("filt", "gamma"):
        exc = rule_excess(got[key], o64[key], o80[key])
        print(f"{who} {key}: {exc:.3g} of the bound")
        assert exc <= 1.0, (who, key, exc)
    for name, sl in groups(M):
        exc = rule_excess(got["rows"][:, sl], o64["rows"][:, sl], o80["rows"][:, sl])
        print(f"{who} rows/{name}: {exc:.3g} of the bound")
        assert exc <= 1.0, (who, name, exc)


def rule_bound(x64, x80):
    """The bound of the rule: 32 max|X64 - X80| + 1e-13 max(1, max|X80|)."""
    x80 = np.asarray(x80, dtype=np.longdouble)
    return float(32 * np.abs(np.asarray(x64).astype(np.longdouble) - x80).max() + 1e-13 * max(1.0, float(np.abs(x80).max())))


def class_counts(rows, U, M):
    """(N, 4): E n01, E n0, E n10, E n1 at the level of the classes, from the expected state pairs of ``rows``."""
    x = np.asarray(rows)[:, : M * M].reshape(-1, M, M)
    return np.stack([x[:, :U, U:].sum((1, 2)), x[:, :U].sum((1, 2)), x[:, U:, :U].sum((1, 2)), x[:, U:].sum((1, 2))], 1)


# ---- E-step -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("U,B", UB_LIST)
@pytest.mark.parametrize("F", F_LIST)
def test_estep_equals_the_oracle(hk, U, B, F):
    """N = 6: rows of all 0, all 1, alternating 0 / 1 and p = prior, and two rows of the three-state reference chain."""
    M = U + B
    theta = fixed_theta(U, B)
    p = with_special_rows(synthetic_hmm(6, F, seed=F)[0], PRIOR)
    o64, o80 = oracle_estep(p, theta, U, B, PRIOR), oracle_estep(p, theta, U, B, PRIOR, np.longdouble)
    got = host_estep(hk, p, theta, U, B, PRIOR)
    check_rule(got, o64, o80, M, f"({U}, {B}) F = {F}")
    assert np.allclose(got["rows"][:, : M * M].sum(1), F - 1, rtol=0, atol=1e-9 * F)
    assert np.abs(got["gamma"].sum(-1) - 1).max() < 1e-14 and np.abs(got["filt"].sum(-1) - 1).max() < 1e-14
    if F == 1:
        assert not got["rows"][:, : M * M].any()


def test_estep_of_a_long_row(hk):
    """F = 5000 at N = 2 and (2, 2): 79 frames a lane."""
    U, B, F = 2, 2, 5000
    theta = fixed_theta(U, B)
    p = synthetic_hmm(2, F, seed=F)[0]
    got = host_estep(hk, p, theta, U, B, PRIOR)
    check_rule(got, oracle_estep(p, theta, U, B, PRIOR), oracle_estep(p, theta, U, B, PRIOR, np.longdouble), 4, "F = 5000")
    assert np.allclose(got["rows"][:, :16].sum(1), F - 1, rtol=0, atol=1e-9 * F)
    assert np.abs(got["gamma"].sum(-1) - 1).max() < 1e-14


# ---- anchors ----------------------------------------------------------------------------------------------------------
def compare_with_two_state(got, U, B, ref, bound_of, who):
    """The class view of an M-state E-step against a two-state one: filt, gamma, the four class counts, loglik, gamma_0."""
    M = U + B
    pairs = {"filt": (class_view(got["filt"], U), ref["filt"]), "gamma": (class_view(got["gamma"], U), ref["gamma"]),
             "counts": (class_counts(got["rows"], U, M), ref["rows"][:, :4]), "loglik": (got["rows"][:, -1], ref["rows"][:, 4]),
             "gamma0": (got["rows"][:, M * M + U: M * M + M].sum(1), ref["rows"][:, 5])}
    for name, (x, y) in pairs.items():
        err = float(np.abs(np.asarray(x).astype(np.longdouble) - np.asarray(y).astype(np.longdouble)).max())
        print(f"{who} {name}: {err:.3g}, bound {bound_of[name]:.3g}")
        assert err <= bound_of[name], (who, name, err, bound_of[name])


def two_state_bounds(p, theta2, hmm64, hmm80, U, B):
    """Per output, the sum of the two rule bounds: the two-state oracle's and the M-state oracle's, both in class view."""
    M = U + B
    t64, t80 = two.oracle_estep(p, theta2, PRIOR), two.oracle_estep(p, theta2, PRIOR, np.longdouble)

    def view(o, name):
        return {"filt": class_view(o["filt"], U), "gamma": class_view(o["gamma"], U), "counts": class_counts(o["rows"], U, M),
                "loglik": o["rows"][:, -1], "gamma0": o["rows"][:, M * M + U: M * M + M].sum(1)}[name]

    ref = {"filt": lambda o: o["filt"], "gamma": lambda o: o["gamma"], "counts": lambda o: o["rows"][:, :4],
           "loglik": lambda o: o["rows"][:, 4], "gamma0": lambda o: o["rows"][:, 5]}
    return {name: rule_bound(view(hmm64, name), view(hmm80, name)) + rule_bound(ref[name](t64), ref[name](t80))
            for name in ref}, t80


@pytest.mark.parametrize("F", [1, 65, 203])
def test_anchor_two_states_agree_with_the_two_state_build(hk, hk2, F):
    """(a): at (1, 1) the general bodies and the specialised ones of tq_smooth.h compute the same chain."""
    kon, koff, pi0 = 0.05, 0.10, 0.4
    theta = pack([[1 - kon, kon], [koff, 1 - koff]], [1 - pi0, pi0])
    p = with_special_rows(two.synthetic_chain(6, F, seed=F)[0], PRIOR)
    got = host_estep(hk, p, theta, 1, 1, PRIOR)
    ref = two.host_estep(hk2, p, (kon, koff, pi0), PRIOR)
    bounds, _ = two_state_bounds(p, (kon, koff, pi0), oracle_estep(p, theta, 1, 1, PRIOR),
                                 oracle_estep(p, theta, 1, 1, PRIOR, np.longdouble), 1, 1)
    compare_with_two_state(got, 1, 1, ref, bounds, f"(a) F = {F}")


LUMPABLE = {
    # (1, 2): both bound states leave to class 0 with koff; the unbound state splits kon 0.3 : 0.7
    (1, 2): (pack([[0.95, 0.015, 0.035], [0.10, 0.85, 0.05], [0.10, 0.20, 0.70]], [0.6, 0.3, 0.1]), (0.05, 0.10, 0.4)),
    # (2, 1): both unbound states bind with kon; the bound state splits koff 0.25 : 0.75
    (2, 1): (pack([[0.90, 0.05, 0.05], [0.30, 0.65, 0.05], [0.025, 0.075, 0.90]], [0.45, 0.15, 0.4]), (0.05, 0.10, 0.4)),
}


@pytest.mark.parametrize("U,B", sorted(LUMPABLE))
def test_anchor_lumpable_chain_has_two_state_marginals(hk, U, B):
    """(b): when the states of a class leave it with one total probability, the class process is the two-state chain."""
    theta, theta2 = LUMPABLE[U, B]
    p = with_special_rows(two.synthetic_chain(6, 129, seed=5)[0], PRIOR)
    got = host_estep(hk, p, theta, U, B, PRIOR)
    bounds, t80 = two_state_bounds(p, theta2, oracle_estep(p, theta, U, B, PRIOR),
                                   oracle_estep(p, theta, U, B, PRIOR, np.longdouble), U, B)
    compare_with_two_state(got, U, B, t80, bounds, f"(b) ({U}, {B})")


@pytest.mark.parametrize("U,B,F", [(1, 2, 1), (1, 2, 65), (2, 2, 500)])
def test_anchor_uninformative_row_has_closed_forms(hk, U, B, F):
    """(c): p = prior (as the float32 the kernel reads): l = 1, so loglik = 0 and gamma_f = filt_f = rho A^f."""
    M = U + B
    prior = float(np.float32(PRIOR))
    theta = fixed_theta(U, B)
    p = np.full((1, F), prior, np.float32)
    got = host_estep(hk, p, theta, U, B, prior)
    A = theta[: M * M].reshape(M, M).astype(np.longdouble)
    want = [theta[M * M:].astype(np.longdouble)]
    for _ in range(F - 1):
        want.append(want[-1] @ A)
    want = np.array(want)
    o64 = oracle_estep(p, theta, U, B, prior)
    for key in ("gamma", "filt"):
        exc = rule_excess(got[key][0], o64[key][0], want)
        print(f"({U}, {B}) F = {F} {key} against rho A^f: {exc:.3g} of the bound")
        assert exc <= 1.0
    exc = rule_excess(got["rows"][:, -1], o64["rows"][:, -1], np.zeros(1, np.longdouble))
    print(f"loglik = {got['rows'][0, -1]:.3g}: {exc:.3g} of the bound")
    assert exc <= 1.0


# ---- M-step -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("U,B", [(1, 2), (2, 2)])
def test_mstep_quotients_floor_and_unoccupied_state(hk, U, B):
    M = U + B
    rng = np.random.default_rng(1)
    rows = rng.random((300, cols(M)))  # more rows than the 256 threads of the device's workgroup
    rows[:, M * M: M * M + M] /= rows[:, M * M: M * M + M].sum(1, keepdims=True)
    theta0 = fixed_theta(U, B)
    theta, ll, sums = host_mstep(hk, rows, theta0, U, B)
    (t64, l64), (t80, l80) = oracle_mstep(rows, theta0, U, B), oracle_mstep(rows, theta0, U, B, np.longdouble)
    for got, o64, o80 in ((theta, t64, t80), ([ll], [l64], [l80]), (sums, rows.sum(0), rows.astype(np.longdouble).sum(0))):
        assert rule_excess(got, o64, o80) <= 1.0
    assert np.array_equal(host_mstep(hk, rows, theta0, U, B)[0], theta)
    ulp = np.spacing(1.0)
    assert np.abs(theta[: M * M].reshape(M, M).sum(1) - 1).max() <= 4 * ulp and abs(theta[M * M:].sum() - 1) <= 4 * ulp

    def from_sums(pairs, gamma0, N=10):
        theta = np.array(theta0)
        s = np.concatenate([np.asarray(pairs, np.float64).ravel(), np.asarray(gamma0, np.float64), [-7.0]])
        hk.hk_hmm_mstep_theta(s.ctypes.data, N, U, B, theta.ctypes.data)
        return theta[: M * M].reshape(M, M), theta[M * M:]

    pairs = np.arange(1.0, M * M + 1).reshape(M, M)
    pairs[1] = 0.0  # state 1 was never occupied: it keeps its row as it is
    pairs[0] = [4.0] + [0.0] * (M - 1)  # the floor, then the renormalisation
    A, rho = from_sums(pairs, [10.0] + [0.0] * (M - 1))
    assert np.array_equal(A[1], theta0[M: 2 * M])
    floored = np.array([1.0] + [RMIN] * (M - 1))
    assert np.allclose(A[0], floored / floored.sum(), rtol=1e-15, atol=0) and A[0].min() > 0
    assert np.allclose(rho, floored / floored.sum(), rtol=1e-15, atol=0)
    assert np.allclose(A[M - 1], pairs[M - 1] / pairs[M - 1].sum(), rtol=1e-15, atol=0)


# ---- EM ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def em_case():
    """N = 40, F = 500 of the three-state reference chain, seed 0, with the oracle's EM of 25 iterations at (1, 2) from the
    default start in both precisions; shared and left unchanged."""
    p, s = synthetic_hmm(40, 500, seed=0)
    start = default_start(1, 2)
    th64, tr64 = oracle_em(p, PRIOR, start, 1, 2, 25)
    th80, tr80 = oracle_em(p, PRIOR, start, 1, 2, 25, np.longdouble)
    return {"p": p, "s": s, "start": start, "th64": th64, "tr64": tr64, "th80": th80, "tr80": tr80}


def test_default_start_is_the_documented_one():
    from tapqir_amd.utils.mle_analysis import hmm_default_start

    for U, B in UB_LIST:
        A, rho = hmm_default_start(U, B)
        assert np.array_equal(pack(A.numpy(), rho.numpy()), default_start(U, B))
    A = default_start(1, 2)[:9].reshape(3, 3)
    assert np.allclose(1 - np.diag(A), [0.3, 0.3, 0.075]) and np.allclose(A[2, :2], 0.0375)


def test_em_follows_the_oracle(hk, em_case):
    thetas, trace = host_em(hk, em_case["p"], PRIOR, em_case["start"], 1, 2, 25)
    for it in (1, 2, 25):
        exc = rule_excess(thetas[it], em_case["th64"][it], em_case["th80"][it])
        print(f"theta after {it} iterations: {exc:.3g} of the bound")
        assert exc <= 1.0, it
    exc = rule_excess(trace, em_case["tr64"], em_case["tr80"])
    print(f"trace: {exc:.3g} of the bound")
    assert exc <= 1.0
    gain = np.diff(trace)
    print(f"smallest gain of an iteration: {gain.min():.3g}")
    assert (gain >= -1e-12 * np.abs(trace[1:])).all() and trace[-1] > trace[0]


def test_canonical_order_is_a_relabelling(hk, em_case):
    """The order of ``hmm_fit``: within a class by descending A_ii; loglik and the class-level z_probs do not move."""
    from tapqir_amd.utils.mle_analysis import hmm_canonical_order, hmm_permute

    p = em_case["p"][:8]
    for U, B, theta in ((1, 2, em_case["th64"][25]), (2, 2, fixed_theta(2, 2, seed=3)), (1, 3, fixed_theta(1, 3, seed=4))):
        M = U + B
        order = hmm_canonical_order(torch.from_numpy(theta), U, B)
        assert sorted(order[:U]) == list(range(U)) and sorted(order[U:]) == list(range(U, M))
        e = host_estep(hk, p, theta, U, B, PRIOR)
        new = hmm_permute(order, M, **{k: torch.from_numpy(v) for k, v in {"theta": theta, **e}.items()})
        A = new["theta"][: M * M].reshape(M, M).numpy()
        stay = np.diag(A)
        assert (np.diff(stay[:U]) <= 0).all() and (np.diff(stay[U:]) <= 0).all()
        assert np.array_equal(A, theta[: M * M].reshape(M, M)[np.ix_(order, order)])
        again = host_estep(hk, p, new["theta"].numpy(), U, B, PRIOR)
        ll, ll2 = e["rows"][:, -1].sum(), again["rows"][:, -1].sum()
        assert abs(ll - ll2) <= 1e-10 * abs(ll)
        assert np.abs(class_view(again["gamma"], U) - class_view(e["gamma"], U)).max() < 1e-10
        for key in ("filt", "gamma", "rows"):
            assert np.abs(again[key] - new[key].numpy()).max() < 1e-9, key


# ---- Viterbi ----------------------------------------------------------------------------------------------------------
def viterbi_case(U, B):
    """N = 37, F = 203, rows 0-2 special: the first generator seed of 0 .. 9 at which the oracle's smallest decision margin
    exceeds 1e-9."""
    theta = fixed_theta(U, B)
    for seed in range(10):
        p = synthetic_hmm(37, 203, seed=seed)[0]
        p[:3] = with_special_rows(p[:3], PRIOR)
        path, margin = oracle_viterbi(p, theta, U, B, PRIOR)
        if margin > 1e-9:
            return {"p": p, "theta": theta, "path": path, "margin": margin, "seed": seed}
    raise AssertionError("no seed of 0 .. 9 has a decision margin above 1e-9")


@pytest.mark.parametrize("U,B", [(1, 2), (2, 2)])
def test_viterbi_path_is_the_oracles(hk, U, B):
    case = viterbi_case(U, B)
    print(f"({U}, {B}): generator seed {case['seed']}, smallest decision margin {case['margin']:.3g}")
    path = host_viterbi(hk, case["p"], case["theta"], U, B, PRIOR)
    assert path.dtype == np.uint8 and np.array_equal(path, case["path"])
    assert (path[0] < U).all() and (path[1] >= U).all() and path.max() < U + B
    assert len(np.unique(path)) == U + B  # every hidden state is used somewhere


@pytest.mark.parametrize("U,B", [(1, 2), (2, 2)])
@pytest.mark.parametrize("F", [1, 4, 5, 8, 9])
def test_viterbi_word_boundaries(hk, U, B, F):
    """Back-pointers are packed four frames to a word."""
    theta = fixed_theta(U, B)
    p = synthetic_hmm(5, F, seed=F)[0]
    path, margin = oracle_viterbi(p, theta, U, B, PRIOR)
    assert margin > 1e-9
    assert np.array_equal(host_viterbi(hk, p, theta, U, B, PRIOR), path)


# ---- backward sampler ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("U,B", [(1, 2), (2, 2)])
def test_sampler_counts_are_those_of_its_raster(hk, U, B):
    M = U + B
    theta = fixed_theta(U, B)
    p = with_special_rows(synthetic_hmm(7, 131, seed=3)[0], PRIOR)
    filt = host_estep(hk, p, theta, U, B, PRIOR)["filt"]
    counts, trans, raster, margin = host_count(hk, filt, theta, U, B, 71, seed=0)
    print(f"smallest |u - t| at seed 0: {margin:.3g}")
    assert raster.max() < M
    assert np.array_equal(counts, oracle_counts(raster >= U))
    assert np.array_equal(trans, state_pair_counts(raster, M))
    assert (trans.sum(-1) == 130).all() and (counts[..., 1] + counts[..., 3] == 130).all()
    assert (raster[:, 0] < U).all() and (raster[:, 1] >= U).all()
    again = host_count(hk, filt, theta, U, B, 71, seed=0)
    assert np.array_equal(again[2], raster) and not np.array_equal(host_count(hk, filt, theta, U, B, 71, 1)[2], raster)
    one = host_count(hk, filt[:, :1], theta, U, B, 3, seed=0)
    assert not one[0].any() and not one[1].any()


def test_sampler_draws_the_smoothed_law(hk):
    """S = 4096, N = 4, F = 129 at (1, 2), seed 0: the numpy replay of the draws (the exact conditional laws and the
    stream's uniforms) has state frequencies within 5 sigma of gamma, sigma^2 = gamma (1 - gamma) / S, and mean pair counts
    within 5 sigma of the E-step's expectations (sigma from the sample); the g++ replay draws the same rasters."""
    S, N, F, U, B, M = 4096, 4, 129, 1, 2, 3
    theta = fixed_theta(U, B)
    p = with_special_rows(synthetic_hmm(N, F, seed=9)[0], PRIOR)
    e = host_estep(hk, p, theta, U, B, PRIOR)
    replay, margin = oracle_sample(e["filt"], theta, U, B, S, seed=0)
    counts, trans, raster, host_margin = host_count(hk, e["filt"], theta, U, B, S, seed=0)
    print(f"smallest |u - t|: numpy replay {margin:.3g}, g++ replay {host_margin:.3g}")
    assert margin > 1e-9 and np.array_equal(raster, replay)
    for name, ras in (("numpy replay", replay), ("g++ replay", raster)):
        freq = np.stack([(ras == i).mean(0) for i in range(M)], -1)
        sigma = np.sqrt(e["gamma"] * (1 - e["gamma"]) / S)
        dev = np.abs(freq - e["gamma"]) / np.maximum(sigma, 1e-4)
        pairs = state_pair_counts(ras, M)
        dev2 = np.abs(pairs.mean(0) - e["rows"][:, : M * M]) / np.maximum(pairs.std(0) / np.sqrt(S), 1e-3)
        print(f"{name}: state frequencies within {dev.max():.2f} sigma, mean pair counts within {dev2.max():.2f} sigma")
        assert dev.max() < 5.0 and dev2.max() < 5.0


# ---- estimate -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("U,B", [(1, 1), (1, 2), (2, 2)])
def test_estimate_sums_and_quotients(hk, tmp_path_factory, U, B):
    M = U + B
    rng = np.random.default_rng(M)
    S, N = 5, 70
    trans = rng.integers(0, 50, (S, N, M * M)).astype(np.int32)
    trans[2].reshape(N, M, M)[:, 1] = 0  # sample 2 never visits state 1: its row of A is 0 / 0
    totals, est = host_estimate(hk, trans, U, B, 0, 0)
    want_totals, want = oracle_estimate(trans, M)
    assert np.array_equal(totals, want_totals) and np.array_equal(est, want, equal_nan=True)
    assert np.isnan(est[2].reshape(M, M)[1]).all() and np.isfinite(np.delete(est, 2, 0)).all()
    assert np.allclose(est[0].reshape(M, M).sum(1), 1, rtol=0, atol=1e-15)
    idx = host_indices(build_rates_check(tmp_path_factory.mktemp("rates")), 11, S, N)
    totals, est = host_estimate(hk, trans, U, B, 1, 11)
    want_totals, want = oracle_estimate(trans, M, idx)
    assert np.array_equal(totals, want_totals) and np.array_equal(est, want, equal_nan=True)
    assert not np.array_equal(totals, oracle_estimate(trans, M)[0])


# ---- model choice -------------------------------------------------------------------------------------------------------
def bic_table(em, seed, iters=60):
    """BIC after ``iters`` EM iterations from the default start, of (1, 1) and (1, 2), on data of the three-state
    reference chain and of the two-state chain of section 20 (N = 40, F = 500); ``em`` is oracle_em or a host_em."""
    out = {}
    for name, p in (("three", synthetic_hmm(40, 500, seed=seed)[0]), ("two", two.synthetic_chain(40, 500, seed=seed)[0])):
        for U, B in ((1, 1), (1, 2)):
            theta = em(p, PRIOR, default_start(U, B), U, B, iters)[0][-1]
            out[name, B] = (p, theta, U, B)
    return out


def test_bic_chooses_the_number_of_bound_states(hk):
    """The first seed of 0 .. 5 at which the oracle prefers (1, 2) on three-state data and (1, 1) on two-state data; the
    build under test must choose the same."""
    def values(table, estep):
        return {k: bic(estep(p, theta, U, B)["rows"][:, -1].sum(), U + B, 40, 500) for k, (p, theta, U, B) in table.items()}

    for seed in range(6):
        want = values(bic_table(oracle_em, seed), lambda p, th, U, B: oracle_estep(p, th, U, B, PRIOR))
        if want["three", 2] < want["three", 1] and want["two", 1] < want["two", 2]:
            break
    else:
        raise AssertionError("no seed of 0 .. 5 at which the oracle's BIC chooses both models")
    got = values(bic_table(lambda *a: host_em(hk, *a), seed), lambda p, th, U, B: host_estep(hk, p, th, U, B, PRIOR))
    print(f"seed {seed}: oracle {want}, build under test {got}")
    assert got["three", 2] < got["three", 1] and got["two", 1] < got["two", 2]
    for k in want:
        assert abs(got[k] - want[k]) <= 1e-6 * abs(want[k])


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


MIRRORS = {"tq_hmm_estep_args": _lib_hmm.HmmEstepArgs, "tq_hmm_mstep_args": _lib_hmm.HmmMstepArgs,
           "tq_hmm_viterbi_args": _lib_hmm.HmmViterbiArgs, "tq_hmm_count_args": _lib_hmm.HmmCountArgs,
           "tq_hmm_estimate_args": _lib_hmm.HmmEstimateArgs}


def test_struct_layouts_match_the_c_header():
    """sizeof and every offsetof of the five mirrors equal the C compiler's, and the mirrors name the header's fields in
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
           + '\n  printf("%d\\n%d\\n%d\\n", TQ_HMM_MAX_STATES, TQ_HMM_COLS(3), TQ_HMM_COLS(4));\n  return 0;\n}\n')
    with tempfile.TemporaryDirectory() as td:
        c = os.path.join(td, "s.c")
        open(c, "w").write(src)
        exe = os.path.join(td, "s")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        got = [int(v) for v in subprocess.check_output([exe]).split()]
    assert got.pop() == _lib_hmm.hmm_cols(4) == 21
    assert got.pop() == _lib_hmm.hmm_cols(3) == 13
    assert got.pop() == _lib_hmm.HMM_MAX_STATES == 4
    assert len(got) == len(want)
    assert [(n, f, g) for (n, f, _), g in zip(want, got)] == want


def test_exports_are_the_headers_declarations():
    names = {"tq_hmm_estep", "tq_hmm_mstep", "tq_hmm_viterbi", "tq_hmm_count", "tq_hmm_estimate"}
    declared = set(re.findall(r"\b(tq_[a-z_0-9]+)\s*\(", header_text()))
    assert {n for n in declared if n.startswith("tq_hmm_")} == names == {n for n in _lib.EXPORTS if n.startswith("tq_hmm_")}
    assert declared == set(_lib.EXPORTS)
    lib = _lib_hmm.lib()
    assert all(hasattr(lib, n) for n in names)
    assert not any(isinstance(v, type) and issubclass(v, ctypes.Structure) and v.__module__ == _lib_hmm.__name__
                   for v in vars(_lib).values())


def test_argument_validation_returns_error_codes_without_a_gpu():
    lib = _lib_hmm.lib()
    buf = (ctypes.c_int64 * 8)()
    addr = ctypes.addressof(buf) & ~15
    A = _lib_hmm
    calls = {"estep": (lib.tq_hmm_estep, A.HmmEstepArgs,
                       dict(p=addr, theta=addr, filt=addr, gamma=addr, rows=addr, N=3, F=5, U=1, B=2, prior=0.3)),
             "mstep": (lib.tq_hmm_mstep, A.HmmMstepArgs, dict(rows=addr, theta=addr, trace=addr, N=3, it=0, U=1, B=2)),
             "viterbi": (lib.tq_hmm_viterbi, A.HmmViterbiArgs,
                         dict(p=addr, theta=addr, back=addr, path=addr, N=3, F=5, U=1, B=2, prior=0.3)),
             "count": (lib.tq_hmm_count, A.HmmCountArgs, dict(filt=addr, theta=addr, counts=addr, N=3, F=5, S=2, U=1, B=2)),
             "estimate": (lib.tq_hmm_estimate, A.HmmEstimateArgs,
                          dict(trans=addr, totals=addr, estimand=addr, N=3, S=2, U=1, B=2, resample=0))}

    def refused(name, text, **change):
        fn, cls, good = calls[name]
        assert fn(ctypes.byref(cls(**{**good, **change})), None) == 1, (name, change)  # TQ_ERR_ARG
        err = lib.tq_last_error()
        assert ("tq_hmm_" + name).encode() in err and text in err, err

    for name, (fn, cls, good) in calls.items():
        assert fn(None, None) == 1
        assert fn(ctypes.byref(cls()), None) == 1 and b"NULL" in lib.tq_last_error()
        for key, value in good.items():
            if value == addr:
                refused(name, b"NULL", **{key: None})
        refused(name, b"positive", N=0)
        for U, B in ((0, 2), (2, 0), (-1, 3), (1, 4), (3, 2), (4, 1)):
            refused(name, b"U + B at most 4", U=U, B=B)
    for name in ("estep", "viterbi", "count"):
        refused(name, b"positive", F=0)
        refused(name, b"65536", F=65537)
    for name in ("estep", "viterbi"):
        for prior in (0.0, 1.0, -0.5, float("nan")):
            refused(name, b"prior", prior=prior)
    refused("mstep", b"non-negative", it=-1)
    for name in ("count", "estimate"):
        refused(name, b"positive", S=0)
        refused(name, b"S too large", S=65535 * 64 + 1)
    refused("count", b"aligned", counts=addr + 4)
    refused("estimate", b"resample", resample=2)


def test_device_entry_points_refuse_host_tensors_and_bad_shapes():
    from tapqir_amd.exceptions import HipExtensionError
    from tapqir_amd.utils.mle_analysis import (hmm_estep, hmm_estimate, hmm_fit, hmm_mstep, hmm_sample, hmm_summary,
                                               hmm_viterbi)

    theta = torch.from_numpy(fixed_theta(1, 2))
    with pytest.raises(HipExtensionError):
        hmm_estep(torch.rand(3, 5), theta, PRIOR, 1, 2)
    with pytest.raises(HipExtensionError):
        hmm_fit(torch.rand(3, 5), PRIOR, 1, 2)
    with pytest.raises(HipExtensionError):
        hmm_viterbi(torch.rand(3, 5), theta, PRIOR, 1, 2)
    with pytest.raises(HipExtensionError):
        hmm_sample(torch.rand(3, 5, 3, dtype=torch.float64), theta, 1, 2, 4)
    with pytest.raises(HipExtensionError):
        hmm_mstep(torch.rand(3, 13, dtype=torch.float64), theta, torch.zeros(1, dtype=torch.float64), 0, 1, 2)
    with pytest.raises(HipExtensionError):
        hmm_estimate(torch.zeros(2, 3, 9, dtype=torch.int32))
    for U, B in ((0, 1), (1, 0), (3, 2), (1, 4)):
        with pytest.raises(ValueError):
            hmm_fit(torch.rand(3, 5), PRIOR, U, B)
    with pytest.raises(ValueError):
        hmm_fit(torch.rand(3, 5), PRIOR, 1, 2, A0=torch.ones(2, 2))
    with pytest.raises(ValueError):
        hmm_fit(torch.rand(3, 5), PRIOR, 1, 2, num_iter=0)
    est = {"A": torch.tensor([[[0.9, 0.1], [0.2, 0.8]], [[0.7, 0.3], [float("nan"), float("nan")]]], dtype=torch.float64)}
    summary = hmm_summary(est, 0.5)
    assert sorted(summary) == ["A00", "A01", "A10", "A11"]
    assert summary["A00"]["mean"] == pytest.approx(0.8) and summary["A00"]["left_out"] == 0
    assert summary["A10"]["mean"] == pytest.approx(0.2) and summary["A10"]["left_out"] == 1


# ---- command line -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags,text", [(["--bound-states", "2", "--cpu"], "GPU"),
                                        (["--bound-states", "2", "--model", "crosstalk"], "cosmos only"),
                                        (["--bound-states", "4"], "at most 4"),
                                        (["--unbound-states", "3", "--bound-states", "2", "--cpu"], "at most 4")])
def test_smooth_refusals(tmp_path, flags, text):
    save(simulate(2, 2, 5, 1, 14, params=dict(TEST_PARAMS)), tmp_path)
    result = CliRunner().invoke(app, ["--cd", str(tmp_path), "smooth", *flags, "--num-samples", "10", "--no-input"])
    assert result.exit_code == 1, result.output  # 2 = no such command or option
    assert text in result.output


def test_smooth_help_shows_the_new_options(tmp_path):
    result = CliRunner().invoke(app, ["--cd", str(tmp_path), "smooth", "--help"])
    assert result.exit_code == 0 and "--unbound-states" in result.output and "--bound-states" in result.output
