"""Two colour channels as one chain without a GPU: the g++ build of tq_joint.h (the batched E-step
with the device's lane ownership and scan order, the M-step under the five structures, the Viterbi path) against the numpy
oracle of joint_fixture by the tolerance rule of section 20; the Kronecker anchor against the two-state oracle, the channel
swap, the EM and the choice of a structure by BIC driven through ``multistart_em`` on that build, the unchanged sampler on
the joint ``filt``, ``joint_rates``, the C layout of the three argument structs, the exports, argument validation of the
entry points, and the exits and the help text of ``smooth --joint``."""

import ctypes
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest
import torch
from typer.testing import CliRunner

import hmm_fixture
import smooth_fixture as two
from joint_fixture import (A_DRIVEN, COLS, F_LIST, M, N_PARAMS, NAMES, PRIORS, SWAP, build_joint_check, default_start, em_case,
                           estep_inputs, fixed_theta, hand_rates, host_estep, host_fit, host_mstep, host_viterbi, oracle_estep,
                           oracle_mstep, oracle_mstep_sums, oracle_viterbi, realised_matrix, rule_bound, rule_excess,
                           selection_case, start_from, swap_rows, swap_theta, synthetic_joint)
from tapqir_amd import _lib, _lib_joint
from tapqir_amd.main import app
from tapqir_amd.utils.dataset import save
from tapqir_amd.utils.simulate import TEST_PARAMS, simulate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GROUPS = (("pairs", slice(0, 16)), ("gamma0", slice(16, 20)), ("loglik", slice(20, 21)))
VITERBI_SEEDS = {203: 203, 1: 1, 4: 4, 5: 5, 8: 8, 9: 9}  # seeds of the Viterbi inputs, chosen for a margin above 1e-9


@pytest.fixture(scope="module")
def hk(tmp_path_factory):
    return build_joint_check(tmp_path_factory.mktemp("joint"))


def check_rule(got, o64, o80, who, keys=("filt", "gamma")):
    """filt, gamma and every column group of rows of one replica by the rule; prints each excess, returns the largest."""
    worst = 0.0
    for key in keys:
        exc = rule_excess(got[key], o64[key], o80[key])
        print(f"{who} {key}: {exc:.3g} of the bound")
        assert exc <= 1.0, (who, key, exc)
        worst = max(worst, exc)
    for name, sl in GROUPS:
        exc = rule_excess(got["rows"][..., sl], o64["rows"][..., sl], o80["rows"][..., sl])
        print(f"{who} rows/{name}: {exc:.3g} of the bound")
        assert exc <= 1.0, (who, name, exc)
        worst = max(worst, exc)
    return worst


def replica(out, r):
    return {k: v[r] for k, v in out.items()}


# ---- E-step -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,F", [(6, F) for F in F_LIST] + [(2, 5000)])
def test_estep_equals_the_oracle(hk, N, F):
    """Every pairing of all 0 / all 1 / alternating / p = prior with a neighbour, at a fully connected theta."""
    theta = fixed_theta()
    pa, pb = estep_inputs(N, F, seed=F)
    o64, o80 = oracle_estep(pa, pb, theta), oracle_estep(pa, pb, theta, dtype=np.longdouble)
    got = replica(host_estep(hk, pa, pb, theta[None]), 0)
    check_rule(got, o64, o80, f"N = {N}, F = {F}")
    assert np.allclose(got["rows"][:, :16].sum(1), F - 1, rtol=0, atol=1e-9 * F)
    assert np.abs(got["gamma"].sum(-1) - 1).max() < 1e-14 and np.abs(got["filt"].sum(-1) - 1).max() < 1e-14
    if F == 1:
        assert not got["rows"][:, :16].any()
    again = replica(host_estep(hk, pa, pb, theta[None]), 0)
    assert all(np.array_equal(again[k], got[k]) for k in got)


@pytest.mark.parametrize("F", [1, 65, 203])
def test_estep_replicas_inactive_and_without_gamma(hk, F):
    """R = 3 with the middle replica inactive: its outputs keep the NaN sentinel, the outer two have the bits of their own
    R = 1 runs; without gamma the rows have the same bits."""
    thetas = np.array([fixed_theta(seed=r) for r in range(3)])
    pa, pb = estep_inputs(6, F, seed=F)
    got = host_estep(hk, pa, pb, thetas, active=[1, 0, 1])
    assert all(np.isnan(got[k][1]).all() for k in got)
    for r in (0, 2):
        alone = host_estep(hk, pa, pb, thetas[r:r + 1])
        assert all(np.array_equal(alone[k][0], got[k][r]) for k in got), r
    bare = host_estep(hk, pa, pb, thetas, gamma=False)
    full = host_estep(hk, pa, pb, thetas)
    assert "gamma" not in bare and np.array_equal(bare["rows"], full["rows"]) and np.array_equal(bare["filt"], full["filt"])


# ---- anchors ----------------------------------------------------------------------------------------------------------
def marginal(x, channel):
    """p(z_c = 1) of (..., 4) joint state probabilities: channel 0 is a, 1 is b."""
    x = np.asarray(x)
    return x[..., 1] + x[..., 3] if channel == 0 else x[..., 2] + x[..., 3]


def check_kronecker(got, pa, pb, theta_a, theta_b, priors, who, refs=None):
    """The joint E-step at kron(theta_b, theta_a) against the two two-state oracles (long double): the row log evidence is
    the sum of theirs and the channel marginals of filt and gamma are theirs, each within the sum of the rule bounds of the
    oracles compared.  ``refs`` replaces the two-state long-double oracles as the values compared against."""
    theta = start_from(theta_a, theta_b)
    j64, j80 = oracle_estep(pa, pb, theta, priors), oracle_estep(pa, pb, theta, priors, np.longdouble)
    t64 = [two.oracle_estep(p, t, pr) for p, t, pr in ((pa, theta_a, priors[0]), (pb, theta_b, priors[1]))]
    t80 = [two.oracle_estep(p, t, pr, np.longdouble) for p, t, pr in ((pa, theta_a, priors[0]), (pb, theta_b, priors[1]))]
    refs = t80 if refs is None else refs
    bound = rule_bound(j64["rows"][:, -1], j80["rows"][:, -1]) + sum(rule_bound(t64[c]["rows"][:, 4], t80[c]["rows"][:, 4]) for c in (0, 1))
    want = np.asarray(refs[0]["rows"][:, 4]).astype(np.longdouble) + np.asarray(refs[1]["rows"][:, 4]).astype(np.longdouble)
    err = float(np.abs(got["rows"][:, -1].astype(np.longdouble) - want).max())
    print(f"{who} loglik: {err:.3g}, bound {bound:.3g}")
    assert err <= bound
    for c in (0, 1):
        for key in ("filt", "gamma"):
            bound = rule_bound(marginal(j64[key], c), marginal(j80[key], c)) + rule_bound(t64[c][key], t80[c][key])
            err = float(np.abs(marginal(got[key], c).astype(np.longdouble) - np.asarray(refs[c][key]).astype(np.longdouble)).max())
            print(f"{who} {key} of channel {'ab'[c]}: {err:.3g}, bound {bound:.3g}")
            assert err <= bound, (who, key, c)


@pytest.mark.parametrize("F", [1, 65, 203])
def test_anchor_kronecker_start_is_two_independent_chains(hk, F):
    from tapqir_amd.utils.joint_analysis import joint_default_start, joint_start_from

    theta_a, theta_b, priors = (0.05, 0.10, 0.4), (0.03, 0.20, 0.25), (1.0 / 3.0, 0.2)
    assert np.allclose(joint_start_from(theta_a, theta_b).numpy(), start_from(theta_a, theta_b), rtol=0, atol=1e-16)
    assert np.allclose(joint_default_start().numpy(), default_start(), rtol=0, atol=1e-16)
    pa, pb = estep_inputs(6, F, seed=F)
    got = replica(host_estep(hk, pa, pb, start_from(theta_a, theta_b)[None], priors), 0)
    check_kronecker(got, pa, pb, theta_a, theta_b, priors, f"F = {F}")


@pytest.mark.parametrize("F", [1, 65, 203])
def test_channel_swap_permutes_the_states(hk, F):
    """(p_a, prior_a) exchanged with (p_b, prior_b) and the states 1 and 2 exchanged in theta: the outputs are those of the
    original with the states 1 and 2 exchanged, by the rule against the original's oracle."""
    theta, priors = fixed_theta(seed=1), (1.0 / 3.0, 0.2)
    pa, pb = estep_inputs(6, F, seed=F)
    o64, o80 = oracle_estep(pa, pb, theta, priors), oracle_estep(pa, pb, theta, priors, np.longdouble)
    got = replica(host_estep(hk, pb, pa, swap_theta(theta)[None], priors[::-1]), 0)
    back = {"filt": got["filt"][..., SWAP], "gamma": got["gamma"][..., SWAP], "rows": swap_rows(got["rows"])}
    check_rule(back, o64, o80, f"swapped, F = {F}")
    assert np.array_equal(swap_theta(swap_theta(theta)), theta)


# ---- M-step -----------------------------------------------------------------------------------------------------------
def mstep_case():
    rng = np.random.default_rng(3)
    rows = rng.random((5, 300, COLS))  # more rows than the 256 threads of the device's workgroup
    rows[:, :, 16:20] /= rows[:, :, 16:20].sum(2, keepdims=True)
    return rows, np.array([fixed_theta(seed=r) for r in range(5)])


def check_structure_identities(thetas, tol=1e-12):
    """The identities a structure puts on A, relative; returns the largest residual seen."""
    worst = 0.0
    A = thetas[:, :16].reshape(-1, 4, 4)
    ulp = np.spacing(1.0)
    assert np.abs(A.sum(2) - 1).max() <= 4 * ulp and np.abs(thetas[:, 16:].sum(1) - 1).max() <= 4 * ulp

    def rel(x, y):
        return float(np.abs(np.asarray(x) - np.asarray(y)).max() / np.abs(y).max())

    # coupled (and everything nested in it): no concerted events beyond chance
    for k in (0, 1, 2, 3):
        worst = max(worst, max(rel(A[k][s, 0] * A[k][s, 3], A[k][s, 1] * A[k][s, 2]) for s in range(4)))
    # independent: the Kronecker product of its own margins
    Pa = np.array([[A[0][za, 0] + A[0][za, 2], A[0][za, 1] + A[0][za, 3]] for za in (0, 1)])
    Pb = np.array([[A[0][2 * zb, 0] + A[0][2 * zb, 1], A[0][2 * zb, 2] + A[0][2 * zb, 3]] for zb in (0, 1)])
    worst = max(worst, rel(A[0], np.kron(Pb, Pa)))
    # a-drives-b: P_a read off rows (z_a, 0) and (z_a, 1) agree; b-drives-a: the mirror image
    for za in (0, 1):
        worst = max(worst, rel(A[1][za, 1] + A[1][za, 3], A[1][za + 2, 1] + A[1][za + 2, 3]))
    for zb in (0, 1):
        worst = max(worst, rel(A[2][2 * zb, 2] + A[2][2 * zb, 3], A[2][2 * zb + 1, 2] + A[2][2 * zb + 1, 3]))
    print(f"largest relative residual of a structural identity: {worst:.3g}")
    assert worst <= tol
    return worst


def test_mstep_of_the_five_structures(hk, tmp_path_factory):
    """N = 300, all five structures in one launch.  Measured on the g++ build: the identities hold to 2.6e-16 relative."""
    rows, theta0 = mstep_case()
    thetas, trace = theta0.copy(), np.full((5, 3), np.nan)
    host_mstep(hk, rows, thetas, trace, 1, range(5))
    for k in range(5):
        (t64, l64), (t80, l80) = oracle_mstep(rows[k], theta0[k], k), oracle_mstep(rows[k], theta0[k], k, np.longdouble)
        exc = rule_excess(thetas[k], t64, t80), rule_excess([trace[k, 1]], [l64], [l80])
        print(f"{NAMES[k]}: theta {exc[0]:.3g}, loglik {exc[1]:.3g} of the bound")
        assert max(exc) <= 1.0, k
    assert np.isnan(trace[:, [0, 2]]).all()
    check_structure_identities(thetas)
    # full is the M-step of the chain of four states, bit for bit
    hmm = hmm_fixture.build_hmm_check(tmp_path_factory.mktemp("hmm"))
    want, ll, _ = hmm_fixture.host_mstep(hmm, rows[4], theta0[4], 2, 2)
    assert np.array_equal(thetas[4], want) and trace[4, 1] == ll
    again, trace2 = theta0.copy(), np.zeros((5, 3))
    host_mstep(hk, rows, again, trace2, 1, range(5))
    assert np.array_equal(again, thetas) and np.array_equal(trace2[:, 1], trace[:, 1])
    frozen, trace3 = theta0.copy(), np.full((5, 3), np.nan)
    host_mstep(hk, rows, frozen, trace3, 1, range(5), active=[1, 1, 0, 1, 1])
    assert np.array_equal(frozen[2], theta0[2]) and np.isnan(trace3[2]).all()
    assert np.array_equal(frozen[[0, 1, 3, 4]], thetas[[0, 1, 3, 4]])


def test_mstep_keeps_a_row_without_occupancy(hk):
    """A row whose denominator -- for a pooled factor, the pooled denominator -- is zero keeps its old values."""
    theta0 = fixed_theta()
    pairs = np.arange(1.0, 17.0).reshape(4, 4)
    pairs[1] = 0.0

    def run(pairs, k):
        theta = theta0.copy()
        s = np.concatenate([pairs.ravel(), [4.0, 3.0, 2.0, 1.0], [-7.0]])
        hk.hk_joint_mstep_theta(s.ctypes.data, 10, k, theta.ctypes.data)
        want = oracle_mstep_sums(s, 10, theta0, k)[0]
        assert np.allclose(theta, want, rtol=1e-14, atol=0), k
        return theta[:16].reshape(4, 4), theta[16:]

    old = theta0[:16].reshape(4, 4)
    for k in (3, 4):  # per-state denominators only: state 1 keeps its row
        A, rho = run(pairs, k)
        assert np.array_equal(A[1], old[1]) and not np.array_equal(A[0], old[0])
        assert np.allclose(rho, [0.4, 0.3, 0.2, 0.1], rtol=1e-15)
    A, _ = run(pairs, 0)  # both factors pooled with a partner that is occupied: state 1 is updated
    assert not np.array_equal(A[1], old[1])
    A, _ = run(pairs, 1)  # P_b(. | z_a = 1, z_b = 0) has no count: state 1 keeps its row, state 3 is updated
    assert np.array_equal(A[1], old[1]) and not np.array_equal(A[3], old[3])
    both = pairs.copy()
    both[3] = 0.0  # z_a = 1 never occupied: the pooled denominator of P_a(. | z_a = 1) is zero
    for k in range(5):
        A, _ = run(both, k)
        assert np.array_equal(A[[1, 3]], old[[1, 3]]) and not np.array_equal(A[0], old[0]) and not np.array_equal(A[2], old[2])
    for k in range(5):
        assert hk.hk_joint_structure_ok(k) == 1
    assert hk.hk_joint_structure_ok(-1) == 0 and hk.hk_joint_structure_ok(5) == 0


# ---- EM -----------------------------------------------------------------------------------------------------------------
def test_em_follows_the_oracle_under_every_structure(hk):
    """The driven chain, N = 40, F = 500, seed 0, from the default start: 25 iterations in chunks of 10, 10 and 5."""
    case = em_case()
    fit = host_fit(hk, case["pa"], case["pb"], num_iter=25, tol=0.0, chunk=10)
    assert fit["iterations"] == [25] * 5
    for k in range(5):
        exc = (rule_excess(fit["thetas"][k], case["th64"][k][25], case["th80"][k][25]),
               rule_excess(fit["traces"][k], case["tr64"][k], case["tr80"][k]))
        print(f"{NAMES[k]}: theta after 25 iterations {exc[0]:.3g}, trace {exc[1]:.3g} of the bound")
        assert max(exc) <= 1.0, k
        gain = np.diff(fit["traces"][k])
        assert (gain >= -1e-12 * np.abs(fit["traces"][k][1:])).all(), (k, gain.min())
    whole = host_fit(hk, case["pa"], case["pb"], num_iter=25, tol=0.0, chunk=25)
    assert np.array_equal(whole["thetas"], fit["thetas"]) and np.array_equal(whole["traces"], fit["traces"])
    check_structure_identities(fit["thetas"])


# ---- selection ------------------------------------------------------------------------------------------------------------
WANT = {"independent": 0, "driven": 1, "driven-swapped": 2}


def check_ladder(logliks, who):
    ll = np.asarray(logliks, np.float64)
    slack = 1e-6 * np.abs(ll).max()
    print(f"{who}: log evidence " + ", ".join(f"{NAMES[k]} {ll[k]:.4f}" for k in range(5)))
    assert ll[0] <= min(ll[1], ll[2]) + slack and max(ll[1], ll[2]) <= ll[3] + slack and ll[4] >= ll[0] - slack


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("kind", sorted(WANT))
def test_bic_chooses_the_generating_structure(hk, kind, seed):
    """60 iterations from the default start, N = 40, F = 500.  First the numpy oracle alone: it makes the choice with a BIC
    margin above 10 (measured: 15.7 at the least); then the build under test."""
    case = selection_case(kind, seed)
    bics = np.array(case["bics"])
    order = np.argsort(bics)
    print(f"{kind} seed {seed}: oracle chooses {NAMES[order[0]]}, {NAMES[order[1]]} is {bics[order[1]] - bics[order[0]]:.2f} worse")
    assert order[0] == WANT[kind] and bics[order[1]] - bics[order[0]] > 10.0
    check_ladder(case["logliks"], "oracle")
    fit = host_fit(hk, case["pa"], case["pb"], num_iter=60, tol=0.0, chunk=50)
    assert fit["best"] == WANT[kind] and fit["n_params"] == list(N_PARAMS)
    check_ladder(fit["logliks"], "build under test")
    if kind == "driven" and seed == 0:
        from tapqir_amd.utils.joint_analysis import joint_rates

        A = fit["thetas"][1, :16].reshape(4, 4)
        got, real, true = joint_rates(torch.from_numpy(A)), hand_rates(realised_matrix(case["states"])), hand_rates(A_DRIVEN)
        for name in ("kon_b|a0", "kon_b|a1", "kon_b ratio", "koff_b|a0", "koff_b|a1", "kon_a|b0", "koff_a|b0"):
            print(f"{name}: generating {true[name]:.4g}, realised {real[name]:.4g}, fitted {got[name].item():.4g}")
        assert got["kon_b ratio"].item() > 5.0


# ---- Viterbi ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", sorted(VITERBI_SEEDS))
def test_viterbi_equals_the_oracle(hk, F):
    """N = 37.  Smallest decision margins of the oracle at these seeds: above 1e-5 (asserted above 1e-9)."""
    theta = fixed_theta()
    pa, pb, _ = synthetic_joint(37, F, VITERBI_SEEDS[F], A_DRIVEN)
    want, margin = oracle_viterbi(pa, pb, theta)
    print(f"F = {F}: smallest decision margin {margin:.3g}")
    assert margin > 1e-9
    got = host_viterbi(hk, pa, pb, theta)
    assert np.array_equal(got, want)


# ---- the unchanged sampler on the joint filt ------------------------------------------------------------------------------
def test_sampler_draws_the_joint_smoothed_law(hk, tmp_path_factory):
    """S = 4096, N = 4, F = 129: the g++ replay of tq_hmm_count at (2, 2) on the joint filt has state frequencies within 5
    sigma of the joint gamma and mean pair counts within 5 sigma of rows[:, :16]."""
    S, N, F = 4096, 4, 129
    theta = fixed_theta()
    pa, pb = estep_inputs(N, F, seed=9)
    e = replica(host_estep(hk, pa, pb, theta[None]), 0)
    hmm = hmm_fixture.build_hmm_check(tmp_path_factory.mktemp("hmm"))
    _, trans, raster, _ = hmm_fixture.host_count(hmm, e["filt"], theta, 2, 2, S, seed=0)
    freq = np.stack([(raster == i).mean(0) for i in range(M)], -1)
    dev1 = np.abs(freq - e["gamma"]) / np.maximum(np.sqrt(e["gamma"] * (1 - e["gamma"]) / S), 1e-4)
    pairs = trans.astype(np.float64)
    dev2 = np.abs(pairs.mean(0) - e["rows"][:, :16]) / np.maximum(pairs.std(0) / np.sqrt(S), 1e-3)
    print(f"state frequencies within {dev1.max():.2f} sigma, mean pair counts within {dev2.max():.2f} sigma")
    assert dev1.max() < 5.0 and dev2.max() < 5.0


# ---- joint_rates ----------------------------------------------------------------------------------------------------------
def test_joint_rates_are_the_sums_and_quotients():
    from tapqir_amd.utils.joint_analysis import RATE_NAMES, RATIO_NAMES, joint_rates

    rng = np.random.default_rng(4)
    A = rng.random((3, 2, 4, 4))
    A /= A.sum(-1, keepdims=True)
    got = joint_rates(torch.from_numpy(A[0, 0]))
    want = hand_rates(A[0, 0])
    assert list(got) == list(RATE_NAMES + RATIO_NAMES) == list(want)
    for name in want:
        assert got[name].shape == () and abs(got[name].item() - want[name]) <= 1e-15 * abs(want[name]), name
    A[1, 1, 2] = np.nan
    batch = joint_rates(torch.from_numpy(A))
    for i in range(3):
        for j in range(2):
            want = hand_rates(A[i, j])
            for name in want:
                assert batch[name].shape == (3, 2)
                assert np.isclose(batch[name][i, j].item(), want[name], rtol=1e-15, atol=0, equal_nan=True), (name, i, j)
    for name in ("kon_a|b1", "koff_b|a0", "kon_a ratio", "koff_b ratio"):  # what reads row 2
        assert torch.isnan(batch[name][1, 1])
    for name in ("kon_a|b0", "kon_b|a1", "koff_a|b1", "kon_b ratio"):
        assert torch.isfinite(batch[name][1, 1])
    with pytest.raises(ValueError):
        joint_rates(torch.zeros(3, 3))


# ---- ABI ------------------------------------------------------------------------------------------------------------
def header_text():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tapqir_hip.h")).read(), flags=re.S)


def header_fields(name):
    """Field names of ``typedef struct { ... } name;`` in include/tapqir_hip.h, in order (an array's name without its
    extent)."""
    body = re.search(r"typedef struct \{([^{}]*)\}\s*%s;" % name, header_text()).group(1)
    out = []
    for decl in body.split(";"):
        if decl.strip():
            out += [re.search(r"(\w+)\s*(\[[^\]]*\]\s*)*$", d.strip()).group(1) for d in decl.split(",")]
    return out


MIRRORS = {"tq_joint_estep_args": _lib_joint.JointEstepArgs, "tq_joint_mstep_args": _lib_joint.JointMstepArgs,
           "tq_joint_viterbi_args": _lib_joint.JointViterbiArgs}
CONSTANTS = ("TQ_JOINT_INDEPENDENT", "TQ_JOINT_A_DRIVES_B", "TQ_JOINT_B_DRIVES_A", "TQ_JOINT_COUPLED", "TQ_JOINT_FULL")


def test_struct_layouts_and_constants_match_the_c_header():
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
    tail = "".join('  printf("%%d\\n", %s);\n' % c for c in CONSTANTS + ("TQ_MULTISTART_MAX", "TQ_HMM_COLS(4)"))
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "tapqir_hip.h"\nint main(void) {\n' + "\n".join(lines) + "\n"
           + tail + '  printf("%zu\\n", sizeof(((tq_joint_mstep_args*)0)->structure));\n  return 0;\n}\n')
    with tempfile.TemporaryDirectory() as td:
        c = os.path.join(td, "s.c")
        open(c, "w").write(src)
        exe = os.path.join(td, "s")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        got = [int(v) for v in subprocess.check_output([exe]).split()]
    assert got.pop() == _lib_joint.JointMstepArgs.structure.size == 4 * 64
    assert got[-7:] == [_lib_joint.JOINT_INDEPENDENT, _lib_joint.JOINT_A_DRIVES_B, _lib_joint.JOINT_B_DRIVES_A,
                        _lib_joint.JOINT_COUPLED, _lib_joint.JOINT_FULL, 64, _lib_joint.JOINT_COLS] == [0, 1, 2, 3, 4, 64, 21]
    got = got[:-7]
    assert len(got) == len(want)
    assert [(n, f, g) for (n, f, _), g in zip(want, got)] == want
    assert [name for name, _ in _lib_joint.STRUCTURES] == list(NAMES)
    assert [k + 3 for _, k in _lib_joint.STRUCTURES] == list(N_PARAMS)


def test_exports_are_the_headers_declarations():
    names = {"tq_joint_estep", "tq_joint_mstep", "tq_joint_viterbi"}
    declared = set(re.findall(r"\b(tq_[a-z_0-9]+)\s*\(", header_text()))
    assert {n for n in declared if n.startswith("tq_joint_")} == names
    assert names == {n for n in _lib.EXPORTS if n.startswith("tq_joint_")}
    lib = _lib_joint.lib()
    assert all(hasattr(lib, n) for n in names)


def test_argument_validation_returns_error_codes_without_a_gpu():
    lib = _lib_joint.lib()
    buf = (ctypes.c_int64 * 8)()
    addr = ctypes.addressof(buf)
    A = _lib_joint
    calls = {"estep": (lib.tq_joint_estep, A.JointEstepArgs,
                       dict(p_a=addr, p_b=addr, theta=addr, filt=addr, gamma=addr, rows=addr, N=3, F=5, R=2, prior_a=0.3, prior_b=0.4)),
             "mstep": (lib.tq_joint_mstep, A.JointMstepArgs,
                       dict(rows=addr, theta=addr, trace=addr, N=3, it=0, T=1, R=2, structure=A.structure_array([0, 4]))),
             "viterbi": (lib.tq_joint_viterbi, A.JointViterbiArgs,
                         dict(p_a=addr, p_b=addr, theta=addr, back=addr, path=addr, N=3, F=5, prior_a=0.3, prior_b=0.4))}
    optional = {"gamma", "active"}

    def refused(name, text, **change):
        fn, cls, good = calls[name]
        assert fn(ctypes.byref(cls(**{**good, **change})), None) == 1, (name, change)  # TQ_ERR_ARG
        err = lib.tq_last_error()
        assert ("tq_joint_" + name).encode() in err and text in err, err

    for name, (fn, cls, good) in calls.items():
        assert fn(None, None) == 1
        assert fn(ctypes.byref(cls()), None) == 1 and b"NULL" in lib.tq_last_error()
        for key, value in good.items():
            if value == addr and key not in optional:
                refused(name, b"NULL", **{key: None})
        refused(name, b"positive", N=0)
        refused(name, b"positive", N=-1)
    for name in ("estep", "viterbi"):
        refused(name, b"positive", F=0)
        refused(name, b"65536", F=65537)
        for prior in (0.0, 1.0, -0.5, float("nan")):
            refused(name, b"prior", prior_a=prior)
            refused(name, b"prior", prior_b=prior)
    for name in ("estep", "mstep"):
        for R in (0, -1, 65):
            refused(name, b"at most 64", R=R)
    refused("mstep", b"non-negative", it=-1)
    refused("mstep", b"T must exceed it", it=1, T=1)
    refused("mstep", b"T must exceed it", it=0, T=0)
    refused("mstep", b"structure", structure=A.structure_array([0, 5]))
    refused("mstep", b"structure", structure=A.structure_array([-1, 0]))
    assert [int(v) for v in A.structure_array([3, 1])[:3]] == [3, 1, 0]


def test_device_entry_points_refuse_host_tensors_and_bad_arguments():
    from tapqir_amd.exceptions import HipExtensionError
    from tapqir_amd.utils import joint_analysis as ja

    p = torch.rand(3, 5)
    thetas = torch.from_numpy(np.array([fixed_theta(seed=r) for r in range(2)]))
    with pytest.raises(HipExtensionError):
        ja.joint_estep(p, p, thetas, 0.3, 0.3)
    with pytest.raises(HipExtensionError):
        ja.joint_mstep(torch.rand(2, 3, 21, dtype=torch.float64), thetas, torch.zeros(2, 1, dtype=torch.float64), 0, [0, 1])
    with pytest.raises(HipExtensionError):
        ja.joint_viterbi(p, p, thetas[0], 0.3, 0.3)
    with pytest.raises(HipExtensionError):
        ja.joint_fit(p, p, 0.3, 0.3)
    for bad in (dict(num_iter=0), dict(structures=[]), dict(structures=["full", 4]), dict(structures=["nope"]),
                dict(structures=[5]), dict(start=torch.ones(19)), dict(start=-torch.ones(20)), dict(start=torch.zeros(20)),
                dict(structures=[0, 1], choose="full")):
        with pytest.raises(ValueError):
            ja.joint_fit(p, p, 0.3, 0.3, **bad)
    assert [ja.joint_n_params(s) for s in ja.STRUCTURE_NAMES] == list(N_PARAMS)
    assert ja.joint_select([-10.0, -10.0, -9.0], [0, 1, 4], 10, 10)[2] == 0  # a tie of the BIC goes to the lowest id
    assert ja.joint_select([-10.0, -1.0], [0, 1], 10, 10)[2] == 1


# ---- command line -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags,text", [
    (["--joint", "0", "--cpu"], "--joint takes A,B"),
    (["--joint", "0,1,2", "--cpu"], "--joint takes A,B"),
    (["--joint", "a,b", "--cpu"], "--joint takes A,B"),
    (["--joint", "1,1", "--cpu"], "--joint takes A,B"),
    (["--joint", "0,1", "--bound-states", "2", "--cpu"], "1 and 1"),
    (["--joint", "0,1", "--unbound-states", "2", "--cpu"], "1 and 1"),
    (["--joint", "0,1", "--restarts", "3", "--cpu"], "--restarts"),
    (["--joint", "0,1", "--restart-seed", "5", "--cpu"], "--restarts"),
    (["--joint", "0,1", "--forbid", "0-1", "--cpu"], "--restarts"),
    (["--structure", "full", "--cpu"], "--structure needs --joint"),
    (["--structure", "auto", "--cpu"], "--structure needs --joint"),
    (["--joint", "0,1", "--structure", "nope", "--cpu"], "--structure takes"),
    (["--joint", "0,1", "--cpu"], "GPU"),
    (["--joint", "0,1", "--model", "crosstalk"], "cosmos only"),
])
def test_smooth_joint_refusals(tmp_path, flags, text):
    save(simulate(2, 2, 5, 1, 14, params=dict(TEST_PARAMS)), tmp_path)
    result = CliRunner().invoke(app, ["--cd", str(tmp_path), "smooth", *flags, "--num-samples", "10", "--no-input"])
    assert result.exit_code == 1, result.output  # 2 = no such command or option
    assert text in result.output


def test_smooth_help_shows_the_new_options(tmp_path):
    result = CliRunner().invoke(app, ["--cd", str(tmp_path), "smooth", "--help"])
    assert result.exit_code == 0
    for option in ("--joint", "--structure"):
        assert option in result.output
