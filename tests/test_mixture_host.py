"""A mixture of hidden Markov chains over the AOIs without a GPU: the g++ build of tq_mixture.h (the
weighted M-step with the device's strided ownership, order of populations and tree; the sampler that draws a population
with every raster; the per-population estimate) against the numpy oracle of mixture_fixture by the tolerance rule of
section 20, the G = 1 bit-identities with the single-chain bodies, the EM and the model-choice table driven through
``multistart_em`` on that build, the starts, the C layout of the argument structs, the exports, argument validation of the
entry points, and the exits of ``smooth --populations``."""

import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest
import torch
from typer.testing import CliRunner

import mixture_fixture as mf
from mixture_fixture import (G_LIST, N_LIST, PRIOR, SAMPLER_F, SAMPLER_S, UB_LIST, HostBuild, check_sample, chi2_bound,
                             oracle_estimate, oracle_mixture_sample, pop_law_chi2, run_choice_case, run_em_case,
                             run_hopeless_population, run_mstep_case, run_mstep_masked_and_swapped, sampler_inputs)
from tapqir_amd import _lib, _lib_mixture
from tapqir_amd.main import app
from tapqir_amd.utils.dataset import save
from tapqir_amd.utils.simulate import TEST_PARAMS, simulate
from test_multistart_host import header_fields, header_text

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def build(tmp_path_factory):
    return HostBuild(tmp_path_factory.mktemp("mixture"))


# ---- M-step -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("U,B", UB_LIST)
@pytest.mark.parametrize("N", N_LIST)
@pytest.mark.parametrize("G", G_LIST)
def test_weighted_mstep_equals_the_oracle(build, U, B, N, G):
    run_mstep_case(build, U, B, N, G)


def test_masked_topology_and_swapped_populations(build):
    run_mstep_masked_and_swapped(build)


def test_a_hopeless_population_keeps_a_finite_theta(build):
    run_hopeless_population(build)


def test_the_oracle_with_one_population_is_the_single_chain_oracle():
    from hmm_fixture import default_start, oracle_em

    p = mf.em_case()["p"]
    one = mf.oracle_em(p, PRIOR, [(default_start(1, 2)[None], np.ones(1))], 1, 2, 4)[0]
    thetas, trace = oracle_em(p, PRIOR, default_start(1, 2), 1, 2, 4)
    assert np.abs(one["thetas"][:, 0] - thetas).max() <= 1e-14 and np.abs(one["trace"] - trace).max() <= 1e-11 * np.abs(trace).max()


# ---- EM and model choice ------------------------------------------------------------------------------------------------
def test_em_follows_the_oracle(build):
    run_em_case(build)


@pytest.mark.parametrize("kind,s", mf.CHOICE_SETS)
def test_model_choice_reproduces_the_table(build, kind, s):
    run_choice_case(build.choice_fits(kind, s), kind, s, build.name)


def test_the_recorded_reference_is_the_oracle():
    """tests/golden/mixture_golden.npz against the oracle's 150 iterations on every data set in both precisions: the longdouble
    BIC bit for bit, the float64 figures to 1e-12 relative (numpy's float64 exp and log may differ in the last bit between
    processors, which 150 iterations carry on) and the trace's bound, a largest difference of such figures, within a half;
    on static data the oracle itself assigns every AOI to its generator."""
    live = mf.choice_summary()
    with np.load(mf.GOLDEN) as z:
        assert sorted(z.files) == sorted(live)
        for key, row in live.items():
            for hi in (1, 5):  # the longdouble BIC of the closing evidence and of the trace's last entry
                assert (np.array_equal(z[key][hi:hi + 2], row[hi:hi + 2])
                        or abs((z[key][hi] - row[hi]) + (z[key][hi + 1] - row[hi + 1])) <= 1e-15 * abs(row[hi])), key
            assert np.allclose(z[key][[0, 3]], row[[0, 3]], rtol=1e-12, atol=0) and np.isclose(z[key][4], row[4], rtol=0.5), key
    for kind, s in mf.CHOICE_SETS:
        case = mf.choice_case(kind, s)
        if case["labels"] is not None:
            pmap = case["g2_64"]["w"].argmax(0)
            assert np.array_equal(pmap, case["labels"]) or np.array_equal(pmap, 1 - case["labels"])


# ---- sampler ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("U,B", UB_LIST)
@pytest.mark.parametrize("G", [1, 2, 4])
@pytest.mark.parametrize("F", SAMPLER_F)
def test_sampler_replay_equals_numpy(build, G, F, U, B):
    """The g++ replay against the numpy replay of the population draw and of the drawn chain's backward sampler, bit for bit,
    after the margins of both kinds of compare; at G = 1 the outputs are the single-chain sampler's."""
    p, thetas, filt, resp = sampler_inputs(build, U, B, G, F)
    for S in SAMPLER_S:
        pop, raster, m_pop, m_state = oracle_mixture_sample(filt, thetas, resp, U, B, S, seed=F)
        print(f"G = {G} F = {F} S = {S}: smallest |u - threshold| {m_pop:.3g} (population), {m_state:.3g} (states)")
        assert m_pop > 1e-9 and m_state > 1e-9
        out = build.count(filt, thetas, resp, U, B, S, F)
        assert out["margins"][1] > 1e-9 and (G == 1 or out["margins"][0] > 1e-9)
        check_sample(out, {"pop": pop, "raster": raster}, U, U + B)
        if G == 1:
            single = build.hmm_count(filt[0], thetas[0], U, B, S, F)
            assert (out["pop"] == 0).all()
            for key in ("counts", "trans", "raster"):
                assert np.array_equal(out[key], single[key]), key


def test_population_draws_follow_the_responsibilities(build):
    """S = 4096, G = 4, N = 6: chi-square of the drawn populations against resp below the 1e-6 quantile."""
    p, thetas, filt, resp = sampler_inputs(build, 1, 1, 4, 2)
    out = build.count(filt, thetas, resp, 1, 1, 4096, 11)
    chi2, dof = pop_law_chi2(out["pop"], resp)
    print(f"chi2 = {chi2:.2f} with {dof} degrees of freedom, bound {chi2_bound(dof):.2f}")
    assert dof >= 6 and chi2 <= chi2_bound(dof)


# ---- estimate -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("resample", [0, 1])
def test_estimate_equals_numpy(build, resample, tmp_path):
    U, B, G, S, N = 1, 2, 3, 70, 6
    rng = np.random.default_rng(5)
    trans = rng.integers(0, 40, (S, N, 9)).astype(np.int32)
    pop = rng.integers(0, 2, (S, N)).astype(np.uint8)  # population 2 has no member
    pop[0] = 0
    idx = mf.host_indices(mf.build_rates_check(tmp_path), 9, S, N) if resample else None
    totals, members, est = build.estimate(trans, pop, G, U, B, resample, 9)
    t, m, e = oracle_estimate(trans, pop, G, U + B, idx)
    assert np.array_equal(totals, t) and np.array_equal(members, m) and np.array_equal(est, e, equal_nan=True)
    assert (members[:, 2] == 0).all() and np.isnan(est[:, 2]).all() and np.isnan(est[0, 1]).all() and members.sum(1).tolist() == [N] * S


# ---- the starts -----------------------------------------------------------------------------------------------------------
def test_starts_are_documented_reproducible_and_respect_the_topology():
    from tapqir_amd.utils.mle_analysis import hmm_random_starts, mixture_default_start, mixture_n_params, mixture_random_starts

    for U, B in ((1, 1), (1, 2), (2, 2)):
        M = U + B
        allow = mf.forbid(M, (M - 1, 0)) if M > 2 else None
        for G in (1, 2, 4):
            th, ph = mixture_default_start(U, B, G, allow)
            want = mf.mixture_default_start(U, B, G, allow)
            assert np.array_equal(th.numpy(), want[0]) and np.array_equal(ph.numpy(), want[1])
            ths, phs = mixture_random_starts(U, B, G, 3, seed=5, allow=allow)
            assert ths.shape == (4, G, M * M + M) and phs.shape == (4, G) and torch.equal(ths[0], th) and torch.equal(phs[0], ph)
            again = mixture_random_starts(U, B, G, 3, seed=5, allow=allow)
            assert torch.equal(ths, again[0]) and torch.equal(phs, again[1])
            A = ths[..., : M * M].reshape(4, G, M, M).numpy()
            assert np.abs(A.sum(-1) - 1).max() < 1e-15 and np.abs(phs.sum(1).numpy() - 1).max() < 1e-15
            if allow is not None:
                assert (A[..., ~allow] == 0).all()
        # one population: the draws of hmm_random_starts, then one Dirichlet draw of phi per start
        rng = np.random.default_rng(5)
        from tapqir_amd.utils.mle_analysis import _hmm_draw_start
        first = _hmm_draw_start(rng, M, np.ones((M, M), bool))
        assert np.array_equal(mixture_random_starts(U, B, 2, 1, seed=5)[0][1, 0].numpy(), first)
        assert np.array_equal(hmm_random_starts(U, B, 1, seed=5)[1].numpy(), first)
    assert mixture_n_params(torch.ones(2, 2, dtype=torch.bool), 2) == 7 == mf.n_params(2, 2)
    assert mixture_n_params(torch.ones(3, 3, dtype=torch.bool), 1) == 8
    for bad in (dict(populations=0), dict(populations=5), dict(populations=4, restarts=16), dict(restarts=-1)):
        with pytest.raises(ValueError):
            mixture_random_starts(1, 1, **{"populations": 2, "restarts": 0, **bad})


# ---- ABI ------------------------------------------------------------------------------------------------------------
MIRRORS = {"tq_mixture_mstep_args": _lib_mixture.MixtureMstepArgs, "tq_mixture_count_args": _lib_mixture.MixtureCountArgs,
           "tq_mixture_estimate_args": _lib_mixture.MixtureEstimateArgs}


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
           + '\n  printf("%d\\n", TQ_MIXTURE_MAX_POP);\n  return 0;\n}\n')
    with tempfile.TemporaryDirectory() as td:
        c = os.path.join(td, "s.c")
        open(c, "w").write(src)
        exe = os.path.join(td, "s")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        got = [int(v) for v in subprocess.check_output([exe]).split()]
    assert got.pop() == _lib_mixture.MIXTURE_MAX_POP == 4
    assert len(got) == len(want)
    assert [(n, f, g) for (n, f, _), g in zip(want, got)] == want


def test_exports_are_the_headers_declarations():
    import re

    names = {"tq_mixture_mstep", "tq_mixture_count", "tq_mixture_estimate"}
    declared = set(re.findall(r"\b(tq_[a-z_0-9]+)\s*\(", header_text()))
    assert {n for n in declared if n.startswith("tq_mixture_")} == names
    assert names == {n for n in _lib.EXPORTS if n.startswith("tq_mixture_")}
    lib = _lib_mixture.lib()
    assert all(hasattr(lib, n) for n in names)
    src = open(os.path.join(ROOT, "tapqir_amd", "csrc", "tq_mixture.h")).read()
    assert "#define TQ_MIXTURE_SITE 0xA05u" in src and _lib_mixture.MIXTURE_SITE == mf.POP_SITE == 0xA05


def test_argument_validation_returns_error_codes_without_a_gpu():
    lib = _lib_mixture.lib()
    buf = (ctypes.c_int64 * 8)()
    addr = ctypes.addressof(buf)
    A = _lib_mixture
    calls = {"mstep": (lib.tq_mixture_mstep, A.MixtureMstepArgs,
                       dict(rows=addr, theta=addr, phi=addr, trace=addr, N=3, it=0, T=1, P=2, G=2, U=1, B=2, allow=0x1FF)),
             "count": (lib.tq_mixture_count, A.MixtureCountArgs,
                       dict(filt=addr, theta=addr, resp=addr, counts=addr, pop=addr, N=3, F=5, S=2, G=2, U=1, B=2)),
             "estimate": (lib.tq_mixture_estimate, A.MixtureEstimateArgs,
                          dict(trans=addr, pop=addr, totals=addr, members=addr, estimand=addr, N=3, S=2, G=2, U=1, B=2))}

    def refused(name, text, **change):
        fn, cls, good = calls[name]
        assert fn(ctypes.byref(cls(**{**good, **change})), None) == 1, (name, change)  # TQ_ERR_ARG
        err = lib.tq_last_error()
        assert ("tq_mixture_" + name).encode() in err and text in err, err

    for name, (fn, cls, good) in calls.items():
        assert fn(None, None) == 1
        assert fn(ctypes.byref(cls()), None) == 1 and b"NULL" in lib.tq_last_error()
        for key, value in good.items():
            if value == addr:
                refused(name, b"NULL", **{key: None})
        refused(name, b"positive", N=0)
        for U, B in ((0, 2), (2, 0), (-1, 3), (1, 4), (3, 2), (4, 1)):
            refused(name, b"U + B at most 4", U=U, B=B)
        for G in (0, -1, 5):
            refused(name, b"G must be at least 1 and at most 4", G=G)
    for P, G in ((0, 2), (-1, 1), (33, 2), (65, 1), (17, 4), (22, 3)):
        refused("mstep", b"P * G at most 64", P=P, G=G)
    refused("mstep", b"non-negative", it=-1)
    refused("mstep", b"T must exceed it", it=1, T=1)
    refused("mstep", b"T must exceed it", it=0, T=0)
    refused("mstep", b"allow", allow=0x3FF)
    refused("mstep", b"allow", allow=0x1FF & ~0b111000)
    refused("mstep", b"allow", allow=0)
    refused("count", b"positive", F=0)
    refused("count", b"positive", S=0)
    refused("count", b"65536", F=65537)
    refused("count", b"16-byte", counts=addr + 8)
    refused("count", b"S too large", S=65535 * 64 + 1)
    refused("estimate", b"positive", S=0)
    refused("estimate", b"resample", resample=2)
    refused("estimate", b"S too large", S=65535 * 64 + 1)


def test_device_entry_points_refuse_host_tensors_and_bad_arguments():
    from tapqir_amd.exceptions import HipExtensionError
    from tapqir_amd.utils import mle_analysis as ma

    p = torch.rand(3, 5)
    with pytest.raises(HipExtensionError):
        ma.mixture_fit(p, PRIOR, 1, 1, populations=2)
    with pytest.raises(HipExtensionError):
        ma.mixture_mstep(torch.rand(1, 2, 3, 7, dtype=torch.float64), torch.rand(1, 2, 6, dtype=torch.float64),
                         torch.rand(1, 2, dtype=torch.float64), torch.zeros(1, 1, dtype=torch.float64))
    with pytest.raises(HipExtensionError):
        ma.mixture_sample(torch.rand(2, 3, 5, 2, dtype=torch.float64), torch.rand(2, 6, dtype=torch.float64),
                          torch.rand(2, 3, dtype=torch.float64), 1, 1, 4)
    with pytest.raises(HipExtensionError):
        ma.mixture_estimate(torch.zeros(2, 3, 4, dtype=torch.int32), torch.zeros(2, 3, dtype=torch.uint8), 2)
    with pytest.raises(HipExtensionError):
        ma.mixture_viterbi(p, torch.rand(2, 6, dtype=torch.float64), torch.rand(2, 3, dtype=torch.float64), PRIOR)
    for bad in (dict(populations=0), dict(populations=5), dict(num_iter=0), dict(populations=4, restarts=16),
                dict(unbound=3, bound=2), dict(allow=torch.ones(3, 3))):
        with pytest.raises(ValueError):
            ma.mixture_fit(p, PRIOR, **{"unbound": 1, "bound": 1, "populations": 2, **bad})


# ---- command line -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags,text", [
    (["--populations", "2", "--cpu"], "GPU"),
    (["--populations", "5", "--cpu"], "--populations must lie in 1 .. 4"),
    (["--populations", "0", "--cpu"], "--populations must lie in 1 .. 4"),
    (["--populations", "2", "--joint", "0,1", "--cpu"], "--joint"),
    (["--populations", "4", "--restarts", "16", "--cpu"], "at most 64"),
    (["--populations", "2", "--forbid", "0-2", "--cpu"], "--forbid takes i-j"),
])
def test_smooth_populations_refusals(tmp_path, flags, text):
    save(simulate(2, 2, 5, 1, 14, params=dict(TEST_PARAMS)), tmp_path)
    result = CliRunner().invoke(app, ["--cd", str(tmp_path), "smooth", *flags, "--num-samples", "10", "--no-input"])
    assert result.exit_code == 1, result.output  # 2 = no such command or option
    assert text in result.output


def test_smooth_help_shows_the_option(tmp_path):
    result = CliRunner().invoke(app, ["--cd", str(tmp_path), "smooth", "--help"])
    assert result.exit_code == 0 and "--populations" in result.output
