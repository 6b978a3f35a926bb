"""``dwelltime --smooth --populations G`` / ``ttfb --smooth --populations G`` without a GPU: the g++
build of the bodies behind ``tq_population_dwell`` as a replay of both modes, exactly equal to the host functions of
``tapqir_amd.utils.imscroll`` on the class view of the raster of the existing replay ``mixture_fixture.host_count``, split by
the populations that replay drew; at one population equal to the replay of ``tq_chain_dwell``; the conditions of the
section on that replay; the C layout of the argument struct, the export, the refusals of the entry point and of the
Python functions, and the exits and the help text of the two commands."""

import ctypes
import logging
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest
import torch
import typer
from typer.testing import CliRunner

import hmm_dwell_fixture
import mixture_dwell_fixture as mdf
import mixture_fixture as mf
from smooth_dwell_fixture import survival_deviation
from tapqir_amd import _lib, _lib_mixture
from tapqir_amd.main import app
from tapqir_amd.utils.dataset import save
from tapqir_amd.utils.simulate import TEST_PARAMS, simulate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def hk(tmp_path_factory):
    return mdf.build_population_dwell_check(tmp_path_factory.mktemp("population_dwell"))


@pytest.fixture(scope="module")
def build(tmp_path_factory):
    return mf.HostBuild(tmp_path_factory.mktemp("mixture"))


# ---- the replay -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("U,B", mdf.UB_HOST)
@pytest.mark.parametrize("G", mdf.G_LIST)
@pytest.mark.parametrize("F", mdf.F_LIST)
def test_replay_equals_the_host_functions_on_the_class_raster_of_mixture_count(hk, build, U, B, G, F):
    """N = 6 with the special rows, S = 70: counts, tau, pop and the table exactly, the histograms of every population and
    their sum; the same uniforms against the same thresholds as the existing replay."""
    S = 70
    who = f"({U}, {B}) G = {G} F = {F}"
    _, thetas, filt, resp = mf.sampler_inputs(build, U, B, G, F)
    existing = build.count(filt, thetas, resp, U, B, S, 0)
    got = mdf.host_sample(hk, filt, thetas, resp, U, B, S, seed=0)
    want = mdf.oracle_of_populations(existing["raster"] >= U, existing["pop"], G)
    mdf.assert_equals_population_oracle(got, want, who)
    assert got["true_total"] == len(want["table"])
    assert np.array_equal(got["margins"], existing["margins"]), who
    assert (got["tau"][:, 0] == F).all() and (got["tau"][:, 1] == 0).all()  # never and always bound
    if G > 1:
        assert len(np.unique(got["pop"])) > 1  # the binning by population is exercised


@pytest.mark.parametrize("U,B", [(1, 2), (2, 2)])
@pytest.mark.parametrize("F", [2, 65])
def test_short_table_holds_the_first_rows_and_nothing_else(hk, build, U, B, F):
    S, G = 70, 2
    _, thetas, filt, resp = mf.sampler_inputs(build, U, B, G, F)
    existing = build.count(filt, thetas, resp, U, B, S, 0)
    want = mdf.oracle_of_raster(existing["raster"] >= U)["table"]
    total = len(want) - 1
    got = mdf.host_sample(hk, filt, thetas, resp, U, B, S, seed=0, total=total)["table"]
    assert len(got) == total
    for col in got.columns:
        assert np.array_equal(got[col].to_numpy(), want[col].to_numpy()[:total]), col
    assert len(mdf.host_sample(hk, filt, thetas, resp, U, B, S, seed=0, total=0)["table"]) == 0


@pytest.mark.parametrize("U,B", mdf.UB_HOST)
def test_one_population_is_the_replay_of_the_single_chain(hk, build, U, B, tmp_path):
    S, F = 70, 65
    single = hmm_dwell_fixture.build_hmm_dwell_check(tmp_path)
    _, thetas, filt, resp = mf.sampler_inputs(build, U, B, 1, F)
    got = mdf.host_sample(hk, filt, thetas, resp, U, B, S, seed=3)
    want = hmm_dwell_fixture.host_sample(single, filt[0], thetas[0], U, B, S, seed=3)
    for key in ("counts", "tau"):
        assert np.array_equal(got[key], want[key]), key
    for key in ("hist_bound", "hist_unbound"):
        assert got[key].shape == (S, 1, F) and np.array_equal(got[key][:, 0], want[key]), key
    assert got["table"].equals(want["table"]) and (got["pop"] == 0).all()
    assert got["margins"][1] == want["margin"] and got["margins"][0] == 1.0


# ---- the law of tau ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("U,B", [(1, 2), (2, 2)])
@pytest.mark.parametrize("G", [2, 4])
def test_first_binding_follows_the_exact_survival_law_of_the_mixture(hk, build, U, B, G):
    """S = 4096, N = 4, F = 129, generator seed 2, theta_g = fixed_theta(U, B, seed=g), phi uniform, resp of the oracle: the
    empirical P(tau > f) within 5 binomial sigma of sum_g resp[g, n] S_g(n, f) wherever that lies in [0.02, 0.98]; at least
    50 such points."""
    S, N, F = 4096, 4, 129
    p = mf.synthetic_hmm(N, F, 2)[0]
    thetas = np.array([mf.fixed_theta(U, B, seed=g) for g in range(G)])
    resp = np.asarray(mf.oracle_final(p, mf.PRIOR, thetas, np.full(G, 1.0 / G), U, B)[1], np.float64)
    got = mdf.host_sample(hk, build.filt(p, thetas, U, B), thetas, resp, U, B, S, seed=0)
    points, dev = survival_deviation(got["tau"], mdf.mixture_survival(p, thetas, resp, U, B, mf.PRIOR))
    print(f"({U}, {B}) G = {G}: {points} points, largest deviation {dev:.2f} sigma, winning responsibilities "
          f"{resp.max(0).round(3)}, margins {got['margins']}")
    assert points >= 50
    assert dev <= 5.0


# ---- the conditions -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,s", [("XY", 0), ("XY", 1), ("XI", 0), ("XI", 1)])
def test_population_rasters_mend_what_the_single_chain_pools(hk, build, kind, s, tmp_path):
    """The conditions of section 30 on the g++ build: 150 EM iterations from the default start, S = 64, sampler seed 0."""
    S = 64
    p = mf.static_data(kind, s)[0]
    fits = {}
    for G in (1, 2):
        th, ph = mf.mixture_default_start(1, 1, G)
        fit = build.fit(p, mf.normalised(th, 2)[None], ph[None], 1, 1, None, 150, 150)
        fits[G] = (fit["thetas"][0], np.ascontiguousarray(fit["resp"][0]))
    thetas, resp = fits[2]
    mixture = mdf.host_sample(hk, build.filt(p, thetas, 1, 1), thetas, resp, 1, 1, S, seed=0)
    single = hmm_dwell_fixture.host_sample(hmm_dwell_fixture.build_hmm_dwell_check(tmp_path),
                                           build.filt(p, fits[1][0], 1, 1)[0], fits[1][0][0], 1, 1, S, seed=0)
    mdf.check_conditions(kind, s, mdf.condition_figures(kind, s, mixture, single, resp), "g++")


# ---- ABI ------------------------------------------------------------------------------------------------------------
def header_text():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tapqir_hip.h")).read(), flags=re.S)


def test_struct_layout_matches_the_c_header():
    """sizeof and every offsetof of the mirror equal gcc's, and the mirror names the header's fields in order."""
    cls, cname = _lib_mixture.PopulationDwellArgs, "tq_population_dwell_args"
    assert cname in cls.__doc__
    body = re.search(r"typedef struct \{([^{}]*)\}\s*%s;" % cname, header_text()).group(1)
    fields = [re.search(r"(\w+)\s*$", d.strip()).group(1) for decl in body.split(";") if decl.strip()
              for d in decl.split(",")]
    names = [f[0] for f in cls._fields_]
    assert names == fields
    lines = ['  printf("%%zu\\n", sizeof(%s));' % cname] + ['  printf("%%zu\\n", offsetof(%s, %s));' % (cname, f)
                                                           for f in names]
    want = [ctypes.sizeof(cls)] + [getattr(cls, f).offset for f in names]
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "tapqir_hip.h"\nint main(void) {\n' + "\n".join(lines)
           + "\n  return 0;\n}\n")
    with tempfile.TemporaryDirectory() as td:
        c = os.path.join(td, "s.c")
        open(c, "w").write(src)
        exe = os.path.join(td, "s")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        got = [int(v) for v in subprocess.check_output([exe]).split()]
    assert got == want


def test_the_export_is_declared_bound_and_kept_out_of_lib():
    assert "tq_population_dwell" in _lib.EXPORTS
    assert "tq_population_dwell" in set(re.findall(r"\b(tq_[a-z_0-9]+)\s*\(", header_text()))
    assert not hasattr(_lib, "PopulationDwellArgs")
    fn = _lib_mixture.lib().tq_population_dwell
    assert fn.restype is ctypes.c_int and fn.argtypes[0]._type_ is _lib_mixture.PopulationDwellArgs


def test_argument_validation_returns_error_codes_without_a_gpu():
    lib = _lib_mixture.lib()
    buf = (ctypes.c_int64 * 8)()
    addr = ctypes.addressof(buf)
    count = dict(filt=addr, theta=addr, resp=addr, counts=addr, pop=addr, hist_bound=addr, hist_unbound=addr, N=3, F=5, S=2,
                 G=2, U=1, B=2, mode=_lib.DWELL_COUNT)
    emit = dict(filt=addr, theta=addr, resp=addr, counts=addr, offsets=addr, intervals=addr, total=4, N=3, F=5, S=2, G=2, U=1,
                B=2, mode=_lib.DWELL_EMIT)

    def call(good, **change):
        return lib.tq_population_dwell(ctypes.byref(_lib_mixture.PopulationDwellArgs(**{**good, **change})), None)

    def refused(good, text, **change):
        assert call(good, **change) == 1, change  # TQ_ERR_ARG
        err = lib.tq_last_error()
        assert b"tq_population_dwell" in err and text in err, err

    assert lib.tq_population_dwell(None, None) == 1
    assert lib.tq_population_dwell(ctypes.byref(_lib_mixture.PopulationDwellArgs()), None) == 1
    assert b"NULL" in lib.tq_last_error()
    for good in (count, emit):
        for key, value in good.items():
            if value == addr:
                refused(good, b"NULL", **{key: None})
        for key in ("N", "F", "S"):
            refused(good, b"positive", **{key: 0})
            refused(good, b"positive", **{key: -1})
        refused(good, b"65536", F=65537)
        refused(good, b"S too large", S=65535 * 64 + 1)
        refused(good, b"non-negative", total=-1)
        for mode in (2, -1):
            refused(good, b"unknown mode", mode=mode)
        for U, B in ((0, 2), (2, 0), (-1, 3), (1, 4), (3, 2), (4, 1)):
            refused(good, b"U + B at most 4", U=U, B=B)
        for G in (0, -1, 5):
            refused(good, b"G must be at least 1 and at most 4", G=G)
    # EMIT of an empty table launches nothing: TQ_OK with no device in sight, with or without a table pointer
    assert call(emit, total=0) == 0
    assert call(emit, total=0, intervals=None) == 0
    assert call(emit, total=0, U=2, B=2, G=4) == 0


def test_device_entry_points_refuse_host_tensors():
    from tapqir_amd.exceptions import HipExtensionError
    from tapqir_amd.utils.mle_analysis import mixture_dwell_intervals, mixture_dwell_sample

    thetas = torch.from_numpy(np.array([mf.fixed_theta(1, 2, seed=g) for g in range(2)]))
    filt = torch.rand(2, 3, 5, 3, dtype=torch.float64)
    resp = torch.full((2, 3), 0.5, dtype=torch.float64)
    with pytest.raises(HipExtensionError):
        mixture_dwell_sample(filt, thetas, resp, 1, 2, 4)
    with pytest.raises(HipExtensionError):
        mixture_dwell_intervals(filt, thetas, resp, 1, 2, 4)
    with pytest.raises(HipExtensionError):
        mixture_dwell_intervals(filt, thetas, resp, 1, 2, 4, sample={"counts": torch.zeros(4, 3, dtype=torch.int32)})


def test_population_first_binding_against_a_loop():
    """The host-side split of tau by population (torch, on the CPU here) against a plain loop, with a population no row of
    a sample drew and one none of whose rows bound."""
    from tapqir_amd.utils.mle_analysis import population_first_binding

    F, G = 7, 3
    tau = torch.tensor([[0.0, 7.0, 3.0, 7.0, 5.0], [7.0, 7.0, 2.0, 1.0, 0.0]])
    pop = torch.tensor([[0, 0, 1, 1, 1], [0, 0, 2, 2, 2]], dtype=torch.uint8)
    got = population_first_binding(tau, pop, G, F)
    for s in range(2):
        for g in range(G):
            rows = tau[s][pop[s] == g]
            if len(rows) == 0:
                assert got["share"][s, g] == 0 and torch.isnan(got["never_bound"][s, g])
                assert torch.isnan(got["first_binding"][s, g]) and torch.isnan(got["fraction_bound"][s, g]).all()
                continue
            assert got["share"][s, g] == len(rows) / 5 and got["never_bound"][s, g] == (rows == F).double().mean()
            bound = rows[rows < F]
            if len(bound):
                assert got["first_binding"][s, g] == bound.double().mean()
            else:
                assert torch.isnan(got["first_binding"][s, g])
            want = torch.stack([(rows < t).double().mean() for t in range(F)])
            assert torch.equal(got["fraction_bound"][s, g], want)


# ---- command line -----------------------------------------------------------------------------------------------------
def invoke(tmp_path, command, *flags):
    save(simulate(2, 2, 5, 1, 14, params=dict(TEST_PARAMS)), tmp_path)
    return CliRunner().invoke(app, ["--cd", str(tmp_path), command, *flags, "--num-samples", "10", "--no-input"])


@pytest.mark.parametrize("command", ["dwelltime", "ttfb"])
@pytest.mark.parametrize("flags,text", [
    (["--populations", "2"], "--populations needs --smooth"),
    (["--populations", "5"], "1 .. 4"),
    (["--smooth", "--populations", "5"], "1 .. 4"),
    (["--smooth", "--populations", "0"], "1 .. 4"),
    (["--populations", "5", "--cpu"], "1 .. 4"),
    (["--bound-states", "2", "--populations", "2"], "need --smooth"),
    (["--smooth", "--populations", "2", "--cpu"], "GPU"),
    (["--populations", "2", "--cpu"], "GPU"),
    (["--smooth", "--populations", "2", "--model", "crosstalk"], "cosmos only"),
    (["--populations", "5", "--model", "crosstalk"], "cosmos only"),
])
def test_population_flags_are_refused_with_exit_status_1(tmp_path, command, flags, text):
    result = invoke(tmp_path, command, *flags)
    assert result.exit_code == 1, result.output  # 2 = no such option
    assert text in result.output


@pytest.mark.parametrize("command", ["dwelltime", "ttfb"])
@pytest.mark.parametrize("U,B,again", [(1, 1, "smooth --populations 2"),
                                       (1, 2, "smooth --unbound-states 1 --bound-states 2 --populations 2")])
def test_missing_mixture_file_names_the_run_to_do_first(tmp_path, caplog, command, U, B, again):
    from tapqir_amd.main import _smooth_suffix, _smoothed_posterior

    assert _smooth_suffix(U, B, 2) == f"-u{U}b{B}g2" and _smooth_suffix(1, 1) == "" and _smooth_suffix(1, 2, 1) == "-u1b2"
    logger = logging.getLogger("tapqir")
    with caplog.at_level(logging.ERROR, logger="tapqir"), pytest.raises(typer.Exit) as exit_info:
        _smoothed_posterior(command, tmp_path, "cosmos", torch.ones(2, dtype=torch.bool), logger, U, B, 2)
    assert exit_info.value.exit_code == 1
    assert f"cosmos_smooth-u{U}b{B}g2.tpqr" in caplog.text and f"run `{again}` first" in caplog.text


@pytest.mark.parametrize("command", ["dwelltime", "ttfb"])
def test_help_shows_the_option_and_what_is_not_promised(tmp_path, command):
    result = CliRunner().invoke(app, ["--cd", str(tmp_path), command, "--help"])
    assert result.exit_code == 0 and "--populations" in result.output
    text = " ".join(result.output.split())
    assert "mixture of G chains" in text and "g<G>" in text and text.count("not bit for bit") >= 2
    if command == "ttfb":
        assert "no per-population ttfb fits" in text
    else:
        assert "population" in text and "g<g>_A<i>" in text
