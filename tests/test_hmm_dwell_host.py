"""Multi-state ``dwelltime --smooth`` / ``ttfb --smooth`` without a GPU: the g++ build of the new
bodies of tq_hmm.h as a replay of ``tq_chain_dwell`` (both modes), exactly equal to the host functions of
``tapqir_amd.utils.imscroll`` on the class view of the raster of the existing replay ``hmm_fixture.host_count``; the three
conditions of the section on that replay; the C layout of the argument struct, the export, the refusals of the entry point
and of the Python functions, and the exits and the help text of the two commands."""

import ctypes
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest
import torch
from typer.testing import CliRunner

import dwell_fixture
from hmm_dwell_fixture import (F_LIST, MARGIN, PRIOR, UB_LIST, build_hmm_dwell_check, check_what_it_is_for, host_sample,
                               oracle_survival)
from hmm_fixture import (build_hmm_check, default_start, fixed_theta, host_count, host_em, host_estep, synthetic_hmm,
                         with_special_rows)
from smooth_dwell_fixture import assert_equals_oracle, n01_of_table, oracle_of_raster, survival_deviation
from tapqir_amd import _lib, _lib_hmm
from tapqir_amd.main import app
from tapqir_amd.utils.dataset import save
from tapqir_amd.utils.imscroll import time_to_first_binding
from tapqir_amd.utils.simulate import TEST_PARAMS, simulate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def hk(tmp_path_factory):
    return build_hmm_dwell_check(tmp_path_factory.mktemp("hmm_dwell"))


@pytest.fixture(scope="module")
def hk_hmm(tmp_path_factory):
    return build_hmm_check(tmp_path_factory.mktemp("hmm"))


# ---- the replay -------------------------------------------------------------------------------------------------------
def replay_case(hk_hmm, U, B, F, S=70, seed=0):
    """N = 6: rows of all 0, all 1, alternating 0 / 1 and p = prior, and two rows of the three-state reference chain; the
    g++ E-step's filt and what the existing replay of tq_hmm_count draws from it."""
    theta = fixed_theta(U, B)
    p = with_special_rows(synthetic_hmm(6, F, seed=F)[0], PRIOR)
    filt = host_estep(hk_hmm, p, theta, U, B, PRIOR)["filt"]
    counts4, _, raster, margin = host_count(hk_hmm, filt, theta, U, B, S, seed)
    return filt, theta, counts4, raster, margin


@pytest.mark.parametrize("U,B", UB_LIST)
@pytest.mark.parametrize("F", F_LIST)
def test_replay_equals_the_host_functions_on_the_class_raster_of_hmm_count(hk, hk_hmm, U, B, F):
    S = 70
    filt, theta, counts4, raster, margin = replay_case(hk_hmm, U, B, F, S)
    got, want = host_sample(hk, filt, theta, U, B, S, seed=0), oracle_of_raster(raster >= U)
    assert_equals_oracle(got, want, f"({U}, {B}) F = {F}")
    assert got["true_total"] == len(want["table"])
    assert got["margin"] == margin  # the same uniforms against the same thresholds as the existing replay
    assert np.array_equal(n01_of_table(got["table"], S, 6), counts4[..., 0])
    assert (got["tau"][:, 0] == F).all() and (got["tau"][:, 1] == 0).all()  # never and always bound
    assert not np.array_equal(host_sample(hk, filt, theta, U, B, S, seed=1)["tau"], got["tau"]) or F == 1


@pytest.mark.parametrize("U,B", [(1, 2), (2, 2)])
@pytest.mark.parametrize("F", [2, 65])
def test_short_table_holds_the_first_rows_and_nothing_else(hk, hk_hmm, U, B, F):
    S = 70
    filt, theta, _, raster, _ = replay_case(hk_hmm, U, B, F, S)
    want = oracle_of_raster(raster >= U)["table"]
    total = len(want) - 1
    got = host_sample(hk, filt, theta, U, B, S, seed=0, total=total)["table"]
    assert len(got) == total
    for col in got.columns:
        assert np.array_equal(got[col].to_numpy(), want[col].to_numpy()[:total]), col
    assert len(host_sample(hk, filt, theta, U, B, S, seed=0, total=0)["table"]) == 0


# ---- the conditions -----------------------------------------------------------------------------------------------------
def test_multi_state_rasters_mend_what_two_states_leave(hk, hk_hmm, tmp_path):
    """Conditions 1 and 2 of section 25: N = 40, F = 500 of the three-state reference chain, generator seed 0, 50 EM
    iterations from the default start, S = 64, sampler seed 0.  For the interior bound and unbound dwell times,
    |(1, 2) - hidden| <= 0.25 |(1, 1) - hidden| (both through the new bodies) and <= 0.25 |independent - hidden|; for the
    mean first-binding frame, |(1, 2) - hidden| <= 0.5 |independent - hidden|."""
    S = 64
    p, states = synthetic_hmm(40, 500, seed=0)
    chains = {}
    for U, B in ((1, 1), (1, 2)):
        theta = host_em(hk_hmm, p, PRIOR, default_start(U, B), U, B, 50)[0][-1]
        filt = host_estep(hk_hmm, p, theta, U, B, PRIOR)["filt"]
        chains[U, B] = host_sample(hk, filt, theta, U, B, S, seed=0)
        print(f"({U}, {B}): {chains[U, B]['true_total'] / S:.0f} intervals per raster, smallest |u - t| "
              f"{chains[U, B]['margin']:.3g}")
    hkd = dwell_fixture.build_dwell_check(tmp_path)
    _, _, ind_hb, ind_hu = dwell_fixture.host_sample(hkd, p, S, 0)
    ind_tau = time_to_first_binding(dwell_fixture.host_raster(hkd, p, S, 0).astype(np.uint8))
    independent = {"hist_bound": ind_hb, "hist_unbound": ind_hu, "tau": ind_tau}
    check_what_it_is_for(oracle_of_raster((states >= 1)[None]), independent, chains[1, 1], chains[1, 2])


@pytest.mark.parametrize("U,B", [(1, 2), (2, 2)])
def test_first_binding_follows_the_exact_survival_law(hk, hk_hmm, U, B):
    """Condition 3: S = 4096, N = 4, F = 129, generator seed 2, theta = fixed_theta(U, B): the empirical P(tau > f) within
    5 binomial sigma of the exact survival of the multi-state chain at every (row, frame) where that lies in
    [0.02, 0.98]; at least 50 such points (the oracle alone has 55)."""
    S, N, F = 4096, 4, 129
    theta = fixed_theta(U, B)
    p = synthetic_hmm(N, F, seed=2)[0]
    filt = host_estep(hk_hmm, p, theta, U, B, PRIOR)["filt"]
    got = host_sample(hk, filt, theta, U, B, S, seed=0)
    points, dev = survival_deviation(got["tau"], oracle_survival(p, theta, U, B, PRIOR))
    print(f"({U}, {B}): {points} points, largest deviation {dev:.2f} sigma, smallest |u - t| {got['margin']:.3g}")
    assert points >= 50
    assert dev <= 5.0
    assert got["margin"] > MARGIN


def test_survival_oracle_at_two_states_is_the_two_state_oracle():
    """The exact survival of this file at (1, 1) against smooth_dwell_fixture's, which shares no code with it."""
    import smooth_dwell_fixture as two

    kon, koff, pi0 = 0.05, 0.10, 0.4
    p = synthetic_hmm(4, 129, seed=2)[0]
    theta = np.array([1 - kon, kon, koff, 1 - koff, 1 - pi0, pi0])
    assert np.abs(oracle_survival(p, theta, 1, 1, PRIOR) - two.oracle_survival(p, (kon, koff, pi0), PRIOR)).max() < 1e-12


# ---- ABI ------------------------------------------------------------------------------------------------------------
def header_text():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tapqir_hip.h")).read(), flags=re.S)


def test_struct_layout_matches_the_c_header():
    """sizeof and every offsetof of the mirror equal gcc's, and the mirror names the header's fields in order."""
    cls, cname = _lib_hmm.ChainDwellArgs, "tq_chain_dwell_args"
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
    assert "tq_chain_dwell" in _lib.EXPORTS
    assert "tq_chain_dwell" in set(re.findall(r"\b(tq_[a-z_0-9]+)\s*\(", header_text()))
    assert not hasattr(_lib, "ChainDwellArgs")
    fn = _lib_hmm.lib().tq_chain_dwell
    assert fn.restype is ctypes.c_int and fn.argtypes[0]._type_ is _lib_hmm.ChainDwellArgs


def test_argument_validation_returns_error_codes_without_a_gpu():
    lib = _lib_hmm.lib()
    buf = (ctypes.c_int64 * 8)()
    addr = ctypes.addressof(buf)
    count = dict(filt=addr, theta=addr, counts=addr, hist_bound=addr, hist_unbound=addr, N=3, F=5, S=2, U=1, B=2,
                 mode=_lib.DWELL_COUNT)
    emit = dict(filt=addr, theta=addr, counts=addr, offsets=addr, intervals=addr, total=4, N=3, F=5, S=2, U=1, B=2,
                mode=_lib.DWELL_EMIT)

    def call(good, **change):
        return lib.tq_chain_dwell(ctypes.byref(_lib_hmm.ChainDwellArgs(**{**good, **change})), None)

    def refused(good, text, **change):
        assert call(good, **change) == 1, change  # TQ_ERR_ARG
        err = lib.tq_last_error()
        assert b"tq_chain_dwell" in err and text in err, err

    assert lib.tq_chain_dwell(None, None) == 1
    assert lib.tq_chain_dwell(ctypes.byref(_lib_hmm.ChainDwellArgs()), None) == 1 and b"NULL" in lib.tq_last_error()
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
    # EMIT of an empty table launches nothing: TQ_OK with no device in sight, with or without a table pointer
    assert call(emit, total=0) == 0
    assert call(emit, total=0, intervals=None) == 0
    assert call(emit, total=0, U=2, B=2) == 0


def test_device_entry_points_refuse_host_tensors_and_bad_shapes():
    from tapqir_amd.exceptions import HipExtensionError
    from tapqir_amd.utils.mle_analysis import hmm_dwell_intervals, hmm_dwell_sample

    theta = torch.from_numpy(fixed_theta(1, 2))
    filt = torch.rand(3, 5, 3, dtype=torch.float64)
    with pytest.raises(HipExtensionError):
        hmm_dwell_sample(filt, theta, 1, 2, 4)
    with pytest.raises(HipExtensionError):
        hmm_dwell_intervals(filt, theta, 1, 2, 4)
    with pytest.raises(HipExtensionError):
        hmm_dwell_intervals(filt, theta, 1, 2, 4, sample={"counts": torch.zeros(4, 3, dtype=torch.int32)})


# ---- command line -----------------------------------------------------------------------------------------------------
def invoke(tmp_path, command, *flags):
    save(simulate(2, 2, 5, 1, 14, params=dict(TEST_PARAMS)), tmp_path)
    return CliRunner().invoke(app, ["--cd", str(tmp_path), command, *flags, "--num-samples", "10", "--no-input"])


@pytest.mark.parametrize("command", ["dwelltime", "ttfb"])
@pytest.mark.parametrize("flags,text", [
    (["--bound-states", "2"], "need --smooth"),
    (["--unbound-states", "2"], "need --smooth"),
    (["--smooth", "--bound-states", "4"], "at most 4"),
    (["--unbound-states", "3", "--bound-states", "2", "--cpu"], "at most 4"),
    (["--smooth", "--bound-states", "2", "--cpu"], "GPU"),
    (["--bound-states", "2", "--cpu"], "GPU"),
    (["--smooth", "--bound-states", "2", "--model", "crosstalk"], "cosmos only"),
    (["--unbound-states", "3", "--bound-states", "2", "--model", "crosstalk"], "cosmos only"),
])
def test_state_flags_are_refused_with_exit_status_1(tmp_path, command, flags, text):
    result = invoke(tmp_path, command, *flags)
    assert result.exit_code == 1, result.output  # 2 = no such option
    assert text in result.output


@pytest.mark.parametrize("command", ["dwelltime", "ttfb"])
def test_help_shows_the_new_options_and_what_is_not_promised(tmp_path, command):
    result = CliRunner().invoke(app, ["--cd", str(tmp_path), command, "--help"])
    assert result.exit_code == 0 and "--unbound-states" in result.output and "--bound-states" in result.output
    text = " ".join(result.output.split())
    assert "not bit for bit" in text
