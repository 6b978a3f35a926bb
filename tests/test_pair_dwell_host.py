"""``dwelltime --smooth --joint A,B`` / ``ttfb --smooth --joint A,B`` without a GPU: the g++ build of
the bodies behind ``tq_pair_dwell`` as a replay of both modes and both channels, exactly equal to the oracle of
pair_dwell_fixture on the raster of joint states of the existing replay ``hmm_fixture.host_count`` at (2, 2); channel b equal
to the replay of ``tq_chain_dwell`` at (2, 2); the condition of the section on that replay; ``joint_arrival_order`` against
a loop; the C layout of the argument struct, the export, the refusals of the entry point and of the Python functions, and
the exits and the help text of the two commands."""

import ctypes
import logging
import os
import re
import subprocess
import tempfile
import types

import numpy as np
import pytest
import torch
import typer
from typer.testing import CliRunner

import hmm_dwell_fixture
import hmm_fixture
import joint_fixture as jf
import pair_dwell_fixture as pdf
import smooth_fixture
from tapqir_amd import _lib, _lib_joint
from tapqir_amd.main import app
from tapqir_amd.utils.dataset import save
from tapqir_amd.utils.imscroll import INTERVAL_COLUMNS
from tapqir_amd.utils.simulate import TEST_PARAMS, simulate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def hk(tmp_path_factory):
    return pdf.build_pair_dwell_check(tmp_path_factory.mktemp("pair_dwell"))


@pytest.fixture(scope="module")
def hk_joint(tmp_path_factory):
    return jf.build_joint_check(tmp_path_factory.mktemp("joint"))


@pytest.fixture(scope="module")
def hk_hmm(tmp_path_factory):
    return hmm_fixture.build_hmm_check(tmp_path_factory.mktemp("hmm"))


@pytest.fixture(scope="module")
def hk_chain(tmp_path_factory):
    return hmm_dwell_fixture.build_hmm_dwell_check(tmp_path_factory.mktemp("hmm_dwell"))


# ---- the replay -------------------------------------------------------------------------------------------------------
def replay_case(hk_joint, hk_hmm, F, S=70, seed=0):
    """N = 6 with the special rows of both channels: the g++ joint E-step's filt at ``fixed_theta()`` and the raster of
    joint states the existing replay of tq_hmm_count draws from it at (2, 2)."""
    theta = jf.fixed_theta()
    pa, pb = jf.estep_inputs(6, F, seed=F)
    filt = np.ascontiguousarray(jf.host_estep(hk_joint, pa, pb, theta[None], gamma=False)["filt"][0])
    _, _, raster, margin = hmm_fixture.host_count(hk_hmm, filt, theta, 2, 2, S, seed)
    return filt, theta, raster, margin


@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("F", pdf.F_LIST)
def test_replay_equals_the_oracle_on_the_raster_of_hmm_count(hk, hk_joint, hk_hmm, which, F):
    S = 70
    who = f"which = {which}, F = {F}"
    filt, theta, raster, margin = replay_case(hk_joint, hk_hmm, F, S)
    got, want = pdf.host_sample(hk, filt, theta, which, S, seed=0), pdf.oracle_of_states(raster, which)
    pdf.assert_equals_pair_oracle(got, want, who)
    assert got["true_total"] == len(want["table"])
    assert got["margin"] == margin  # the same uniforms against the same thresholds as the existing replay
    for kind in ("bound", "unbound"):  # the partner's state splits the pooled histogram and nothing else
        assert got[f"hist_{kind}"].shape == (S, 2, F)
        assert np.array_equal(got[f"hist_{kind}"].sum(1), want[f"pooled_{kind}"]), (who, kind)
    if F >= 63:
        assert len(np.unique(got["partner"])) > 4 and got["hist_unbound"][:, 0].any() and got["hist_unbound"][:, 1].any()


@pytest.mark.parametrize("F", pdf.F_LIST)
def test_channel_b_is_the_replay_of_the_chain_walker_at_two_and_two(hk, hk_joint, hk_hmm, hk_chain, F):
    S = 70
    filt, theta, _, _ = replay_case(hk_joint, hk_hmm, F, S)
    got = pdf.host_sample(hk, filt, theta, 1, S, seed=3)
    want = hmm_dwell_fixture.host_sample(hk_chain, filt, theta, 2, 2, S, seed=3)
    for key in ("counts", "tau"):
        assert np.array_equal(got[key], want[key]), key
    for key in ("hist_bound", "hist_unbound"):
        assert np.array_equal(got[key].sum(1), want[key]), key
    assert got["table"].equals(want["table"]) and got["margin"] == want["margin"]


@pytest.mark.parametrize("which", [0, 1])
def test_both_channels_describe_the_same_rasters(hk, hk_joint, hk_hmm, which):
    """The first-binding frame of the partner's own walk is where this walk's tau_after can start from: with the two calls
    at one seed, tau_after >= the partner's tau, and equal to it where the partner binds no earlier than the lead."""
    S, F = 70, 129
    filt, theta, _, _ = replay_case(hk_joint, hk_hmm, F, S)
    lead, other = (pdf.host_sample(hk, filt, theta, w, S, seed=5) for w in (which, 1 - which))
    assert (lead["tau_after"] >= other["tau"]).all()
    late = other["tau"] >= lead["tau"]
    assert late.any() and np.array_equal(lead["tau_after"][late], other["tau"][late])
    assert (lead["tau_after"][lead["tau"] == F] == F).all()


@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("F", [2, 65])
def test_short_table_holds_the_first_rows_and_nothing_else(hk, hk_joint, hk_hmm, which, F):
    S = 70
    filt, theta, raster, _ = replay_case(hk_joint, hk_hmm, F, S)
    want = pdf.oracle_of_states(raster, which)
    total = len(want["table"]) - 1
    got = pdf.host_sample(hk, filt, theta, which, S, seed=0, total=total)  # asserts the guard entries itself
    assert len(got["table"]) == total and len(got["partner"]) == total
    for col in INTERVAL_COLUMNS:
        assert np.array_equal(got["table"][col].to_numpy(), want["table"][col].to_numpy()[:total]), col
    assert np.array_equal(got["partner"].astype(np.int64), want["partner"][:total])
    empty = pdf.host_sample(hk, filt, theta, which, S, seed=0, total=0)
    assert len(empty["table"]) == 0 and len(empty["partner"]) == 0


# ---- the condition ------------------------------------------------------------------------------------------------------
def test_hidden_figures_of_the_driven_fixture():
    """The figures the condition compares against, from numpy on the hidden raster alone."""
    (m0, m1), (n0, n1) = pdf.hidden_unbound_means(pdf.driven_case()[2])
    print(f"hidden raster: {m0:.2f} frames over {n0} runs with a unbound at the start, {m1:.2f} over {n1} with a bound")
    assert (round(m0, 2), round(m1, 2)) == pdf.HIDDEN_UNBOUND_B and (n0, n1) == (216, 198)


def test_partner_split_recovers_what_the_pooled_histogram_hides(hk, hk_joint, hk_chain, tmp_path):
    """The condition of section 32 on the g++ build: the driven chain N = 40, F = 500, seed 0; two-state fits of 50 EM
    iterations per channel from (0.5, 0.5, 0.5), then 50 EM iterations of ``a-drives-b`` from their Kronecker product;
    S = 64, sampler seed 0, channel b.  Measured here: q = 0 38.931 (ratio 0.084), q = 1 21.527 (ratio 0.086), pooled
    30.690; k_after / k_base 1.274 from 25.4 events a sample, reported and only asserted to be finite."""
    from tapqir_amd.utils.joint_analysis import joint_arrival_order

    S = 64
    pa, pb, _ = pdf.driven_case()
    hk_smooth = smooth_fixture.build_smooth_check(tmp_path)
    two = [smooth_fixture.host_em(hk_smooth, p, prior, (0.5, 0.5, 0.5), 50)[0][-1] for p, prior in zip((pa, pb), jf.PRIORS)]
    fit = jf.host_fit(hk_joint, pa, pb, structures=[1], start=jf.start_from(*two), num_iter=50, tol=0.0)
    assert fit["iterations"] == [50]
    theta = fit["thetas"][0]
    filt = np.ascontiguousarray(jf.host_estep(hk_joint, pa, pb, theta[None], gamma=False)["filt"][0])
    b = pdf.host_sample(hk, filt, theta, 1, S, seed=0)
    a = pdf.host_sample(hk, filt, theta, 0, S, seed=0)
    pooled = hmm_dwell_fixture.host_sample(hk_chain, filt, theta, 2, 2, S, seed=0)
    pdf.check_condition(b["hist_unbound"], pooled["hist_unbound"], "g++")
    order = joint_arrival_order(torch.from_numpy(a["tau"]), torch.from_numpy(a["tau_after"]), torch.from_numpy(b["tau"]), 500)
    events = (order["later"] * order["binds"] * 40).mean().item()
    print(f"g++: k_after / k_base = {order['ratio'].mean().item():.3f} from {events:.1f} events a sample (hidden raster: 1.4 "
          f"from 29); bound dwells of b by q: {pdf.interior_means(b['hist_bound'][:, 0]):.3f} / "
          f"{pdf.interior_means(b['hist_bound'][:, 1]):.3f} (hidden 12.38 / 12.19)")
    assert bool(torch.isfinite(order["ratio"]).all())


# ---- the order of arrival ---------------------------------------------------------------------------------------------
def test_arrival_order_against_a_loop():
    """Host-side torch against a plain loop: a sample where no row binds (every share and k_after NaN), one where every
    partner is there at once (no late arrival and no frame at risk: mean_delay and k_after NaN), one whose partner never binds (k_base 0, ratio
    NaN), and random ones."""
    from tapqir_amd.utils.joint_analysis import ORDER_NAMES, joint_arrival_order

    F = 9
    rng = np.random.default_rng(0)
    lead = rng.integers(0, F + 1, (6, 12)).astype(np.float32)
    after = np.where(lead < F, np.minimum(lead + rng.integers(0, 5, lead.shape), F), F).astype(np.float32)
    own = np.where(rng.random(lead.shape) < 0.5, after, rng.integers(0, F + 1, lead.shape)).astype(np.float32)
    lead[0], after[0] = F, F  # no row binds
    after[1] = lead[1]  # the partner is there when the lead arrives
    lead[1, lead[1] == F] = 0
    after[1] = lead[1]
    own[2], after[2] = F, F  # the partner never binds
    got = joint_arrival_order(torch.from_numpy(lead), torch.from_numpy(after), torch.from_numpy(own), F)
    want = pdf.arrival_order_by_loop(lead, after, own, F)
    assert tuple(got) == ORDER_NAMES
    for key in ORDER_NAMES:
        assert got[key].dtype == torch.float64 and got[key].shape == (6,)
        assert np.allclose(got[key].numpy(), np.array(want[key]), rtol=1e-14, atol=0, equal_nan=True), key
    assert all(np.isnan(got[key][0].item()) for key in ("together", "later", "never", "mean_delay", "k_after", "ratio"))
    assert got["binds"][0] == 0 and got["together"][1] == 1 and np.isnan(got["mean_delay"][1].item())
    assert np.isnan(got["k_after"][1].item())
    assert got["k_base"][2] == 0 and np.isnan(got["ratio"][2].item()) and got["never"][2] == 1
    with pytest.raises(ValueError):
        joint_arrival_order(torch.zeros(2, 3), torch.zeros(2, 4), torch.zeros(2, 3), F)


# ---- ABI ------------------------------------------------------------------------------------------------------------
def header_text():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tapqir_hip.h")).read(), flags=re.S)


def test_struct_layout_matches_the_c_header():
    """sizeof and every offsetof of the mirror equal gcc's, and the mirror names the header's fields in order."""
    cls, cname = _lib_joint.PairDwellArgs, "tq_pair_dwell_args"
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
    assert "tq_pair_dwell" in _lib.EXPORTS
    assert "tq_pair_dwell" in set(re.findall(r"\b(tq_[a-z_0-9]+)\s*\(", header_text()))
    assert not hasattr(_lib, "PairDwellArgs")
    fn = _lib_joint.lib().tq_pair_dwell
    assert fn.restype is ctypes.c_int and fn.argtypes[0]._type_ is _lib_joint.PairDwellArgs


def test_argument_validation_returns_error_codes_without_a_gpu():
    lib = _lib_joint.lib()
    buf = (ctypes.c_int64 * 8)()
    addr = ctypes.addressof(buf)
    count = dict(filt=addr, theta=addr, counts=addr, hist_bound=addr, hist_unbound=addr, N=3, F=5, S=2, which=1,
                 mode=_lib.DWELL_COUNT)
    emit = dict(filt=addr, theta=addr, counts=addr, offsets=addr, intervals=addr, partner=addr, total=4, N=3, F=5, S=2, which=0,
                mode=_lib.DWELL_EMIT)

    def call(good, **change):
        return lib.tq_pair_dwell(ctypes.byref(_lib_joint.PairDwellArgs(**{**good, **change})), None)

    def refused(good, text, **change):
        assert call(good, **change) == 1, change  # TQ_ERR_ARG
        err = lib.tq_last_error()
        assert b"tq_pair_dwell" in err and text in err, err

    assert lib.tq_pair_dwell(None, None) == 1
    assert lib.tq_pair_dwell(ctypes.byref(_lib_joint.PairDwellArgs()), None) == 1
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
        for which in (2, -1, 4):
            refused(good, b"which must be 0 (channel a) or 1 (channel b)", which=which)
    # EMIT of an empty table launches nothing: TQ_OK with no device in sight, with or without table and code pointers
    assert call(emit, total=0) == 0
    assert call(emit, total=0, intervals=None, partner=None) == 0
    assert call(emit, total=0, which=1) == 0


def test_device_entry_points_refuse_host_tensors():
    from tapqir_amd.exceptions import HipExtensionError
    from tapqir_amd.utils.joint_analysis import joint_dwell_intervals, joint_dwell_sample

    theta = torch.from_numpy(jf.fixed_theta())
    filt = torch.rand(3, 5, 4, dtype=torch.float64)
    for which in (0, 1):
        with pytest.raises(HipExtensionError):
            joint_dwell_sample(filt, theta, which, 4)
        with pytest.raises(HipExtensionError):
            joint_dwell_intervals(filt, theta, which, 4)
        with pytest.raises(HipExtensionError):
            joint_dwell_intervals(filt, theta, which, 4, sample={"counts": torch.zeros(4, 3, dtype=torch.int32)})


# ---- command line -----------------------------------------------------------------------------------------------------
def invoke(tmp_path, command, *flags):
    save(simulate(2, 2, 5, 1, 14, params=dict(TEST_PARAMS)), tmp_path)
    return CliRunner().invoke(app, ["--cd", str(tmp_path), command, *flags, "--num-samples", "10", "--no-input"])


@pytest.mark.parametrize("command", ["dwelltime", "ttfb"])
@pytest.mark.parametrize("flags,text", [
    (["--smooth", "--joint", "0"], "--joint takes A,B"),
    (["--smooth", "--joint", "0,1,2"], "--joint takes A,B"),
    (["--smooth", "--joint", "a,b"], "--joint takes A,B"),
    (["--smooth", "--joint", "1,1"], "two different channel indices"),
    (["--joint", "0;1", "--cpu"], "--joint takes A,B"),
    (["--joint", "0,1"], "--joint needs --smooth"),
    (["--smooth", "--joint", "0,1", "--bound-states", "2"], "does not go with --unbound-states"),
    (["--smooth", "--joint", "0,1", "--unbound-states", "2"], "does not go with --unbound-states"),
    (["--smooth", "--joint", "0,1", "--populations", "2"], "does not go with --populations"),
    (["--smooth", "--joint", "0,1", "--model", "crosstalk"], "cosmos only"),
    (["--joint", "0,0", "--model", "crosstalk"], "cosmos only"),
    (["--smooth", "--joint", "0,1", "--cpu"], "GPU"),
    (["--joint", "0,1", "--cpu"], "GPU"),
])
def test_joint_flags_are_refused_with_exit_status_1(tmp_path, command, flags, text):
    result = invoke(tmp_path, command, *flags)
    assert result.exit_code == 1, result.output  # 2 = no such option
    assert text in result.output


def test_joint_does_not_go_with_censored(tmp_path):
    result = invoke(tmp_path, "dwelltime", "--smooth", "--joint", "0,1", "--censored")
    assert result.exit_code == 1 and "does not go with --censored" in result.output, result.output
    result = invoke(tmp_path, "ttfb", "--smooth", "--joint", "0,1", "--censored")
    assert result.exit_code == 2, result.output  # ttfb has no such option


@pytest.mark.parametrize("command", ["dwelltime", "ttfb"])
def test_after_loading_the_pair_the_file_and_the_mask_are_checked(tmp_path, caplog, command):
    from tapqir_amd.main import _joint_posterior

    logger = logging.getLogger("tapqir")
    mask = torch.ones(3, dtype=torch.bool)
    m = types.SimpleNamespace(name="cosmos", data=types.SimpleNamespace(C=2))

    def refused(pair, mask, *texts):
        caplog.clear()
        with caplog.at_level(logging.ERROR, logger="tapqir"), pytest.raises(typer.Exit) as exit_info:
            _joint_posterior(command, tmp_path, m, mask, pair, logger)
        assert exit_info.value.exit_code == 1
        for text in texts:
            assert text in caplog.text, caplog.text

    refused((0, 2), mask, "--joint 0,2 needs channels 0 and 2, the data has 2 channels")
    refused((2, 0), mask, "the data has 2 channels")
    refused((1, 0), mask, "cosmos_smooth-joint10.tpqr", "run `smooth --joint 1,0` first")
    torch.save({"theta": torch.zeros(20, dtype=torch.float64), "prior": torch.tensor([0.3, 0.3], dtype=torch.float64),
                "channels": (1, 0), "mask": mask, "chosen": "full"}, tmp_path / "cosmos_smooth-joint10.tpqr")
    assert _joint_posterior(command, tmp_path, m, mask, (1, 0), logger)["chosen"] == "full"
    other = mask.clone()
    other[1] = False
    refused((1, 0), other, "another mask", "run `smooth --joint 1,0` again")
    refused((1, 0), torch.ones(4, dtype=torch.bool), "another mask")


@pytest.mark.parametrize("command", ["dwelltime", "ttfb"])
def test_help_shows_the_option_and_what_is_not_promised(tmp_path, command):
    result = CliRunner().invoke(app, ["--cd", str(tmp_path), command, "--help"])
    assert result.exit_code == 0 and "--joint" in result.output
    text = " ".join(result.output.split())
    assert "smooth --joint A,B" in text and "smooth-joint<A><B>" in text and "not bit for bit" in text
    if command == "ttfb":
        assert "-order.csv" in text and "no (ka, kns, Af) fit" in text and "k_after" in text
    else:
        assert "partner_start" in text and "q<q>_A<i>" in text and "There are no plots" in text and "--censored" in text
