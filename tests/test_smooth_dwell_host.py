"""``dwelltime --smooth`` / ``ttfb --smooth`` without a GPU: the g++ build of the backward interval walker of tq_smooth.h on
fixed rasters and as a replay of ``tq_smooth_dwell`` (both modes), exactly equal to the host functions of
``tapqir_amd.utils.imscroll`` on the raster of the existing replay ``host_count``; the law of the first binding and the
size of the correction on that replay; the C layout of the argument struct, the refusals of the entry point, and the exits
of the two commands off the device or off cosmos."""

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
from smooth_dwell_fixture import (F_LIST, assert_equals_oracle, build_smooth_dwell_check, host_sample, host_walk,
                                  interior_means, n01_of_table, oracle_of_raster, oracle_survival, survival_deviation)
from smooth_fixture import build_smooth_check, host_count, host_em, host_estep, synthetic_chain, with_special_rows
from tapqir_amd import _lib, _lib_smooth
from tapqir_amd.main import app
from tapqir_amd.utils.dataset import save
from tapqir_amd.utils.imscroll import count_intervals, time_to_first_binding
from tapqir_amd.utils.simulate import TEST_PARAMS, simulate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRIOR = 1.0 / 3.0
THETA = (0.05, 0.10, 0.4)


@pytest.fixture(scope="module")
def hk(tmp_path_factory):
    return build_smooth_dwell_check(tmp_path_factory.mktemp("smooth_dwell"))


@pytest.fixture(scope="module")
def hk_smooth(tmp_path_factory):
    return build_smooth_check(tmp_path_factory.mktemp("smooth"))


# ---- the walker alone -------------------------------------------------------------------------------------------------
def fixed_rasters(F):
    """(2, 6, F): all 0, all 1, alternating from 0 and from 1, a single bound frame at 0 and at F - 1; sample 1 is the
    complement of sample 0."""
    z = np.zeros((6, F), np.uint8)
    z[1] = 1
    z[2] = np.arange(F) % 2
    z[3] = (np.arange(F) + 1) % 2
    z[4, 0] = 1
    z[5, F - 1] = 1
    return np.stack([z, 1 - z])


@pytest.mark.parametrize("F", [1, 2, 3, 8, 64, 65])
def test_walker_equals_count_intervals_on_fixed_rasters(hk, F):
    z = fixed_rasters(F)
    got, want = host_walk(hk, z), oracle_of_raster(z)
    assert_equals_oracle(got, want, f"F = {F}")
    assert (got["counts"][:, 2:4] == F).all()  # alternating: F intervals of length 1, the most a row can have
    assert (got["counts"][:, :2] == 1).all()
    assert got["tau"][0].tolist() == [F, 0, min(1, F), 0, 0, F - 1]
    table = got["table"]
    assert (table.groupby(["posterior_sample", "aoi"])["dwell_time"].sum() == F).all()
    if F == 1:  # one interval per row, first and last at once: the stop type wins
        assert table["low_or_high"].tolist() == [2 + v for v in z.reshape(-1)]


def test_emit_slot_drops_what_lies_outside_the_row(hk):
    slot = hk.hk_sd_emit_slot
    assert [slot(10, 3, k, 100) for k in range(5)] == [12, 11, 10, -1, -1]  # more runs than counted: dropped at the front
    assert [slot(10, 3, k, 12) for k in range(3)] == [-1, 11, 10]  # beyond total: dropped at the end
    assert slot(10, 3, 0, 10) == -1 and slot(10, 0, 0, 100) == -1 and slot(10, -4, 0, 100) == -1
    assert slot(-2, 3, 0, 100) == -1 and slot(-2, 3, 2, 100) == -1


# ---- the replay -------------------------------------------------------------------------------------------------------
def replay_case(hk_smooth, F, S=70, seed=0):
    p = with_special_rows(synthetic_chain(6, F, 0)[0], PRIOR)
    filt = host_estep(hk_smooth, p, THETA, PRIOR)["filt"]
    counts4, raster, margin = host_count(hk_smooth, filt, THETA, S, seed)
    return filt, counts4, raster, margin


@pytest.mark.parametrize("F", F_LIST)
def test_replay_equals_the_host_functions_on_the_raster_of_smooth(hk, hk_smooth, F):
    S = 70
    filt, counts4, raster, _ = replay_case(hk_smooth, F, S)
    got, want = host_sample(hk, filt, THETA, S, seed=0), oracle_of_raster(raster)
    assert_equals_oracle(got, want, f"F = {F}")
    assert got["true_total"] == len(want["table"])
    assert np.array_equal(n01_of_table(got["table"], S, 6), counts4[..., 0])
    assert not raster[:, 0].any() and raster[:, 1].all()
    assert (got["tau"][:, 0] == F).all() and (got["tau"][:, 1] == 0).all()
    assert not np.array_equal(host_sample(hk, filt, THETA, S, seed=1)["tau"], got["tau"]) or F == 1


@pytest.mark.parametrize("F", [2, 65])
def test_short_table_holds_the_first_rows_and_nothing_else(hk, hk_smooth, F):
    S = 70
    filt, _, raster, _ = replay_case(hk_smooth, F, S)
    want = oracle_of_raster(raster)["table"]
    total = len(want) - 1
    got = host_sample(hk, filt, THETA, S, seed=0, total=total)["table"]
    assert len(got) == total
    for col in got.columns:
        assert np.array_equal(got[col].to_numpy(), want[col].to_numpy()[:total]), col
    assert len(host_sample(hk, filt, THETA, S, seed=0, total=0)["table"]) == 0


def test_first_binding_follows_the_exact_survival_law(hk, hk_smooth):
    """S = 4096, N = 4, F = 129: the empirical P(tau > f) within 5 binomial sigma of the exact survival of the smoothed
    chain at every (row, frame) where that lies in [0.02, 0.98]; at least 100 such points.  Generator seed 4 is the first
    of 0 .. 5 whose exact survival (the oracle alone) has that many: 136."""
    S, N, F = 4096, 4, 129
    p = synthetic_chain(N, F, seed=4)[0]
    filt = host_estep(hk_smooth, p, THETA, PRIOR)["filt"]
    tau = host_sample(hk, filt, THETA, S, seed=7)["tau"]
    points, dev = survival_deviation(tau, oracle_survival(p, THETA, PRIOR))
    print(f"{points} points, largest deviation {dev:.2f} sigma")
    assert points >= 100
    assert dev <= 5.0


def test_markov_rasters_mend_the_dwell_times_and_the_first_binding(hk, hk_smooth, tmp_path):
    """N = 40, F = 500, seed 0, 50 EM iterations, S = 64: for the interior bound and unbound dwell times and for tau,
    |Markov - hidden| <= 0.25 |independent - hidden| (means over samples of per-sample means)."""
    S = 64
    p, z = synthetic_chain(40, 500, seed=0)
    theta = host_em(hk_smooth, p, PRIOR, (0.5, 0.5, 0.5), 50)[0][-1]
    filt = host_estep(hk_smooth, p, theta, PRIOR)["filt"]
    markov = host_sample(hk, filt, theta, S, seed=0)
    hkd = dwell_fixture.build_dwell_check(tmp_path)
    _, _, ind_hb, ind_hu = dwell_fixture.host_sample(hkd, p, S, 0)
    ind_tau = time_to_first_binding(dwell_fixture.host_raster(hkd, p, S, 0).astype(np.uint8))
    hidden = oracle_of_raster(z[None])
    for name, h, i, m in (("bound", hidden["hist_bound"], ind_hb, markov["hist_bound"]),
                          ("unbound", hidden["hist_unbound"], ind_hu, markov["hist_unbound"])):
        h, i, m = interior_means(h), interior_means(i), interior_means(m)
        print(f"{name}: hidden {h:.3f}, independent {i:.3f}, Markov {m:.3f}, ratio {abs(m - h) / abs(i - h):.3f}")
        assert abs(m - h) <= 0.25 * abs(i - h)
    h, i, m = hidden["tau"].mean(), ind_tau.mean(), markov["tau"].mean()
    print(f"tau: hidden {h:.3f}, independent {i:.3f}, Markov {m:.3f}, ratio {abs(m - h) / abs(i - h):.3f}")
    assert abs(m - h) <= 0.25 * abs(i - h)


# ---- ABI ------------------------------------------------------------------------------------------------------------
def header_text():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tapqir_hip.h")).read(), flags=re.S)


def test_struct_layout_matches_the_c_header():
    """sizeof and every offsetof of the mirror equal gcc's, and the mirror names the header's fields in order."""
    cls, cname = _lib_smooth.SmoothDwellArgs, "tq_smooth_dwell_args"
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
    assert "tq_smooth_dwell" in _lib.EXPORTS
    assert "tq_smooth_dwell" in set(re.findall(r"\b(tq_[a-z_0-9]+)\s*\(", header_text()))
    assert not hasattr(_lib, "SmoothDwellArgs")
    fn = _lib_smooth.lib().tq_smooth_dwell
    assert fn.restype is ctypes.c_int and fn.argtypes[0]._type_ is _lib_smooth.SmoothDwellArgs


def test_argument_validation_returns_error_codes_without_a_gpu():
    lib = _lib_smooth.lib()
    buf = (ctypes.c_int64 * 8)()
    addr = ctypes.addressof(buf)
    count = dict(filt=addr, theta=addr, counts=addr, hist_bound=addr, hist_unbound=addr, N=3, F=5, S=2,
                 mode=_lib.DWELL_COUNT)
    emit = dict(filt=addr, theta=addr, counts=addr, offsets=addr, intervals=addr, total=4, N=3, F=5, S=2,
                mode=_lib.DWELL_EMIT)

    def call(good, **change):
        return lib.tq_smooth_dwell(ctypes.byref(_lib_smooth.SmoothDwellArgs(**{**good, **change})), None)

    def refused(good, text, **change):
        assert call(good, **change) == 1, change  # TQ_ERR_ARG
        err = lib.tq_last_error()
        assert b"tq_smooth_dwell" in err and text in err, err

    assert lib.tq_smooth_dwell(None, None) == 1
    assert lib.tq_smooth_dwell(ctypes.byref(_lib_smooth.SmoothDwellArgs()), None) == 1 and b"NULL" in lib.tq_last_error()
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
    # EMIT of an empty table launches nothing: TQ_OK with no device in sight, with or without a table pointer
    assert call(emit, total=0) == 0
    assert call(emit, total=0, intervals=None) == 0


def test_device_entry_points_refuse_host_tensors():
    from tapqir_amd.exceptions import HipExtensionError
    from tapqir_amd.utils.mle_analysis import smooth_dwell_intervals, smooth_dwell_sample

    theta = torch.tensor(THETA, dtype=torch.float64)
    filt = torch.rand(3, 5, dtype=torch.float64)
    with pytest.raises(HipExtensionError):
        smooth_dwell_sample(filt, theta, 4)
    with pytest.raises(HipExtensionError):
        smooth_dwell_intervals(filt, theta, 4)


# ---- command line -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("command", ["dwelltime", "ttfb"])
@pytest.mark.parametrize("flags", [["--cpu"], ["--model", "crosstalk"]])
def test_smooth_switch_off_the_device_or_off_cosmos_is_refused(tmp_path, command, flags):
    save(simulate(2, 2, 5, 1, 14, params=dict(TEST_PARAMS)), tmp_path)
    result = CliRunner().invoke(app, ["--cd", str(tmp_path), command, "--smooth", *flags, "--num-samples", "10",
                                      "--no-input"])
    assert result.exit_code == 1, result.output  # 2 = no such option
    assert ("GPU" if flags == ["--cpu"] else "cosmos only") in result.output


def test_hidden_raster_oracle_is_count_intervals(hk):
    """The fixture's oracle on a raster whose table is known by heart."""
    z = np.array([[[0, 1, 1, 0, 0, 0, 1, 0]]], np.uint8)
    want = oracle_of_raster(z)
    assert want["counts"].tolist() == [[5]] and want["tau"].tolist() == [[1]]
    assert want["hist_bound"][0].tolist() == [0, 1, 1, 0, 0, 0, 0, 0]
    assert want["hist_unbound"][0].tolist() == [0, 0, 0, 1, 0, 0, 0, 0]
    assert want["table"]["low_or_high"].tolist() == [-2, 1, 0, 1, 2]
    assert len(count_intervals(z)) == 5
    assert_equals_oracle(host_walk(hk, z), want)
