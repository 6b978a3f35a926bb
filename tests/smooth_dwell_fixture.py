"""Test-side helpers of the ``dwelltime --smooth`` / ``ttfb --smooth`` tests: the build and binding of the g++ host check of
the backward interval walker (tests/hostcheck/smooth_dwell_check.cpp), the oracle of a raster -- the host functions
``count_intervals``, ``bound_dwell_times``, ``unbound_dwell_times`` and ``time_to_first_binding`` of
``tapqir_amd.utils.imscroll``, which run no code of the feature -- and the exact survival law of the first binding of the
smoothed chain in float64 numpy."""

import ctypes as C
import os

import numpy as np
import pandas as pd

from helpers import build_host_check
from smooth_fixture import _evidence, _model, oracle_estep
from tapqir_amd.utils.imscroll import (INTERVAL_COLUMNS, bound_dwell_times, count_intervals, time_to_first_binding,
                                       unbound_dwell_times)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "hostcheck", "smooth_dwell_check.cpp")
F_LIST = [1, 2, 63, 64, 65, 129, 203]  # one frame, the 64-frame staging block's edge, a ragged last block


# ---- oracle -----------------------------------------------------------------------------------------------------------
def oracle_of_raster(z):
    """What ``tq_smooth_dwell`` must give for the (S, N, F) 0 / 1 raster ``z``: ``table`` (count_intervals, int64 columns),
    ``counts`` (S, N), ``hist_bound`` / ``hist_unbound`` (S, F) and ``tau`` (S, N), all int64.  The histograms are the
    bincounts of ``bound_dwell_times`` / ``unbound_dwell_times`` of each sample's rows taken alone (as sample 0, so that a
    sample without interior runs does not shift the padded rows of the others)."""
    z = np.ascontiguousarray(z, dtype=np.uint8)
    S, N, F = z.shape
    table = count_intervals(z).astype(np.int64)
    assert list(table.columns) == INTERVAL_COLUMNS
    counts = np.bincount(table["posterior_sample"] * N + table["aoi"], minlength=S * N).reshape(S, N)
    hist = {"hist_bound": np.zeros((S, F), np.int64), "hist_unbound": np.zeros((S, F), np.int64)}
    for s, rows in table.groupby("posterior_sample"):
        rows = rows.assign(posterior_sample=0)
        for key, fn in (("hist_bound", bound_dwell_times), ("hist_unbound", unbound_dwell_times)):
            d = fn(rows).reshape(-1)
            hist[key][s] = np.bincount(d[d > 0].astype(np.int64), minlength=F)[:F]
    tau = time_to_first_binding(z)
    assert np.array_equal(tau, np.rint(tau))
    return {"table": table.reset_index(drop=True), "counts": counts, **hist, "tau": tau.astype(np.int64)}


def interior_means(hist):
    """Mean over the samples (that have any) of the per-sample mean dwell time of (S, F) interior-run histograms."""
    h = np.asarray(hist, dtype=np.float64)
    n = h.sum(1)
    return float(((h * np.arange(h.shape[1])).sum(1)[n > 0] / n[n > 0]).mean())


def n01_of_table(table, S, N):
    """(S, N) number of 0 -> 1 steps of every row, recomputed from its interval table: the bound runs that do not start at
    frame 0."""
    rows = table[(table["z"] == 1) & (table["start_frame"] > 0)]
    return np.bincount(rows["posterior_sample"] * N + rows["aoi"], minlength=S * N).reshape(S, N)


def oracle_survival(p, theta, prior):
    """Exact P(z_0 = ... = z_f = 0 | data) (N, F) of the smoothed chain, float64:
    (1 - gamma_0(1)) prod_{g < f} P(z_{g+1} = 0 | z_g = 0, data), P(z_{g+1} = j | z_g = i, data) ~ A_ij l_{g+1}(j)
    beta_{g+1}(j), with gamma_0 from ``oracle_estep`` and beta from the same A and l."""
    A, _, inv = _model(theta, prior, np.float64)
    ell = _evidence(p, inv, np.float64)
    N, F = ell.shape[:2]
    beta = np.ones((N, F, 2))
    for f in range(F - 2, -1, -1):
        b = (ell[:, f + 1] * beta[:, f + 1]) @ A.T
        beta[:, f] = b / b.sum(-1)[:, None]
    surv = np.zeros((N, F))
    surv[:, 0] = 1.0 - oracle_estep(p, theta, prior)["gamma"][:, 0]
    for g in range(F - 1):
        w = A[0][None] * ell[:, g + 1] * beta[:, g + 1]  # (N, j): from state 0
        surv[:, g + 1] = surv[:, g] * w[:, 0] / w.sum(-1)
    return surv


def survival_deviation(tau, surv, lo=0.02, hi=0.98):
    """(number of (row, frame) points with exact survival in [lo, hi], largest |empirical - exact| there in binomial
    sigmas) for first-binding frames ``tau`` (S, N)."""
    tau = np.asarray(tau)
    S = tau.shape[0]
    F = surv.shape[1]
    emp = (tau[:, :, None] > np.arange(F)[None, None]).mean(0)  # (N, F): P(tau > f) = P(z_0 .. z_f = 0)
    sel = (surv >= lo) & (surv <= hi)
    sigma = np.sqrt(surv[sel] * (1.0 - surv[sel]) / S)
    return int(sel.sum()), float((np.abs(emp[sel] - surv[sel]) / sigma).max())


# ---- g++ host check -----------------------------------------------------------------------------------------------------
def build_smooth_dwell_check(out_dir):
    """Compile tests/hostcheck/smooth_dwell_check.cpp into ``out_dir`` and bind it."""
    so = os.path.join(str(out_dir), "libtq_smooth_dwell_check.so")
    build_host_check(SRC, so)
    lib = C.CDLL(so)
    vp = C.c_void_p
    lib.hk_sd_walk.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, C.c_int64]
    lib.hk_sd_walk.restype = None
    lib.hk_sd_sample.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_uint64, vp, vp, vp, vp, vp, vp, C.c_int64]
    lib.hk_sd_sample.restype = None
    lib.hk_sd_emit_slot.argtypes = [C.c_int64, C.c_int, C.c_int, C.c_int64]
    lib.hk_sd_emit_slot.restype = C.c_int64
    return lib


def _two_passes(run, S, N, F, total=None):
    """COUNT, the exclusive scan, EMIT into a table of ``total`` rows (default: the true total), preset to -7 and with
    guard words of -7 behind it.  ``run(counts, hb, hu, tau, offsets, cols, total)`` takes addresses (None for unused)."""
    counts = np.full((S, N), -1, np.int32)
    hb, hu = np.zeros((S, F), np.int32), np.zeros((S, F), np.int32)
    tau = np.full((S, N), -1.0, np.float32)
    run(counts.ctypes.data, hb.ctypes.data, hu.ctypes.data, tau.ctypes.data, None, None, 0)
    csum = np.cumsum(counts.reshape(-1).astype(np.int64))
    offsets = np.ascontiguousarray(csum - counts.reshape(-1))
    true_total = int(csum[-1])
    total = true_total if total is None else total
    flat = np.full(7 * total + 8, -7, np.int32)
    run(counts.ctypes.data, None, None, None, offsets.ctypes.data, flat.ctypes.data, total)
    assert (flat[7 * total:] == -7).all()  # nothing behind the table is written
    table = flat[: 7 * total].reshape(7, total)
    frame = pd.DataFrame({name: table[i].astype(np.int64) for i, name in enumerate(INTERVAL_COLUMNS)})
    return {"table": frame, "counts": counts, "hist_bound": hb, "hist_unbound": hu, "tau": tau, "true_total": true_total}


def host_walk(lib, z, total=None):
    """The g++ backward walker on a (S, N, F) 0 / 1 raster, both modes."""
    z = np.ascontiguousarray(z, dtype=np.uint8)
    S, N, F = z.shape
    return _two_passes(lambda *a: lib.hk_sd_walk(z.ctypes.data, S, N, F, *a), S, N, F, total)


def host_sample(lib, filt, theta, S, seed, total=None):
    """The g++ replay of tq_smooth_dwell, both modes."""
    filt = np.ascontiguousarray(filt, dtype=np.float64)
    theta = np.ascontiguousarray(theta, dtype=np.float64)
    N, F = filt.shape
    return _two_passes(lambda *a: lib.hk_sd_sample(filt.ctypes.data, theta.ctypes.data, S, N, F, seed, *a), S, N, F, total)


def assert_equals_oracle(got, want, who=""):
    """counts, both histograms, tau and the whole table, exactly."""
    for key in ("counts", "hist_bound", "hist_unbound", "tau"):
        g = np.asarray(got[key])
        assert g.shape == want[key].shape, (who, key, g.shape, want[key].shape)
        assert np.array_equal(g.astype(np.int64), want[key]), (who, key)
    assert list(got["table"].columns) == INTERVAL_COLUMNS
    assert len(got["table"]) == len(want["table"]), (who, len(got["table"]), len(want["table"]))
    for col in INTERVAL_COLUMNS:
        assert np.array_equal(got["table"][col].to_numpy(), want["table"][col].to_numpy()), (who, col)
