"""Test-side helpers of the ``dwelltime --smooth --joint A,B`` / ``ttfb --smooth --joint A,B`` tests:
the oracle of a raster of joint states -- ``smooth_dwell_fixture.oracle_of_raster`` on the class view of one channel, and a
plain loop for what is new: the histograms by the partner's state at a run's start, the partner codes and the partner's
first bound frame from the first binding on --, the build and binding of the g++ host check of ``tq_pair_dwell``
(tests/hostcheck/pair_dwell_check.cpp), the order of arrival by a loop, and the condition the CPU and the GPU tests share.
The rasters the oracle is applied to come from the existing samplers (``hmm_fixture.host_count``, ``hmm_sample``), which
run no code of the feature."""

import ctypes as C
import functools
import os

import numpy as np
import pandas as pd

import joint_fixture as jf
from helpers import build_host_check
from smooth_dwell_fixture import F_LIST, assert_equals_oracle, interior_means, oracle_of_raster  # noqa: F401 (re-exported)
from tapqir_amd.utils.imscroll import INTERVAL_COLUMNS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "hostcheck", "pair_dwell_check.cpp")
MARGIN = 1e-9  # the rule of section 22: a replay stands for the device where no uniform lies this close to a threshold
PARTNER_COLUMNS = ["partner_start", "partner_before", "partner_stop", "partner_after"]
BAR = 0.25  # section 21: the error of the new figure against that of what it replaces
HIDDEN_UNBOUND_B = (38.29, 20.67)  # mean interior unbound run of b on the hidden raster, a unbound / bound at its start


# ---- oracle -----------------------------------------------------------------------------------------------------------
def oracle_of_states(r, which):
    """What ``tq_pair_dwell`` must give for the (S, N, F) raster ``r`` of joint states s = z_a + 2 z_b and the channel
    ``which``: ``oracle_of_raster`` of the class view ``(r >> which) & 1`` (its histograms as ``pooled_bound`` /
    ``pooled_unbound``), and by a plain loop over its table ``hist_bound`` / ``hist_unbound`` (S, 2, F) by the partner's
    state at the run's first frame, ``partner`` (one code per interval: bit 0 = q(start), bit 1 = q(start - 1), bit 2 =
    q(stop), bit 3 = q(stop + 1), a frame outside the record counting as 0), the four ``partner_*`` columns (-1 for such
    a frame) and ``tau_after`` (S, N): the smallest f >= tau with q(f) = 1, or F."""
    r = np.ascontiguousarray(r, dtype=np.uint8)
    S, N, F = r.shape
    z, q = (r >> which) & 1, (r >> (1 - which)) & 1
    want = oracle_of_raster(z)
    out = {**want, "pooled_bound": want["hist_bound"], "pooled_unbound": want["hist_unbound"],
           "hist_bound": np.zeros((S, 2, F), np.int64), "hist_unbound": np.zeros((S, 2, F), np.int64)}
    table = want["table"]
    codes = np.zeros(len(table), np.int64)
    columns = {name: np.zeros(len(table), np.int64) for name in PARTNER_COLUMNS}
    rows = zip(table["posterior_sample"], table["aoi"], table["start_frame"], table["stop_frame"], table["dwell_time"],
               table["low_or_high"], table["z"])
    for k, (s, n, start, stop, d, code, zz) in enumerate(rows):
        at = [q[s, n, start], q[s, n, start - 1] if start > 0 else -1, q[s, n, stop], q[s, n, stop + 1] if stop < F - 1 else -1]
        for name, value in zip(PARTNER_COLUMNS, at):
            columns[name][k] = value
        codes[k] = sum(max(int(v), 0) << bit for bit, v in enumerate(at))
        if code in (0, 1):
            out["hist_bound" if zz else "hist_unbound"][s, at[0], d] += 1
    tau_after = np.full((S, N), F, np.int64)
    for s in range(S):
        for n in range(N):
            t = want["tau"][s, n]
            later = np.nonzero(q[s, n, t:])[0] if t < F else []
            if len(later):
                tau_after[s, n] = t + later[0]
    return {**out, "partner": codes, "tau_after": tau_after, **columns}


def assert_equals_pair_oracle(got, want, who=""):
    """counts, tau and the table exactly (``assert_equals_oracle``, which also compares the (S, 2, F) histograms),
    tau_after, the partner codes, and the histograms summed over the partner's state against the oracle's pooled ones."""
    assert_equals_oracle(got, want, who)
    assert np.array_equal(np.asarray(got["tau_after"]).astype(np.int64), want["tau_after"]), (who, "tau_after")
    assert np.asarray(got["partner"]).dtype == np.uint8, who
    assert np.array_equal(np.asarray(got["partner"]).astype(np.int64), want["partner"]), (who, "partner")
    for kind in ("bound", "unbound"):
        assert np.array_equal(np.asarray(got[f"hist_{kind}"]).astype(np.int64).sum(1), want[f"pooled_{kind}"]), (who, kind)


def arrival_order_by_loop(tau_lead, tau_after, tau_partner, F):
    """``joint_arrival_order`` row by row in Python floats: a dict of lists, one entry per sample, NaN for 0 / 0."""
    nan = float("nan")
    out = {key: [] for key in ("binds", "together", "later", "never", "mean_delay", "k_after", "k_base", "ratio")}
    for lead, after, own in zip(*(np.asarray(x, dtype=np.float64).tolist() for x in (tau_lead, tau_after, tau_partner))):
        bound = together = never = events = delay = risk = base_events = base_risk = 0
        for t, ta, tp in zip(lead, after, own):
            if t < F:
                bound += 1
                if ta == F:
                    never += 1
                    risk += F - 1 - t
                elif ta == t:
                    together += 1
                else:
                    events += 1
                    delay += ta - t
                    risk += ta - t
            if tp == F:
                base_risk += F - 1
            elif tp > 0:
                base_events += 1
                base_risk += tp
        k_after = events / risk if risk else nan
        k_base = base_events / base_risk if base_risk else nan
        out["binds"].append(bound / len(lead))
        for key, value in (("together", together), ("later", events), ("never", never)):
            out[key].append(value / bound if bound else nan)
        out["mean_delay"].append(delay / events if events else nan)
        out["k_after"].append(k_after)
        out["k_base"].append(k_base)
        out["ratio"].append(k_after / k_base if k_base == k_base and k_base > 0 else nan)
    return out


# ---- g++ host check -----------------------------------------------------------------------------------------------------
def build_pair_dwell_check(out_dir):
    """Compile tests/hostcheck/pair_dwell_check.cpp into ``out_dir`` and bind it."""
    so = os.path.join(str(out_dir), "libtq_pair_dwell_check.so")
    build_host_check(SRC, so)
    lib = C.CDLL(so)
    vp, i = C.c_void_p, C.c_int
    lib.hk_pw_sample.argtypes = [vp, vp, i, i, i, i, C.c_uint64, vp, vp, vp, vp, vp, vp, vp, vp, C.c_int64, vp]
    lib.hk_pw_sample.restype = C.c_double
    return lib


def host_sample(lib, filt, theta, which, S, seed, total=None):
    """The g++ replay of tq_pair_dwell, both modes: COUNT, the exclusive scan, EMIT into a table and a code array of
    ``total`` entries (default: the true total), preset to -7 / 0xEE with guard entries behind them that must stay.  Returns
    ``table``, ``partner`` (total,) uint8, ``counts``, ``hist_bound`` / ``hist_unbound`` (S, 2, F), ``tau``, ``tau_after``,
    ``true_total`` and ``margin``, the smallest |u - t| of all compares."""
    filt = np.ascontiguousarray(filt, dtype=np.float64)
    theta = np.ascontiguousarray(theta, dtype=np.float64)
    N, F = filt.shape[:2]
    assert filt.shape == (N, F, 4) and theta.shape == (20,)
    counts = np.full((S, N), -1, np.int32)
    hb, hu = np.zeros((S, 2, F), np.int32), np.zeros((S, 2, F), np.int32)
    tau, tau_after = np.full((S, N), -1.0, np.float32), np.full((S, N), -1.0, np.float32)
    m0 = lib.hk_pw_sample(filt.ctypes.data, theta.ctypes.data, which, S, N, F, seed, counts.ctypes.data, hb.ctypes.data,
                          hu.ctypes.data, tau.ctypes.data, tau_after.ctypes.data, None, None, None, 0, None)
    csum = np.cumsum(counts.reshape(-1).astype(np.int64))
    offsets = np.ascontiguousarray(csum - counts.reshape(-1))
    true_total = int(csum[-1])
    total = true_total if total is None else total
    flat = np.full(7 * total + 8, -7, np.int32)
    codes = np.full(total + 8, 0xEE, np.uint8)
    m1 = lib.hk_pw_sample(filt.ctypes.data, theta.ctypes.data, which, S, N, F, seed, counts.ctypes.data, None, None, None, None,
                          offsets.ctypes.data, flat.ctypes.data, codes.ctypes.data, total, None)
    assert m0 == m1 >= 0.0  # both passes draw the same uniforms against the same thresholds
    assert (flat[7 * total:] == -7).all() and (codes[total:] == 0xEE).all()  # nothing behind the table or the codes
    table = flat[: 7 * total].reshape(7, total)
    frame = pd.DataFrame({name: table[i].astype(np.int64) for i, name in enumerate(INTERVAL_COLUMNS)})
    return {"table": frame, "partner": codes[:total].copy(), "counts": counts, "hist_bound": hb, "hist_unbound": hu,
            "tau": tau, "tau_after": tau_after, "true_total": true_total, "margin": m0}


# ---- the condition ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def driven_case():
    """The driven chain N = 40, F = 500, seed 0 of the condition: p_a, p_b (N, F) float32 and the hidden states."""
    return jf.synthetic_joint(40, 500, 0, jf.A_DRIVEN)


def hidden_unbound_means(states, which=1):
    """Mean interior unbound run of channel ``which`` on the hidden raster (N, F) by the partner's state at the run's
    start, and the number of runs: ((mean_0, mean_1), (runs_0, runs_1))."""
    hist = oracle_of_states(np.asarray(states)[None], which)["hist_unbound"][0].astype(np.float64)
    d = np.arange(hist.shape[-1])
    return tuple(float((hist[q] * d).sum() / hist[q].sum()) for q in (0, 1)), tuple(int(hist[q].sum()) for q in (0, 1))


def check_condition(hist_unbound, pooled_unbound, who):
    """``hist_unbound`` (S, 2, F) of the new kernel for channel b and ``pooled_unbound`` (S, F) of ``tq_chain_dwell`` at
    (2, 2) on the same filt.  Prints every figure, then asserts: the q = 0 mean lies above the q = 1 mean, and for each q
    |mean_q - hidden_q| <= 0.25 |pooled - hidden_q|.  Returns (means, pooled, ratios)."""
    hist = np.asarray(hist_unbound)
    means = [interior_means(hist[:, q]) for q in (0, 1)]
    pooled = interior_means(pooled_unbound)
    ratios = [abs(means[q] - HIDDEN_UNBOUND_B[q]) / abs(pooled - HIDDEN_UNBOUND_B[q]) for q in (0, 1)]
    for q in (0, 1):
        print(f"{who}: interior unbound runs of b with a {'bound' if q else 'unbound'} at their start: hidden "
              f"{HIDDEN_UNBOUND_B[q]:.2f}, by partner {means[q]:.3f}, pooled {pooled:.3f}, error ratio {ratios[q]:.3f}")
    assert means[0] > means[1]
    for q in (0, 1):
        assert ratios[q] <= BAR, (who, q, ratios[q])
    return means, pooled, ratios
