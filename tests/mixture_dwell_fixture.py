"""Test-side helpers of the ``dwelltime --smooth --populations G`` / ``ttfb --smooth --populations G`` tests (DESIGN.md section
30): the build and binding of the g++ host check of ``tq_population_dwell`` (tests/hostcheck/population_dwell_check.cpp), the
oracle of a raster with its drawn populations, the exact survival law of the first binding under the mixture, and the
conditions the CPU and the GPU tests share.  The oracle of a raster, the two passes and the exact comparison are
smooth_dwell_fixture's; the rasters and populations the oracle is applied to come from the existing samplers
(``mixture_fixture.host_count``, ``mixture_sample``), which run no code of the feature."""

import ctypes as C
import os

import numpy as np

import hmm_dwell_fixture
from helpers import build_host_check
from mixture_fixture import PRIOR, mixture_default_start, normalised, static_data  # noqa: F401 (re-exported)
from smooth_dwell_fixture import F_LIST, _two_passes, assert_equals_oracle, oracle_of_raster  # noqa: F401 (re-exported)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "hostcheck", "population_dwell_check.cpp")
MARGIN = 1e-9  # the rule of sections 22 and 29: a replay stands for the device where no uniform lies this close to a threshold
UB_HOST = [(1, 1), (1, 2), (2, 1), (2, 2), (1, 3)]
G_LIST = [1, 2, 4]
BAR = 0.25  # sections 21 and 25: the error of the new rasters against that of what they replace


# ---- oracle -----------------------------------------------------------------------------------------------------------
def oracle_of_populations(z, pop, G):
    """What ``tq_population_dwell`` must give for the (S, N, F) 0 / 1 raster ``z`` whose rows drew the populations ``pop``
    (S, N): ``smooth_dwell_fixture.oracle_of_raster`` of the whole raster (its pooled histograms as ``pooled_bound`` /
    ``pooled_unbound``), and ``hist_bound`` / ``hist_unbound`` (S, G, F): the oracle's histograms of z * (pop == g).  A row
    outside g becomes one unbound run that touches both ends of the record, so it adds nothing interior."""
    z = np.ascontiguousarray(z, dtype=np.uint8)
    pop = np.asarray(pop)
    want = oracle_of_raster(z)
    out = {**want, "pooled_bound": want["hist_bound"], "pooled_unbound": want["hist_unbound"], "pop": pop.astype(np.int64)}
    for key in ("hist_bound", "hist_unbound"):
        out[key] = np.stack([oracle_of_raster(z * (pop == g)[:, :, None].astype(np.uint8))[key] for g in range(G)], 1)
    return out


def assert_equals_population_oracle(got, want, who=""):
    """counts, tau and the table exactly (``assert_equals_oracle``, which also compares the (S, G, F) histograms), pop, and
    the histograms summed over the populations against the oracle's pooled ones."""
    assert_equals_oracle(got, want, who)
    assert np.asarray(got["pop"]).dtype == np.uint8 and np.array_equal(got["pop"], want["pop"]), (who, "pop")
    for kind in ("bound", "unbound"):
        assert np.array_equal(np.asarray(got[f"hist_{kind}"]).astype(np.int64).sum(1), want[f"pooled_{kind}"]), (who, kind)


def mixture_survival(p, thetas, resp, U, B, prior):
    """Exact P(states 0 .. f all unbound | data) (N, F) under the mixture: sum_g resp[g, n] times the survival of chain g."""
    return sum(np.asarray(resp)[g][:, None] * hmm_dwell_fixture.oracle_survival(p, thetas[g], U, B, prior)
               for g in range(len(thetas)))


# ---- g++ host check -----------------------------------------------------------------------------------------------------
def build_population_dwell_check(out_dir):
    """Compile tests/hostcheck/population_dwell_check.cpp into ``out_dir`` and bind it."""
    so = os.path.join(str(out_dir), "libtq_population_dwell_check.so")
    build_host_check(SRC, so)
    lib = C.CDLL(so)
    vp, i = C.c_void_p, C.c_int
    lib.hk_pd_sample.argtypes = [vp, vp, vp, i, i, i, i, i, i, C.c_uint64, vp, vp, vp, vp, vp, vp, vp, C.c_int64, vp, vp]
    lib.hk_pd_sample.restype = C.c_int
    return lib


def host_sample(lib, filt, thetas, resp, U, B, S, seed, total=None):
    """The g++ replay of tq_population_dwell, both modes: the dict of ``smooth_dwell_fixture.host_sample`` with histograms
    (S, G, F), ``"pop"`` (S, N) uint8 and ``"margins"``: the smallest |u - tail| of the population draws (1 at G = 1) and
    the smallest |u - t| of the state draws."""
    filt = np.ascontiguousarray(filt, dtype=np.float64)
    thetas = np.ascontiguousarray(thetas, dtype=np.float64)
    resp = np.ascontiguousarray(resp, dtype=np.float64)
    G, N, F = filt.shape[:3]
    assert filt.shape == (G, N, F, U + B) and thetas.shape == (G, (U + B) ** 2 + U + B) and resp.shape == (G, N)
    pop = np.full((S, N), 255, np.uint8)
    margins = []

    def run(counts, hb, hu, tau, offsets, cols, n_rows):
        m = np.zeros(2)
        rc = lib.hk_pd_sample(filt.ctypes.data, thetas.ctypes.data, resp.ctypes.data, U, B, G, S, N, F, seed, counts,
                              pop.ctypes.data if cols is None else None, hb, hu, tau, offsets, cols, n_rows, None, m.ctypes.data)
        assert rc == 0
        margins.append(m)

    # _two_passes allocates (S, F) histograms per population count: run it on G * F bins per sample
    out = _two_passes(run, S, N, G * F, total)
    assert np.array_equal(margins[0], margins[1]) and margins[0].min() >= 0.0  # both passes draw the same uniforms
    for key in ("hist_bound", "hist_unbound"):
        out[key] = out[key].reshape(S, G, F)
    return {**out, "pop": pop, "margins": margins[0]}


# ---- the conditions -----------------------------------------------------------------------------------------------------
def interior_mean(hist):
    """Mean dwell over all interior runs of (S, F) histograms, the samples pooled: total frames over total runs."""
    h = np.asarray(hist, dtype=np.float64)
    return float((h * np.arange(h.shape[-1])).sum() / h.sum())


def hidden_of(kind, s):
    """The generator's own raster of ``mixture_fixture.static_data(kind, s)``: (40, F) classes and the generating population
    (40,), from the same calls that draw p."""
    from mixture_fixture import POPS, synthetic_hmm, two_state

    a = synthetic_hmm(24, 300, s, A=two_state(*POPS[kind[0]]))[1]
    b = synthetic_hmm(16, 300, 100 + s, A=two_state(*POPS[kind[1]]))[1]
    return (np.concatenate([a, b]) >= 1).astype(np.uint8), np.repeat([0, 1], [24, 16])


def condition_figures(kind, s, mixture, single, resp):
    """The figures of the conditions on one data set.  ``mixture``: hist_bound (S, 2, F), tau and pop (S, N) of the G = 2
    rasters; ``single``: hist_bound (S, F) and tau (S, N) of the (1, 1) chain's rasters; ``resp`` (2, N) of the mixture.
    Fitted population g(k) is the one holding most AOIs of generator k (by the largest responsibility).  Returns per
    generator k {"dwell": (hidden, mixture, single), "first": (...), "never": (...)}: mean interior bound dwell, mean
    first-binding frame (F where never bound) and the share of AOIs never bound."""
    z, labels = hidden_of(kind, s)
    F = z.shape[1]
    pmap = np.asarray(resp).argmax(0)
    tau_m, tau_s, pop = (np.asarray(x, dtype=np.float64) for x in (mixture["tau"], single["tau"], mixture["pop"]))
    out = {}
    for k in (0, 1):
        g = int(np.bincount(pmap[labels == k], minlength=2).argmax())
        hid = oracle_of_raster(z[None, labels == k])
        sel = pop == g
        out[k] = {"g": g,
                  "dwell": (interior_mean(hid["hist_bound"]), interior_mean(np.asarray(mixture["hist_bound"])[:, g]),
                            interior_mean(single["hist_bound"])),
                  "first": (float(hid["tau"].mean()), float(tau_m[sel].mean()), float(tau_s.mean())),
                  "never": (float((hid["tau"] == F).mean()), float((tau_m[sel] == F).mean()), float((tau_s == F).mean()))}
    return out


def check_conditions(kind, s, figures, who):
    """Prints every figure, then asserts the bar: on XY the mean interior bound dwell of both generators, on XI the mean
    first-binding frame of both and the never-bound share of the inactive one."""
    wanted = [(k, "dwell") for k in (0, 1)] if kind == "XY" else [(0, "first"), (1, "first"), (1, "never")]
    ratios = {}
    for k, key in wanted:
        hidden, mix, single = figures[k][key]
        ratios[k, key] = abs(mix - hidden) / abs(single - hidden)
        print(f"{who} {kind} s = {s}, generator {kind[k]} (fitted population {figures[k]['g']}), {key}: hidden {hidden:.3f}, "
              f"G = 2 {mix:.3f}, (1, 1) pooled {single:.3f}, error ratio {ratios[k, key]:.3f}")
    for pair, ratio in ratios.items():
        assert ratio <= BAR, (kind, s, pair, ratio)
    return ratios
