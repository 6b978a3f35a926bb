"""Test-side helpers of the multi-state ``dwelltime --smooth`` / ``ttfb --smooth`` tests: the build
and binding of the g++ host check of ``tq_chain_dwell`` (tests/hostcheck/hmm_dwell_check.cpp), the exact survival law of
the first binding of the multi-state chain in float64 numpy, and the three conditions the CPU and the GPU tests share.  The
oracle of a raster, the two passes and the exact comparison are smooth_dwell_fixture's; the rasters the oracle is applied to
come from the existing samplers (``hmm_fixture.host_count``, ``hmm_sample``), which run no code of the feature."""

import ctypes as C
import os

import numpy as np

from helpers import build_host_check
from hmm_fixture import PRIOR, UB_LIST, _evidence, _model, oracle_estep  # noqa: F401 (re-exported)
from smooth_dwell_fixture import F_LIST, _two_passes, interior_means  # noqa: F401 (re-exported)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "hostcheck", "hmm_dwell_check.cpp")
MARGIN = 1e-9  # the rule of section 22: a replay stands for the device where no uniform lies this close to a threshold


# ---- oracle -----------------------------------------------------------------------------------------------------------
def oracle_survival(p, theta, U, B, prior):
    """Exact P(states 0 .. f all unbound | data) (N, F) of the multi-state chain, float64: sum_{j < U} w_f(j) with
    w_0 = gamma_0 restricted to the unbound states and w_{g+1}(j) = sum_{i < U} w_g(i) P(s_{g+1} = j | s_g = i, data),
    P(s_{g+1} = j | s_g = i, data) ~ A_ij l_{g+1}(j) beta_{g+1}(j); gamma_0 from ``oracle_estep``, beta from the same A
    and l."""
    M = U + B
    A, _, inv = _model(theta, U, B, prior, np.float64)
    ell = _evidence(p, inv, U, B, np.float64)
    N, F = ell.shape[:2]
    beta = np.ones((N, F, M))
    for f in range(F - 2, -1, -1):
        b = (ell[:, f + 1] * beta[:, f + 1]) @ A.T
        beta[:, f] = b / b.sum(-1)[:, None]
    w = oracle_estep(p, theta, U, B, prior)["gamma"][:, 0, :U].copy()  # (N, U)
    surv = np.zeros((N, F))
    surv[:, 0] = w.sum(-1)
    for g in range(F - 1):
        step = A[None, :U, :] * (ell[:, g + 1] * beta[:, g + 1])[:, None, :]  # (N, i < U, j)
        step = step / step.sum(-1, keepdims=True)
        w = np.einsum("ni,nij->nj", w, step[:, :, :U])
        surv[:, g + 1] = w.sum(-1)
    return surv


# ---- g++ host check -----------------------------------------------------------------------------------------------------
def build_hmm_dwell_check(out_dir):
    """Compile tests/hostcheck/hmm_dwell_check.cpp into ``out_dir`` and bind it."""
    so = os.path.join(str(out_dir), "libtq_hmm_dwell_check.so")
    build_host_check(SRC, so)
    lib = C.CDLL(so)
    vp, i = C.c_void_p, C.c_int
    lib.hk_hd_sample.argtypes = [vp, vp, i, i, i, i, i, C.c_uint64, vp, vp, vp, vp, vp, vp, C.c_int64, vp]
    lib.hk_hd_sample.restype = C.c_double
    return lib


def host_sample(lib, filt, theta, U, B, S, seed, total=None):
    """The g++ replay of tq_chain_dwell, both modes: the dict of ``smooth_dwell_fixture.host_sample`` and ``"margin"``,
    the smallest |u - t| of all compares."""
    filt = np.ascontiguousarray(filt, dtype=np.float64)
    theta = np.ascontiguousarray(theta, dtype=np.float64)
    N, F = filt.shape[:2]
    assert filt.shape == (N, F, U + B)
    margins = []

    def run(*a):
        margins.append(lib.hk_hd_sample(filt.ctypes.data, theta.ctypes.data, U, B, S, N, F, seed, *a, None))

    out = _two_passes(run, S, N, F, total)
    assert margins[0] == margins[1] >= 0.0  # both passes draw the same uniforms against the same thresholds
    return {**out, "margin": margins[0]}


# ---- the conditions -----------------------------------------------------------------------------------------------------
def check_what_it_is_for(hidden, independent, one_one, one_two):
    """Conditions 1 and 2.  Every argument is a dict of ``hist_bound``, ``hist_unbound`` (S, F) and ``tau`` (S, N) as numpy
    arrays: the hidden raster's, the independent draws', and the new kernel's at (1, 1) and at (1, 2).  Prints every figure
    before it asserts."""
    cases = (hidden, independent, one_one, one_two)
    means = {key: [interior_means(x[key]) for x in cases] for key in ("hist_bound", "hist_unbound")}
    means["tau"] = [float(np.asarray(x["tau"], dtype=np.float64).mean()) for x in cases]
    for key, (h, i, a, b) in means.items():
        print(f"{key}: hidden {h:.3f}, independent {i:.3f}, (1, 1) {a:.3f}, (1, 2) {b:.3f}; |(1, 2) - hidden| = "
              f"{abs(b - h):.3f} against {abs(a - h):.3f} of (1, 1) (ratio {abs(b - h) / abs(a - h):.3f}) and "
              f"{abs(i - h):.3f} of independent draws (ratio {abs(b - h) / abs(i - h):.4f})")
    for key in ("hist_bound", "hist_unbound"):
        h, i, a, b = means[key]
        assert abs(b - h) <= 0.25 * abs(a - h), key
        assert abs(b - h) <= 0.25 * abs(i - h), key
    h, i, a, b = means["tau"]
    assert abs(b - h) <= 0.5 * abs(i - h)
