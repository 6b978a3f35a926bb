"""The continuous-time hidden Markov chain on the frame timestamps without a GPU: the g++ build of
tq_timed.h (the tables, the E-step with the device's ownership of frames and scan order, the M-step with the device's
strided sums and tree) against the numpy oracle of timed_fixture by the tolerance rule of section 20, the identities of the
tables, the EM on the two-speed record and its statistical condition, ``timed_gaps``, the C layout of the three argument
structs, the exports, argument validation of the entry points, and the exits and the help text of ``smooth --timed``.  The
``check_*`` functions take a backend, so that tests/test_gpu_timed.py runs them on the kernels."""

import ctypes
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest
import torch
from typer.testing import CliRunner

import hmm_fixture as hf
import timed_fixture as tf
from tapqir_amd import _lib, _lib_timed
from tapqir_amd.main import app
from tapqir_amd.utils.dataset import save
from tapqir_amd.utils.simulate import TEST_PARAMS, simulate
from timed_fixture import PRIOR, rule_bound, rule_excess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UB_OF_M = {2: (1, 1), 3: (1, 2), 4: (2, 2)}
EPS = float(np.spacing(1.0))


class HostBackend:
    """The g++ builds behind the interface the checks use: numpy in, numpy out."""

    name = "g++"

    def __init__(self, timed, hmm):
        self.timed, self.hmm = timed, hmm

    def tables(self, theta, d, U, B, allow):
        return tf.host_tables(self.timed, theta, d, U, B, allow)

    def estep(self, p, theta, P, K, cls, U, B, allow, gamma=True):
        return tf.host_estep(self.timed, p, theta, P, K, cls, U, B, allow, PRIOR, gamma)

    def mstep(self, rows, theta, U, B, allow):
        return tf.host_mstep(self.timed, rows, theta, U, B, allow)

    def em(self, p, theta0, d, cls, U, B, allow, num_iter):
        return tf.host_em(self.timed, p, PRIOR, theta0, d, cls, U, B, allow, num_iter)

    def hmm_estep(self, p, theta, U, B):
        return hf.host_estep(self.hmm, p, theta, U, B, PRIOR)

    def fits(self, p, times, U, B, num_iter):
        """The timed and the per-frame EM of ``num_iter`` iterations from their default starts: (kon, koff) per unit of
        ``times`` and the two log evidences at the final theta."""
        d, cls, scale = tf.gap_classes(times)
        allow = tf.allow_bits(U + B)
        th, _ = self.em(p, tf.default_start(U, B), d, cls, U, B, allow, num_iter)
        P, K = self.tables(th[-1], d, U, B, allow)
        ll = self.estep(p, th[-1], P, K, cls, U, B, allow, gamma=False)["rows"][:, -1].sum()
        thf, _ = hf.host_em(self.hmm, p, PRIOR, hf.default_start(U, B), U, B, num_iter)
        llf = self.hmm_estep(p, thf[-1], U, B)["rows"][:, -1].sum()
        return th[-1][1] / scale, th[-1][2] / scale, ll, llf


@pytest.fixture(scope="module")
def be(tmp_path_factory):
    d = tmp_path_factory.mktemp("timed")
    return HostBackend(tf.build_timed_check(d), hf.build_hmm_check(d))


# ---- tables -------------------------------------------------------------------------------------------------------------
def check_tables(be, name):
    """P and K of every class against the oracle by the rule; both identities; two runs give the same bits."""
    case = tf.table_case(name)
    U, B, M, d = case["U"], case["B"], case["U"] + case["B"], case["d"]
    P, K = be.tables(case["theta"], d, U, B, case["allow"])
    (P64, K64), (P80, K80) = case["t64"], case["t80"]
    worst = {"P": 0.0, "K": 0.0}
    for k in range(len(d)):  # every class by itself: the sizes of K differ by ten orders of magnitude
        exc = rule_excess(P[k], P64[k], P80[k]), rule_excess(K[k], K64[k], K80[k])
        print(f"{be.name} {name} d = {d[k]:g}: P {exc[0]:.3g}, K {exc[1]:.3g} of the bound")
        assert max(exc) <= 1.0, (name, d[k], exc)
        worst = {"P": max(worst["P"], exc[0]), "K": max(worst["K"], exc[1])}
    assert (P >= 0).all() and (K >= 0).all()
    # sum_b P_ab = 1: the rows are divided by their sums last, M products and M - 1 additions from 1
    assert np.abs(P.sum(-1) - 1).max() <= 2 * M * EPS
    # sum_i K[a][b][i][i] = d P_ab: at most 21 terms and 16 squarings of non-negative sums, each within (2 M + 1) eps
    ident = np.abs(np.einsum("kabii->kab", K) - d[:, None, None] * P) / d[:, None, None]
    print(f"{be.name} {name}: trace identity {ident.max():.3g}, scipy differs from the float64 oracle by "
          f"{tf.scipy_difference(case['theta'], d, U, B, case['allow']):.3g}")
    assert ident.max() <= (21 + 16 * (2 * M + 1)) * (2 * M + 1) * EPS
    # a forbidden rate is an exact zero: at the shortest gap P_ij is second order in d
    if name == "ref":
        assert 0 <= P[0, 1, 2] < 1e-12 and 0 <= P[0, 2, 1] < 1e-12
    P2, K2 = be.tables(case["theta"], d, U, B, case["allow"])
    assert np.array_equal(P2, P) and np.array_equal(K2, K)
    return worst


@pytest.mark.parametrize("name", ["m2", "m3", "m4", "ref"])
def test_tables(be, name):
    check_tables(be, name)


# ---- E-step -------------------------------------------------------------------------------------------------------------
def check_estep(be, F, U, B, pattern, N=6):
    """filt, gamma and rows against the oracle by the rule; the expected times of a row add up to the record's duration;
    gamma = NULL and one class per gap change no bit of the rows."""
    case = tf.estep_case(F, U, B, pattern, N)
    M, theta, allow, d, cls = U + B, case["theta"], case["allow"], case["d"], case["cls"]
    P, K = be.tables(theta, d, U, B, allow)
    got = be.estep(case["p"], theta, P, K, cls, U, B, allow)
    exc = {k: rule_excess(got[k], case["o64"][k], case["o80"][k]) for k in ("filt", "gamma", "rows")}
    print(f"{be.name} F = {F} ({U}, {B}) {pattern}: " + ", ".join(f"{k} {v:.3g}" for k, v in exc.items()) + " of the bound")
    assert max(exc.values()) <= 1.0, exc
    diag = [i * M + i for i in range(M)]
    dur = got["rows"][:, diag].sum(1)
    d64, d80 = case["o64"]["rows"][:, diag].sum(1), case["o80"]["rows"][:, diag].sum(1)
    want = (case["times"][-1] - case["times"][0]) / case["scale"]
    assert np.abs(dur - want).max() <= rule_bound(d64, d80) + 1e-13 * max(1.0, want)
    if F == 1:
        assert (got["rows"][:, : M * M] == 0).all()
    bare = be.estep(case["p"], theta, P, K, cls, U, B, allow, gamma=False)
    assert np.array_equal(bare["rows"], got["rows"]) and np.array_equal(bare["filt"], got["filt"])
    if F > 1:  # the same stamps with one class per gap
        d1, cls1, _ = tf.gap_classes(case["times"], dedup=False)
        P1, K1 = be.tables(theta, d1, U, B, allow)
        each = be.estep(case["p"], theta, P1, K1, cls1, U, B, allow)
        assert all(np.array_equal(each[k], got[k]) for k in ("filt", "gamma", "rows"))
    return exc


@pytest.mark.parametrize("pattern", tf.PATTERNS)
@pytest.mark.parametrize("U,B", tf.UB_LIST)
@pytest.mark.parametrize("F", tf.F_LIST)
def test_estep(be, F, U, B, pattern):
    check_estep(be, F, U, B, pattern)


def test_estep_long_rows(be):
    check_estep(be, 5000, 2, 2, "two-speed", N=2)


def check_forbidden_k_plays_no_part(be):
    """The reference chain with its two zeros forbidden: K[.][.][i][j] of a forbidden pair may hold anything, NaN included."""
    F, U, B = 65, 1, 2
    case = tf.estep_case(F, U, B, "two-speed", forbidden=True)
    theta, allow, d, cls = case["theta"], case["allow"], case["d"], case["cls"]
    P, K = be.tables(theta, d, U, B, allow)
    got = be.estep(case["p"], theta, P, K, cls, U, B, allow)
    exc = {k: rule_excess(got[k], case["o64"][k], case["o80"][k]) for k in ("filt", "gamma", "rows")}
    print(f"{be.name} forbidden: " + ", ".join(f"{k} {v:.3g}" for k, v in exc.items()) + " of the bound")
    assert max(exc.values()) <= 1.0, exc
    assert (got["rows"][:, [1 * 3 + 2, 2 * 3 + 1]] == 0).all()
    poisoned = K.copy()
    poisoned[:, :, :, 1, 2] = np.nan
    poisoned[:, :, :, 2, 1] = 1e300
    again = be.estep(case["p"], theta, P, poisoned, cls, U, B, allow)
    assert all(np.array_equal(again[k], got[k]) for k in ("filt", "gamma", "rows"))


def test_forbidden_k_plays_no_part(be):
    check_forbidden_k_plays_no_part(be)


def check_equal_spacing_is_the_per_frame_chain(be, F, U, B):
    """D = 1, d = 1: filt, gamma and the log evidence are those of tq_hmm_estep at A = the oracle's P, within twice the
    rule's bound."""
    case = tf.estep_case(F, U, B, "equal")
    theta, allow = case["theta"], case["allow"]
    assert len(case["d"]) == 1 and case["d"][0] == 1.0
    P, K = be.tables(theta, case["d"], U, B, allow)
    got = be.estep(case["p"], theta, P, K, case["cls"], U, B, allow)
    A = tf.oracle_tables(theta, case["d"], U, B, allow)[0][0]
    frame = be.hmm_estep(case["p"], tf.pack(A, theta[(U + B) ** 2:]), U, B)
    for k in ("filt", "gamma"):
        assert np.abs(frame[k] - got[k]).max() <= 2 * rule_bound(case["o64"][k], case["o80"][k]), k
    ll64, ll80 = case["o64"]["rows"][:, -1], case["o80"]["rows"][:, -1]
    assert np.abs(frame["rows"][:, -1] - got["rows"][:, -1]).max() <= 2 * rule_bound(ll64, ll80)


@pytest.mark.parametrize("U,B", tf.UB_LIST)
@pytest.mark.parametrize("F", [2, 65, 203])
def test_equal_spacing_is_the_per_frame_chain(be, F, U, B):
    check_equal_spacing_is_the_per_frame_chain(be, F, U, B)


# ---- M-step -------------------------------------------------------------------------------------------------------------
def mstep_case(N, M):
    U, B = UB_OF_M[M]
    rng = np.random.default_rng(100 * N + M)
    rows = rng.random((N, tf.cols(M)))
    rows[:, [i * M + i for i in range(M)]] *= 20.0  # times are longer than jumps are many
    rows[:, M * M: M * M + M] /= rows[:, M * M: M * M + M].sum(1, keepdims=True)
    rows[:, -1] = -50.0 * rng.random(N) - 1.0
    return U, B, rows, tf.fixed_theta(U, B, seed=2)


def check_mstep(be, N, M):
    U, B, rows, theta0 = mstep_case(N, M)
    full = tf.allow_bits(M)
    got, ll = be.mstep(rows, theta0, U, B, full)
    t64, l64 = tf.oracle_mstep(rows, theta0, U, B, full)
    t80, l80 = tf.oracle_mstep(rows, theta0, U, B, full, np.longdouble)
    exc = rule_excess(got, t64, t80), rule_excess([ll], [l64], [l80])
    print(f"{be.name} N = {N} M = {M}: theta {exc[0]:.3g}, loglik {exc[1]:.3g} of the bound")
    assert max(exc) <= 1.0, exc
    Q = got[: M * M].reshape(M, M)
    assert np.abs(Q.sum(1)).max() <= 4 * M * EPS * np.abs(Q).max() and abs(got[M * M:].sum() - 1) <= 4 * EPS
    # a cleared allow bit stays exactly 0, whatever the rows and the old theta hold there
    allow = tf.allow_bits(M, [(0, M - 1)])
    masked, _ = be.mstep(rows, theta0, U, B, allow)
    m64, _ = tf.oracle_mstep(rows, theta0, U, B, allow)
    m80, _ = tf.oracle_mstep(rows, theta0, U, B, allow, np.longdouble)
    assert masked[M - 1] == 0.0 and rule_excess(masked, m64, m80) <= 1.0
    off = ~np.eye(M, dtype=bool) & tf.allow_matrix(M, allow)
    assert (masked[: M * M].reshape(M, M)[off] >= 1e-9).all()
    # a state without expected time keeps its rates
    empty = rows.copy()
    empty[:, 1 * M + 1] = 0.0
    kept, _ = be.mstep(empty, theta0, U, B, full)
    assert np.array_equal(kept[M:2 * M][np.arange(M) != 1], theta0[M:2 * M][np.arange(M) != 1])
    assert np.array_equal(kept[:M], got[:M])
    # two runs give the same bits
    again, ll2 = be.mstep(rows, theta0, U, B, full)
    assert np.array_equal(again, got) and ll2 == ll
    return exc


@pytest.mark.parametrize("M", [2, 3, 4])
@pytest.mark.parametrize("N", [1, 2, 255, 256, 257])
def test_mstep(be, N, M):
    check_mstep(be, N, M)


# ---- fit ----------------------------------------------------------------------------------------------------------------
def check_fit(be, U, B):
    """25 EM iterations on the two-speed record (N = 40, F = 500, every gap its own class): theta and the trace of every
    iteration against the oracle's by the rule, and a trace that does not decrease beyond the rule's bound."""
    case = tf.fit_case(U, B)
    T = 25
    thetas, trace = be.em(case["p"], case["start"], case["d"], case["cls"], U, B, case["allow"], T)
    worst = 0.0
    for it in range(1, T + 1):
        exc = rule_excess(thetas[it], case["th64"][it], case["th80"][it])
        assert exc <= 1.0, (it, exc)
        worst = max(worst, exc)
    exc = rule_excess(trace, case["tr64"], case["tr80"])
    print(f"{be.name} ({U}, {B}): theta of every iteration {worst:.3g}, trace {exc:.3g} of the bound")
    assert exc <= 1.0
    assert np.diff(trace).min() >= -rule_bound(case["tr64"], case["tr80"])
    return worst, exc


@pytest.mark.parametrize("U,B", [(1, 1), (1, 2)])
def test_fit_follows_the_oracles_em(be, U, B):
    check_fit(be, U, B)


def check_statistical_condition(be):
    """The two-speed record generated at kon 0.05 / s and koff 0.10 / s, at most 200 iterations: both fitted rates within
    10 % of the generating ones, and the timed log evidence at least 100 above the per-frame chain's.  The seed of the
    record was fixed after the float64 oracle alone gave 0.0502 / 0.1031 and +249.85 for it."""
    p, times = tf.record()
    kon, koff, ll, llf = be.fits(p, times, 1, 1, 200)
    print(f"{be.name}: kon {kon:.5f} koff {koff:.5f} per second; log evidence {ll:.3f} timed, {llf:.3f} per frame, "
          f"gain {ll - llf:+.2f}")
    assert abs(kon / tf.KON - 1) <= 0.10 and abs(koff / tf.KOFF - 1) <= 0.10
    assert ll - llf >= 100.0


def test_statistical_condition(be):
    check_statistical_condition(be)


# ---- gaps ---------------------------------------------------------------------------------------------------------------
def test_timed_gaps():
    from tapqir_amd.utils.mle_analysis import timed_canonical_order, timed_default_start, timed_gaps

    for F, pattern, D in ((5, "equal", 1), (203, "two-speed", 3), (65, "jitter", 64)):
        times = tf.stamps(F, pattern, seed=F)
        d, cls, scale = timed_gaps(torch.from_numpy(times))
        wd, wcls, wscale = tf.gap_classes(times)
        assert d.dtype == torch.float64 and cls.dtype == torch.int32 and len(d) == D and len(cls) == F - 1
        assert np.array_equal(d.numpy(), wd) and np.array_equal(cls.numpy(), wcls) and scale == wscale
        assert np.array_equal((d[cls.long()] * scale).numpy(), np.diff(times) / scale * scale)
    d, cls, scale = timed_gaps([3.0])
    assert d.tolist() == [1.0] and cls.numel() == 0 and scale == 1.0
    for bad in ([0.0, 1.0, 1.0], [0.0, 2.0, 1.0], [0.0, float("nan"), 2.0], [0.0, float("inf")], []):
        with pytest.raises(ValueError):
            timed_gaps(bad)
    for U, B in tf.UB_LIST:
        Q, rho = timed_default_start(U, B)
        assert np.allclose(tf.pack(Q.numpy(), rho.numpy()), tf.default_start(U, B), rtol=0, atol=1e-16)
    theta = torch.from_numpy(tf.pack([[-9, 0.2, 0.1, 0.0], [0.5, 0, 0.1, 0.1], [0.3, 0.3, 0, 0.3], [0.1, 0.1, 0.1, 5]], [0.25] * 4))
    assert timed_canonical_order(theta, 2, 2) == [0, 1, 3, 2]


# ---- ABI ------------------------------------------------------------------------------------------------------------
def header_text():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tapqir_hip.h")).read(), flags=re.S)


def header_fields(name):
    """Field names of ``typedef struct { ... } name;`` in include/tapqir_hip.h, in order."""
    body = re.search(r"typedef struct \{([^{}]*)\}\s*%s;" % name, header_text()).group(1)
    out = []
    for decl in body.split(";"):
        if decl.strip():
            out += [re.search(r"(\w+)\s*$", d.strip()).group(1) for d in decl.split(",")]
    return out


MIRRORS = {"tq_timed_table_args": _lib_timed.TimedTableArgs, "tq_timed_estep_args": _lib_timed.TimedEstepArgs,
           "tq_timed_mstep_args": _lib_timed.TimedMstepArgs}


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
           + "\n  return 0;\n}\n")
    with tempfile.TemporaryDirectory() as td:
        c = os.path.join(td, "s.c")
        open(c, "w").write(src)
        exe = os.path.join(td, "s")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        got = [int(v) for v in subprocess.check_output([exe]).split()]
    assert len(got) == len(want)
    assert [(n, f, g) for (n, f, _), g in zip(want, got)] == want


def test_exports_are_the_headers_declarations():
    names = {"tq_timed_table", "tq_timed_estep", "tq_timed_mstep"}
    declared = set(re.findall(r"\b(tq_[a-z_0-9]+)\s*\(", header_text()))
    assert {n for n in declared if n.startswith("tq_timed_")} == names
    assert names == {n for n in _lib.EXPORTS if n.startswith("tq_timed_")}
    lib = _lib_timed.lib()
    assert all(hasattr(lib, n) for n in names)


def test_argument_validation_returns_error_codes_without_a_gpu():
    lib = _lib_timed.lib()
    buf = (ctypes.c_int64 * 8)()
    addr = ctypes.addressof(buf)
    gaps = (ctypes.c_double * 3)(0.5, 1.0, 2.0)
    classes = (ctypes.c_int32 * 4)(0, 2, 1, 1)
    A = _lib_timed
    calls = {"table": (lib.tq_timed_table, A.TimedTableArgs,
                       dict(theta=addr, d=addr, d_host=ctypes.addressof(gaps), P=addr, K=addr, D=3, U=1, B=2, allow=0x1FF)),
             "estep": (lib.tq_timed_estep, A.TimedEstepArgs,
                       dict(p=addr, theta=addr, P=addr, K=addr, cls=addr, cls_host=ctypes.addressof(classes), filt=addr,
                            rows=addr, N=3, F=5, D=3, U=1, B=2, allow=0x1FF, prior=0.3)),
             "mstep": (lib.tq_timed_mstep, A.TimedMstepArgs,
                       dict(rows=addr, theta=addr, trace=addr, N=3, it=0, T=1, U=1, B=2, allow=0x1FF))}

    def refused(name, text, **change):
        fn, cls, good = calls[name]
        assert fn(ctypes.byref(cls(**{**good, **change})), None) == 1, (name, change)  # TQ_ERR_ARG
        err = lib.tq_last_error()
        assert ("tq_timed_" + name).encode() in err and text in err, err

    for name, (fn, cls, good) in calls.items():
        assert fn(None, None) == 1
        assert fn(ctypes.byref(cls()), None) == 1 and b"NULL" in lib.tq_last_error()
        for key, value in good.items():
            if key not in ("N", "F", "D", "U", "B", "allow", "prior", "it", "T"):
                refused(name, b"NULL", **{key: None})
        for U, B in ((0, 2), (2, 0), (-1, 3), (1, 4), (3, 2), (4, 1)):
            refused(name, b"U + B at most 4", U=U, B=B)
        refused(name, b"allow", allow=0x3FF)      # a bit beyond M * M = 9
        refused(name, b"allow", allow=0x1FF & ~0b111000)  # row 1 has no set bit
        refused(name, b"allow", allow=0)
    for name in ("table", "estep"):
        for D in (0, -1):
            refused(name, b"D must be positive", D=D)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        for k in range(3):
            g = (ctypes.c_double * 3)(0.5, 1.0, 2.0)
            g[k] = bad
            refused("table", b"finite and positive", d_host=ctypes.addressof(g))
    for k, bad in ((0, -1), (3, 3), (1, 2**31 - 1)):
        c = (ctypes.c_int32 * 4)(0, 2, 1, 1)
        c[k] = bad
        refused("estep", b"[0, D)", cls_host=ctypes.addressof(c))
    refused("estep", b"[0, D)", D=2)
    refused("estep", b"positive", N=0)
    refused("estep", b"positive", F=0)
    refused("estep", b"65536", F=65537)
    for prior in (0.0, 1.0, -0.5, float("nan")):
        refused("estep", b"prior", prior=prior)
    refused("mstep", b"positive", N=0)
    refused("mstep", b"non-negative", it=-1)
    refused("mstep", b"T must exceed it", it=1, T=1)
    refused("mstep", b"T must exceed it", it=0, T=0)


def test_device_entry_points_refuse_host_tensors_and_bad_arguments():
    from tapqir_amd.exceptions import HipExtensionError
    from tapqir_amd.utils import mle_analysis as ma

    p, theta = torch.rand(3, 5), torch.from_numpy(tf.fixed_theta(1, 2))
    times = torch.arange(5.0)
    with pytest.raises(HipExtensionError):
        ma.timed_fit(p, PRIOR, times, 1, 2)
    with pytest.raises(HipExtensionError):
        ma.timed_tables(theta, [1.0], 1, 2)
    with pytest.raises(HipExtensionError):
        ma.timed_estep(p, theta, {"P": torch.zeros(1, 3, 3), "K": torch.zeros(1, 3, 3, 3, 3)}, [0] * 4, PRIOR, 1, 2)
    with pytest.raises(HipExtensionError):
        ma.timed_mstep(torch.rand(3, 13, dtype=torch.float64), theta, torch.zeros(1, dtype=torch.float64), 0, 1, 2)
    for U, B in ((0, 1), (1, 0), (3, 2), (1, 4)):
        with pytest.raises(ValueError):
            ma.timed_fit(p, PRIOR, times, U, B)
    for bad in (dict(num_iter=0), dict(allow=torch.ones(2, 2)), dict(Q0=torch.ones(2, 2)), dict(Q0=-torch.ones(3, 3)),
                dict(rho0=torch.zeros(3))):
        with pytest.raises(ValueError):
            ma.timed_fit(p, PRIOR, times, 1, 2, **bad)
    with pytest.raises(ValueError):
        ma.timed_fit(p, PRIOR, torch.tensor([0.0, 1.0, 1.0, 2.0, 3.0]), 1, 2)


# ---- command line -----------------------------------------------------------------------------------------------------
GOES_WITH = "--timed does not go with --restarts, --refit, --joint, --structure or --populations"


@pytest.mark.parametrize("flags,text", [
    (["--timed", "--restarts", "4", "--bound-states", "2"], GOES_WITH),
    (["--timed", "--refit", "4"], GOES_WITH),
    (["--timed", "--joint", "0,1"], GOES_WITH),
    (["--timed", "--structure", "full"], GOES_WITH),
    (["--timed", "--populations", "2"], GOES_WITH),
    (["--timed", "--refit", "4", "--cpu"], GOES_WITH),
    (["--frame-time", "0.5"], "--frame-time needs --timed"),
    (["--timed", "--forbid", "0-0"], "--forbid takes i-j"),
    (["--timed", "--forbid", "0-1", "--cpu"], "GPU"),
    (["--timed", "--cpu"], "GPU"),
    (["--timed", "--frame-time", "0.5", "--bound-states", "2", "--cpu"], "GPU"),
    (["--timed", "--model", "crosstalk"], "cosmos only"),
])
def test_smooth_refusals(tmp_path, flags, text):
    save(simulate(2, 2, 5, 1, 14, params=dict(TEST_PARAMS)), tmp_path)
    result = CliRunner().invoke(app, ["--cd", str(tmp_path), "smooth", *flags, "--num-samples", "10", "--no-input"])
    assert result.exit_code == 1, result.output  # 2 = no such command or option
    assert text in result.output


def test_smooth_help_shows_the_new_options(tmp_path):
    result = CliRunner().invoke(app, ["--cd", str(tmp_path), "smooth", "--help"])
    assert result.exit_code == 0
    for option in ("--timed", "--frame-time", "--time-scale"):
        assert option in result.output
