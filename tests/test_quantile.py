"""The g++ build of the credible-interval bodies (tapqir_amd/csrc/tq_quantile.h) against scipy: quantiles on the whole
grid, the complement identities of the two incomplete functions, and the iteration caps on out-of-domain input."""

import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
from scipy import stats as sps

from helpers import build_host_check
from quantile_host import host_intervals, open_lib
from quantile_fixture import BOUNDS, CIS, KIND_AFFINE_BETA, KIND_GAMMA, TOL, beta_grid, beta_oracle, gamma_grid, gamma_oracle, worst_error

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostcheck", "quantile_check.cpp")


@pytest.fixture(scope="module")
def so_path(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("quantile") / "quantile_check.so")
    build_host_check(SRC, so)
    return so


@pytest.fixture(scope="module")
def lib(so_path):
    return open_lib(so_path)


@pytest.mark.parametrize("CI", CIS)
def test_gamma_quantiles_match_scipy(lib, CI):
    loc, beta = gamma_grid()
    ll, ul = host_intervals(lib, KIND_GAMMA, loc.numpy(), beta.numpy(), 0.0, 0.0, CI)
    err = worst_error(ll, ul, *gamma_oracle(CI))
    print(f"gamma host CI={CI}: worst error / width = {err:.3e}")
    assert err <= TOL


@pytest.mark.parametrize("CI", CIS)
@pytest.mark.parametrize("bounds", BOUNDS)
def test_beta_quantiles_match_scipy(lib, bounds, CI):
    mean, size = beta_grid(*bounds)
    ll, ul = host_intervals(lib, KIND_AFFINE_BETA, mean.numpy(), size.numpy(), bounds[0], bounds[1], CI)
    err = worst_error(ll, ul, *beta_oracle(*bounds, CI))
    print(f"beta host {bounds} CI={CI}: worst error / width = {err:.3e}")
    assert err <= TOL


def test_gamma_tails_sum_to_one(lib):
    """P + Q = 1 at the scipy quantiles of the grid, and P is the probability the quantile was taken at."""
    loc, beta = gamma_grid()
    conc = (loc * beta).double().numpy()
    P, Q = C.c_double(), C.c_double()
    for CI in CIS:
        for q in ((1 - CI) / 2, (1 + CI) / 2):
            for a, y in zip(conc, sps.gamma(conc).ppf(q)):
                lib.hq_igamma(a, y, C.byref(P), C.byref(Q))
                assert abs(P.value + Q.value - 1.0) <= 1e-13, (a, y)
                assert 0.0 <= P.value <= 1.0 and 0.0 <= Q.value <= 1.0
                if y > 1e-300:
                    assert abs(P.value - q) <= 1e-9 * min(q, 1 - q), (a, y, q)


def test_beta_tails_sum_to_one(lib):
    """I_x(a, b) + I_{1-x}(b, a) = 1 at the scipy quantiles of the grid, evaluated from both ends."""
    low, high = BOUNDS[0]
    mean, size = (v.double().numpy() for v in beta_grid(low, high))
    c1, c0 = size * (mean - low) / (high - low), size * (high - mean) / (high - low)
    P, Q, P2, Q2 = C.c_double(), C.c_double(), C.c_double(), C.c_double()
    for CI in CIS:
        for q in ((1 - CI) / 2, (1 + CI) / 2):
            for a, b, x in zip(c1, c0, sps.beta(c1, c0).ppf(q)):
                xc = 1.0 - x
                lib.hq_ibeta(a, b, x, xc, C.byref(P), C.byref(Q))
                lib.hq_ibeta(b, a, xc, x, C.byref(P2), C.byref(Q2))
                assert abs(P.value + P2.value - 1.0) <= 1e-13, (a, b, x)
                assert abs(P.value + Q.value - 1.0) <= 1e-13 and abs(Q.value - P2.value) <= 1e-13, (a, b, x)


CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[2])
from quantile_host import host_intervals, open_lib
BAD = (float('nan'), float('inf'), float('-inf'), 0.0, -1.0)
lib = open_lib(sys.argv[1])
good = 2.0
for kind, low, high in ((0, 0.0, 0.0), (1, -7.5, 7.5)):
    p0 = np.array([b for b in BAD] + [good] * len(BAD) + [b for b in BAD], dtype=np.float32)
    p1 = np.array([good] * len(BAD) + [b for b in BAD] + [b for b in BAD], dtype=np.float32)
    if kind == 1:  # 0 and -1 are inside (low, high): the out-of-domain means are the bounds themselves and beyond
        p0 = np.where(p0 == 0.0, np.float32(high), np.where(p0 == -1.0, np.float32(low - 1.0), p0))
    ll, ul = host_intervals(lib, kind, p0, p1, low, high, 0.95)
    assert np.isnan(ll).all() and np.isnan(ul).all(), (kind, p0, p1, ll, ul)
print("ok")
"""


def test_out_of_domain_parameters_give_nan_and_return(so_path):
    """NaN, +-inf, 0 and negative parameters (each alone and both together) give NaN for LL and UL, and the loops end
    on their caps: the child process is killed after a few seconds."""
    out = subprocess.run([sys.executable, "-c", CHILD, so_path, HERE], capture_output=True, text=True, timeout=20)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stderr


def test_extreme_finite_parameters_return(so_path):
    """Finite parameters far outside the model's range come back (finite or NaN) without spinning."""
    code = CHILD.split("good = 2.0")[0] + r"""
big = np.array([1e-30, 1e-8, 1e8, 1e19, 3e38], dtype=np.float32)
p0, p1 = (v.ravel() for v in np.meshgrid(big, big))
host_intervals(lib, 0, p0, p1, 0.0, 0.0, 0.95)
host_intervals(lib, 1, np.full(5, 1.0, dtype=np.float32), big, 0.0, 2.0, 0.999)
host_intervals(lib, 1, np.float32([1e-30, 1e-8, 1.0, 2.0 - 1e-6, 1.9999999]), np.full(5, 3.0, dtype=np.float32), 0.0, 2.0, 0.5)
print("ok")
"""
    out = subprocess.run([sys.executable, "-c", code, so_path, HERE], capture_output=True, text=True, timeout=30)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stderr


def test_argument_validation_returns_error_codes_without_a_gpu():
    """Every refusal of ``tq_credible_intervals`` comes before the launch, so it can be checked on host addresses."""
    from tapqir_amd import _lib

    lib = _lib.load()
    buf = np.ones(4, dtype=np.float64)

    def args(**kw):
        a = _lib.IntervalArgs()
        a.kind, a.p0, a.p1, a.ll, a.ul = _lib.INTERVAL_AFFINE_BETA, *(buf.ctypes.data,) * 4
        a.n, a.ci, a.low, a.high = 1, 0.95, 0.0, 1.0
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    for a in (args(p0=None), args(p1=None), args(ll=None), args(ul=None), args(n=0), args(n=-3), args(ci=1.0), args(ci=0.0),
              args(ci=float("nan")), args(kind=2), args(high=0.0), args(low=float("-inf"))):
        assert lib.tq_credible_intervals(C.byref(a), None) == 1  # TQ_ERR_ARG
        assert len(lib.tq_last_error()) > 0
    assert lib.tq_credible_intervals(None, None) == 1
    assert C.sizeof(_lib.IntervalArgs) == 72 and _lib.IntervalArgs.high.offset == 64
