"""Benchmark of ``tq_chain_dwell`` at the ``dwelltime`` command's defaults: S = 500 posterior rasters, 400 on-target AOIs x
1000 frames of the three-state reference chain of the test fixture, theta after 50 EM iterations from the default start.
Reports on the device (events, median of `--reps` after a warm-up, the launches taking turns in one process, every launch
on buffers allocated before the clock starts): the COUNT and the EMIT launch of ``tq_chain_dwell`` at (U, B) = (1, 1),
(1, 2) and (2, 2), and beside them the yardsticks on the same data: both launches of the unchanged ``tq_smooth_dwell`` (the
two-state chain after 50 EM iterations of its own) and ``tq_hmm_count`` without its optional outputs at the same three
chains.  One JSON line.

    python scripts/hmm_dwell_bench.py [--reps 20]
"""

import argparse
import ctypes as C
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "scripts"), os.path.join(ROOT, "tests")]

from dwelltime_bench import log  # noqa: E402
from hmm_fixture import synthetic_hmm  # noqa: E402
from rates_bench import median_ms  # noqa: E402
from smooth_dwell_bench import Launches, smooth_launches, stream  # noqa: E402
from tapqir_amd import _lib, _lib_hmm, _lib_rates  # noqa: E402
from tapqir_amd.utils.mle_analysis import hmm_fit, smooth_fit  # noqa: E402

CHAINS = ((1, 1), (1, 2), (2, 2))


def chain_launches(filt, theta, U, B, S, seed):
    N, F = filt.shape[:2]

    def make_args(b, mode):
        return _lib_hmm.ChainDwellArgs(filt=_lib.ptr(filt), theta=_lib.ptr(theta), counts=_lib.ptr(b.counts),
                                       hist_bound=_lib.ptr(b.hb), hist_unbound=_lib.ptr(b.hu), tau=_lib.ptr(b.tau),
                                       offsets=_lib.ptr(b.offsets), intervals=_lib.ptr(b.cols), total=b.total, N=N, F=F,
                                       S=S, U=U, B=B, mode=mode, seed=seed)

    return Launches(S, N, F, make_args, _lib_hmm.lib().tq_chain_dwell, "tq_chain_dwell")


def count_launch(filt, theta, U, B, S, seed):
    """``tq_hmm_count`` with its class-level counts alone, on a buffer of its own."""
    N, F = filt.shape[:2]
    counts = torch.empty(S, N, _lib_rates.RATES_COLS, dtype=torch.int32, device="cuda")
    a = _lib_hmm.HmmCountArgs(filt=_lib.ptr(filt), theta=_lib.ptr(theta), counts=_lib.ptr(counts), N=N, F=F, S=S, U=U, B=B,
                              seed=seed)
    entry = _lib_hmm.lib().tq_hmm_count

    def launch():
        _lib.check(entry(C.byref(a), stream()), "tq_hmm_count")

    launch.keep = (counts, filt, theta)
    return launch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=500)
    ap.add_argument("--aois", type=int, default=400)
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "hmm_dwell_bench measures the MI355X"
    prior, S = 1.0 / 3.0, args.samples
    p = torch.from_numpy(synthetic_hmm(args.aois, args.frames, seed=0)[0]).to("cuda")
    two = smooth_fit(p, prior, num_iter=50, tol=0.0)
    runs = {"smooth": smooth_launches(two["filt"], two["theta"].clone(), S, 0)}
    fns = {}
    for U, B in CHAINS:
        fit = hmm_fit(p, prior, U, B, num_iter=50, tol=0.0)
        filt, theta = fit["filt"].contiguous(), fit["theta"].clone()
        runs[f"chain_u{U}b{B}"] = chain_launches(filt, theta, U, B, S, 0)
        fns[f"hmm_count_u{U}b{B}"] = count_launch(filt, theta, U, B, S, 0)
    for r in runs.values():
        r.count()
        r.scan()
    fns.update({f"{name}_{mode}": getattr(r, mode) for name, r in runs.items() for mode in ("count", "emit")})
    ms, _ = median_ms(fns, args.reps)
    log(" ".join(f"{k} {v:.4f} ms" for k, v in ms.items()))
    out = {"bench": "hmm_dwell", "S": S, "N": args.aois, "F": args.frames, "reps": args.reps}
    for name, r in runs.items():
        out[f"{name}_intervals"] = r.total
    out.update({f"{k}_ms": round(v, 4) for k, v in ms.items()})
    for mode in ("count", "emit"):
        out[f"chain_u1b1_over_smooth_{mode}"] = round(ms[f"chain_u1b1_{mode}"] / ms[f"smooth_{mode}"], 4)
    for U, B in CHAINS:
        out[f"chain_over_hmm_count_u{U}b{B}"] = round(ms[f"chain_u{U}b{B}_count"] / ms[f"hmm_count_u{U}b{B}"], 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
