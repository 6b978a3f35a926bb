"""Side-by-side EM benchmark at the ``smooth`` command's scale: 400 on-target AOIs x 1000 frames of the three-state
reference chain, (U, B) = (1, 2) and (2, 2), R = 1, 8 and 32 replicas (the default start and R - 1 random ones).  Reports on
the device (events, median of `--reps` after a warm-up with the spread max - min of each, all launches taking turns in one
process) per configuration: one batched E-step, one batched M-step, ``hmm_fit_restarts`` of `--em-iters` iterations with
tol = 0 (2 launches an iteration for all replicas, then the closing batched E-step, the winner's E-step and relabelling),
and the baseline: R calls of ``hmm_fit`` from the same starts, one after the other.  ``batched_faster`` says whether the
batched run at R = 8 is faster than the 8 serial fits by more than the two spreads together.  One JSON line.

    python scripts/multistart_bench.py [--reps 20]
"""

import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "scripts"), os.path.join(ROOT, "tests")]

from dwelltime_bench import log  # noqa: E402
from hmm_fixture import synthetic_hmm  # noqa: E402
from tapqir_amd.utils.mle_analysis import (hmm_fit, hmm_fit_restarts, hmm_random_starts, multistart_estep,  # noqa: E402
                                           multistart_mstep)

CONFIGS = [(1, 2), (2, 2)]
REPLICAS = [1, 8, 32]


def timed(fns, reps):
    """Event-timed calls of each function of ``fns`` (name -> callable), ``reps`` times after one warm-up call, the
    functions taking turns within a repetition; returns ({name: [ms]}, {name: last result})."""
    out = {name: fn() for name, fn in fns.items()}
    torch.cuda.synchronize()
    times = {name: [] for name in fns}
    for _ in range(reps):
        for name, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out[name] = fn()
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1))
    return times, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--aois", type=int, default=400)
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--em-iters", type=int, default=50)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "multistart_bench measures the MI355X"
    prior, iters = 1.0 / 3.0, args.em_iters
    p = torch.from_numpy(synthetic_hmm(args.aois, args.frames, seed=0)[0]).to("cuda")
    N, F = p.shape
    runs = {}
    for U, B in CONFIGS:
        M = U + B
        for R in REPLICAS:
            tag = f"u{U}b{B}_r{R}"
            starts = hmm_random_starts(U, B, R - 1, seed=0)
            thetas = starts.to("cuda")
            rows = torch.empty(R, N, M * M + M + 1, dtype=torch.float64, device="cuda")
            scratch = torch.empty(R, N, F, M, dtype=torch.float64, device="cuda")
            trace = torch.zeros(R, 1, dtype=torch.float64, device="cuda")
            multistart_estep(p, thetas, prior, U, B, None, rows, scratch)

            def serial(U=U, B=B, M=M, starts=starts):
                return [hmm_fit(p, prior, U, B, A0=s[: M * M].reshape(M, M), rho0=s[M * M:], num_iter=iters, tol=0.0, chunk=iters)
                        for s in starts]

            runs.update({
                f"{tag}_estep": lambda U=U, B=B, th=thetas, rows=rows, scratch=scratch: multistart_estep(p, th, prior, U, B, None, rows, scratch),
                f"{tag}_mstep": lambda U=U, B=B, th=thetas.clone(), rows=rows, trace=trace: multistart_mstep(rows, th, trace, 0, U, B),
                f"{tag}_em_batched": lambda U=U, B=B, starts=starts: hmm_fit_restarts(p, prior, U, B, starts=starts, num_iter=iters,
                                                                                     tol=0.0, chunk=iters),
                f"{tag}_em_serial": serial,
            })
    times, out = timed(runs, args.reps)
    ms = {k: statistics.median(v) for k, v in times.items()}
    spread = {k: max(v) - min(v) for k, v in times.items()}
    log(" ".join(f"{k} {ms[k]:.4f} ms (spread {spread[k]:.4f})" for k in ms))
    result = {"bench": "multistart", "N": N, "F": F, "reps": args.reps, "em_iters": iters}
    result.update({f"{k}_ms": round(v, 4) for k, v in ms.items()})
    result.update({f"{k}_spread_ms": round(v, 4) for k, v in spread.items()})
    for U, B in CONFIGS:
        for R in REPLICAS:
            tag = f"u{U}b{B}_r{R}"
            batched, fits = out[f"{tag}_em_batched"], out[f"{tag}_em_serial"]
            # the same fits: every replica's final log evidence against hmm_fit's from the same start
            diff = max(abs(batched["logliks"][r].item() - fits[r]["loglik"]) / abs(fits[r]["loglik"]) for r in range(R))
            assert diff < 1e-6, (tag, diff)
            result[f"{tag}_max_rel_loglik_difference"] = diff
            result[f"{tag}_serial_over_batched"] = round(ms[f"{tag}_em_serial"] / ms[f"{tag}_em_batched"], 3)
            result[f"{tag}_best"] = batched["best"]
            result[f"{tag}_loglik_best_minus_default"] = round(batched["logliks"][batched["best"]].item() - batched["logliks"][0].item(), 4)
        tag = f"u{U}b{B}_r8"
        gap = ms[f"{tag}_em_serial"] - ms[f"{tag}_em_batched"]
        result[f"u{U}b{B}_batched_faster"] = bool(gap > spread[f"{tag}_em_serial"] + spread[f"{tag}_em_batched"])
    print(json.dumps(result))


if __name__ == "__main__":
    main()
