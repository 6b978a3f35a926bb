"""Hidden-Markov smoothing benchmark at the ``smooth`` command's scale: 400 on-target AOIs x 1000 frames, S = 1000
posterior rasters.  Reports on the device (events, median of `--reps` after a warm-up, the launches taking turns): one
E-step, one M-step, an EM run of `--em-iters` iterations (2 launches each, no host synchronisation inside), the Viterbi
launch and the count launch of the backward sampler; beside them, in the same process, ``tq_rates_count`` at the same
S, N, F (it draws as many numbers and compares against p instead of a threshold picked by the next label: the count
launch's yardstick) and the numpy forward-backward of the test fixture on the host (`--cpu-reps` repetitions).  One JSON
line.

    python scripts/smooth_bench.py [--reps 20] [--cpu-reps 3]
"""

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "scripts"), os.path.join(ROOT, "tests")]

from dwelltime_bench import log  # noqa: E402
from rates_bench import median_ms  # noqa: E402
from smooth_fixture import oracle_estep, synthetic_chain  # noqa: E402
from tapqir_amd.utils.mle_analysis import (rates_sample, smooth_estep, smooth_fit, smooth_mstep, smooth_sample,  # noqa: E402
                                           smooth_viterbi)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=1000)
    ap.add_argument("--aois", type=int, default=400)
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--em-iters", type=int, default=50)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--cpu-reps", type=int, default=3)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "smooth_bench measures the MI355X"
    prior, S = 1.0 / 3.0, args.samples
    p_host, _ = synthetic_chain(args.aois, args.frames, seed=0)
    p = torch.from_numpy(p_host).to("cuda")
    fit = smooth_fit(p, prior)
    theta = fit["theta"].clone()
    scratch_theta = theta.clone()
    trace = torch.zeros(1, dtype=torch.float64, device="cuda")
    ms, out = median_ms({
        "estep": lambda: smooth_estep(p, theta, prior),
        "mstep": lambda: smooth_mstep(fit["rows"], scratch_theta, trace, 0),
        "em": lambda: smooth_fit(p, prior, num_iter=args.em_iters, tol=0.0, chunk=args.em_iters),
        "viterbi": lambda: smooth_viterbi(p, theta, prior),
        "count": lambda: smooth_sample(fit["filt"], theta, S, seed=0),
        "rates_count": lambda: rates_sample(p, S, seed=0),
    }, args.reps)
    log(" ".join(f"{k} {v:.4f} ms" for k, v in ms.items()))
    # "em" holds, besides its 2 * em_iters launches, one read of the trace and the closing E-step
    assert torch.equal(out["estep"]["gamma"], fit["gamma"])

    oracle_estep(p_host, theta.tolist(), prior)  # warm-up
    t0 = time.perf_counter()
    for _ in range(args.cpu_reps):
        host = oracle_estep(p_host, theta.tolist(), prior)
    cpu_ms = (time.perf_counter() - t0) * 1e3 / args.cpu_reps
    err = float(np.abs(out["estep"]["gamma"].cpu().numpy() - host["gamma"]).max())
    print(json.dumps({
        "bench": "smooth", "S": S, "N": args.aois, "F": args.frames, "reps": args.reps, "em_iters": args.em_iters,
        "estep_ms": round(ms["estep"], 4), "mstep_ms": round(ms["mstep"], 4), "em_ms": round(ms["em"], 4),
        "em_ms_per_iteration": round(ms["em"] / args.em_iters, 4), "viterbi_ms": round(ms["viterbi"], 4),
        "count_ms": round(ms["count"], 4), "rates_count_ms": round(ms["rates_count"], 4),
        "count_over_rates_count": round(ms["count"] / ms["rates_count"], 4),
        "cpu_reps": args.cpu_reps, "numpy_estep_ms": round(cpu_ms, 2), "numpy_over_device_estep": round(cpu_ms / ms["estep"], 1),
        "max_gamma_difference": err, "fit_iterations": fit["iterations"], "fit_converged": fit["converged"],
        "kon": theta[0].item(), "koff": theta[1].item(), "pi0": theta[2].item(),
    }))


if __name__ == "__main__":
    main()
