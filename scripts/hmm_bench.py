"""Multi-state hidden-Markov smoothing benchmark at the ``smooth`` command's scale: 400 on-target AOIs x 1000 frames,
S = 1000 posterior rasters, for (U, B) = (1, 1), (1, 2) and (2, 2) hidden states.  Reports on the device (events, median
of `--reps` after a warm-up, the launches taking turns) per configuration: one E-step, one M-step, an EM run of
`--em-iters` iterations (2 launches each, no host synchronisation inside), the Viterbi launch and the count launch of the
backward sampler with its state-pair counts; beside them, in the same process, the two-state ``tq_smooth_estep`` and
``tq_smooth_count`` on the same input: the yardsticks, and the (1, 1) general kernel over the specialised one.  One JSON
line.

    python scripts/hmm_bench.py [--reps 20]
"""

import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "scripts"), os.path.join(ROOT, "tests")]

from dwelltime_bench import log  # noqa: E402
from hmm_fixture import synthetic_hmm  # noqa: E402
from rates_bench import median_ms  # noqa: E402
from tapqir_amd.utils.mle_analysis import (hmm_estep, hmm_fit, hmm_mstep, hmm_sample, hmm_viterbi, smooth_estep,  # noqa: E402
                                           smooth_fit, smooth_sample)

CONFIGS = [(1, 1), (1, 2), (2, 2)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=1000)
    ap.add_argument("--aois", type=int, default=400)
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--em-iters", type=int, default=50)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "hmm_bench measures the MI355X"
    prior, S = 1.0 / 3.0, args.samples
    p = torch.from_numpy(synthetic_hmm(args.aois, args.frames, seed=0)[0]).to("cuda")
    two = smooth_fit(p, prior, num_iter=args.em_iters, tol=0.0, chunk=args.em_iters)
    trace = torch.zeros(1, dtype=torch.float64, device="cuda")
    runs, fits = {
        "smooth_estep": lambda: smooth_estep(p, two["theta"], prior),
        "smooth_count": lambda: smooth_sample(two["filt"], two["theta"], S, seed=0),
    }, {}
    for U, B in CONFIGS:
        fit = fits[U, B] = hmm_fit(p, prior, U, B, num_iter=args.em_iters, tol=0.0, chunk=args.em_iters)
        tag, theta, scratch_theta = f"u{U}b{B}", fit["theta"], fit["theta"].clone()
        runs.update({
            f"{tag}_estep": lambda U=U, B=B, theta=theta: hmm_estep(p, theta, prior, U, B),
            f"{tag}_mstep": lambda U=U, B=B, fit=fit, th=scratch_theta: hmm_mstep(fit["rows"], th, trace, 0, U, B),
            f"{tag}_em": lambda U=U, B=B: hmm_fit(p, prior, U, B, num_iter=args.em_iters, tol=0.0, chunk=args.em_iters),
            f"{tag}_viterbi": lambda U=U, B=B, theta=theta: hmm_viterbi(p, theta, prior, U, B),
            f"{tag}_count": lambda U=U, B=B, fit=fit, theta=theta: hmm_sample(fit["filt"], theta, U, B, S, seed=0, trans=True),
        })
    ms, out = median_ms(runs, args.reps)
    log(" ".join(f"{k} {v:.4f} ms" for k, v in ms.items()))
    # "em" holds, besides its 2 * em_iters launches, one read of the trace, the closing E-step and the relabelling
    # the fit's outputs are relabelled after its closing E-step, so an E-step at the relabelled theta adds in another order
    diff = max((out[f"u{U}b{B}_estep"]["gamma"] - fits[U, B]["gamma"]).abs().max().item() for U, B in CONFIGS)
    assert diff < 1e-12, diff
    result = {"bench": "hmm", "S": S, "N": args.aois, "F": args.frames, "reps": args.reps, "em_iters": args.em_iters}
    result.update({f"{k}_ms": round(v, 4) for k, v in ms.items()})
    result.update({"estep_u1b1_over_smooth": round(ms["u1b1_estep"] / ms["smooth_estep"], 4),
                   "count_u1b1_over_smooth": round(ms["u1b1_count"] / ms["smooth_count"], 4),
                   "max_gamma_difference_to_fit": diff,
                   "bic": {f"u{U}b{B}": fits[U, B]["bic"] for U, B in CONFIGS}})
    print(json.dumps(result))


if __name__ == "__main__":
    main()
