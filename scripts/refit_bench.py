"""Bootstrap-refit benchmark at the ``smooth`` command's scale: 400 on-target AOIs x 1000 frames of the three-state reference
chain, (U, B) = (1, 1), (1, 2) and (2, 2), 64 fits (the data as they are and 63 resamples of the AOIs: one batch) of
`--em-iters` EM iterations from the default start.  Reports on the device (events, median of `--reps` after a warm-up with
the spread max - min of each, all launches taking turns in one process) per configuration:

  a  ``hmm_fit_refits``: the weights, 2 launches an iteration for all replicas, the closing batched E-step;
  b  the same 64 fits without the weighted kernels: ``hmm_fit`` once per replica on the rows of ``p`` gathered as the
     resample draws them (an AOI of weight w is w rows);
  c  one ``tq_refit_estep`` next to one ``tq_multistart_estep`` at R = 64 on the same theta: what leaving out the
     workgroups of weight 0 (about 37 % of them) buys on this grid, and one ``tq_refit_mstep`` next to one
     ``tq_multistart_mstep``.

``a_over_b`` and ``refit_over_multistart_estep`` are the ratios of the medians.  One JSON line.

    python scripts/refit_bench.py [--reps 20]
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
from multistart_bench import timed  # noqa: E402
from tapqir_amd.utils.mle_analysis import (hmm_default_start, hmm_fit, hmm_fit_refits, multistart_estep,  # noqa: E402
                                           multistart_mstep, refit_estep, refit_mstep, refit_weights)

CONFIGS = [(1, 1), (1, 2), (2, 2)]
FITS = 64


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--aois", type=int, default=400)
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--em-iters", type=int, default=50)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "refit_bench measures the MI355X"
    prior, iters = 1.0 / 3.0, args.em_iters
    p = torch.from_numpy(synthetic_hmm(args.aois, args.frames, seed=0)[0]).to("cuda")
    N, F = p.shape
    weights = torch.cat([torch.ones(1, N, dtype=torch.int32, device="cuda"),
                         refit_weights(N, FITS - 1, args.seed, 0, "cuda")]).contiguous()
    gathered = [p[torch.repeat_interleave(torch.arange(N, device="cuda"), weights[r].long())].contiguous() for r in range(FITS)]
    runs = {}
    for U, B in CONFIGS:
        M = U + B
        tag = f"u{U}b{B}"
        A0, rho0 = hmm_default_start(U, B)
        start = torch.cat([A0.reshape(-1), rho0])
        thetas = start.reshape(1, -1).repeat(FITS, 1).to("cuda")
        rows = torch.zeros(FITS, N, M * M + M + 1, dtype=torch.float64, device="cuda")
        scratch = torch.empty(FITS, N, F, M, dtype=torch.float64, device="cuda")
        trace = torch.zeros(FITS, 1, dtype=torch.float64, device="cuda")
        multistart_estep(p, thetas, prior, U, B, None, rows, scratch)

        def serial(U=U, B=B, A0=A0, rho0=rho0):
            return [hmm_fit(g, prior, U, B, A0=A0, rho0=rho0, num_iter=iters, tol=0.0, chunk=iters) for g in gathered]

        runs.update({
            f"{tag}_a_batched": lambda U=U, B=B, start=start: hmm_fit_refits(p, prior, start, U, B, FITS - 1, seed=args.seed,
                                                                             num_iter=iters, tol=-1.0, chunk=iters),
            f"{tag}_b_serial": serial,
            f"{tag}_refit_estep": lambda U=U, B=B, th=thetas, rows=rows, scratch=scratch: refit_estep(p, th, weights, prior, U, B,
                                                                                                  None, rows, scratch),
            f"{tag}_multistart_estep": lambda U=U, B=B, th=thetas, rows=rows, scratch=scratch: multistart_estep(p, th, prior, U, B,
                                                                                                            None, rows, scratch),
            f"{tag}_refit_mstep": lambda U=U, B=B, th=thetas.clone(), rows=rows, trace=trace: refit_mstep(rows, th, weights, trace,
                                                                                                      0, U, B),
            f"{tag}_multistart_mstep": lambda U=U, B=B, th=thetas.clone(), rows=rows, trace=trace: multistart_mstep(rows, th, trace,
                                                                                                                0, U, B),
        })
    times, out = timed(runs, args.reps)
    ms = {k: statistics.median(v) for k, v in times.items()}
    spread = {k: max(v) - min(v) for k, v in times.items()}
    log(" ".join(f"{k} {ms[k]:.4f} ms (spread {spread[k]:.4f})" for k in ms))
    result = {"bench": "refit", "N": N, "F": F, "fits": FITS, "reps": args.reps, "em_iters": iters,
              "zero_weight_share": round(float((weights == 0).double().mean()), 4)}
    result.update({f"{k}_ms": round(v, 4) for k, v in ms.items()})
    result.update({f"{k}_spread_ms": round(v, 4) for k, v in spread.items()})
    for U, B in CONFIGS:
        tag = f"u{U}b{B}"
        batched, fits = out[f"{tag}_a_batched"], out[f"{tag}_b_serial"]
        # the same fits: every replica's weighted log evidence against hmm_fit's on the gathered rows
        diff = max(abs(batched["logliks"][r].item() - fits[r]["loglik"]) / abs(fits[r]["loglik"]) for r in range(FITS))
        assert diff < 1e-6, (tag, diff)
        result[f"{tag}_max_rel_loglik_difference"] = diff
        result[f"{tag}_a_over_b"] = round(ms[f"{tag}_a_batched"] / ms[f"{tag}_b_serial"], 4)
        result[f"{tag}_refit_over_multistart_estep"] = round(ms[f"{tag}_refit_estep"] / ms[f"{tag}_multistart_estep"], 4)
        result[f"{tag}_refit_over_multistart_mstep"] = round(ms[f"{tag}_refit_mstep"] / ms[f"{tag}_multistart_mstep"], 4)
        gap = ms[f"{tag}_multistart_estep"] - ms[f"{tag}_refit_estep"]
        result[f"{tag}_skipping_faster"] = bool(gap > spread[f"{tag}_multistart_estep"] + spread[f"{tag}_refit_estep"])
    print(json.dumps(result))


if __name__ == "__main__":
    main()
