"""Benchmark of `dwelltime --censored` at the command's defaults: S = 500 posterior samples, 400 on-target AOIs x 1000
frames of a slow complex (kon 0.01, koff 0.002 per frame), K = 3.  Reports on the device (events, median of `--reps` after
a warm-up and the spread max - min, the launches taking turns within a repetition, all in one process):

* one 1000-step launch of ``tq_dwell_censored_fit`` on the bound histograms, next to one of ``tq_dwell_fit`` on the same
  complete pairs, with both pair counts and the ratio of the two times;
* ``tq_dwell_censored_hist`` on the interval table of that sampler;
* ``tq_dwell_survival`` on its histograms.

One JSON line.

    python scripts/censored_bench.py [--reps 20]
"""

import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "scripts")]

from dwelltime_bench import posterior_like  # noqa: E402
from tapqir_amd.utils.censored_analysis import (dwell_censored_fit_steps, dwell_censored_hist,  # noqa: E402
                                                dwell_csr_from_censored_hist, dwell_survival)
from tapqir_amd.utils.mle_analysis import (dwell_csr_from_hist, dwell_fit_steps, dwell_init_state, dwell_intervals,  # noqa: E402
                                           dwell_sample)


def log(msg):
    print(msg, file=sys.stderr, flush=True)


def timed(fns, reps):
    """Event-timed calls of each function of ``fns`` (name -> callable), taking turns within a repetition so that clock
    drift touches all alike: ({name: median ms}, {name: max - min ms}) of ``reps`` calls after one warm-up call each."""
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    times = {name: [] for name in fns}
    for _ in range(reps):
        for name, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1))
    return ({name: statistics.median(t) for name, t in times.items()},
            {name: max(t) - min(t) for name, t in times.items()})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=500)
    ap.add_argument("--aois", type=int, default=400)
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("-K", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "censored_bench measures the MI355X"
    S, N, F, K = args.samples, args.aois, args.frames, args.K
    p = posterior_like(N, F, torch.Generator().manual_seed(0), kon=0.01, koff=0.002).to("cuda")
    sample = dwell_sample(p, S, seed=0)
    _, table = dwell_intervals(p, S, seed=0, sample=sample, device_table=True)
    cens = dwell_censored_hist(table, S, N, F)
    hist, open_runs = sample["hist_bound"], cens["cens_bound"]
    csr, ccsr = dwell_csr_from_hist(hist), dwell_csr_from_censored_hist(open_runs)
    pairs = (csr[2][1:] - csr[2][:-1]).double()
    cpairs = (ccsr[2][1:] - ccsr[2][:-1]).double()
    log(f"{table.shape[1]} intervals; complete pairs per row {pairs.mean().item():.1f} (max {int(pairs.max())}), censored "
        f"{cpairs.mean().item():.1f} (max {int(cpairs.max())})")
    loss = torch.empty(S, dtype=torch.float32, device="cuda")

    def censored_fit():
        dwell_censored_fit_steps(dwell_init_state(S, K, "cuda"), csr, ccsr, K, n_steps=args.steps, loss=loss)

    def plain_fit():
        dwell_fit_steps(dwell_init_state(S, K, "cuda"), csr, K, n_steps=args.steps, loss=loss)

    fns = {"censored_fit": censored_fit, "dwell_fit": plain_fit,
           "censored_hist": lambda: dwell_censored_hist(table, S, N, F), "survival": lambda: dwell_survival(hist, open_runs)}
    ms, spread = timed(fns, args.reps)
    log(" ".join(f"{k} {v:.4f} (+- {spread[k]:.4f}) ms" for k, v in ms.items()))
    out = {"bench": "censored", "S": S, "N": N, "F": F, "K": K, "steps": args.steps, "reps": args.reps,
           "intervals": int(table.shape[1]), "complete_pairs_mean_max": [round(pairs.mean().item(), 1), int(pairs.max())],
           "censored_pairs_mean_max": [round(cpairs.mean().item(), 1), int(cpairs.max())],
           "complete_open_runs_per_sample": [round(hist.sum(1).double().mean().item(), 1),
                                             round(open_runs[:, 2:].sum(1).double().mean().item(), 1)]}
    out.update({f"{k}_ms": round(v, 4) for k, v in ms.items()})
    out.update({f"{k}_spread_ms": round(v, 4) for k, v in spread.items()})
    out["censored_over_dwell_fit"] = round(ms["censored_fit"] / ms["dwell_fit"], 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
