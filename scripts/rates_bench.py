"""Two-state rate benchmark at the ``rates`` command's defaults: S = 1000 posterior samples, 400 on-target AOIs x 1000
frames, bootstrap over AOIs.  Reports on the device (events, median of `--reps` after a warm-up): the count launch
(``rates_sample``), the estimate launch (``rates_estimate``), and in the same process, interleaved with them, launch A of the
dwell-time sampler (``dwell_sample``) at the same S, N, F -- it draws the same numbers and does more per frame, so it is
the count launch's yardstick.  The host restatement is the reference's loop: one ``Bernoulli(p).sample()`` and one
``association_rate`` per repetition (`--cpu-threads` threads, `--cpu-reps` repetitions, extrapolated to S).  One JSON line.

    python scripts/rates_bench.py [--cpu-reps 20] [--cpu-threads 16]
"""

import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "scripts")]

from dwelltime_bench import log, posterior_like  # noqa: E402
from tapqir_amd.utils.imscroll import association_rate  # noqa: E402
from tapqir_amd.utils.mle_analysis import dwell_sample, rates_estimate, rates_sample, rates_summary  # noqa: E402


def median_ms(fns, reps):
    """Event-timed median of ``reps`` calls of each function of ``fns`` (name -> callable), the functions taking turns
    within a repetition so that clock drift touches all alike; returns ({name: ms}, {name: last result})."""
    out = {name: fn() for name, fn in fns.items()}  # warm-up: code objects, allocator
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
    return {name: statistics.median(t) for name, t in times.items()}, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=1000)
    ap.add_argument("--aois", type=int, default=400)
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--cpu-reps", type=int, default=20)
    ap.add_argument("--cpu-threads", type=int, default=16)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "rates_bench measures the MI355X"
    gen = torch.Generator().manual_seed(0)
    p_host = posterior_like(args.aois, args.frames, gen)
    p = p_host.to("cuda")
    S = args.samples
    counts = rates_sample(p, S, seed=0)
    ms, out = median_ms({"count": lambda: rates_sample(p, S, seed=0),
                         "dwell_count": lambda: dwell_sample(p, S, seed=0),
                         "estimate_bootstrap": lambda: rates_estimate(counts, bootstrap=True, seed=0),
                         "estimate_pooled": lambda: rates_estimate(counts)}, args.reps)
    log(" ".join(f"{k} {v:.4f} ms" for k, v in ms.items()))
    assert torch.equal(out["count"], counts)
    summary = rates_summary(out["estimate_bootstrap"], 0.95)

    torch.set_num_threads(args.cpu_threads)
    dist = torch.distributions.Bernoulli(p_host)
    association_rate(dist.sample())  # warm-up
    t0 = time.perf_counter()
    for _ in range(args.cpu_reps):
        association_rate(dist.sample())
    cpu_ms_rep = (time.perf_counter() - t0) * 1e3 / args.cpu_reps
    gpu_ms = ms["count"] + ms["estimate_bootstrap"]
    print(json.dumps({
        "bench": "rates", "S": S, "N": args.aois, "F": args.frames, "reps": args.reps,
        "count_ms": round(ms["count"], 4), "dwell_count_ms": round(ms["dwell_count"], 4),
        "count_over_dwell_count": round(ms["count"] / ms["dwell_count"], 4),
        "estimate_bootstrap_ms": round(ms["estimate_bootstrap"], 4), "estimate_pooled_ms": round(ms["estimate_pooled"], 4),
        "total_gpu_ms": round(gpu_ms, 4), "cpu_threads": args.cpu_threads, "cpu_reps": args.cpu_reps,
        "cpu_sample_and_rate_ms_per_rep": round(cpu_ms_rep, 3),
        "cpu_one_rate_s_extrapolated": round(cpu_ms_rep * S / 1e3, 2),
        "speedup_one_rate": round(cpu_ms_rep * S / gpu_ms, 1),
        "kon": summary["kon"], "koff": summary["koff"],
    }))


if __name__ == "__main__":
    main()
