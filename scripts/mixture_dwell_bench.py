"""Benchmark of ``tq_population_dwell`` at the ``dwelltime`` command's defaults: S = 500 posterior rasters, 400 on-target AOIs
x 1000 frames of the three-state reference chain of the test fixture, the mixture after 50 EM iterations from the default
start.  Reports on the device (events, median of `--reps` after a warm-up and the spread max - min, the launches taking
turns in one process, every launch on buffers allocated before the clock starts): the COUNT and the EMIT launch of
``tq_population_dwell`` at (U, B) = (1, 1), (1, 2), (2, 2) and G = 1, 2, 4, and beside them its two parents on the same
data: both launches of ``tq_chain_dwell`` on population 0's chain and filt, and ``tq_mixture_count`` without its optional
outputs on the same mixture.  No time is fixed in advance: the ratios to the parents are the result.  One JSON line.

    python scripts/mixture_dwell_bench.py [--reps 20]
"""

import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "scripts"), os.path.join(ROOT, "tests")]

from dwelltime_bench import log  # noqa: E402
from hmm_dwell_bench import CHAINS, chain_launches  # noqa: E402
from hmm_fixture import synthetic_hmm  # noqa: E402
from smooth_dwell_bench import Launches, stream  # noqa: E402
from tapqir_amd import _lib, _lib_mixture, _lib_rates  # noqa: E402
from tapqir_amd.utils.mle_analysis import mixture_fit  # noqa: E402

POPULATIONS = (1, 2, 4)


class PopulationLaunches(Launches):
    """``Launches`` with histograms of (S, G, F) and the populations the COUNT launch writes."""

    def __init__(self, S, N, F, G, make_args, entry, name):
        super().__init__(S, N, F, make_args, entry, name)
        self.hb = torch.zeros(S, G, F, dtype=torch.int32, device="cuda")
        self.hu = torch.zeros(S, G, F, dtype=torch.int32, device="cuda")
        self.pop = torch.empty(S, N, dtype=torch.uint8, device="cuda")


def population_launches(filt, thetas, resp, U, B, S, seed):
    G, N, F = filt.shape[:3]

    def make_args(b, mode):
        return _lib_mixture.PopulationDwellArgs(filt=_lib.ptr(filt), theta=_lib.ptr(thetas), resp=_lib.ptr(resp),
                                                counts=_lib.ptr(b.counts), pop=_lib.ptr(b.pop), hist_bound=_lib.ptr(b.hb),
                                                hist_unbound=_lib.ptr(b.hu), tau=_lib.ptr(b.tau), offsets=_lib.ptr(b.offsets),
                                                intervals=_lib.ptr(b.cols), total=b.total, N=N, F=F, S=S, G=G, U=U, B=B,
                                                mode=mode, seed=seed)

    return PopulationLaunches(S, N, F, G, make_args, _lib_mixture.lib().tq_population_dwell, "tq_population_dwell")


def mixture_count_launch(filt, thetas, resp, U, B, S, seed):
    """``tq_mixture_count`` with its class-level counts and populations alone, on buffers of its own."""
    G, N, F = filt.shape[:3]
    counts = torch.empty(S, N, _lib_rates.RATES_COLS, dtype=torch.int32, device="cuda")
    pop = torch.empty(S, N, dtype=torch.uint8, device="cuda")
    a = _lib_mixture.MixtureCountArgs(filt=_lib.ptr(filt), theta=_lib.ptr(thetas), resp=_lib.ptr(resp), counts=_lib.ptr(counts),
                                      pop=_lib.ptr(pop), N=N, F=F, S=S, G=G, U=U, B=B, seed=seed)
    entry = _lib_mixture.lib().tq_mixture_count

    def launch():
        _lib.check(entry(C.byref(a), stream()), "tq_mixture_count")

    launch.keep = (counts, pop, filt, thetas, resp)
    return launch


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
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "mixture_dwell_bench measures the MI355X"
    prior, S = 1.0 / 3.0, args.samples
    p = torch.from_numpy(synthetic_hmm(args.aois, args.frames, seed=0)[0]).to("cuda")
    runs, fns = {}, {}
    for U, B in CHAINS:
        for G in POPULATIONS:
            fit = mixture_fit(p, prior, U, B, populations=G, num_iter=50, tol=0.0)
            filt, thetas, resp = fit["filt"].contiguous(), fit["thetas"].contiguous().clone(), fit["resp"].contiguous().clone()
            tag = f"u{U}b{B}g{G}"
            runs[f"population_{tag}"] = population_launches(filt, thetas, resp, U, B, S, 0)
            fns[f"mixture_count_{tag}"] = mixture_count_launch(filt, thetas, resp, U, B, S, 0)
            if G == 1:  # the single chain the mixture of one population is
                runs[f"chain_u{U}b{B}"] = chain_launches(filt[0].contiguous(), thetas[0].contiguous(), U, B, S, 0)
    for r in runs.values():
        r.count()
        r.scan()
    fns.update({f"{name}_{mode}": getattr(r, mode) for name, r in runs.items() for mode in ("count", "emit")})
    ms, spread = timed(fns, args.reps)
    log(" ".join(f"{k} {v:.4f} (+- {spread[k]:.4f}) ms" for k, v in ms.items()))
    out = {"bench": "mixture_dwell", "S": S, "N": args.aois, "F": args.frames, "reps": args.reps}
    for name, r in runs.items():
        out[f"{name}_intervals"] = r.total
    out.update({f"{k}_ms": round(v, 4) for k, v in ms.items()})
    out.update({f"{k}_spread_ms": round(v, 4) for k, v in spread.items()})
    for U, B in CHAINS:
        for G in POPULATIONS:
            tag = f"u{U}b{B}g{G}"
            for mode in ("count", "emit"):
                out[f"population_over_chain_{tag}_{mode}"] = round(ms[f"population_{tag}_{mode}"] / ms[f"chain_u{U}b{B}_{mode}"], 4)
            out[f"population_over_mixture_count_{tag}"] = round(ms[f"population_{tag}_count"] / ms[f"mixture_count_{tag}"], 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
