"""Mixture-of-chains benchmark at the ``smooth`` command's scale: 400 on-target AOIs x 1000 frames of the three-state
reference chain.  Reports on the device (events, median of `--reps` after a warm-up with the spread max - min of each, all
launches taking turns in one process), each new kernel next to the parent's kernel that does the same work:

* ``tq_mixture_mstep`` at G = 1, 2, 4 of (1, 2) chains next to ``tq_multistart_mstep`` at R = G;
* ``mixture_fit`` of `--em-iters` iterations (tol 0, one chunk) at G = 2 and 3 of (1, 1) chains next to one ``hmm_fit`` at (1, 1)
  and one at (1, 2);
* ``tq_mixture_count`` (with the state pairs) and ``tq_mixture_estimate`` at S = `--samples`, G = 1 and 2 of (1, 2) chains, next
  to ``tq_hmm_count`` and ``tq_hmm_estimate``.

``<a>_over_<b>`` is a ratio of medians and ``..._within_spread`` says whether the two medians differ by no more than the two
spreads together.  One JSON line.

    python scripts/mixture_bench.py [--reps 20]
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
from tapqir_amd.utils.mle_analysis import (hmm_estep, hmm_estimate, hmm_fit, hmm_random_starts, hmm_sample,  # noqa: E402
                                           mixture_estimate, mixture_fit, mixture_mstep, mixture_sample, multistart_estep,
                                           multistart_mstep)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--aois", type=int, default=400)
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--samples", type=int, default=1000)
    ap.add_argument("--em-iters", type=int, default=50)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "mixture_bench measures the MI355X"
    prior, iters, S = 1.0 / 3.0, args.em_iters, args.samples
    p = torch.from_numpy(synthetic_hmm(args.aois, args.frames, seed=0)[0]).to("cuda")
    N, F = p.shape
    U, B, M = 1, 2, 3
    runs, pairs = {}, []
    for G in (1, 2, 4):
        thetas = hmm_random_starts(U, B, G - 1, seed=0).to("cuda")
        rows = multistart_estep(p, thetas, prior, U, B)
        trace = torch.zeros(G, 1, dtype=torch.float64, device="cuda")
        phi = torch.full((1, G), 1.0 / G, dtype=torch.float64, device="cuda")
        runs[f"mstep_mixture_g{G}"] = lambda rows=rows, th=thetas.clone(), phi=phi, trace=trace: mixture_mstep(
            rows[None], th[None], phi, trace[:1], 0, U, B)
        runs[f"mstep_multistart_r{G}"] = lambda rows=rows, th=thetas.clone(), trace=trace: multistart_mstep(rows, th, trace, 0, U, B)
        pairs.append((f"mstep_mixture_g{G}", f"mstep_multistart_r{G}"))
    for G in (2, 3):
        runs[f"em_mixture_g{G}"] = lambda G=G: mixture_fit(p, prior, 1, 1, populations=G, num_iter=iters, tol=0.0, chunk=iters)
        pairs += [(f"em_mixture_g{G}", "em_hmm_u1b1"), (f"em_mixture_g{G}", "em_hmm_u1b2")]
    runs["em_hmm_u1b1"] = lambda: hmm_fit(p, prior, 1, 1, num_iter=iters, tol=0.0, chunk=iters)
    runs["em_hmm_u1b2"] = lambda: hmm_fit(p, prior, 1, 2, num_iter=iters, tol=0.0, chunk=iters)
    thetas = hmm_random_starts(U, B, 1, seed=0).to("cuda")
    filt = torch.stack([hmm_estep(p, t, prior, U, B)["filt"] for t in thetas])
    resp = torch.rand(2, N, dtype=torch.float64, device="cuda")
    resp = resp / resp.sum(0)
    one = torch.ones(1, N, dtype=torch.float64, device="cuda")
    drawn = mixture_sample(filt, thetas, resp, U, B, S, seed=0, trans=True)
    runs["count_hmm"] = lambda: hmm_sample(filt[0], thetas[0], U, B, S, seed=0, trans=True)
    runs["count_mixture_g1"] = lambda: mixture_sample(filt[:1], thetas[:1], one, U, B, S, seed=0, trans=True)
    runs["count_mixture_g2"] = lambda: mixture_sample(filt, thetas, resp, U, B, S, seed=0, trans=True)
    runs["estimate_hmm"] = lambda: hmm_estimate(drawn["trans"], bootstrap=True, seed=0)
    runs["estimate_mixture_g1"] = lambda zero=torch.zeros_like(drawn["pop"]): mixture_estimate(drawn["trans"], zero, 1, bootstrap=True, seed=0)
    runs["estimate_mixture_g2"] = lambda: mixture_estimate(drawn["trans"], drawn["pop"], 2, bootstrap=True, seed=0)
    pairs += [("count_mixture_g1", "count_hmm"), ("count_mixture_g2", "count_hmm"), ("estimate_mixture_g1", "estimate_hmm"),
              ("estimate_mixture_g2", "estimate_hmm")]
    times, out = timed(runs, args.reps)
    ms = {k: statistics.median(v) for k, v in times.items()}
    spread = {k: max(v) - min(v) for k, v in times.items()}
    log(" ".join(f"{k} {ms[k]:.4f} ms (spread {spread[k]:.4f})" for k in ms))
    assert torch.equal(out["count_mixture_g1"]["trans"], out["count_hmm"]["trans"])  # the same rasters at G = 1
    assert torch.equal(out["estimate_mixture_g1"]["totals"][:, 0], out["estimate_hmm"]["totals"])
    result = {"bench": "mixture", "N": N, "F": F, "S": S, "reps": args.reps, "em_iters": iters}
    result.update({f"{k}_ms": round(v, 4) for k, v in ms.items()})
    result.update({f"{k}_spread_ms": round(v, 4) for k, v in spread.items()})
    for a, b in pairs:
        result[f"{a}_over_{b}"] = round(ms[a] / ms[b], 3)
        result[f"{a}_over_{b}_within_spread"] = bool(abs(ms[a] - ms[b]) <= spread[a] + spread[b])
    for G in (2, 3):
        result[f"em_mixture_g{G}_bic"] = round(out[f"em_mixture_g{G}"]["bic"], 4)
    result["em_hmm_u1b1_bic"], result["em_hmm_u1b2_bic"] = round(out["em_hmm_u1b1"]["bic"], 4), round(out["em_hmm_u1b2"]["bic"], 4)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
