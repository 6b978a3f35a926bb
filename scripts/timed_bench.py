"""Continuous-time chain benchmark at the ``smooth`` command's scale: 400 on-target AOIs x 1000 frames of the three-state
reference chain, (U, B) = (1, 1), (1, 2) and (2, 2), and three sets of time stamps with D = 1 (equal spacing), D = 3 (two
speeds and a pause) and D = F - 1 (jittered) gap classes.  Reports on the device (events, median of `--reps` after a
warm-up with the spread max - min of each, all timed calls taking turns in one process) per configuration:

  table   one ``tq_timed_table`` launch for the D classes;
  estep   one ``tq_timed_estep`` next to one ``tq_hmm_estep`` on the same rows;
  mstep   one ``tq_timed_mstep`` next to one ``tq_hmm_mstep``;
  fit     ``timed_fit`` next to ``hmm_fit``, `--em-iters` EM iterations each from their default starts.

``estep_bytes_per_row`` is the table traffic of one wave of the E-step, (F - 1) (M^2 + M^4) 8 B: the forward and the
backward sweep read P[cls] once each and the backward sweep K[cls].  One JSON line.

    python scripts/timed_bench.py [--reps 20]
"""

import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "scripts"), os.path.join(ROOT, "tests")]

from dwelltime_bench import log  # noqa: E402
from hmm_fixture import synthetic_hmm  # noqa: E402
from multistart_bench import timed  # noqa: E402
from tapqir_amd.utils.mle_analysis import (hmm_default_start, hmm_estep, hmm_fit, hmm_mstep, timed_default_start,  # noqa: E402
                                           timed_estep, timed_fit, timed_gaps, timed_mstep, timed_tables)

CONFIGS = [(1, 1), (1, 2), (2, 2)]


def stamp_sets(F, seed):
    """Equal spacing, two speeds with a pause, and a 2 % jitter: D = 1, 3 and F - 1 classes."""
    two = np.ones(F - 1)
    two[(F - 1) // 2:] = 5.0
    two[(F - 1) // 2] = 60.0
    jitter = 1.0 + 0.02 * np.random.default_rng(seed).uniform(-1, 1, F - 1)
    return {"d1": np.arange(F, dtype=np.float64), "d3": np.concatenate([[0.0], np.cumsum(two)]),
            "dF": np.concatenate([[0.0], np.cumsum(jitter)])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--aois", type=int, default=400)
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--em-iters", type=int, default=50)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "timed_bench measures the MI355X"
    prior, iters = 1.0 / 3.0, args.em_iters
    p = torch.from_numpy(synthetic_hmm(args.aois, args.frames, seed=0)[0]).to("cuda")
    N, F = p.shape
    runs, classes = {}, {}
    for U, B in CONFIGS:
        M = U + B
        tag = f"u{U}b{B}"
        A0, rho0 = hmm_default_start(U, B)
        theta_a = torch.cat([A0.reshape(-1), rho0]).to("cuda")
        Q0, _ = timed_default_start(U, B)
        theta_q = torch.cat([Q0.reshape(-1), rho0]).to("cuda")
        trace = torch.zeros(1, dtype=torch.float64, device="cuda")
        frame_rows = hmm_estep(p, theta_a, prior, U, B)["rows"]
        runs[f"{tag}_hmm_estep"] = lambda U=U, B=B, th=theta_a: hmm_estep(p, th, prior, U, B)
        runs[f"{tag}_hmm_mstep"] = lambda U=U, B=B, th=theta_a.clone(), rows=frame_rows: hmm_mstep(rows, th, trace, 0, U, B)
        runs[f"{tag}_hmm_fit"] = lambda U=U, B=B: hmm_fit(p, prior, U, B, num_iter=iters, tol=-1.0, chunk=iters)
        for name, times in stamp_sets(F, args.seed).items():
            d, cls, _ = timed_gaps(times)
            classes[name] = len(d)
            tables = timed_tables(theta_q, d, U, B)
            rows = timed_estep(p, theta_q, tables, cls, prior, U, B)["rows"]
            key = f"{tag}_{name}"
            runs[f"{key}_table"] = lambda U=U, B=B, th=theta_q, d=d: timed_tables(th, d, U, B)
            runs[f"{key}_estep"] = lambda U=U, B=B, th=theta_q, t=tables, cls=cls: timed_estep(p, th, t, cls, prior, U, B)
            runs[f"{key}_mstep"] = lambda U=U, B=B, th=theta_q.clone(), rows=rows: timed_mstep(rows, th, trace, 0, U, B)
            runs[f"{key}_fit"] = lambda U=U, B=B, times=times: timed_fit(p, prior, times, U, B, num_iter=iters, tol=-1.0,
                                                                         chunk=iters)
    times_ms, _ = timed(runs, args.reps)
    ms = {k: statistics.median(v) for k, v in times_ms.items()}
    spread = {k: max(v) - min(v) for k, v in times_ms.items()}
    log(" ".join(f"{k} {ms[k]:.4f} ms (spread {spread[k]:.4f})" for k in ms))
    result = {"bench": "timed", "N": N, "F": F, "reps": args.reps, "em_iters": iters, "classes": classes}
    result.update({f"{k}_ms": round(v, 4) for k, v in ms.items()})
    result.update({f"{k}_spread_ms": round(v, 4) for k, v in spread.items()})
    for U, B in CONFIGS:
        M, tag = U + B, f"u{U}b{B}"
        result[f"{tag}_estep_bytes_per_row"] = (F - 1) * (M ** 2 + M ** 4) * 8
        for name in classes:
            result[f"{tag}_{name}_estep_over_hmm"] = round(ms[f"{tag}_{name}_estep"] / ms[f"{tag}_hmm_estep"], 4)
            result[f"{tag}_{name}_fit_over_hmm"] = round(ms[f"{tag}_{name}_fit"] / ms[f"{tag}_hmm_fit"], 4)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
