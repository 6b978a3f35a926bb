"""Two-channel chain benchmark at the ``smooth`` command's scale: 400 on-target AOIs x 1000 frames of the driven chain of
the tests (b binds at 0.005 per frame without a and at 0.10 with it).  Reports on the device (events, median of `--reps`
after a warm-up with the spread max - min of each, all launches taking turns in one process), every joint launch next to
the existing launch it is modelled on, on the same rows:

  * ``tq_joint_estep`` at R = 1 and R = 5, with and without gamma, next to ``tq_hmm_estep`` at (2, 2) and
    ``tq_multistart_estep`` at (2, 2), R = 5, on channel a;
  * ``tq_joint_mstep`` at R = 5 (the five structures) next to ``tq_multistart_mstep`` at R = 5;
  * ``joint_fit`` of `--em-iters` iterations with tol = 0 of the five structures side by side, next to five one-structure
    fits in sequence;
  * ``tq_joint_viterbi`` next to ``tq_hmm_viterbi`` at (2, 2).

One JSON line with the medians, the spreads and the ratios.

    python scripts/joint_bench.py [--reps 20]
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
from joint_fixture import A_DRIVEN, PRIORS, synthetic_joint  # noqa: E402
from multistart_bench import timed  # noqa: E402
from tapqir_amd.utils.joint_analysis import (STRUCTURE_NAMES, joint_default_start, joint_estep, joint_fit, joint_mstep,  # noqa: E402
                                             joint_viterbi)
from tapqir_amd.utils.mle_analysis import (hmm_default_start, hmm_estep, hmm_viterbi, multistart_estep,  # noqa: E402
                                           multistart_mstep)

PAIRS = [("joint_estep_r1", "hmm_estep"), ("joint_estep_r5", "multistart_estep_r5"), ("joint_estep_r5_gamma", "multistart_estep_r5"),
         ("joint_mstep_r5", "multistart_mstep_r5"), ("joint_viterbi", "hmm_viterbi"), ("joint_em_serial", "joint_em_side_by_side")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--aois", type=int, default=400)
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--em-iters", type=int, default=50)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "joint_bench measures the MI355X"
    iters, (prior_a, prior_b) = args.em_iters, PRIORS
    pa, pb, _ = synthetic_joint(args.aois, args.frames, 0, A_DRIVEN)
    pa, pb = torch.from_numpy(pa).to("cuda"), torch.from_numpy(pb).to("cuda")
    N, F = pa.shape
    f64 = dict(dtype=torch.float64, device="cuda")
    theta1 = joint_default_start()[None].to("cuda")
    theta5 = theta1.repeat(5, 1).contiguous()
    A4, rho4 = hmm_default_start(2, 2)
    chain4 = torch.cat([A4.reshape(-1), rho4]).to("cuda")
    chain4x5 = chain4.repeat(5, 1).contiguous()
    rows1, filt1, gam1 = torch.empty(1, N, 21, **f64), torch.empty(1, N, F, 4, **f64), torch.empty(1, N, F, 4, **f64)
    rows5, filt5, gam5 = torch.empty(5, N, 21, **f64), torch.empty(5, N, F, 4, **f64), torch.empty(5, N, F, 4, **f64)
    trace5, rows5m = torch.zeros(5, 1, **f64), torch.empty(5, N, 21, **f64)
    joint_estep(pa, pb, theta5, prior_a, prior_b, None, None, rows5, filt5)

    def serial():
        return [joint_fit(pa, pb, prior_a, prior_b, structures=[s], num_iter=iters, tol=0.0, chunk=iters) for s in range(5)]

    runs = {
        "joint_estep_r1": lambda: joint_estep(pa, pb, theta1, prior_a, prior_b, None, None, rows1, filt1),
        "joint_estep_r1_gamma": lambda: joint_estep(pa, pb, theta1, prior_a, prior_b, None, gam1, rows1, filt1),
        "hmm_estep": lambda: hmm_estep(pa, chain4, prior_a, 2, 2),
        "joint_estep_r5": lambda: joint_estep(pa, pb, theta5, prior_a, prior_b, None, None, rows5, filt5),
        "joint_estep_r5_gamma": lambda: joint_estep(pa, pb, theta5, prior_a, prior_b, None, gam5, rows5, filt5),
        "multistart_estep_r5": lambda: multistart_estep(pa, chain4x5, prior_a, 2, 2, None, rows5m, filt5),
        "joint_mstep_r5": lambda: joint_mstep(rows5, theta5.clone(), trace5, 0, range(5)),
        "multistart_mstep_r5": lambda: multistart_mstep(rows5, chain4x5.clone(), trace5, 0, 2, 2),
        "joint_viterbi": lambda: joint_viterbi(pa, pb, theta1[0], prior_a, prior_b),
        "hmm_viterbi": lambda: hmm_viterbi(pa, chain4, prior_a, 2, 2),
        "joint_em_side_by_side": lambda: joint_fit(pa, pb, prior_a, prior_b, num_iter=iters, tol=0.0, chunk=iters),
        "joint_em_serial": serial,
    }
    times, out = timed(runs, args.reps)
    ms = {k: statistics.median(v) for k, v in times.items()}
    spread = {k: max(v) - min(v) for k, v in times.items()}
    log(" ".join(f"{k} {ms[k]:.4f} ms (spread {spread[k]:.4f})" for k in ms))
    result = {"bench": "joint", "N": N, "F": F, "reps": args.reps, "em_iters": iters}
    result.update({f"{k}_ms": round(v, 4) for k, v in ms.items()})
    result.update({f"{k}_spread_ms": round(v, 4) for k, v in spread.items()})
    for num, den in PAIRS:
        result[f"{num}_over_{den}"] = round(ms[num] / ms[den], 3)
    together, apart = out["joint_em_side_by_side"], out["joint_em_serial"]
    # the same fits: every structure's final log evidence side by side against its own fit
    diff = max(abs(together["fits"][k]["loglik"] - apart[k]["fits"][0]["loglik"]) / abs(apart[k]["fits"][0]["loglik"])
               for k in range(5))
    assert diff < 1e-9, diff
    result["max_rel_loglik_difference"] = diff
    result["chosen"] = STRUCTURE_NAMES[together["best"]]
    gap = ms["joint_em_serial"] - ms["joint_em_side_by_side"]
    result["side_by_side_faster"] = bool(gap > spread["joint_em_serial"] + spread["joint_em_side_by_side"])
    print(json.dumps(result))


if __name__ == "__main__":
    main()
