"""Benchmark of ``tq_pair_dwell`` at the ``dwelltime`` command's defaults: S = 500 posterior rasters, 400 on-target AOIs x
1000 frames of the driven two-channel chain of the test fixture, the ``a-drives-b`` structure after 50 EM iterations from
the default start.  Reports on the device (events, median of `--reps` after a warm-up and the spread max - min, the
launches taking turns in one process, every launch on buffers allocated before the clock starts): the COUNT and the EMIT
launch of ``tq_pair_dwell`` for channel a (which = 0) and channel b (which = 1), and beside them both launches of its
parent ``tq_chain_dwell`` at (U, B) = (2, 2) on the same filt.  No time is fixed in advance: the ratios to the parent are
the result.  One JSON line.

    python scripts/pair_dwell_bench.py [--reps 20]
"""

import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "scripts"), os.path.join(ROOT, "tests")]

from dwelltime_bench import log  # noqa: E402
from hmm_dwell_bench import chain_launches  # noqa: E402
from joint_fixture import A_DRIVEN, PRIORS, synthetic_joint  # noqa: E402
from mixture_dwell_bench import timed  # noqa: E402
from smooth_dwell_bench import Launches  # noqa: E402
from tapqir_amd import _lib, _lib_joint  # noqa: E402
from tapqir_amd.utils.joint_analysis import joint_fit  # noqa: E402


class PairLaunches(Launches):
    """``Launches`` with histograms of (S, 2, F), the partner's first bound frame that the COUNT launch writes and the
    partner codes that the EMIT launch writes."""

    def __init__(self, S, N, F, make_args, entry, name):
        super().__init__(S, N, F, make_args, entry, name)
        self.hb = torch.zeros(S, 2, F, dtype=torch.int32, device="cuda")
        self.hu = torch.zeros(S, 2, F, dtype=torch.int32, device="cuda")
        self.tau_after = torch.empty(S, N, dtype=torch.float32, device="cuda")
        self.codes = None

    def scan(self):
        super().scan()
        self.codes = torch.empty(max(self.total, 1), dtype=torch.uint8, device="cuda")


def pair_launches(filt, theta, which, S, seed):
    N, F = filt.shape[:2]

    def make_args(b, mode):
        return _lib_joint.PairDwellArgs(filt=_lib.ptr(filt), theta=_lib.ptr(theta), counts=_lib.ptr(b.counts),
                                        hist_bound=_lib.ptr(b.hb), hist_unbound=_lib.ptr(b.hu), tau=_lib.ptr(b.tau),
                                        tau_after=_lib.ptr(b.tau_after), offsets=_lib.ptr(b.offsets), intervals=_lib.ptr(b.cols),
                                        partner=_lib.ptr(b.codes), total=b.total, N=N, F=F, S=S, which=which, mode=mode,
                                        seed=seed)

    return PairLaunches(S, N, F, make_args, _lib_joint.lib().tq_pair_dwell, "tq_pair_dwell")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=500)
    ap.add_argument("--aois", type=int, default=400)
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "pair_dwell_bench measures the MI355X"
    S = args.samples
    pa, pb, _ = synthetic_joint(args.aois, args.frames, 0, A_DRIVEN)
    fit = joint_fit(torch.from_numpy(pa).to("cuda"), torch.from_numpy(pb).to("cuda"), *PRIORS, structures=["a-drives-b"],
                    num_iter=50, tol=0.0)
    filt, theta = fit["filt"].contiguous(), fit["theta"].contiguous()
    runs = {"pair_a": pair_launches(filt, theta, 0, S, 0), "pair_b": pair_launches(filt, theta, 1, S, 0),
            "chain_u2b2": chain_launches(filt, theta, 2, 2, S, 0)}
    for r in runs.values():
        r.count()
        r.scan()
    fns = {f"{name}_{mode}": getattr(r, mode) for name, r in runs.items() for mode in ("count", "emit")}
    ms, spread = timed(fns, args.reps)
    log(" ".join(f"{k} {v:.4f} (+- {spread[k]:.4f}) ms" for k, v in ms.items()))
    out = {"bench": "pair_dwell", "S": S, "N": args.aois, "F": args.frames, "reps": args.reps}
    for name, r in runs.items():
        out[f"{name}_intervals"] = r.total
    out.update({f"{k}_ms": round(v, 4) for k, v in ms.items()})
    out.update({f"{k}_spread_ms": round(v, 4) for k, v in spread.items()})
    for name in ("pair_a", "pair_b"):
        for mode in ("count", "emit"):
            out[f"{name}_over_chain_{mode}"] = round(ms[f"{name}_{mode}"] / ms[f"chain_u2b2_{mode}"], 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
