"""Benchmark of ``tq_smooth_dwell`` at the ``dwelltime`` command's defaults: S = 500 posterior rasters, 400 on-target AOIs x
1000 frames of the synthetic two-state chain of the test fixture, smoothed by an EM fit.  Reports on the device (events,
median of `--reps` after a warm-up, the launches taking turns in one process, every launch on buffers allocated before
the clock starts): the COUNT and the EMIT launch of ``tq_smooth_dwell``, and beside them the yardstick, the COUNT and the
EMIT launch of ``tq_dwell_sample`` on as many draws -- once on the fit's p itself (what ``dwelltime`` without ``--smooth``
runs; independent draws flicker, so its rows have several times as many intervals to count and to write) and once on the
Viterbi path as p in {0, 1} (one fixed raster: a like number of intervals per row).  One JSON line.

    python scripts/smooth_dwell_bench.py [--reps 20]
"""

import argparse
import ctypes as C
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "scripts"), os.path.join(ROOT, "tests")]

from dwelltime_bench import log  # noqa: E402
from rates_bench import median_ms  # noqa: E402
from smooth_fixture import synthetic_chain  # noqa: E402
from tapqir_amd import _lib, _lib_smooth  # noqa: E402
from tapqir_amd.utils.mle_analysis import smooth_fit, smooth_viterbi  # noqa: E402


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class Launches:
    """The two launches of one sampler on buffers of their own: ``count()`` and, after ``scan()``, ``emit()``.  The
    histograms are zeroed once: repeated COUNT launches only add to them, which costs the same."""

    def __init__(self, S, N, F, make_args, entry, name):
        dev = "cuda"
        self.S, self.N, self.F, self.make_args, self.entry, self.name = S, N, F, make_args, entry, name
        self.counts = torch.empty(S, N, dtype=torch.int32, device=dev)
        self.hb = torch.zeros(S, F, dtype=torch.int32, device=dev)
        self.hu = torch.zeros(S, F, dtype=torch.int32, device=dev)
        self.tau = torch.empty(S, N, dtype=torch.float32, device=dev)
        self.offsets, self.cols, self.total = None, None, 0

    def count(self):
        a = self.make_args(self, _lib.DWELL_COUNT)
        _lib.check(self.entry(C.byref(a), stream()), self.name)

    def scan(self):
        flat = self.counts.reshape(-1).to(torch.int64)
        csum = torch.cumsum(flat, 0)
        self.offsets = (csum - flat).contiguous()
        self.total = int(csum[-1].item())
        self.cols = torch.empty(_lib.DWELL_COLS, max(self.total, 1), dtype=torch.int32, device="cuda")

    def emit(self):
        a = self.make_args(self, _lib.DWELL_EMIT)
        _lib.check(self.entry(C.byref(a), stream()), self.name)


def dwell_launches(p, S, seed):
    N, F = p.shape

    def make_args(b, mode):
        return _lib.DwellSampleArgs(p=_lib.ptr(p), counts=_lib.ptr(b.counts), hist_bound=_lib.ptr(b.hb),
                                    hist_unbound=_lib.ptr(b.hu), offsets=_lib.ptr(b.offsets), intervals=_lib.ptr(b.cols),
                                    total=b.total, N=N, F=F, S=S, mode=mode, seed=seed)

    return Launches(S, N, F, make_args, _lib.load().tq_dwell_sample, "tq_dwell_sample")


def smooth_launches(filt, theta, S, seed):
    N, F = filt.shape

    def make_args(b, mode):
        return _lib_smooth.SmoothDwellArgs(filt=_lib.ptr(filt), theta=_lib.ptr(theta), counts=_lib.ptr(b.counts),
                                           hist_bound=_lib.ptr(b.hb), hist_unbound=_lib.ptr(b.hu), tau=_lib.ptr(b.tau),
                                           offsets=_lib.ptr(b.offsets), intervals=_lib.ptr(b.cols), total=b.total, N=N,
                                           F=F, S=S, mode=mode, seed=seed)

    return Launches(S, N, F, make_args, _lib_smooth.lib().tq_smooth_dwell, "tq_smooth_dwell")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=500)
    ap.add_argument("--aois", type=int, default=400)
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "smooth_dwell_bench measures the MI355X"
    prior, S = 1.0 / 3.0, args.samples
    p = torch.from_numpy(synthetic_chain(args.aois, args.frames, seed=0)[0]).to("cuda")
    fit = smooth_fit(p, prior)
    theta = fit["theta"].clone()
    path = smooth_viterbi(p, theta, prior).float()
    runs = {"smooth": smooth_launches(fit["filt"], theta, S, 0), "dwell": dwell_launches(p, S, 0),
            "dwell_path": dwell_launches(path, S, 0)}
    for r in runs.values():
        r.count()
        r.scan()
    fns = {f"{name}_{mode}": getattr(r, mode) for name, r in runs.items() for mode in ("count", "emit")}
    ms, _ = median_ms(fns, args.reps)
    log(" ".join(f"{k} {v:.4f} ms" for k, v in ms.items()))
    out = {"bench": "smooth_dwell", "S": S, "N": args.aois, "F": args.frames, "reps": args.reps,
           "fit_iterations": fit["iterations"], "kon": theta[0].item(), "koff": theta[1].item()}
    for name, r in runs.items():
        out[f"{name}_intervals"] = r.total
        for mode in ("count", "emit"):
            out[f"{name}_{mode}_ms"] = round(ms[f"{name}_{mode}"], 4)
    for mode in ("count", "emit"):
        out[f"smooth_over_dwell_{mode}"] = round(ms[f"smooth_{mode}"] / ms[f"dwell_{mode}"], 4)
        out[f"smooth_over_dwell_path_{mode}"] = round(ms[f"smooth_{mode}"] / ms[f"dwell_path_{mode}"], 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
