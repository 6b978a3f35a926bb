"""Dwell-time benchmark at the ``dwelltime`` command's defaults: S = 500 posterior samples, 400 on-target AOIs x 1000
frames, K = 3, 10 000 Adam steps.  Reports on the device (events, after a warm-up): launch A (counts and histograms),
the scan plus launch B (the interval table, without its copy to the host), and the koff and kon fits on the histograms;
and the same fit restated in float64 torch on the CPU (autograd + torch.optim.Adam on the padded data, `--cpu-threads`
threads, `--cpu-steps` steps, extrapolated to 10 000).  One JSON line.

    python scripts/dwelltime_bench.py [--cpu-steps 200] [--cpu-threads 16]
"""

import argparse
import ctypes as C
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "scripts")]

from dwell_fixture import loglik64, init_par  # noqa: E402
from tapqir_amd import _lib  # noqa: E402
from tapqir_amd.utils.imscroll import bound_dwell_times  # noqa: E402
from tapqir_amd.utils.mle_analysis import dwell_csr_from_hist, dwell_fit, dwell_intervals, dwell_sample  # noqa: E402
from ttfb_bench import device_ms  # noqa: E402


def posterior_like(N, F, gen, kon=0.01, koff=0.05):
    """p(z = 1) rasters shaped like a fit's output: a two-state (telegraph) binding process per AOI with on / off rates
    per frame, near 0.97 while bound and near 0.02 while unbound, with some noise."""
    state = torch.zeros(N, dtype=torch.bool)
    z = torch.empty(N, F, dtype=torch.bool)
    u = torch.rand(N, F, generator=gen)
    for f in range(F):
        state = torch.where(state, u[:, f] >= koff, u[:, f] < kon)
        z[:, f] = state
    noise = torch.rand(N, F, generator=gen) * 0.03
    return torch.where(z, 0.97 + noise, 0.02 + noise).clamp(max=1.0)


def log(msg):
    print(msg, file=sys.stderr, flush=True)


def emit_only(p, sample, seed):
    """Scan + launch B as dwell_intervals runs them, without the copy of the table to the host."""
    counts = sample["counts"].reshape(-1).to(torch.int64)
    csum = torch.cumsum(counts, 0)
    offsets = (csum - counts).contiguous()
    total = int(csum[-1].item())
    cols = torch.empty(_lib.DWELL_COLS, max(total, 1), dtype=torch.int32, device=p.device)
    N, F = p.shape
    a = _lib.DwellSampleArgs(p=_lib.ptr(p), offsets=_lib.ptr(offsets), intervals=_lib.ptr(cols), total=total, N=N, F=F,
                             S=sample["counts"].shape[0], mode=_lib.DWELL_EMIT, seed=seed)
    _lib.check(_lib.load().tq_dwell_sample(C.byref(a), C.c_void_p(torch.cuda.current_stream().cuda_stream)), "emit")
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=500)
    ap.add_argument("--steps", type=int, default=10000)
    ap.add_argument("--aois", type=int, default=400)
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("-K", type=int, default=3)
    ap.add_argument("--chunk", type=int, default=1000)
    ap.add_argument("--cpu-steps", type=int, default=200)
    ap.add_argument("--cpu-threads", type=int, default=16)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "dwelltime_bench measures the MI355X"
    gen = torch.Generator().manual_seed(0)
    p = posterior_like(args.aois, args.frames, gen).to("cuda")
    S = args.samples
    count_ms, sample = device_ms(lambda: dwell_sample(p, S, seed=0), reps=10)
    emit_ms, total = device_ms(lambda: emit_only(p, sample, 0), reps=10)
    log(f"count {count_ms:.3f} ms, scan + emit {emit_ms:.3f} ms, {total} intervals")
    table_s = time.perf_counter()
    table = dwell_intervals(p, S, seed=0, sample=sample)
    table_s = time.perf_counter() - table_s
    log(f"table on the host in {table_s:.2f} s")
    fits = {}
    for kind in ("bound", "unbound"):
        hist = sample[f"hist_{kind}"]
        hist = hist[hist.sum(1) > 0]
        csr = dwell_csr_from_hist(hist)
        ms, fit = device_ms(lambda: dwell_fit(csr, args.K, n_steps=args.steps, chunk=args.chunk))
        fits[kind] = (ms, fit, hist.shape[0], int((hist > 0).sum(1).max()))
        log(f"{kind} fit {ms:.2f} ms")
    finite = all(bool(torch.isfinite(f[1][k]).all()) for f in fits.values() for k in ("k", "A", "loss"))

    torch.set_num_threads(args.cpu_threads)
    padded = torch.from_numpy(bound_dwell_times(table)).double()
    par = init_par(padded.shape[0], args.K).requires_grad_(True)
    opt = torch.optim.Adam([par], lr=5e-3, betas=(0.9, 0.999), eps=1e-8)

    def cpu_step():
        opt.zero_grad()
        (-loglik64(par, padded, args.K).sum()).backward()
        opt.step()

    for _ in range(3):  # warm-up
        cpu_step()
    t0 = time.perf_counter()
    for _ in range(args.cpu_steps):
        cpu_step()
    cpu_ms_step = (time.perf_counter() - t0) * 1e3 / args.cpu_steps
    fit_ms = fits["bound"][0] + fits["unbound"][0]
    out = {
        "bench": "dwelltime", "S": S, "N": args.aois, "F": args.frames, "K": args.K, "steps": args.steps,
        "chunk": args.chunk, "intervals": total, "count_ms": round(count_ms, 4), "scan_emit_ms": round(emit_ms, 4),
        "table_to_host_s": round(table_s, 3), "fit_bound_ms": round(fits["bound"][0], 3),
        "fit_unbound_ms": round(fits["unbound"][0], 3), "fits_bound_unbound": [fits["bound"][2], fits["unbound"][2]],
        "max_pairs_bound_unbound": [fits["bound"][3], fits["unbound"][3]],
        "gpu_fit_ms_per_step": round(fits["bound"][0] / args.steps, 5),
        "padded_bound_shape": list(padded.shape), "cpu_f64_bound_ms_per_step": round(cpu_ms_step, 3),
        "cpu_threads": args.cpu_threads, "cpu_steps": args.cpu_steps,
        "cpu_f64_bound_fit_s_extrapolated": round(cpu_ms_step * args.steps / 1e3, 1),
        "speedup_bound_fit": round(cpu_ms_step * args.steps / fits["bound"][0], 1),
        "mean_koff": fits["bound"][1]["k"].mean(0).tolist(), "mean_kon": fits["unbound"][1]["k"].mean(0).tolist(),
        "finite": finite, "total_gpu_ms": round(count_ms + emit_ms + fit_ms, 3),
    }
    print(json.dumps(out))


if __name__ == "__main__":
    main()
