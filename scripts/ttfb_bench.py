"""Time-to-first-binding benchmark at the ``ttfb`` command's defaults: S = 2000 posterior samples, 15 000 Adam steps,
400 on-target AOIs x 1000 frames.  Reports the sampler and fit times on the device (events, after a warm-up), ms per
Adam step, and the same fit restated in float64 torch on the CPU (autograd + torch.optim.Adam, `--cpu-threads`
threads, `--cpu-steps` steps, extrapolated to 15 000).  One JSON line.

    python scripts/ttfb_bench.py [--cpu-steps 200] [--cpu-threads 16]
"""

import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from tapqir_amd.utils.mle_analysis import ttfb_fit, ttfb_sample  # noqa: E402
from ttfb_fixture import torch_fit64  # noqa: E402


def posterior_like(N, F, gen):
    """p(z = 1) rasters shaped like a fit's output: mostly near 0, binding runs near 1 after an exponential wait."""
    p = torch.rand(N, F, generator=gen) * 0.02
    start = (-torch.log(torch.rand(N, generator=gen)) / 0.01).long()
    f = torch.arange(F)
    bound = (f[None, :] >= start[:, None]) & (torch.rand(N, F, generator=gen) < 0.3)
    return torch.where(bound, 0.9 + 0.1 * torch.rand(N, F, generator=gen), p)


def device_ms(fn, reps=1):
    fn()  # warm-up: code objects, allocator
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=2000)
    ap.add_argument("--steps", type=int, default=15000)
    ap.add_argument("--aois", type=int, default=400)
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--chunk", type=int, default=1000)
    ap.add_argument("--cpu-steps", type=int, default=200)
    ap.add_argument("--cpu-threads", type=int, default=16)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "ttfb_bench measures the MI355X"
    gen = torch.Generator().manual_seed(0)
    p = posterior_like(args.aois, args.frames, gen).to("cuda")
    sample_ms, tau = device_ms(lambda: ttfb_sample(p, args.samples, seed=0), reps=10)
    fit_ms, fit = device_ms(lambda: ttfb_fit(tau, float(args.frames), n_steps=args.steps, chunk=args.chunk))
    finite = all(bool(torch.isfinite(fit[k]).all()) for k in ("ka", "kns", "Af", "loss"))

    torch.set_num_threads(args.cpu_threads)
    tau_cpu = tau.cpu()
    torch_fit64(tau_cpu[:, :], float(args.frames), n_steps=5)  # warm-up
    t0 = time.perf_counter()
    torch_fit64(tau_cpu, float(args.frames), n_steps=args.cpu_steps)
    cpu_ms_step = (time.perf_counter() - t0) * 1e3 / args.cpu_steps
    out = {
        "bench": "ttfb", "S": args.samples, "N": args.aois, "F": args.frames, "steps": args.steps, "chunk": args.chunk,
        "sampler_ms": round(sample_ms, 4), "fit_ms": round(fit_ms, 3), "gpu_ms_per_step": round(fit_ms / args.steps, 5),
        "cpu_f64_ms_per_step": round(cpu_ms_step, 3), "cpu_threads": args.cpu_threads, "cpu_steps": args.cpu_steps,
        "cpu_f64_fit_s_extrapolated": round(cpu_ms_step * args.steps / 1e3, 1),
        "speedup": round(cpu_ms_step * args.steps / fit_ms, 1),
        "mean_ka": fit["ka"].mean().item(), "mean_kns": fit["kns"].mean().item(), "mean_Af": fit["Af"].mean().item(),
        "finite": finite,
    }
    print(json.dumps(out))


if __name__ == "__main__":
    main()
