"""Credible intervals of a c2-sized fit (400 AOIs x 1000 frames, K = 2): device time of ``tq_credible_intervals`` over the five
per-unit posteriors, wall time of ``compute_params(0.95)``, and the scipy helpers on the same inputs on this machine.

Two parameter sets: the initial values, and the same with N(0, 0.3) added to every unconstrained leaf.  The line
"compute_params with the host helpers" routes the five per-unit posteriors through scipy, which is what compute_params
did before the device path existed."""
import ctypes as C, math, os, statistics, sys, time
import torch
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from tapqir_amd import _lib
from tapqir_amd.models import models
from tapqir_amd.utils import stats
from tapqir_amd.utils.simulate import TEST_PARAMS, simulate

N, F, K, P, CI = 400, 1000, 2, 14, 0.95


def local_inputs(m):
    cp = {n: v.detach() for n, v in m.engine.layout.constrained(m.engine.params).items()}
    H, pr = (P + 1) / 2, m.priors
    return [("background", _lib.INTERVAL_GAMMA, cp["b_loc"], cp["b_beta"], 0.0, 0.0),
            ("height", _lib.INTERVAL_GAMMA, cp["h_loc"], cp["h_beta"], 0.0, 0.0),
            ("width", _lib.INTERVAL_AFFINE_BETA, cp["w_mean"], cp["w_size"], pr["width_min"], pr["width_max"]),
            ("x", _lib.INTERVAL_AFFINE_BETA, cp["x_mean"], cp["size"], -H, H),
            ("y", _lib.INTERVAL_AFFINE_BETA, cp["y_mean"], cp["size"], -H, H)]


def kernel_ms(kind, p0, p1, low, high, reps=7, warm=2):
    shape = torch.broadcast_shapes(p0.shape, p1.shape)
    a0, a1 = p0.float().expand(shape).contiguous(), p1.float().expand(shape).contiguous()
    ll, ul = (torch.empty(shape, dtype=torch.float64, device=a0.device) for _ in range(2))
    a = _lib.IntervalArgs()
    a.kind, a.p0, a.p1, a.ll, a.ul = kind, _lib.ptr(a0), _lib.ptr(a1), _lib.ptr(ll), _lib.ptr(ul)
    a.n, a.ci, a.low, a.high = a0.numel(), CI, float(low), float(high)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    times = []
    for r in range(warm + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        _lib.check(_lib.load().tq_credible_intervals(C.byref(a), stream), "tq_credible_intervals")
        e1.record()
        e1.synchronize()
        if r >= warm:
            times.append(e0.elapsed_time(e1))
    return statistics.median(times), a0.numel()


def wall(fn, reps):
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return statistics.median(out)


def main():
    class _M:
        K, device = 2, torch.device("cuda", 0)

    m = models["cosmos"](S=1, K=K, device="cuda", dtype="double")
    m.data = simulate(_M, N, F, 1, P, seed=2, params=TEST_PARAMS)
    m.init(lr=0.005, nbatch_size=N, fbatch_size=F)
    print(f"device {torch.cuda.get_device_name(0)}; host cores available to this process: {len(os.sched_getaffinity(0))} "
          f"(of {os.cpu_count()}); scipy is single-threaded here")
    for tag in ("init values", "perturbed (unconstrained + 0.3 N(0, 1))"):
        if tag != "init values":
            g = torch.Generator().manual_seed(1)
            m.engine.params += 0.3 * torch.randn(m.engine.params.shape, generator=g).to(m.engine.params)
        m._probs = None
        m.compute_probs  # the spot probabilities are not what is measured: keep them cached
        print(f"-- {tag}")
        total, elems = 0.0, 0
        for name, kind, p0, p1, low, high in local_inputs(m):
            ms, n = kernel_ms(kind, p0, p1, low, high)
            total, elems = total + ms, elems + n
            print(f"   tq_credible_intervals {name:10s} {n:8d} elements: {ms:8.3f} ms (median of 7 after 2 warm-ups)")
        print(f"   device kernels, five posteriors, {elems} elements: {total:.3f} ms")
        t_dev = wall(lambda: m.compute_params(CI), 5)
        print(f"   compute_params wall (device path): {t_dev * 1e3:.1f} ms (median of 5)")
        t0 = time.perf_counter()
        for name, kind, p0, p1, low, high in local_inputs(m):
            if kind == _lib.INTERVAL_GAMMA:
                stats.gamma_interval(p0, p1, CI)
            else:
                stats.affine_beta_interval(p0, p1, low, high, CI)
        t_scipy = time.perf_counter() - t0
        print(f"   scipy helpers on the same inputs: {t_scipy:.2f} s (one pass)")
        keep = stats.gamma_interval_device, stats.affine_beta_interval_device
        stats.gamma_interval_device, stats.affine_beta_interval_device = stats.gamma_interval, stats.affine_beta_interval
        try:
            t_host = wall(lambda: m.compute_params(CI), 1)
        finally:
            stats.gamma_interval_device, stats.affine_beta_interval_device = keep
        print(f"   compute_params wall with the host helpers (as before the device path): {t_host:.2f} s (one pass)")


if __name__ == "__main__":
    main()
