"""
The device-drawn minibatch subsample beyond 2048 AOIs or frames (include/tapqir_hip.h: tq_subsample_draw, next_ndx / next_fdx;
CosmosEngine.draw_subsample_device / step_subsampled).

The definition, evaluated on the CPU: the `take` smallest of the n Philox keys of (seed, step, site, element = index) under the
order (key, index), listed ascending by (index mod 256, index div 256).  The export runs the very routine the tail workgroup
of the single-launch minibatch step runs, so it is compared with that definition element by element: at the sizes where the
routine changes path (2048 | 2049: registers | chunks of 256; 2304, 2305: a full last chunk, one key in another) and at the
end of the 16-bit index field (65535, 65536), with seeds and steps whose 65536 keys contain ties.  Then in a fit: what a
launch wrote is what the export gives, and the step on it is the step on the same indices handed over by the host.
"""

import ctypes as C

import numpy as np
import pytest
import torch

from helpers import CosmosEngine, load_hostcheck, make_dataset
from tapqir_amd import _lib
from tapqir_amd.models.cosmos import initial_values

pytestmark = pytest.mark.gpu

SITE = (0xA00, 0xA01)  # TQ_SITE_SUBSAMPLE_N, TQ_SITE_SUBSAMPLE_F (tapqir_amd/csrc/tq_step_minibatch.h)
SEEDS, STEPS = (5, 77), (1, 2)  # (5, 1, frames), (77, 1, both axes), (77, 2, AOIs): two of the 65536 keys are equal
SIZES = (1, 40, 2047, 2048, 2049, 2304, 2305, 4000, 65535, 65536)
_keys = {}


def keys(seed, step, axis, n):
    """The first n Philox keys of the stream, from the host build of the kernels' own generator.  hc_philox draws successive
    values of ONE element's stream, so the 65536 keys of a stream are 65536 calls (0.2 s); each of the eight streams is computed
    once for the whole module and every size reads a prefix of it."""
    k = _keys.get((seed, step, axis))
    if k is None:
        hc = load_hostcheck()
        hc.hc_philox.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint64, C.POINTER(C.c_uint32), C.c_int]
        out = (C.c_uint32 * 1)()
        k = np.empty(_lib.SUBSAMPLE_MAX, np.uint32)
        for i in range(k.size):
            hc.hc_philox(seed, step, SITE[axis], i, out, 1)
            k[i] = out[0]
        k.setflags(write=False)
        _keys[(seed, step, axis)] = k
    return k[:n]


def expected(seed, step, axis, n, take):
    index = np.arange(n)
    sel = np.lexsort((index, keys(seed, step, axis, n)))[:take]
    return sel[np.lexsort((sel // 256, sel % 256))].astype(np.int32)


def takes(n, key):
    """1, min(512, n - 1), n - 1 where valid -- and, where two of the keys are equal, the take that separates the pair: the
    smaller index of the two is selected and the larger is not, which only the index part of the composite decides."""
    t = {t for t in (1, min(512, n - 1), n - 1) if 1 <= t <= n}
    order = np.lexsort((np.arange(n), key))
    tied = np.nonzero(key[order][1:] == key[order][:-1])[0]
    t.update(int(p) + 1 for p in tied)
    return sorted(t)


def test_some_stream_has_a_key_tie():
    """Without one the index tie-break of the composite would go untested (about every second stream of 65536 keys has one)."""
    tied = [(s, t, ax) for s in SEEDS for t in STEPS for ax in (0, 1) if np.unique(keys(s, t, ax, 65536)).size < 65536]
    print("streams with equal keys:", tied)
    assert tied


@pytest.mark.parametrize("n", SIZES)
def test_export_equals_the_definition(n):
    lib = _lib.load()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    pad = 64  # the export writes out[0..take) and nothing else
    split = 0  # takes that fall between two equal keys
    for seed in SEEDS:
        for step in STEPS:
            for axis in (0, 1):
                for take in takes(n, keys(seed, step, axis, n)):
                    out = torch.full((take + pad,), -1, dtype=torch.int32, device="cuda:0")
                    _lib.check(lib.tq_subsample_draw(seed, step, axis, n, take, _lib.ptr(out), stream), "tq_subsample_draw")
                    got = out.cpu().numpy()
                    want = expected(seed, step, axis, n, take)
                    assert np.array_equal(got[:take], want), (n, take, seed, step, axis)
                    assert (got[take:] == -1).all(), (n, take, seed, step, axis)
                    split += take not in (1, min(512, n - 1), n - 1)
    if n == 65536:
        assert split >= 1  # the index tie-break decided at least one selection


def _written(eng):
    """The slot the launch of the step just enqueued wrote (the next step's subsample)."""
    st = eng._sub
    return st["slots"][st["turn"]]


def _engine(d, seed):
    eng = CosmosEngine(d, K=2, device="cuda:0", seed=seed)
    eng.layout.set_constrained(eng.params, initial_values(eng, d))
    return eng


@pytest.mark.parametrize("N,F,nb,fb", [(2, 2049, 2, 16), (2049, 16, 5, 16)])
def test_fit_draws_what_the_export_draws_and_steps_like_a_host_fed_fit(N, F, nb, fb):
    d = make_dataset(N=N, F=F)
    a, b = _engine(d, 9), _engine(d, 9)
    g = torch.Generator().manual_seed(1)
    for it in range(4):
        assert a.step_subsampled(nb, fb, g)
        st = a._sub
        used = st["slots"][1 - st["turn"]].cpu()
        nd = used[:nb].long() if nb < N else None
        fd = used[N:N + fb].long() if fb < F else None
        # the launch of step `it` wrote the subsample of step it + 1 = a.adam_step
        wn, wf = a.draw_subsample_device(nb, fb, a.adam_step)
        nxt = _written(a)
        assert (wn is None) == (nb >= N) and (wf is None) == (fb >= F)
        if wn is not None:
            assert torch.equal(nxt[:nb], wn), it
            assert wn.unique().numel() == nb and 0 <= int(wn.min()) and int(wn.max()) < N
        if wf is not None:
            assert torch.equal(nxt[N:N + fb], wf), it
            assert wf.unique().numel() == fb and 0 <= int(wf.min()) and int(wf.max()) < F
        if it > 0:  # (step 0 ran on the host's draw; every later one on what the launch before it wrote)
            for prev, now in ((prev_n, nd), (prev_f, fd)):
                assert (prev is None and now is None) or torch.equal(prev.cpu().long(), now)
        prev_n, prev_f = wn, wf
        b.step(nd, fd)
        for e in (a, b):
            e.join()
        torch.cuda.synchronize()
        ea, eb = float(a.elbo_out[0]), float(b.elbo_out[0])
        print("step", it, "ELBO", ea, eb)
        assert np.isfinite(eb) and abs(ea - eb) <= 1e-9 * abs(eb), (it, ea, eb)
    va, vb = a.named("params"), b.named("params")
    for n in va:
        assert torch.isfinite(va[n]).all() and torch.equal(va[n], vb[n]), n


def test_opt_out_keeps_the_host_draw(monkeypatch):
    d = make_dataset(N=2, F=2049)
    eng = _engine(d, 3)
    monkeypatch.setenv("TAPQIR_AMD_DEVICE_SUBSAMPLE", "0")
    assert eng.step_subsampled(2, 16, torch.Generator().manual_seed(0)) is False
    assert eng.adam_step == 0  # nothing ran


def test_the_engine_gates_on_the_keys_it_would_draw():
    """The library draws up to 65536 per axis; the engine hands the draw back to the host where the launch's draw would outlast
    its workers: more than engine.DEVICE_SUBSAMPLE_MAX keys over the axes that are subsampled (a measured size).  An axis taken
    whole draws nothing and does not count, whatever its size."""
    from tapqir_amd.models import engine

    assert 2 * 2048 <= engine.DEVICE_SUBSAMPLE_MAX <= _lib.SUBSAMPLE_MAX  # (every data set the parent served stays served)
    F = 4 * engine.DEVICE_SUBSAMPLE_MAX
    eng = _engine(make_dataset(N=2, F=F), 3)
    assert eng.step_subsampled(2, 16, torch.Generator().manual_seed(0)) is False
    assert eng.adam_step == 0
    wn, wf = eng.draw_subsample_device(2, 16, 1)  # (the export itself still serves that size)
    assert wn is None and wf.unique().numel() == 16 and int(wf.max()) < F
    # more AOIs than the gate, all of them taken: only the 17 frames are drawn from
    N = engine.DEVICE_SUBSAMPLE_MAX + 1
    eng = _engine(make_dataset(N=N, F=17), 3)
    assert eng.step_subsampled(N, 16, torch.Generator().manual_seed(0)) is True
    assert eng.step_subsampled(N, 16, None) is True
    wn, wf = eng.draw_subsample_device(N, 16, 2)
    assert wn is None and torch.equal(_written(eng)[N:N + 16], wf)
    eng.join()
    torch.cuda.synchronize()
    assert torch.isfinite(eng.params).all()
