"""
Offset histograms of every length the kernels branch on, on the CPU: the g++ build of the kernels' inline math
(tests/hostcheck) against the float64 oracle at O in {2, 7, 8, 65, 257, 1024, 1025, 2048, 2049} -- one below / at / above the
lane strides (64, 256), the packed kernel's table (TQ_MO_MAX_O = 1024) and the LDS offset table (TQ_OFFTAB_MAX = 2048) --
with the masked, peaked and low-background (exact-Binet) regimes at those lengths, P = 9 and P = 32, and crosstalk.
The host build has none of the launch code, LDS tables or lane strides: those run in test_gpu_offset_histograms.py, which takes
the runner, the checker and the regimes from here.  This file says that the MATH holds at these lengths at the tolerances of
test_hostcheck_parity.py, so that a GPU failure at one of them points at the device code.

Also here: the LDS request of the 16-lane tile routine (helpers.lds_request_bytes) pinned to the header it restates.
"""

import os
import re

import pytest
import torch

from helpers import (GIVEN_STAGES, ROOT, CosmosEngine, fp32_latents, grid, lds_request_bytes, load_hostcheck, make_dataset,
                     make_oracle, oracle_grads, oracle_to_engine, put_latents, rel_err, tile_stride)

FAST_ALPHA = 8.0  # TQ_FAST_ALPHA (tq_pixel.h): background / gain below it takes the exact-Binet side of `fast`
LENGTHS = [2, 7, 8, 65, 257, 1024, 1025, 2048, 2049]
MASKED = dict(hi=330.0, sigma=60.0)  # offsets reaching above the dimmest pixels (~140): masked per pixel, as "wide"
PEAKED = dict(sigma=2.0)             # weights spread over 2^52 > 2^40: the non-factored form of the packed kernel, as "peaked"
WORST = {}  # case -> (ELBO relative error, worst gradient rel_err, its family, ll rel_err): printed by the GPU module


def run_given(dkw, K, ndx=None, fdx=None, device="cpu", crosstalk=False, il_min_units=None, low=None, perturb=0.3, prepare=None):
    """The staged calls on given latents (as run_case / run_xt_case of the parity tests), on the host build (device "cpu") or
    the GPU.  ``low`` = (list of (n, f, c) positions of the batch, value): those background draws are replaced before the base
    draws are recovered, so oracle and kernels see the same values; ``prepare(eng)`` is called on the new engine.  Returns
    (oracle, engine, oracle ELBO, oracle gradients, latents)."""
    gpu = device != "cpu"
    d = make_dataset(K=K, **dkw)
    o = make_oracle(d, K, perturb=perturb, crosstalk=crosstalk)
    eng = CosmosEngine(d, K=K, device=device, lib=None if gpu else load_hostcheck(), crosstalk=crosstalk)
    if il_min_units is not None:
        eng.il_min_units = il_min_units
    if prepare is not None:
        prepare(eng)
    oracle_to_engine(o, eng)
    nd = torch.arange(d.images.shape[0]) if ndx is None else torch.tensor(ndx)
    fd = torch.arange(d.images.shape[1]) if fdx is None else torch.tensor(fdx)
    lat32, base = fp32_latents(o, nd, fd)
    if low is not None:
        for pos in low[0]:
            lat32["background"][pos] = torch.tensor(low[1]).float().double()
        with torch.no_grad():
            base = o.base_draws(lat32, o._guide_dists(o.constrained(o.params), nd, fd))
    elbo_o, g_o = oracle_grads(o, nd, fd, base)
    a = eng.make_args(None if ndx is None else nd, None if fdx is None else fd, draw_globals=False)
    put_latents(eng, lat32, base)
    for stage in GIVEN_STAGES:
        eng.call(stage, a)
    if gpu:
        torch.cuda.synchronize()
    return o, eng, elbo_o, g_o, lat32


def check(o, eng, elbo_o, g_o, where=None):
    """ELBO to 1e-5 relative, every gradient rel_err < 1e-4, and (cosmos: the crosstalk kernels keep per-dye marginals, which
    the oracle does not form) the log-likelihood of every spot-presence combination to 1e-5 of the largest magnitude."""
    elbo_k = float(eng.elbo_out[0])
    e_err = abs(elbo_k - elbo_o) / abs(elbo_o)
    gv = eng.named("grad")
    assert set(g_o) == set(gv)
    errs = {n: rel_err(gv[n].cpu().double().reshape(ref.shape), ref) for n, ref in g_o.items()}
    fam = max(errs, key=errs.get)
    ll_err = None
    if not eng.crosstalk:
        ll_o = o.last_terms["ll"].detach()
        M, B = ll_o.shape[0], ll_o[0].numel()
        ll_err = rel_err(eng.pix[: M * B].view(M, B).cpu(), ll_o.reshape(M, B))
    if where is not None:
        WORST[where] = (e_err, errs[fam], fam, ll_err)
    assert e_err <= 1e-5, (elbo_k, elbo_o)
    assert errs[fam] < 1e-4, (fam, errs[fam])
    assert ll_err is None or ll_err <= 1e-5, ll_err


def low_background(lat32, low_at, per_wave):
    """The two facts of a low-background case, from the latents: background / gain is below TQ_FAST_ALPHA exactly at the batch
    positions ``low_at`` (flat indices of the (nb, fb, C) batch), and -- ``per_wave`` batch positions share a wave -- the
    launch has another wave with every position at or above it.  Returns background / gain."""
    ratio = (lat32["background"] / lat32["gain"]).reshape(-1)
    is_low = ratio < FAST_ALPHA
    assert sorted(int(i) for i in is_low.nonzero().reshape(-1)) == sorted(low_at), (ratio, low_at)
    waves = [is_low[w:w + per_wave] for w in range(0, ratio.numel(), per_wave)]
    for i in low_at:  # the low unit sits among units that would take the fast side by themselves
        assert per_wave == 1 or int((~waves[i // per_wave]).sum()) >= 1
    assert any(not bool(w.any()) for w in waves), "no wave that is entirely at or above TQ_FAST_ALPHA"
    return ratio


# ---- every length -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("O", LENGTHS)
def test_every_length(O):
    o, eng, elbo_o, g_o, _ = run_given(dict(N=2, F=2, offsets=grid(O)), 2)
    assert eng.O == O
    check(o, eng, elbo_o, g_o)


def test_k4_first_length_without_a_table():
    o, eng, elbo_o, g_o, _ = run_given(dict(N=2, F=2, offsets=grid(2049)), 4)
    assert eng.O == 2049 and eng.K == 4
    check(o, eng, elbo_o, g_o)


def drop_pixel_statistics(eng):
    """What a C caller with one offset value and no pixel statistics gets: the histogram form of every kernel at O = 1."""
    assert eng.O == 1 and eng.pixstats is not None
    eng.pixstats = None


def test_one_offset_without_pixel_statistics():
    o, eng, elbo_o, g_o, _ = run_given(dict(N=2, F=2), 2, prepare=drop_pixel_statistics)
    assert eng.O == 1 and eng.pixstats is None
    check(o, eng, elbo_o, g_o)


@pytest.mark.parametrize("O", [40, 1025])
def test_low_background_unit(O):
    """One unit of four with background / gain ~ 3: the exact-Binet side of `fast` with an offset loop."""
    o, eng, elbo_o, g_o, lat = run_given(dict(N=2, F=2, offsets=grid(O)), 2, low=([(0, 1, 0)], 20.0))
    low_background(lat, [1], 1)
    check(o, eng, elbo_o, g_o)


@pytest.mark.parametrize("O", [257, 2049])
def test_partly_masked(O):
    dkw = dict(N=2, F=2, offsets=grid(O, **MASKED))
    assert float(make_dataset(K=2, **dkw).images.min()) < 330.0
    o, eng, elbo_o, g_o, _ = run_given(dkw, 2)
    check(o, eng, elbo_o, g_o)


def test_peaked_weights():
    o, eng, elbo_o, g_o, _ = run_given(dict(N=2, F=2, offsets=grid(257, **PEAKED)), 2)
    lw = eng.offset_logits.double() / torch.log(torch.tensor(2.0, dtype=torch.float64))
    assert float(lw.max() - lw.min()) > 40.0  # what tq_il2m_body tests before it factors the weights out
    check(o, eng, elbo_o, g_o)


@pytest.mark.parametrize("P,O", [(9, 40), (15, 40), (32, 1), (32, 8)])
def test_odd_and_large_tiles(P, O):
    dkw = dict(N=2, F=2, P=P) if O == 1 else dict(N=2, F=2, P=P, offsets=grid(O))
    o, eng, elbo_o, g_o, _ = run_given(dkw, 2)
    assert (eng.P, eng.O) == (P, O)
    check(o, eng, elbo_o, g_o)


@pytest.mark.parametrize("O", [2, 257])
def test_crosstalk(O):
    o, eng, elbo_o, g_o, _ = run_given(dict(N=2, F=2, C=2, offsets=grid(O)), 2, crosstalk=True)
    assert eng.crosstalk and eng.O == O
    check(o, eng, elbo_o, g_o)


@pytest.mark.parametrize("O", [1, 40])
def test_crosstalk_low_background(O):
    """One AOI-frame of six with background 20 in both channels (background / gain ~ 3)."""
    dkw = dict(N=2, F=3, C=2) if O == 1 else dict(N=2, F=3, C=2, offsets=grid(O))
    o, eng, elbo_o, g_o, lat = run_given(dkw, 2, crosstalk=True, low=([(0, 1, 0), (0, 1, 1)], 20.0))
    low_background(lat, [2, 3], 8)
    check(o, eng, elbo_o, g_o)


# ---- the LDS request --------------------------------------------------------------------------------------------------------
def _define(text, name):
    m = re.search(r"#define\s+%s\s+\(?(\d+)" % name, text)
    assert m, name
    return int(m.group(1))


def test_lds_request_is_the_headers():
    """helpers.lds_request_bytes against tq_tile16_lds_floats: the constants it restates are read from the headers, the formula
    is held to values worked out by hand from the header's text (tq_tile_stride: npix rounded up to 16 mod 32)."""
    csrc = os.path.join(ROOT, "tapqir_amd", "csrc")
    dev = open(os.path.join(csrc, "tq_ksmogn_dev.h")).read()
    api = open(os.path.join(ROOT, "include", "tapqir_hip.h")).read()
    assert (_define(dev, "TQ_UNITS_PER_BLOCK"), _define(dev, "TQ_LANES_PER_UNIT"), _define(dev, "TQ_OFFTAB_MAX")) == (16, 16, 2048)
    assert (_define(api, "TQ_MAX_P"), _define(api, "TQ_MAX_K")) == (32, 4)
    assert ("(size_t)units * (tq_tile_stride(P * P) + 2 * K * TQ_MAX_P) + (((O > 1 || histogram_form) && O <= TQ_OFFTAB_MAX) "
            "? 4 + 4 * (size_t)O : 0)") in dev
    assert "return ((npix + 15) / 32) * 32 + 16;" in dev
    assert "sizeof(int) * (2048 + 8)" in open(os.path.join(csrc, "tq_step_minibatch.h")).read()
    assert [tile_stride(n) for n in (81, 196, 225, 400, 1024)] == [112, 208, 240, 400, 1040]
    # P = 14, K = 2: 16 (208 + 128) floats = 21504 B; K = 3: 16 (208 + 192) = 25600 B; P = 20, K = 2: 16 (400 + 128) = 33792 B
    assert lds_request_bytes(14, 2) == 21504 and lds_request_bytes(14, 3) == 25600 and lds_request_bytes(20, 2) == 33792
    assert lds_request_bytes(14, 2, 1) == lds_request_bytes(14, 2, 2049) == 21504      # no table at O = 1 and above 2048
    assert lds_request_bytes(14, 2, 2) == 21504 + 16 + 32
    assert lds_request_bytes(14, 2, 1, no_pixstats=True) == 21504 + 16 + 16        # the histogram form at O = 1: a table of one
    assert lds_request_bytes(14, 2, 2048) == 21504 + 16 + 32768
    assert lds_request_bytes(14, 2, 2048, slots=4) == 5376 + 16 + 32768                 # the wave-per-unit kernel
    # where the request crosses 64 KB: K = 3, P = 14 in the minibatch kernel above O = (65536 - 25600 - 9264 - 16) / 16 = 1916;
    # K = 2, P = 20 above O = (65536 - 33792 - 16) / 16 = 1983; K = 2 from P = 30 on without any table
    assert lds_request_bytes(14, 3, 1916, minibatch=True) == 65536 < lds_request_bytes(14, 3, 1917, minibatch=True)
    assert lds_request_bytes(20, 2, 2048) == 66576 and lds_request_bytes(20, 2, 1983) == 65536 < lds_request_bytes(20, 2, 1984)
    assert lds_request_bytes(32, 2) == 74752 and lds_request_bytes(30, 2) == 66560 > 65536 > lds_request_bytes(29, 2) == 62464
    # the largest admitted request: K = 4, P = 32, O = 2048 in the minibatch kernel (9264 B of static LDS on top)
    assert lds_request_bytes(32, 4, 2048) == 115728 and lds_request_bytes(32, 4, 2048, minibatch=True) == 124992
    assert lds_request_bytes(14, 1, 1, minibatch=True, draws=True) == 4 * 16 * (208 + 64) + 9264
    assert lds_request_bytes(2, 1, 1, minibatch=True, draws=True) == 8224 + 9264       # the subsample draw's floor
    assert max(lds_request_bytes(P, K, O, minibatch=True, draws=True) for P in range(2, 33) for K in range(1, 5)
               for O in (1, 2, 2048, 2049)) == 124992
