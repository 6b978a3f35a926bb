"""
16-bit tiles of the fused pixel + per-unit launch (tq_cosmos_args.images_il16; tq_ksmogn_il2.h, tq_step_rows.h): where the
images are integers in [0, 65535] the packed pixel loop streams a 2-byte-per-pixel interleaved copy instead of the fp32 one.
A 16-bit integer converts to fp32 exactly and everything behind the conversion is the same source, so a step gives the same
BITS with either copy -- which is what these tests hold it to (torch.equal, no tolerance).

Shape: N = 3 AOIs x F = 300 frames = 900 units = 15 tiles, the shape of test_gpu_split_tiles.py: tile 14 has 4 live lanes,
tiles 4 and 9 straddle an AOI boundary.  il_min_units = 1, fuse_unit = True.  The simulator floors its images
(utils/simulate.py), so the data are exact as they come; the tests check that.

  * the copy itself against tq_images_interleave_n, element for element with the padding, and its exactness flag;
  * an engine over inexact data keeps no 16-bit copy and steps as with TAPQIR_AMD_TILE16=0;
  * three steps with the 16-bit tiles against three with TAPQIR_AMD_TILE16=0, (K, P) in {(1, 14), (2, 14), (2, 20)}, no
    tile split and every tile split: parameters, both moments and the ELBO bit for bit;
  * the same with one unit on the scalar loop of small background / gain, which reads the fp32 copy in both engines;
  * one step against the oracle with the unchanged budget of helpers.assert_gradients_match.
Reference semantics: tapqir/models/cosmos.py:82-462, tapqir/models/model.py:169-183.
"""

import functools

import pytest
import torch

from helpers import (CosmosEngine, gradient_report, lr0_sequence, make_dataset, make_oracle, oracle_to_engine,
                     read_engine_latents)
from test_gpu_production_kernels import setup

from tapqir_amd import _lib

assert gradient_report  # (a fixture: imported for pytest to find it)

N, F = 3, 300
NTILES = (N * F + 63) // 64
FAST_ALPHA = 8.0  # TQ_FAST_ALPHA: below it a tile takes the scalar loop
SEED = 11


# ---- the copy ----------------------------------------------------------------------------------------------------------
def test_the_copy_refuses_bad_arguments():
    """(host code only: refused before any launch)"""
    lib = _lib.load()
    assert lib.tq_version() >= 104
    assert lib.tq_images_interleave_u16_n(None, None, 0, 196, None, None) == 1  # TQ_ERR_ARG
    assert b"tq_images_interleave_u16_n" in lib.tq_last_error()
    assert lib.tq_images_interleave_u16_n(8, 8, 0, 196, 8, None) == 1  # no unit
    assert lib.tq_images_interleave_u16_n(8, 8, 1, 3, 8, None) == 1    # less than one group of pixels
    assert lib.tq_images_interleave_u16_n(8, 8, 1, 196, None, None) == 1  # no flag
    assert lib.tq_interleaved_u16_n(65, 196) == lib.tq_interleaved_floats_n(65, 196) == 2 * 49 * 256


@pytest.mark.gpu
@pytest.mark.parametrize("U,npix", [(65, 196), (65, 400), (900, 196), (900, 400)])
def test_the_copy_and_its_flag(U, npix):
    """U = 65: two blocks, the second with one live lane; U = 900: 15 blocks, the last with 4.  The 16-bit copy widened to
    float equals tq_images_interleave_n's output element for element, padding included (both buffers start from other
    values), and the flag stays 0; with one pixel set in turn to 0.5, -1, 65536 and NaN the flag is 1."""
    lib = _lib.load()
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(1000 * U + npix)
    img = torch.randint(0, 65536, (U, npix), generator=g).float()
    img[0, 0], img[U - 1, npix - 1], img[U // 2, 1] = 0.0, 65535.0, 32768.0
    n = int(lib.tq_interleaved_floats_n(U, npix))
    assert int(lib.tq_interleaved_u16_n(U, npix)) == n == ((U + 63) // 64) * (npix // 4) * 256

    def copies(images):
        images = images.to(dev).contiguous()
        il = torch.full((n,), -1.0, dtype=torch.float32, device=dev)
        il16 = torch.full((n,), 0x7777, dtype=torch.int16, device=dev)  # (the 16 bits of a uint16_t)
        flag = torch.zeros(1, dtype=torch.int32, device=dev)
        _lib.check(lib.tq_images_interleave_n(images.data_ptr(), il.data_ptr(), U, npix, None), "tq_images_interleave_n")
        _lib.check(lib.tq_images_interleave_u16_n(images.data_ptr(), il16.data_ptr(), U, npix, flag.data_ptr(), None),
                   "tq_images_interleave_u16_n")
        torch.cuda.synchronize()
        return il, (il16.to(torch.int32) & 0xFFFF).float(), int(flag.item())

    il, wide, flag = copies(img)
    assert flag == 0
    assert torch.equal(wide, il)
    assert float(il.min()) == 0.0 and float(il.max()) == 65535.0  # (nothing of the -1 / 0x7777 fill is left)
    places = [(0, 0), (U - 1, npix - 1), (64, npix // 2), (U // 2, 3)]
    for (u, p), bad in zip(places, (0.5, -1.0, 65536.0, float("nan"))):
        spoilt = img.clone()
        spoilt[u, p] = bad
        assert copies(spoilt)[2] == 1, (u, p, bad)


# ---- engines on identical data ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _data(K, P):
    """The data set and the oracle that holds the initial parameters of a (K, P) case: built once, never changed."""
    d = make_dataset(K=K, N=N, F=F, P=P)
    assert bool((d.images == d.images.floor()).all()) and 0 <= float(d.images.min()) and float(d.images.max()) <= 65535
    return d, make_oracle(d, K, perturb=0.3)


def _engine(monkeypatch, d, o, K, tile16, split):
    monkeypatch.setenv("TAPQIR_AMD_TILE16", "auto" if tile16 else "0")
    eng = CosmosEngine(d, K=K, device="cuda:0", seed=SEED)
    oracle_to_engine(o, eng)
    eng.il_min_units = 1
    eng.fuse_unit = True
    eng.pu_split = split
    assert eng._fusable() and NTILES == 15 and eng.images_il16 is None  # (built by the first fused step)
    return eng


def _run(eng, tile16, split, steps=3, after_step=None):
    """`steps` steps, each checked to have taken the fused launch with the tiles in the format asked for; returns device
    copies of the parameters, both moments and the ELBO after the last one."""
    for it in range(steps):
        eng.step()
        a = eng._tail_args
        assert a is not None and a.pixel_mode == _lib.PIXEL_FUSED_UNIT and a.pu_split == split
        assert split == 0 or (a.pu_scratch and a.pu_scratch_tiles >= split)
        assert bool(a.images_il16) == tile16 and bool(a.images_il)
        assert (eng.images_il16 is not None) == tile16
        if tile16:
            assert a.images_il16 == eng.images_il16.data_ptr() and eng.images_il16.numel() == eng.images_il.numel()
        if after_step is not None:
            after_step(eng)
    out = [t.detach().clone() for t in (eng.params, eng.exp_avg, eng.exp_avg_sq, eng.elbo_out)]  # (the reads join)
    assert all(bool(torch.isfinite(t).all()) for t in out)
    return out


def _assert_same_bits(got, want, where):
    for name, x, y in zip(("params", "exp_avg", "exp_avg_sq", "elbo_out"), got, want):
        assert torch.equal(x, y), (where, name, int((x != y).sum()), float((x.double() - y.double()).abs().max()))


@pytest.mark.gpu
@pytest.mark.parametrize("split", [0, NTILES], ids=["unsplit", "every_tile_split"])
@pytest.mark.parametrize("K,P", [(1, 14), (2, 14), (2, 20)])
def test_steps_are_bit_identical_with_either_tile_format(monkeypatch, K, P, split):
    d, o = _data(K, P)
    want = _run(_engine(monkeypatch, d, o, K, False, split), False, split)
    got = _run(_engine(monkeypatch, d, o, K, True, split), True, split)
    _assert_same_bits(got, want, (K, P, split))


@pytest.mark.gpu
def test_inexact_data_keep_the_fp32_tiles(monkeypatch):
    """One pixel of 900 x 196 is half a count off an integer: the engine builds the copy at its first fused step, reads the
    flag, keeps nothing, and steps bit for bit as an engine with TAPQIR_AMD_TILE16=0 does."""
    d = make_dataset(K=2, N=N, F=F, P=14)
    d.images[1, 7, 0, 3, 5] += 0.5
    o = make_oracle(d, 2, perturb=0.3)
    want = _run(_engine(monkeypatch, d, o, 2, False, 0), False, 0)
    eng = _engine(monkeypatch, d, o, 2, True, 0)
    assert eng.tile16
    got = _run(eng, False, 0)
    assert eng.images_il16 is None and eng._tile16_tried
    _assert_same_bits(got, want, "inexact data")


@pytest.mark.gpu
@pytest.mark.parametrize("split", [0, NTILES], ids=["unsplit", "every_tile_split"])
def test_a_scalar_loop_tile_reads_the_fp32_copy(monkeypatch, split):
    """Unit (AOI 2, frame 100) = unit 700 of tile 10 draws its background near 10, far below TQ_FAST_ALPHA x gain: tile 10
    takes the scalar loop, which reads the fp32 copy whatever the packed loop streams (split: in the wave that draws the
    tile's last ticket)."""
    d, _ = _data(2, 14)
    o = make_oracle(d, 2, perturb=0.3)
    with torch.no_grad():
        o.params["b_loc"][2, 100, 0] = torch.tensor(10.0).log()
        o.params["b_beta"][2, 100, 0] = torch.tensor(5.0).log()

    def scalar_loop_for_tile_10_only(eng):
        lat = read_engine_latents(eng, N, F)
        alpha = lat["background"][:, :, 0] / lat["gain"]
        assert float(alpha[2, 100]) < FAST_ALPHA
        alpha[2, 100] = 1e9
        assert float(alpha.min()) >= FAST_ALPHA

    want = _run(_engine(monkeypatch, d, o, 2, False, split), False, split, after_step=scalar_loop_for_tile_10_only)
    got = _run(_engine(monkeypatch, d, o, 2, True, split), True, split, after_step=scalar_loop_for_tile_10_only)
    _assert_same_bits(got, want, ("scalar loop", split))


@pytest.mark.gpu
@pytest.mark.usefixtures("gradient_report")
def test_a_step_with_16_bit_tiles_against_the_oracle(monkeypatch):
    """One step of K = 2, P = 14 with the 16-bit tiles, every gradient per element against the oracle with the budget of
    helpers.assert_gradients_match, unchanged (1e-4 |g| + 16 E32 + R).  Measured on MI355X: worst excess over the relative
    term 1.37 E32 (b_beta; budget 16) -- m_probs 0.55, b_loc 0.74, w_size 0.36, the others below 0.1 -- the figures of the
    fp32-tile step of the same inputs (test_gpu_split_tiles.py)."""
    monkeypatch.delenv("TAPQIR_AMD_TILE16", raising=False)
    d, o, eng = setup(2, dict(N=N, F=F, P=14), perturb=0.3)
    eng.il_min_units = 1
    eng.fuse_unit = True
    eng.pu_split = 0
    assert eng._fusable() and eng.tile16

    def post(e):
        a = e._tail_args
        assert a is not None and a.pixel_mode == _lib.PIXEL_FUSED_UNIT and a.images_il16
        assert e.images_il16 is not None and a.images_il16 == e.images_il16.data_ptr()

    pend = lr0_sequence(eng, o, [dict(nd=None, fd=None, post=post)], "16-bit tiles K2 P14")
    assert pend == [True]
