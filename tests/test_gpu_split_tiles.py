"""
Split tiles of the fused pixel + per-unit launch (tq_cosmos_args.pu_split; tq_step_rows.h): the last n tiles of 64 units are
each rendered by four waves that take a range of rows, and the wave that finishes last adds the four partial sums in a fixed
order and goes on as the wave of a whole tile does.

Shape: N = 3 AOIs x F = 300 frames = 900 units = 15 tiles, the shape of the fused-kernel tests.  (The rows layout, which the
fused launch needs, takes F C >= 256 -- a group of 4096 units must not touch more than 17 AOIs -- so no smaller batch with an
AOI boundary inside a tile reaches the kernel; an AOI boundary is then at least four tiles from the end.)  Tile 4 straddles
AOIs 0 / 1, tile 9 straddles AOIs 1 / 2, tile 14 has 4 live lanes.  pu_split in {1, 6, 15}: the partial last tile alone, the
tiles 9 .. 14 with a straddled AOI boundary, every tile.  il_min_units = 1, fuse_unit = True.

Gradients per element against the oracle with the budget of helpers.assert_gradients_match, unchanged; split against
unsplit on identical inputs with that same budget; bit-identical repeats; a unit of a split tile on the scalar loop of small
background / gain; the automatic rule.
Measured on MI355X: worst excess over the relative term in units of E32 (budget 16) -- K = 2, P = 14: 1.37 (b_beta);
K = 1, P = 14: 2.83 (m_probs); K = 2, P = 20: 5.0 (m_probs); small alpha: 1.37 (b_beta); the unsplit step of the same
inputs: 1.37 (b_beta).  Split against unsplit, all 15 tiles: largest difference of a gradient element 4.5e-6 of the family's
largest gradient, parameters after the update 1.5e-8, second moments 7.7e-9 of the largest, -ELBO 7.2e-9 relative.
Reference semantics: tapqir/models/cosmos.py:82-462, tapqir/models/model.py:169-183.
"""

import pytest
import torch

from helpers import (ADAM_B2, ELBO_RTOL, EPS32, PARAM_ATOL, assert_gradients_match, check_step, engine_state, gradient_report,
                     lr0_sequence, oracle_grads, oracle_grads32, oracle_to_engine, read_engine_latents, recover_step_gradient)
from test_gpu_production_kernels import setup

from tapqir_amd import _lib

assert gradient_report  # (a fixture: imported for pytest to find it)

N, F = 3, 300
NTILES = (N * F + 63) // 64
SPLITS = (1, 6, NTILES)  # the last tile; tiles 9 .. 14 (tile 9 straddles AOIs 1 / 2); every tile
FAST_ALPHA = 8.0         # TQ_FAST_ALPHA: below it a tile takes the scalar loop


def _engine(K, P, perturb=0.3):
    d, o, eng = setup(K, dict(N=N, F=F, P=P), perturb=perturb)
    eng.il_min_units = 1
    eng.fuse_unit = True
    assert eng._fusable() and NTILES == 15
    return d, o, eng


def _step(split):
    """One step of a plan: sets pu_split before the launch and checks afterwards that the fused launch ran with it."""
    def pre(e):
        e.pu_split = split

    def post(e):
        a = e._tail_args
        assert a is not None and a.pixel_mode == _lib.PIXEL_FUSED_UNIT and a.pu_split == split
        assert split == 0 or (a.pu_scratch and a.pu_scratch_tiles >= split)
    return dict(nd=None, fd=None, pre=pre, post=post)


@pytest.mark.gpu
@pytest.mark.usefixtures("gradient_report")
@pytest.mark.parametrize("K,P", [(2, 14), (1, 14), (2, 20)])
def test_split_steps_against_oracle(K, P):
    """Split and unsplit steps in turn, each launch carrying the tail of the one before: 1, none, 6, none, 15, 6 tiles."""
    d, o, eng = _engine(K, P)
    plan = [_step(s) for s in (SPLITS[0], 0, SPLITS[1], 0, SPLITS[2], SPLITS[1])]
    found = []
    for e in plan:
        def pre(eng, inner=e["pre"]):
            inner(eng)
            found.append(eng._tail_args is not None and eng._ws_key == (N, F))
        e["pre"] = pre
    pend = lr0_sequence(eng, o, plan, "split tiles K%d P%d" % (K, P))
    assert pend == [True] * 6 and found == [False] + [True] * 5


def _restore(eng, state, step):
    for name, saved in zip(("params", "exp_avg", "exp_avg_sq"), state):
        getattr(eng, name).copy_(saved)
    eng.reset_adam_clock(step)


def _one_step(eng, state, split):
    """One step at the engine's lr from `state` (device copies of params and moments at Adam step 0) with pu_split = split:
    (engine_state after, -ELBO, raw device copies of everything the step wrote)."""
    _restore(eng, state, 0)
    eng.pu_split = split
    eng.step()
    assert eng._tail_args.pu_split == split and eng._tail_args.pixel_mode == _lib.PIXEL_FUSED_UNIT
    after = engine_state(eng)  # (joins)
    torch.cuda.synchronize()
    raw = [t.detach().clone() for t in (eng.params, eng.exp_avg, eng.exp_avg_sq, eng.elbo_out, eng.lat)]
    return after, -float(eng.elbo_out[0]), raw


@pytest.mark.gpu
@pytest.mark.usefixtures("gradient_report")
def test_split_against_unsplit_on_identical_inputs(capsys):
    """One step at lr = 0.005 with every tile split and with none, from the same state and the same draws: both against the
    oracle (check_step), and one against the other with the budget of the gradient helper -- element-wise
    1e-4 |g| + 16 E32 + R with the unsplit gradient as the reference and E32 the oracle's own fp32 error."""
    d, o, eng = _engine(2, 14)
    state = tuple(getattr(eng, n).detach().clone() for n in ("params", "exp_avg", "exp_avg_sq"))
    before = engine_state(eng)
    after_s, loss_s, raw_s = _one_step(eng, state, NTILES)
    after_u, loss_u, raw_u = _one_step(eng, state, 0)
    assert torch.equal(raw_s[4], raw_u[4])  # the same draws
    nd, fd = torch.arange(N), torch.arange(F)
    lat32 = read_engine_latents(eng, N, F)
    with torch.no_grad():
        base = o.base_draws(lat32, o._guide_dists(o.constrained(o.params), nd, fd))
    elbo_o, g64 = oracle_grads(o, nd, fd, base)
    g32 = oracle_grads32(o, nd, fd, base)
    for after, loss, tag in ((after_s, loss_s, "every tile split"), (after_u, loss_u, "no tile split")):
        assert abs(loss + elbo_o) <= ELBO_RTOL * abs(elbo_o), (tag, loss, -elbo_o)
        check_step(eng, before, after, g64, g32, "split / unsplit: " + tag)
    # one against the other
    lay = eng.layout
    gs, Rs = recover_step_gradient(before[1], after_s[1])
    gu, Ru = recover_step_gradient(before[1], after_u[1])
    ref = {n: v for n, v in lay.views(gu).items() if n in g64}
    shifted32 = {n: ref[n].reshape(g64[n].shape) + (g32[n].double() - g64[n].detach().double()) for n in ref}  # same E32 per family
    assert_gradients_match(lay.views(gs), {n: v.reshape(g64[n].shape) for n, v in ref.items()}, shifted32, lay.views(Rs + Ru),
                           "split against unsplit")
    # the second moments: v = (1 - b2) g^2 on both sides, so they differ by what the gradients may differ by
    e32 = torch.zeros_like(gu)
    for n, v in lay.views(e32).items():
        if n in g64:
            v.fill_(float((g32[n].double() - g64[n].detach().double()).abs().max()))
    bg = 1e-4 * gu.abs() + 16.0 * e32 + Rs + Ru
    bound_v = (1.0 - ADAM_B2) * (2.0 * gu.abs() * bg + bg ** 2) + 4.0 * EPS32 * (after_s[2] + after_u[2])
    dv = (after_s[2] - after_u[2]).abs()
    assert bool((dv <= bound_v).all()), ("exp_avg_sq", int((dv - bound_v).argmax()))
    dp = float((after_s[0] - after_u[0]).abs().max())
    assert dp < PARAM_ATOL, dp
    assert abs(loss_s - loss_u) <= ELBO_RTOL * abs(loss_u)
    rel = max(float((a - b).abs().max() / b.abs().max()) for a, b in
              ((lay.views(gs)[n], lay.views(gu)[n]) for n in g64))
    with capsys.disabled():
        print("\nsplit against unsplit: largest gradient difference %.3g of a family's largest gradient, parameters %.3g, "
              "second moments %.3g relative to the largest, -ELBO %.3g relative" % (
                  rel, dp, float(dv.max() / after_u[2].max()), abs(loss_s - loss_u) / abs(loss_u)))


@pytest.mark.gpu
def test_split_steps_are_bit_identical_whoever_arrives_last():
    """Three pairs of runs with every tile split from the same state: parameters, both moments, -ELBO and the draws are
    bit-identical in all six (the partial sums are added in a fixed order by whichever wave draws the last ticket)."""
    d, o, eng = _engine(2, 14)
    state = tuple(getattr(eng, n).detach().clone() for n in ("params", "exp_avg", "exp_avg_sq"))
    first = None
    for pair in range(3):
        for run in range(2):
            raw = _one_step(eng, state, NTILES)[2]
            if first is None:
                first = raw
                assert bool(torch.isfinite(raw[0]).all()) and bool(torch.isfinite(raw[3]).all())
            for name, x, y in zip(("params", "exp_avg", "exp_avg_sq", "elbo", "lat"), first, raw):
                assert torch.equal(x, y), (pair, run, name)


@pytest.mark.gpu
@pytest.mark.usefixtures("gradient_report")
def test_a_small_alpha_unit_in_a_split_tile():
    """Unit (AOI 2, frame 100) = unit 700 of tile 10 draws its background near 10: background / gain is far below
    TQ_FAST_ALPHA, so tile 10 takes the scalar loop -- which is not shared out: the wave that draws the tile's last ticket
    runs all of it.  Tile 10 is among the split tiles for pu_split = 6 and 15."""
    d, o, eng = _engine(2, 14)
    with torch.no_grad():
        o.params["b_loc"][2, 100, 0] = torch.tensor(10.0).log()
        o.params["b_beta"][2, 100, 0] = torch.tensor(5.0).log()
    oracle_to_engine(o, eng)
    plan = [_step(SPLITS[1]), _step(SPLITS[2]), _step(0)]
    for e in plan:
        def post(eng, inner=e["post"]):
            inner(eng)
            lat = read_engine_latents(eng, N, F)
            alpha = lat["background"][:, :, 0] / lat["gain"]
            assert float(alpha[2, 100]) < FAST_ALPHA  # the scalar loop for tile 10 ...
            alpha[2, 100] = 1e9
            assert float(alpha.min()) >= FAST_ALPHA   # ... and for no other tile
        e["post"] = post
    pend = lr0_sequence(eng, o, plan, "small alpha in a split tile")
    assert pend == [True] * 3


def test_the_automatic_rule():
    """pu_split = -1 (host arithmetic only): nothing below one full round of waves; the last round where it is at most an
    eighth full (the issue's quarter was measured to lose at its boundary) -- at 2048 wave slots
    106 of the 6250 tiles of c2, none of the 25 000 of a c3 shard (424 left over)."""
    lib = _lib.load()
    auto = lib.tq_cosmos_pu_split_auto
    for slots in (2048, 1024, 1536, 3072):
        assert all(auto(n, slots) == 0 for n in range(0, slots))
        assert auto(slots, slots) == 0 and auto(slots + 1, slots) == 1
        assert auto(slots + slots // 8, slots) == slots // 8 and auto(slots + slots // 8 + 1, slots) == 0
        assert auto(5 * slots - 1, slots) == 0
    assert auto(6250, 2048) == 106 and auto(25000, 2048) == 0 and auto(6401, 2048) == 0 and auto(6400, 2048) == 256
    assert auto(6250, 0) == 0
    assert lib.tq_cosmos_pu_scratch_bytes(0) == 0 and lib.tq_cosmos_pu_scratch_bytes(106) >= 106 * (4 + 4 * 46 * 64 * 4)


@pytest.mark.gpu
def test_the_automatic_rule_on_the_device():
    """With the wave slots the device reports for the instantiated kernel: an engine below one round (every shape of the
    suite) gets no scratch and splits nothing, and c2's tile count splits ntiles mod slots where the rule allows it."""
    lib = _lib.load()
    slots = lib.tq_cosmos_pu_slots(2, 14)
    assert slots >= 256 and slots % 4 == 0, slots
    assert lib.tq_cosmos_pu_slots(3, 14) == 0 and lib.tq_cosmos_pu_slots(2, 16) == 0
    r = 6250 % slots
    assert lib.tq_cosmos_pu_split_auto(6250, slots) == (r if 6250 >= slots and 0 < r <= slots // 8 else 0)
    d, o, eng = _engine(2, 14, perturb=0.0)
    assert NTILES < slots
    eng.pu_split = -1
    eng.step()
    a = eng._tail_args
    assert a.pixel_mode == _lib.PIXEL_FUSED_UNIT and a.pu_split == -1 and not a.pu_scratch and a.pu_scratch_tiles == 0
    eng.join()
    assert bool(torch.isfinite(eng.params).all())
