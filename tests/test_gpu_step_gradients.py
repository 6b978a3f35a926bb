"""
Gradients of the tails a fit actually runs, and of steps that change route, against the oracle per element.

Every replay calls join() after each step, so its tail always runs as tq_cosmos_tail.  A fit leaves the tail of a step pending
and runs it inside the NEXT launch (tq_sample_locals_tail_kernel, tq_minibatch_kernel, the split sampling of a sharded step).
helpers.lr0_sequence reaches those with ``eng.lr = 0``: the parameters never move, so the oracle holds them exactly with nothing
read back and no join() in between, while exp_avg still accumulates every step's gradient, which is recovered from it --
local parameters across the launch of the step, per-AOI and global parameters across the launch that carried its tail -- and
held to helpers.assert_gradients_match; -ELBO of every step is read where helpers.free_run reads it.

A change of batch geometry makes the engine join() before it re-sizes its workspace, so a tail is carried only between steps
of one geometry: the full-batch step changes family (fused, two launches with rows of 256, the single launch of small
batches, the flat layout) at a fixed geometry below, and the minibatches carry the tails of minibatches.  Each sequence
asserts which of its launches found a pending tail.
Measured worst excess over the relative term in units of E32 (MI355X; budget 16): sharded in flight 2.5 (m_probs), full-batch
families 1.9 (m_probs; 3.1 with two channels), full / minibatch in turn 1.4 (b_beta), 20 units per workgroup 1.1 (K = 1) / 0.8 (K = 3 hist), flat
layout 0.7 (b_loc).
Reference semantics: tapqir/models/cosmos.py:82-462, tapqir/models/model.py:169-183.
"""

import pytest
import torch

from helpers import gradient_report, lr0_sequence
from test_gpu_production_kernels import TWO_CHANNELS, _Done, setup

from tapqir_amd import _lib

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("gradient_report")]
assert gradient_report  # (a fixture: imported for pytest to find it)


def _subs(N, F, nb, fb, count, seed=5):
    g = torch.Generator().manual_seed(seed)
    return [dict(nd=torch.randperm(N, generator=g)[:nb], fd=torch.randperm(F, generator=g)[:fb]) for _ in range(count)]


def _carried(eng, plan):
    """Adds to every step of ``plan`` a ``pre`` hook recording whether the launch finds a pending tail to carry (a tail is
    pending and the batch geometry, hence the workspace, stays)."""
    found = []
    for e in plan:
        inner = e.get("pre")
        nb = eng.Nt if e.get("nd") is None else len(e["nd"])
        fb = eng.F if e.get("fd") is None else len(e["fd"])

        def pre(eng, inner=inner, key=(nb, fb)):
            if inner is not None:
                inner(eng)
            found.append((eng._tail_args is not None or eng._pending is not None) and eng._ws_key == key)
        e["pre"] = pre
    return found


def test_full_batch_and_minibatch_steps_in_turn():
    """N = 3, F = 300 (900 units): full fused; minibatch 2 x 40 twice; full as two launches (rows of 256); minibatch; full.
    The second minibatch launch carries the first one's rows-of-16 tail; every change between full batch and minibatch
    re-sizes the workspace, which joins: those tails run as tq_cosmos_tail and every unit is brought to the current step."""
    N, F = 3, 300
    d, o, eng = setup(2, dict(N=N, F=F), perturb=0.3)
    eng.il_min_units = 1
    mb = _subs(N, F, 2, 40, 3)

    def fused(e):
        e.fuse_unit = True

    def two_launches(e):
        e.fuse_unit = False

    def is_fused(e):
        assert e._tail_args.pixel_mode == _lib.PIXEL_FUSED_UNIT

    def is_rows(e):
        assert e._tail_args.pixel_mode != _lib.PIXEL_FUSED_UNIT and e._tail_args.tail_kind != _lib.TAIL_ROWS16

    def is_rows16(e):
        assert e._tail_args.tail_kind == _lib.TAIL_ROWS16

    plan = [dict(nd=None, fd=None, pre=fused, post=is_fused), dict(mb[0], post=is_rows16), dict(mb[1], post=is_rows16),
            dict(nd=None, fd=None, pre=two_launches, post=is_rows), dict(mb[2], post=is_rows16),
            dict(nd=None, fd=None, pre=fused, post=is_fused)]
    found = _carried(eng, plan)
    pend = lr0_sequence(eng, o, plan, "full / minibatch in turn")
    assert pend == [True] * 6 and found == [False, False, True, False, False, False]


@pytest.mark.parametrize("dkw", [dict(N=3, F=300), TWO_CHANNELS], ids=["3x300", "3x150x2"])
def test_full_batch_families_carry_each_other_s_tails(dkw):
    """N = 3, F = 300 (and N = 3, F = 150, C = 2: the channel columns of the rows), whole-batch steps of one geometry, so
    that every launch carries the tail of the step before, each time of another family: fused -> two launches with rows of
    256 (the fused step's rows tail inside tq_sample_locals_tail_kernel) -> the single launch of small batches (rows or
    groups inside tq_minibatch_kernel) -> two launches (tq_cosmos_tail of the rows-of-16 tail before the overlapped step) ->
    single launch -> fused."""
    N, F = dkw["N"], dkw["F"]
    d, o, eng = setup(2, dkw, perturb=0.3)

    def fused(e):
        e.il_min_units, e.fuse_unit = 1, True
        e.__dict__.pop("_tmpl_key", None)  # (argument templates carry il_min_units)

    def two_launches(e):
        e.il_min_units, e.fuse_unit = 1, False
        e.__dict__.pop("_tmpl_key", None)

    def one_launch(e):
        e.il_min_units = 65536
        e.__dict__.pop("_tmpl_key", None)

    def route(want):
        def post(e):
            assert e._route(N, F, None) == want
            assert (e._tail_args.tail_kind == _lib.TAIL_ROWS16) == (want == "one_launch")
        return post

    plan = [dict(pre=fused, post=route("overlapped")), dict(pre=two_launches, post=route("overlapped")),
            dict(pre=one_launch, post=route("one_launch")), dict(pre=two_launches, post=route("overlapped")),
            dict(pre=one_launch, post=route("one_launch")), dict(pre=fused, post=route("overlapped"))]
    found = _carried(eng, plan)
    pend = lr0_sequence(eng, o, plan, "full-batch families" + (" C = 2" if dkw.get("C") else ""))
    assert pend == [True] * 6 and found == [False] + [True] * 5


def test_flat_layout_tail_and_minibatches():
    """N = 5, F = 24 (F C < 64: the flat layout of partial sums) with small_full_max_units = 0: full; minibatch 3 x 17; full
    (the changes of geometry join); then, at the full geometry, the single launch of small batches carries the flat tail
    (TQ_PREV_FLAT inside tq_minibatch_kernel) and a two-launch step runs the rows-of-16 tail first."""
    N, F = 5, 24
    d, o, eng = setup(2, dict(N=N, F=F), perturb=0.3)

    def flat(e):
        e.small_full_max_units = 0

    def small(e):
        e.small_full_max_units = 10240

    def route(want, nb=N, fb=F):
        def post(e):
            assert e._route(nb, fb, None) == want
        return post

    full = lambda pre, want: dict(nd=None, fd=None, pre=pre, post=route(want))
    plan = [full(flat, "overlapped"), dict(_subs(N, F, 3, 17, 1)[0], post=route("one_launch", 3, 17)), full(flat, "overlapped"),
            full(small, "one_launch"), full(flat, "overlapped"), full(flat, "overlapped")]
    found = _carried(eng, plan)
    pend = lr0_sequence(eng, o, plan, "flat layout")
    assert pend == [True] * 6 and found == [False, False, False, True, True, True]


@pytest.mark.parametrize("K,offsets", [(3, "hist"), (1, None)], ids=["K3_hist", "K1_one_offset"])
def test_minibatches_of_20_units_per_workgroup_carry_their_tails(K, offsets, monkeypatch):
    """N = 5, F = 24, minibatches 3 x 21 = 63 units with 20 units per workgroup (forced, as
    test_single_launch_minibatch_kernel_20_units_per_workgroup does): five launches, each carrying the rows-of-20 tail of the
    one before, the lazy clock running throughout."""
    monkeypatch.setenv("TAPQIR_AMD_MB_UNITS", "20")
    N, F = 5, 24
    d, o, eng = setup(K, dict(N=N, F=F, **({} if offsets is None else {"offsets": offsets})), perturb=0.3)
    assert eng._route(3, 21, None) == "one_launch" and (eng.O == 1) == (offsets is None)
    plan = _subs(N, F, 3, 21, 5)
    for e in plan:
        e["post"] = lambda eng: None if eng._stale and eng._tail_args.tail_kind == _lib.TAIL_ROWS16 else pytest.fail("route")
    found = _carried(eng, plan)
    pend = lr0_sequence(eng, o, plan, "20 units per workgroup K%d" % K)
    assert pend == [True] * 5 and found == [False] + [True] * 4


def test_sharded_steps_with_the_collective_in_flight():
    """N = 3, F = 300, the AOI-sharded sequence with a handle left in flight: the tail of every step (after the all-reduce)
    runs inside the split sampling of the next one (TQ_PREV_REDUCED in tq_sample_locals_tail_kernel)."""
    N, F = 3, 300
    d, o, eng = setup(2, dict(N=N, F=F), perturb=0.3)
    eng.il_min_units = 1
    eng.fuse_unit = True
    plan = [dict(nd=None, fd=None, kw=dict(allreduce=lambda g: _Done()),
                 post=lambda e: None if e._pending is not None else pytest.fail("no pending all-reduce")) for _ in range(5)]
    found = _carried(eng, plan)
    pend = lr0_sequence(eng, o, plan, "sharded in flight")
    assert pend == [True] * 5 and found == [False] + [True] * 4
