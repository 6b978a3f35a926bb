"""
The offset-histogram kernels at every length and regime boundary, on the MI355X against the float64 oracle.

A data set read by `glimpse` carries an offset histogram of hundreds to thousands of values; the other GPU tests meet that
path at O = 1, 8, 40 and 65 only.  The launch code branches on O at 8, TQ_MO_MAX_O = 1024 and TQ_OFFTAB_MAX = 2048, and the
LDS tables are filled in strides of 64 and 256 lanes: every test here names the kernel its inputs select (from launch_kb of
tq_ksmogn.hip, tq_ksmogn_crosstalk_log_prob and CosmosEngine._route), asserts the inputs of that decision, and computes the LDS
the launch asks for (helpers.lds_request_bytes) against the limit the runtime reports before it launches anything.

Given-latent cases: the staged calls (test_offset_histograms_host.run_given), ELBO to 1e-5 relative, every gradient rel_err
< 1e-4, the log-likelihood of every combination to 1e-5 of the largest.  Step cases: whole device steps replayed by the oracle
(setup / replay of test_gpu_production_kernels.py, per-element gradient budgets of helpers.assert_gradients_match).
The math itself is checked at the same lengths on the CPU in test_offset_histograms_host.py.

Measured on the MI355X (worst ELBO relative error / worst gradient rel_err per route): see DESIGN.md, "Offset histograms at
every length".
"""

import pytest
import torch

from helpers import (LDS_SLOTS_WAVE, device_lds_limit, gradient_report, grid, lds_request_bytes, make_dataset, oracle_to_engine,
                     read_engine_latents, replay_steps)
from test_gpu_production_kernels import replay, setup
from test_offset_histograms_host import MASKED, PEAKED, WORST, check, drop_pixel_statistics, low_background, run_given

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("gradient_report", "error_report")]
assert gradient_report  # (a fixture: imported for pytest to find it)

GATHERED = 1 << 30  # il_min_units no batch reaches: the tile kernels (16 lanes or a wave per unit), as a gathered minibatch takes
PACKED = 1          # il_min_units every batch reaches: the lane-per-unit kernels on the interleaved layout


@pytest.fixture
def error_report(capsys, request):
    """Prints the figures of the given-latent checks a test ran: ELBO relative error, worst gradient rel_err, ll rel_err."""
    WORST.clear()
    yield
    with capsys.disabled():
        for where, (e, g, fam, ll) in WORST.items():
            print("\noffset histogram %s [%s]: ELBO %.3g  gradient %.3g (%s)  ll %s" % (
                request.node.name, where, e, g, fam, "-" if ll is None else "%.3g" % ll))
    WORST.clear()


def fits(P, K, O, **kw):
    """The launch rule of this file: the request is computed first, and a launch is issued only within the reported limit."""
    need, limit = lds_request_bytes(P, K, O, **kw), device_lds_limit()
    assert need <= limit, "a launch of P = %d, K = %d, O = %d asks for %d B of LDS, the device grants %d" % (P, K, O, need, limit)
    return need


def given(dkw, K, il_min_units, where, **kw):
    o, eng, elbo_o, g_o, lat = run_given(dkw, K, device="cuda:0", il_min_units=il_min_units, **kw)
    check(o, eng, elbo_o, g_o, where)
    return eng, lat


class MinibatchSpy:
    """Counts the calls of tq_cosmos_minibatch_step (the engine takes other launches silently otherwise)."""

    def __init__(self, eng):
        self.calls, self._lib = 0, eng.lib
        eng.lib = self

    def __getattr__(self, n):
        f = getattr(self._lib, n)
        if n != "tq_cosmos_minibatch_step":
            return f

        def counted(*a):
            self.calls += 1
            return f(*a)
        return counted


# ---- gathered batches, 16 lanes per unit: O < 8 -------------------------------------------------------------------------------
@pytest.mark.parametrize("O", [2, 7])
def test_16_lane_kernel_below_eight_offsets(O):
    # tq_ksmogn_kernel<2, false, BWD, 16>: B = 9 < il_min_units, O > 1 (no pixel statistics), O < 8.  One workgroup of 16
    # unit slots, 7 of them dead; the offset table (4 + 4 O floats) behind the 16 tiles.
    fits(14, 2, O)
    eng, _ = given(dict(N=3, F=3, offsets=grid(O)), 2, GATHERED, "16-lane O=%d" % O)
    assert eng.O == O < 8 and eng.pixstats is None and eng.Nt * eng.F * eng.C == 9 < eng.il_min_units


def test_16_lane_kernel_one_offset_without_pixel_statistics():
    # tq_ksmogn_kernel<2, false, BWD, 16> at O = 1: launch_k takes the histogram form where a caller passes no pixel statistics,
    # and that form builds its table -- 4 extrema + one entry -- at O = 1 as well.  The request used to count a table from O = 2
    # on and left those 8 floats outside it; it now asks for them (tq_tile16_lds_floats, histogram_form).
    assert fits(14, 2, 1, no_pixstats=True) == fits(14, 2, 1) + 32
    eng, _ = given(dict(N=3, F=3), 2, GATHERED, "16-lane O=1, no pixel statistics", prepare=drop_pixel_statistics)
    assert eng.O == 1 and eng.pixstats is None and 9 < eng.il_min_units


# ---- gathered batches, a wave per unit: O >= 8 --------------------------------------------------------------------------------
@pytest.mark.parametrize("K,O", [(2, 8), (2, 65), (2, 257), (2, 2048), (2, 2049), (4, 2049)])
def test_wave_per_unit_kernel(K, O):
    # tq_ksmogn_kernel<K, false, BWD, 64>: B = 9 < il_min_units, O >= 8.  Three workgroups of 4 units, the last with one live.
    # O = 8: the first length of this form; 65: one lane past the 64-stride of the extrema pass; 257: one past the 256-stride
    # of the fill; 2048: the last length with the table in LDS; 2049: the first that reads global memory (s_off == nullptr).
    fits(14, K, O, slots=LDS_SLOTS_WAVE)
    eng, _ = given(dict(N=3, F=3, offsets=grid(O)), K, GATHERED, "wave-per-unit K=%d O=%d" % (K, O))
    assert eng.O == O >= 8 and eng.K == K and eng.Nt * eng.F * eng.C == 9 < eng.il_min_units


# ---- contiguous batches: the packed histogram kernels -------------------------------------------------------------------------
PACKED_CASES = [
    # id, K, P, offsets: 5 x 15 = 75 units = two waves, the second with 11 live lanes
    ("K2_P14_O2", 2, 14, grid(2)),
    ("K2_P14_O257", 2, 14, grid(257)),           # the table fill `o += 256` takes a second pass
    ("K2_P14_O1024", 2, 14, grid(1024)),         # TQ_MO_MAX_O: the whole of s_tab
    ("K1_P14_O257", 1, 14, grid(257)),
    ("K1_P14_O1024", 1, 14, grid(1024)),
    ("K3_P14_O257", 3, 14, grid(257)),           # K >= 3: tq_ksmogn_il2m_wide_kernel
    ("K3_P14_O2", 3, 14, grid(2)),
    ("K2_P20_O257", 2, 20, grid(257)),
    ("K2_P20_O2", 2, 20, grid(2)),
    ("K2_P14_O257_peaked", 2, 14, grid(257, **PEAKED)),   # log2(w_max / w_min) > 40: the non-factored form (wfac false)
    ("K2_P14_O257_masked", 2, 14, grid(257, **MASKED)),   # offsets above the dimmest pixels: the scalar routine of the pair
]


@pytest.mark.parametrize("name,K,P,offsets", PACKED_CASES, ids=[c[0] for c in PACKED_CASES])
def test_packed_histogram_kernel(name, K, P, offsets):
    # tq_ksmogn_il2m_kernel<K> (K <= 2) / tq_ksmogn_il2m_wide_kernel<K> (K >= 3): contiguous full batch, interleaved images,
    # B = 75 >= il_min_units, no pixel statistics (O > 1), P even, O <= 1024.  Static LDS only (s_tab).
    dkw = dict(N=5, F=15, P=P, offsets=offsets)
    lo = float(make_dataset(K=K, **dkw).images.min())
    assert (lo < offsets[3]) == name.endswith("masked"), (lo, offsets)
    eng, _ = given(dkw, K, PACKED, "packed " + name)
    assert eng.images_il is not None and eng.pixstats is None and eng.P % 2 == 0 and 1 < eng.O == offsets[1] <= 1024
    assert eng.Nt * eng.F * eng.C == 75 >= eng.il_min_units
    lw = eng.offset_logits.double().cpu() / torch.log(torch.tensor(2.0, dtype=torch.float64))
    assert (float(lw.max() - lw.min()) > 40.0) == name.endswith("peaked")


# ---- contiguous batches the packed kernel does not take -----------------------------------------------------------------------
@pytest.mark.parametrize("K,P,O", [(2, 14, 1025), (2, 9, 40), (2, 15, 40)], ids=["P14_O1025", "P9_O40", "P15_O40"])
def test_lane_per_unit_kernel_beyond_the_packed_form(K, P, O):
    # tq_ksmogn_il_kernel<K, false, BWD>: contiguous full batch of 75 >= il_min_units units on the interleaved layout with
    # O = 1025 > TQ_MO_MAX_O at even P, or odd P (npix no multiple of 4: the padded last float4 of a tile).
    eng, _ = given(dict(N=5, F=15, P=P, offsets=grid(O)), K, PACKED, "il P=%d O=%d" % (P, O))
    assert eng.images_il is not None and eng.O == O > 1 and (eng.O > 1024 or eng.P % 2 == 1)
    assert eng.Nt * eng.F * eng.C == 75 >= eng.il_min_units


# ---- the single-launch minibatch step -----------------------------------------------------------------------------------------
def minibatch_case(K, P, O, fb, units, monkeypatch, steps=3, F=24):
    """nb = 1 of N = 2, fb of F frames through tq_cosmos_minibatch_step, replayed by the oracle."""
    monkeypatch.setenv("TAPQIR_AMD_MB_UNITS", str(units))
    fits(P, K, O, minibatch=True)
    d, o, eng = setup(K, dict(N=2, F=F, P=P, offsets=grid(O)))
    assert eng.O == O and eng.fused_minibatch and eng.lazy_adam and fb * eng.C >= units and eng._route(1, fb, None) == "one_launch"
    spy = MinibatchSpy(eng)
    replay(eng, o, 2, F, steps=steps, nb=1, fb=fb, where="minibatch %d units O=%d" % (units, O))
    assert spy.calls == steps
    eng.join()  # (the pending tail is sized by the same environment variable)
    torch.cuda.synchronize()


@pytest.mark.parametrize("O", [257, 2048, 2049])
def test_minibatch_kernel_16_units_per_workgroup(O, monkeypatch):
    # tq_minibatch_kernel<2, false, 16>: 1 x 17 units = one full workgroup and one with a single live unit (+ the tail
    # workgroup); tq_ksmogn_tile_at<.., 16, 16, false> builds the table (O <= 2048) or reads global memory (2049).
    minibatch_case(2, 14, O, 17, 16, monkeypatch)


@pytest.mark.parametrize("O", [257, 2048, 2049])
def test_minibatch_kernel_20_units_per_workgroup(O, monkeypatch):
    # tq_minibatch_kernel<2, false, 20>: 1 x 21 units = one workgroup of 16 + 4 and one of 1; the wave-per-unit second pass
    # (tq_ksmogn_tile_at<.., 64, 16, true>) reuses the table of the first (TAB_READY), at O = 2049 without one.
    minibatch_case(2, 14, O, 21, 20, monkeypatch)


def test_minibatch_kernel_one_offset_without_pixel_statistics(monkeypatch):
    # tq_minibatch_kernel<2, false, 16> at O = 1 (`one` is false without pixel statistics): the table of one entry, as above.
    monkeypatch.setenv("TAPQIR_AMD_MB_UNITS", "16")
    assert fits(14, 2, 1, minibatch=True, no_pixstats=True) == fits(14, 2, 1, minibatch=True) + 32
    d, o, eng = setup(2, dict(N=2, F=24))
    drop_pixel_statistics(eng)
    assert eng._route(1, 17, None) == "one_launch"
    spy = MinibatchSpy(eng)
    replay(eng, o, 2, 24, steps=2, nb=1, fb=17, where="minibatch 16 units O=1, no pixel statistics")
    assert spy.calls == 2
    eng.join()
    torch.cuda.synchronize()


# ---- crosstalk ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("O", [2, 257])
def test_crosstalk_16_lane_kernel(O):
    # tq_xtalk_kernel<2, BWD>: O > 1 keeps a crosstalk batch off the packed kernel whatever il_min_units says (here: 1).
    eng, _ = given(dict(N=2, F=2, C=2, offsets=grid(O)), 2, PACKED, "crosstalk O=%d" % O, crosstalk=True)
    assert eng.crosstalk and eng.O == O > 1


# ---- background / gain below TQ_FAST_ALPHA with a histogram -------------------------------------------------------------------
def test_low_background_wave_per_unit_kernel():
    # tq_ksmogn_kernel<2, false, BWD, 64> (O = 40 >= 8, B = 9 < il_min_units): a unit is a wave, unit 4 of 9 takes the
    # exact-Binet loop (tq_pixel_loop<.., FAST = false>), the other eight the fast one, in the same launch.
    fits(14, 2, 40, slots=LDS_SLOTS_WAVE)
    eng, lat = given(dict(N=3, F=3, offsets=grid(40)), 2, GATHERED, "low background, wave-per-unit", low=([(1, 1, 0)], 20.0))
    low_background(lat, [4], 1)
    assert eng.O == 40 and 9 < eng.il_min_units


def test_low_background_packed_kernel():
    # tq_ksmogn_il2m_kernel<2> (75 units, il_min_units = 1, P = 14, O = 40): unit 3 makes wave 0 take fast = false for all
    # its 64 lanes, wave 1 (units 64..74) stays fast.
    eng, lat = given(dict(N=5, F=15, offsets=grid(40)), 2, PACKED, "low background, packed", low=([(0, 3, 0)], 20.0))
    low_background(lat, [3], 64)
    assert eng.images_il is not None and eng.O == 40 and eng.P == 14 and 75 >= eng.il_min_units


def test_low_background_packed_kernel_masked_offsets():
    # the same wave through the scalar routine of a pair with masked offsets: tq_pix_multi_offset<M, BWD, false>.  (Samples up
    # to 330 with the weights kept about 90 -- sigma 20, not MASKED's 60: the initial backgrounds are the data mean less the
    # offset mean, and a higher offset mean would put further units below TQ_FAST_ALPHA.)
    dkw = dict(N=5, F=15, offsets=grid(65, hi=330.0, sigma=20.0))
    assert float(make_dataset(K=2, **dkw).images.min()) < 330.0
    eng, lat = given(dkw, 2, PACKED, "low background, packed, masked", low=([(0, 3, 0)], 20.0))
    low_background(lat, [3], 64)
    assert eng.images_il is not None and eng.O == 65 and 75 >= eng.il_min_units


@pytest.mark.parametrize("units,fb", [(16, 17), (20, 21)])
def test_low_background_minibatch_kernel(units, fb, monkeypatch):
    # tq_minibatch_kernel<2, false, units> at O = 40: the guide of frame 5 of AOI 1 draws its background about 20 (b_loc),
    # so unit 5 of the batch -- second wave of the first workgroup, with units 4, 6, 7 -- is below TQ_FAST_ALPHA in every step.
    monkeypatch.setenv("TAPQIR_AMD_MB_UNITS", str(units))
    fits(14, 2, 40, minibatch=True)
    d, o, eng = setup(2, dict(N=2, F=24, offsets=grid(40)))
    o.params["b_loc"].data[1, 5, 0] = float(torch.log(torch.tensor(20.0)).float())
    oracle_to_engine(o, eng)
    assert eng.O == 40 and eng._route(1, fb, None) == "one_launch"
    spy = MinibatchSpy(eng)
    nd, fd = torch.tensor([1]), torch.arange(fb)

    def step(eng, it):
        eng.step(nd, fd)
        torch.cuda.synchronize()
        low_background(read_engine_latents(eng, 1, fb), [5], 4)
        return nd, fd

    replay_steps(eng, o, step, steps=3, where="low background, minibatch %d units" % units)
    assert spy.calls == 3
    eng.join()
    torch.cuda.synchronize()


def test_low_background_crosstalk_16_lane_kernel():
    # tq_xtalk_kernel<2, BWD> at O = 40: 6 AOI-frames, 4 per wave; AOI-frame 1 has background 20 in both channels, the second
    # wave (AOI-frames 4, 5) is entirely above.
    eng, lat = given(dict(N=2, F=3, C=2, offsets=grid(40)), 2, PACKED, "low background, crosstalk", crosstalk=True,
                     low=([(0, 1, 0), (0, 1, 1)], 20.0))
    low_background(lat, [2, 3], 8)
    assert eng.crosstalk and eng.O == 40


def test_low_background_packed_crosstalk_kernel():
    # tq_xtalk_il_kernel<BWD> (K = 2, O = 1 with pixel statistics, P even, 75 AOI-frames >= il_min_units): AOI-frame 3 has
    # background 20 in both channels, which takes its whole wave out through the early scalar exit; wave 1 stays packed.
    eng, lat = given(dict(N=5, F=15, C=2), 2, PACKED, "low background, packed crosstalk", crosstalk=True,
                     low=([(0, 3, 0), (0, 3, 1)], 20.0))
    low_background(lat, [6, 7], 128)
    assert eng.crosstalk and eng.O == 1 and eng.pixstats is not None and eng.images_il is not None and eng.P % 2 == 0
    assert eng.Nt * eng.F == 75 >= eng.il_min_units


# ---- the largest tiles and the largest LDS requests ---------------------------------------------------------------------------
@pytest.mark.parametrize("O", [1, 8])
@pytest.mark.parametrize("il_min_units", [GATHERED, PACKED], ids=["gathered", "contiguous"])
def test_tiles_of_32_pixels(O, il_min_units):
    # P = TQ_MAX_P = 32, K = 2, 4 units.  gathered: tq_ksmogn_kernel<2, ONE, BWD, 16> at O = 1 -- 74752 B of dynamic LDS, more
    # than 64 KB without any table -- and the wave-per-unit form at O = 8 (4 slots).  contiguous: tq_ksmogn_il_kernel<2, true>
    # at O = 1 (the packed single-offset kernel is built for P = 14 and 20), tq_ksmogn_il2m_kernel<2> at O = 8.
    need = fits(32, 2, O, slots=LDS_SLOTS_WAVE if O >= 8 else 16)
    assert O != 1 or need == 74752 > 65536
    dkw = dict(N=2, F=2, P=32) if O == 1 else dict(N=2, F=2, P=32, offsets=grid(O))
    eng, _ = given(dkw, 2, il_min_units, "P=32 O=%d %s" % (O, "gathered" if il_min_units > 1 else "contiguous"))
    assert eng.P == 32 and eng.O == O and (eng.pixstats is not None) == (O == 1) and (4 >= eng.il_min_units) == (il_min_units == PACKED)


@pytest.mark.parametrize("K,P,steps", [(3, 14, 2), (4, 20, 1)], ids=["K3_P14", "K4_P20"])
def test_minibatch_kernel_largest_lds_requests(K, P, steps, monkeypatch):
    # tq_minibatch_kernel<K, false, 16> at O = 2048, the longest table: 67648 B (K = 3, P = 14) and 84032 B (K = 4, P = 20)
    # of LDS per workgroup, both beyond 64 KB; the device reports 163840 B.  1 x 16 units: one full workgroup.
    # The dense oracle at K = 4, P = 20, O = 2048 takes seconds per step: one step there, two at K = 3.
    need = fits(P, K, 2048, minibatch=True)
    assert need == {(3, 14): 67648, (4, 20): 84032}[(K, P)] > 65536
    minibatch_case(K, P, 2048, 16, 16, monkeypatch, steps=steps, F=16 + 4)


def test_largest_admitted_request_is_within_the_device_limit():
    """K = 4, P = 32, O = 2048 in the minibatch kernel, 124992 B, is the most any admitted shape asks for: no launch of the
    library can ask for more than this device grants."""
    assert lds_request_bytes(32, 4, 2048, minibatch=True, draws=True) == 124992 <= device_lds_limit()
