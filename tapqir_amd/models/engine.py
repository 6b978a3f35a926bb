"""
Device-side state of a cosmos fit and the launcher of the HIP step.

Owns what the reference keeps in Pyro's global param store + ``pyro.optim.Adam`` state
(tapqir/models/model.py:153-186): the flat unconstrained parameter buffer, its gradient and the
two Adam moments, the dataset resident in HBM (the reference re-uploads every minibatch,
tapqir/utils/dataset.py:140-151) and the step workspace.  All arithmetic happens in
``libtapqir_hip.so`` (include/tapqir_hip.h); torch is used for allocation, streams and the
``torch.distributed`` all-reduce only.
"""

import ctypes as C
import math
import os

import torch

from tapqir_amd import _lib
from tapqir_amd.exceptions import HipExtensionError
from tapqir_amd.models.layout import ParamLayout

DEFAULT_PRIORS = {  # tapqir/models/cosmos.py:55-64
    "background_mean_std": 1000.0, "background_std_std": 100.0, "lamda_rate": 1.0, "height_std": 10000.0,
    "width_min": 0.75, "width_max": 2.25, "proximity_rate": 1.0, "gain_std": 50.0,
}


# Most keys CosmosEngine.step_subsampled lets a launch walk for the next step's subsample: the sizes of the axes it actually
# subsamples, added up (an axis taken whole draws nothing).  The library draws up to _lib.SUBSAMPLE_MAX = 65536 per axis, but
# the draw is one workgroup walking every key, and where it outlasts the workers of the launch the step is slower than one on
# indices the host supplies.  400 + 4000 keys (the shard of BASELINE config c3) is the largest draw measured that is not slower;
# 16384 is slower ("Subsamples beyond 2048 AOIs or frames").  Every data set within 2048 x 2048 is below it.
DEVICE_SUBSAMPLE_MAX = 4400


def merge_offsets(samples, weights):
    """Offset samples with equal value are one mixture component: sum_o w_o f(D - d_o) is
    unchanged when equal d_o are merged (simulate.py:92-103 stores 3 identical samples)."""
    s = samples.detach().double().cpu()
    w = weights.detach().double().cpu()
    uniq, inv = torch.unique(s, return_inverse=True)
    wsum = torch.zeros_like(uniq).index_add_(0, inv, w)
    eps = torch.finfo(torch.float64).eps
    logits = torch.log(wsum.clamp(eps, 1 - eps)) if len(uniq) > 1 else torch.log(wsum.clamp(min=eps))
    return uniq.float(), logits.float()


class CosmosEngine:
    # what the library's launch sequence supports (tests/helpers.py derives a checker of the kernels' inline math that
    # runs the same bodies in plain host loops and switches these off)
    pipelined_tail = True      # tq_cosmos_step_overlapped: the tail of step t inside the sampling launch of step t+1
    split_sampling = True      # tq_cosmos_sample_locals_range: sampling split around an in-flight all-reduce
    lazy_adam_default = True   # tq_cosmos_adam_catchup
    fused_minibatch = True     # tq_cosmos_minibatch_step: a minibatch step (or a small full batch) as ONE launch

    def __init__(self, data, K=2, priors=None, device="cuda", eps=None, seed=0, n_offset=0, Nt_global=None,
                 crosstalk=False, hbm_budget=None):
        """``hbm_budget`` (bytes; default: the TAPQIR_AMD_HBM_BUDGET environment variable, else unlimited): device memory the
        IMAGES may take.  A data set whose resident form (the images and their interleaved copy) is larger is STREAMED: the
        images stay in page-locked host memory and every step brings the AOIs it needs through two device windows, group by
        group (the reference fetches every minibatch from host memory, tapqir/utils/dataset.py:140-151); parameters, optimiser
        state and the 12 B per unit of data statistics stay resident (section "streamed data sets" of DESIGN.md)."""
        self.device = torch.device(device)
        self.lib = self._open_library()
        lib = self.lib
        # With one dye and one channel the crosstalk model IS cosmos (alpha = [[1]] is a one-component Dirichlet:
        # constant draw, zero log-density, no gradient; the reference's smoke test runs this case,
        # test/test_tapqir.py:27-30): the cosmos kernels run and alpha_mean / alpha_size are inert parameters.
        nch = int(data.images.shape[2])
        self.crosstalk = bool(crosstalk) and nch > 1
        self.layout_crosstalk = bool(crosstalk)
        if self.crosstalk and (nch != 2 or int(K) > 2):
            raise ValueError("the crosstalk model is implemented for Q = C <= 2 dyes/channels and K <= 2 "
                             "(2^(K Q) joint spot-presence combinations; tapqir/models/crosstalk.py is experimental "
                             "upstream and indexes dyes and channels alike)")
        self.K = int(K)
        self.priors = dict(DEFAULT_PRIORS if priors is None else priors)
        self.eps = float(torch.finfo(torch.float32).eps if eps is None else eps)
        self.seed = int(seed)
        Nt, F, Cc, P = data.images.shape[:4]
        self.Nt, self.F, self.C, self.P = int(Nt), int(F), int(Cc), int(P)
        self.Nt_global = int(Nt_global) if Nt_global else self.Nt
        self.n_offset = int(n_offset)
        dev = self.device
        f32 = torch.float32
        if hbm_budget is None and os.environ.get("TAPQIR_AMD_HBM_BUDGET"):
            hbm_budget = int(float(os.environ["TAPQIR_AMD_HBM_BUDGET"]))
        img_bytes = 4 * data.images.numel()
        self.streamed = bool(hbm_budget) and 2 * img_bytes > hbm_budget and self.device.type == "cuda"
        if self.streamed:
            if self.crosstalk:
                raise ValueError("streaming of data sets larger than the device memory is implemented for the cosmos model")
            self._init_windows(data, int(hbm_budget))
        else:
            self.images = data.images.to(dev, f32).contiguous()
        self.xy = data.xy.to(dev, f32).contiguous()
        self.is_ontarget = data.is_ontarget.to(dev, torch.uint8).contiguous()
        self.mask = data.mask.to(dev, torch.uint8).contiguous()
        # the kernels take NULL for "no AOI is masked" (the default, dataset.py:63-65) and then skip the per-unit mask load
        self._mask_arg = self.mask if not bool(data.mask.all()) else None
        # tile-interleaved copy for the contiguous-batch pixel kernel (include/tapqir_hip.h); built by the
        # library so that any C caller gets the same layout
        self.images_il = None if self.streamed else self._interleaved_images()
        off_s, off_l = merge_offsets(data.offset.samples, data.offset.weights)
        self.offset_samples, self.offset_logits = off_s.to(dev), off_l.to(dev)
        self.O = int(off_s.numel())
        # per-unit data statistics of the single-offset formulation (sum v, sum ln v, #masked pixels)
        self.pixstats = None
        if self.O == 1:
            U = self.Nt * self.F * self.C
            self.pixstats = torch.empty(3 * U, dtype=f32, device=dev)
            if self.streamed:
                self._image_stats_streamed()
            else:
                self._image_stats(U)
        self.layout = ParamLayout(self.Nt, self.F, self.C, self.K, self.P, self.eps, crosstalk=self.layout_crosstalk)
        n = self.layout.total
        self._params = torch.zeros(n, dtype=f32, device=dev)
        self.grad = torch.zeros(n, dtype=f32, device=dev)
        self._exp_avg = torch.zeros(n, dtype=f32, device=dev)
        self._exp_avg_sq = torch.zeros(n, dtype=f32, device=dev)
        # lazy Adam of minibatch steps (include/tapqir_hip.h: tq_cosmos_adam_catchup): per-unit clock of the last update;
        # meaningful only while `_stale` (some unit's local parameters lag behind adam_step).  lazy_adam = False (tests):
        # every minibatch step streams the whole buffers through the dense Adam kernel instead
        self.lazy_adam = self.lazy_adam_default
        self._last_step = torch.zeros(self.Nt * self.F * self.C, dtype=torch.int32, device=dev)
        self._stale = False
        self._grad_dirty = False  # `grad` holds gradients no minibatch step has cleared (_open_step)
        gsz, bsz = self.struct_sizes()
        self.globals = torch.zeros(gsz // 4, dtype=f32, device=dev)
        self.gbase = torch.zeros(bsz // 8, dtype=torch.float64, device=dev)
        self._gsum_buf = torch.zeros(_lib.GSUM_LEN, dtype=torch.float64, device=dev)
        self.n_gsum = 3 + 3 * self.C + (self.C * self.C if self.crosstalk else 0)
        self.gsum = self._gsum_buf[: self.n_gsum]  # the part that crosses ranks
        self.elbo_out = torch.zeros(1, dtype=torch.float64, device=dev)
        self._ws_key = None
        self._pending = None  # (args, handle) of a step whose all-reduce is in flight
        self.adam_step = 0
        self.lr, self.betas, self.adam_eps = 0.005, (0.9, 0.999), 1e-8
        # contiguous batches at least this large use the lane-per-unit pixel kernel (64 units per wave):
        # 65536 units = one wave per SIMD of an MI355X
        self.il_min_units = 65536
        # full batches of at most this many units (BASELINE config c1: 5000) take the one-launch step of the minibatches
        # (_route)
        self.small_full_max_units = 10240
        # full-batch single-GPU steps leave their single-workgroup tail pending and run it inside the next step's
        # sampling launch (include/tapqir_hip.h: tq_cosmos_step_overlapped)
        self._tail_args = None  # arguments of the step whose tail is pending
        # form of the stand-alone pixel kernel: always 0, the one wave per tile form is the only one (bench.py reads this)
        self.pixel_mode = 0
        # full-batch steps run the pixel kernel and the per-unit kernel as ONE launch (pixel_mode = TQ_PIXEL_FUSED_UNIT of
        # tq_cosmos_args) wherever the step qualifies (_fusable); TAPQIR_AMD_FUSE_UNIT=0 keeps the two launches for A/B timing
        fu = os.environ.get("TAPQIR_AMD_FUSE_UNIT", "1")
        if fu not in ("0", "1"):
            raise ValueError(f"TAPQIR_AMD_FUSE_UNIT={fu!r}: expected 0 or 1")
        self.fuse_unit = fu != "0"
        # the fused launch can split its last tiles by rows over four waves each, dispatched first, so that a nearly empty
        # last round of tiles goes (tq_cosmos_args.pu_split): -1 = the library's rule (tq_cosmos_pu_split_auto), 0 = never,
        # n = the last n tiles.  TAPQIR_AMD_PU_SPLIT=auto|0|n fixes it for A/B timing.
        ps = os.environ.get("TAPQIR_AMD_PU_SPLIT", "auto")
        self.pu_split = -1 if ps == "auto" else int(ps)
        self._pu_scratch, self._pu_scratch_tiles = None, 0
        # the fused launch streams the tiles as 16-bit integers where the images are integers in [0, 65535] (tq_cosmos_args.
        # images_il16, built when a step first takes the fused route: _tile16); TAPQIR_AMD_TILE16=auto|0 fixes it for A/B timing
        t16 = os.environ.get("TAPQIR_AMD_TILE16", "auto")
        if t16 not in ("auto", "0"):
            raise ValueError(f"TAPQIR_AMD_TILE16={t16!r}: expected auto or 0")
        self.tile16 = t16 != "0"
        self.images_il16, self._tile16_tried = None, False
        self._sync = torch.zeros(_lib.SYNC_WORDS, dtype=torch.int32, device=dev)  # tickets, flags; diagnostic stamps of a TQ_MB_STAMPS build
        self._sync_value = 0

    # -- the library --------------------------------------------------------------------------------
    def _open_library(self):
        if self.device.type != "cuda":
            raise HipExtensionError(
                "the cosmos SVI step only runs on an AMD GPU through libtapqir_hip.so "
                f"(device={str(self.device)!r} requested); there is no CPU path")
        return _lib.load()

    def struct_sizes(self):
        """(bytes of TqGlobals, bytes of TqGlobalBase)."""
        return int(self.lib.tq_globals_size()), int(self.lib.tq_gbase_size())

    def _interleaved_images(self):
        """Tile-interleaved copy for the contiguous-batch pixel kernel (include/tapqir_hip.h); built by the library so
        that any C caller gets the same layout.  cosmos: one (P, P) tile per unit (n, f, c); crosstalk: one (C, P, P)
        tile per AOI-frame (n, f)."""
        tiles = self.Nt * self.F * (1 if self.crosstalk else self.C)
        npix = self.P * self.P * (self.C if self.crosstalk else 1)
        out = torch.empty(int(self.lib.tq_interleaved_floats_n(tiles, npix)), dtype=torch.float32, device=self.device)
        _lib.check(self.lib.tq_images_interleave_n(_lib.ptr(self.images), _lib.ptr(out), tiles, npix, self._stream()),
                   "tq_images_interleave_n")
        return out

    def _tile16(self):
        """The 16-bit interleaved copy of the tiles for the fused launch (tq_cosmos_args.images_il16), built by the library
        when a step first takes that route and kept only if every pixel is an integer in [0, 65535] (one read-back of the
        library's flag); None otherwise, with TAPQIR_AMD_TILE16=0, and for engines without the fp32 interleaved copy, which
        stays resident beside it (2 more bytes per pixel of device memory)."""
        if self._tile16_tried or not self.tile16:
            return self.images_il16
        self._tile16_tried = True
        if self.images_il is None or self.crosstalk:
            return None
        tiles, npix = self.Nt * self.F * self.C, self.P * self.P
        out = torch.empty(int(self.lib.tq_interleaved_u16_n(tiles, npix)), dtype=torch.uint16, device=self.device)
        inexact = torch.zeros(1, dtype=torch.int32, device=self.device)
        _lib.check(self.lib.tq_images_interleave_u16_n(_lib.ptr(self.images), _lib.ptr(out), tiles, npix, _lib.ptr(inexact),
                                                       self._stream()), "tq_images_interleave_u16_n")
        if int(inexact.item()) == 0:
            self.images_il16 = out
        return self.images_il16

    def _image_stats(self, U):
        _lib.check(self.lib.tq_image_stats(_lib.ptr(self.images), _lib.ptr(self.offset_samples), _lib.ptr(self.pixstats),
                                           U, self.P, self._stream()), "tq_image_stats")

    def _blk_floats(self, B):
        return int(self.lib.tq_cosmos_blk_floats(self.Nt, self.F, self.C, int(self.crosstalk), B))

    def _run_snr_chi2(self, a):
        _lib.check(self.lib.tq_snr_chi2(C.byref(a), self._stream()), "tq_snr_chi2")

    def snr_chi2(self, offset_mean, offset_var):
        """Signal-to-noise ratio of every spot ``(K, Nt, F, Q)`` and chi2 of the fitted image ``(Nt, F, Q)`` at the
        posterior means of the variational parameters (tapqir/utils/stats.py:29-86, 166-182), computed where the images
        are: one kernel over all units instead of the reference's host loop over AOIs."""
        cp = self.layout.constrained(self.params, {"h_loc", "w_mean", "x_mean", "y_mean", "b_loc", "gain_loc"})
        f32 = torch.float32
        U = self.Nt * self.F * self.C
        flat = lambda t: t.detach().to(f32).reshape(self.K, U).contiguous()
        h, w, x, y = flat(cp["h_loc"]), flat(cp["w_mean"]), flat(cp["x_mean"]), flat(cp["y_mean"])
        b = cp["b_loc"].detach().to(f32).reshape(U).contiguous()
        snr = torch.empty(self.K, U, dtype=f32, device=self.device)
        chi2 = torch.empty(U, dtype=f32, device=self.device)
        gain = float(cp["gain_loc"])
        p = _lib.ptr

        def launch(images, xy, hh, ww, xx, yy, bb, snr_o, chi2_o, n_units):
            a = _lib.SnrArgs()
            a.images, a.xy = p(images), p(xy)
            a.height, a.width, a.x, a.y, a.background = p(hh), p(ww), p(xx), p(yy), p(bb)
            a.snr, a.chi2 = p(snr_o), p(chi2_o)
            a.U, a.P, a.K = n_units, self.P, self.K
            a.gain, a.offset_mean, a.offset_var = gain, float(offset_mean), float(offset_var)
            self._run_snr_chi2(a)

        if not self.streamed:
            launch(self.images, self.xy, h, w, x, y, b, snr, chi2, U)
        else:  # window by window (whole AOIs): the same kernel on slices of every array
            fc = self.F * self.C
            xy2 = self.xy.reshape(U, 2)
            for aois in self._groups(None):  # (upload, then wait: one window in flight -- not _windows, which prefetches)
                wi, n0, n = self._upload_group(aois), int(aois[0]), aois.numel()
                torch.cuda.current_stream(self.device).wait_event(self._win_ready[wi])
                u0, u1 = n0 * fc, (n0 + n) * fc
                parts = [t[:, u0:u1].contiguous() for t in (h, w, x, y)]
                snr_g = torch.empty(self.K, u1 - u0, dtype=f32, device=self.device)
                chi2_g = torch.empty(u1 - u0, dtype=f32, device=self.device)
                launch(self._win[wi], xy2[u0:u1].contiguous(), *parts, b[u0:u1].contiguous(), snr_g, chi2_g, u1 - u0)
                snr[:, u0:u1] = snr_g
                chi2[u0:u1] = chi2_g
                self._release_window(wi)
        return snr.view(self.K, self.Nt, self.F, self.C), chi2.view(self.Nt, self.F, self.C)

    def run_probs(self, a):
        _lib.check(self.lib.tq_cosmos_probs(C.byref(a), self._stream()), "tq_cosmos_probs")

    # -- streamed data sets (images larger than the device memory they may take) --------------------------
    def _init_windows(self, data, budget):
        """Images in page-locked host memory; two device windows of W whole AOIs each (all frames of an AOI travel together:
        the per-AOI sites need every frame of the batch, and an AOI's F C P P floats are contiguous on the host)."""
        f32 = torch.float32
        self.images = None
        self.images_host = data.images.to("cpu", f32).contiguous().pin_memory()
        Nt = self.images_host.shape[0]
        per_aoi = 4 * self.images_host[0].numel()
        self.window_aois = int(max(1, min(Nt, budget // (2 * per_aoi))))
        shape = (self.window_aois,) + tuple(self.images_host.shape[1:])
        self._win = [torch.empty(shape, dtype=f32, device=self.device) for _ in range(2)]
        self._win_free = [None, None]  # event after the last launch that reads the window
        self._win_ready = [torch.cuda.Event(), torch.cuda.Event()]
        self._copy_stream = torch.cuda.Stream(self.device)
        self._win_count = 0

    def _upload_group(self, aois):
        """Bring the AOIs `aois` (host int64 tensor, in batch order) into the next window on the copy stream; returns the
        window index.  Runs of consecutive AOIs are one copy."""
        w = self._win_count % 2
        self._win_count += 1
        win = self._win[w]
        with torch.cuda.stream(self._copy_stream):
            if self._win_free[w] is not None:
                self._copy_stream.wait_event(self._win_free[w])  # the kernels that read this window two groups ago are done
            idx = aois.tolist()
            j = 0
            while j < len(idx):
                k = j
                while k + 1 < len(idx) and idx[k + 1] == idx[k] + 1:
                    k += 1
                win[j:k + 1].copy_(self.images_host[idx[j]:idx[k] + 1], non_blocking=True)
                j = k + 1
            self._win_ready[w].record(self._copy_stream)
        return w

    def _groups(self, ndx):
        aois = torch.arange(self.Nt) if ndx is None else ndx.detach().to("cpu", torch.int64).reshape(-1)
        return [aois[i:i + self.window_aois] for i in range(0, aois.numel(), self.window_aois)]

    def _release_window(self, w):
        """The launches that read window `w` have been issued on the current stream: the copy stream may refill it after them."""
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(self.device))
        self._win_free[w] = ev

    def _windows(self, groups):
        """Yields (window index, AOIs) for every group, the window filled as far as the current stream is concerned (it
        waits for the upload) and the NEXT group's upload already issued, so that it travels while this group computes; the
        window is released when the consumer comes back for the next group."""
        cur = torch.cuda.current_stream(self.device)
        nxt = self._upload_group(groups[0])
        for g, aois in enumerate(groups):
            w = nxt
            cur.wait_event(self._win_ready[w])
            if g + 1 < len(groups):
                nxt = self._upload_group(groups[g + 1])
            yield w, aois
            self._release_window(w)

    def _image_stats_streamed(self):
        U, fc = self.Nt * self.F * self.C, self.F * self.C
        for w, aois in self._windows(self._groups(None)):
            n0, n = int(aois[0]), aois.numel()
            tmp = torch.empty(3, n * fc, dtype=torch.float32, device=self.device)
            _lib.check(self.lib.tq_image_stats(_lib.ptr(self._win[w]), _lib.ptr(self.offset_samples), _lib.ptr(tmp), n * fc, self.P,
                                               self._stream()), "tq_image_stats")
            self.pixstats.view(3, U)[:, n0 * fc:(n0 + n) * fc] = tmp

    def _step_streamed(self, ndx, fdx):
        """One SVI step of a streamed data set: the step's AOIs in groups of at most `window_aois`; per group the staged
        launches of a gathered batch (lazy-Adam catch-up for minibatches, local sampling, likelihood + per-unit + per-AOI
        terms with the Adam of the local parameters fused in) on the window the copy stream has filled meanwhile; the
        cross-unit sums of the groups are added and ONE tail (global sites, ELBO, Adam of the per-AOI / global parameters)
        closes the step.  Draws are keyed by the global unit index, so the step is the resident step up to the order in
        which the groups' sums are added."""
        self._finish_pending()
        self._finish_tail()
        groups = self._groups(ndx)
        nb_total = sum(g.numel() for g in groups)
        fb = self.F if fdx is None else int(fdx.numel())
        minibatch = nb_total < self.Nt or fb < self.F
        self._workspace(min(self.window_aois, nb_total), fb)  # (a new workspace joins first: before the lazy clock is started)
        ws_key = self._ws_key
        fdx_dev = None if fdx is None else self._index_to_device(fdx, 1)
        gtot = torch.zeros_like(self.gsum)
        a = None
        for w, aois in self._windows(groups):
            first = a is None
            nd = aois.to(self.device, torch.int32)
            a = self.make_args(nd, fdx_dev, draw_globals=True, _for_step=True, _ws=ws_key)
            a.images, a.images_il, a.images_by_slot = _lib.ptr(self._win[w]), None, 1
            a.scale_n = self.Nt_global / self._nb_global(nb_total)
            a.scale = a.scale_n * self.F / fb
            a.zero_grad = int(minibatch)  # (of the step, not of the group)
            lazy = self._open_step(a)
            if first:
                self.call("cosmos_sample_globals", a)
            if lazy:
                self._adam_catchup(a, 0)
            self.call("cosmos_sample_locals", a)
            self.call("cosmos_elbo_grads", a)
            gtot += self.gsum
        self.gsum.copy_(gtot)
        self._tail_reduced(a, None)
        self.adam_step += 1

    # -- parameter / moment buffers ---------------------------------------------------------------
    # Reading them from outside the step completes deferred work first: the pending tail of a pipelined step and the
    # zero-gradient Adam steps that lazy minibatch steps still owe to the units outside their minibatches.
    @property
    def params(self):
        self.join()
        return self._params

    @property
    def exp_avg(self):
        self.join()
        return self._exp_avg

    @property
    def exp_avg_sq(self):
        self.join()
        return self._exp_avg_sq

    def _catch_up_all(self):
        """Bring the local parameters and moments of every unit to `adam_step` (lazy Adam)."""
        if self._stale:
            self._stale = False
            a = self._core_args()  # all the replay reads, with the full geometry and the step count (no join, no workspace)
            a.nb, a.fb = self.Nt, self.F
            a.step = self.adam_step
            self._adam_catchup(a, 1)

    def _adam_catchup(self, a, all_units):
        _lib.check(self.lib.tq_cosmos_adam_catchup(C.byref(a), all_units, self._stream()), "tq_cosmos_adam_catchup")

    def reset_adam_clock(self, step=0):
        """The buffers were (re)written from outside (initialisation, checkpoint): everything is current at `step`."""
        self.join()
        self.adam_step = int(step)
        self._stale = False
        # the ticket / flag words of the single-launch minibatch step start from a known state again: a launch that timed
        # out waiting for its flag (the kernel then leaves a NaN loss, which brings Model.run here through its checkpoint
        # reload) must not leave a ticket counter that no later launch can start from
        self._sync.zero_()
        self._sync_value = 0
        if self._pu_scratch is not None:
            self._pu_scratch[:self._pu_scratch_tiles].zero_()  # the tickets of the split tiles (four per tile and launch)
        if "_sub" in self.__dict__:
            self._sub["ready"] = None  # a device-drawn subsample belongs to the step count it was drawn for

    # -- workspace ---------------------------------------------------------------------------------
    def _workspace(self, nb, fb):
        key = (nb, fb)
        if self._ws_key == key:
            return
        self.join()
        K, M = self.K, 1 << self.K
        B = nb * fb * self.C
        dev, f32 = self.device, torch.float32
        self.lat = torch.zeros((1 + 4 * K) * B, dtype=f32, device=dev)
        self.site = torch.zeros(5 * (1 + 4 * K) * B, dtype=f32, device=dev)  # TQ_NSITE_STORED rows (tq_site.h)
        self.pix = torch.zeros((M + 2 + 4 * K + (1 + self.C if self.crosstalk else 0)) * B, dtype=f32, device=dev)
        self.aoi_part = torch.zeros(3 * B, dtype=f32, device=dev)
        self.blk_part = torch.zeros(self._blk_floats(B), dtype=f32, device=dev)
        self._ws_key = key

    def _pu_split_tiles(self, nb, fb):
        """Tiles that a fused full-batch launch of this engine splits by rows (tq_cosmos_args.pu_split): the engine's fixed
        count, or the library's rule for the wave slots of the instantiated kernel; 0 where no step can be fused."""
        if not self.pu_split or nb < self.Nt or fb < self.F or not self._fusable():
            return 0
        ntiles = (nb * fb * self.C + 63) // 64
        if self.pu_split > 0:
            return min(self.pu_split, ntiles)
        if "_pu_slots" not in self.__dict__:
            self._pu_slots = int(self.lib.tq_cosmos_pu_slots(self.K, self.P))
        return int(self.lib.tq_cosmos_pu_split_auto(ntiles, self._pu_slots))

    def _pu_split_scratch(self, nb, fb):
        """Tickets and partial sums of the split tiles: grown to what the batch geometry needs, zeroed when allocated (the
        tickets count four per tile and launch and are never reset)."""
        tiles = self._pu_split_tiles(nb, fb)
        if tiles > self._pu_scratch_tiles:
            words = int(self.lib.tq_cosmos_pu_scratch_bytes(tiles)) // 4
            self._pu_scratch = torch.zeros(words, dtype=torch.int32, device=self.device)
            self._pu_scratch_tiles = tiles
        return self._pu_scratch, self._pu_scratch_tiles

    def _index_to_device(self, idx, which):
        """One subsample index vector as a device int32 tensor (see _indices_to_device for the step's fast path)."""
        return idx.to(self.device, torch.int32).contiguous()

    def _indices_to_device(self, ndx, fdx):
        """Subsample indices of a step as device int32 tensors.  Host tensors (what ``torch.randperm`` gives the caller
        every step) take ONE asynchronous copy: both vectors are written, converted to int32, into a pinned staging
        slot and copied into a persistent device slot of the same ring -- no allocation, no pageable copy (which would
        block the host until the stream has drained) and a few microseconds of host time instead of ~40 per vector,
        which made the host the bottleneck of the default 10 x 512 minibatch step."""
        host = [t is not None and t.device.type == "cpu" for t in (ndx, fdx)]
        if self.device.type != "cuda" or not any(host):
            return (None if ndx is None else self._index_to_device(ndx, 0)), (None if fdx is None else self._index_to_device(fdx, 1))
        pin, pin_np, dev, ev, _ = slot = self._idx_slot()
        pos, out = 0, []
        for t, h in zip((ndx, fdx), host):
            if t is None:
                out.append(None)
            elif h:
                k = t.numel()
                pin_np[pos:pos + k] = t.numpy().reshape(-1)  # int64 -> int32
                out.append((pos, k))
                pos += k
            else:
                out.append(t.to(self.device, torch.int32).contiguous())
        dev[:pos].copy_(pin[:pos], non_blocking=True)
        ev.record()  # on the current stream
        slot[4] = True
        return tuple(dev[o[0]:o[0] + o[1]] if isinstance(o, tuple) else o for o in out)

    def _idx_slot(self):
        """Next slot of the 16-deep ring of pinned + device index buffers ([Nt | F] int32 each)."""
        ring = self.__dict__.get("_idx_ring")
        if ring is None:
            n = self.Nt + self.F
            ring = []
            for _ in range(16):
                pin = torch.empty(n, dtype=torch.int32).pin_memory()
                ring.append([pin, pin.numpy(), torch.empty(n, dtype=torch.int32, device=self.device), torch.cuda.Event(), False])
            self._idx_ring, self._idx_count = ring, 0
        slot = ring[self._idx_count % len(ring)]
        self._idx_count += 1
        if slot[4]:
            slot[3].synchronize()  # the copy that last read this staging slot (16 steps ago) has completed
        return slot

    def draw_subsample(self, nb, fb, generator):
        """``torch.randperm(Nt)[:nb]``, ``torch.randperm(F)[:fb]`` (pyro.plate's subsample, cosmos.py:194-208) drawn straight
        into a pinned staging slot as int32 and copied to the device in ONE asynchronous copy: returns device index
        tensors for ``step`` (None where the whole axis is taken).  Saves the slicing and int64 -> int32 copies of
        ``_indices_to_device`` -- at the default minibatch the host, not the device, bounds ``Model.run``."""
        if self.device.type != "cuda":
            raise RuntimeError("draw_subsample stages through pinned memory: GPU engines only")
        take_n, take_f = nb < self.Nt, fb < self.F
        if not (take_n or take_f):
            return None, None
        pin, _, dev, ev, _ = slot = self._idx_slot()
        Nt, F = self.Nt, self.F
        if take_n:
            torch.randperm(Nt, generator=generator, dtype=torch.int32, out=pin[:Nt])
        if take_f:
            torch.randperm(F, generator=generator, dtype=torch.int32, out=pin[Nt:Nt + F])
        if take_n and take_f:
            dev.copy_(pin, non_blocking=True)
        elif take_n:
            dev[:nb].copy_(pin[:nb], non_blocking=True)
        else:
            dev[Nt:Nt + fb].copy_(pin[Nt:Nt + fb], non_blocking=True)
        ev.record()
        slot[4] = True
        return (dev[:nb] if take_n else None), (dev[Nt:Nt + fb] if take_f else None)

    def _core_args(self):
        """An argument block with the parameter / optimiser buffers, the geometry of the data set and the optimiser constants."""
        p = _lib.ptr
        a = _lib.CosmosArgs()
        a.params, a.exp_avg, a.exp_avg_sq, a.last_step = p(self._params), p(self._exp_avg), p(self._exp_avg_sq), p(self._last_step)
        a.globals, a.gbase = p(self.globals), p(self.gbase)
        a.Nt, a.F, a.C, a.P, a.K, a.O = self.Nt, self.F, self.C, self.P, self.K, self.O
        a.lr, a.beta1, a.beta2, a.adam_eps = self.lr, self.betas[0], self.betas[1], self.adam_eps
        a.beta1_d, a.beta2_d = float(self.betas[0]), float(self.betas[1])
        a.crosstalk = int(self.crosstalk)
        return a

    def make_args(self, ndx=None, fdx=None, draw_globals=True, global_weight=1.0, step=None, draw_locals=None,
                  _for_step=False, _ws=None):
        if not _for_step:
            # staged calls from outside read the parameters of arbitrary units and overwrite globals / gsum / grad: finish
            # a pipelined tail or an in-flight all-reduce first, then bring every unit to the current Adam step
            self.join()
            self._grad_dirty = True
        nb = self.Nt if ndx is None else int(ndx.numel())
        fb = self.F if fdx is None else int(fdx.numel())
        if _ws is None:
            self._workspace(nb, fb)  # (_ws: the caller has set up a workspace for batches up to that size)
        ndx, fdx = self._indices_to_device(ndx, fdx)
        # keep the index tensors alive while kernels run (the previous step's too: its tail may still be pending)
        self._keep_prev, self._keep = getattr(self, "_keep", None), (ndx, fdx)
        p = _lib.ptr
        a = self._core_args()
        a.images, a.xy, a.is_ontarget, a.aoi_mask = p(self.images), p(self.xy), p(self.is_ontarget), p(self._mask_arg)
        a.images_il = p(self.images_il)
        a.images_il16 = p(self.images_il16)  # (None until a step has taken the fused route: _fuse)
        a.pixstats = p(self.pixstats)
        a.ndx, a.fdx = p(ndx), p(fdx)
        a.offset_samples, a.offset_logits = p(self.offset_samples), p(self.offset_logits)
        a.grad = p(self.grad)
        a.lat, a.pix, a.aoi_part, a.blk_part = p(self.lat), p(self.pix), p(self.aoi_part), p(self.blk_part)
        a.site = p(self.site)
        a.draw_locals = int(bool(draw_globals if draw_locals is None else draw_locals))
        a.il_min_units = self.il_min_units
        a.gsum, a.elbo_out = p(self._gsum_buf), p(self.elbo_out)
        a.nb, a.fb, a.n_offset, a.draw_globals = nb, fb, self.n_offset, int(bool(draw_globals))
        a.scale_n = self.Nt_global / self._nb_global(nb)
        a.scale = a.scale_n * self.F / fb
        a.global_weight = global_weight
        a.eps = self.eps
        pr = self.priors
        a.width_min, a.width_max, a.height_std = pr["width_min"], pr["width_max"], pr["height_std"]
        a.background_mean_std, a.background_std_std = pr["background_mean_std"], pr["background_std_std"]
        a.gain_std, a.lamda_rate, a.proximity_rate = pr["gain_std"], pr["lamda_rate"], pr["proximity_rate"]
        t = self.adam_step + 1
        a.bias_correction1 = 1.0 - self.betas[0] ** t
        a.bias_correction2 = 1.0 - self.betas[1] ** t
        a.zero_grad = int(nb < self.Nt or fb < self.F)
        a.fuse_adam = 0  # set by _open_step()
        a.seed = self.seed
        a.step = self.adam_step if step is None else int(step)
        a.pixel_mode = 0  # (_step_overlapped / _step_sharded ask for the fused launch)
        a.sync, a.tail_kind = p(self._sync), 0
        a.pu_split = self.pu_split
        scratch, a.pu_scratch_tiles = self._pu_split_scratch(nb, fb)
        a.pu_scratch = p(scratch)
        return a

    def _step_args(self, ndx, fdx):
        """make_args for step(): the ~60 fields are filled once per batch geometry / optimiser setting and copied
        afterwards; only the subsample pointers, the step count and the bias corrections change from step to step
        (minibatch steps are launch-bound: the host side of a step must stay well below the ~50 us of its kernels)."""
        nb = self.Nt if ndx is None else int(ndx.numel())
        fb = self.F if fdx is None else int(fdx.numel())
        key = (nb, fb, self.lr, self.betas, self.adam_eps, self.seed, id(self.priors), self.pu_split)
        if self.__dict__.get("_tmpl_key") != key or self._ws_key != (nb, fb):  # (the template points into the workspace)
            a = self.make_args(ndx, fdx, _for_step=True)
            self._tmpl, self._tmpl_key = _lib.CosmosArgs.from_buffer_copy(a), key
            return a
        a = _lib.CosmosArgs.from_buffer_copy(self._tmpl)
        ndx, fdx = self._indices_to_device(ndx, fdx)
        self._keep_prev, self._keep = self._keep, (ndx, fdx)
        a.ndx, a.fdx = _lib.ptr(ndx), _lib.ptr(fdx)
        t = self.adam_step + 1
        a.bias_correction1 = 1.0 - self.betas[0] ** t
        a.bias_correction2 = 1.0 - self.betas[1] ** t
        a.step = self.adam_step
        return a

    def _nb_global(self, nb):
        # AOI sharding: every rank subsamples nb local AOIs of Nt local ones, so the global
        # subsample is nb * (Nt_global / Nt)
        return nb * self.Nt_global / self.Nt

    # -- launches ------------------------------------------------------------------------------------
    def _stream(self):
        # the raw handle of torch's current stream (torch.cuda.current_stream() builds a Stream object: ~9 us a call,
        # several calls per step)
        index = self.device.index if self.device.index is not None else torch.cuda.current_device()
        return C.c_void_p(torch._C._cuda_getCurrentRawStream(index))

    def call(self, name, args):
        _lib.check(getattr(self.lib, "tq_" + name)(C.byref(args), self._stream()), "tq_" + name)

    def ksmogn_args(self, backward=True):
        """Argument block of ``tq_ksmogn_log_prob`` for the full batch with the latents in the workspace (diagnostics and
        bench.py's roofline leg)."""
        self._workspace(self.Nt, self.F)
        K, M = self.K, 1 << self.K
        B = self.Nt * self.F * self.C
        k = _lib.KsmognArgs()
        p = _lib.ptr
        k.images, k.images_il, k.xy, k.ndx, k.fdx = p(self.images), p(self.images_il), p(self.xy), None, None
        k.nb_full, k.il_min_units = self.Nt, self.il_min_units
        k.pixstats, k.stats_stride = p(self.pixstats), B
        f = lambda row: self.lat.data_ptr() + 4 * row * B
        k.background, k.height, k.width, k.x, k.y = f(0), f(1), f(1 + K), f(1 + 2 * K), f(1 + 3 * K)
        k.gain = self.globals.data_ptr()
        k.offset_samples, k.offset_logits = p(self.offset_samples), p(self.offset_logits)
        k.gout, k.m_logit, k.aoi_mask = None, p(self._params), p(self._mask_arg)
        g = lambda row: self.pix.data_ptr() + 4 * row * B
        k.ll = g(0)
        if backward:
            k.g_background, k.g_gain = g(M), g(M + 1)
            k.g_height, k.g_width, k.g_x, k.g_y = g(M + 2), g(M + 2 + K), g(M + 2 + 2 * K), g(M + 2 + 3 * K)
        k.m_kstride = B
        k.nb, k.fb, k.C, k.F, k.P, k.K, k.O = self.Nt, self.F, self.C, self.F, self.P, K, self.O
        k.scale = 1.0
        k.pixel_mode = 0
        return k

    def _fusable(self):
        """Can a full-batch step of this engine run pixel + per-unit kernel in one launch?  (The host predicate
        tq_fused_pixel_unit of tq_cosmos.hip asks the same of a step's arguments.)"""
        return (self.pipelined_tail and not self.crosstalk and self.K <= 2 and self.O == 1 and self.P in (14, 20)
                and self.Nt * self.F * self.C >= self.il_min_units and self.F * self.C >= 256)

    def _fuse(self, a):
        """Step `a` takes the fused launch: with the 16-bit tiles where the engine has them (built at the first such step)."""
        a.pixel_mode = _lib.PIXEL_FUSED_UNIT
        a.images_il16 = _lib.ptr(self._tile16())

    def _route(self, nb, fb, allreduce):
        """The launch sequence of a step of nb AOIs x fb frames (step() and step_subsampled() both ask here):

        * ``"streamed"``: the images do not fit the device, the step's AOIs go through in groups (_step_streamed);
        * ``"one_launch"``: catch-up, site draws, likelihood, per-unit terms + Adam in ONE launch that also runs the pending
          tail of the previous step (tq_cosmos_minibatch_step): minibatches with the lazy Adam clock, and SMALL full batches
          (BASELINE config c1: 5000 units), whose few hundred workgroups are latency in every phase as a minibatch's are;
        * ``"overlapped"``: the pipelined step, its tail runs inside the next step's sampling launch
          (tq_cosmos_step_overlapped): full batches, and the lazy-clock minibatches the single launch does not take
          (crosstalk, fb C < 16);
        * ``"staged"``: the launches one after the other (tq_cosmos_step): minibatches with the dense Adam;
        * ``"sharded"``: the staged launches with the cross-unit sums all-reduced between them (AOI sharding), also the
          route of engines without the pipelined tail.

        Attribute reads and integer tests only: at the default 10 x 512 minibatch the host bounds ``Model.run``."""
        if self.streamed:
            return "streamed"
        if allreduce is not None or not self.pipelined_tail:
            return "sharded"
        minibatch = nb < self.Nt or fb < self.F
        if self.fused_minibatch and not self.crosstalk:
            # (offset histograms stay in the single launch: the staged sequence with the wave-per-unit likelihood kernel
            # measured 0.150 against 0.162 ms at O = 50 -- not worth a second path through the step)
            if minibatch and self.lazy_adam and fb * self.C >= 16:
                return "one_launch"
            B = self.Nt * self.F * self.C
            if (not minibatch and B <= self.small_full_max_units and B < self.il_min_units
                    and self.F * self.C >= 16):
                return "one_launch"
        return "overlapped" if not minibatch or self.lazy_adam else "staged"

    def step_subsampled(self, nb, fb, generator=None):
        """A minibatch step on a subsample the DEVICE has drawn: the single-launch minibatch step also draws the next step's
        `randperm(Nt)[:nb]`, `randperm(F)[:fb]` (include/tapqir_hip.h: next_ndx / next_fdx) into the other of two index
        slots, so the host of a running fit neither draws, stages nor copies an index -- at the default 10 x 512 the two
        host-side randperm calls and their copy, not the GPU, bounded ``Model.run``.  The first step of a sequence (and any
        step whose batch sizes differ from what the previous launch prepared) takes a host draw from ``generator``.  Returns
        False if this engine cannot run that path (the caller then passes its own subsample to ``step``)."""
        nb, fb = min(int(nb), self.Nt), min(int(fb), self.F)
        drawn = (self.Nt if nb < self.Nt else 0) + (self.F if fb < self.F else 0)  # keys the launch would walk
        if not (0 < drawn <= DEVICE_SUBSAMPLE_MAX
                and self._route(nb, fb, None) == "one_launch"
                and os.environ.get("TAPQIR_AMD_DEVICE_SUBSAMPLE", "1") != "0"):
            return False
        st = self.__dict__.get("_sub")
        if st is None:  # (not setdefault: its argument -- two device allocations + fills -- would be built at every step)
            st = self._sub = {"slots": [torch.zeros(self.Nt + self.F, dtype=torch.int32, device=self.device) for _ in range(2)],
                              "turn": 0, "ready": None}
        cur, Nt = st["turn"], self.Nt
        slot, nxt = st["slots"][cur], st["slots"][1 - cur]
        if st["ready"] != (nb, fb, self.adam_step):
            if nb < self.Nt:
                slot[:nb].copy_(torch.randperm(self.Nt, generator=generator)[:nb].to(torch.int32))
            if fb < self.F:
                slot[Nt:Nt + fb].copy_(torch.randperm(self.F, generator=generator)[:fb].to(torch.int32))
        ndx = slot[:nb] if nb < self.Nt else None
        fdx = slot[Nt:Nt + fb] if fb < self.F else None
        self.step(ndx, fdx, _next_sub=(nxt[:nb] if nb < self.Nt else None, nxt[Nt:Nt + fb] if fb < self.F else None))
        st["turn"], st["ready"] = 1 - cur, (nb, fb, self.adam_step)
        return True

    def draw_subsample_device(self, nb, fb, step):
        """The subsample of the minibatch step that starts from ``adam_step == step``, as the device draws it for this engine's
        seed: ``(ndx, fdx)``, int32 device tensors of nb AOI / fb frame indices, ``None`` where the whole axis is taken.
        Mind the off-by-one: the launch of step ``s`` draws the subsample of step ``s + 1`` with the key stream
        ``(seed, s + 1)``, so what this returns is what the launch of step ``step - 1`` writes into its ``next_ndx`` /
        ``next_fdx`` (``tq_subsample_draw``, the same device routine in a launch of its own) -- the indices
        ``step_subsampled`` runs step ``step`` on, unless that step opened a sequence with a host draw.  Replaces
        pyro.plate's subsample (tapqir/models/cosmos.py:194-208); a fit's subsamples are reproducible from (seed, step)."""
        nb, fb = min(int(nb), self.Nt), min(int(fb), self.F)
        out = []
        for axis, (n, take) in enumerate(((self.Nt, nb), (self.F, fb))):
            if take >= n:
                out.append(None)
                continue
            idx = torch.empty(take, dtype=torch.int32, device=self.device)
            _lib.check(self.lib.tq_subsample_draw(self.seed & 0xFFFFFFFFFFFFFFFF, int(step), axis, n, take, _lib.ptr(idx), self._stream()),
                       "tq_subsample_draw")
            out.append(idx)
        return tuple(out)

    def step(self, ndx=None, fdx=None, allreduce=None, _next_sub=None):
        """One SVI step; returns nothing (the ELBO stays on the device in ``elbo_out``).

        ``allreduce(gsum)`` sums the cross-unit sums over the ranks of an AOI-sharded run.  If it returns a handle with
        ``wait()`` (an asynchronous collective) and the step is a full-batch one, the global tail of the step (global
        sites, Adam of the per-AOI and global parameters) is deferred: it runs after the NEXT step's local guide
        sampling, which needs local parameters only, so the collective's latency hides behind that kernel.  ``join()``
        (called by every read-out) completes a deferred tail."""
        nb = self.Nt if ndx is None else int(ndx.numel())
        fb = self.F if fdx is None else int(fdx.numel())
        route = self._route(nb, fb, allreduce)
        if route == "streamed":  # (its groups have an argument block each)
            if allreduce is not None:
                raise NotImplementedError("AOI sharding of a streamed data set: shard first, each rank then streams its own AOIs "
                                          "(not built: a rank's shard of every BASELINE config fits its 288 GB many times over)")
            return self._step_streamed(ndx, fdx)
        a = self._step_args(ndx, fdx)
        self._open_step(a)
        if route == "one_launch":
            self._step_one_launch(a, _next_sub)
        elif route == "overlapped":
            self._step_overlapped(a)
        elif route == "staged":
            self._step_staged(a)
        else:
            self._step_sharded(a, allreduce)
        self.adam_step += 1

    def _open_step(self, a):
        """The optimiser side of a step's start, for its argument block `a` (a streamed step: of every group): Adam of the local
        block fused into the per-unit kernel for full batches and for minibatches with the lazy clock, which starts here if
        it is not running; any other step first brings every unit to the current Adam step and carries no clock.  Returns
        whether the step is a lazy one: its route then catches up the units of the batch before it samples."""
        minibatch = bool(a.zero_grad)
        lazy = minibatch and self.lazy_adam
        a.fuse_adam = int(not minibatch or lazy)
        if not minibatch:
            self._grad_dirty = True  # a full-batch step writes every element it reads and clears none
        elif self._grad_dirty:
            # A minibatch step writes the gradient of its own units and AOIs only and relies on the rest being zero (the Adam
            # of a minibatch step clears what it read).  After a full-batch step or staged calls from outside the buffer
            # holds THEIR gradients: the per-AOI parameters of the AOIs outside this minibatch would take them again.
            self._finish_pending()
            self._finish_tail()
            self.grad.zero_()
            self._grad_dirty = False
        if lazy:
            if not self._stale:
                self._last_step.fill_(self.adam_step)  # every unit is current: start the clock here
                self._stale = True
        else:
            self._catch_up_all()
            a.last_step = None  # no unit falls behind
        return lazy

    def _step_one_launch(self, a, next_sub):
        """Catch-up, site draws, likelihood, per-unit terms + Adam of this step and the pending tail of the previous one in
        a single launch; the tail of this step stays pending."""
        self._finish_pending()
        prev = self._tail_args
        self._sync_value = self._sync_value % 0x3FFFFFFF + 1  # never 0, never the same value twice in a row
        a.sync_value = self._sync_value
        if next_sub is not None:
            a.next_ndx, a.next_fdx = _lib.ptr(next_sub[0]), _lib.ptr(next_sub[1])
        _lib.check(self.lib.tq_cosmos_minibatch_step(C.byref(a), None if prev is None else C.byref(prev), self._stream()),
                   "tq_cosmos_minibatch_step")
        a.tail_kind = _lib.TAIL_ROWS16
        self._tail_args = a

    def _step_overlapped(self, a):
        """The pipelined step: the pending tail of the previous step inside this step's sampling launch; its own stays pending."""
        if a.last_step:
            self._adam_catchup(a, 0)
        self._finish_pending()
        if self.fuse_unit and not a.zero_grad and self._fusable():
            self._fuse(a)
        prev = self._tail_args
        _lib.check(self.lib.tq_cosmos_step_overlapped(C.byref(a), None if prev is None else C.byref(prev), self._stream()),
                   "tq_cosmos_step_overlapped")
        self._tail_args = a

    def _step_staged(self, a):
        """The launches one after the other, nothing left pending."""
        self._finish_pending()
        self._finish_tail()
        self.call("cosmos_step", a)

    def _step_sharded(self, a, allreduce):
        """The staged launches with the cross-unit sums all-reduced between them; a full-batch step whose collective is
        asynchronous leaves its global tail pending for the next step's sampling."""
        if a.last_step:
            self._adam_catchup(a, 0)
        self._finish_tail()
        pending = self._pending
        if pending is not None and not a.fuse_adam:
            self._finish_pending()  # a minibatch step samples after the dense Adam of the previous one
            pending = None
        if pending is not None and self.split_sampling and getattr(pending[1], "in_stream", False):
            # the collective was issued on this stream (tapqir_amd.rccl.RcclDirect): stream order is the dependency.  ONE
            # sampling launch that carries the pending step's post-all-reduce tail and this step's global draws
            prev, _ = self._pending
            self._pending = None
            _lib.check(self.lib.tq_cosmos_sample_locals_range(C.byref(a), 0, 1 + 4 * self.K, C.byref(prev), self._stream()),
                       "tq_cosmos_sample_locals_range")
        elif pending is not None and self.split_sampling:
            # first half of the local sites while the all-reduce is in flight; the rest in a launch that also
            # carries the pending step's post-all-reduce tail and this step's global draws
            nsites = 1 + 4 * self.K
            n1 = nsites // 2
            prev, handle = self._pending
            self._pending = None
            _lib.check(self.lib.tq_cosmos_sample_locals_range(C.byref(a), 0, n1, None, self._stream()),
                       "tq_cosmos_sample_locals_range")
            handle.wait()  # the current stream waits for the collective
            _lib.check(self.lib.tq_cosmos_sample_locals_range(C.byref(a), n1, nsites - n1, C.byref(prev), self._stream()),
                       "tq_cosmos_sample_locals_range")
        else:
            self.call("cosmos_sample_locals", a)
            if pending is not None:
                self._finish_pending(next_args=a)  # ... and draws this step's global sites in the same launch
            else:
                self.call("cosmos_sample_globals", a)
        if a.fuse_adam and not a.zero_grad and self.fuse_unit and self._fusable():
            self._fuse(a)
        self.call("cosmos_elbo_grads", a)
        handle = allreduce(self.gsum) if allreduce is not None else None
        if handle is not None and hasattr(handle, "wait") and a.fuse_adam:
            self._pending = (a, handle)
        else:
            if handle is not None and hasattr(handle, "wait"):
                handle.wait()
            self._tail_reduced(a, None)

    def _tail_reduced(self, a, next_args):
        """Everything of step `a` after the all-reduce (one launch), plus the global draws of `next_args`."""
        nxt = None if next_args is None else C.byref(next_args)
        _lib.check(self.lib.tq_cosmos_tail_reduced(C.byref(a), nxt, self._stream()), "tq_cosmos_tail_reduced")

    def _finish_pending(self, next_args=None):
        """Global tail of a step whose all-reduce was left in flight."""
        if self._pending is None:
            return
        a, handle = self._pending
        self._pending = None
        handle.wait()  # the current stream waits for the collective
        self._tail_reduced(a, next_args)

    def _finish_tail(self):
        """Tail of a pipelined full-batch step (tq_cosmos_step_overlapped left it pending)."""
        if self._tail_args is not None:
            a, self._tail_args = self._tail_args, None
            self.call("cosmos_tail", a)

    def join(self):
        """Complete deferred work: the pending tail of a pipelined step, or the global tail of a sharded step that waits
        for its all-reduce.  Every read-out of elbo_out / parameters goes through here."""
        self._finish_pending()
        self._finish_tail()
        self._catch_up_all()

    # -- named views -----------------------------------------------------------------------------------
    def named(self, which="params"):
        self.join()  # finish a pending global tail first: the views then hold the parameters after the last step
        return self.layout.views(getattr(self, which))
