"""
ctypes binding of ``libtapqir_hip.so`` (C ABI declared in ``include/tapqir_hip.h``).

There is no fallback: if the shared library is missing or fails to load, every entry point
raises ``HipExtensionError``.  Build it with ``python -m tapqir_amd.build`` (or
``__graft_entry__.build()``).
"""

import ctypes as C
import os

from tapqir_amd.exceptions import HipExtensionError

_HERE = os.path.dirname(os.path.abspath(__file__))
# TAPQIR_AMD_LIB selects another build of the same library (A/B timing of compiler flags)
LIB_PATH = os.environ.get("TAPQIR_AMD_LIB") or os.path.join(_HERE, "libtapqir_hip.so")

c_float_p = C.POINTER(C.c_float)
c_double_p = C.POINTER(C.c_double)
c_int32_p = C.POINTER(C.c_int32)
c_uint8_p = C.POINTER(C.c_uint8)


class KsmognArgs(C.Structure):
    """``tq_ksmogn_args`` (include/tapqir_hip.h)."""

    _fields_ = [
        ("images", C.c_void_p), ("images_il", C.c_void_p), ("pixstats", C.c_void_p), ("xy", C.c_void_p),
        ("ndx", C.c_void_p), ("fdx", C.c_void_p), ("background", C.c_void_p), ("height", C.c_void_p), ("width", C.c_void_p),
        ("x", C.c_void_p), ("y", C.c_void_p), ("gain", C.c_void_p),
        ("offset_samples", C.c_void_p), ("offset_logits", C.c_void_p),
        ("gout", C.c_void_p), ("m_logit", C.c_void_p), ("aoi_mask", C.c_void_p),
        ("ll", C.c_void_p), ("g_background", C.c_void_p), ("g_height", C.c_void_p),
        ("g_width", C.c_void_p), ("g_x", C.c_void_p), ("g_y", C.c_void_p), ("g_gain", C.c_void_p),
        ("m_kstride", C.c_int64), ("stats_stride", C.c_int64),
        ("nb", C.c_int32), ("fb", C.c_int32), ("C", C.c_int32), ("F", C.c_int32),
        ("P", C.c_int32), ("K", C.c_int32), ("O", C.c_int32),
        ("nb_full", C.c_int32), ("il_min_units", C.c_int32),
        ("scale", C.c_float), ("pixel_mode", C.c_int32), ("images_by_slot", C.c_int32),
        ("images_il16", C.c_void_p),
    ]


class CosmosArgs(C.Structure):
    """``tq_cosmos_args`` (include/tapqir_hip.h)."""

    _fields_ = [
        ("images", C.c_void_p), ("images_il", C.c_void_p), ("pixstats", C.c_void_p), ("xy", C.c_void_p),
        ("is_ontarget", C.c_void_p), ("aoi_mask", C.c_void_p),
        ("ndx", C.c_void_p), ("fdx", C.c_void_p), ("offset_samples", C.c_void_p), ("offset_logits", C.c_void_p),
        ("params", C.c_void_p), ("grad", C.c_void_p), ("exp_avg", C.c_void_p), ("exp_avg_sq", C.c_void_p),
        ("lat", C.c_void_p), ("site", C.c_void_p), ("pix", C.c_void_p), ("aoi_part", C.c_void_p), ("blk_part", C.c_void_p),
        ("gsum", C.c_void_p), ("globals", C.c_void_p), ("gbase", C.c_void_p), ("elbo_out", C.c_void_p),
        ("Nt", C.c_int32), ("F", C.c_int32), ("C", C.c_int32), ("P", C.c_int32), ("K", C.c_int32), ("O", C.c_int32),
        ("nb", C.c_int32), ("fb", C.c_int32), ("n_offset", C.c_int32), ("draw_globals", C.c_int32),
        ("draw_locals", C.c_int32), ("il_min_units", C.c_int32),
        ("scale_n", C.c_float), ("scale", C.c_float), ("global_weight", C.c_float),
        ("eps", C.c_float),
        ("width_min", C.c_float), ("width_max", C.c_float), ("height_std", C.c_float),
        ("background_mean_std", C.c_float), ("background_std_std", C.c_float),
        ("gain_std", C.c_float), ("lamda_rate", C.c_float), ("proximity_rate", C.c_float),
        ("lr", C.c_float), ("beta1", C.c_float), ("beta2", C.c_float), ("adam_eps", C.c_float),
        ("bias_correction1", C.c_float), ("bias_correction2", C.c_float),
        ("zero_grad", C.c_int32), ("fuse_adam", C.c_int32), ("crosstalk", C.c_int32),
        ("seed", C.c_uint64), ("step", C.c_uint32),
        ("last_step", C.c_void_p), ("beta1_d", C.c_double), ("beta2_d", C.c_double),
        ("pixel_mode", C.c_int32), ("tail_kind", C.c_int32), ("sync", C.c_void_p), ("sync_value", C.c_int32),
        ("images_by_slot", C.c_int32), ("next_ndx", C.c_void_p), ("next_fdx", C.c_void_p),
        ("pu_split", C.c_int32), ("pu_scratch_tiles", C.c_int32), ("pu_scratch", C.c_void_p),
        ("images_il16", C.c_void_p),
    ]


TAIL_ROWS16 = 1       # TQ_TAIL_ROWS16 (tail_kind)
PIXEL_FUSED_UNIT = 2  # TQ_PIXEL_FUSED_UNIT (pixel_mode)
SYNC_WORDS = 64       # TQ_SYNC_WORDS
SUBSAMPLE_MAX = 65536  # TQ_SUBSAMPLE_MAX
GSUM_LEN = 32         # TQ_GSUM_LEN


class XtalkArgs(C.Structure):
    """``tq_xtalk_args`` (include/tapqir_hip.h)."""

    _fields_ = [
        ("images", C.c_void_p), ("images_il", C.c_void_p), ("pixstats", C.c_void_p), ("xy", C.c_void_p),
        ("ndx", C.c_void_p), ("fdx", C.c_void_p),
        ("background", C.c_void_p), ("height", C.c_void_p), ("width", C.c_void_p), ("x", C.c_void_p), ("y", C.c_void_p),
        ("gain", C.c_void_p), ("alpha", C.c_void_p), ("offset_samples", C.c_void_p), ("offset_logits", C.c_void_p),
        ("gout", C.c_void_p), ("m_logit", C.c_void_p), ("aoi_mask", C.c_void_p),
        ("ll_joint", C.c_void_p), ("ll", C.c_void_p), ("ell_excess", C.c_void_p),
        ("g_background", C.c_void_p), ("g_height", C.c_void_p), ("g_width", C.c_void_p), ("g_x", C.c_void_p),
        ("g_y", C.c_void_p), ("g_gain", C.c_void_p), ("g_alpha", C.c_void_p),
        ("m_kstride", C.c_int64),
        ("nb", C.c_int32), ("fb", C.c_int32), ("C", C.c_int32), ("F", C.c_int32),
        ("P", C.c_int32), ("K", C.c_int32), ("O", C.c_int32),
        ("nb_full", C.c_int32), ("il_min_units", C.c_int32),
        ("scale", C.c_float),
    ]


class ProbsArgs(C.Structure):
    """``tq_probs_args`` (include/tapqir_hip.h)."""

    _fields_ = [
        ("params", C.c_void_p), ("is_ontarget", C.c_void_p), ("globals_p", C.c_void_p), ("gbase_p", C.c_void_p),
        ("xy_given", C.c_void_p), ("z_probs", C.c_void_p), ("theta_probs", C.c_void_p),
        ("Nt", C.c_int32), ("F", C.c_int32), ("C", C.c_int32), ("P", C.c_int32), ("K", C.c_int32),
        ("particles", C.c_int32), ("draw", C.c_int32), ("eps", C.c_float), ("seed", C.c_uint64),
        ("n_offset", C.c_int32),
    ]


class RsampleArgs(C.Structure):
    """``tq_rsample_args`` (include/tapqir_hip.h)."""

    _fields_ = [
        ("height", C.c_void_p), ("width", C.c_void_p), ("x", C.c_void_p), ("y", C.c_void_p), ("xy", C.c_void_p),
        ("background", C.c_void_p), ("gain", C.c_void_p), ("offset_samples", C.c_void_p), ("offset_logits", C.c_void_p),
        ("out", C.c_void_p), ("B", C.c_int64), ("P", C.c_int32), ("K", C.c_int32), ("O", C.c_int32), ("seed", C.c_uint64),
    ]


class SnrArgs(C.Structure):
    """``tq_snr_args`` (include/tapqir_hip.h)."""

    _fields_ = [
        ("images", C.c_void_p), ("xy", C.c_void_p), ("height", C.c_void_p), ("width", C.c_void_p), ("x", C.c_void_p),
        ("y", C.c_void_p), ("background", C.c_void_p), ("snr", C.c_void_p), ("chi2", C.c_void_p),
        ("U", C.c_int64), ("P", C.c_int32), ("K", C.c_int32),
        ("gain", C.c_float), ("offset_mean", C.c_float), ("offset_var", C.c_float),
    ]


class IntervalArgs(C.Structure):
    """``tq_interval_args`` (include/tapqir_hip.h)."""

    _fields_ = [
        ("kind", C.c_int32), ("p0", C.c_void_p), ("p1", C.c_void_p), ("ll", C.c_void_p), ("ul", C.c_void_p),
        ("n", C.c_int64), ("ci", C.c_double), ("low", C.c_double), ("high", C.c_double),
    ]


INTERVAL_GAMMA, INTERVAL_AFFINE_BETA = 0, 1  # TQ_INTERVAL_GAMMA, TQ_INTERVAL_AFFINE_BETA


class GlimpseArgs(C.Structure):
    """``tq_glimpse_args`` (include/tapqir_hip.h)."""

    _fields_ = [
        ("frames", C.c_void_p), ("raw_xy", C.c_void_p), ("images", C.c_void_p), ("target_xy", C.c_void_p),
        ("offset_hist", C.c_void_p), ("status", C.c_void_p),
        ("H", C.c_int32), ("W", C.c_int32), ("N", C.c_int32), ("F", C.c_int32), ("C", C.c_int32), ("P", C.c_int32),
        ("c", C.c_int32), ("f0", C.c_int32), ("nf", C.c_int32),
        ("offset_x", C.c_int32), ("offset_y", C.c_int32), ("offset_P", C.c_int32),
    ]


class TtfbSampleArgs(C.Structure):
    """``tq_ttfb_sample_args`` (include/tapqir_hip.h)."""

    _fields_ = [
        ("p", C.c_void_p), ("log_surv", C.c_void_p), ("tau", C.c_void_p),
        ("N", C.c_int32), ("F", C.c_int32), ("S", C.c_int32), ("seed", C.c_uint64),
    ]


class TtfbFitArgs(C.Structure):
    """``tq_ttfb_fit_args`` (include/tapqir_hip.h)."""

    _fields_ = [
        ("tau", C.c_void_p), ("tauc", C.c_void_p), ("state", C.c_void_p), ("loss", C.c_void_p),
        ("S", C.c_int32), ("N", C.c_int32), ("Nc", C.c_int32), ("step0", C.c_int32), ("n_steps", C.c_int32),
        ("stage_lds", C.c_int32), ("Tmax", C.c_float),
        ("lr", C.c_double), ("beta1", C.c_double), ("beta2", C.c_double), ("eps", C.c_double),
    ]


TTFB_LDS_POINTS = 8192  # TQ_TTFB_LDS_POINTS
TTFB_STATE = 9          # TQ_TTFB_STATE


class DwellSampleArgs(C.Structure):
    """``tq_dwell_sample_args`` (include/tapqir_hip.h)."""

    _fields_ = [
        ("p", C.c_void_p), ("counts", C.c_void_p), ("hist_bound", C.c_void_p), ("hist_unbound", C.c_void_p),
        ("offsets", C.c_void_p), ("intervals", C.c_void_p), ("total", C.c_int64),
        ("N", C.c_int32), ("F", C.c_int32), ("S", C.c_int32), ("mode", C.c_int32), ("seed", C.c_uint64),
    ]


class DwellFitArgs(C.Structure):
    """``tq_dwell_fit_args`` (include/tapqir_hip.h)."""

    _fields_ = [
        ("values", C.c_void_p), ("weights", C.c_void_p), ("row_ptr", C.c_void_p), ("state", C.c_void_p),
        ("loss", C.c_void_p), ("S", C.c_int32), ("K", C.c_int32), ("step0", C.c_int32), ("n_steps", C.c_int32),
        ("stage_lds", C.c_int32), ("lr", C.c_double), ("beta1", C.c_double), ("beta2", C.c_double), ("eps", C.c_double),
    ]


DWELL_COUNT, DWELL_EMIT = 0, 1  # TQ_DWELL_COUNT, TQ_DWELL_EMIT
DWELL_COLS = 7                  # TQ_DWELL_COLS
DWELL_KMAX = 8                  # TQ_DWELL_KMAX
DWELL_LDS_PAIRS = 2048          # TQ_DWELL_LDS_PAIRS


# every symbol include/tapqir_hip.h declares (checked by tests/test_abi.py)
EXPORTS = [
    "tq_version", "tq_last_error", "tq_ksmogn_log_prob", "tq_ksmogn_crosstalk_log_prob", "tq_crosstalk_param_count",
    "tq_interleaved_floats", "tq_interleaved_floats_n", "tq_images_interleave_n", "tq_images_interleave", "tq_image_stats",
    "tq_interleaved_u16_n", "tq_images_interleave_u16_n",
    "tq_globals_size", "tq_gbase_size", "tq_cosmos_nblk", "tq_cosmos_param_count",
    "tq_cosmos_sample_globals", "tq_cosmos_sample_locals", "tq_cosmos_elbo_grads",
    "tq_cosmos_globals_grad", "tq_cosmos_adam", "tq_cosmos_adam_catchup", "tq_cosmos_step", "tq_cosmos_step_overlapped", "tq_cosmos_tail", "tq_cosmos_tail_reduced", "tq_cosmos_sample_locals_range",
    "tq_cosmos_blk_floats", "tq_cosmos_minibatch_step", "tq_subsample_draw", "tq_cosmos_pixel_unit",
    "tq_cosmos_pu_slots", "tq_cosmos_pu_split_auto", "tq_cosmos_pu_scratch_bytes",
    "tq_cosmos_probs", "tq_glimpse_extract", "tq_ksmogn_rsample", "tq_snr_chi2", "tq_ttfb_sample", "tq_ttfb_fit",
    "tq_dwell_sample", "tq_dwell_fit", "tq_credible_intervals",
    "tq_rates_count", "tq_rates_estimate",  # argument structs and prototypes: tapqir_amd/_lib_rates.py
    "tq_smooth_estep", "tq_smooth_mstep", "tq_smooth_viterbi", "tq_smooth_count",  # ... tapqir_amd/_lib_smooth.py
    "tq_smooth_dwell",
    "tq_hmm_estep", "tq_hmm_mstep", "tq_hmm_viterbi", "tq_hmm_count", "tq_hmm_estimate",  # ... tapqir_amd/_lib_hmm.py
    "tq_chain_dwell",
    "tq_multistart_estep", "tq_multistart_mstep",  # ... tapqir_amd/_lib_multistart.py
    "tq_joint_estep", "tq_joint_mstep", "tq_joint_viterbi",  # ... tapqir_amd/_lib_joint.py
    "tq_pair_dwell",
    "tq_mixture_mstep", "tq_mixture_count", "tq_mixture_estimate",  # ... tapqir_amd/_lib_mixture.py
    "tq_population_dwell",
    "tq_dwell_censored_hist", "tq_dwell_censored_fit", "tq_dwell_survival",  # ... tapqir_amd/_lib_censored.py
    "tq_refit_weights", "tq_refit_estep", "tq_refit_mstep",  # ... tapqir_amd/_lib_refit.py
    "tq_timed_table", "tq_timed_estep", "tq_timed_mstep",  # ... tapqir_amd/_lib_timed.py
]

_lib = None


def load():
    """Load the HIP library once; raise loudly if it is not there."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise HipExtensionError(
            f"{LIB_PATH} not found: the HIP extension is not built (run `python -m tapqir_amd.build`). "
            "tapqir_amd has no CPU fallback for the SVI hot path."
        )
    try:
        lib = C.CDLL(LIB_PATH)
    except OSError as err:
        raise HipExtensionError(f"failed to load {LIB_PATH}: {err}")
    lib.tq_version.restype = C.c_int
    lib.tq_last_error.restype = C.c_char_p
    for name in ("tq_globals_size", "tq_gbase_size"):
        getattr(lib, name).restype = C.c_int64
    lib.tq_cosmos_nblk.restype = C.c_int64
    lib.tq_cosmos_nblk.argtypes = [C.c_int64]
    lib.tq_cosmos_param_count.restype = C.c_int64
    lib.tq_cosmos_param_count.argtypes = [C.c_int32] * 4
    lib.tq_crosstalk_param_count.restype = C.c_int64
    lib.tq_crosstalk_param_count.argtypes = [C.c_int32] * 4
    lib.tq_ksmogn_crosstalk_log_prob.argtypes = [C.POINTER(XtalkArgs), C.c_void_p]
    lib.tq_ksmogn_crosstalk_log_prob.restype = C.c_int
    lib.tq_interleaved_floats.restype = C.c_int64
    lib.tq_interleaved_floats.argtypes = [C.c_int64, C.c_int32]
    lib.tq_interleaved_floats_n.restype = C.c_int64
    lib.tq_interleaved_floats_n.argtypes = [C.c_int64, C.c_int32]
    lib.tq_images_interleave_n.restype = C.c_int
    lib.tq_images_interleave_n.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p]
    lib.tq_interleaved_u16_n.restype = C.c_int64
    lib.tq_interleaved_u16_n.argtypes = [C.c_int64, C.c_int32]
    lib.tq_images_interleave_u16_n.restype = C.c_int
    lib.tq_images_interleave_u16_n.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p]
    lib.tq_images_interleave.restype = C.c_int
    lib.tq_images_interleave.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p]
    lib.tq_image_stats.restype = C.c_int
    lib.tq_image_stats.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p]
    lib.tq_ksmogn_log_prob.argtypes = [C.POINTER(KsmognArgs), C.c_void_p]
    lib.tq_ksmogn_log_prob.restype = C.c_int
    for name in ("tq_cosmos_sample_globals", "tq_cosmos_sample_locals", "tq_cosmos_elbo_grads",
                 "tq_cosmos_globals_grad", "tq_cosmos_adam", "tq_cosmos_adam_catchup", "tq_cosmos_step", "tq_cosmos_tail",
                 "tq_cosmos_pixel_unit"):
        fn = getattr(lib, name)
        fn.argtypes = [C.POINTER(CosmosArgs), C.c_void_p]
        fn.restype = C.c_int
    lib.tq_cosmos_blk_floats.argtypes = [C.c_int32] * 4 + [C.c_int64]
    lib.tq_cosmos_blk_floats.restype = C.c_int64
    lib.tq_cosmos_pu_slots.argtypes = [C.c_int32, C.c_int32]
    lib.tq_cosmos_pu_slots.restype = C.c_int32
    lib.tq_cosmos_pu_split_auto.argtypes = [C.c_int64, C.c_int32]
    lib.tq_cosmos_pu_split_auto.restype = C.c_int32
    lib.tq_cosmos_pu_scratch_bytes.argtypes = [C.c_int32]
    lib.tq_cosmos_pu_scratch_bytes.restype = C.c_int64
    for name in ("tq_cosmos_step_overlapped", "tq_cosmos_tail_reduced", "tq_cosmos_minibatch_step"):
        fn = getattr(lib, name)
        fn.argtypes = [C.POINTER(CosmosArgs), C.POINTER(CosmosArgs), C.c_void_p]
        fn.restype = C.c_int
    lib.tq_cosmos_sample_locals_range.argtypes = [C.POINTER(CosmosArgs), C.c_int32, C.c_int32, C.POINTER(CosmosArgs), C.c_void_p]
    lib.tq_cosmos_sample_locals_range.restype = C.c_int
    lib.tq_subsample_draw.argtypes = [C.c_uint64, C.c_uint32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
    lib.tq_subsample_draw.restype = C.c_int
    lib.tq_cosmos_adam_catchup.argtypes = [C.POINTER(CosmosArgs), C.c_int32, C.c_void_p]
    lib.tq_cosmos_adam_catchup.restype = C.c_int
    lib.tq_cosmos_probs.argtypes = [C.POINTER(ProbsArgs), C.c_void_p]
    lib.tq_cosmos_probs.restype = C.c_int
    lib.tq_ksmogn_rsample.argtypes = [C.POINTER(RsampleArgs), C.c_void_p]
    lib.tq_ksmogn_rsample.restype = C.c_int
    lib.tq_snr_chi2.argtypes = [C.POINTER(SnrArgs), C.c_void_p]
    lib.tq_snr_chi2.restype = C.c_int
    lib.tq_credible_intervals.argtypes = [C.POINTER(IntervalArgs), C.c_void_p]
    lib.tq_credible_intervals.restype = C.c_int
    lib.tq_glimpse_extract.argtypes = [C.POINTER(GlimpseArgs), C.c_void_p]
    lib.tq_glimpse_extract.restype = C.c_int
    lib.tq_ttfb_sample.argtypes = [C.POINTER(TtfbSampleArgs), C.c_void_p]
    lib.tq_ttfb_sample.restype = C.c_int
    lib.tq_ttfb_fit.argtypes = [C.POINTER(TtfbFitArgs), C.c_void_p]
    lib.tq_ttfb_fit.restype = C.c_int
    lib.tq_dwell_sample.argtypes = [C.POINTER(DwellSampleArgs), C.c_void_p]
    lib.tq_dwell_sample.restype = C.c_int
    lib.tq_dwell_fit.argtypes = [C.POINTER(DwellFitArgs), C.c_void_p]
    lib.tq_dwell_fit.restype = C.c_int
    _lib = lib
    return lib


def check(rc, what):
    if rc != 0:
        msg = load().tq_last_error().decode()
        raise HipExtensionError(f"{what} failed (code {rc}): {msg}")


def ptr(t):
    """Raw address of a torch tensor (or None)."""
    return None if t is None else t.data_ptr()
