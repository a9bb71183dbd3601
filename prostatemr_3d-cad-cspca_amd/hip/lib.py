"""ctypes binding of libm1hip.so (the C ABI declared in include/m1hip.h).

The library is built in-tree by ``build()`` (``make`` + hipcc --offload-arch=gfx950) and is the ONLY
compute path of this package: there is no eager/torch fallback.  If the shared object is missing or an
entry point returns a non-zero status, a RuntimeError naming the m1_status is raised.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess
import threading

_HERE = os.path.dirname(os.path.abspath(__file__))
PKG_DIR = os.path.dirname(_HERE)
CSRC_DIR = os.path.join(PKG_DIR, "csrc")
SO_PATH = os.path.join(PKG_DIR, "libm1hip.so")
if os.environ.get("M1HIP_SO"):          # harness only: a bisection build of the same sources (csrc/Makefile PK_FILES), e.g. libm1hip_pk.so
    SO_PATH = os.path.join(PKG_DIR, os.path.basename(os.environ["M1HIP_SO"]))
HEADER = os.path.join(os.path.dirname(PKG_DIR), "include", "m1hip.h")

M1_F32, M1_BF16 = 0, 1
M1_MAX_SRC = 6


class m1_src_t(C.Structure):
    _fields_ = [("ptr", C.c_void_p), ("C", C.c_int), ("_pad", C.c_int)]


class m1_conv_desc_t(C.Structure):
    _fields_ = [("N", C.c_int), ("D", C.c_int), ("H", C.c_int), ("W", C.c_int),
                ("Cin", C.c_int), ("Cout", C.c_int),
                ("kd", C.c_int), ("kh", C.c_int), ("kw", C.c_int),
                ("sd", C.c_int), ("sh", C.c_int), ("sw", C.c_int),
                ("dtype", C.c_int), ("nsrc", C.c_int),
                ("src", m1_src_t * M1_MAX_SRC)]


class m1_head_t(C.Structure):
    _fields_ = [("logits", C.c_void_p), ("dlogits", C.c_void_p),
                ("u0", C.c_int), ("u1", C.c_int), ("u2", C.c_int), ("_pad", C.c_int)]


class SeGateFwdJob(C.Structure):
    """m1_se_gate_fwd_job_t"""
    _fields_ = [(n, C.c_void_p) for n in ("beta3", "W6", "b6", "W7", "b7", "hidden", "g")] + [("F", C.c_int), ("Fr", C.c_int)]


class SeGateJob(C.Structure):
    """m1_se_gate_job_t"""
    _fields_ = [(n, C.c_void_p) for n in ("beta3", "W6", "W7", "hidden", "g", "dg", "dbeta3_add", "dW6", "db6", "dW7", "db7")] \
        + [("F", C.c_int), ("Fr", C.c_int), ("accumulate", C.c_int), ("_pad", C.c_int)]


class m1_aug_params_t(C.Structure):
    """One sample's augmentation record (include/m1hip.h); ``AUG_DTYPE`` is the same layout for numpy."""
    _fields_ = [("fired", C.c_uint32), ("gamma_ch", C.c_uint32), ("poor_ch", C.c_uint32), ("scale", C.c_int32),
                ("rot_pad", C.c_int32), ("rot", C.c_float * 6), ("tr", C.c_int32 * 4), ("cs", C.c_int32 * 4),
                ("cs_channel", C.c_int32), ("gamma", C.c_float), ("noise_std", C.c_float), ("angle_deg", C.c_float),
                ("_pad", C.c_int32)]


# enum m1_aug_stage
M1_AUG_MASTER, M1_AUG_ZOOM, M1_AUG_FLIP, M1_AUG_ROTATE, M1_AUG_TRANSLATE = 1, 2, 4, 8, 16
M1_AUG_CSHIFT, M1_AUG_GAMMA, M1_AUG_POOR, M1_AUG_NOISE = 32, 64, 128, 256


class m1_crop_pad_t(C.Structure):
    """The crop / pad index map of the preprocessing kernels (include/m1hip.h)."""
    _fields_ = [("src", C.c_int * 3), ("dst", C.c_int * 3), ("start", C.c_int * 3), ("mode", C.c_int), ("cval", C.c_float)]


# enum m1_raw_dtype / m1_pad_mode
M1_RAW_F32, M1_RAW_I16, M1_RAW_I32 = 0, 1, 2          # (M1_RAW_I32: m1_restore with order 0 only)
M1_PAD_CONSTANT, M1_PAD_EDGE, M1_PAD_REFLECT, M1_PAD_SYMMETRIC = 0, 1, 2, 3


class m1_resample_t(C.Structure):
    """The axis-aligned resampling grid of m1_resample (include/m1hip.h)."""
    _fields_ = [("src", C.c_int * 3), ("dst", C.c_int * 3), ("first", C.c_int * 3), ("order", C.c_int), ("step", C.c_double * 3),
                ("defval", C.c_float), ("_pad", C.c_int)]


M1_RESAMPLE_MAX_LINE = 1024


class m1_restore_t(C.Structure):
    """The back-projection geometry of m1_restore (include/m1hip.h): per axis the scan's length ``dst``, ratio = spacing / out_spacing,
    the kept window (first, count) of the resampled grid and the pad voxels ``lo`` in front on the network grid."""
    _fields_ = [("src", C.c_int * 3), ("dst", C.c_int * 3), ("first", C.c_int * 3), ("count", C.c_int * 3), ("lo", C.c_int * 3),
                ("order", C.c_int), ("ratio", C.c_double * 3), ("defval", C.c_float), ("deflabel", C.c_int)]


M1_RESTORE_MAX_SEL = 4              # the widest channel selection m1_restore stores with vector stores (wider: element stores)

M1_TILE_MAX_AXIS = 16


class m1_tile_t(C.Structure):
    """The tile geometry of m1_tile_gather / m1_tile_blend (include/m1hip.h): per axis the volume's and the tile's length, the number
    of tiles and their ascending origins (``tiling.tile_geometry`` fills it)."""
    _fields_ = [("vol", C.c_int * 3), ("tile", C.c_int * 3), ("n", C.c_int * 3), ("origin", (C.c_int * M1_TILE_MAX_AXIS) * 3)]


class m1_cc_row_t(C.Structure):
    """One component's row of m1_cc_stats (include/m1hip.h); ``CC_ROW_DTYPE`` in hip/ops.py is the same layout for numpy."""
    _fields_ = [("count", C.c_int32), ("vmax", C.c_float), ("argmax", C.c_int64), ("lo", C.c_int32 * 3), ("hi", C.c_int32 * 3),
                ("sum", C.c_int64 * 3)]


# enum m1_cc_dtype / m1_cc_state, the labelling tile
M1_CC_F32, M1_CC_U8 = 0, 1
(M1_CC_ST_PEAK, M1_CC_ST_ARGMAX, M1_CC_ST_THRESHOLD, M1_CC_ST_SEL, M1_CC_ST_COUNT, M1_CC_ST_DONE, M1_CC_ST_NCAND,
 M1_CC_ST_SPARE) = range(8)
M1_CC_TILE = (4, 8, 32)

class m1_sd_row_t(C.Structure):
    """One (batch entry, class) row of m1_sd_metrics (include/m1hip.h); hip/ops.py views the same 160 bytes as 40 int32 words."""
    _fields_ = [("n", C.c_int64 * 2), ("le", (C.c_int64 * 4) * 2), ("sum", C.c_double * 2), ("hd", C.c_float), ("hd_ab", C.c_float),
                ("hd_ba", C.c_float), ("assd", C.c_float), ("mean_ab", C.c_float), ("mean_ba", C.c_float), ("hdq", C.c_float),
                ("hdq_ab", C.c_float), ("hdq_ba", C.c_float), ("dice", C.c_float), ("nsd", C.c_float * 4), ("_pad", C.c_float * 2)]


# enum m1_sd_dtype / m1_sd_stage, the limits of the surface-distance entry points
M1_SD_U8, M1_SD_I32 = 0, 1
M1_SD_STAGE_BORDER, M1_SD_STAGE_DISTANCE, M1_SD_STAGE_METRICS = 0, 1, 2
M1_SD_MAX_CLASSES, M1_SD_MAX_TOLERANCES, M1_SD_MAX_LINE = 8, 4, 256

# enum m1_val_dtype, the record of m1_val_score: 40 doubles = an 8-double header + 4 classes of 8 doubles
M1_VAL_Y_F32, M1_VAL_Y_U8 = 0, 1
M1_VAL_SLOTS, M1_VAL_MAX_K = 40, 4
VAL_HEAD_KEYS = ("focal", "entropy_sum", "entropy_fg_sum", "n_voxels", "n_fg")
VAL_CLASS_KEYS = ("sum_p", "sum_y", "sum_py", "n_pred", "n_true", "n_both", "p_max")

# the record of m1_cal_score: 8 header slots, then K + 2 histograms (top, cls[0..K), unc) of count[M], sum[M], hits[M]
M1_CAL_HEAD, M1_CAL_MIN_K, M1_CAL_MAX_K, M1_CAL_MAX_BINS, M1_CAL_MAX_VOXELS = 8, 2, 4, 64, 1 << 27
CAL_HEAD_KEYS = ("n_valid", "n_invalid", "n_ignored", "nll")
CAL_HIST_KEYS = {"top": ("count", "conf_sum", "correct"), "cls": ("count", "p_sum", "pos"), "unc": ("count", "u_sum", "errors")}

# m1_bootstrap_metrics: the Philox stream id of the draw, the caps and the items per block-wide scan
M1_STREAM_BOOTSTRAP = 0x424F4F54
M1_BOOTSTRAP_MAX_CASES, M1_BOOTSTRAP_MAX_BOOT, M1_BOOTSTRAP_MAX_RATES, M1_BOOTSTRAP_MAX_VALUES = 16384, 1 << 20, 8, 16
M1_BOOTSTRAP_CHUNK = 1024


class m1_bootstrap_table_t(C.Structure):
    """The packed table of m1_bootstrap_metrics (include/m1hip.h): device pointers and the four counts."""
    _fields_ = [(n, C.c_void_p) for n in ("case_label", "case_group_end", "case_lesions", "ev_case", "ev_tp", "ev_group_end",
                                          "values", "draw_perm")] + [(n, C.c_int) for n in ("N", "M", "V", "P")]


# enum m1_label_objective / m1_feed_mode
M1_LABEL_LESION, M1_LABEL_ZONAL = 0, 1
M1_FEED_TRAIN, M1_FEED_VALID, M1_FEED_TEST = 0, 1, 2


class m1_prof_rec_t(C.Structure):
    _fields_ = [("name", C.c_char * 48), ("total_ms", C.c_double), ("flops", C.c_double),
                ("bytes", C.c_double), ("launches", C.c_longlong)]


_vp, _i, _ll, _f, _u64, _sz, _d = C.c_void_p, C.c_int, C.c_longlong, C.c_float, C.c_uint64, C.c_size_t, C.c_double
_desc_p = C.POINTER(m1_conv_desc_t)

# name -> (restype, argtypes).  Must list EVERY symbol include/m1hip.h declares (tests check this).
SIGNATURES = {
    "m1_status_name": (C.c_char_p, [_i]),
    "m1_abi_version": (_i, []),
    "m1_conv_ws_bytes": (_sz, [_desc_p, _i, _i]),
    "m1_conv_pack_jobs": (_i, [_desc_p, _i, _i, _vp, C.POINTER(_vp)]),
    "m1_pack_batch": (_i, [_vp, _vp, _i, _i, _vp]),
    "m1_set_force_direct": (_i, [_i]),
    "m1_conv3d_fwd": (_i, [_desc_p, _vp, _vp, _vp, _vp, _vp, _i, _vp]),
    "m1_conv3d_dgrad": (_i, [_desc_p, _vp, _vp, C.POINTER(_vp), C.POINTER(_i), _vp, _i, _vp]),
    "m1_conv3d_dgrad_inbwd_rows": (_i, [_desc_p]),
    "m1_conv3d_dgrad_inbwd": (_i, [_desc_p, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _f, _vp, _i, C.POINTER(_i), _vp, _i, _vp]),
    "m1_config_set": (_i, [C.c_char_p, _i]),
    "m1_config_unset": (_i, [C.c_char_p]),
    "m1_config_get": (_i, [C.c_char_p, C.POINTER(_i)]),
    "m1_debug_lds_canary": (_i, [_vp, _i, _i, _vp]),
    "m1_debug_checksum": (_i, [_vp, _ll, _vp, _vp]),
    "m1_debug_scribble": (_i, [_i, _i, _vp]),
    "m1_debug_kernels": (C.c_char_p, [_i]),
    "m1_debug_plans": (C.c_char_p, [_i]),
    "m1_conv3d_wgrad": (_i, [_desc_p, _vp, _vp, _vp, _vp, _i, _vp]),
    "m1_conv3d_pair_supported": (_i, [_desc_p, _i]),
    "m1_conv3d_pair_fwd": (_i, [_desc_p, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _i, _vp]),
    "m1_conv3d_pair_dgrad": (_i, [_desc_p, _vp, _vp, _i, _vp, _vp, C.POINTER(_vp), C.POINTER(_i), _vp, _i, _vp]),
    "m1_convT3d_fwd": (_i, [_desc_p, _vp, _vp, _vp, _vp, _i, _vp]),
    "m1_convT3d_dgrad": (_i, [_desc_p, _vp, _vp, C.POINTER(_vp), C.POINTER(_i), _vp, _i, _vp]),
    "m1_convT3d_wgrad": (_i, [_desc_p, _vp, _vp, _vp, _vp, _i, _vp]),
    "m1_reduce_ws_floats": (_sz, [_i, _ll, _i, _i]),
    "m1_instnorm_stats": (_i, [_vp, _i, _ll, _i, _i, _f, _vp, _vp, _vp]),
    "m1_instnorm_apply": (_i, [_vp, _vp, _vp, _vp, _f, _vp, _i, _ll, _i, _i, _vp]),
    "m1_instnorm_bwd": (_i, [_vp, _vp, _vp, _vp, _f, _vp, _vp, _vp, _vp, _i, _ll, _i, _i, _vp, _i, _vp]),
    "m1_instnorm_bwd_partials": (_i, [_vp, _vp, _vp, _vp, _f, _vp, _vp, _vp, _vp, _i, _ll, _i, _i, _vp, _i, _vp, _i, _vp]),
    "m1_se_gate_fwd": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp]),
    "m1_se_gate_fwd_batch": (_i, [C.POINTER(SeGateFwdJob), _i, _vp]),
    "m1_se_gate_bwd_batch": (_i, [C.POINTER(SeGateJob), _i, _vp]),
    "m1_se_gate_bwd": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _i, _vp]),
    "m1_se_combine_fwd": (_i, [_vp] * 10 + [_i, _ll, _i, _i, _f, _vp, _u64, _vp, _vp]),
    "m1_se_combine_bwd": (_i, [_vp] * 17 + [_i, _ll, _i, _i, _f, _vp, _u64, _vp, _vp, _i, _vp]),
    "m1_se_combine_dup_fwd": (_i, [_vp] * 10 + [_i, _ll, _i, _i, _f, _vp, _u64, _vp, _vp]),
    "m1_se_combine_dup_bwd": (_i, [_vp] * 17 + [_i, _ll, _i, _i, _f, _vp, _u64, _vp, _vp, _i, _vp]),
    "m1_gate_sigma_fwd": (_i, [_vp] * 5 + [_i] * 9 + [_vp]),
    "m1_gate_sigma_bwd": (_i, [_vp] * 9 + [_i] * 9 + [_vp, _i, _vp]),
    "m1_mul_sigma_fwd": (_i, [_vp] * 3 + [_i] * 9 + [_vp]),
    "m1_gate_sigma_mul_fwd": (_i, [_vp] * 7 + [_i] * 16 + [_vp]),
    "m1_mul_sigma_bwd": (_i, [_vp] * 5 + [_i] * 10 + [_vp]),
    "m1_latent_sample_fwd": (_i, [_vp, _vp, _vp, _i, _ll, _i, _i, _i, _vp]),
    "m1_latent_sample_bwd": (_i, [_vp, _vp, _vp, _vp, _i, _ll, _i, _i, _i, _vp]),
    "m1_latent_sample_rng_fwd": (_i, [_vp, _vp, _u64, _vp, _i, _ll, _i, _i, _i, _vp]),
    "m1_latent_sample_rng_bwd": (_i, [_vp, _vp, _u64, _vp, _vp, _i, _ll, _i, _i, _i, _vp]),
    "m1_kl_fwd": (_i, [_vp, _vp, _vp, _i, _ll, _i, _i, _vp]),
    "m1_kl_bwd": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _ll, _i, _i, _vp]),
    "m1_kl_bwd_first": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _ll, _i, _i, _i, _vp]),
    "m1_softmax_heads_fwd": (_i, [C.POINTER(m1_head_t), _i, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    "m1_softmax_heads_bwd": (_i, [C.POINTER(m1_head_t), _i, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    "m1_mc_accum": (_i, [_vp, _i, _i, _ll, _i, _i, _vp, _i, _vp, _vp]),
    "m1_mc_finish": (_i, [_vp, _i, _i, _ll, _i, _vp, _vp, _vp]),
    "m1_mc_accum_u": (_i, [_vp, _i, _i, _ll, _i, _i, _vp, _vp, _vp, _i, _vp, _vp]),
    "m1_mc_finish_u": (_i, [_vp, _vp, _vp, _i, _i, _ll, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "m1_mc_accum_v": (_i, [_vp, _i, _i, _i, _i, _i, _i, _i, _u64, _vp, _vp, _vp, _i, _vp, _vp]),
    "m1_tta_views": (_i, [_vp, _i, _i, _i, _i, _i, _i, _i, _u64, _vp, _vp]),
    "m1_tile_gather": (_i, [_vp, _i, _i, _i, C.POINTER(m1_tile_t), _vp, _vp]),
    "m1_tile_blend": (_i, [_vp, _i, _i, C.POINTER(m1_tile_t), _vp, _vp, _vp]),
    "m1_focal_ws_floats": (_sz, [_i, _ll, _i]),
    "m1_focal_fwd": (_i, [_vp, _vp, _i, C.POINTER(_f), _f, _i, _ll, _i, _i, _vp, _vp, _vp]),
    "m1_focal_bwd": (_i, [_vp, _vp, _i, C.POINTER(_f), _f, _i, _ll, _i, _i, _vp, _vp, _vp]),
    "m1_dist_map_ws_bytes": (_sz, [_i, _i, _i, _i, _i]),
    "m1_dist_map": (_i, [_vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp]),
    "m1_dice_bd_ws_floats": (_sz, [_ll, _i]),
    "m1_dice_bd_fwd": (_i, [_vp, _vp, _i, _vp, _ll, _i, _i, _f, _f, _f, _vp, _vp, _vp]),
    "m1_dice_bd_bwd": (_i, [_vp, _vp, _i, _vp, _ll, _i, _i, _f, _f, _f, _vp, _vp, _vp, _vp]),
    "m1_aug_draw": (_i, [_vp, _i, _vp, _u64, _d, _d, _d, _d, _i, _d, _d, _d, _i, _d, _d, _i, _i, _i, _i, _vp]),
    "m1_aug_ws_bytes": (_sz, [_i, _i, _i, _i, _i]),
    "m1_aug_geom": (_i, [_vp] * 5 + [_i] * 9 + [_vp, _vp]),
    "m1_aug_gamma_stats": (_i, [_vp, _vp] + [_i] * 8 + [_vp, _vp]),
    "m1_aug_intensity": (_i, [_vp, _vp, _vp, _u64, _vp] + [_i] * 8 + [_vp, _vp]),
    "m1_contour_smooth_u8": (_i, [_vp, _vp, _vp, _ll, _i, _i, C.POINTER(_i), _i, _vp]),
    "m1_label_prepare": (_i, [_vp] * 5 + [_i] * 8 + [C.POINTER(_i), _vp]),
    "m1_preprocess_ws_bytes": (_sz, [C.POINTER(m1_crop_pad_t), _i, _i, _i]),
    "m1_crop_pad": (_i, [_vp, _i, C.POINTER(m1_crop_pad_t), _i, _i, _vp, _i, _vp]),
    "m1_order_stats": (_i, [_vp, _i, C.POINTER(m1_crop_pad_t), _i, _i, C.POINTER(_i), C.POINTER(_d), _i, _vp, _vp, _vp, _vp]),
    "m1_whiten": (_i, [_vp, _i, C.POINTER(m1_crop_pad_t), _i, _i, _vp, _vp, _i, _vp, _vp, _vp]),
    "m1_resample_ws_bytes": (_sz, [C.POINTER(m1_resample_t), _i, _i]),
    "m1_resample": (_i, [_vp, _i, C.POINTER(m1_resample_t), _i, _i, _vp, _i, _vp, _vp]),
    "m1_restore": (_i, [_vp, _i, C.POINTER(m1_restore_t), _i, _i, _i, _i, _vp, _vp, _vp]),
    "m1_cc_ws_bytes": (_sz, [_i, _i, _i, _i]),
    "m1_cc_label": (_i, [_vp, _i, _f, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp]),
    "m1_cc_stats": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _vp, _vp]),
    "m1_cc_overlap": (_i, [_vp, _vp, _i, _ll, _i, _i, _vp, _vp]),
    "m1_cc_peak": (_i, [_vp, _i, _ll, _f, _f, _i, _vp, _vp, _vp]),
    "m1_cc_select": (_i, [_vp, _i, _ll, _vp, _vp]),
    "m1_cc_take": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _ll, _i, _i, _i, _vp]),
    "m1_cc_relabel": (_i, [_vp, _vp, _i, _ll, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "m1_sd_ws_bytes": (_sz, [_i, _i, _i, _i, _i, _i]),
    "m1_sd_border": (_i, [_vp, _vp, _i, C.POINTER(_i), _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp]),
    "m1_sd_distance": (_i, [_vp, _i, _i, _i, _i, C.POINTER(_d), _vp, _vp, _vp]),
    "m1_sd_metrics": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _d, C.POINTER(_f), _i, _vp, _vp, _vp]),
    "m1_dropout": (_i, [_vp, _vp, _ll, _f, _vp, _u64, _i, _vp]),
    "m1_cast": (_i, [_vp, _i, _vp, _i, _ll, _vp]),
    "m1_adam_amsgrad": (_i, [_vp] * 5 + [_ll, _ll, _ll, _f, _f, _f, _vp, _f, _f, _f, _vp, _vp]),
    "m1_step_advance": (_i, [_vp, _vp, _vp]),
    "m1_grad_norm_ws": (_sz, [_ll]),
    "m1_grad_norm": (_i, [_vp, _vp, _ll, _ll, _ll, _f, _f, _f, _f, _f, _i, _vp, _sz, _vp, _vp]),
    "m1_adam_amsgrad_ctl": (_i, [_vp] * 5 + [_ll, _ll, _ll, _f, _f, _f, _vp, _f, _f, _f, _vp, _f, _vp, _vp]),
    "m1_step_advance_ctl": (_i, [_vp, _vp, _vp]),
    "m1_val_score_ws": (_sz, [_i, _ll, _i]),
    "m1_val_score": (_i, [_vp, _vp, _i, _vp, C.POINTER(_f), _f, _i, _ll, _i, _vp, _vp, _sz, _vp]),
    "m1_cal_record_slots": (_sz, [_i, _i]),
    "m1_cal_score": (_i, [_vp, _i, _vp, _vp, _vp, _f, _i, _ll, _i, _i, _vp, _vp]),
    "m1_bootstrap_metrics": (_i, [C.POINTER(m1_bootstrap_table_t), _i, _u64, _vp, C.POINTER(_d), _i, _vp, _vp]),
    "m1_wgrad_defer": (_i, [_i]),
    "m1_wgrad_fold_pending": (_i, [_vp]),
    "m1_wgrad_fold_drop": (_i, []),
    "m1_prof_enable": (_i, [_i]),
    "m1_prof_reset": (_i, []),
    "m1_prof_read": (_i, [C.POINTER(m1_prof_rec_t), _i]),
}

_lib = None
_lock = threading.Lock()


def build(verbose: bool = False) -> str:
    """Compile every HIP source for gfx950 into libm1hip.so (cross-compiles without a GPU)."""
    cmd = ["make", "-C", CSRC_DIR, "-j8"]
    res = subprocess.run(cmd, capture_output=True, text=True)
    if verbose or res.returncode != 0:
        print(res.stdout[-4000:])
        print(res.stderr[-4000:])
    if res.returncode != 0:
        raise RuntimeError("hipcc build of libm1hip.so failed (see output above)")
    return SO_PATH


def load() -> C.CDLL:
    """Load libm1hip.so (after torch so that both share one HIP runtime). Raises if it is missing."""
    global _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(SO_PATH):
            raise RuntimeError(
                f"libm1hip.so not found at {SO_PATH}: the HIP extension is the only compute path of this "
                "package (no CPU/eager fallback). Run `python -c 'import __graft_entry__ as g; g.build()'`.")
        import torch  # noqa: F401  -- loads torch's libamdhip64.so.7 first; ours then binds to the same runtime
        lib = C.CDLL(SO_PATH, mode=C.RTLD_GLOBAL)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)       # AttributeError => symbol missing: fail loudly
            fn.restype = res
            fn.argtypes = args
        _lib = lib
        return _lib


def status_name(rc: int) -> str:
    return load().m1_status_name(rc).decode()


def check(rc: int, what: str) -> None:
    if rc != 0:
        raise RuntimeError(f"{what} failed: {status_name(rc)} ({rc})")
