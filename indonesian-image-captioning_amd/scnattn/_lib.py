"""ctypes binding of libscnattn.so (the C ABI declared in include/scnattn.h).

There is deliberately NO fallback: if the shared library is missing or a call fails, a
RuntimeError is raised.  The library is built in-tree by ``__graft_entry__.build()`` (``make -C
indonesian-image-captioning_amd/csrc``) so that it travels with the repository snapshot.
"""
import ctypes as C
import os
import threading

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libscnattn.so")

_lib = None
_lock = threading.Lock()

vp, i32, i64, f32, f64, sz = C.c_void_p, C.c_int, C.c_long, C.c_float, C.c_double, C.c_size_t


class Dims(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("B", "P", "E", "A", "D", "F", "M", "S", "V", "T", "L", "has_att")]


PARAM_FIELDS = (
    "attention_encoder_att_weight", "attention_encoder_att_bias",
    "attention_decoder_att_weight", "attention_decoder_att_bias",
    "attention_full_att_weight", "attention_full_att_bias",
    "embedding_weight",
    "decode_step_weight_ia", "decode_step_weight_ib", "decode_step_weight_ic",
    "decode_step_weight_ha", "decode_step_weight_hb", "decode_step_weight_hc",
    "decode_step_bias_ih", "decode_step_bias_hh",
    "init_h_weight", "init_h_bias", "init_c_weight", "init_c_bias",
    "f_beta_weight", "f_beta_bias", "fc_weight", "fc_bias",
)


class Params(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in PARAM_FIELDS]


class Pool(C.Structure):      # scnattn_pool
    _fields_ = [("Q", C.c_int), ("qtap_max", C.c_int), ("tap_idx", C.c_void_p), ("tap_w", C.c_void_p),
                ("qtap_idx", C.c_void_p), ("qtap_w", C.c_void_p), ("col_w", C.c_void_p)]


class ConvExtra(C.Structure):      # scnattn_conv_extra
    _fields_ = [("pro", C.c_int), ("epi", C.c_int), ("pro_ss", C.c_void_p),
                ("stat_partial", C.c_void_p), ("stat_shift", C.c_void_p), ("ez", C.c_void_p), ("emean", C.c_void_p),
                ("einvstd", C.c_void_p), ("egamma", C.c_void_p), ("ebeta", C.c_void_p), ("ldz", C.c_long),
                ("stride", C.c_int), ("Hi", C.c_int), ("Wi", C.c_int), ("Ho", C.c_int), ("Wo", C.c_int),
                ("force_split", C.c_int), ("force_mi", C.c_int)]


class BnEval(C.Structure):         # scnattn_bn_eval
    _fields_ = [("gamma", C.c_void_p), ("beta", C.c_void_p), ("mean", C.c_void_p), ("var", C.c_void_p), ("eps", C.c_float),
                ("res", C.c_void_p), ("ldres", C.c_long), ("relu", C.c_int)]


class BnEval16(C.Structure):       # scnattn_bn_eval16: the same layout, res is a bf16 map
    _fields_ = BnEval._fields_


class LaunchPlan(C.Structure):     # scnattn_launch_plan
    _fields_ = [(n, C.c_int) for n in ("family", "mi", "tA", "tB", "pro", "epi", "gather", "c3", "vec", "out_bf16", "wbf",
                                       "nb", "chunks", "empty", "kslice", "seg", "Q", "ntiles", "S", "kper", "mt", "nt")] + \
               [("tiles", C.c_long)] + \
               [(n, C.c_int) for n in ("grid_x", "grid_y", "grid_z", "in_launch", "second", "second_mode")]


# SCNATTN_PLAN_* / SCNATTN_SECOND_*
PLAN_NONE, PLAN_CGEMM, PLAN_SGEMM, PLAN_SKINNY, PLAN_CGEMM16, PLAN_CONV3_WGRAD, PLAN_WGRAD16_W9, PLAN_WGRAD16_W1 = range(8)
(SECOND_NONE, SECOND_CREDUCE, SECOND_CSTATS1, SECOND_CSTATS2_SLABS, SECOND_CSTATS2_C, SECOND_CREDUCE16, SECOND_CGEMM_REDUCE,
 SECOND_SPLITK_REDUCE) = range(8)


class ImageDesc(C.Structure):      # scnattn_image_desc
    _fields_ = [("offset", C.c_int64), ("H", C.c_int32), ("W", C.c_int32), ("C", C.c_int32), ("tab_h", C.c_int32),
                ("tab_v", C.c_int32), ("reserved", C.c_int32)]


MAX_BANNED, MAX_NGRAM = 64, 8      # SCNATTN_MAX_BANNED, SCNATTN_MAX_NGRAM


class SearchOpts(C.Structure):     # scnattn_search_options
    _fields_ = [("min_length", C.c_int32), ("no_repeat_ngram", C.c_int32), ("n_banned", C.c_int32),
                ("banned", C.c_int32 * MAX_BANNED)]


class Diversity(C.Structure):      # scnattn_diversity
    _fields_ = [("groups", C.c_int32), ("penalty", C.c_float)]


MAX_REQUIRED = 4                   # SCNATTN_MAX_REQUIRED


class Constraints(C.Structure):    # scnattn_constraints; `required` points at a HOST int32 [n_images][4] the caller keeps alive
    _fields_ = [("n_images", C.c_int32), ("pad_token", C.c_int32), ("required", C.c_void_p)]


class SampleFilter(C.Structure):   # scnattn_sample_filter
    _fields_ = [("top_k", C.c_int32), ("top_p", C.c_float)]


class AugmentConfig(C.Structure):  # scnattn_augment_config
    _fields_ = [(k, C.c_float) for k in ("scale_lo", "scale_hi", "ratio_lo", "ratio_hi", "flip_p", "brightness", "contrast",
                                         "saturation")]


AUGMENT_NPARAM = 8                 # SCNATTN_AUGMENT_NPARAM


class TagLossOpts(C.Structure):    # scnattn_tag_loss_options
    _fields_ = [(k, C.c_float) for k in ("gamma_pos", "gamma_neg", "margin")]


_SIGS = {
    "scnattn_version": ([], i32),
    "scnattn_set_option": ([C.c_char_p, i32], i32),
    "scnattn_plan_next": ([C.POINTER(LaunchPlan)], i32),
    "scnattn_profile_collect": ([C.POINTER(C.c_double)], i32),
    "scnattn_seq_workspace": ([C.POINTER(Dims), C.POINTER(Pool), C.POINTER(sz), C.POINTER(sz)], i32),
    "scnattn_seq_fwd": ([vp, C.POINTER(Dims), C.POINTER(Params), vp, vp, vp, vp, vp, vp, vp, vp, vp, vp,
                         C.POINTER(Pool)], i32),
    "scnattn_seq_bwd": ([vp, C.POINTER(Dims), C.POINTER(Params), vp, vp, vp, vp, vp, vp, vp, vp, vp, vp,
                         C.POINTER(Params), vp, vp, C.POINTER(Pool)], i32),
    "scnattn_beam_workspace": ([C.POINTER(Dims), i32, i32, C.POINTER(sz)], i32),
    "scnattn_beam_layout": ([C.POINTER(Dims), i32, i32, C.POINTER(i64)], i32),
    "scnattn_beam_init": ([vp, C.POINTER(Dims), i32, i32, C.POINTER(Params), vp, vp, i32, vp], i32),
    "scnattn_beam_steps": ([vp, C.POINTER(Dims), i32, i32, C.POINTER(Params), vp, i32, i32, i32, vp], i32),
    "scnattn_beam_attn_scores": ([vp, i32, i32, i32, i32, vp, vp, i32, i64, i64, vp, vp, vp, vp, vp], i32),
    "scnattn_beam_attn_context": ([vp, i32, i32, i32, i32, vp, vp, vp, i32, i64, i64, vp, vp, vp, vp, vp], i32),
    "scnattn_beam_row_topk": ([vp, i32, i32, i32, vp, i64, vp, vp, vp, vp, i32], i32),
    "scnattn_beam_merge": ([vp, i32, i32, i32, i32, i32, vp, vp, C.POINTER(vp)], i32),
    "scnattn_beam_advance": ([vp, i32, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp], i32),
    "scnattn_beam_row_topk_ens": ([vp, i32, i32, i32, i32, C.POINTER(vp), C.POINTER(i64), C.POINTER(f32), i32, vp, vp, vp, vp,
                                   i32], i32),
    "scnattn_ensemble_workspace": ([i32, C.POINTER(Dims), i32, i32, i32, C.POINTER(sz)], i32),
    "scnattn_ensemble_layout": ([i32, C.POINTER(Dims), i32, i32, i32, C.POINTER(i64)], i32),
    "scnattn_ensemble_init": ([vp, i32, C.POINTER(Dims), i32, i32, i32, C.POINTER(Params), vp, C.POINTER(vp), i32, vp], i32),
    "scnattn_ensemble_steps": ([vp, i32, C.POINTER(Dims), i32, i32, i32, C.POINTER(Params), vp, C.POINTER(f32), i32, i32, i32,
                                i32, vp], i32),
    "scnattn_beam_workspace_opt": ([C.POINTER(Dims), i32, i32, C.POINTER(SearchOpts), C.POINTER(sz)], i32),
    "scnattn_beam_layout_opt": ([C.POINTER(Dims), i32, i32, C.POINTER(SearchOpts), C.POINTER(i64)], i32),
    "scnattn_beam_init_opt": ([vp, C.POINTER(Dims), i32, i32, C.POINTER(SearchOpts), C.POINTER(Params), vp, vp, i32, vp], i32),
    "scnattn_beam_steps_opt": ([vp, C.POINTER(Dims), i32, i32, C.POINTER(SearchOpts), C.POINTER(Params), vp, i32, i32, i32,
                                vp], i32),
    "scnattn_ensemble_workspace_opt": ([i32, C.POINTER(Dims), i32, i32, i32, C.POINTER(SearchOpts), C.POINTER(sz)], i32),
    "scnattn_ensemble_layout_opt": ([i32, C.POINTER(Dims), i32, i32, i32, C.POINTER(SearchOpts), C.POINTER(i64)], i32),
    "scnattn_ensemble_init_opt": ([vp, i32, C.POINTER(Dims), i32, i32, i32, C.POINTER(SearchOpts), C.POINTER(Params), vp,
                                   C.POINTER(vp), i32, vp], i32),
    "scnattn_ensemble_steps_opt": ([vp, i32, C.POINTER(Dims), i32, i32, i32, C.POINTER(SearchOpts), C.POINTER(Params), vp,
                                    C.POINTER(f32), i32, i32, i32, i32, vp], i32),
    "scnattn_beam_row_topk_opt": ([vp, i32, i32, i32, vp, i64, vp, vp, C.POINTER(SearchOpts), i32, i32, vp, i32, vp, vp,
                                   i32], i32),
    "scnattn_beam_row_topk_ens_opt": ([vp, i32, i32, i32, i32, C.POINTER(vp), C.POINTER(i64), C.POINTER(f32), i32, vp, vp,
                                       C.POINTER(SearchOpts), i32, i32, vp, i32, vp, vp, i32], i32),
    "scnattn_beam_advance_opt": ([vp, i32, i32, i32, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp], i32),
    "scnattn_beam_workspace_div": ([C.POINTER(Dims), i32, i32, C.POINTER(SearchOpts), C.POINTER(Diversity), C.POINTER(sz)],
                                   i32),
    "scnattn_beam_layout_div": ([C.POINTER(Dims), i32, i32, C.POINTER(SearchOpts), C.POINTER(Diversity), C.POINTER(i64)], i32),
    "scnattn_beam_init_div": ([vp, C.POINTER(Dims), i32, i32, C.POINTER(SearchOpts), C.POINTER(Diversity), C.POINTER(Params),
                               vp, vp, i32, vp], i32),
    "scnattn_beam_steps_div": ([vp, C.POINTER(Dims), i32, i32, C.POINTER(SearchOpts), C.POINTER(Diversity), C.POINTER(Params),
                                vp, i32, i32, i32, vp], i32),
    "scnattn_ensemble_workspace_div": ([i32, C.POINTER(Dims), i32, i32, i32, C.POINTER(SearchOpts), C.POINTER(Diversity),
                                        C.POINTER(sz)], i32),
    "scnattn_ensemble_layout_div": ([i32, C.POINTER(Dims), i32, i32, i32, C.POINTER(SearchOpts), C.POINTER(Diversity),
                                     C.POINTER(i64)], i32),
    "scnattn_ensemble_init_div": ([vp, i32, C.POINTER(Dims), i32, i32, i32, C.POINTER(SearchOpts), C.POINTER(Diversity),
                                   C.POINTER(Params), vp, C.POINTER(vp), i32, vp], i32),
    "scnattn_ensemble_steps_div": ([vp, i32, C.POINTER(Dims), i32, i32, i32, C.POINTER(SearchOpts), C.POINTER(Diversity),
                                    C.POINTER(Params), vp, C.POINTER(f32), i32, i32, i32, i32, vp], i32),
    "scnattn_beam_merge_groups": ([vp, i32, i32, i32, f32, i32, i32, i32, vp, vp, C.POINTER(vp)], i32),
    "scnattn_beam_row_topk_groups": ([vp, i32, i32, i32, i32, vp, i64, vp, vp, vp, vp, i32], i32),
    "scnattn_beam_workspace_con": ([C.POINTER(Dims), i32, i32, C.POINTER(SearchOpts), C.POINTER(Constraints), C.POINTER(sz)],
                                   i32),
    "scnattn_beam_layout_con": ([C.POINTER(Dims), i32, i32, C.POINTER(SearchOpts), C.POINTER(Constraints), C.POINTER(i64)],
                                i32),
    "scnattn_beam_init_con": ([vp, C.POINTER(Dims), i32, i32, C.POINTER(SearchOpts), C.POINTER(Constraints),
                               C.POINTER(Params), vp, vp, i32, vp], i32),
    "scnattn_beam_steps_con": ([vp, C.POINTER(Dims), i32, i32, C.POINTER(SearchOpts), C.POINTER(Constraints),
                                C.POINTER(Params), vp, i32, i32, i32, vp], i32),
    "scnattn_ensemble_workspace_con": ([i32, C.POINTER(Dims), i32, i32, i32, C.POINTER(SearchOpts), C.POINTER(Constraints),
                                        C.POINTER(sz)], i32),
    "scnattn_ensemble_layout_con": ([i32, C.POINTER(Dims), i32, i32, i32, C.POINTER(SearchOpts), C.POINTER(Constraints),
                                     C.POINTER(i64)], i32),
    "scnattn_ensemble_init_con": ([vp, i32, C.POINTER(Dims), i32, i32, i32, C.POINTER(SearchOpts), C.POINTER(Constraints),
                                   C.POINTER(Params), vp, C.POINTER(vp), i32, vp], i32),
    "scnattn_ensemble_steps_con": ([vp, i32, C.POINTER(Dims), i32, i32, i32, C.POINTER(SearchOpts), C.POINTER(Constraints),
                                    C.POINTER(Params), vp, C.POINTER(f32), i32, i32, i32, i32, vp], i32),
    "scnattn_beam_row_topk_con": ([vp, i32, i32, i32, vp, i64, vp, vp, C.POINTER(SearchOpts), i32, i32, vp, i32, vp, vp, vp,
                                   vp, vp, vp, i32], i32),
    "scnattn_beam_row_topk_ens_con": ([vp, i32, i32, i32, i32, C.POINTER(vp), C.POINTER(i64), C.POINTER(f32), i32, vp, vp,
                                       C.POINTER(SearchOpts), i32, i32, vp, i32, vp, vp, vp, vp, vp, vp, i32], i32),
    "scnattn_beam_merge_banks": ([vp, i32, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, C.POINTER(vp)], i32),
    "scnattn_rollout_workspace": ([C.POINTER(Dims), i32, i32, i32, C.POINTER(sz)], i32),
    "scnattn_rollout_layout": ([C.POINTER(Dims), i32, i32, i32, C.POINTER(i64)], i32),
    "scnattn_rollout_init": ([vp, C.POINTER(Dims), i32, i32, i32, C.POINTER(Params), vp, vp, i32, vp], i32),
    "scnattn_rollout_steps": ([vp, C.POINTER(Dims), i32, i32, i32, C.POINTER(Params), vp, i32, f32, C.c_uint64, C.c_uint32,
                               i32, i32, i32, vp], i32),
    "scnattn_rollout_pick": ([vp, i32, i32, i32, vp, i64, f32, C.c_uint64, C.c_uint32, i32, i32, i32, i32,
                              C.POINTER(vp)], i32),
    "scnattn_rollout_advance": ([vp, i32, i32, i32, i32, vp, vp, vp, vp, vp], i32),
    "scnattn_rollout_workspace_f": ([C.POINTER(Dims), i32, i32, i32, C.POINTER(SampleFilter), C.POINTER(sz)], i32),
    "scnattn_rollout_layout_f": ([C.POINTER(Dims), i32, i32, i32, C.POINTER(SampleFilter), C.POINTER(i64)], i32),
    "scnattn_rollout_init_f": ([vp, C.POINTER(Dims), i32, i32, i32, C.POINTER(SampleFilter), C.POINTER(Params), vp, vp, i32,
                                vp], i32),
    "scnattn_rollout_steps_f": ([vp, C.POINTER(Dims), i32, i32, i32, C.POINTER(SampleFilter), C.POINTER(Params), vp, i32, f32,
                                 C.c_uint64, C.c_uint32, i32, i32, i32, vp], i32),
    "scnattn_rollout_pick_f": ([vp, i32, i32, i32, vp, i64, f32, C.c_uint64, C.c_uint32, i32, i32, i32, i32, C.POINTER(vp),
                                C.POINTER(SampleFilter), vp, i32], i32),
    "scnattn_rollout_workspace_sc": ([C.POINTER(Dims), i32, i32, i32, C.POINTER(sz)], i32),
    "scnattn_rollout_layout_sc": ([C.POINTER(Dims), i32, i32, i32, C.POINTER(i64)], i32),
    "scnattn_rollout_init_sc": ([vp, C.POINTER(Dims), i32, i32, i32, C.POINTER(Params), vp, vp, i32, vp, i64, vp, vp], i32),
    "scnattn_rollout_steps_sc": ([vp, C.POINTER(Dims), i32, i32, i32, C.POINTER(Params), vp, f32, i32, i32, vp], i32),
    "scnattn_rollout_score": ([vp, i32, i32, i32, vp, i64, f32, i32, i32, C.POINTER(vp), vp, vp, vp], i32),
    "scnattn_rollout_workspace_ss": ([C.POINTER(Dims), i32, i32, i32, C.POINTER(sz)], i32),
    "scnattn_rollout_layout_ss": ([C.POINTER(Dims), i32, i32, i32, C.POINTER(i64)], i32),
    "scnattn_rollout_init_ss": ([vp, C.POINTER(Dims), i32, i32, i32, C.POINTER(Params), vp, vp, i32, vp, i64, vp, vp], i32),
    "scnattn_rollout_steps_ss": ([vp, C.POINTER(Dims), i32, i32, i32, C.POINTER(Params), vp, f32, f32, C.c_uint64, C.c_uint32,
                                  i32, i32, i32, vp], i32),
    "scnattn_rollout_pick_mixed": ([vp, i32, i32, i32, vp, i64, f32, f32, C.c_uint64, C.c_uint32, i32, i32, i32,
                                    C.POINTER(vp), vp, vp, vp], i32),
    "scnattn_sgemm": ([vp, i32, i32, i32, i32, i32, f32, vp, i64, vp, i64, f32, vp, i64, vp, vp, i32, i64, i64, i64], i32),
    "scnattn_sgemm_ws": ([vp, i32, i32, i32, i32, i32, f32, vp, i64, vp, i64, f32, vp, i64, vp, vp, i32, i64, i64, i64,
                          vp, i64], i32),
    "scnattn_cgemm": ([vp, i32, i32, i32, i32, i32, f32, vp, i64, vp, i64, f32, vp, i64, vp, vp, i32, i64, i64, i64,
                       vp, i64, C.POINTER(ConvExtra)], i32),
    "scnattn_cgemm_row_tiles": ([i32], i32),
    "scnattn_conv1x1_fwd": ([vp, i32, i32, i32, vp, vp, vp, C.POINTER(ConvExtra), vp, i64], i32),
    "scnattn_conv1x1_dgrad": ([vp, i32, i32, i32, vp, vp, i32, f32, vp, C.POINTER(ConvExtra), vp, i64], i32),
    "scnattn_conv1x1_wgrad": ([vp, i32, i32, i32, vp, vp, vp, C.POINTER(ConvExtra), vp, i64], i32),
    "scnattn_conv3x3_fwd": ([vp, i32, i32, i32, i32, i32, i32, vp, vp, vp, C.POINTER(ConvExtra), vp, i64], i32),
    "scnattn_conv3x3_dgrad": ([vp, i32, i32, i32, i32, i32, vp, vp, vp, C.POINTER(ConvExtra), vp, i64], i32),
    "scnattn_conv3x3_wgrad": ([vp, i32, i32, i32, i32, i32, i32, vp, vp, vp, vp, i64, i32], i32),
    "scnattn_conv3x3_dgrad_strided": ([vp, i32, i32, i32, i32, i32, i32, vp, vp, vp, vp, i64], i32),
    "scnattn_conv1x1_fwd_bn_eval": ([vp, i32, i32, i32, vp, vp, vp, C.POINTER(BnEval), C.POINTER(ConvExtra), vp, i64], i32),
    "scnattn_conv3x3_fwd_bn_eval": ([vp, i32, i32, i32, i32, i32, i32, vp, vp, vp, C.POINTER(BnEval), C.POINTER(ConvExtra),
                                     vp, i64], i32),
    "scnattn_cgemm_stat_ld": ([i32], i32),
    "scnattn_bn_finalize": ([vp, i64, i32, vp, i32, i32, vp, f32, f32, vp, vp, vp, vp, vp, vp, vp], i32),
    "scnattn_bn_apply_fin": ([vp, i64, i32, vp, vp, i32, vp, i32, i32, vp, f32, f32, vp, vp, i32, vp, vp, vp, vp, vp, vp], i32),
    "scnattn_bn_bwd_reduce": ([vp, i32, i32, vp, vp, vp, i32, vp, vp, i32, vp, i32, vp, C.POINTER(C.c_int)], i32),
    "scnattn_bn_bwd_dx_fin": ([vp, i64, i32, vp, vp, i32, vp, vp, vp, vp, i32, i32, vp, vp, vp], i32),
    "scnattn_bf16_weights": ([vp, i32, vp, vp, i32], i32),
    "scnattn_cgemm16": ([vp, i32, i32, i32, vp, i64, vp, i64, f32, vp, i64, i32, vp, i64, C.POINTER(ConvExtra)], i32),
    "scnattn_conv3x3_fwd16": ([vp, i32, i32, i32, i32, i32, i32, vp, vp, vp, C.POINTER(ConvExtra), vp, i64], i32),
    "scnattn_conv1x1_fwd_bn_eval16": ([vp, i32, i32, i32, vp, vp, vp, C.POINTER(BnEval16), C.POINTER(ConvExtra), vp, i64], i32),
    "scnattn_conv3x3_fwd_bn_eval16": ([vp, i32, i32, i32, i32, i32, i32, vp, vp, vp, C.POINTER(BnEval16), C.POINTER(ConvExtra),
                                       vp, i64], i32),
    "scnattn_conv3x3_dgrad16": ([vp, i32, i32, i32, i32, i32, i32, vp, vp, vp, C.POINTER(ConvExtra), vp, i64], i32),
    "scnattn_wgrad16_3x3": ([vp, i32, i32, i32, i32, i32, vp, vp, vp, vp, i64, i32], i32),
    "scnattn_block16_sizes": ([vp, vp, vp, vp, vp, vp], i32),
    "scnattn_block16_fwd": ([vp, vp], i32),
    "scnattn_block16_bwd": ([vp, vp, vp, vp], i32),
    "scnattn_wgrad16_rows": ([vp, i32, i32, i32, vp, vp, i64, vp, i64, i32, i32, i32, i32, i32, i32, i32, vp, i64, i32], i32),
    "scnattn_stem_tiles": ([i32, i32, i32], i32),
    "scnattn_stem_conv7": ([vp, i32, i32, i32, vp, i64, i64, i64, i64, vp, i64, i64, i64, i64, vp, vp, vp], i32),
    "scnattn_stem_bn_relu_maxpool": ([vp, i32, i32, i32, i32, vp, vp, vp, i32], i32),
    "scnattn_bn_stats_fold": ([vp, i32, i32, vp, f32, f32, vp, vp, vp, vp, vp, vp, vp, vp], i32),
    "scnattn_skinny_gemm": ([vp, i32, i32, i32, i32, vp, i64, i64, vp, i64, i64, vp, i64, i64, i64, i32,
                             C.POINTER(i32)], i32),
    "scnattn_skinny_gemm_bf16w": ([vp, i32, i32, i32, i32, vp, i64, i64, vp, i64, i64, vp, i64, i64, i64, i32,
                                   C.POINTER(i32)], i32),
    "scnattn_skinny_gemm_bf16": ([vp, i32, i32, i32, i32, vp, i64, i64, vp, i64, i64, vp, i64, i64, i64, i32,
                                  C.POINTER(i32)], i32),
    "scnattn_f32_to_bf16": ([vp, i64, vp, vp], i32),
    "scnattn_attn_scores": ([vp, i32, i32, i32, vp, vp, i32, i64, i64, vp, vp, vp, vp, vp], i32),
    "scnattn_attn_context": ([vp, i32, i32, i32, vp, vp, vp, i32, i64, i64, vp, vp, i64, vp, vp, vp, vp], i32),
    "scnattn_mean_pixels": ([vp, i32, i32, i32, vp, vp], i32),
    "scnattn_attn_dalpha": ([vp, i32, i32, i32, vp, vp, vp, i64, vp], i32),
    "scnattn_attn_softmax_bwd": ([vp, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, i64], i32),
    "scnattn_attn_datt1_post_blocks": ([i32, i32], i32),
    "scnattn_attn_datt1_post": ([vp, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp], i32),
    "scnattn_attn_scores_bf16": ([vp, i32, i32, i32, vp, vp, i32, i64, i64, vp, vp, vp, vp, vp], i32),
    "scnattn_attn_context_bf16": ([vp, i32, i32, i32, vp, vp, vp, i32, i64, i64, vp, vp, i64, vp, vp, vp, vp], i32),
    "scnattn_attn_dalpha_bf16": ([vp, i32, i32, i32, vp, vp, vp, i64, vp], i32),
    "scnattn_attn_softmax_bwd_bf16": ([vp, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, i64], i32),
    "scnattn_attn_datt1_post_bf16": ([vp, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp], i32),
    "scnattn_attn_context_pooled": ([vp, i32, i32, i32, vp, i32, C.POINTER(Pool), vp, vp, i32, i64, i64, vp, vp, i64, vp, vp,
                                     vp, vp, vp], i32),
    "scnattn_attn_softmax_bwd_pooled": ([vp, i32, i32, i32, vp, i32, vp, vp, vp, C.POINTER(Pool), vp, vp, i64, vp, vp,
                                         i64], i32),
    "scnattn_weighted_rows": ([vp, i32, i32, i32, vp, vp, vp], i32),
    "scnattn_pool_expand": ([vp, i32, i32, i32, C.POINTER(Pool), vp, vp, vp], i32),
    "scnattn_pool_transpose": ([vp, i32, i32, i32, C.POINTER(Pool), vp, vp], i32),
    "scnattn_add_bcast_rows_w": ([vp, i32, i32, i32, vp, vp, vp], i32),
    "scnattn_scn_mix_fwd": ([vp, i32, i32, vp, i32, i64, i64, vp, vp, i32, i64, i64, vp, vp, vp, vp, vp], i32),
    "scnattn_lstm_fwd": ([vp, i32, i32, vp, i32, i64, i64, i64, vp, vp, vp, vp, vp, vp, vp], i32),
    "scnattn_lstm_bwd": ([vp, i32, i32, i32, vp, vp, i32, i64, i64, vp, vp, vp, vp, vp], i32),
    "scnattn_scn_mix_bwd": ([vp, i32, i32, vp, i32, i64, i64, i64, vp, vp, vp, vp, vp, vp, i64, vp, vp], i32),
    "scnattn_gate_bwd": ([vp, i32, i32, vp, i32, i64, i64, vp, vp, vp, vp, i64], i32),
    "scnattn_transpose2d": ([vp, i32, i32, vp, i64, vp, i64], i32),
    "scnattn_colsum": ([vp, i32, i32, vp, i64, vp, f32], i32),
    "scnattn_mul_bcast": ([vp, i32, i32, i32, vp, vp, vp], i32),
    "scnattn_gather_rows_tm": ([vp, i32, i32, i32, i32, vp, vp, i32, vp], i32),
    "scnattn_scatter_add_rows_tm": ([vp, i32, i32, i32, i32, vp, vp, vp, i32, vp, vp], i32),
    "scnattn_hidden_to_bm": ([vp, i32, i32, i32, vp, vp, vp, vp, vp], i32),
    "scnattn_hidden_from_bm": ([vp, i32, i32, i32, vp, vp, vp, vp], i32),
    "scnattn_colsum_masked": ([vp, i32, i32, vp, i64, vp, vp, f32], i32),
    "scnattn_reduce_slabs": ([vp, i32, i32, vp, i32, i64, i64, vp], i32),
    "scnattn_copy2d": ([vp, i32, i32, vp, i64, vp, i64], i32),
    "scnattn_add_bcast_rows": ([vp, i32, i32, i32, vp, f32, vp], i32),
    "scnattn_pool_permute_fwd": ([vp, i32, i32, i32, i32, i32, i32, vp, i64, i64, i64, i64, vp], i32),
    "scnattn_pool_permute_bwd": ([vp, i32, i32, i32, i32, i32, i32, vp, vp, i64, i64, i64, i64], i32),
    "scnattn_caption_loss_fwd": ([vp, i32, i32, i32, i32, vp, vp, i64, vp, i64, vp, f32, vp, vp, vp, vp, vp], i32),
    "scnattn_caption_loss_metrics_fwd": ([vp, i32, i32, i32, i32, vp, vp, i64, vp, i64, vp, f32, vp, vp, vp, vp, vp,
                                          i32, vp, vp, i64, vp], i32),
    "scnattn_caption_loss_bwd": ([vp, i32, i32, i32, i32, vp, vp, i64, vp, i64, vp, vp, f32, vp, vp, vp], i32),
    "scnattn_caption_loss_weighted_fwd": ([vp, i32, i32, i32, i32, vp, vp, i64, vp, i64, vp, vp, f32, vp, vp, vp, vp, vp], i32),
    "scnattn_caption_loss_weighted_bwd": ([vp, i32, i32, i32, i32, vp, vp, i64, vp, i64, vp, vp, vp, f32, vp, vp, vp], i32),
    "scnattn_tag_pool_fwd": ([vp, i32, i32, i32, vp, i32, i64, i64, i64, vp, i64, vp, i64], i32),
    "scnattn_tag_pool_bwd": ([vp, i32, i32, i32, vp, i64, vp, i64, vp, i32, i64, i64, i64], i32),
    "scnattn_bce_fwd": ([vp, i32, i32, vp, i64, vp, i64, vp, i64, vp, vp], i32),
    "scnattn_bce_bwd": ([vp, i32, i32, vp, i64, vp, i64, vp, vp, i64], i32),
    "scnattn_tagloss_fwd": ([vp, i32, i32, vp, i64, vp, i64, vp, C.POINTER(TagLossOpts), vp, i64, vp, vp], i32),
    "scnattn_tagloss_bwd": ([vp, i32, i32, vp, i64, vp, i64, vp, C.POINTER(TagLossOpts), vp, vp, i64], i32),
    "scnattn_u8_gather_normalize": ([vp, vp, i64, vp, i64, i32, i64, vp, vp, i32, i32], i32),
    "scnattn_u8_mean_grey": ([vp, vp, i64, i64, vp, vp], i32),
    "scnattn_augment_draw": ([vp, i64, vp, i32, C.c_uint64, C.POINTER(AugmentConfig), i32, i32, vp], i32),
    "scnattn_u8_gather_augment": ([vp, vp, i64, vp, i64, i32, i32, vp, vp, C.POINTER(C.c_float), C.POINTER(C.c_float), vp,
                                   i32, i32], i32),
    "scnattn_resize_table_ints": ([i32, i32], i64),
    "scnattn_u8_resize_bilinear": ([vp, vp, i64, vp, vp, i32, vp, i64, i32, i32, vp, vp, i32, i32], i32),
    "scnattn_u8_resize_taps": ([vp, vp, i64, vp, vp, i32, vp, vp, i64, i32, i32, vp, vp, i32, i32], i32),
    "scnattn_attn_strips": ([i32], i32),
    "scnattn_attn_expand": ([vp, vp, i32, i32, i32, vp, vp, i32, i32, vp, vp, vp], i32),
    "scnattn_attn_overlay": ([vp, vp, i32, i32, i32, vp, vp, i32, i32, vp, vp, vp, i32, vp, vp, vp, vp], i32),
    "scnattn_text_max_len": ([], i32),
    "scnattn_text_ngram_stats": ([vp, i32, i32, vp, i32, vp, vp, i32, vp, vp, i32, vp, i32, vp], i32),
    "scnattn_text_lcs": ([vp, i32, i32, vp, i32, vp, vp, i32, vp, vp, i32, vp, i32, vp, vp, vp], i32),
    "scnattn_text_ref_keys": ([vp, i32, i32, i32, vp, i32, vp, vp, i32, vp, vp], i32),
    "scnattn_text_cider": ([vp, i32, i32, vp, i32, vp, vp, i32, vp, vp, i32, vp, i32, vp, vp, vp, i64, vp, vp, vp], i32),
    "scnattn_tag_store_size": ([i32, i64, C.POINTER(sz), C.POINTER(sz)], i32),
    "scnattn_tag_rows": ([vp, i32, i32, vp, i64, vp, i32, i64, i64, i64, C.POINTER(C.c_int32), i32, vp, vp, vp, vp, vp, vp], i32),
    "scnattn_tag_cols": ([vp, i32, i64, i64, vp, vp, C.POINTER(C.c_float), i32, vp, vp, vp, vp], i32),
    "scnattn_tag_finalize": ([vp, i32, i64, C.POINTER(C.c_int32), i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp], i32),
    "scnattn_bn_workspace_floats": ([i32], i32),
    "scnattn_bn_stats": ([vp, i32, i32, vp, i32, f32, f32, vp, vp, vp, vp, vp], i32),
    "scnattn_bn_apply": ([vp, i32, i32, vp, vp, i32, vp, vp, vp, vp, i32, vp], i32),
    "scnattn_bn_bwd": ([vp, i32, i32, vp, vp, vp, i32, vp, vp, vp, vp, i32, i32, vp, vp, vp, vp, vp], i32),
    "scnattn_dp_unique_id": ([C.c_char_p], i32),
    "scnattn_dp_comm_create": ([C.c_char_p, i32, i32, C.POINTER(vp)], i32),
    "scnattn_dp_comm_allreduce_bucket": ([vp, vp, vp, i64], i32),
    "scnattn_dp_comm_finish": ([vp, vp], i32),
    "scnattn_dp_comm_set_stream": ([vp, vp], i32),
    "scnattn_dp_comm_world": ([vp], i32),
    "scnattn_dp_comm_destroy": ([vp], i32),
    "scnattn_clamp_adam": ([vp, i64, vp, vp, vp, vp, f64, f64, f64, f64, i32, f64, f64], i32),
}

BEAM_NOFF = 13      # SCNATTN_BEAM_NOFF
BEAM_NOFF_OPT = 14  # SCNATTN_BEAM_NOFF_OPT
BEAM_NOFF_CON = 16  # SCNATTN_BEAM_NOFF_CON
ROLLOUT_NOFF = 8    # SCNATTN_ROLLOUT_NOFF
ROLLOUT_NOFF_F = 9  # SCNATTN_ROLLOUT_NOFF_F
ROLLOUT_NOFF_SC = 11  # SCNATTN_ROLLOUT_NOFF_SC
ROLLOUT_NOFF_SS = 11  # SCNATTN_ROLLOUT_NOFF_SS
MAX_BEAM = 8
MAX_ENSEMBLE = 4    # SCNATTN_MAX_ENSEMBLE
RESIZE_MAX_DIM = 16384      # SCNATTN_RESIZE_MAX_DIM
OVERLAY_MAX_MAP, OVERLAY_MAX_OUT = 32, 1024      # SCNATTN_OVERLAY_MAX_MAP, SCNATTN_OVERLAY_MAX_OUT
TEXT_MAX_LEN, TEXT_MAX_REFS, TEXT_CIDER_MAX_TOKEN = 128, 32, 65534      # SCNATTN_TEXT_MAX_LEN, _MAX_REFS, _CIDER_MAX_TOKEN
# SCNATTN_TAG_MAX_S, _MAX_K, _MAX_THRESHOLDS, _MAX_IMAGES, _SUMMARY_LEN
TAG_MAX_S, TAG_MAX_K, TAG_MAX_THRESHOLDS, TAG_MAX_IMAGES, TAG_SUMMARY_LEN = 4096, 4, 8, 1 << 30, 64

EXPORTS = tuple(_SIGS) + ("scnattn_last_error",)


def lib():
    """Load (once) and return the ctypes handle.  Raises RuntimeError when the .so is absent."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is None:
            if not os.path.exists(LIB_PATH):
                raise RuntimeError(
                    "libscnattn.so not found at %s -- build it with `python -c 'import __graft_entry__ as g; "
                    "g.build()'` or `make -C indonesian-image-captioning_amd/csrc`. There is no CPU fallback." % LIB_PATH)
            h = C.CDLL(LIB_PATH)
            for name, (args, res) in _SIGS.items():
                fn = getattr(h, name)
                fn.argtypes = args
                fn.restype = res
            h.scnattn_last_error.argtypes = []
            h.scnattn_last_error.restype = C.c_char_p
            # A/B runs without touching code: SCNATTN_OPTIONS="cgemm_combine=0,cgemm_mi=2" (scnattn_set_option names)
            for item in filter(None, os.environ.get("SCNATTN_OPTIONS", "").split(",")):
                name, _, val = item.partition("=")
                if h.scnattn_set_option(name.strip().encode(), int(val)) != 0:
                    raise RuntimeError("SCNATTN_OPTIONS: %s" % h.scnattn_last_error().decode())
            _lib = h
    return _lib


def check(rc, what):
    if rc != 0:
        msg = lib().scnattn_last_error()
        raise RuntimeError("%s failed (code %d): %s" % (what, rc, msg.decode() if msg else "?"))


def call(name, *args):
    check(getattr(lib(), name)(*args), name)


def plan(name, *args):
    """The launch plan of the call `name(*args)` (scnattn_plan_next): its argument checks and its dispatch policy run, nothing
    is launched, no HIP API is called -- the pointers may be host memory.  A refusal raises as the call would; an empty
    problem gives family == PLAN_NONE."""
    h, out = lib(), LaunchPlan()
    try:
        h.scnattn_plan_next(C.byref(out))
        check(getattr(h, name)(*args), name)
    finally:
        h.scnattn_plan_next(None)
    return out


def ptr(t):
    """Raw device pointer of a tensor (None -> NULL)."""
    if t is None:
        return None
    return C.c_void_p(t.data_ptr())


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def stream_of(t):
    """The current HIP stream of the tensor's device, as the void* the C ABI takes."""
    if _raw_stream is not None:     # ~10x cheaper than building a torch.cuda.Stream object per call
        return C.c_void_p(_raw_stream(t.device.index if t.device.index is not None else torch.cuda.current_device()))
    return C.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def require_cuda(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError("scnattn: the HIP path needs tensors on an MI355X device (got a %s tensor); "
                               "there is no CPU fallback" % t.device.type)


def f32c(t):
    """float32 + contiguous (no copy when already so)."""
    if t is None:
        return None
    if t.dtype != torch.float32:
        t = t.float()
    return t.contiguous()
