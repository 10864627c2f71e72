"""ctypes binding of libtavhip.so: one table per public header under include/, the tables listed in ABIS.

The library is the product: there is no CPU or eager-PyTorch fallback.  `lib()` raises if the shared object has not
been built (run `python -c "import __graft_entry__ as g; g.build()"` or `make -C multi-modal-emotion_amd/csrc`).
Every wrapper turns a non-zero return code into RuntimeError carrying tav_error_string().
"""
import ctypes as C
import os
from typing import NamedTuple

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("TAV_LIB") or os.path.join(_HERE, "libtavhip.so")      # TAV_LIB: developer knob, A/B of two builds (tools/ab_build.sh)

TAV_F32, TAV_BF16, TAV_FP8, TAV_U8, TAV_I16 = 0, 1, 2, 3, 4
ABI_VERSION = 7

i32, i64, f32, vp = C.c_int32, C.c_int64, C.c_float, C.c_void_p


class GemmNTArgs(C.Structure):
    _fields_ = [("A", vp), ("B", vp), ("C", vp), ("C_pre", vp), ("bias", vp), ("gelu_in", vp), ("resid", vp),
                ("M", i64), ("N", i64), ("K", i64),
                ("lda", i64), ("ldb", i64), ("ldc", i64), ("ld_pre", i64), ("ld_gelu_in", i64), ("ld_resid", i64),
                ("nzb", i32), ("nzg", i32),
                ("a_zb", i64), ("a_zg", i64), ("b_zb", i64), ("b_zg", i64), ("c_zb", i64), ("c_zg", i64), ("bias_zg", i64),
                ("in_dtype", i32), ("out_dtype", i32), ("act", i32), ("accumulate", i32), ("alpha", f32),
                ("a_dequant", vp), ("b_dequant", vp), ("gelu_zb", i64), ("tile_m_hint", i32)]


class GemmTNArgs(C.Structure):
    _fields_ = [("A", vp), ("B", vp), ("slabs", vp), ("out", vp), ("dbias", vp), ("bias_partials", vp),
                ("N1", i64), ("N2", i64), ("lda", i64), ("ldb", i64), ("rows_per_batch", i64), ("nbatch", i64),
                ("a_zb", i64), ("b_zb", i64), ("chunk_rows", i32), ("nsplit", i32), ("perm_inner", i32), ("perm_outer", i32),
                ("dtype", i32), ("accumulate", i32), ("scale", f32)]


class GemmTNProblem(C.Structure):
    _fields_ = [("A", vp), ("B", vp), ("out", vp), ("dbias", vp), ("N1", i64), ("N2", i64), ("lda", i64), ("ldb", i64)]


class AttnArgs(C.Structure):
    _fields_ = [("q", vp), ("k", vp), ("v", vp), ("o", vp), ("key_mask", vp), ("lse", vp), ("corr", vp), ("o_soft", vp),
                ("dout", vp), ("dq", vp), ("dk", vp), ("dv", vp), ("delta", vp),
                ("B", i64), ("S", i64), ("nheads", i64),
                ("ld_q", i64), ("ld_k", i64), ("ld_v", i64), ("ld_o", i64), ("ld_do", i64), ("ld_dq", i64), ("ld_dk", i64), ("ld_dv", i64),
                ("dtype", i32), ("mask_mode", i32), ("scale", f32), ("q_prescaled", i32)]


class LnArgs(C.Structure):
    _fields_ = [("x", vp), ("x_dtype", i32), ("gamma", vp), ("beta", vp), ("y_f32", vp), ("y_lp", vp), ("lp_dtype", i32),
                ("mean", vp), ("rstd", vp),
                ("dy", vp), ("dy_dtype", i32), ("dx_add", vp), ("dx_f32", vp), ("dx_lp", vp),
                ("dgamma", vp), ("dbeta", vp), ("partials", vp), ("accumulate_params", i32),
                ("rows", i64), ("W", i64), ("ld_x", i64), ("ld_y", i64), ("ld_dy", i64), ("ld_dx", i64), ("eps", f32), ("act", i32),
                ("defer_param_reduce", i32)]


class LnReduceItem(C.Structure):
    _fields_ = [("partials", vp), ("dgamma", vp), ("dbeta", vp), ("nblocks", i32), ("W", i32), ("accumulate", i32), ("pad_", i32)]


LN_REDUCE_MAX = 64


class TextEmbedArgs(C.Structure):
    _fields_ = [("ids", vp), ("word", vp), ("pos", vp), ("type", vp), ("gamma", vp), ("beta", vp), ("pre", vp), ("pos_ids", vp),
                ("y_f32", vp), ("y_lp", vp), ("lp_dtype", i32), ("mean", vp), ("rstd", vp),
                ("B", i64), ("S", i64), ("W", i64), ("vocab", i64), ("max_pos", i64), ("pad_id", i32), ("eps", f32)]


class ClipXform(C.Structure):
    _fields_ = [("src_dtype", i32), ("T", i32), ("H", i32), ("W", i32), ("sT", i64), ("sH", i64), ("sW", i64), ("sC", i64),
                ("nf", i32), ("frame", i32 * 32), ("crop_top", i32), ("crop_left", i32), ("crop_h", i32), ("crop_w", i32),
                ("mid_h", i32), ("mid_w", i32), ("out_h", i32), ("out_w", i32), ("hflip", i32), ("vflip", i32),
                ("scale", f32 * 3), ("shift", f32 * 3)]


class ResampleArgs(C.Structure):
    _fields_ = [("src_dtype", i32), ("C", i32), ("L", i64), ("sC", i64), ("sL", i64), ("o", i32), ("n", i32), ("width", i32), ("ntap", i32),
                ("first_max", i32), ("reserved", i32), ("T_row", i64)]


_SIGS = {
    "tav_version": (C.c_int, []),
    "tav_error_string": (C.c_char_p, [C.c_int]),
    "tav_gemm_nt": (C.c_int, [C.POINTER(GemmNTArgs), vp]),
    "tav_gemm_nt_schedule": (C.c_int, [C.POINTER(GemmNTArgs), C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]),
    "tav_gemm_tn_splits": (C.c_int, [i64, i64, i64, i64, C.POINTER(i32), C.POINTER(i32)]),
    "tav_gemm_tn": (C.c_int, [C.POINTER(GemmTNArgs), vp]),
    "tav_gemm_tn_grouped": (C.c_int, [C.POINTER(GemmTNProblem), i32, i64, i32, vp]),
    "tav_gemm_tn_grouped_ws_bytes": (C.c_int64, [C.POINTER(GemmTNProblem), i32, i64, i32, i32]),
    "tav_gemm_tn_grouped_ws": (C.c_int, [C.POINTER(GemmTNProblem), i32, i64, i32, vp, i64, i32, vp]),
    "tav_colsum": (C.c_int, [vp, i32, i64, i64, i64, vp, i32, vp, i32, vp]),
    "tav_fp8_amax_partials": (C.c_int, [i64, i64]),
    "tav_fp8_amax": (C.c_int, [vp, i32, i64, i64, i64, vp, vp, vp]),
    "tav_fp8_quantize": (C.c_int, [vp, i32, i64, i64, i64, vp, vp, i64, vp, i64, i64, vp]),
    "tav_fp8_quantize_delayed": (C.c_int, [vp, i32, i64, i64, i64, vp, vp, i64, vp, i64, i64, vp]),
    "tav_fp8_roll_states": (C.c_int, [vp, i64, vp]),
    "tav_splitk_reduce": (C.c_int, [vp, vp, i32, i64, i32, vp]),
    "tav_comm_rccl_version": (C.c_int, [C.POINTER(i32)]),
    "tav_comm_unique_id": (C.c_int, [vp]),
    "tav_comm_init_rank": (C.c_int, [C.POINTER(vp), i32, vp, i32]),
    "tav_comm_destroy": (C.c_int, [vp]),
    "tav_allreduce_bucket": (C.c_int, [vp, i64, i32, vp, vp]),
    "tav_attn_fwd": (C.c_int, [C.POINTER(AttnArgs), vp]),
    "tav_attn_bwd": (C.c_int, [C.POINTER(AttnArgs), vp]),
    "tav_attn_fwd_len": (C.c_int, [C.POINTER(AttnArgs), vp, vp]),
    "tav_attn_bwd_len": (C.c_int, [C.POINTER(AttnArgs), vp, vp]),
    "tav_attn_probs": (C.c_int, [C.POINTER(AttnArgs), vp, vp, i64, vp]),
    "tav_head_scale": (C.c_int, [vp, vp, vp, i32, vp, i64, f32, i64, i64, i64, i64, i64, i64, vp]),
    "tav_ln_fwd": (C.c_int, [C.POINTER(LnArgs), vp]),
    "tav_ln_bwd": (C.c_int, [C.POINTER(LnArgs), vp]),
    "tav_ln_bwd_partials": (C.c_int, [i64]),
    "tav_ln_param_reduce_multi": (C.c_int, [C.POINTER(LnReduceItem), i32, vp]),
    "tav_cast_weight": (C.c_int, [vp, i64, i64, vp, i64, vp, i64, i32, vp]),
    "tav_cast_weights_multi": (C.c_int, [vp, i32, i32, vp]),
    "tav_cast_conv_weight": (C.c_int, [vp, i64, i64, i64, vp, vp, vp, i64, i32, vp]),
    "tav_zero_pad_rows": (C.c_int, [vp, i32, i64, i64, i64, i64, vp]),
    "tav_cast2d": (C.c_int, [vp, i32, i64, vp, i32, i64, i64, i64, vp]),
    "tav_transpose2d": (C.c_int, [vp, vp, i32, i64, i64, i64, vp]),
    "tav_add_f32": (C.c_int, [vp, vp, vp, vp, i32, i64, vp]),
    "tav_fill_f32": (C.c_int, [vp, f32, i64, vp]),
    "tav_embed_add_fwd": (C.c_int, [vp, vp, vp, vp, i64, i64, i64, vp]),
    "tav_embed_add_bwd": (C.c_int, [vp, vp, vp, vp, i64, i64, i64, i32, vp]),
    "tav_embed_add_bwd_parts": (C.c_int, [i64]),
    "tav_text_embed_fwd": (C.c_int, [C.POINTER(TextEmbedArgs), vp]),
    "tav_scatter_add_rows": (C.c_int, [vp, vp, vp, i64, i64, i64, vp]),
    "tav_gather_rows": (C.c_int, [vp, vp, vp, i64, i64, i64, vp]),
    "tav_patchify": (C.c_int, [vp, vp, vp, i32, i64, i64, i64, i64, i64, vp]),
    "tav_video_clip_transform": (C.c_int, [vp, vp, C.POINTER(ClipXform), vp]),
    "tav_audio_resample": (C.c_int, [vp, vp, vp, vp, vp, C.POINTER(ResampleArgs), vp]),
    "tav_audio_resample_tile": (C.c_int, [i32, i32, i32]),
    "tav_mask_to_index": (C.c_int, [vp, i32, vp, vp, i64, i64, i64, vp]),
    "tav_ragged_lens": (C.c_int, [vp, vp, vp, vp, vp, i64, i64, i64, i64, i64, vp]),
    "tav_mean_pool_fwd": (C.c_int, [vp, vp, i64, i64, i64, vp]),
    "tav_mean_pool_bwd": (C.c_int, [vp, vp, vp, i32, i64, i64, i64, vp]),
    "tav_mean_pool_fwd_len": (C.c_int, [vp, vp, vp, i64, i64, i64, vp]),
    "tav_mean_pool_bwd_len": (C.c_int, [vp, vp, vp, i32, vp, i64, i64, i64, vp]),
    "tav_head_fwd": (C.c_int, [vp, vp, vp, vp, i64, i64, i64, vp]),
    "tav_head_bwd": (C.c_int, [vp, vp, vp, vp, vp, vp, i64, i64, i64, i32, vp]),
    "tav_tanh_fwd": (C.c_int, [vp, vp, i64, vp]),
    "tav_tanh_bwd": (C.c_int, [vp, vp, vp, i64, vp]),
    "tav_cross_entropy": (C.c_int, [vp, vp, vp, vp, vp, i64, i64, f32, vp]),
    "tav_step_stats": (C.c_int, [vp, vp, vp, vp, vp, vp, vp, i64, i64, vp]),
    "tav_dropout_fwd": (C.c_int, [vp, vp, vp, i64, f32, C.c_uint64, C.c_uint64, vp]),
    "tav_dropout_fwd_dev": (C.c_int, [vp, vp, vp, i64, f32, vp, C.c_uint64, vp]),
    "tav_dropout_bwd": (C.c_int, [vp, vp, vp, i64, f32, vp]),
    "tav_specaug_draw": (C.c_int, [vp, vp, vp, i64, i64, f32, i64, i64, C.c_uint64, C.c_uint64, vp]),
    "tav_specaug_draw_dev": (C.c_int, [vp, vp, vp, i64, i64, f32, i64, i64, vp, C.c_uint64, vp]),
    "tav_specaug_fwd": (C.c_int, [vp, vp, vp, vp, vp, i64, i64, i64, vp]),
    "tav_specaug_bwd_ws_bytes": (C.c_int64, [i64, i64]),
    "tav_specaug_bwd": (C.c_int, [vp, vp, vp, vp, vp, vp, i64, i64, i64, i64, vp]),
    "tav_conv0_fwd": (C.c_int, [vp, vp, vp, vp, i32, i64, i64, i64, i64, i64, i64, vp]),
    "tav_conv0_bwd_w": (C.c_int, [vp, vp, i32, vp, vp, vp, i64, i64, i64, i64, i64, i64, i32, vp]),
    "tav_conv0_bwd_partials": (C.c_int, [i64, i64, i64, i64]),
    "tav_gn_workspace_floats": (C.c_int, [i64, i64]),
    "tav_gn_gelu_fwd": (C.c_int, [vp, vp, i32, vp, vp, vp, vp, i64, i64, i64, f32, vp]),
    "tav_gn_gelu_bwd": (C.c_int, [vp, vp, vp, i32, vp, vp, vp, vp, vp, vp, i64, i64, i64, i32, vp]),
    "tav_gelu_fwd": (C.c_int, [vp, vp, i32, i64, vp]),
    "tav_gelu_bwd": (C.c_int, [vp, vp, vp, i32, i64, vp]),
    "tav_col2im_1d": (C.c_int, [vp, vp, vp, i32, i64, i64, i64, i64, i64, i64, vp]),
    "tav_group_pad": (C.c_int, [vp, i32, vp, i32, i64, i64, i64, i64, i64, i64, vp]),
    "tav_weight_norm_partials": (C.c_int, [i64, i64]),
    "tav_weight_norm_fwd": (C.c_int, [vp, vp, vp, vp, vp, vp, i32, i64, i64, i64, vp]),
    "tav_weight_norm_bwd": (C.c_int, [vp, vp, vp, vp, vp, vp, vp, i64, i64, i64, i32, vp]),
    "tav_sumsq_partials": (C.c_int, [i32]),
    "tav_sumsq_multi": (C.c_int, [vp, vp, i32, vp, vp, vp]),
    "tav_clip_coef": (C.c_int, [vp, f32, vp, vp, vp]),
    "tav_adamw_multi": (C.c_int, [vp, vp, vp, vp, vp, i32, vp, vp, f32, f32, f32, f32, vp, vp, vp]),
    "tav_optim_chunk_elems": (C.c_int, []),
    "tav_sumsq_chunked": (C.c_int, [vp, vp, vp, i32, i32, vp, vp, vp]),
    "tav_sum_partials": (C.c_int, [vp, i64, vp, vp]),
    "tav_adamw_chunked": (C.c_int, [vp, vp, vp, vp, vp, vp, i32, i32, vp, vp, f32, f32, f32, f32, vp, vp, vp]),
    "tav_optim_max_groups": (C.c_int, []),
    "tav_adamw_chunked_groups": (C.c_int, [vp, vp, vp, vp, vp, vp, i32, i32, vp, vp, vp, i32, f32, f32, f32, vp, vp, vp]),
}

# Every public header after include/tavhip.h has a table, a version constant and a version function of its own and one row in ABIS
# below; lib() binds and checks all rows alike.  declared_symbols() stays the main table alone: the symbol set of include/tavhip.h is
# pinned by a recorded table ("Adding an entry-point family").

# include/tavhip_align.h: the forced-alignment entry points.
ALIGN_ABI_VERSION = 1


class AlignPlan(C.Structure):
    _fields_ = [("block", i32), ("tokens_per_thread", i32), ("frames_per_stage", i32), ("bits_frames", i32), ("lds_bytes", i64), ("ws_bytes_per_row", i64)]


class CtcAlignArgs(C.Structure):
    _fields_ = [("emission", vp), ("tokens", vp), ("n_frames", vp), ("n_tokens", vp), ("trellis", vp), ("path_token", vp), ("path_prob", vp),
                ("seg", vp), ("seg_score", vp), ("span", vp), ("workspace", vp), ("workspace_bytes", i64),
                ("B", i64), ("Tmax", i64), ("Nmax", i64), ("V", i64), ("ld", i64), ("blank_id", i32), ("reserved", i32)]


_ALIGN_SIGS = {
    "tav_align_version": (C.c_int, []),
    "tav_ctc_log_softmax": (C.c_int, [vp, vp, i64, i64, i64, i64, vp]),
    "tav_ctc_align_plan": (C.c_int, [i64, i64, i64, C.POINTER(AlignPlan)]),
    "tav_ctc_align_ws_bytes": (C.c_int64, [i64, i64, i64, i64]),
    "tav_ctc_align": (C.c_int, [C.POINTER(CtcAlignArgs), vp]),
}

# include/tavhip_rnn.h: the recurrent entry points (LSTM recurrence, log-sigmoid).
RNN_ABI_VERSION = 1


class LstmPlan(C.Structure):
    _fields_ = [("block", i32), ("rows_per_wg", i32), ("Hp", i32), ("tiles_per_wave", i32), ("lds_bytes", i64), ("ws_gates_off", i64),
                ("ws_cell_off", i64), ("ws_bytes", i64)]


class LstmFwdArgs(C.Structure):
    _fields_ = [("xproj", vp), ("w_hh", vp), ("b_hh", vp), ("h0", vp), ("c0", vp), ("y", vp), ("workspace", vp), ("workspace_bytes", i64),
                ("B", i64), ("T", i64), ("H", i64), ("xp_stride_b", i64), ("xp_stride_t", i64), ("dtype", i32), ("reserved", i32)]


class LstmBwdArgs(C.Structure):
    _fields_ = [("dy", vp), ("dh_T", vp), ("dc_T", vp), ("w_hh_t", vp), ("workspace", vp), ("workspace_bytes", i64), ("dz", vp), ("dh0", vp),
                ("dc0", vp), ("dc_trace", vp), ("B", i64), ("T", i64), ("H", i64), ("dy_stride_b", i64), ("dy_stride_t", i64),
                ("dz_stride_b", i64), ("dz_stride_t", i64), ("dtype", i32), ("reserved", i32)]


_RNN_SIGS = {
    "tav_rnn_version": (C.c_int, []),
    "tav_lstm_get_plan": (C.c_int, [i64, i64, i64, i32, C.POINTER(LstmPlan)]),
    "tav_lstm_ws_bytes": (C.c_int64, [i64, i64, i64, i32]),
    "tav_lstm_fwd": (C.c_int, [C.POINTER(LstmFwdArgs), vp]),
    "tav_lstm_bwd": (C.c_int, [C.POINTER(LstmBwdArgs), vp]),
    "tav_logsigmoid_fwd": (C.c_int, [vp, vp, i64, vp]),
    "tav_logsigmoid_bwd": (C.c_int, [vp, vp, vp, i64, vp]),
}

# include/tavhip_conv.h: the dense 3-D convolution entry points (Conv3d forward / input gradient / weight gradient, flatten + Linear,
# sigmoid).
CONV_ABI_VERSION = 1


class Conv3dPlan(C.Structure):
    _fields_ = [("cin_p", i32), ("cout_p", i32), ("tw", i32), ("th", i32), ("block", i32), ("n_tiles", i32), ("n_passes", i32), ("k_steps", i32),
                ("kp", i64), ("lds_bytes", i64), ("od", i64), ("oh", i64), ("ow", i64), ("patches", i64),
                ("wg_block", i32), ("wg_ci_tiles", i32), ("wg_co_tiles", i32), ("wg_groups", i32), ("wg_nslabs", i32), ("reserved", i32),
                ("wg_lds_bytes", i64), ("wg_slab_floats", i64)]


class Conv3dFwdArgs(C.Structure):
    _fields_ = [("x", vp), ("w", vp), ("bias", vp), ("y", vp), ("g", vp), ("B", i64), ("D", i64), ("H", i64), ("W", i64), ("Cin", i64), ("Cout", i64),
                ("pad", i32), ("gelu", i32), ("dtype", i32), ("reserved", i32)]


class Conv3dWgradArgs(C.Structure):
    _fields_ = [("x", vp), ("dz", vp), ("workspace", vp), ("workspace_bytes", i64), ("dw", vp), ("db", vp),
                ("B", i64), ("D", i64), ("H", i64), ("W", i64), ("Cin", i64), ("Cout", i64), ("nslabs", i32), ("dtype", i32)]


class FlatLinearFwdArgs(C.Structure):
    _fields_ = [("x", vp), ("w", vp), ("bias", vp), ("out", vp), ("workspace", vp), ("workspace_bytes", i64),
                ("B", i64), ("S", i64), ("C", i64), ("O", i64), ("nparts", i32), ("dtype", i32)]


class FlatLinearBwdArgs(C.Structure):
    _fields_ = [("x", vp), ("w", vp), ("dy", vp), ("dx", vp), ("dw", vp), ("db", vp), ("B", i64), ("S", i64), ("C", i64), ("O", i64),
                ("dtype", i32), ("reserved", i32)]


_CONV_SIGS = {
    "tav_conv_version": (C.c_int, []),
    "tav_conv3d_get_plan": (C.c_int, [i64, i64, i64, i64, i64, i64, i32, i32, C.POINTER(Conv3dPlan)]),
    "tav_conv3d_wgrad_ws_bytes": (C.c_int64, [i64, i64, i64, i64, i64, i64, i32, i32]),
    "tav_conv3d_pack_input": (C.c_int, [vp, vp, i64, i64, i64, i64, i64, i32, vp]),
    "tav_conv3d_pack_weight": (C.c_int, [vp, vp, i64, i64, i32, i32, vp]),
    "tav_conv3d_fwd": (C.c_int, [C.POINTER(Conv3dFwdArgs), vp]),
    "tav_conv3d_dz": (C.c_int, [vp, vp, vp, i64, i32, vp]),
    "tav_conv3d_wgrad": (C.c_int, [C.POINTER(Conv3dWgradArgs), vp]),
    "tav_flat_linear_parts": (C.c_int32, [i64]),
    "tav_flat_linear_ws_bytes": (C.c_int64, [i64, i64, i64, i32]),
    "tav_flat_linear_fwd": (C.c_int, [C.POINTER(FlatLinearFwdArgs), vp]),
    "tav_flat_linear_bwd": (C.c_int, [C.POINTER(FlatLinearBwdArgs), vp]),
    "tav_sigmoid_fwd": (C.c_int, [vp, vp, i64, vp]),
    "tav_sigmoid_bwd": (C.c_int, [vp, vp, vp, i64, vp]),
}


class Abi(NamedTuple):
    """One public header and its binding.  `version` is the constant as it stood at import, for readers of the table; lib() reads the
    constant named `version_const` when it is called, so that a changed constant is what the loaded library is held to."""
    header: str            # file name under include/ (under csrc/ for a row of PRIVATE_ABIS)
    version_fn: str        # the exported function that returns the library's version of this family
    version_const: str     # the module constant of this file that holds the binding's version
    version: int
    sigs: dict             # name -> (restype, argtypes): the table object itself
    structs: dict          # C struct name -> ctypes Structure class
    what: str              # the family's word in the version message ("" for the main header)


ABIS = (
    Abi("tavhip.h", "tav_version", "ABI_VERSION", ABI_VERSION, _SIGS,
        {"tav_gemm_nt_args": GemmNTArgs, "tav_gemm_tn_args": GemmTNArgs, "tav_gemm_tn_problem": GemmTNProblem, "tav_attn_args": AttnArgs,
         "tav_ln_args": LnArgs, "tav_ln_reduce_item": LnReduceItem, "tav_text_embed_args": TextEmbedArgs, "tav_clip_xform": ClipXform,
         "tav_resample_args": ResampleArgs}, ""),
    Abi("tavhip_align.h", "tav_align_version", "ALIGN_ABI_VERSION", ALIGN_ABI_VERSION, _ALIGN_SIGS,
        {"tav_align_plan": AlignPlan, "tav_ctc_align_args": CtcAlignArgs}, "alignment"),
    Abi("tavhip_rnn.h", "tav_rnn_version", "RNN_ABI_VERSION", RNN_ABI_VERSION, _RNN_SIGS,
        {"tav_lstm_plan": LstmPlan, "tav_lstm_fwd_args": LstmFwdArgs, "tav_lstm_bwd_args": LstmBwdArgs}, "recurrent"),
    Abi("tavhip_conv.h", "tav_conv_version", "CONV_ABI_VERSION", CONV_ABI_VERSION, _CONV_SIGS,
        {"tav_conv3d_plan": Conv3dPlan, "tav_conv3d_fwd_args": Conv3dFwdArgs, "tav_conv3d_wgrad_args": Conv3dWgradArgs,
         "tav_flat_linear_fwd_args": FlatLinearFwdArgs, "tav_flat_linear_bwd_args": FlatLinearBwdArgs}, "convolution"),
)

# Package-private entry points: declared in a header next to the sources (csrc/), bound and version-checked by lib() like the public
# rows, but not part of the recorded public tables.  A change that re-records those tables promotes such a header to include/ and its
# row to ABIS.
# csrc/tavhip_loss.h: the soft F-beta / soft precision loss.
LOSS_ABI_VERSION = 1
SOFT_F_FBETA, SOFT_F_PRECISION = 0, 1


class SoftFArgs(C.Structure):
    _fields_ = [("logits", vp), ("target", vp), ("weight", vp), ("loss", vp), ("dlogits", vp), ("stats", vp), ("B", i64), ("C", i64), ("ld", i64),
                ("beta", C.c_double), ("eps", C.c_double), ("grad_scale", f32), ("mode", i32)]


_LOSS_SIGS = {
    "tav_loss_version": (C.c_int, []),
    "tav_soft_f_loss": (C.c_int, [C.POINTER(SoftFArgs), vp]),
}

PRIVATE_ABIS = (
    Abi("tavhip_loss.h", "tav_loss_version", "LOSS_ABI_VERSION", LOSS_ABI_VERSION, _LOSS_SIGS, {"tav_soft_f_args": SoftFArgs}, "loss"),
)

_lib = None


def _header_path(abi):
    return ("csrc/" if abi in PRIVATE_ABIS else "include/") + abi.header


def lib():
    """Load (once) and return the ctypes handle; fail loudly when the HIP library is absent, lacks a declared symbol or is of another version."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: the TAV hot path has no fallback. Build it with "
                "`make -C multi-modal-emotion_amd/csrc` (hipcc --offload-arch=gfx950).")
        h = C.CDLL(LIB_PATH)
        for abi in ABIS + PRIVATE_ABIS:
            for name, (res, args) in abi.sigs.items():
                fn = getattr(h, name, None)
                if fn is None:
                    raise RuntimeError(f"{LIB_PATH} does not export {name}, which {_header_path(abi)} declares; rebuild")
                fn.restype, fn.argtypes = res, args
        for abi in ABIS + PRIVATE_ABIS:
            got, want = getattr(h, abi.version_fn)(), globals()[abi.version_const]
            if got != want:
                raise RuntimeError(f"libtavhip {abi.what + ' ' if abi.what else ''}ABI {got} != binding {want}; rebuild")
        _lib = h
    return _lib


def declared_symbols():
    return sorted(_SIGS)


def check(code, what=""):
    if code != 0:
        msg = lib().tav_error_string(code).decode()
        raise RuntimeError(f"libtavhip {what} failed: {msg} (code {code})")


def ptr(t):
    """Device pointer of a tensor (or None)."""
    return None if t is None else t.data_ptr()


def dt(t_or_dtype):
    d = t_or_dtype.dtype if isinstance(t_or_dtype, torch.Tensor) else t_or_dtype
    if d == torch.float32:
        return TAV_F32
    if d == torch.bfloat16:
        return TAV_BF16
    if d == torch.float8_e4m3fn:
        return TAV_FP8
    raise TypeError(f"libtavhip supports float32, bfloat16 and (GEMM operands) float8_e4m3fn tensors, got {d}")


def stream():
    return torch.cuda.current_stream().cuda_stream
