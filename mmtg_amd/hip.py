"""ctypes binding of libmmtg_hip.so (the C ABI declared in include/mmtg_hip.h).

PyTorch is plumbing here: tensors provide device memory (``data_ptr()``) and the
current HIP stream; every compute step of the hot path is one of the entry
points below.  There is NO fallback: if the library is missing or a call fails
a RuntimeError is raised.
"""
from __future__ import annotations

import ctypes as C
import os

import torch

from .constraints import check_mirostat, check_warp

F32, BF16 = 0, 1
ABI_VERSION = 12
EPI_NONE, EPI_GELU, EPI_TANH, EPI_RESID, EPI_DGELU, EPI_DTANH, EPI_ATOMIC, EPI_ROWDOT = range(8)
GEMM_NO_TR, GEMM_REGSTAGE, GEMM_SKINNY, GEMM_NO_SKINNY, GEMM_WIDE, GEMM_NO_WIDE = 1, 2, 4, 8, 16, 32
GEMM_PERSIST, GEMM_NO_PERSIST, GEMM_ROW_ORDER, GEMM_OCC4, GEMM_NO_OCC4, GEMM_COL_BLOCK, GEMM_P256, GEMM_NO_P8, GEMM_P8 = 64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384
GEMM_GELU_GRAD = 32768
GEMM_P8_288 = 65536
GEMM_AUX2_BF16 = 131072     # mmtg_gemm_x3: the GELU epilogue stores the pre-activation as bf16 rows (bf16x3f)
PROF_CATS = ["gemm_bf16", "gemm_f32", "attn_fwd", "attn_bwd", "layernorm", "embed", "loss",
             "optim", "encoder", "decode", "misc"]

_LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libmmtg_hip.so")
_lib = None

_vp, _i, _l, _f, _u = C.c_void_p, C.c_int, C.c_long, C.c_float, C.c_uint

_SIGS = {
    "mmtg_abi_version": ([], _i),
    "mmtg_last_error": ([], C.c_char_p),
    "mmtg_build_flags": ([], C.c_char_p),
    "mmtg_prof_enable": ([_i], _i),
    "mmtg_prof_read": ([_vp, _vp, _vp, _vp], _i),
    "mmtg_gemm_trace": ([_vp, _i], _i),
    "mmtg_gemm_cu_budget": ([_i], _i),
    "mmtg_debug_occupy": ([_i, _i, C.c_double, _vp], _i),
    "mmtg_gemm": ([_i, _i, _i, _i, _i, _i, _vp, _l, _vp, _l, _vp, _l, _vp, _i, _vp, _l, _vp, _i, _f, _i, _u, _u, _i, _vp], _i),
    "mmtg_gemm_gather": ([_i, _i, _i, _i, _vp, _l, _vp, _l, _vp, _l, _vp, _i, _vp, _i, _vp, _l, _vp, _i, _vp], _i),
    "mmtg_splitk_finish": ([_i, _vp, _i, _i, _i, _l, _vp, _i, _vp, _l, _vp, _l, _vp, _vp, _vp, _f, _vp], _i),
    "mmtg_colsum": ([_i, _vp, _l, _i, _i, _vp, _vp, _l, _vp], _i),
    "mmtg_colsum_ws": ([_i, _i], _l),
    "mmtg_layernorm_fwd": ([_i, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _f, _vp], _i),
    "mmtg_layernorm_bwd_ws": ([_i, _i], _l),
    "mmtg_layernorm_bwd": ([_i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _vp, _u, _u, _vp, _vp, _l, _vp], _i),
    "mmtg_layernorm_bwd_x3": ([_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _vp, _l, _u, _u, _vp, _vp, _l, _vp], _i),
    "mmtg_attn_fwd": ([_i, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _u, _u, _vp], _i),
    "mmtg_attn_fwd_x3": ([_vp, _l, _vp, _vp, _vp, _l, _vp, _i, _i, _i, _i, _u, _u, _vp], _i),
    "mmtg_attn_bwd_x3": ([_vp, _l, _vp, _vp, _vp, _l, _vp, _vp, _i, _vp, _l, _vp, _l, _vp, _vp, _l, _i, _i, _i, _i, _u, _u, _vp], _i),
    "mmtg_attn_trace": ([_vp], _i),
    "mmtg_attn_bwd": ([_i, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _u, _u, _i, _vp], _i),
    "mmtg_embed_condition": ([_i, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp], _i),
    "mmtg_segment_sum": ([_i, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp], _i),
    "mmtg_embed_add": ([_i, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _u, _u, _vp], _i),
    "mmtg_embed_add_bwd": ([_i, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _u, _u, _vp, _l, _vp], _i),
    "mmtg_embed_add_bwd_ws": ([_i, _i, _i], _l),
    "mmtg_dropout_apply": ([_i, _vp, _vp, _l, _i, _u, _u, _vp], _i),
    "mmtg_loss_fwd": ([_i, _vp, _l, _i, _vp, _vp, _vp, _i, _i, _i, _i, _i, _f, _vp, _vp, _vp, _vp, _vp, _vp], _i),
    "mmtg_loss_bwd": ([_i, _i, _vp, _l, _i, _vp, _vp, _vp, _vp, _f, _f, _i, _i, _i, _vp, _l, _i, _vp], _i),
    "mmtg_loss_bwd_x3": ([_vp, _l, _i, _vp, _vp, _vp, _vp, _f, _f, _i, _i, _i, _vp, _l, _l, _i, _vp], _i),
    "mmtg_loss_ul_fwd": ([_i, _vp, _l, _i, _vp, _vp, _vp, _i, _i, _i, _i, _f, _vp, _vp, _vp, _vp, _vp], _i),
    "mmtg_loss_bwd_ul": ([_i, _i, _vp, _l, _i, _vp, _vp, _vp, _vp, _f, _f, _vp, _f, _vp, _i, _i, _i, _i, _vp, _l, _i, _vp], _i),
    "mmtg_loss_bwd_ul_x3": ([_vp, _l, _i, _vp, _vp, _vp, _vp, _f, _f, _vp, _f, _vp, _i, _i, _i, _i, _vp, _l, _l, _i, _vp], _i),
    "mmtg_cl_fwd": ([_i, _vp, _l, _vp, _l, _f, _i, _i, _i, _i, _f, _vp, _vp, _vp, _vp, _vp], _i),
    "mmtg_cl_bwd": ([_i, _i, _vp, _l, _vp, _l, _vp, _f, _f, _i, _i, _i, _i, _vp, _l, _vp], _i),
    "mmtg_gru_cell_fwd": ([_i, _vp, _l, _vp, _l, _vp, _l, _vp, _l, _vp, _i, _i, _vp], _i),
    "mmtg_gru_cell_bwd_fused": ([_i, _vp, _l, _vp, _vp, _i, _vp, _vp, _l, _vp, _l, _vp, _vp, _i, _i, _vp], _i),
    "mmtg_rnn_cell_fwd": ([_i, _i, _vp, _l, _vp, _l, _vp, _vp, _l, _vp, _vp, _i, _i, _vp], _i),
    "mmtg_rnn_cell_bwd": ([_i, _i, _vp, _l, _vp, _vp, _vp, _vp, _l, _vp, _i, _vp, _l, _i, _i, _vp], _i),
    "mmtg_gru_cell_bwd": ([_i, _vp, _vp, _vp, _l, _vp, _l, _vp, _vp, _i, _i, _vp], _i),
    "mmtg_alpha_attn_fwd": ([_i, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp], _i),
    "mmtg_alpha_attn_bwd": ([_i, _vp, _vp, _vp, _vp, _f, _vp, _i, _i, _i, _i, _vp], _i),
    "mmtg_beta_fuse_fwd": ([_i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp], _i),
    "mmtg_beta_fuse_bwd": ([_i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp, _l, _vp], _i),
    "mmtg_beta_fuse_bwd_ws": ([_i, _i, _i], _l),
    "mmtg_prefetch": ([_vp, _l, _i, _vp, _vp], _i),
    "mmtg_zero_ranges": ([_vp, _vp, _i, _vp], _i),
    "mmtg_sumsq": ([_vp, _l, _vp, _vp, _l, _vp], _i),
    "mmtg_sumsq_ws": ([_l], _l),
    "mmtg_adamw": ([_vp, _vp, _vp, _vp, _vp, _vp, _l, _f, _f, _f, _f, _f, _i, _vp, _f, _f, _vp, _vp], _i),
    "mmtg_param_groups_check": ([_vp, _i, _i, _l], _i),
    "mmtg_sumsq_groups_ws": ([_l, _i], _l),
    "mmtg_sumsq_groups": ([_vp, _l, _vp, _vp, _i, _i, _u, _vp, _vp, _l, _vp], _i),
    "mmtg_adamw_groups": ([_vp, _vp, _vp, _vp, _vp, _vp, _l, _vp, _vp, _i, _vp, _i, _f, _f, _f, _f, _i, _vp, _f, _f, _vp, _vp], _i),
    "mmtg_ema_update": ([_vp, _vp, _l, _f, _vp, _vp], _i),
    "mmtg_swap_f32": ([_vp, _vp, _l, _vp], _i),
    "mmtg_gemm_x3": ([_i, _i, _i, _vp, _l, _l, _vp, _l, _l, _vp, _l, _vp, _l, _l, _vp, _i, _vp, _l, _vp, _u, _u, _i, _vp], _i),
    "mmtg_split_planes": ([_vp, _l, _i, _i, _vp, _l, _l, _vp], _i),
    "mmtg_layernorm_fwd_x3": ([_vp, _vp, _l, _l, _vp, _vp, _vp, _vp, _i, _i, _f, _vp, _vp], _i),
    "mmtg_cast_f32_to": ([_i, _vp, _vp, _l, _vp], _i),
    "mmtg_cast_pad_rows": ([_i, _vp, _l, _vp, _l, _i, _i, _vp], _i),
    "mmtg_cast_to_f32": ([_i, _vp, _vp, _l, _vp], _i),
    "mmtg_axpy_f32": ([_vp, _vp, _f, _l, _vp], _i),
    "mmtg_slab_sum": ([_vp, _i, _l, _vp, _i, _l, _vp], _i),
    "mmtg_wgrad_group": ([_i, _i, _vp, _i, _i, _vp, _l, _vp, _l, _i, _vp], _i),
    "mmtg_transpose_batch": ([_i, _vp, _vp, _vp, _i, _i, _i, _vp], _i),
    "mmtg_logits_process_argmax": ([_vp, _l, _i, _vp, _l, _vp, _f, _f, _vp, _i, _vp], _i),
    "mmtg_decode_embed": ([_i, _vp, _vp, _l, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _l, _i, _i, _i, _i, _i, _i, _i, _i, _vp], _i),
    "mmtg_decode_embed_add": ([_i, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _vp, _vp], _i),
    "mmtg_decode_gemm": ([_i, _i, _i, _i, _vp, _l, _vp, _l, _vp, _l, _vp, _vp, _vp, _i, _f, _i, _i, _vp, _l, _vp, _i, _vp, _l, _vp, _l,
                          _vp, _vp, _vp, _vp, _vp], _i),
    "mmtg_ln_fold_weights": ([_vp, _l, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _vp], _i),
    "mmtg_decode_gemm_x3": ([_i, _i, _i, _i, _vp, _l, _l, _vp, _l, _l, _vp, _l, _vp, _l, _l, _vp, _vp, _vp, _i, _f, _i, _vp, _l, _vp, _i, _vp, _l,
                             _vp, _l, _vp, _vp, _vp, _vp, _vp], _i),
    "mmtg_ln_fold_weights_x3": ([_vp, _l, _l, _vp, _vp, _vp, _vp, _l, _l, _vp, _vp, _i, _i, _vp], _i),
    "mmtg_decode_attn_split_x3": ([_vp, _i, _vp, _vp, _vp, _vp, _l, _vp, _vp, _l, _i, _i, _i, _i, _vp], _i),
    "mmtg_decode_embed_x3": ([_vp, _vp, _l, _vp, _vp, _l, _vp, _vp, _vp, _vp, _vp, _l, _i, _i, _i, _i, _i, _i, _i, _i, _vp], _i),
    "mmtg_decode_attn": ([_i, _vp, _vp, _vp, _vp, _l, _vp, _vp, _i, _i, _i, _i, _vp], _i),
    "mmtg_decode_attn_split": ([_i, _vp, _i, _vp, _vp, _vp, _vp, _l, _vp, _vp, _i, _i, _i, _i, _vp], _i),
    "mmtg_logits_process_sample": ([_vp, _l, _i, _vp, _l, _vp, _f, _f, _i, _f, _vp, _vp, _vp, _i, _vp], _i),
    "mmtg_logits_process_sample_warp": ([_vp, _l, _i, _vp, _l, _vp, _f, _f, _i, _f, _f, _f, _f, _f, _vp, _vp, _vp, _i, _vp], _i),
    "mmtg_logits_process_sample_mirostat": ([_vp, _l, _i, _vp, _l, _vp, _f, _f, _i, _f, _f, _f, _f, _f, _vp, _vp, _vp, _i, _f, _f, _vp, _vp,
                                             _vp], _i),
    "mmtg_decode_sample": ([_vp, _l, _i, _vp, _l, _vp, _i, _i, _f, _f, _i, _f, _vp, _l, _i, _vp, _vp], _i),
    "mmtg_decode_select": ([_vp, _l, _i, _vp, _l, _vp, _i, _i, _f, _f, _i, _vp, _vp], _i),
    "mmtg_decode_advance": ([_vp, _vp], _i),
    "mmtg_decode_attn_split_rows": ([_i, _vp, _i, _vp, _vp, _vp, _vp, _l, _vp, _l, _vp, _vp, _i, _i, _i, _i, _vp], _i),
    "mmtg_decode_attn_split_x3_rows": ([_vp, _i, _vp, _vp, _vp, _vp, _l, _vp, _l, _vp, _vp, _l, _i, _i, _i, _i, _vp], _i),
    "mmtg_decode_beam_candidates": ([_vp, _l, _i, _vp, _l, _vp, _i, _i, _f, _f, _i, _vp, _vp, _i, _vp], _i),
    "mmtg_decode_beam_merge": ([_vp, _vp, _vp, _vp, _l, _vp, _l, _vp, _l, _vp, _i, _i, _i, _i, _vp, _vp], _i),
    "mmtg_decode_select_fixed": ([_vp, _l, _i, _vp, _l, _vp, _i, _i, _f, _f, _i, _vp, _vp, _vp], _i),
    "mmtg_decode_sample_fixed": ([_vp, _l, _i, _vp, _l, _vp, _i, _i, _f, _f, _i, _f, _vp, _l, _i, _vp, _vp, _vp], _i),
    "mmtg_decode_beam_candidates_fixed": ([_vp, _l, _i, _vp, _l, _vp, _i, _i, _f, _f, _i, _vp, _vp, _i, _vp, _vp], _i),
    "mmtg_decode_beam_merge_fixed": ([_vp, _vp, _vp, _vp, _l, _vp, _l, _vp, _l, _vp, _i, _i, _i, _i, _vp, _vp, _vp], _i),
    "mmtg_decode_beam_merge_groups": ([_vp, _vp, _vp, _vp, _l, _vp, _l, _vp, _l, _vp, _i, _i, _i, _i, _vp, _i, _f, _vp], _i),
    "mmtg_decode_beam_merge_groups_fixed": ([_vp, _vp, _vp, _vp, _l, _vp, _l, _vp, _l, _vp, _i, _i, _i, _i, _vp, _vp, _i, _f, _vp], _i),
    "mmtg_decode_select_ngram": ([_vp, _l, _i, _vp, _l, _vp, _i, _i, _f, _f, _i, _vp, _vp, _i, _vp], _i),
    "mmtg_decode_sample_ngram": ([_vp, _l, _i, _vp, _l, _vp, _i, _i, _f, _f, _i, _f, _vp, _l, _i, _vp, _vp, _i, _vp], _i),
    "mmtg_decode_beam_candidates_ngram": ([_vp, _l, _i, _vp, _l, _vp, _i, _i, _f, _f, _i, _vp, _vp, _i, _vp, _i, _vp], _i),
    "mmtg_decode_select_lines": ([_vp, _l, _i, _vp, _l, _vp, _i, _i, _f, _f, _i, _vp, _vp, _i, _vp, _vp, _i, _vp, _i, _vp, _vp], _i),
    "mmtg_decode_sample_lines": ([_vp, _l, _i, _vp, _l, _vp, _i, _i, _f, _f, _i, _f, _vp, _l, _i, _vp, _vp, _i, _vp, _vp, _i, _vp, _i,
                                 _vp, _vp], _i),
    "mmtg_decode_beam_candidates_lines": ([_vp, _l, _i, _vp, _l, _vp, _i, _i, _f, _f, _i, _vp, _vp, _i, _vp, _i, _vp, _vp, _i, _vp, _i,
                                          _vp, _vp], _i),
    "mmtg_decode_select_tmpl": ([_vp, _l, _i, _vp, _l, _vp, _i, _i, _f, _f, _i, _vp, _vp, _i, _vp, _vp, _i, _vp, _i, _vp, _vp, _vp], _i),
    "mmtg_decode_sample_tmpl": ([_vp, _l, _i, _vp, _l, _vp, _i, _i, _f, _f, _i, _f, _vp, _l, _i, _vp, _vp, _i, _vp, _vp, _i, _vp, _i,
                                _vp, _vp, _vp], _i),
    "mmtg_decode_beam_candidates_tmpl": ([_vp, _l, _i, _vp, _l, _vp, _i, _i, _f, _f, _i, _vp, _vp, _i, _vp, _i, _vp, _vp, _i, _vp, _i,
                                         _vp, _vp, _vp], _i),
    "mmtg_decode_select_rhyme": ([_vp, _l, _i, _vp, _l, _vp, _i, _i, _f, _f, _i, _vp, _vp, _i, _vp, _vp, _i, _vp, _i, _vp, _vp, _vp, _vp, _i,
                                  _vp], _i),
    "mmtg_decode_sample_rhyme": ([_vp, _l, _i, _vp, _l, _vp, _i, _i, _f, _f, _i, _f, _vp, _l, _i, _vp, _vp, _i, _vp, _vp, _i, _vp, _i,
                                 _vp, _vp, _vp, _vp, _i, _vp], _i),
    "mmtg_decode_beam_candidates_rhyme": ([_vp, _l, _i, _vp, _l, _vp, _i, _i, _f, _f, _i, _vp, _vp, _i, _vp, _i, _vp, _vp, _i, _vp, _i,
                                          _vp, _vp, _vp, _vp, _i, _vp], _i),
    "mmtg_decode_select_refrain": ([_vp, _l, _i, _vp, _l, _vp, _i, _i, _f, _f, _i, _vp, _vp, _i, _vp, _vp, _i, _vp, _i, _vp, _vp, _vp, _vp, _i,
                                    _vp, _vp], _i),
    "mmtg_decode_sample_refrain": ([_vp, _l, _i, _vp, _l, _vp, _i, _i, _f, _f, _i, _f, _vp, _l, _i, _vp, _vp, _i, _vp, _vp, _i, _vp, _i,
                                   _vp, _vp, _vp, _vp, _i, _vp, _vp], _i),
    "mmtg_decode_sample_warp": ([_vp, _l, _i, _vp, _l, _vp, _i, _i, _f, _f, _i, _f, _f, _f, _f, _f, _vp, _l, _i, _vp, _vp, _i, _vp, _vp, _i,
                                _vp, _i, _vp, _vp, _vp, _vp, _i, _vp, _vp], _i),
    "mmtg_decode_sample_mirostat": ([_vp, _l, _i, _vp, _l, _vp, _i, _i, _f, _f, _i, _f, _f, _f, _f, _f, _vp, _l, _i, _vp, _vp, _i, _vp, _vp, _i,
                                    _vp, _i, _vp, _vp, _vp, _vp, _i, _vp, _f, _f, _vp, _vp], _i),
    "mmtg_decode_beam_candidates_refrain": ([_vp, _l, _i, _vp, _l, _vp, _i, _i, _f, _f, _i, _vp, _vp, _i, _vp, _i, _vp, _vp, _i, _vp, _i,
                                            _vp, _vp, _vp, _vp, _i, _vp, _vp], _i),
    "mmtg_decode_logprob": ([_vp, _l, _i, _vp, _l, _vp, _i, _vp, _l, _i, _i, _vp], _i),
    "mmtg_decode_beam_candidates_kw": ([_vp, _l, _i, _vp, _l, _vp, _i, _i, _f, _f, _i, _vp, _vp, _i, _vp, _i, _vp, _vp, _i, _vp, _i,
                                       _vp, _vp, _vp, _vp, _i, _vp, _vp, _i, _i, _vp, _vp], _i),
    "mmtg_decode_beam_merge_kw": ([_vp, _vp, _vp, _vp, _vp, _l, _vp, _l, _vp, _l, _vp, _i, _i, _i, _i, _vp, _i, _vp], _i),
    "mmtg_decode_beam_merge_kw_fixed": ([_vp, _vp, _vp, _vp, _vp, _l, _vp, _l, _vp, _l, _vp, _i, _i, _i, _i, _vp, _vp, _i, _vp], _i),
    "mmtg_decode_contrastive_sim": ([_i, _vp, _l, _vp, _vp, _f, _vp, _i, _vp, _vp, _vp, _l, _vp, _l, _vp, _i, _i, _i, _vp], _i),
    "mmtg_decode_contrastive_merge": ([_vp, _vp, _vp, _vp, _vp, _f, _vp, _l, _vp, _l, _vp, _l, _vp, _i, _i, _i, _i, _vp, _vp, _vp], _i),
    "mmtg_decode_gumbel_candidates": ([_vp, _l, _i, _vp, _l, _vp, _i, _i, _f, _f, _i, _vp, _vp, _i, _vp, _i, _vp, _vp, _i, _vp, _i,
                                      _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp], _i),
    "mmtg_decode_gumbel_merge": ([_vp, _vp, _vp, _vp, _vp, _vp, _l, _vp, _l, _vp, _l, _vp, _i, _i, _i, _i, _vp, _vp, _vp], _i),
    "mmtg_decode_guidance": ([_vp, _vp, _l, _i, _f, _vp, _l, _i, _vp], _i),
    "mmtg_experience_drop": ([_i, _vp, _vp, _vp, _vp, _vp, _i, _l, _u, C.c_longlong, C.c_longlong, C.c_longlong, _vp], _i),
    "mmtg_guided_loss": ([_i, _vp, _vp, _l, _i, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _f, _vp, _vp, _vp, _vp], _i),
    "mmtg_guided_loss_multi": ([_i, _vp, _vp, _i, _l, _i, _vp, _vp, _i, _i, _i, _i, _f, _vp, _vp, _vp, _vp], _i),
    "mmtg_distill_fwd": ([_i, _vp, _l, _i, _vp, _vp, _l, _i, _vp, _vp, _vp, _f, _i, _i, _i, _f, _vp, _vp, _vp, _vp, _vp], _i),
    "mmtg_loss_bwd_kd": ([_i, _i, _vp, _l, _i, _vp, _vp, _vp, _vp, _f, _f, _i, _vp, _vp, _l, _vp, _vp, _f, _vp, _f, _i, _i, _i,
                         _vp, _l, _i, _vp], _i),
    "mmtg_loss_bwd_kd_x3": ([_vp, _l, _i, _vp, _vp, _vp, _vp, _f, _f, _i, _vp, _vp, _l, _vp, _vp, _f, _vp, _f, _i, _i, _i,
                            _vp, _l, _l, _i, _vp], _i),
    "mmtg_decode_mirror": ([_vp, _l, _vp, _i, _vp], _i),
    "mmtg_decode_guidance_multi": ([_vp, _l, _i, _i, _vp, _vp, _l, _i, _vp], _i),
    "mmtg_decode_guidance_multi_form": ([_vp, _l, _i, _i, _vp, _vp, _l, _i, _i, _vp], _i),
    "mmtg_decode_mirror_multi": ([_vp, _l, _vp, _i, _i, _vp], _i),
    "mmtg_decode_mlp_ws_floats": ([_i], _l),
    "mmtg_decode_mlp_sync_words": ([], _i),
    "mmtg_decode_mlp_census": ([_vp, _vp], _i),
    "mmtg_decode_mlp": ([_i, _i, _vp, _l, _vp, _i, _f, _vp, _l, _vp, _vp, _vp, _l, _vp, _vp, _l, _vp, _l, _vp, _vp, _l, _vp, _i, _vp, _vp], _i),
    "mmtg_colsum_batch": ([_vp, _i, _vp], _i),
    "mmtg_layernorm_bwd_partial": ([_i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _vp, _u, _u, _i, _vp, _l, _vp, _vp], _i),
    "mmtg_attn_bwd_dbias_rows": ([_i, _i, _i], _i),
    "mmtg_layernorm_bwd_x3_partial": ([_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _vp, _l, _u, _u, _i, _vp, _l, _vp, _vp], _i),
    "mmtg_comm_unique_id": ([_vp], _i),
    "mmtg_comm_init": ([_i, _i, _vp], _i),
    "mmtg_comm_info": ([_vp, _vp, _vp, _vp], _i),
    "mmtg_allreduce_bucket": ([_vp, _l, _i, _vp], _i),
    "mmtg_allreduce_bucket_async": ([_vp, _l, _i, _vp], _i),
    "mmtg_comm_join": ([_vp], _i),
    "mmtg_comm_destroy": ([], _i),
}


def lib_path():
    return _LIB_PATH


def source_sha():
    """sha1 over the kernel sources and the ABI header the library is built from (csrc/*.hip, csrc/*.h,
    include/mmtg_hip.h): ties a committed PMC measurement to the kernels it was taken on (bench.py roofline.traffic)."""
    import hashlib
    here = os.path.dirname(os.path.abspath(__file__))
    csrc = os.path.join(here, "csrc")
    h = hashlib.sha1()
    for name in sorted(f for f in os.listdir(csrc) if f.endswith(".hip") or f.endswith(".h")):
        with open(os.path.join(csrc, name), "rb") as f:
            h.update(name.encode() + b"\0" + f.read())
    with open(os.path.join(here, "..", "include", "mmtg_hip.h"), "rb") as f:
        h.update(f.read())
    return h.hexdigest()


def exported_symbols():
    return sorted(_SIGS)


def lib():
    """Load the shared library (once).  Raises if it is not built."""
    global _lib
    if _lib is None:
        if not os.path.exists(_LIB_PATH):
            raise RuntimeError(
                "libmmtg_hip.so is not built (%s). Run `python -m mmtg_amd.build` -- the MMTG hot "
                "path has no CPU/PyTorch fallback." % _LIB_PATH)
        L = C.CDLL(_LIB_PATH)
        for name, (args, res) in _SIGS.items():
            fn = getattr(L, name)  # AttributeError if the symbol is missing
            fn.argtypes = args
            fn.restype = res
        if L.mmtg_abi_version() != ABI_VERSION:
            raise RuntimeError("libmmtg_hip.so ABI version mismatch")
        flags = L.mmtg_build_flags().decode()
        if flags and os.environ.get("MMTG_ALLOW_DIAGNOSTIC_BUILD") != "1":
            raise RuntimeError("libmmtg_hip.so is a diagnostic build (MMTG_EXTRA_DEFS=%r): rebuild with `python -m mmtg_amd.build` "
                               "or set MMTG_ALLOW_DIAGNOSTIC_BUILD=1" % flags)
        _lib = L
    return _lib


def _check(rc, what):
    if rc != 0:
        raise RuntimeError("%s failed (%d): %s" % (what, rc, lib().mmtg_last_error().decode()))


def _p(t):
    return 0 if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def dt(t):
    if t.dtype == torch.float32:
        return F32
    if t.dtype == torch.bfloat16:
        return BF16
    raise TypeError("unsupported storage dtype %s" % t.dtype)


def torch_dtype(code):
    return torch.float32 if code == F32 else torch.bfloat16


def drop_thresh(p):
    """dropout probability -> 32-bit threshold (0 disables)."""
    return 0 if p <= 0.0 else min(int(p * 4294967296.0), 4294967295)


# ------------------------------------------------------------------ profiler
def prof_enable(on=True):
    _check(lib().mmtg_prof_enable(int(on)), "prof_enable")


def prof_read():
    n = len(PROF_CATS)
    la = (C.c_int * n)()
    ms = (C.c_double * n)()
    fl = (C.c_double * n)()
    by = (C.c_double * n)()
    _check(lib().mmtg_prof_read(C.addressof(la), C.addressof(ms), C.addressof(fl), C.addressof(by)), "prof_read")
    return {PROF_CATS[i]: {"launches": la[i], "ms": ms[i], "flops": fl[i], "bytes": by[i]} for i in range(n)}


# ------------------------------------------------------------------ GEMM
def zero_ranges(base, desc, n):
    """Zero n (first element, count) ranges of the fp32 tensor `base` in one launch; desc: int64 device tensor [n, 2]."""
    _check(lib().mmtg_zero_ranges(_p(base), _p(desc), int(n), _stream()), "zero_ranges")


def gemm_cu_budget(cus):
    """CUs the eight-phase kernel's tile rule may count on (0 = all, > 0 = that many, < 0 = all but that many)."""
    _check(lib().mmtg_gemm_cu_budget(int(cus)), "gemm_cu_budget")


# ------------------------------------------------------------------ the data-parallel exchange (csrc/comm.hip)
COMM_ID_BYTES = 128


def comm_unique_id():
    """Rank 0: the 128-byte id every rank passes to comm_init (ship it over any side channel)."""
    buf = C.create_string_buffer(COMM_ID_BYTES)
    _check(lib().mmtg_comm_unique_id(C.addressof(buf)), "comm_unique_id")
    return buf.raw


def comm_init(rank, world, unique_id):
    """Collective: the process's RCCL communicator on the current device (one process per GPU)."""
    if len(unique_id) != COMM_ID_BYTES:
        raise ValueError("comm_init: the id is %d bytes, not %d" % (len(unique_id), COMM_ID_BYTES))
    buf = C.create_string_buffer(bytes(unique_id), COMM_ID_BYTES)
    _check(lib().mmtg_comm_init(int(rank), int(world), C.addressof(buf)), "comm_init")


def comm_info():
    """{"rank", "world", "device", "rccl_version"} of the live communicator (world 0: none)."""
    v = (C.c_int * 4)()
    base = C.addressof(v)
    _check(lib().mmtg_comm_info(base, base + 4, base + 8, base + 12), "comm_info")
    return {"rank": v[0], "world": v[1], "device": v[2], "rccl_version": v[3]}


def allreduce_bucket(t, stream=None):
    """In-place SUM all-reduce of the contiguous fp32 / bf16 tensor `t`, enqueued on `stream` (default: the current one)."""
    assert t.is_contiguous()
    st = _stream() if stream is None else stream.cuda_stream
    _check(lib().mmtg_allreduce_bucket(t.data_ptr(), t.numel(), dt(t), st), "allreduce_bucket")


def allreduce_bucket_async(t):
    """The same on the library's side stream, ordered after what the current stream holds now; comm_join() ends the overlap."""
    assert t.is_contiguous()
    _check(lib().mmtg_allreduce_bucket_async(t.data_ptr(), t.numel(), dt(t), _stream()), "allreduce_bucket_async")


def comm_join():
    """The current stream waits for every bucket enqueued with allreduce_bucket_async so far."""
    _check(lib().mmtg_comm_join(_stream()), "comm_join")


def comm_destroy():
    _check(lib().mmtg_comm_destroy(), "comm_destroy")


def debug_occupy(workgroups, usec, lds_bytes=163840, stream=None):
    """Measurement hook: hold `workgroups` CU-sized slots (lds_bytes of LDS each) for `usec` microseconds on `stream`."""
    st = _stream() if stream is None else stream.cuda_stream
    _check(lib().mmtg_debug_occupy(int(workgroups), int(lds_bytes), float(usec), st), "debug_occupy")


def gemm_trace(buf=None):
    """Switch the in-kernel timeline of the LDS-DMA GEMMs on (buf: int64 CUDA tensor [max_wgs, 6]) or off."""
    _check(lib().mmtg_gemm_trace(_p(buf), 0 if buf is None else buf.shape[0]), "gemm_trace")


def gemm(A, B, C_, M, N, K, transA=False, transB=False, lda=None, ldb=None, ldc=None, bias=None,
         epi=EPI_NONE, aux=None, ldaux=0, aux2=None, out_f32=False, alpha=1.0, splits=1,
         drop_p=0.0, drop_seed=0, flags=0, dtype=None):
    """C[M,N] = epi(opA * opB); see include/mmtg_hip.h (mmtg_gemm)."""
    d = dt(A) if dtype is None else dtype
    if lda is None:
        lda = M if transA else K
    if ldb is None:
        ldb = K if transB else N
    if ldc is None:
        ldc = N
    if aux is not None and not ldaux:
        ldaux = N
    _check(lib().mmtg_gemm(d, int(transA), int(transB), M, N, K, _p(A), lda, _p(B), ldb, _p(C_), ldc,
                           _p(bias), epi, _p(aux), ldaux, _p(aux2), int(out_f32), float(alpha), splits,
                           drop_thresh(drop_p), drop_seed & 0xFFFFFFFF, flags, _stream()), "gemm")


EPI_SPLIT = 8
EPI_TANH_ADD = 9


# ------------------------------------------------------------------ split-precision ("bf16x3") products
class Planes:
    """(hi | lo) bf16 plane pair of an fp32 matrix [rows, cols]: ``t`` is a bf16 tensor [2, rows, ld] (or any tensor whose
    storage holds the two planes ``plane`` elements apart, the hi plane at its data pointer)."""
    __slots__ = ("t", "rows", "cols", "ld", "plane")

    def __init__(self, t, rows, cols, ld=None, plane=None):
        self.t, self.rows, self.cols = t, rows, cols
        self.ld = cols if ld is None else ld
        self.plane = rows * self.ld if plane is None else plane

    @staticmethod
    def empty(rows, cols, device):
        return Planes(torch.empty(2, rows, cols, device=device, dtype=torch.bfloat16), rows, cols)

    def float(self):
        """hi + lo as fp32 [rows, cols] (tests)."""
        flat = self.t.reshape(-1)
        hi = torch.as_strided(flat, (self.rows, self.cols), (self.ld, 1), 0)
        lo = torch.as_strided(flat, (self.rows, self.cols), (self.ld, 1), self.plane)
        return hi.float() + lo.float()


def split_planes(src, rows, cols, out, lds=None):
    """fp32 [rows, cols] -> Planes ``out``."""
    _check(lib().mmtg_split_planes(_p(src), cols if lds is None else lds, rows, cols, _p(out.t), out.ld, out.plane, _stream()), "split_planes")
    return out


def layernorm_fwd_x3(x, out, gamma, beta, mean, rstd, rows, cols, eps=1e-5, xb=None):
    _check(lib().mmtg_layernorm_fwd_x3(_p(x), _p(out.t), out.ld, out.plane, _p(gamma), _p(beta), _p(mean), _p(rstd), rows, cols,
                                       float(eps), _p(xb), _stream()), "layernorm_fwd_x3")


def gemm_x3(A, B, C_, M, N, K, planes=None, ldc=None, bias=None, epi=EPI_NONE, aux=None, ldaux=0, aux2=None,
            drop_p=0.0, drop_seed=0, flags=0):
    """C[M,N] (fp32, nullable) / planes (Planes, nullable) = epi(A B^T + bias), A [M,K] and B [N,K] as Planes
    (include/mmtg_hip.h, mmtg_gemm_x3)."""
    if aux is not None and not ldaux:
        ldaux = N
    _check(lib().mmtg_gemm_x3(M, N, K, _p(A.t), A.ld, A.plane, _p(B.t), B.ld, B.plane, _p(C_), N if ldc is None else ldc,
                              0 if planes is None else _p(planes.t), 0 if planes is None else planes.ld,
                              0 if planes is None else planes.plane, _p(bias), epi, _p(aux), ldaux, _p(aux2),
                              drop_thresh(drop_p), drop_seed & 0xFFFFFFFF, flags, _stream()), "gemm_x3")


def gemm_gather(mode, A, B, C_, M, N, K, rows, table_rows, lda, ldb, ldc=None, bias=None, epi=EPI_NONE, aux=None, ldaux=0,
                aux_rows=None, splits=1):
    """Products with table-gathered operand rows (include/mmtg_hip.h, mmtg_gemm_gather): mode 0 forward, mode 1 weight gradient."""
    _check(lib().mmtg_gemm_gather(int(mode), M, N, K, _p(A), lda, _p(B), ldb, _p(C_), N if ldc is None else ldc, _p(bias), epi,
                                  _p(rows), int(table_rows), _p(aux), ldaux or N, _p(aux_rows), int(splits), _stream()), "gemm_gather")


def splitk_finish(part, splits, M, N, out, bias=None, epi=EPI_NONE, aux=None, ldaux=0, ldp=None, ldo=None,
                  ln_gamma=None, ln_beta=None, ln_out=None, eps=1e-5):
    """out = epi(sum of the `splits` fp32 slabs of an EPI_SPLIT product + bias) [, ln_out = LayerNorm(out)]."""
    _check(lib().mmtg_splitk_finish(dt(out), _p(part), splits, M, N, N if ldp is None else ldp, _p(bias), epi, _p(aux),
                                    ldaux or N, _p(out), N if ldo is None else ldo, _p(ln_gamma), _p(ln_beta), _p(ln_out),
                                    float(eps), _stream()), "splitk_finish")


_colsum_ws = {}


def colsum(X, M, N, out, ldx=None, ws=None):
    """out[n] += sum_m X[m, n], in a fixed order (no atomics).  Tall inputs (mmtg_colsum_ws(M, N) > 0) sum in two stages through
    `ws` (default: a cached workspace per device, size and stream)."""
    need = int(lib().mmtg_colsum_ws(M, N))
    if need and (ws is None or ws.numel() < need):
        key = (X.device, need, _stream())        # per stream: two streams summing the same width must not share slices
        ws = _colsum_ws.get(key)
        if ws is None:
            ws = _colsum_ws[key] = torch.empty(need, device=X.device, dtype=torch.float32)
    _check(lib().mmtg_colsum(dt(X), _p(X), N if ldx is None else ldx, M, N, _p(out), _p(ws) if need else 0, need, _stream()), "colsum")


class ColsumItem(C.Structure):
    """mmtg_colsum_item of include/mmtg_hip.h."""
    _fields_ = [("X", C.c_void_p), ("out", C.c_void_p), ("ldx", C.c_long), ("M", C.c_int), ("N", C.c_int)]


_colsum_batch_cache = {}


def colsum_batch(items):
    """items: list of (X data_ptr, out data_ptr, ldx, M, N) -- fp32 rows, M <= 2048: out[c] += sum_r X[r * ldx + c] for every item in ONE
    launch (64 items per launch), each in mmtg_colsum's order.  The ctypes array is cached per item list (a step repeats its list)."""
    if not items:
        return
    key = tuple(items)
    arr = _colsum_batch_cache.get(key)
    if arr is None:
        if len(_colsum_batch_cache) > 64:
            _colsum_batch_cache.clear()
        arr = _colsum_batch_cache[key] = (ColsumItem * len(items))(*[ColsumItem(*it) for it in items])
    _check(lib().mmtg_colsum_batch(C.addressof(arr), len(items), _stream()), "colsum_batch")


# ------------------------------------------------------------------ LayerNorm
def layernorm_fwd(x, y, gamma, beta, mean, rstd, rows, cols, eps=1e-5):
    _check(lib().mmtg_layernorm_fwd(dt(x), _p(x), _p(y), _p(gamma), _p(beta), _p(mean), _p(rstd), rows, cols,
                                    float(eps), _stream()), "layernorm_fwd")


_ln_ws = {}


def layernorm_bwd(dy, x, gamma, mean, rstd, dres, dx, dgamma, dbeta, rows, cols, dx_masked=None, drop_p=0.0,
                  drop_seed=0, dcolsum=None, ws=None):
    if ws is None:   # convenience for tests; the engine passes its own workspace
        need = lib().mmtg_layernorm_bwd_ws(rows, cols)
        key = (x.device, need)
        ws = _ln_ws.get(key)
        if ws is None:
            ws = _ln_ws[key] = torch.empty(need, device=x.device, dtype=torch.float32)
    _check(lib().mmtg_layernorm_bwd(dt(x), _p(dy), _p(x), _p(gamma), _p(mean), _p(rstd), _p(dres), _p(dx),
                                    _p(dgamma), _p(dbeta), rows, cols, _p(dx_masked), drop_thresh(drop_p),
                                    drop_seed & 0xFFFFFFFF, _p(dcolsum), _p(ws), ws.numel(), _stream()), "layernorm_bwd")


def layernorm_bwd_partial(dy, x, gamma, mean, rstd, dres, dx, rows, cols, ws, dx_masked=None, drop_p=0.0, drop_seed=0, want_colsum=False):
    """First stage of layernorm_bwd only; returns the number of partial rows left in ws ([rows][3][cols]) for colsum_batch."""
    n = C.c_int(0)
    _check(lib().mmtg_layernorm_bwd_partial(dt(x), _p(dy), _p(x), _p(gamma), _p(mean), _p(rstd), _p(dres), _p(dx), rows, cols,
                                            _p(dx_masked), drop_thresh(drop_p), drop_seed & 0xFFFFFFFF, int(want_colsum),
                                            _p(ws), ws.numel(), C.addressof(n), _stream()), "layernorm_bwd_partial")
    return n.value


def layernorm_bwd_x3(dy, x, gamma, mean, rstd, dres, dx, dgamma, dbeta, rows, cols, dx_planes, drop_p=0.0, drop_seed=0, dcolsum=None, ws=None):
    """fp32 LayerNorm backward whose (masked) input gradient goes to the Planes ``dx_planes`` (x3 mode)."""
    _check(lib().mmtg_layernorm_bwd_x3(_p(dy), _p(x), _p(gamma), _p(mean), _p(rstd), _p(dres), _p(dx), _p(dgamma), _p(dbeta), rows, cols,
                                       _p(dx_planes.t), dx_planes.plane, drop_thresh(drop_p), drop_seed & 0xFFFFFFFF, _p(dcolsum),
                                       _p(ws), ws.numel(), _stream()), "layernorm_bwd_x3")


def layernorm_bwd_x3_partial(dy, x, gamma, mean, rstd, dres, dx, rows, cols, dx_planes, ws, drop_p=0.0, drop_seed=0, want_colsum=False):
    """First stage of layernorm_bwd_x3 only; returns the number of partial rows left in ws ([rows][3][cols]) for colsum_batch."""
    n = C.c_int(0)
    _check(lib().mmtg_layernorm_bwd_x3_partial(_p(dy), _p(x), _p(gamma), _p(mean), _p(rstd), _p(dres), _p(dx), rows, cols,
                                               _p(dx_planes.t), dx_planes.plane, drop_thresh(drop_p), drop_seed & 0xFFFFFFFF,
                                               int(want_colsum), _p(ws), ws.numel(), C.addressof(n), _stream()), "layernorm_bwd_x3_partial")
    return n.value


# ------------------------------------------------------------------ attention
def attn_fwd(qkv, keep, out, lse, B, T, nH, dh, drop_p=0.0, drop_seed=0):
    _check(lib().mmtg_attn_fwd(dt(qkv), _p(qkv), _p(keep), _p(out), _p(lse), B, T, nH, dh,
                               drop_thresh(drop_p), drop_seed & 0xFFFFFFFF, _stream()), "attn_fwd")


def attn_fwd_x3(qkv_planes, keep, out, out_planes, lse, B, T, nH, dh, drop_p=0.0, drop_seed=0):
    """Split-precision attention forward; qkv_planes: Planes [B*T, 3D] (what the c_attn product writes), out fp32, out_planes:
    Planes or None (include/mmtg_hip.h)."""
    if qkv_planes.ld != 3 * nH * dh:
        raise ValueError("attn_fwd_x3: the qkv plane pair must be dense ([B*T, 3D], ld = 3D)")
    _check(lib().mmtg_attn_fwd_x3(_p(qkv_planes.t), qkv_planes.plane, _p(keep), _p(out), 0 if out_planes is None else _p(out_planes.t),
                                  0 if out_planes is None else out_planes.plane, _p(lse), B, T, nH, dh,
                                  drop_thresh(drop_p), drop_seed & 0xFFFFFFFF, _stream()), "attn_fwd_x3")


def attn_bwd_x3_dq_floats(B, T, D):
    """Floats of attn_bwd_x3's dq32 scratch: one [B*T, D] buffer per block of 128 keys."""
    return (-(-T // 128)) * B * T * D


def attn_bwd_x3_ws(B, T, D):
    """Floats of the dbias workspace of attn_bwd_x3: the partial rows + the workspaces of their ordered column sums (mmtg_colsum_ws:
    128 x N floats once a reduction has more than 2048 rows)."""
    nkv, nq = B * (-(-T // 128)), -(-(B * T) // 16)
    return (nkv + nq) * 3 * D + (128 * 3 * D if nkv > 2048 else 0) + (128 * D if nq > 2048 else 0)


def attn_bwd_x3(qkv_planes, keep, out, dout_planes, lse, delta, dq32, dqkv_planes, B, T, nH, dh, drop_p=0.0, drop_seed=0, dbias=None,
                dbias_ws=None, delta_ready=False):
    """Split-precision attention backward: qkv [B*T, 3D] and d(ctx) [B*T, D] as Planes, out fp32; d(qkv) as the Planes
    ``dqkv_planes`` [B*T, 3D]; dq32: fp32 scratch of attn_bwd_x3_dq_floats(B, T, D) elements."""
    if qkv_planes.ld != 3 * nH * dh or dout_planes.ld != nH * dh or dqkv_planes.ld != 3 * nH * dh:
        raise ValueError("attn_bwd_x3: the plane pairs must be dense (ld = columns)")
    _check(lib().mmtg_attn_bwd_x3(_p(qkv_planes.t), qkv_planes.plane, _p(keep), _p(out), _p(dout_planes.t), dout_planes.plane, _p(lse), _p(delta),
                                  int(delta_ready), _p(dq32), dq32.numel(), _p(dqkv_planes.t), dqkv_planes.plane,
                                  _p(dbias), _p(dbias_ws), 0 if dbias_ws is None else dbias_ws.numel(), B, T, nH, dh,
                                  drop_thresh(drop_p), drop_seed & 0xFFFFFFFF, _stream()), "attn_bwd_x3")


ATTN_ELEM_MASK = 1      # attn_bwd flags: the tiled / split-precision kernels' per-element dropout mask in the whole-head kernels


def attn_bwd(qkv, keep, out, dout, lse, delta, dq32, dqkv, B, T, nH, dh, drop_p=0.0, drop_seed=0, delta_ready=False,
             dbias=None, dbias_ws=None, flags=0):
    _check(lib().mmtg_attn_bwd(dt(qkv), _p(qkv), _p(keep), _p(out), _p(dout), _p(lse), _p(delta), int(delta_ready), _p(dq32),
                               _p(dqkv), _p(dbias), _p(dbias_ws), B, T, nH, dh, drop_thresh(drop_p), drop_seed & 0xFFFFFFFF,
                               int(flags), _stream()), "attn_bwd")


def attn_trace(buf):
    _check(lib().mmtg_attn_trace(_p(buf)), "attn_trace")


ATTN_DBIAS_ROWS = 2


def attn_bwd_dbias_rows(dtype_code, B, T):
    """Partial bias rows attn_bwd(flags=ATTN_DBIAS_ROWS) leaves unsummed at the head of dbias_ws for this shape (0: it sums inside the call)."""
    return int(lib().mmtg_attn_bwd_dbias_rows(dtype_code, B, T))


def attn_bwd_bias_rows(B, T, dtype_code):
    """Rows of the dbias_ws scratch of attn_bwd ([rows, 3*D] f32): one partial bias row per (batch row, key block) + 44 rows the
    tiled kernels' ordered column sum of dQ uses as its workspace."""
    return B * (-(-T // (128 if dtype_code == F32 else 256))) + 44


# ------------------------------------------------------------------ conditioning front end
def embed_condition(table, topic_ids, targets, c, x, B, P, L, S, E, two_sents, V):
    _check(lib().mmtg_embed_condition(dt(table), _p(table), _p(topic_ids), _p(targets), _p(c), _p(x),
                                      B, P, L, S, E, two_sents, V, _stream()), "embed_condition")


def segment_sum(g, out, B, P, L, S, H, two_sents):
    _check(lib().mmtg_segment_sum(dt(g), _p(g), _p(out), B, P, L, S, H, two_sents, _stream()), "segment_sum")


def embed_add(g, wpe, wte, type_ids, h, M, T, D, drop_p=0.0, drop_seed=0):
    _check(lib().mmtg_embed_add(dt(g), _p(g), _p(wpe), _p(wte), _p(type_ids), _p(h), M, T, D,
                                drop_thresh(drop_p), drop_seed & 0xFFFFFFFF, _stream()), "embed_add")


_embed_ws = {}


def embed_add_bwd(dh, type_ids, dwpe, dwte, M, T, D, ntypes, drop_p=0.0, drop_seed=0, ws=None):
    need = int(lib().mmtg_embed_add_bwd_ws(M, D, ntypes))
    if ws is None or ws.numel() < need:     # (the engine passes its own workspace; tests get a cached one)
        key = (dh.device, need)
        ws = _embed_ws.get(key)
        if ws is None:
            ws = _embed_ws[key] = torch.empty(need, device=dh.device, dtype=torch.float32)
    _check(lib().mmtg_embed_add_bwd(dt(dh), _p(dh), _p(type_ids), _p(dwpe), _p(dwte), M, T, D, ntypes,
                                    drop_thresh(drop_p), drop_seed & 0xFFFFFFFF, _p(ws), ws.numel(), _stream()), "embed_add_bwd")


def dropout_apply(x, y, n, drop_p, drop_seed):
    _check(lib().mmtg_dropout_apply(dt(x), _p(x), _p(y), n, 0, drop_thresh(drop_p), drop_seed & 0xFFFFFFFF,
                                    _stream()), "dropout_apply")


# ------------------------------------------------------------------ loss
def loss_fwd(logits, ldl, V, topic_ids, targets, ratings, stage, label_zero, B, P, L, batch_den,
             nll, lse, sample_ce, coef, scalars):
    _check(lib().mmtg_loss_fwd(dt(logits), _p(logits), ldl, V, _p(topic_ids), _p(targets), _p(ratings), stage,
                               int(label_zero), B, P, L, float(batch_den), _p(nll), _p(lse), _p(sample_ce),
                               _p(coef), _p(scalars), _stream()), "loss_fwd")


def loss_bwd(logits, ldl, V, topic_ids, targets, lse, coef, gscale, B, P, L, dlogits, ldd, Vpad, lm_coef=0.0):
    _check(lib().mmtg_loss_bwd(dt(dlogits), dt(logits), _p(logits), ldl, V, _p(topic_ids), _p(targets), _p(lse), _p(coef),
                               float(gscale), float(lm_coef), B, P, L, _p(dlogits), ldd, Vpad, _stream()), "loss_bwd")


def loss_bwd_x3(logits, ldl, V, topic_ids, targets, lse, coef, gscale, B, P, L, planes, Vpad, lm_coef=0.0):
    """d(logits) of fp32 logits as a Planes pair (x3 mode)."""
    _check(lib().mmtg_loss_bwd_x3(_p(logits), ldl, V, _p(topic_ids), _p(targets), _p(lse), _p(coef), float(gscale), float(lm_coef), B, P, L,
                                  _p(planes.t), planes.ld, planes.plane, Vpad, _stream()), "loss_bwd_x3")


# token-level unlikelihood on repeated lyric tokens (the rule: include/mmtg_hip.h)
UL_FLOOR, UL_MAX_EXCLUDE, UL_MAX_L = 1e-5, 32, 1024


def _n_ex(exclude):
    return 0 if exclude is None else int(exclude.numel())


def loss_ul_fwd(logits, ldl, V, targets, lse, exclude, B, P, L, batch_den, ul_row, ul_S, ul_sample, ul):
    """ul_row [M], ul_S [M], ul_sample [B] and the scalar ul [1] from the logits and the row lse of loss_fwd; exclude: an int64
    device tensor of at most 32 ids, or None."""
    _check(lib().mmtg_loss_ul_fwd(dt(logits), _p(logits), ldl, V, _p(targets), _p(lse), _p(exclude), _n_ex(exclude), B, P, L,
                                  float(batch_den), _p(ul_row), _p(ul_S), _p(ul_sample), _p(ul), _stream()), "loss_ul_fwd")


def loss_bwd_ul(logits, ldl, V, topic_ids, targets, lse, coef, gscale, ul_S, ul_coef, exclude, B, P, L, dlogits, ldd, Vpad, lm_coef=0.0):
    """loss_bwd with the term's gradient: ul_S from loss_ul_fwd, ul_coef = ul_weight * gscale / (ntok * batch_den)."""
    _check(lib().mmtg_loss_bwd_ul(dt(dlogits), dt(logits), _p(logits), ldl, V, _p(topic_ids), _p(targets), _p(lse), _p(coef),
                                  float(gscale), float(lm_coef), _p(ul_S), float(ul_coef), _p(exclude), _n_ex(exclude), B, P, L,
                                  _p(dlogits), ldd, Vpad, _stream()), "loss_bwd_ul")


def loss_bwd_ul_x3(logits, ldl, V, topic_ids, targets, lse, coef, gscale, ul_S, ul_coef, exclude, B, P, L, planes, Vpad, lm_coef=0.0):
    """... into a Planes pair (x3 mode): hi and lo of the candidate columns are both rewritten."""
    _check(lib().mmtg_loss_bwd_ul_x3(_p(logits), ldl, V, _p(topic_ids), _p(targets), _p(lse), _p(coef), float(gscale), float(lm_coef),
                                     _p(ul_S), float(ul_coef), _p(exclude), _n_ex(exclude), B, P, L,
                                     _p(planes.t), planes.ld, planes.plane, Vpad, _stream()), "loss_bwd_ul_x3")


# contrastive token loss on the last-layer states (the rule: include/mmtg_hip.h)
CL_MAX_L, CL_MAX_D = 1024, 1024


def cl_fwd(hf, ldh, keep, ldkeep, margin, B, P, L, D, batch_den, rinv, cl_row, cl_sample, cl):
    """rinv [M], cl_row [M], cl_sample [B] and the scalar cl [1] from hf [M, D] (fp32 or bf16, row stride ldh) and the int32 keep
    mask [B, P + L]."""
    _check(lib().mmtg_cl_fwd(dt(hf), _p(hf), ldh, _p(keep), ldkeep, float(margin), B, P, L, D, float(batch_den),
                             _p(rinv), _p(cl_row), _p(cl_sample), _p(cl), _stream()), "cl_fwd")


def cl_bwd(hf, ldh, keep, ldkeep, rinv, margin, coef, B, P, L, D, dhf, ldd):
    """dhf += coef * d(sum_b cl_sample)/d hf in place (rinv from cl_fwd); dhf fp32 or bf16, bf16 hf goes with bf16 dhf."""
    _check(lib().mmtg_cl_bwd(dt(hf), dt(dhf), _p(hf), ldh, _p(keep), ldkeep, _p(rinv), float(margin), float(coef), B, P, L, D,
                             _p(dhf), ldd, _stream()), "cl_bwd")


# ------------------------------------------------------------------ encoder pieces
def gru_cell_bwd_fused(rows, ld_rows, carry, part, splits, save, h_prev, dgi, dgh, dh_prev, B, H, ld_hp=None, ld_dgi=None):
    """gru_cell_bwd with dh_t = rows + carry + sum of the carry product's slabs assembled in the kernel."""
    _check(lib().mmtg_gru_cell_bwd_fused(dt(dgi), _p(rows), ld_rows, _p(carry), _p(part), splits, _p(save), _p(h_prev),
                                         H if ld_hp is None else ld_hp, _p(dgi), 3 * H if ld_dgi is None else ld_dgi,
                                         _p(dgh), _p(dh_prev), B, H, _stream()), "gru_cell_bwd_fused")



def gru_cell_fwd(gi, gh, h_prev, h, save, B, H, ld_gi=None, ld_hp=None, ld_h=None, ld_gh=None):
    _check(lib().mmtg_gru_cell_fwd(dt(gi), _p(gi), 3 * H if ld_gi is None else ld_gi, _p(gh), 3 * H if ld_gh is None else ld_gh, _p(h_prev),
                                   H if ld_hp is None else ld_hp, _p(h), H if ld_h is None else ld_h, _p(save),
                                   B, H, _stream()), "gru_cell_fwd")


def gru_cell_bwd(dh, save, h_prev, dgi, dgh, dh_prev, B, H, ld_hp=None, ld_dgi=None):
    _check(lib().mmtg_gru_cell_bwd(dt(dgi), _p(dh), _p(save), _p(h_prev), H if ld_hp is None else ld_hp, _p(dgi),
                                   3 * H if ld_dgi is None else ld_dgi, _p(dgh), _p(dh_prev), B, H, _stream()),
           "gru_cell_bwd")


RNN_RELU, RNN_LSTM = 0, 1
RNN_GATES = {"GRU": 3, "LSTM": 4, "RNN": 1}


def rnn_cell_fwd(kind, gi, gh, c_prev, h, c, save, B, H, ld_gi, ld_h, ld_gh=None):
    """ReLU-RNN / LSTM cell of one step (reference model.py:41-59 encoder types)."""
    G = 4 if kind == RNN_LSTM else 1
    _check(lib().mmtg_rnn_cell_fwd(dt(gi), kind, _p(gi), ld_gi, _p(gh), G * H if ld_gh is None else ld_gh, _p(c_prev), _p(h), ld_h,
                                   _p(c), _p(save), B, H, _stream()), "rnn_cell_fwd")


def rnn_cell_bwd(kind, rows, ld_rows, part, save, c_prev, h, ld_h, dc, dc_in, da, ld_da, B, H):
    _check(lib().mmtg_rnn_cell_bwd(dt(da), kind, _p(rows), ld_rows, _p(part), _p(save), _p(c_prev), _p(h), ld_h, _p(dc), int(dc_in),
                                   _p(da), ld_da, B, H, _stream()), "rnn_cell_bwd")


def alpha_attn_fwd(qkv, prior, ctx, probs, kl, B, S, H, heads):
    _check(lib().mmtg_alpha_attn_fwd(dt(qkv), _p(qkv), _p(prior), _p(ctx), _p(probs), _p(kl), B, S, H, heads,
                                     _stream()), "alpha_attn_fwd")


def alpha_attn_bwd(qkv, prior, probs, dctx, dkl, dqkv, B, S, H, heads):
    _check(lib().mmtg_alpha_attn_bwd(dt(qkv), _p(qkv), _p(prior), _p(probs), _p(dctx), float(dkl), _p(dqkv),
                                     B, S, H, heads, _stream()), "alpha_attn_bwd")


def beta_fuse_fwd(topic, img, txt, att_w, att_b, o, a, B, S, H):
    _check(lib().mmtg_beta_fuse_fwd(dt(topic), _p(topic), _p(img), _p(txt), _p(att_w), _p(att_b), _p(o), _p(a),
                                    B, S, H, _stream()), "beta_fuse_fwd")


_beta_ws = {}


def beta_fuse_bwd(topic, img, txt, att_w, a, d_o, dtopic, dimg, dtxt, datt_w, datt_b, B, S, H):
    need = int(lib().mmtg_beta_fuse_bwd_ws(B, S, H))             # 0.7 MB at the released sizes
    key = (d_o.device, need, _stream())                          # one workspace per device, size and stream (not one per step)
    ws = _beta_ws.get(key)
    if ws is None:
        if len(_beta_ws) > 64:
            _beta_ws.clear()
        ws = _beta_ws[key] = torch.empty(need, device=d_o.device, dtype=torch.float32)
    _check(lib().mmtg_beta_fuse_bwd(dt(topic), _p(topic), _p(img), _p(txt), _p(att_w), _p(a), _p(d_o), _p(dtopic),
                                    _p(dimg), _p(dtxt), _p(datt_w), _p(datt_b), B, S, H, _p(ws), ws.numel(), _stream()), "beta_fuse_bwd")


# ------------------------------------------------------------------ optimizer / casts
def prefetch(t, sink, workgroups=256, stream=None):
    """Pull tensor `t` into the Infinity Cache on `stream` (default: the current one)."""
    _check(lib().mmtg_prefetch(_p(t), t.numel() * t.element_size(), int(workgroups), _p(sink),
                               _stream() if stream is None else stream.cuda_stream), "prefetch")


_sumsq_ws = {}


def sumsq(x, n, out):
    """out[0] = sum of squares of x[:n] (written, not accumulated), in a fixed summation order."""
    need = int(lib().mmtg_sumsq_ws(n))
    key = (x.device, need, _stream())
    ws = _sumsq_ws.get(key)
    if ws is None:
        ws = _sumsq_ws[key] = torch.empty(need, device=x.device, dtype=torch.float32)
    _check(lib().mmtg_sumsq(_p(x), n, _p(out), _p(ws), need, _stream()), "sumsq")


def adamw(p, g, m, v, p_bf16, n, lr, beta1, beta2, eps, wd, step, normsq, max_norm, grad_scale=1.0, count=None, p_lo=None):
    """count: optional device scalar (float32) = global row count; g is then a SUM over rows (see the header).
    p_lo: the x3 mode's lo plane (p_bf16 is then the hi plane)."""
    _check(lib().mmtg_adamw(_p(p), _p(g), _p(m), _p(v), _p(p_bf16), _p(p_lo), n, float(lr), float(beta1), float(beta2),
                            float(eps), float(wd), int(step), _p(normsq), float(max_norm), float(grad_scale),
                            _p(count), _stream()), "adamw")


class ParamGroup(C.Structure):
    """mmtg_param_group of include/mmtg_hip.h."""
    _fields_ = [("lr_scale", C.c_float), ("weight_decay", C.c_float), ("frozen", C.c_int), ("pad", C.c_int)]


def param_groups_check(segments, ngroups, n):
    """Host-only validation of an int64 [S, 3] (begin, end, group) table (no device call); raises RuntimeError with the library's message."""
    import numpy as np
    segs = np.ascontiguousarray(segments, dtype=np.int64).reshape(-1, 3)
    _check(lib().mmtg_param_groups_check(segs.ctypes.data, len(segs), int(ngroups), int(n)), "param_groups_check")


class GroupTable:
    """A parameter-group plan (mmtg_amd.param_groups.build_param_groups) as the grouped optimizer entries take it: the segment
    table on the host and, uploaded once, on the device; the groups' records; the frozen groups as a bit mask."""

    def __init__(self, plan, device):
        import numpy as np
        self.plan = plan
        self.segs_host = np.ascontiguousarray(plan.segments, dtype=np.int64).reshape(-1, 3)
        self.nsegs, self.ngroups = len(self.segs_host), len(plan.groups)
        param_groups_check(self.segs_host, self.ngroups, plan.total)
        self.segs_dev = torch.from_numpy(self.segs_host.copy()).to(device) if self.nsegs else None
        self.records = (ParamGroup * self.ngroups)(*[ParamGroup(float(g["lr_scale"]), float(g["weight_decay"]), int(bool(g["frozen"])), 0)
                                                      for g in plan.groups])
        self.frozen_mask = sum(1 << i for i, g in enumerate(plan.groups) if g["frozen"])


_sumsq_groups_ws = {}


def sumsq_groups(x, n, table, out):
    """out[g] = sum of squares of group g's segments of x[:n] (0 for frozen groups), out[ngroups] = the trainable groups' total:
    written, not accumulated, in a fixed summation order.  Gaps and frozen segments are not read."""
    need = int(lib().mmtg_sumsq_groups_ws(n, table.ngroups))
    key = (x.device, need, _stream())
    ws = _sumsq_groups_ws.get(key)
    if ws is None:
        ws = _sumsq_groups_ws[key] = torch.empty(need, device=x.device, dtype=torch.float32)
    _check(lib().mmtg_sumsq_groups(_p(x), n, _p(table.segs_dev), table.segs_host.ctypes.data, table.nsegs, table.ngroups,
                                   table.frozen_mask, _p(out), _p(ws), need, _stream()), "sumsq_groups")


def adamw_groups(p, g, m, v, p_bf16, n, table, lr, beta1, beta2, eps, step, normsq, max_norm, grad_scale=1.0, count=None, p_lo=None):
    """mmtg_adamw per parameter group: group i runs with the fp32 product lr * lr_scale_i and its own weight decay; frozen groups
    and the elements outside every segment keep every bit of p, m, v and both planes."""
    _check(lib().mmtg_adamw_groups(_p(p), _p(g), _p(m), _p(v), _p(p_bf16), _p(p_lo), n, _p(table.segs_dev), table.segs_host.ctypes.data,
                                   table.nsegs, C.addressof(table.records), table.ngroups, float(lr), float(beta1), float(beta2),
                                   float(eps), int(step), _p(normsq), float(max_norm), float(grad_scale), _p(count), _stream()),
           "adamw_groups")


def ema_update(ema, p, n, w, count=None):
    """ema[:n] = fmaf(w, p - ema, ema), w = 1 - decay rounded once to fp32; p == ema keeps ema's bits.  count: the optional device
    scalar of adamw -- a count that is not greater than 0 leaves ema untouched."""
    _check(lib().mmtg_ema_update(_p(ema), _p(p), n, float(w), _p(count), _stream()), "ema_update")


def swap_f32(a, b, n):
    """a[:n] <-> b[:n], bit for bit."""
    _check(lib().mmtg_swap_f32(_p(a), _p(b), n, _stream()), "swap_f32")


def cast_f32_to(src, dst, n):
    _check(lib().mmtg_cast_f32_to(dt(dst), _p(src), _p(dst), n, _stream()), "cast_f32_to")


def cast_pad_rows(src, lds, dst, ldd, rows, cols):
    _check(lib().mmtg_cast_pad_rows(dt(dst), _p(src), lds, _p(dst), ldd, rows, cols, _stream()), "cast_pad_rows")


def cast_to_f32(src, dst, n):
    _check(lib().mmtg_cast_to_f32(dt(src), _p(src), _p(dst), n, _stream()), "cast_to_f32")


def axpy_f32(y, x, a, n):
    _check(lib().mmtg_axpy_f32(_p(y), _p(x), float(a), n, _stream()), "axpy_f32")


def slab_sum(part, splits, stride, dst, n, accumulate=True):
    """dst[0:n] (+)= sum of the `splits` fp32 slabs (stride floats apart) of a weight-gradient EPI_SPLIT product."""
    _check(lib().mmtg_slab_sum(_p(part), splits, stride, _p(dst), int(accumulate), n, _stream()), "slab_sum")


class WgradProblem(C.Structure):
    """mmtg_wgrad_problem of include/mmtg_hip.h."""
    _fields_ = [("A", C.c_void_p), ("lda", C.c_long), ("B", C.c_void_p), ("ldb", C.c_long),
                ("C", C.c_void_p), ("ldc", C.c_long), ("M", C.c_int), ("N", C.c_int),
                ("planeA", C.c_long), ("planeB", C.c_long)]


WGRAD_RING = 8      # mmtg_wgrad_group config: 256x256 tiles, one 16-wave workgroup per CU over a 3-deep ring of 32-k stages


def wgrad_group_sizes(shapes, splits, config=0):
    """(tiles, workspace floats, counters) of a grouped launch over problems of the given (M, N) shapes.  The split-precision
    bits of config (2, 6) do not change the tiles: configs 2 and 6 size as config 0."""
    config &= ~6
    tb, nw = (256, 16) if config == WGRAD_RING else (256, 8) if config else (128, 4)
    tiles = sum(((M + tb - 1) // tb) * ((N + tb - 1) // tb) for (M, N) in shapes)
    return tiles, tiles * splits * tb * tb, tiles * nw


def wgrad_group(problems, K, splits, ws, counters, accumulate=False, config=0):
    """Grouped weight gradients C (+)= A^T B (include/mmtg_hip.h, mmtg_wgrad_group).
    problems: list of (A [K, lda] bf16, B [K, ldb] bf16, C [M, ldc] f32, M, N[, lda, ldb, ldc]).
    config 2 (x3): A and B are Planes (hi | lo plane pairs); config WGRAD_RING: the 16-wave ring form of the bf16 product."""
    arr = (WgradProblem * len(problems))()
    for i, pr in enumerate(problems):
        A, B, C_, M, N = pr[:5]
        lda, ldb, ldc = (pr[5:8] if len(pr) >= 8 else (M, N, N))
        if config & 2:
            arr[i] = WgradProblem(_p(A.t), lda, _p(B.t), ldb, _p(C_), ldc, M, N, A.plane, B.plane)
        else:
            arr[i] = WgradProblem(_p(A), lda, _p(B), ldb, _p(C_), ldc, M, N, 0, 0)
    _check(lib().mmtg_wgrad_group(int(config), len(problems), C.addressof(arr), int(K), int(splits), _p(ws), 0 if ws is None else ws.numel(),
                                  _p(counters), 0 if counters is None else counters.numel(), int(accumulate), _stream()), "wgrad_group")


def transpose_batch(src, dst, desc, n, max_rows, max_cols):
    """Matrix i ([rows, cols] at src + desc[i,0]) -> [cols, rows] at dst + desc[i,3]; desc: int64 CUDA [n,4]."""
    _check(lib().mmtg_transpose_batch(dt(src), _p(src), _p(dst), _p(desc), n, max_rows, max_cols, _stream()), "transpose_batch")


# ------------------------------------------------------------------ generation
def logits_process_argmax(logits, ldl, V, generated, ldg, gen_len, temperature, rep_penalty, nxt, B):
    _check(lib().mmtg_logits_process_argmax(_p(logits), ldl, V, _p(generated), ldg, _p(gen_len),
                                            float(temperature), float(rep_penalty), _p(nxt), B, _stream()),
           "logits_process_argmax")


def logits_process_sample(logits, ldl, V, generated, ldg, gen_len, temperature, rep_penalty, top_k, top_p, uniforms, nxt, B,
                          filtered=None):
    """One draw per row from the reference's filtered distribution (include/mmtg_hip.h); uniforms: f32 [B] in [0,1)."""
    _check(lib().mmtg_logits_process_sample(_p(logits), ldl, V, _p(generated), ldg, _p(gen_len), float(temperature),
                                            float(rep_penalty), int(top_k), float(top_p), _p(uniforms), _p(nxt), _p(filtered),
                                            B, _stream()), "logits_process_sample")


def logits_process_sample_warp(logits, ldl, V, generated, ldg, gen_len, temperature, rep_penalty, top_k, top_p, uniforms, nxt, B,
                               min_p=0.0, typical_p=1.0, epsilon_cutoff=0.0, eta_cutoff=0.0, filtered=None):
    """logits_process_sample with the min-p, typical, epsilon and eta stages between the nucleus filter and the draw
    (include/mmtg_hip.h; constraints.warp_filter restates them)."""
    warp = check_warp(min_p, typical_p, epsilon_cutoff, eta_cutoff)
    _check(lib().mmtg_logits_process_sample_warp(_p(logits), ldl, V, _p(generated), ldg, _p(gen_len), float(temperature),
                                                 float(rep_penalty), int(top_k), float(top_p), *warp, _p(uniforms), _p(nxt),
                                                 _p(filtered), B, _stream()), "logits_process_sample_warp")


def logits_process_sample_mirostat(logits, ldl, V, generated, ldg, gen_len, temperature, rep_penalty, top_k, top_p, uniforms, nxt, B,
                                   mirostat_tau, mirostat_eta, mu, surprise=None, min_p=0.0, typical_p=1.0, epsilon_cutoff=0.0,
                                   eta_cutoff=0.0, filtered=None):
    """logits_process_sample_warp with Mirostat v2 as the last stage (include/mmtg_hip.h; constraints.mirostat_filter and
    mirostat_update restate it).  mu: f32 [B], read and written; surprise: f32 [B] or None."""
    warp = check_warp(min_p, typical_p, epsilon_cutoff, eta_cutoff)
    tau, eta = check_mirostat(mirostat_tau, mirostat_eta)
    if tau == 0.0:
        raise ValueError("mirostat_tau must be in (0, 32] here: 0 (off) is logits_process_sample_warp")
    _check(lib().mmtg_logits_process_sample_mirostat(_p(logits), ldl, V, _p(generated), ldg, _p(gen_len), float(temperature),
                                                     float(rep_penalty), int(top_k), float(top_p), *warp, _p(uniforms), _p(nxt),
                                                     _p(filtered), B, tau, eta, _p(mu), _p(surprise), _stream()),
           "logits_process_sample_mirostat")


# ------------------------------------------------------------------ KV-cached decode step
def decode_embed(table, seq, c, x, pos, tpw_type, tpw_mask, type_out, keep, B, P, S, E, two_sents, V, sent, max_sent_num):
    _check(lib().mmtg_decode_embed(dt(table), _p(table), _p(seq), seq.stride(0), _p(c), _p(x), _p(pos), _p(tpw_type),
                                   _p(tpw_mask), _p(type_out), _p(keep), keep.stride(0), B, P, S, E, two_sents, V, sent,
                                   max_sent_num, _stream()), "decode_embed")


def decode_embed_add(g, wpe, wte, type_ids, pos, h, B, D, stats=None):
    _check(lib().mmtg_decode_embed_add(dt(g), _p(g), _p(wpe), _p(wte), _p(type_ids), _p(pos), _p(h), B, D, _p(stats), _stream()),
           "decode_embed_add")


DG_NP = 32      # statistics partials per row (include/mmtg_hip.h, mmtg_decode_gemm)


def decode_gemm(mode, A, W, C_, M, N, K, bias=None, colsum=None, stats_in=None, np_in=0, eps=1e-5, act=EPI_NONE, out_f32=False,
                resid=None, stats_out=None, splits=1, ws=None, counters=None, lda=None, ldw=None, ldc=None, ldr=None,
                emb_pos=None, emb_type=None, type_ids=None, pos=None):
    """The fused products of the decode step (include/mmtg_hip.h, mmtg_decode_gemm)."""
    _check(lib().mmtg_decode_gemm(int(mode), M, N, K, _p(A), K if lda is None else lda, _p(W), K if ldw is None else ldw, _p(C_),
                                  N if ldc is None else ldc, _p(bias), _p(colsum), _p(stats_in), int(np_in), float(eps), int(act),
                                  int(out_f32), _p(resid), N if ldr is None else ldr, _p(stats_out), int(splits), _p(ws),
                                  0 if ws is None else ws.numel(), _p(counters), 0 if counters is None else counters.numel(),
                                  _p(emb_pos), _p(emb_type), _p(type_ids), _p(pos), _stream()), "decode_gemm")


def decode_gemm_x3(mode, A, W, M, N, K, C_=None, Cp=None, ldc=None, bias=None, colsum=None, stats_in=None, np_in=0, eps=1e-5, act=EPI_NONE,
                   resid=None, ldr=None, stats_out=None, splits=1, ws=None, counters=None, emb_pos=None, emb_type=None, type_ids=None, pos=None):
    """The fused decode products on plane pairs (include/mmtg_hip.h, mmtg_decode_gemm_x3); A, W, Cp: Planes."""
    _check(lib().mmtg_decode_gemm_x3(int(mode), M, N, K, _p(A.t), A.ld, A.plane, _p(W.t), W.ld, W.plane, _p(C_), N if ldc is None else ldc,
                                     0 if Cp is None else _p(Cp.t), 0 if Cp is None else Cp.ld, 0 if Cp is None else Cp.plane,
                                     _p(bias), _p(colsum), _p(stats_in), int(np_in), float(eps), int(act), _p(resid), N if ldr is None else ldr,
                                     _p(stats_out), int(splits), _p(ws), 0 if ws is None else ws.numel(), _p(counters),
                                     0 if counters is None else counters.numel(), _p(emb_pos), _p(emb_type), _p(type_ids), _p(pos), _stream()),
           "decode_gemm_x3")


def ln_fold_weights_x3(W, gamma, beta, bias, Wf, colsum, bias_f, N, K):
    _check(lib().mmtg_ln_fold_weights_x3(_p(W.t), W.ld, W.plane, _p(gamma), _p(beta), _p(bias), _p(Wf.t), Wf.ld, Wf.plane, _p(colsum), _p(bias_f),
                                         N, K, _stream()), "ln_fold_weights_x3")


def decode_attn_split_x3(part, splits, bias, kcache, vcache, keep, pos, out, B, nH, dh, Tmax, rows=None):
    """rows (int32 [B, >= Tmax], beam search): the ancestry table -- the keys j < pos of row b come from cache row rows[b, j]."""
    if rows is not None:
        _check(lib().mmtg_decode_attn_split_x3_rows(_p(part), splits, _p(bias), _p(kcache), _p(vcache), _p(keep), keep.stride(0), _p(rows),
                                                    rows.stride(0), _p(pos), _p(out.t), out.plane, B, nH, dh, Tmax, _stream()),
               "decode_attn_split_x3_rows")
        return
    _check(lib().mmtg_decode_attn_split_x3(_p(part), splits, _p(bias), _p(kcache), _p(vcache), _p(keep), keep.stride(0), _p(pos), _p(out.t),
                                           out.plane, B, nH, dh, Tmax, _stream()), "decode_attn_split_x3")


def decode_embed_x3(table, seq, c, x, pos, tpw_type, tpw_mask, type_out, keep, B, P, S, E, two_sents, V, sent, max_sent_num):
    _check(lib().mmtg_decode_embed_x3(_p(table), _p(seq), seq.stride(0), _p(c), _p(x.t), x.plane, _p(pos), _p(tpw_type), _p(tpw_mask),
                                      _p(type_out), _p(keep), keep.stride(0), B, P, S, E, two_sents, V, sent, max_sent_num, _stream()),
           "decode_embed_x3")


def ln_fold_weights(W, gamma, beta, bias, Wf, colsum, bias_f, N, K, ldw=None):
    _check(lib().mmtg_ln_fold_weights(_p(W), K if ldw is None else ldw, _p(gamma), _p(beta), _p(bias), _p(Wf), _p(colsum), _p(bias_f),
                                      N, K, _stream()), "ln_fold_weights")


def decode_attn(qkv, kcache, vcache, keep, pos, out, B, nH, dh, Tmax):
    _check(lib().mmtg_decode_attn(dt(qkv), _p(qkv), _p(kcache), _p(vcache), _p(keep), keep.stride(0), _p(pos), _p(out),
                                  B, nH, dh, Tmax, _stream()), "decode_attn")


def decode_attn_split(part, splits, bias, kcache, vcache, keep, pos, out, B, nH, dh, Tmax, rows=None):
    """rows (int32 [B, >= Tmax], beam search): the ancestry table -- the keys j < pos of row b come from cache row rows[b, j]."""
    if rows is not None:
        _check(lib().mmtg_decode_attn_split_rows(dt(out), _p(part), splits, _p(bias), _p(kcache), _p(vcache), _p(keep), keep.stride(0),
                                                 _p(rows), rows.stride(0), _p(pos), _p(out), B, nH, dh, Tmax, _stream()),
               "decode_attn_split_rows")
        return
    _check(lib().mmtg_decode_attn_split(dt(out), _p(part), splits, _p(bias), _p(kcache), _p(vcache), _p(keep), keep.stride(0),
                                        _p(pos), _p(out), B, nH, dh, Tmax, _stream()), "decode_attn_split")


def _fixed(fixed_end, B):
    """The int32 [>= B] prefix-end array of the *_fixed entries (None is passed on: the library rejects it)."""
    if fixed_end is not None:
        if fixed_end.dtype != torch.int32 or fixed_end.dim() != 1 or fixed_end.numel() < B or not fixed_end.is_contiguous():
            raise ValueError("fixed_end must be a contiguous int32 vector of at least %d entries" % B)
    return _p(fixed_end)


def _lines(tables, B, V):
    """The line tables of decode.check_lines on the device, (lo, hi, sets or None, set_of or None), as the *_lines entries' trailing
    arguments (lo, hi, n_lines, sets, n_sets, set_of); shapes and dtypes are checked here, the values by check_lines."""
    lo, hi, sets, set_of = tables
    if not (lo.dtype == torch.uint8 and hi.dtype == torch.uint8 and lo.dim() == 2 and lo.shape == hi.shape and lo.shape[0] >= B
            and lo.is_contiguous() and hi.is_contiguous()):
        raise ValueError("line tables: lo / hi must be contiguous uint8 [rows >= %d, n_lines]" % B)
    if (sets is None) != (set_of is None):
        raise ValueError("line tables: sets and set_of come together")
    n_sets = 0
    if sets is not None:
        if not (sets.dtype == torch.int32 and sets.dim() == 2 and sets.shape[1] == (V + 31) // 32 and sets.is_contiguous()):
            raise ValueError("line tables: sets must be contiguous int32 [n_sets, ceil(V / 32) = %d]" % ((V + 31) // 32))
        if not (set_of.dtype == torch.int16 and set_of.shape == lo.shape and set_of.is_contiguous()):
            raise ValueError("line tables: set_of must be contiguous int16 of lo's shape")
        n_sets = sets.shape[0]
    return _p(lo), _p(hi), lo.shape[1], _p(sets), n_sets, _p(set_of)


def _template(tmpl, tables, B, sent):
    """The symbol table of decode.check_lines on the device, int32 [rows >= B, n_lines of the line tables, sent - 2] (None is passed
    on: the library rejects it)."""
    if tmpl is not None:
        if not (tmpl.dtype == torch.int32 and tmpl.dim() == 3 and tmpl.shape[0] >= B and tmpl.shape[1] == tables[0].shape[1]
                and tmpl.shape[2] == sent - 2 and tmpl.is_contiguous()):
            raise ValueError("template table must be contiguous int32 [rows >= %d, n_lines, sent - 2 = %d]" % (B, sent - 2))
    return _p(tmpl)


def _rhyme(rhyme, tables, B, V):
    """The rhyme tables of decode.check_lines on the device, (class_of int16 [V], lead int8 [rows >= B, n_lines of the line tables],
    distinct), as the *_rhyme entries' last arguments before the stream (None is passed on: the library rejects it)."""
    if rhyme is None:
        return _p(None), _p(None), 0
    class_of, lead, distinct = rhyme
    if not (class_of.dtype == torch.int16 and class_of.dim() == 1 and class_of.numel() >= V and class_of.is_contiguous()):
        raise ValueError("rhyme tables: class_of must be a contiguous int16 vector of at least V = %d entries" % V)
    if not (lead.dtype == torch.int8 and lead.dim() == 2 and lead.shape[0] >= B and lead.shape[1] == tables[0].shape[1]
            and lead.is_contiguous()):
        raise ValueError("rhyme tables: lead must be contiguous int8 [rows >= %d, n_lines]" % B)
    return _p(class_of), _p(lead), int(bool(distinct))


def _refrain(src, tables, B):
    """The refrain table of constraints.check_refrain on the device, int8 [rows >= B, n_lines] (of the line tables' width where there are
    any), as the *_refrain entries' last argument before the stream (None is passed on: the library rejects it)."""
    if src is not None:
        if not (src.dtype == torch.int8 and src.dim() == 2 and src.shape[0] >= B and 1 <= src.shape[1] <= 128 and src.is_contiguous()
                and (tables is None or src.shape[1] == tables[0].shape[1])):
            raise ValueError("refrain table: src must be contiguous int8 [rows >= %d, n_lines]" % B)
    return _p(src)


def _rule_tail(form, B, V, fixed_end, ngram, tables, tmpl=None, sent=0, rhyme=None, refrain=None):
    """What the selection entry of `form` ("" plain, "_fixed", "_ngram", "_lines", "_tmpl", "_rhyme", "_refrain") takes between its own
    arguments and the stream (the template table of "_rhyme" may be None: a scheme without templates; "_refrain" is the rhyme form's
    tail, whose tables may be None -- no line rule -- and whose rhyme may be None -- no rhyme scheme --, plus src)."""
    if form == "":
        return ()
    if form == "_refrain":
        if tables is None:
            if rhyme is not None or tmpl is not None:
                raise ValueError("refrain: templates / a rhyme scheme come with line tables")
            rule = (0, 0, 0 if refrain is None else refrain.shape[1], 0, 0, 0, 0, 0, 0, 0)
        else:
            rule = _lines(tables, B, V) + (_template(tmpl, tables, B, sent),) + _rhyme(rhyme, tables, B, V)
        return (_fixed(fixed_end, B), int(ngram)) + rule + (_refrain(refrain, tables, B),)
    tail = (_fixed(fixed_end, B),)
    if form != "_fixed":
        tail += (int(ngram),)
    if form in ("_lines", "_tmpl", "_rhyme"):
        tail += _lines(tables, B, V)
    if form in ("_tmpl", "_rhyme"):
        tail += (_template(tmpl, tables, B, sent),)
    if form == "_rhyme":
        tail += _rhyme(rhyme, tables, B, V)
    return tail


def _select(form, logits, ldl, V, seq, pos, P, sent, temperature, rep_penalty, B, pos_next, sampling=None, fixed_end=None, ngram=0,
            tables=None, tmpl=None, rhyme=None, refrain=None):
    """mmtg_decode_select<form>, or with sampling = (top_k, top_p, uniforms) mmtg_decode_sample<form>."""
    name = ("decode_select" if sampling is None else "decode_sample") + form
    draw = () if sampling is None else (int(sampling[0]), float(sampling[1]), _p(sampling[2]), sampling[2].stride(0))
    _check(getattr(lib(), "mmtg_" + name)(_p(logits), ldl, V, _p(seq), seq.stride(0), _p(pos), P, sent, float(temperature),
                                          float(rep_penalty), *draw, B, _p(pos_next),
                                          *_rule_tail(form, B, V, fixed_end, ngram, tables, tmpl, sent, rhyme, refrain), _stream()), name)


def decode_sample_warp(logits, ldl, V, seq, pos, P, sent, temperature, rep_penalty, top_k, top_p, warp, uniforms, B, src, tables=None,
                       rhyme=None, tmpl=None, ngram=0, pos_next=None, fixed_end=None):
    """mmtg_decode_sample_warp: the refrain form's draw with warp = (min_p, typical_p, epsilon_cutoff, eta_cutoff) (include/mmtg_hip.h).
    src is required (int8 [rows >= B, n_lines], all -1 without a refrain); every other table may be None."""
    _check(lib().mmtg_decode_sample_warp(_p(logits), ldl, V, _p(seq), seq.stride(0), _p(pos), P, sent, float(temperature),
                                         float(rep_penalty), int(top_k), float(top_p), *check_warp(*warp), _p(uniforms),
                                         0 if uniforms is None else uniforms.stride(0), B, _p(pos_next),
                                         *_rule_tail("_refrain", B, V, fixed_end, ngram, tables, tmpl, sent, rhyme, src), _stream()),
           "decode_sample_warp")


def decode_sample_mirostat(logits, ldl, V, seq, pos, P, sent, temperature, rep_penalty, top_k, top_p, warp, mirostat, mu, uniforms, B, src,
                           tables=None, rhyme=None, tmpl=None, ngram=0, pos_next=None, fixed_end=None):
    """mmtg_decode_sample_mirostat: decode_sample_warp's draw with mirostat = (tau, eta) and the rows' state mu (f32 [B], read and
    written) behind the four stages of warp (include/mmtg_hip.h)."""
    tau, eta = check_mirostat(*mirostat)
    if tau == 0.0:
        raise ValueError("mirostat_tau must be in (0, 32] here: 0 (off) is decode_sample_warp")
    _check(lib().mmtg_decode_sample_mirostat(_p(logits), ldl, V, _p(seq), seq.stride(0), _p(pos), P, sent, float(temperature),
                                             float(rep_penalty), int(top_k), float(top_p), *check_warp(*warp), _p(uniforms),
                                             0 if uniforms is None else uniforms.stride(0), B, _p(pos_next),
                                             *_rule_tail("_refrain", B, V, fixed_end, ngram, tables, tmpl, sent, rhyme, src), tau, eta,
                                             _p(mu), _stream()),
           "decode_sample_mirostat")


def _beam_candidates(form, logits, ldl, V, seq, pos, P, sent, temperature, rep_penalty, nb, cand_val, cand_id, B, fixed_end=None, ngram=0,
                     tables=None, tmpl=None, rhyme=None, refrain=None):
    name = "decode_beam_candidates" + form
    _check(getattr(lib(), "mmtg_" + name)(_p(logits), ldl, V, _p(seq), seq.stride(0), _p(pos), P, sent, float(temperature),
                                          float(rep_penalty), int(nb), _p(cand_val), _p(cand_id), B,
                                          *_rule_tail(form, B, V, fixed_end, ngram, tables, tmpl, sent, rhyme, refrain), _stream()), name)


def _beam_merge(form, cand_val, cand_id, scores, seq, keep, rows, pos, P, sent, nb, n_prompts, pos_next, fixed_end=None, groups=1,
                diversity_penalty=0.0):
    """mmtg_decode_beam_merge<form>, form "" / "_fixed" or, for the grouped merge, "_groups" / "_groups_fixed" (the held form's
    tail, then groups and the penalty)."""
    name = "decode_beam_merge" + form
    grouped = form.startswith("_groups")
    tail = _rule_tail(form[len("_groups"):] if grouped else form, n_prompts * nb, 0, fixed_end, 0, None)
    if grouped:
        tail += (int(groups), float(diversity_penalty))
    _check(getattr(lib(), "mmtg_" + name)(_p(cand_val), _p(cand_id), _p(scores), _p(seq), seq.stride(0), _p(keep), keep.stride(0),
                                          _p(rows), rows.stride(0), _p(pos), P, sent, int(nb), int(n_prompts), _p(pos_next),
                                          *tail, _stream()), name)


def decode_select(logits, ldl, V, seq, pos, P, sent, temperature, rep_penalty, B, pos_next=None):
    _select("", logits, ldl, V, seq, pos, P, sent, temperature, rep_penalty, B, pos_next)


def decode_sample(logits, ldl, V, seq, pos, P, sent, temperature, rep_penalty, top_k, top_p, uniforms, B, pos_next=None):
    _select("", logits, ldl, V, seq, pos, P, sent, temperature, rep_penalty, B, pos_next, (top_k, top_p, uniforms))


def decode_beam_candidates(logits, ldl, V, seq, pos, P, sent, temperature, rep_penalty, nb, cand_val, cand_id, B):
    """Per row: the nb best (log-probability, id) continuations of the processed logits (include/mmtg_hip.h)."""
    _beam_candidates("", logits, ldl, V, seq, pos, P, sent, temperature, rep_penalty, nb, cand_val, cand_id, B)


def decode_beam_merge(cand_val, cand_id, scores, seq, keep, rows, pos, P, sent, nb, n_prompts, pos_next=None):
    """Per prompt: keep the nb best candidates, reorder seq / keep / rows in place, append (include/mmtg_hip.h)."""
    _beam_merge("", cand_val, cand_id, scores, seq, keep, rows, pos, P, sent, nb, n_prompts, pos_next)


def decode_select_fixed(logits, ldl, V, seq, pos, P, sent, temperature, rep_penalty, B, fixed_end, pos_next=None):
    """decode_select that leaves row b's column pos + 1 alone while pos + 1 < fixed_end[b] (a host-written prefix, include/mmtg_hip.h)."""
    _select("_fixed", logits, ldl, V, seq, pos, P, sent, temperature, rep_penalty, B, pos_next, fixed_end=fixed_end)


def decode_sample_fixed(logits, ldl, V, seq, pos, P, sent, temperature, rep_penalty, top_k, top_p, uniforms, B, fixed_end, pos_next=None):
    _select("_fixed", logits, ldl, V, seq, pos, P, sent, temperature, rep_penalty, B, pos_next, (top_k, top_p, uniforms), fixed_end=fixed_end)


def decode_beam_candidates_fixed(logits, ldl, V, seq, pos, P, sent, temperature, rep_penalty, nb, cand_val, cand_id, B, fixed_end):
    """decode_beam_candidates; a row on a prefix column (pos + 1 < fixed_end[b]) offers nothing."""
    _beam_candidates("_fixed", logits, ldl, V, seq, pos, P, sent, temperature, rep_penalty, nb, cand_val, cand_id, B, fixed_end=fixed_end)


def decode_beam_merge_fixed(cand_val, cand_id, scores, seq, keep, rows, pos, P, sent, nb, n_prompts, fixed_end, pos_next=None):
    """decode_beam_merge; a prompt on a prefix column keeps every beam, score and token (include/mmtg_hip.h)."""
    _beam_merge("_fixed", cand_val, cand_id, scores, seq, keep, rows, pos, P, sent, nb, n_prompts, pos_next, fixed_end=fixed_end)


def decode_beam_merge_groups(cand_val, cand_id, scores, seq, keep, rows, pos, P, sent, nb, n_prompts, groups, diversity_penalty,
                             pos_next=None):
    """decode_beam_merge over `groups` beam groups per prompt, a later group penalised by diversity_penalty per earlier slot that
    chose the same content id at this step; the stored scores are unpenalised (include/mmtg_hip.h)."""
    _beam_merge("_groups", cand_val, cand_id, scores, seq, keep, rows, pos, P, sent, nb, n_prompts, pos_next, groups=groups,
                diversity_penalty=diversity_penalty)


def decode_beam_merge_groups_fixed(cand_val, cand_id, scores, seq, keep, rows, pos, P, sent, nb, n_prompts, fixed_end, groups,
                                   diversity_penalty, pos_next=None):
    """decode_beam_merge_groups; a prompt on a prefix column keeps every beam, score and token (include/mmtg_hip.h)."""
    _beam_merge("_groups_fixed", cand_val, cand_id, scores, seq, keep, rows, pos, P, sent, nb, n_prompts, pos_next, fixed_end=fixed_end,
                groups=groups, diversity_penalty=diversity_penalty)


def decode_select_ngram(logits, ldl, V, seq, pos, P, sent, temperature, rep_penalty, B, ngram, fixed_end=None, pos_next=None):
    """decode_select that never writes a content n-gram (n = ngram) the row already holds (include/mmtg_hip.h); fixed_end: as
    decode_select_fixed, or None (no prefix)."""
    _select("_ngram", logits, ldl, V, seq, pos, P, sent, temperature, rep_penalty, B, pos_next, fixed_end=fixed_end, ngram=ngram)


def decode_sample_ngram(logits, ldl, V, seq, pos, P, sent, temperature, rep_penalty, top_k, top_p, uniforms, B, ngram, fixed_end=None,
                        pos_next=None):
    _select("_ngram", logits, ldl, V, seq, pos, P, sent, temperature, rep_penalty, B, pos_next, (top_k, top_p, uniforms),
            fixed_end=fixed_end, ngram=ngram)


def decode_beam_candidates_ngram(logits, ldl, V, seq, pos, P, sent, temperature, rep_penalty, nb, cand_val, cand_id, B, ngram,
                                 fixed_end=None):
    """decode_beam_candidates with the n-gram bans of decode_select_ngram applied before the log_softmax and the top nb."""
    _beam_candidates("_ngram", logits, ldl, V, seq, pos, P, sent, temperature, rep_penalty, nb, cand_val, cand_id, B, fixed_end=fixed_end,
                     ngram=ngram)


def decode_select_lines(logits, ldl, V, seq, pos, P, sent, temperature, rep_penalty, B, tables, ngram=0, fixed_end=None, pos_next=None):
    """decode_select_ngram (ngram may be 0) under the line-length bounds and line-end sets of `tables` (include/mmtg_hip.h)."""
    _select("_lines", logits, ldl, V, seq, pos, P, sent, temperature, rep_penalty, B, pos_next, fixed_end=fixed_end, ngram=ngram,
            tables=tables)


def decode_sample_lines(logits, ldl, V, seq, pos, P, sent, temperature, rep_penalty, top_k, top_p, uniforms, B, tables, ngram=0,
                        fixed_end=None, pos_next=None):
    _select("_lines", logits, ldl, V, seq, pos, P, sent, temperature, rep_penalty, B, pos_next, (top_k, top_p, uniforms),
            fixed_end=fixed_end, ngram=ngram, tables=tables)


def decode_beam_candidates_lines(logits, ldl, V, seq, pos, P, sent, temperature, rep_penalty, nb, cand_val, cand_id, B, tables, ngram=0,
                                 fixed_end=None):
    """decode_beam_candidates_ngram (ngram may be 0) under the line rule: a full line offers PAD the way sticky PAD does."""
    _beam_candidates("_lines", logits, ldl, V, seq, pos, P, sent, temperature, rep_penalty, nb, cand_val, cand_id, B, fixed_end=fixed_end,
                     ngram=ngram, tables=tables)


def decode_select_tmpl(logits, ldl, V, seq, pos, P, sent, temperature, rep_penalty, B, tables, tmpl, ngram=0, fixed_end=None,
                       pos_next=None):
    """decode_select_lines under the line templates of `tmpl` (include/mmtg_hip.h): a given column writes its id, a class column is
    confined to the class."""
    _select("_tmpl", logits, ldl, V, seq, pos, P, sent, temperature, rep_penalty, B, pos_next, fixed_end=fixed_end, ngram=ngram,
            tables=tables, tmpl=tmpl)


def decode_sample_tmpl(logits, ldl, V, seq, pos, P, sent, temperature, rep_penalty, top_k, top_p, uniforms, B, tables, tmpl, ngram=0,
                       fixed_end=None, pos_next=None):
    _select("_tmpl", logits, ldl, V, seq, pos, P, sent, temperature, rep_penalty, B, pos_next, (top_k, top_p, uniforms),
            fixed_end=fixed_end, ngram=ngram, tables=tables, tmpl=tmpl)


def decode_beam_candidates_tmpl(logits, ldl, V, seq, pos, P, sent, temperature, rep_penalty, nb, cand_val, cand_id, B, tables, tmpl,
                                ngram=0, fixed_end=None):
    """decode_beam_candidates_lines under the line templates: a given column offers its id the way a full line offers PAD."""
    _beam_candidates("_tmpl", logits, ldl, V, seq, pos, P, sent, temperature, rep_penalty, nb, cand_val, cand_id, B, fixed_end=fixed_end,
                     ngram=ngram, tables=tables, tmpl=tmpl)


def decode_select_rhyme(logits, ldl, V, seq, pos, P, sent, temperature, rep_penalty, B, tables, rhyme, tmpl=None, ngram=0,
                        fixed_end=None, pos_next=None):
    """decode_select_tmpl (tmpl may be None) under the rhyme tables `rhyme` = (class_of, lead, distinct) of include/mmtg_hip.h: a
    follower line ends in the class its leader's last content id has."""
    _select("_rhyme", logits, ldl, V, seq, pos, P, sent, temperature, rep_penalty, B, pos_next, fixed_end=fixed_end, ngram=ngram,
            tables=tables, tmpl=tmpl, rhyme=rhyme)


def decode_sample_rhyme(logits, ldl, V, seq, pos, P, sent, temperature, rep_penalty, top_k, top_p, uniforms, B, tables, rhyme,
                        tmpl=None, ngram=0, fixed_end=None, pos_next=None):
    _select("_rhyme", logits, ldl, V, seq, pos, P, sent, temperature, rep_penalty, B, pos_next, (top_k, top_p, uniforms),
            fixed_end=fixed_end, ngram=ngram, tables=tables, tmpl=tmpl, rhyme=rhyme)


def decode_beam_candidates_rhyme(logits, ldl, V, seq, pos, P, sent, temperature, rep_penalty, nb, cand_val, cand_id, B, tables, rhyme,
                                 tmpl=None, ngram=0, fixed_end=None):
    """decode_beam_candidates_tmpl under the rhyme tables: every beam reads its own (reordered) history for its leader's rhyme."""
    _beam_candidates("_rhyme", logits, ldl, V, seq, pos, P, sent, temperature, rep_penalty, nb, cand_val, cand_id, B, fixed_end=fixed_end,
                     ngram=ngram, tables=tables, tmpl=tmpl, rhyme=rhyme)


def decode_select_refrain(logits, ldl, V, seq, pos, P, sent, temperature, rep_penalty, B, src, tables=None, rhyme=None, tmpl=None, ngram=0,
                          fixed_end=None, pos_next=None):
    """decode_select_rhyme (tables None: no line rule; rhyme None: no rhyme scheme) under the refrain table `src` of include/mmtg_hip.h:
    on a copy column the row writes the id its own history holds at that column of the source line.  logits may be None (a step that
    skipped the head): copy columns and the forced cadence are written, nothing else."""
    _select("_refrain", logits, ldl, V, seq, pos, P, sent, temperature, rep_penalty, B, pos_next, fixed_end=fixed_end, ngram=ngram,
            tables=tables, tmpl=tmpl, rhyme=rhyme, refrain=src)


def decode_sample_refrain(logits, ldl, V, seq, pos, P, sent, temperature, rep_penalty, top_k, top_p, uniforms, B, src, tables=None,
                          rhyme=None, tmpl=None, ngram=0, fixed_end=None, pos_next=None):
    _select("_refrain", logits, ldl, V, seq, pos, P, sent, temperature, rep_penalty, B, pos_next, (top_k, top_p, uniforms),
            fixed_end=fixed_end, ngram=ngram, tables=tables, tmpl=tmpl, rhyme=rhyme, refrain=src)


def decode_beam_candidates_refrain(logits, ldl, V, seq, pos, P, sent, temperature, rep_penalty, nb, cand_val, cand_id, B, src, tables=None,
                                   rhyme=None, tmpl=None, ngram=0, fixed_end=None):
    """decode_beam_candidates_rhyme under the refrain table: a row on a copy column offers the source's id the way a template's given id
    is offered; every beam copies from its own (reordered) history."""
    _beam_candidates("_refrain", logits, ldl, V, seq, pos, P, sent, temperature, rep_penalty, nb, cand_val, cand_id, B, fixed_end=fixed_end,
                     ngram=ngram, tables=tables, tmpl=tmpl, rhyme=rhyme, refrain=src)


def _keywords(keywords, n_prompts):
    """The keyword tables of constraints.check_keywords on the device, (phrases int32 [prompts, 8, 4], lens int8 [prompts, 8], K,
    the longest phrase), as the *_kw candidates entry takes them (phrases, phrase_len, K, phrase_cap)."""
    phrases, lens, K, cap = keywords
    if not (phrases.dtype == torch.int32 and phrases.dim() == 3 and phrases.shape[0] >= n_prompts and tuple(phrases.shape[1:]) == (8, 4)
            and phrases.is_contiguous()):
        raise ValueError("keyword tables: phrases must be contiguous int32 [prompts >= %d, 8, 4]" % n_prompts)
    if not (lens.dtype == torch.int8 and lens.dim() == 2 and lens.shape[0] >= n_prompts and lens.shape[1] == 8 and lens.is_contiguous()):
        raise ValueError("keyword tables: lens must be contiguous int8 [prompts >= %d, 8]" % n_prompts)
    return _p(phrases), _p(lens), int(K), int(cap)


def _cand_tables(cand_val, cand_id, cand_bank, B, W):
    if cand_val is None and cand_id is None:
        return
    for t, dt in ((cand_val, torch.float32), (cand_id, torch.int32), (cand_bank, torch.int32)):
        if t is None or t.dtype != dt or t.dim() != 2 or t.shape[0] < B or t.shape[1] != W or not t.is_contiguous():
            raise ValueError("keyword candidates: cand_val fp32 / cand_id int32 / cand_bank int32 must be contiguous [rows >= %d, nb + K = %d]"
                             % (B, W))


def decode_beam_candidates_kw(logits, ldl, V, seq, pos, P, sent, temperature, rep_penalty, nb, cand_val, cand_id, cand_bank, B, keywords,
                              tables=None, rhyme=None, tmpl=None, ngram=0, fixed_end=None):
    """decode_beam_candidates_rhyme (tables None: no line rule at all; rhyme None with tables: the caller's lead table says no line
    has a leader) offering nb + K slots per row, the last K the keywords' next ids, and each slot's bank (include/mmtg_hip.h).
    keywords: (phrases, lens, K, longest phrase) on the device; cand_val / cand_id / cand_bank are [B, nb + K]."""
    kw = _keywords(keywords, B // max(int(nb), 1))
    _cand_tables(cand_val, cand_id, cand_bank, B, int(nb) + kw[2])
    if tables is None:
        if rhyme is not None or tmpl is not None:
            raise ValueError("keyword candidates: templates / a rhyme scheme come with line tables")
        rule = (_fixed(fixed_end, B), int(ngram), 0, 0, 0, 0, 0, 0, 0, 0, 0, 0)
    else:
        rule = _rule_tail("_rhyme", B, V, fixed_end, ngram, tables, tmpl, sent, rhyme)
    _check(lib().mmtg_decode_beam_candidates_kw(_p(logits), ldl, V, _p(seq), seq.stride(0), _p(pos), P, sent, float(temperature),
                                                float(rep_penalty), int(nb), _p(cand_val), _p(cand_id), B, *rule, *kw, _p(cand_bank),
                                                _stream()), "decode_beam_candidates_kw")


def decode_beam_merge_kw(cand_val, cand_id, cand_bank, scores, seq, keep, rows, pos, P, sent, nb, n_prompts, K, fixed_end=None,
                         pos_next=None):
    """decode_beam_merge (fixed_end given: decode_beam_merge_fixed) over nb + K candidates per parent and their banks: the nb places
    go to the best of every bank, highest bank first, then the second best of every bank, and so on (include/mmtg_hip.h)."""
    _cand_tables(cand_val, cand_id, cand_bank, n_prompts * nb, int(nb) + int(K))
    held = () if fixed_end is None else (_fixed(fixed_end, n_prompts * nb),)
    name = "decode_beam_merge_kw" + ("_fixed" if held else "")
    _check(getattr(lib(), "mmtg_" + name)(_p(cand_val), _p(cand_id), _p(cand_bank), _p(scores), _p(seq), seq.stride(0), _p(keep),
                                          keep.stride(0), _p(rows), rows.stride(0), _p(pos), P, sent, int(nb), int(n_prompts), _p(pos_next),
                                          *held, int(K), _stream()), name)


def decode_beam_merge_kw_fixed(cand_val, cand_id, cand_bank, scores, seq, keep, rows, pos, P, sent, nb, n_prompts, fixed_end, K,
                               pos_next=None):
    """decode_beam_merge_kw; a prompt on a prefix column keeps every beam, score and token (include/mmtg_hip.h)."""
    if fixed_end is None:
        raise ValueError("decode_beam_merge_kw_fixed needs fixed_end")
    decode_beam_merge_kw(cand_val, cand_id, cand_bank, scores, seq, keep, rows, pos, P, sent, nb, n_prompts, K, fixed_end=fixed_end,
                         pos_next=pos_next)


def decode_logprob(logits, ldl, V, seq, pos, P, out, B):
    """out[b, pos + 1 - P] = log_softmax(logits[b, :V])[seq[b, pos + 1]] over the raw fp32 logits (include/mmtg_hip.h,
    mmtg_decode_logprob); out is fp32 [B, ncols], and a column outside it or an id outside 0 .. V - 1 writes nothing."""
    if out.dtype != torch.float32 or out.dim() != 2 or out.stride(1) != 1:
        raise ValueError("out must be fp32 [B, ncols] with unit column stride")
    _check(lib().mmtg_decode_logprob(_p(logits), ldl, V, _p(seq), seq.stride(0), _p(pos), P, _p(out), out.stride(0), out.shape[1], B,
                                     _stream()), "decode_logprob")


def decode_contrastive_sim(x, gamma, beta, eps, hc, sim, keep, rows, pos, P, B, D, scores=None):
    """Per row: u = unit(ln_f(x[b])) into hc[b, pos - P] and sim[b] = the largest dot(u, hc[rows[b, t], t - P]) over the row's kept
    lyric columns t in [P, pos), 0 for none (include/mmtg_hip.h, mmtg_decode_contrastive_sim).  hc is fp32 [B, hc_len, D]."""
    if hc.dtype != torch.float32 or hc.dim() != 3 or not hc.is_contiguous() or hc.shape[0] != B or hc.shape[2] != D:
        raise ValueError("hc must be a contiguous fp32 [B, hc_len, D]")
    if gamma.dtype != torch.float32 or beta.dtype != torch.float32 or sim.dtype != torch.float32:
        raise ValueError("gamma, beta and sim must be fp32")
    _check(lib().mmtg_decode_contrastive_sim(dt(x), _p(x), x.stride(0), _p(gamma), _p(beta), float(eps), _p(hc), hc.shape[1], _p(sim),
                                             _p(scores), _p(keep), keep.stride(0), _p(rows), rows.stride(0), _p(pos), P, int(B), int(D),
                                             _stream()), "decode_contrastive_sim")


def decode_contrastive_merge(cand_val, cand_id, scores, sim, total, alpha, seq, keep, rows, pos, P, sent, k, n_prompts, pos_next=None,
                             fixed_end=None):
    """Per prompt: keep the row r* with the best (1 - alpha) * exp(score) - alpha * sim, give its column pos to every row, append the
    next candidates (include/mmtg_hip.h, mmtg_decode_contrastive_merge)."""
    _check(lib().mmtg_decode_contrastive_merge(_p(cand_val), _p(cand_id), _p(scores), _p(sim), _p(total), float(alpha), _p(seq),
                                               seq.stride(0), _p(keep), keep.stride(0), _p(rows), rows.stride(0), _p(pos), P, sent, int(k),
                                               int(n_prompts), _p(pos_next), _p(fixed_end), _stream()), "decode_contrastive_merge")


def _gumbel_state(what, B, nb, scores, gum, row_seed, cand_g):
    """The per-row state of stochastic beam search: scores / gum fp32 [>= B], row_seed int32 [>= B] (the library reads its words as
    uint32), cand_g fp32 [>= B, nb] (None for the merge of a step without candidates).  None is passed on: the library rejects it."""
    for name, t, dtype, n in (("scores", scores, torch.float32, B), ("gum", gum, torch.float32, B), ("row_seed", row_seed, torch.int32, B),
                              ("cand_g", cand_g, torch.float32, B * nb)):
        if t is not None and (t.dtype != dtype or t.numel() < n or not t.is_contiguous()):
            raise ValueError("%s: %s must be a contiguous %s tensor of at least %d entries" % (what, name, dtype, n))


def decode_gumbel_candidates(logits, ldl, V, seq, pos, P, sent, temperature, rep_penalty, nb, cand_val, cand_id, cand_g, scores, gum,
                             row_seed, B, src, tables=None, rhyme=None, tmpl=None, ngram=0, fixed_end=None):
    """Per row: its nb largest t_v = log_softmax(x)[v] + Gumbel noise, as (cand_id, cand_val = the log-probability, cand_g = the
    child's perturbed value given the row's own gum[b]) (include/mmtg_hip.h, mmtg_decode_gumbel_candidates).  The rule is the refrain
    form's: src is required (int8 [rows >= B, n_lines], all -1 without a refrain); every other table may be None."""
    _gumbel_state("decode_gumbel_candidates", B, nb, scores, gum, row_seed, cand_g)
    _check(lib().mmtg_decode_gumbel_candidates(_p(logits), ldl, V, _p(seq), seq.stride(0), _p(pos), P, sent, float(temperature),
                                               float(rep_penalty), int(nb), _p(cand_val), _p(cand_id), B,
                                               *_rule_tail("_refrain", B, V, fixed_end, ngram, tables, tmpl, sent, rhyme, src),
                                               _p(scores), _p(gum), _p(row_seed), _p(cand_g), _stream()), "decode_gumbel_candidates")


def decode_gumbel_merge(cand_val, cand_id, cand_g, scores, gum, seq, keep, rows, pos, P, sent, nb, n_prompts, pos_next=None,
                        fixed_end=None):
    """Per prompt: keep the nb candidates with the largest cand_g (then parent, then rank), reorder seq / keep / rows as the beam merge
    does, append the ids, scores[b] = scores[parent] + cand_val, gum[b] = cand_g (include/mmtg_hip.h, mmtg_decode_gumbel_merge).
    cand_val / cand_id / cand_g None: a step without candidates (the beam merge's identity; gum untouched)."""
    _gumbel_state("decode_gumbel_merge", n_prompts * nb, nb, scores, gum, None, cand_g)
    _check(lib().mmtg_decode_gumbel_merge(_p(cand_val), _p(cand_id), _p(cand_g), _p(scores), _p(gum), _p(seq), seq.stride(0), _p(keep),
                                          keep.stride(0), _p(rows), rows.stride(0), _p(pos), P, sent, int(nb), int(n_prompts),
                                          _p(pos_next), _fixed(fixed_end, n_prompts * nb), _stream()), "decode_gumbel_merge")


def decode_guidance(cond, uncond, ldl, V, scale, out, N):
    """out[b, :V] = lu + scale * (lc - lu), lc / lu the log-softmax of cond[b, :V] / uncond[b, :V], for b < N (include/mmtg_hip.h,
    mmtg_decode_guidance).  cond and uncond are fp32 row starts ldl apart; out is fp32 [>= N, >= V]; columns V .. stay as they are."""
    if cond.dtype != torch.float32 or uncond.dtype != torch.float32 or out.dtype != torch.float32:
        raise ValueError("cond, uncond and out must be fp32")
    if out.dim() != 2 or out.stride(1) != 1 or out.shape[0] < N:
        raise ValueError("out must be fp32 [>= N, >= V] with unit column stride")
    _check(lib().mmtg_decode_guidance(_p(cond), _p(uncond), int(ldl), int(V), float(scale), _p(out), out.stride(0), int(N), _stream()),
           "decode_guidance")


def decode_mirror(seq, pos, N):
    """seq[N + b, pos + 1] = seq[b, pos + 1] for b < N, where the column exists (include/mmtg_hip.h, mmtg_decode_mirror).  seq is
    int64 [>= 2 N, ld]; pos is the position slot the selection left alone."""
    if seq.dtype != torch.long or seq.dim() != 2 or seq.stride(1) != 1 or seq.shape[0] < 2 * N:
        raise ValueError("seq must be int64 [>= 2 N, ld] with unit column stride")
    _check(lib().mmtg_decode_mirror(_p(seq), seq.stride(0), _p(pos), int(N), _stream()), "decode_mirror")


GUIDANCE_FORMS = {"auto": 0, "resident": 1, "reread": 2}


def decode_guidance_multi(logits, ldl, V, scales, out, N, form="auto"):
    """out[b, :V] = lc + sum_k (scales[k - 1] - 1) * (lc - l_k), k = 1 .. K - 1 = len(scales), lc / l_k the log-softmax of
    logits[b, :V] / logits[k N + b, :V], for b < N (include/mmtg_hip.h, mmtg_decode_guidance_multi).  logits is fp32 [>= K N, >= V]
    with rows ldl apart; scales are host numbers, handed to the kernel by value; out is fp32 [>= N, >= V]; columns V .. stay as
    they are.  form: "auto" (the entry's own choice), "resident" or "reread" (mmtg_decode_guidance_multi_form)."""
    K = len(scales) + 1
    if logits.dtype != torch.float32 or out.dtype != torch.float32:
        raise ValueError("logits and out must be fp32")
    if logits.dim() != 2 or logits.stride(1) != 1 or logits.stride(0) != ldl or logits.shape[0] < K * N:
        raise ValueError("logits must be fp32 [>= K N, >= V] with unit column stride and rows ldl apart")
    if out.dim() != 2 or out.stride(1) != 1 or out.shape[0] < N:
        raise ValueError("out must be fp32 [>= N, >= V] with unit column stride")
    if form not in GUIDANCE_FORMS:
        raise ValueError("form must be one of %s, got %r" % (sorted(GUIDANCE_FORMS), form))
    host = (C.c_float * max(K - 1, 1))(*[float(s) for s in scales])
    if form == "auto":
        rc = lib().mmtg_decode_guidance_multi(_p(logits), int(ldl), int(V), K, host, _p(out), out.stride(0), int(N), _stream())
    else:
        rc = lib().mmtg_decode_guidance_multi_form(_p(logits), int(ldl), int(V), K, host, _p(out), out.stride(0), int(N),
                                                   GUIDANCE_FORMS[form], _stream())
    _check(rc, "decode_guidance_multi")


def decode_mirror_multi(seq, pos, N, K):
    """seq[k N + b, pos + 1] = seq[b, pos + 1] for k = 1 .. K - 1 and b < N, where the column exists (include/mmtg_hip.h,
    mmtg_decode_mirror_multi).  seq is int64 [>= K N, ld]; pos is the position slot the selection left alone."""
    if seq.dtype != torch.long or seq.dim() != 2 or seq.stride(1) != 1 or seq.shape[0] < K * N:
        raise ValueError("seq must be int64 [>= K N, ld] with unit column stride")
    _check(lib().mmtg_decode_mirror_multi(_p(seq), seq.stride(0), _p(pos), int(N), int(K), _stream()), "decode_mirror_multi")


# the training side of guidance (the rules: include/mmtg_hip.h; csrc/guidance_train.hip)
GUIDED_MAX_SCALES = 8


def drop_thresholds(probs):
    """(p_both, p_img, p_txt) -> the cumulative 64-bit thresholds (c_both, c_img, c_txt) of mmtg_experience_drop: each share is
    min(int(p * 2**32), 2**32) in float64, accumulated."""
    out, acc = [], 0
    for p in probs:
        acc += min(int(float(p) * 4294967296.0), 4294967296)
        out.append(acc)
    return tuple(out)


def experience_drop(img, txt, img_out, txt_out, code, B, n, seed, thresholds):
    """img_out / txt_out [B, n] (fp32 or bf16) = img / txt (fp32, never written) with the rows of dropped samples +0.0; code int32 [B]
    (bit 0: images dropped, bit 1: texts dropped).  thresholds: (c_both, c_img, c_txt) as drop_thresholds gives them."""
    if img.dtype != torch.float32 or txt.dtype != torch.float32 or code.dtype != torch.int32 or img_out.dtype != txt_out.dtype:
        raise ValueError("img and txt must be fp32, code int32, img_out and txt_out of one dtype")
    c_both, c_img, c_txt = (int(c) for c in thresholds)
    _check(lib().mmtg_experience_drop(dt(img_out), _p(img), _p(txt), _p(img_out), _p(txt_out), _p(code), int(B), int(n),
                                      int(seed) & 0xFFFFFFFF, c_both, c_img, c_txt, _stream()), "experience_drop")


def guided_loss(cond, uncond, ldl, V, lse_c, lse_u, topic_ids, targets, scales, B, P, L, batch_den, nll, sample_ce, ce):
    """nll [K, M], sample_ce [K, B] and ce [K] (fp32): the cross-entropy of the lyric under softmax(lu + s_k (lc - lu)) for the K <= 8
    host floats `scales`, from the two logits matrices (one storage type, row stride ldl) and their row lse of loss_fwd."""
    if cond.dtype != uncond.dtype:
        raise ValueError("cond and uncond must have one storage type")
    K = len(scales)
    arr = (C.c_float * max(K, 1))(*[float(s) for s in scales])
    _check(lib().mmtg_guided_loss(dt(cond), _p(cond), _p(uncond), int(ldl), int(V), _p(lse_c), _p(lse_u), _p(topic_ids), _p(targets),
                                  C.addressof(arr), K, int(B), int(P), int(L), float(batch_den), _p(nll), _p(sample_ce), _p(ce),
                                  _stream()), "guided_loss")


GUIDED_MAX_BRANCHES = 4


def guided_loss_multi(mats, lses, ldl, V, targets, scale_tuples, B, P, L, batch_den, nll, sample_ce, ce):
    """nll [G, M], sample_ce [G, B] and ce [G] (fp32): the cross-entropy of the lyric under lc + sum_k (s_k - 1) (lc - l_k), the rule of
    decode_guidance_multi, for the G <= 8 tuples of K - 1 host floats `scale_tuples`, from the K = 2 .. 4 logits matrices `mats`
    (mats[0] the conditional one; one storage type, row stride ldl) and their row lse of loss_fwd `lses`."""
    K, G = len(mats), len(scale_tuples)
    if len(lses) != K:
        raise ValueError("guided_loss_multi: %d logits matrices beside %d lse vectors" % (K, len(lses)))
    if any(m.dtype != mats[0].dtype for m in mats[1:]):
        raise ValueError("guided_loss_multi: the logits matrices must have one storage type")
    if any(len(t) != K - 1 for t in scale_tuples):
        raise ValueError("guided_loss_multi: every scale tuple holds K - 1 = %d scales" % (K - 1))
    xs = (C.c_void_p * max(K, 1))(*[_p(m) for m in mats])
    ls = (C.c_void_p * max(K, 1))(*[_p(v) for v in lses])
    arr = (C.c_float * max(G * (K - 1), 1))(*[float(s) for t in scale_tuples for s in t])
    _check(lib().mmtg_guided_loss_multi(dt(mats[0]) if K else F32, C.addressof(xs), C.addressof(ls), K, int(ldl), int(V), _p(targets),
                                        C.addressof(arr), G, int(B), int(P), int(L), float(batch_den), _p(nll), _p(sample_ce), _p(ce),
                                        _stream()), "guided_loss_multi")


# distillation of a teacher's (guided) distribution (the rule: include/mmtg_hip.h; csrc/distill.hip)
def _teacher(cond, uncond, lse_u):
    if (uncond is None) != (lse_u is None):
        raise ValueError("uncond and lse_u are given together or not at all")
    if uncond is not None and (uncond.dtype != cond.dtype or uncond.shape != cond.shape):
        raise ValueError("cond and uncond must have one storage type and shape")


def distill_fwd(logits, ldl, cond, uncond, ldt, V, lse, lse_c, lse_u, scale, B, P, L, batch_den, kd_row, kd_lg, kd_sample, kd):
    """kd_row [M], kd_lg [M], kd_sample [B] and the scalar kd [1] (fp32): KL(q || p) of the student's logits (row lse of loss_fwd)
    against q = softmax(lu + scale (lc - lu)) of the teacher's cond / uncond logits and their row lse; uncond = lse_u = None:
    q = softmax(lc).  Student and teacher are each fp32 or bf16."""
    _teacher(cond, uncond, lse_u)
    _check(lib().mmtg_distill_fwd(dt(logits), _p(logits), int(ldl), dt(cond), _p(cond), _p(uncond), int(ldt), int(V), _p(lse), _p(lse_c),
                                  _p(lse_u), float(scale), int(B), int(P), int(L), float(batch_den), _p(kd_row), _p(kd_lg),
                                  _p(kd_sample), _p(kd), _stream()), "distill_fwd")


def loss_bwd_kd(logits, ldl, V, topic_ids, targets, lse, coef, gscale, cond, uncond, ldt, lse_c, lse_u, scale, kd_lg, kd_coef,
                B, P, L, dlogits, ldd, Vpad, lm_coef=0.0):
    """loss_bwd with the term's gradient: kd_lg from distill_fwd, kd_coef = distill_weight * gscale / (ntok * batch_den)."""
    _teacher(cond, uncond, lse_u)
    _check(lib().mmtg_loss_bwd_kd(dt(dlogits), dt(logits), _p(logits), int(ldl), int(V), _p(topic_ids), _p(targets), _p(lse), _p(coef),
                                  float(gscale), float(lm_coef), dt(cond), _p(cond), _p(uncond), int(ldt), _p(lse_c), _p(lse_u),
                                  float(scale), _p(kd_lg), float(kd_coef), int(B), int(P), int(L), _p(dlogits), int(ldd), int(Vpad),
                                  _stream()), "loss_bwd_kd")


def loss_bwd_kd_x3(logits, ldl, V, topic_ids, targets, lse, coef, gscale, cond, uncond, ldt, lse_c, lse_u, scale, kd_lg, kd_coef,
                   B, P, L, planes, Vpad, lm_coef=0.0):
    """... into a Planes pair (x3 mode)."""
    _teacher(cond, uncond, lse_u)
    _check(lib().mmtg_loss_bwd_kd_x3(_p(logits), int(ldl), int(V), _p(topic_ids), _p(targets), _p(lse), _p(coef), float(gscale),
                                     float(lm_coef), dt(cond), _p(cond), _p(uncond), int(ldt), _p(lse_c), _p(lse_u), float(scale),
                                     _p(kd_lg), float(kd_coef), int(B), int(P), int(L), _p(planes.t), planes.ld, planes.plane, int(Vpad),
                                     _stream()), "loss_bwd_kd_x3")


def decode_advance(pos):
    _check(lib().mmtg_decode_advance(_p(pos), _stream()), "decode_advance")


def decode_mlp_ws_floats(M):
    return int(lib().mmtg_decode_mlp_ws_floats(int(M)))


def decode_mlp_sync_words():
    return int(lib().mmtg_decode_mlp_sync_words())


def decode_mlp_census(device):
    """Workgroup placement of a 256-workgroup, one-per-CU launch: an [8, 8] int tensor, [v, x] = workgroups with id % 8 == v found on
    physical XCD x (include/mmtg_hip.h, mmtg_decode_mlp_census).  Synchronises."""
    out = torch.zeros(64, dtype=torch.int32, device=device)
    _check(lib().mmtg_decode_mlp_census(_p(out), _stream()), "decode_mlp_census")
    return out.view(8, 8).cpu()


def decode_mlp(X, stats_in, np_in, eps, W1f, colsum1, bias1f, W2t, bias2, G, C_, stats_out, ws, sync, M, D, plain=False, trace=None):
    """c_fc (LN-fold + GELU) -> mlp.c_proj (+ bias + residual + statistics) of a GPT-2 block in one launch (include/mmtg_hip.h, mmtg_decode_mlp)."""
    _check(lib().mmtg_decode_mlp(int(M), int(D), _p(X), X.stride(0), _p(stats_in), int(np_in), float(eps), _p(W1f), W1f.stride(0), _p(colsum1),
                                 _p(bias1f), _p(W2t), W2t.stride(0), _p(bias2), _p(G), G.stride(0), _p(C_), C_.stride(0), _p(stats_out),
                                 _p(ws), ws.numel(), _p(sync), int(bool(plain)), _p(trace), _stream()), "decode_mlp")
