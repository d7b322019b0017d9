"""ctypes binding of libheadct_hip.so (include/headct_hip.h).

The product path has NO CPU fallback: if the library is missing or a call fails, this module raises.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libheadct_hip.so")

HCT_F32, HCT_BF16, HCT_F16 = 0, 1, 2
NORM_LAYERNORM, NORM_RMSNORM = 0, 1  # hct_mae_config.norm_kind
HCT_ACT_NONE, HCT_ACT_GELU, HCT_ACT_DGELU, HCT_ACT_TANH, HCT_ACT_GELU_D, HCT_ACT_MULAUX = 0, 1, 2, 3, 4, 5
ACT_NONE, ACT_GELU, ACT_DGELU = 0, 1, 2

c_void_p, c_int, c_float, c_size_t, c_int64 = C.c_void_p, C.c_int, C.c_float, C.c_size_t, C.c_int64


class GemmArgs(C.Structure):
    _fields_ = [
        ("M", c_int), ("N", c_int), ("K", c_int),
        ("A", c_void_p), ("a_dtype", c_int), ("lda", c_int64), ("transA", c_int),
        ("B", c_void_p), ("b_dtype", c_int), ("ldb", c_int64), ("transB", c_int),
        ("C", c_void_p), ("c_dtype", c_int), ("ldc", c_int64),
        ("bias", c_void_p), ("residual", c_void_p), ("ldr", c_int64),
        ("act", c_int),
        ("aux", c_void_p), ("aux_dtype", c_int), ("ldaux", c_int64),
        ("C2", c_void_p), ("c2_dtype", c_int), ("ldc2", c_int64),
        ("alpha", c_float), ("force_generic", c_int), ("colsum_out", c_void_p), ("workspace_armed", c_int),
    ]


class GemmPlanInfo(C.Structure):
    """include/headct_hip.h hct_gemm_plan_info: what hct_gemm would launch (hct_gemm_describe)"""
    _fields_ = [("kernel", c_int), ("epilogue_mode", c_int), ("fuse_colsum", c_int), ("row_tiles_per_wave", c_int), ("tiles", c_int),
                ("grid", c_int), ("sk_tiles", c_int), ("sk_wgs", c_int), ("splits", c_int), ("r_chunk", c_int), ("colsum_bytes", c_size_t),
                ("stream_k_offset", c_size_t), ("slab_bytes", c_size_t), ("workspace_bytes", c_size_t), ("walk_width", c_int)]


class ProfShape(C.Structure):
    """include/headct_hip.h hct_prof_shape: launches of one GEMM shape recorded by the in-library HIP-event profile"""
    _fields_ = [("M", c_int), ("N", c_int), ("K", c_int), ("mode", c_int), ("tiles", c_int), ("sk_tiles", c_int),
                ("launches", c_int64), ("total_ms", C.c_double), ("work", C.c_double), ("bytes", C.c_double)]


def prof_shapes(lib, kernel_class: int, cap: int = 256):
    """List of ProfShape entries of the recorded launches of a kernel class (0 = NT GEMM, 1 = wgrad GEMM)."""
    buf = (ProfShape * cap)()
    n = lib.hct_prof_shapes(kernel_class, C.cast(buf, c_void_p), cap)
    if n < 0:
        raise HctError("hct_prof_shapes failed")
    return [buf[i] for i in range(min(n, cap))]


class MaeConfig(C.Structure):
    _fields_ = [
        ("input_size", c_int), ("patch_size", c_int), ("in_chans", c_int), ("mask_ratio", C.c_double),
        ("pos_embed", c_int),
        ("encoder_depth", c_int), ("encoder_embed_dim", c_int), ("encoder_mlp_dim", c_int), ("encoder_num_heads", c_int),
        ("decoder_depth", c_int), ("decoder_embed_dim", c_int), ("decoder_mlp_dim", c_int), ("decoder_num_heads", c_int),
        ("norm_pix_loss", c_int), ("use_bias", c_int),
        ("encoder_only", c_int), ("num_register_tokens", c_int), ("final_norm_eps", c_float),
        ("lora_rank", c_int),
        ("norm_kind", c_int),
        ("dropout_rate", c_float),
        ("drop_path_rate", c_float),
        ("mask_token", c_int),
        ("patch_dropout", C.c_double),
    ]


class ParamInfo(C.Structure):
    _fields_ = [
        ("name", C.c_char * 96), ("ndim", c_int), ("shape", c_int64 * 5), ("offset", c_int64), ("numel", c_int64),
        ("requires_grad", c_int), ("is_matrix", c_int), ("bf16_t_offset", c_int64),
    ]


_PROTOS = {
    # name: (restype, argtypes)
    "hct_last_error_string": (C.c_char_p, []),
    "hct_version": (c_int, []),
    "hct_has_mfma_kernels": (c_int, []),
    "hct_gemm_workspace_bytes": (c_size_t, [C.POINTER(GemmArgs)]),
    "hct_gemm_nt_flags_offset": (c_size_t, [c_size_t]),
    "hct_gemm_describe": (c_int, [C.POINTER(GemmArgs), c_int, c_size_t, C.POINTER(GemmPlanInfo)]),
    "hct_gemm_stream_k_items": (c_int, [c_int, c_int, c_int, c_int, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "hct_gemm_nt_walk": (c_int, [c_int, c_int, c_int, c_int, C.POINTER(c_int)]),
    "hct_set_cu_reserve": (None, [c_int]),
    "hct_gemm": (c_int, [C.POINTER(GemmArgs), c_void_p, c_size_t, c_void_p]),
    "hct_mask_rank": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "hct_patch_gather": (c_int, [c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_int, c_void_p]),
    "hct_encoder_assemble_fwd": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    "hct_encoder_assemble_bwd": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "hct_assemble_bwd_workspace_bytes": (c_size_t, [c_int]),
    "hct_layernorm_fwd": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_float, c_void_p, c_int, c_void_p, c_void_p, c_void_p]),
    "hct_layernorm_bwd_workspace_bytes": (c_size_t, [c_int, c_int]),
    "hct_layernorm_bwd": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p,
                                  c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "hct_layernorm_bwd_mapped": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p,
                                         c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "hct_rmsnorm_fwd": (c_int, [c_void_p, c_void_p, c_int, c_int, c_float, c_void_p, c_int, c_void_p, c_void_p]),
    "hct_rmsnorm_bwd_workspace_bytes": (c_size_t, [c_int, c_int]),
    "hct_rmsnorm_bwd": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_int, c_void_p,
                                c_void_p, c_void_p, c_size_t, c_void_p]),
    "hct_rmsnorm_bwd_mapped": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p,
                                       c_int, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "hct_tail_rows": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "hct_gather_rows": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p]),
    "hct_attention_fwd": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "hct_attention_bwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    "hct_debug_force_simple_attention": (None, [c_int]),
    "hct_dropout_mask": (c_int, [C.c_uint64, c_int, c_int, c_int64, c_int, c_int, c_float, c_void_p, c_void_p]),
    "hct_dropout_apply": (c_int, [c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int64, c_int64, C.c_uint64,
                                  c_int, c_float, c_void_p]),
    "hct_attention_dropout_fwd": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_float, C.c_uint64, c_int, c_void_p, c_void_p, c_void_p]),
    "hct_attention_dropout_bwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_float, C.c_uint64, c_int,
                                          c_void_p, c_void_p]),
    "hct_drop_path_scales": (c_int, [C.c_uint64, C.POINTER(c_int), C.POINTER(c_float), c_int, c_int, c_void_p, c_void_p]),
    "hct_residual_drop_apply": (c_int, [c_void_p, c_int, c_void_p, c_int, c_void_p, c_int64, c_int64, c_void_p, C.c_uint64, c_int, c_float,
                                        c_void_p]),
    "hct_mae_plan_set_dropout": (c_int, [c_void_p, c_int, C.c_uint64]),
    "hct_decoder_assemble_fwd": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    "hct_decoder_assemble_bwd": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_void_p,
                                         c_void_p, c_size_t, c_void_p]),
    "hct_masked_mse": (c_int, [c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_int, c_int, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "hct_unpatchify": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    "hct_vit_assemble_fwd": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    "hct_channel_norm": (c_int, [c_void_p, c_void_p, c_void_p, c_float, c_void_p, c_int, c_int64, c_int, c_void_p]),
    "hct_query_attention": (c_int, [c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_int, c_int, c_float, c_void_p, c_void_p]),
    "hct_head_linear": (c_int, [c_void_p, c_int64, c_int, c_void_p, c_void_p, c_float, c_void_p, c_void_p, c_int, c_void_p, c_int, c_int,
                                c_int, c_void_p]),
    "hct_batchnorm_stats": (c_int, [c_void_p, c_int, c_int, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "hct_softmax_xent": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "hct_sigmoid_bce_workspace_bytes": (c_size_t, [c_int, c_int]),
    "hct_sigmoid_bce": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "hct_mix_volumes": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "hct_mix_xent": (c_int, [c_void_p, c_void_p, c_void_p, c_float, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "hct_head_linear_wgrad": (c_int, [c_void_p, c_void_p, c_void_p, c_float, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "hct_bn_rows_workspace_bytes": (c_size_t, [c_int, c_int]),
    "hct_bn_stats_rows": (c_int, [c_void_p, c_int, c_int64, c_int, c_int, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                  c_size_t, c_void_p]),
    "hct_bn_norm": (c_int, [c_void_p, c_int, c_int64, c_int64, c_int, c_void_p, c_void_p, c_float, c_void_p, c_int, c_void_p]),
    "hct_bn_bwd_input": (c_int, [c_void_p, c_int, c_int64, c_void_p, c_void_p, c_float, c_void_p, c_int64, c_void_p, c_void_p, c_int,
                                 c_int, c_int, c_int, c_void_p, c_int, c_int64, c_void_p, c_size_t, c_void_p]),
    "hct_head_linear_x": (c_int, [c_void_p, c_int, c_int64, c_int, c_void_p, c_void_p, c_float, c_void_p, c_void_p, c_void_p, c_int,
                                  c_int, c_int, c_void_p]),
    "hct_head_linear_bwd": (c_int, [c_void_p, c_int, c_int64, c_int, c_void_p, c_void_p, c_float, c_void_p, c_int, c_int, c_int,
                                    c_void_p, c_void_p, c_void_p]),
    "hct_query_attention_lse": (c_int, [c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_int, c_int, c_float, c_void_p, c_void_p,
                                        c_void_p]),
    "hct_query_attention_bwd_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int]),
    "hct_query_attention_bwd": (c_int, [c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_int, c_int, c_float, c_void_p, c_void_p,
                                        c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "hct_clip_total_norm": (c_int, [c_void_p, c_int64, c_void_p, c_int, c_float, c_void_p, c_void_p]),
    "hct_add_f32": (c_int, [c_void_p, c_void_p, c_int64, c_void_p]),
    "hct_dino_loss_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "hct_dino_loss": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_float, c_float, c_void_p, c_void_p, c_void_p, c_void_p,
                              c_void_p, c_size_t, c_void_p]),
    "hct_dino_center_update": (c_int, [c_void_p, c_void_p, c_int, C.c_double, C.c_double, c_void_p]),
    "hct_dino_sk_workspace_bytes": (c_size_t, [c_int, c_int]),
    "hct_dino_sk_col_lse": (c_int, [c_void_p, c_int, c_int, c_int, c_float, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "hct_dino_sk_row_lse": (c_int, [c_void_p, c_int, c_int, c_int, c_float, c_void_p, c_void_p, c_void_p]),
    "hct_dino_loss_sk_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "hct_dino_loss_sk": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_float, c_float, c_float, c_void_p, c_void_p,
                                 c_void_p, c_void_p, c_size_t, c_void_p]),
    "hct_ibot_loss_workspace_bytes": (c_size_t, [c_int, c_int]),
    "hct_ibot_loss": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_float, c_float, c_float, c_void_p, c_void_p, c_void_p,
                              c_void_p, c_void_p, c_size_t, c_void_p]),
    "hct_ibot_loss_sk": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_float, c_float, c_float, c_float, c_void_p,
                                 c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "hct_koleo_fwd": (c_int, [c_void_p, c_int, c_int, c_int, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "hct_koleo_bwd": (c_int, [c_void_p, c_int, c_int, c_int, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p]),
    "hct_ema_update": (c_int, [c_void_p, c_void_p, c_int64, C.c_double, c_void_p]),
    "hct_l2norm_rows_fwd": (c_int, [c_void_p, c_int, c_int, c_void_p, c_int, c_void_p, c_void_p]),
    "hct_l2norm_rows_bwd": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_int, c_int, c_void_p, c_void_p]),
    "hct_weight_norm_fwd": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_int, c_void_p, c_void_p]),
    "hct_weight_norm_bwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "hct_bn_gelu_fwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_int, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p]),
    "hct_bn_gelu_bwd_sums": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p]),
    "hct_bn_gelu_bwd_apply": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_void_p, C.c_double, c_int, c_int, c_void_p, c_int,
                                      c_void_p]),
    "hct_hu_window": (c_int, [c_void_p, c_int, c_void_p, c_int, c_int, c_int64, c_int, c_void_p, c_void_p, c_void_p]),
    "hct_augment_volume": (c_int, [c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "hct_gather_augment": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int64, c_void_p, c_void_p, c_void_p]),
    "hct_affine_augment": (c_int, [c_void_p, c_int, c_void_p, c_int64, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                                   c_void_p]),
    "hct_affine_labels": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, C.c_uint8, c_void_p]),
    "hct_gaussian_smooth3d": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "hct_crop_resize_area": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "hct_adjust_contrast_workspace_bytes": (c_size_t, [c_int, c_int64]),
    "hct_adjust_contrast": (c_int, [c_void_p, c_int, c_int64, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "hct_volume_to_ras": (c_int, [c_void_p, c_int, c_int, c_int, c_int, C.POINTER(c_int), C.POINTER(c_int), c_int, C.c_double, C.c_double,
                                  c_void_p, c_void_p]),
    "hct_bspline3_resample_workspace_bytes": (c_size_t, [c_int] * 6),
    "hct_bspline3_resample": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "hct_foreground_bbox_workspace_bytes": (c_size_t, [c_int] * 3),
    "hct_foreground_bbox": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "hct_crop_window_resize_area": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int,
                                            c_void_p]),
    "hct_pos_embed_interp3d": (c_int, [c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_void_p]),
    "hct_colsum_workspace_bytes": (c_size_t, [c_int, c_int]),
    "hct_colsum": (c_int, [c_void_p, c_int, c_int, c_int, c_int64, c_void_p, c_void_p, c_size_t, c_void_p]),
    "hct_cast": (c_int, [c_void_p, c_int, c_void_p, c_int, c_int64, c_void_p]),
    "hct_transpose_cast": (c_int, [c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_void_p]),
    "hct_grad_norms_workspace_bytes": (c_size_t, [c_int64]),
    "hct_grad_norms": (c_int, [c_void_p, c_void_p, c_int, c_int64, c_float, c_int, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "hct_adamw_step": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int64, c_float, c_float,
                               c_float, c_float, c_float, c_int, c_void_p, c_void_p]),
    "hct_lion_step": (c_int, [c_void_p] * 6 + [c_int, c_int64] + [C.c_double] * 4 + [c_void_p, c_void_p]),
    "hct_sgd_step": (c_int, [c_void_p] * 6 + [c_int, c_int64] + [C.c_double] * 2 + [c_void_p, c_void_p]),
    "hct_lamb_workspace_bytes": (c_size_t, [c_int64, c_int]),
    "hct_lamb_step": (c_int, [c_void_p] * 7 + [c_int, c_int64] + [C.c_double] * 5 + [c_void_p] * 4 + [c_size_t, c_void_p, c_void_p]),
    "hct_adamw_step_scaled": (c_int, [c_void_p] * 7 + [c_int, c_int64] + [c_float] * 5 + [c_int] + [c_void_p] * 4),
    "hct_adamw_step_counts": (c_int, [c_void_p] * 7 + [c_int, c_int64] + [c_float] * 5 + [c_void_p] * 5),
    "hct_lion_step_scaled": (c_int, [c_void_p] * 6 + [c_int, c_int64] + [C.c_double] * 4 + [c_void_p] * 4),
    "hct_sgd_step_scaled": (c_int, [c_void_p] * 6 + [c_int, c_int64] + [C.c_double] * 2 + [c_void_p] * 3),
    "hct_lamb_step_scaled": (c_int, [c_void_p] * 7 + [c_int, c_int64] + [C.c_double] * 5 + [c_void_p] * 4 + [c_size_t] + [c_void_p] * 4),
    "hct_debug_set_gemm_variant": (None, [c_int]),
    "hct_gemm_nt_stream_k_bytes": (c_size_t, []),
    "hct_gemm_tn_group_workspace_bytes": (c_size_t, [c_int]),
    "hct_gemm_tn_group_prepare": (c_int, [c_void_p, c_int, c_void_p, c_size_t, c_void_p]),
    "hct_gemm_tn_group_run": (c_int, [c_void_p, c_int, c_void_p, c_size_t, c_void_p]),
    "hct_prof_enable": (None, [c_int]),
    "hct_prof_reset": (None, []),
    "hct_prof_read": (c_int, [c_int, C.POINTER(C.c_double), C.POINTER(c_int64), C.POINTER(C.c_double)]),
    "hct_prof_read_bytes": (c_int, [c_int, C.POINTER(C.c_double)]),
    "hct_prof_shapes": (c_int, [c_int, c_void_p, c_int]),
    "hct_mae_plan_create": (c_void_p, [C.POINTER(MaeConfig), c_int, c_int]),
    "hct_mae_plan_destroy": (None, [c_void_p]),
    "hct_mae_plan_num_params": (c_int, [c_void_p]),
    "hct_mae_plan_param_info": (c_int, [c_void_p, c_int, C.POINTER(ParamInfo)]),
    "hct_mae_plan_param_elems": (c_int64, [c_void_p]),
    "hct_mae_plan_bf16_t_elems": (c_int64, [c_void_p]),
    "hct_mae_plan_workspace_bytes": (c_size_t, [c_void_p]),
    "hct_mae_plan_len_keep": (c_int, [c_void_p]),
    "hct_mae_plan_set_tail": (c_int, [c_void_p, c_int]),
    "hct_mae_plan_set_dec0": (c_int, [c_void_p, c_int]),
    "hct_mae_backward_final_offset": (c_int64, [c_void_p]),
    "hct_mae_plan_set_wgrad_defer": (c_int, [c_void_p, c_int, c_int]),
    "hct_mae_plan_set_requires_grad": (c_int, [c_void_p, c_int, c_int]),
    "hct_lora_qv_fwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "hct_lora_qv_bwd_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int]),
    "hct_lora_qv_bwd": (c_int, [c_void_p] * 11 + [c_int] * 6 + [c_void_p] * 6 + [c_size_t, c_void_p]),
    "hct_topk_dot_chunks": (c_int, [c_int, c_int64]),
    "hct_topk_dot_workspace": (c_size_t, [c_int, c_int64, c_int]),
    "hct_topk_dot": (c_int, [c_void_p, c_int, c_void_p, c_int64, c_int, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "hct_attention_row_probs": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_void_p]),
    "hct_mae_recon_accum": (c_int, [c_void_p, c_int, c_int, c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p,
                                    c_void_p]),
    "hct_mae_recon_finish": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "hct_seg_loss_workspace_bytes": (c_size_t, [c_int] * 4),
    "hct_seg_loss": (c_int, [c_void_p, c_int, c_int64, c_void_p, c_void_p] + [c_int] * 6 + [c_float, c_float] + [c_void_p] * 6 + [c_int64, c_int,
                             c_void_p, c_size_t, c_void_p]),
    "hct_seg_predict_workspace_bytes": (c_size_t, [c_int] * 4),
    "hct_seg_predict": (c_int, [c_void_p, c_int, c_int64, c_void_p] + [c_int] * 7 + [c_void_p] * 4 + [c_size_t, c_void_p]),
    "hct_label_to_item": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]),
    "hct_gather_flip_labels": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int64, c_void_p, c_void_p]),
    "hct_seg_to_native_workspace_bytes": (c_size_t, [c_int] * 4),
    "hct_seg_to_native": (c_int, [c_void_p, c_int, c_int64] + [c_int] * 5 + [c_void_p] * 4 + [c_int] * 6 + [c_void_p] * 5 + [c_size_t, c_void_p]),
    "hct_surface_edges_workspace_bytes": (c_size_t, [c_int] * 3),
    "hct_surface_edges": (c_int, [c_void_p, c_void_p] + [c_int] * 4 + [c_void_p] * 3 + [c_size_t, c_void_p]),
    "hct_edt3d": (c_int, [c_void_p] + [c_int] * 10 + [C.c_double] * 3 + [c_void_p, c_void_p]),
    "hct_surface_stats_workspace_bytes": (c_size_t, [c_int] * 3),
    "hct_surface_stats": (c_int, [c_void_p] * 3 + [c_int] * 9 + [C.c_double] + [c_void_p] * 3 + [c_size_t, c_void_p]),
    "hct_surface_select_workspace_bytes": (c_size_t, []),
    "hct_surface_select": (c_int, [c_void_p] * 3 + [c_int] * 9 + [c_int64] * 4 + [c_void_p] * 2 + [c_size_t, c_void_p]),
    "hct_cc_masks": (c_int, [c_void_p, c_void_p] + [c_int] * 4 + [c_void_p, c_void_p]),
    "hct_cc_label_workspace_bytes": (c_size_t, [c_int] * 3),
    "hct_cc_label": (c_int, [c_void_p] + [c_int] * 5 + [c_void_p, c_void_p, c_size_t, c_void_p]),
    "hct_cc_compact_workspace_bytes": (c_size_t, [c_int] * 3),
    "hct_cc_compact": (c_int, [c_void_p] + [c_int] * 3 + [c_void_p, c_void_p, c_size_t, c_void_p]),
    "hct_cc_sizes": (c_int, [c_void_p, c_int64, c_int64, c_void_p, c_void_p]),
    "hct_cc_overlap": (c_int, [c_void_p, c_int64, c_void_p, c_int, c_int64, c_void_p, c_void_p]),
    "hct_cc_remove_small": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_void_p]),
    "hct_cc_count_small": (c_int, [c_void_p, c_int64, c_int64, c_void_p, c_void_p]),
    "hct_seg_recount_workspace_bytes": (c_size_t, [c_int] * 4),
    "hct_seg_recount": (c_int, [c_void_p, c_void_p] + [c_int] * 4 + [c_void_p] * 3 + [c_size_t, c_void_p]),
    "hct_cc_tile_dims": (None, [C.POINTER(c_int)] * 3),
    "hct_mae_plan_bind": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t]),
    "hct_mae_refresh_weights": (c_int, [c_void_p, c_int, c_void_p]),
    "hct_mae_forward": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_float, c_void_p]),
    "hct_mae_set_loss_grad": (c_int, [c_void_p, c_void_p]),
    "hct_mae_num_backward_stages": (c_int, [c_void_p]),
    "hct_mae_backward_stage_range": (c_int, [c_void_p, c_int, C.POINTER(c_int64), C.POINTER(c_int64)]),
    "hct_mae_backward_stage": (c_int, [c_void_p, c_int, c_void_p]),
    "hct_vit_forward": (c_int, [c_void_p, c_void_p, c_int, c_void_p]),
    "hct_vit_forward_parts": (c_int, [c_void_p, C.POINTER(c_void_p), c_int, c_int, c_void_p]),
    "hct_vit_backward_stage": (c_int, [c_void_p, c_int, c_void_p, c_void_p]),
    "hct_vit_assemble_bwd": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "hct_vit_assemble_keep_fwd": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    "hct_vit_assemble_keep_bwd": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p,
                                          c_void_p]),
    "hct_vit_forward_parts_keep": (c_int, [c_void_p, C.POINTER(c_void_p), c_int, c_int, c_void_p, c_void_p]),
    "hct_vit_assemble_masked_fwd": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p,
                                            c_void_p]),
    "hct_vit_assemble_masked_bwd_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "hct_vit_assemble_masked_bwd": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                                            c_void_p, c_size_t, c_void_p]),
    "hct_vit_forward_parts_masked": (c_int, [c_void_p, C.POINTER(c_void_p), c_int, c_int, c_void_p, c_void_p]),
    "hct_mae_plan_activation": (c_void_p, [c_void_p, C.c_char_p, C.POINTER(c_int64), C.POINTER(c_int64), C.POINTER(c_int)]),
}

_lib: Optional[C.CDLL] = None


class HctError(RuntimeError):
    pass


def exported_symbols():
    """Names every build of the library must export (checked by the CPU test-suite)."""
    return sorted(_PROTOS)


def load() -> C.CDLL:
    """Load libheadct_hip.so; raise loudly if it is absent (no CPU fallback exists)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise HctError(
            f"{LIB_PATH} not found: build it with `python -m headct_foundation_amd.build` "
            "(hipcc --offload-arch=gfx950).  There is no CPU fallback for the MAE hot path.")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in _PROTOS.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is missing
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc: int, what: str = "") -> None:
    if rc != 0:
        msg = load().hct_last_error_string()
        raise HctError(f"{what} failed (rc={rc}): {msg.decode() if msg else ''}")


def ptr(t) -> Optional[int]:
    """Device pointer of a torch tensor (None -> NULL)."""
    if t is None:
        return None
    return t.data_ptr()


def stream_ptr(device=None) -> int:
    """HIP stream handle of the current stream (of `device` when given, else of the current device)."""
    import torch
    return torch.cuda.current_stream(device).cuda_stream


def dtype_code(t) -> int:
    """HCT_* element-type code of a tensor or a torch dtype: bf16, fp16, anything else fp32."""
    import torch
    dt = getattr(t, "dtype", t)
    return HCT_BF16 if dt == torch.bfloat16 else HCT_F16 if dt == torch.float16 else HCT_F32


def gemm(a, b, out, trans_a: bool = False, trans_b: bool = True, bias=None, residual=None, act: int = HCT_ACT_NONE, aux=None,
         alpha: float = 1.0, workspace: bool = False, stream: Optional[int] = None):
    """out[M, N] = act(alpha * op(a) . op(b) + bias) (+ residual) over hct_gemm, op = transpose where `trans_*` says so.  a / b are
    read with their row stride; out, residual and aux are [M, N] row-major.  `workspace=True` hands hct_gemm the workspace it asks
    for (hct_gemm_workspace_bytes), which lets it take the stream-K path; without one it never does.  Returns `out`."""
    import torch
    lib = load()
    M, N = out.shape
    g = GemmArgs()
    g.M, g.N, g.K = M, N, a.shape[0] if trans_a else a.shape[1]
    g.A, g.a_dtype, g.lda, g.transA = a.data_ptr(), dtype_code(a), a.stride(0), int(trans_a)
    g.B, g.b_dtype, g.ldb, g.transB = b.data_ptr(), dtype_code(b), b.stride(0), int(trans_b)
    g.C, g.c_dtype, g.ldc = out.data_ptr(), dtype_code(out), N
    if bias is not None:
        g.bias = bias.data_ptr()
    if residual is not None:
        g.residual, g.ldr = residual.data_ptr(), N
    g.act = act
    if aux is not None:
        g.aux, g.aux_dtype, g.ldaux = aux.data_ptr(), dtype_code(aux), N
    g.alpha = alpha
    ws = None
    if workspace:
        need = lib.hct_gemm_workspace_bytes(C.byref(g))
        ws = torch.empty(max(16, need), dtype=torch.uint8, device=out.device) if need else None
    check(lib.hct_gemm(C.byref(g), ptr(ws), ws.numel() if ws is not None else 0, stream_ptr() if stream is None else stream), "hct_gemm")
    return out


def cast_weight(w, dtype, stream: Optional[int] = None):
    """fp32 weight `w` in the compute dtype: `w` itself for fp32, else a fresh copy over hct_cast."""
    import torch
    if dtype == torch.float32:
        return w
    out = torch.empty(w.shape, dtype=dtype, device=w.device)
    check(load().hct_cast(w.data_ptr(), HCT_F32, out.data_ptr(), dtype_code(dtype), w.numel(), stream_ptr() if stream is None else stream),
          "hct_cast")
    return out
