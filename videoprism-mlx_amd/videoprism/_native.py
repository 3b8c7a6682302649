"""ctypes binding of libvideoprism_hip.so (C-ABI declared in include/videoprism_hip.h).

There is no fallback: if the library is missing or cannot be loaded, every entry point
raises NativeLibraryError.  Device memory is passed as raw pointers of PyTorch-ROCm
tensors; streams as hipStream_t handles of torch streams.
"""

from __future__ import annotations

import ctypes
import os
from ctypes import POINTER, c_char_p, c_float, c_int, c_int32, c_int64, c_size_t, c_void_p

_LIB_NAME = "libvideoprism_hip.so"
_LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), _LIB_NAME)
# tools' A/B library (`make -C videoprism-mlx_amd diag`): the product library plus ablation builds;
# loaded only when VP_DIAG_LIB=1 (tools/), never by the package's tests or the bench
_DIAG_LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libvideoprism_hip_diag.so")

VP_OK, VP_EINVAL, VP_ENOMEM, VP_EHIP, VP_ESTATE, VP_ENOTSUP, VP_ECOMM = range(7)
VP_F32, VP_BF16, VP_U8 = 0, 1, 2

EPI_STORE, EPI_GELU, EPI_RESID, EPI_POS, EPI_RESID_FFN = 0, 1, 2, 3, 4
# bf16 residual stream variants (bf16 resid / out; bf16 precision only)
EPI_RESID_BF16, EPI_POS_BF16, EPI_RESID_FFN_BF16 = 5, 6, 7
PERM_NONE, PERM_BTN_TO_BNT, PERM_BNT_TO_BTN = 0, 1, 2
VP_RESIZE_CENTER_CROP, VP_RESIZE_STRETCH = 0, 1
VP_YUV_NV12, VP_YUV_I420, VP_YUV_P010 = 0, 1, 2
VP_YUV_BT601, VP_YUV_BT709 = 0, 1
VP_YUV_LIMITED, VP_YUV_FULL = 0, 1


class NativeLibraryError(RuntimeError):
    """libvideoprism_hip.so is missing or failed to load (no CPU fallback exists)."""


class VPError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"[vp status {code}] {msg}")
        self.code = code


class vp_config(ctypes.Structure):
    _fields_ = [
        ("patch_size", c_int32),
        ("pos_emb_t", c_int32),
        ("pos_emb_h", c_int32),
        ("pos_emb_w", c_int32),
        ("model_dim", c_int32),
        ("num_spatial_layers", c_int32),
        ("num_temporal_layers", c_int32),
        ("num_heads", c_int32),
        ("mlp_dim", c_int32),
        ("atten_logit_cap", c_float),
        ("fprop_dtype", c_int32),
    ]


class vp_clip_config(ctypes.Structure):
    _fields_ = [
        ("video", vp_config),
        ("num_auxiliary_layers", c_int32),
        ("vocabulary_size", c_int32),
        ("num_unimodal_layers", c_int32),
        ("enable_causal_atten", c_int32),
        ("norm_policy", c_int32),  # text tower: 0 'pre' (the default), 1 'primer_hybrid'
    ]


NORM_POLICIES = {"pre": 0, "primer_hybrid": 1}


class vp_probe_dims(ctypes.Structure):
    _fields_ = [("model_dim", c_int32), ("num_heads", c_int32), ("num_classes", c_int32)]


# members of vp_probe_params / vp_probe_grads, in order, and the leaf each one is (path under 'params')
PROBE_LEAVES = (
    ("query", "atten_pooler/pooling_attention_query"),
    ("per_dim_scale", "atten_pooler/pooling_attention/per_dim_scale/per_dim_scale"),
    ("query_w", "atten_pooler/pooling_attention/query/w"),
    ("query_b", "atten_pooler/pooling_attention/query/b"),
    ("key_w", "atten_pooler/pooling_attention/key/w"),
    ("key_b", "atten_pooler/pooling_attention/key/b"),
    ("value_w", "atten_pooler/pooling_attention/value/w"),
    ("value_b", "atten_pooler/pooling_attention/value/b"),
    ("post_w", "atten_pooler/pooling_attention/post/w"),
    ("post_b", "atten_pooler/pooling_attention/post/b"),
    ("ln_scale", "atten_pooler/pooling_attention_layer_norm/scale"),
    ("ln_bias", "atten_pooler/pooling_attention_layer_norm/bias"),
    ("proj_kernel", "projection/linear/kernel"),
    ("proj_bias", "projection/linear/bias"),
)


class vp_probe_params(ctypes.Structure):  # device fp32 pointers; vp_probe_grads has the same members
    _fields_ = [(member, c_void_p) for member, _ in PROBE_LEAVES]


class vp_yuv_frames(ctypes.Structure):  # device planes Y, UV, - (NV12, P010) or Y, U, V (I420); strides in bytes
    _fields_ = [("plane", c_void_p * 3), ("row_stride", c_int64 * 3), ("frame_stride", c_int64 * 3),
                ("format", c_int), ("matrix", c_int), ("range", c_int)]


# name -> (restype, argtypes)
_SIGNATURES = {
    "vp_last_error": (c_char_p, []),
    "vp_abi_version": (c_int, []),
    "vp_create": (c_int, [POINTER(vp_config), c_int, POINTER(c_void_p)]),
    "vp_destroy": (c_int, [c_void_p]),
    "vp_set_param": (c_int, [c_void_p, c_char_p, c_void_p, POINTER(c_int64), c_int]),
    "vp_param_count": (c_int, [c_void_p, POINTER(c_int)]),
    "vp_param_name": (c_int, [c_void_p, c_int, POINTER(c_char_p)]),
    "vp_finalize": (c_int, [c_void_p]),
    "vp_prepare_geometry": (c_int, [c_void_p, c_int64, c_int64]),
    "vp_prepare_frames": (c_int, [c_void_p, c_int64]),
    "vp_workspace_bytes": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_int64, POINTER(c_size_t)]),
    "vp_forward": (c_int, [c_void_p, c_void_p, c_int, c_int64, c_int64, c_int64, c_int64, c_void_p,
                           c_void_p, c_int, c_void_p, c_void_p, c_size_t, c_void_p]),
    # sliding windows: per-frame spatial states once, then the temporal half over windows of them
    "vp_spatial_workspace_bytes": (c_int, [c_void_p, c_int64, c_int64, c_int64, POINTER(c_size_t)]),
    "vp_forward_spatial": (c_int, [c_void_p, c_void_p, c_int, c_int64, c_int64, c_int64, c_void_p, c_void_p,
                                   c_void_p, c_size_t, c_void_p]),
    "vp_temporal_workspace_bytes": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_int64, POINTER(c_size_t)]),
    "vp_forward_temporal": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_int64, c_int64, c_int64,
                                    c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_size_t, c_void_p]),
    "vp_clip_video_windows_workspace_bytes": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_int64,
                                                      POINTER(c_size_t)]),
    "vp_clip_encode_video_windows": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_int64, c_int64,
                                             c_int64, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                                             c_int, c_void_p, c_size_t, c_void_p]),
    "vp_classifier_windows_workspace_bytes": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_int64,
                                                      POINTER(c_size_t)]),
    "vp_classifier_forward_windows": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_int64, c_int64,
                                              c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int,
                                              c_void_p, c_size_t, c_void_p]),
    # not in the public header: the frame gather of vp_forward_temporal on its own
    "vp_dev_gather_frames": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_int64, c_void_p, c_void_p]),
    # ... followed by the LayerNorm, as vp_forward_temporal launches the two
    "vp_dev_layernorm_gather": (c_int, [c_void_p, c_int, c_int64, c_void_p, c_int64, c_int64, c_void_p, c_void_p,
                                        c_void_p, c_int, c_int, c_int64, c_int64, c_void_p, c_void_p, c_void_p,
                                        c_void_p]),
    "vp_profile_enable": (c_int, [c_void_p, c_int]),
    "vp_profile_read": (c_int, [c_void_p, c_int, POINTER(ctypes.c_double), POINTER(ctypes.c_double),
                                POINTER(ctypes.c_double), POINTER(c_int64)]),
    "vp_profile_set_mask": (c_int, [c_void_p, ctypes.c_uint32]),
    "vp_profile_class_count": (c_int, []),
    "vp_profile_class_name": (c_int, [c_int, POINTER(c_char_p)]),
    "vp_profile_kernel_name": (c_int, [c_void_p, c_int, POINTER(c_char_p)]),
    # multi-GPU: RCCL all-gather of pooled clip embeddings
    "vp_comm_id_bytes": (c_int, []),
    "vp_comm_unique_id": (c_int, [c_void_p, c_int64]),
    "vp_comm_init": (c_int, [c_void_p, c_int64, c_int, c_int, c_int, POINTER(c_void_p)]),
    "vp_comm_destroy": (c_int, [c_void_p]),
    "vp_allgather": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int, c_void_p]),
    "vp_op_gemm": (c_int, [c_int, c_int, c_void_p, c_int64, c_void_p, c_int64, c_int64, c_int64,
                           c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_void_p,
                           c_int64, c_void_p, c_void_p]),
    "vp_op_attention": (c_int, [c_int, c_void_p, c_void_p, c_int64, c_int64, c_int64, c_float,
                                c_void_p, c_void_p]),
    "vp_op_attention_dh": (c_int, [c_int, c_void_p, c_void_p, c_int64, c_int64, c_int64, c_int64, c_float,
                                   c_void_p, c_void_p]),
    "vp_op_layernorm": (c_int, [c_void_p, c_int, c_int64, c_int64, c_void_p, c_void_p, c_void_p,
                                c_int, c_int, c_int64, c_int64, c_void_p, c_void_p]),
    "vp_op_patchify": (c_int, [c_void_p, c_int, c_void_p, c_int, c_int64, c_int64, c_int64, c_int64,
                               c_int64, c_int64, c_void_p]),
    "vp_op_preprocess_frames": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_int64, c_int64, c_void_p,
                                        c_int64, c_int, c_int, c_int64, c_void_p, c_void_p]),
    "vp_op_preprocess_yuv": (c_int, [POINTER(vp_yuv_frames), c_int64, c_int64, c_int64, c_void_p, c_int64, c_int,
                                     c_int64, c_void_p, c_void_p]),
    # the same two with a device table of views [V, 9] in place of the resize mode
    "vp_op_preprocess_views": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_int64, c_int64, c_void_p, c_void_p,
                                       c_int64, c_int64, c_int, c_int64, c_void_p, c_void_p]),
    "vp_op_preprocess_yuv_views": (c_int, [POINTER(vp_yuv_frames), c_int64, c_int64, c_int64, c_void_p, c_void_p,
                                           c_int64, c_int64, c_int64, c_void_p, c_void_p]),
    # the conversion's integer table (tests/yuv_restatement.py); no GPU call
    "vp_dev_yuv_coefficients": (c_int, [c_int, c_int, c_int, POINTER(c_int32)]),
    "vp_op_pool_l2": (c_int, [c_void_p, c_int, c_int64, c_int64, c_int64, c_void_p, c_void_p]),
    "vp_op_attention_masked": (c_int, [c_int, c_void_p, c_void_p, c_int64, c_int64, c_int64, c_float,
                                       c_void_p, c_int, c_void_p]),
    "vp_op_attention_masked_dh": (c_int, [c_int, c_void_p, c_void_p, c_int64, c_int64, c_int64, c_int64, c_float,
                                          c_void_p, c_int, c_void_p]),
    "vp_op_similarity": (c_int, [c_void_p, c_void_p, c_int64, c_int64, c_int64, c_void_p, c_void_p]),
    # LvT video-text model (FactorizedVideoCLIP)
    "vp_clip_create": (c_int, [POINTER(vp_clip_config), c_int, POINTER(c_void_p)]),
    "vp_clip_destroy": (c_int, [c_void_p]),
    "vp_clip_set_param": (c_int, [c_void_p, c_char_p, c_void_p, POINTER(c_int64), c_int]),
    "vp_clip_param_count": (c_int, [c_void_p, POINTER(c_int)]),
    "vp_clip_param_name": (c_int, [c_void_p, c_int, POINTER(c_char_p)]),
    "vp_clip_finalize": (c_int, [c_void_p]),
    "vp_clip_video_handle": (c_int, [c_void_p, POINTER(c_void_p)]),
    "vp_clip_video_workspace_bytes": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_int64,
                                              POINTER(c_size_t)]),
    "vp_clip_encode_video": (c_int, [c_void_p, c_void_p, c_int, c_int64, c_int64, c_int64, c_int64,
                                     c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int,
                                     c_void_p, c_size_t, c_void_p]),
    # FactorizedVideoClassifier
    "vp_classifier_create": (c_int, [POINTER(vp_config), c_int, c_int, POINTER(c_void_p)]),
    "vp_classifier_destroy": (c_int, [c_void_p]),
    "vp_classifier_set_param": (c_int, [c_void_p, c_char_p, c_void_p, POINTER(c_int64), c_int]),
    "vp_classifier_param_count": (c_int, [c_void_p, POINTER(c_int)]),
    "vp_classifier_param_name": (c_int, [c_void_p, c_int, POINTER(c_char_p)]),
    "vp_classifier_finalize": (c_int, [c_void_p]),
    "vp_classifier_video_handle": (c_int, [c_void_p, POINTER(c_void_p)]),
    "vp_classifier_workspace_bytes": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_int64,
                                              POINTER(c_size_t)]),
    "vp_classifier_forward": (c_int, [c_void_p, c_void_p, c_int, c_int64, c_int64, c_int64, c_int64,
                                      c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int,
                                      c_void_p, c_size_t, c_void_p]),
    "vp_clip_text_workspace_bytes": (c_int, [c_void_p, c_int64, c_int64, POINTER(c_size_t)]),
    "vp_clip_encode_text": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int, c_void_p,
                                    c_void_p, c_size_t, c_void_p]),
    # the classifier head's training ops over frozen tokens (videoprism/probe.py)
    "vp_op_probe_workspace_bytes": (c_int, [POINTER(vp_probe_dims), c_int64, c_int64, POINTER(c_size_t)]),
    "vp_op_probe_forward": (c_int, [POINTER(vp_probe_dims), POINTER(vp_probe_params), c_void_p, c_int, c_int64,
                                    c_int64, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "vp_op_probe_backward": (c_int, [POINTER(vp_probe_dims), POINTER(vp_probe_params), c_void_p, c_int, c_int64,
                                     c_int64, c_void_p, POINTER(vp_probe_params), c_void_p, c_size_t, c_void_p]),
    # ... under token paddings [B, S] (device fp32, after S; NULL: the calls above)
    "vp_op_probe_forward_masked": (c_int, [POINTER(vp_probe_dims), POINTER(vp_probe_params), c_void_p, c_int, c_int64,
                                           c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "vp_op_probe_backward_masked": (c_int, [POINTER(vp_probe_dims), POINTER(vp_probe_params), c_void_p, c_int, c_int64,
                                            c_int64, c_void_p, c_void_p, POINTER(vp_probe_params), c_void_p, c_size_t,
                                            c_void_p]),
    # gallery search: fused scores and top-k (videoprism/retrieval.py)
    "vp_op_topk_workspace_bytes": (c_int, [c_int64, c_int64, POINTER(c_size_t)]),
    "vp_op_topk": (c_int, [c_void_p, c_int64, c_void_p, c_int, c_int64, c_int64, c_int64, c_int64, c_int64, c_void_p,
                           c_void_p, c_void_p, c_size_t, c_void_p]),
    "vp_op_topk_merge": (c_int, [c_void_p, c_void_p, c_int64, c_int64, c_int64, c_int64, c_void_p, c_void_p,
                                 c_void_p]),
    # grouped gallery search: the k best groups of rows, each with its best row (EmbeddingIndex.search_groups)
    "vp_op_topk_groups_workspace_bytes": (c_int, [c_int64, c_int64, POINTER(c_size_t)]),
    "vp_op_topk_groups": (c_int, [c_void_p, c_int64, c_void_p, c_int, c_int64, c_int64, c_int64, c_void_p, c_int64,
                                  c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "vp_op_topk_groups_merge": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int64, c_int64, c_void_p,
                                        c_void_p, c_void_p, c_void_p]),
    # masked gallery search: a packed bit per row, shared or per query (EmbeddingIndex.remove, search(allow=...))
    "vp_op_rowmask_pack": (c_int, [c_void_p, c_int64, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_void_p]),
    "vp_op_topk_masked": (c_int, [c_void_p, c_int64, c_void_p, c_int, c_int64, c_int64, c_int64, c_int64, c_int64,
                                  c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "vp_op_topk_groups_masked": (c_int, [c_void_p, c_int64, c_void_p, c_int, c_int64, c_int64, c_int64, c_void_p,
                                         c_int64, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p,
                                         c_size_t, c_void_p]),
    # fp8 gallery: e4m3 codes and a power-of-two scale per row (EmbeddingIndex(dtype=torch.float8_e4m3fn))
    "vp_op_quantize_rows_f8": (c_int, [c_void_p, c_int, c_int64, c_int64, c_int64, c_void_p, c_int64, c_void_p,
                                       c_void_p]),
    "vp_op_topk_f8": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_int64, c_int64, c_int64, c_int64,
                              c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "vp_op_topk_groups_f8": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_int64, c_int64, c_void_p,
                                     c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "vp_op_topk_masked_f8": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_int64, c_int64, c_int64,
                                     c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "vp_op_topk_groups_masked_f8": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_int64, c_int64,
                                            c_void_p, c_int64, c_int64, c_void_p, c_int64, c_void_p, c_void_p,
                                            c_void_p, c_void_p, c_size_t, c_void_p]),
    # not in the public header: queries per workgroup of the search at (D, k) (tools/retrieval_bench.py); no GPU call
    "vp_dev_topk_group": (c_int, [c_int64, c_int64]),
    "vp_dev_topk_groups_group": (c_int, [c_int64, c_int64]),
    # not in the public header: one streaming pass of the backward on its own (tools/probe_bench.py)
    "vp_dev_probe_backward_pass": (c_int, [POINTER(vp_probe_dims), c_void_p, c_int, c_int64, c_int64, c_int, c_void_p,
                                           c_size_t, c_void_p]),
    # not in the public header: named-kernel GEMM for A/B tests and tools/gemm_bench.py
    "vp_dev_gemm_kernel": (c_int, [c_int, c_int, c_void_p, c_void_p, c_int64, c_int64, c_int64,
                                   c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p,
                                   c_void_p]),
    "vp_dev_gemm_ln": (c_int, [c_int, c_void_p, c_void_p, c_int64, c_int64, c_int64, c_void_p,
                               c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p,
                               c_void_p, c_void_p, c_void_p]),
    "vp_dev_ln_stats": (c_int, [c_int, c_void_p, c_int64, c_int64, c_void_p, c_void_p]),
    "vp_dev_patch_embed": (c_int, [c_void_p, c_int64, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_void_p,
                                   c_void_p]),
    "vp_dev_attention_spatial_blk": (c_int, [c_void_p, c_void_p, c_int64, c_int64, c_float, c_void_p, c_void_p]),
    "vp_dev_gemm_tattn": (c_int, [c_int, c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_void_p,
                                  c_void_p, c_void_p, c_int64, c_float, c_void_p]),
    # which attention kernel the library picks (vpi::choose_attention); no GPU call
    "vp_dev_attention_choice": (c_int, [c_int, c_int, c_int64, c_float, c_int]),
    "vp_dev_attention_choice_dh": (c_int, [c_int, c_int, c_int64, c_float, c_int, c_int64]),
    # the pooler, small GEMM and text kernels one at a time (tests/test_gpu_clip_kernels.py)
    "vp_dev_pool_split_u": (c_int, [c_void_p, c_int64, c_int64, c_void_p]),
    "vp_dev_pool_chunks": (c_int, [c_int64]),
    "vp_dev_pool_logits": (c_int, [c_void_p, c_int, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_int64,
                                   c_void_p, c_void_p]),
    "vp_dev_pool_softmax_wsum": (c_int, [c_void_p, c_int, c_int64, c_int64, c_int64, c_int64, c_void_p, c_void_p,
                                         c_void_p, c_void_p, c_void_p]),
    "vp_dev_small_gemm": (c_int, [c_void_p, c_int64, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_void_p,
                                  c_int64, c_int64, c_int64, c_int64, c_int64, c_int64, c_int64, c_void_p,
                                  c_void_p]),
    "vp_dev_ln_l2_rows": (c_int, [c_void_p, c_int, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_int,
                                  c_void_p, c_void_p]),
    "vp_dev_text_embed": (c_int, [c_void_p, c_int64, c_int64, c_void_p, c_int, c_int64, c_void_p, c_void_p,
                                  c_float, c_int64, c_void_p, c_int, c_void_p, c_void_p, c_void_p]),
    # the same three over D up to 1536 (Giant's 1408), and the primer_hybrid LayerNorm-then-residual kernel
    "vp_dev_pool_logits_wide": (c_int, [c_void_p, c_int, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_int64,
                                        c_void_p, c_void_p]),
    "vp_dev_pool_softmax_wsum_wide": (c_int, [c_void_p, c_int, c_int64, c_int64, c_int64, c_int64, c_void_p,
                                              c_void_p, c_void_p, c_void_p, c_void_p]),
    "vp_dev_ln_l2_rows_wide": (c_int, [c_void_p, c_int, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_int,
                                       c_void_p, c_void_p]),
    "vp_dev_layernorm_residual": (c_int, [c_void_p, c_int, c_int64, c_int64, c_void_p, c_void_p, c_void_p,
                                          c_void_p, c_void_p]),
    "vp_dev_pooler": (c_int, [c_int, c_void_p, c_void_p, c_int64, c_int64, c_int, c_void_p, c_void_p,
                              POINTER(c_size_t), c_void_p]),
}
# diag library only (ablation builds for tools/)
_DIAG_SIGNATURES = {
    "vp_dev_gemm_f32_var": (c_int, [c_int, c_int, c_int, c_void_p, c_void_p, c_int64, c_int64, c_int64, c_void_p,
                                    c_void_p, c_void_p]),
    "vp_dev_attention_long_var": (c_int, [c_int, c_void_p, c_void_p, c_int64, c_int64, c_int64, c_float, c_void_p]),
    "vp_dev_gemm_tattn_abl": (c_int, [c_int, c_int, c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_void_p,
                                      c_void_p, c_void_p, c_void_p, c_int64, c_float, c_void_p]),
    "vp_dev_gemm_w4_abl": (c_int, [c_int, c_int, c_void_p, c_void_p, c_int64, c_int64, c_int64, c_void_p,
                                   c_void_p, c_void_p]),
    "vp_dev_gemm_ffn1_abl": (c_int, [c_int, c_void_p, c_void_p, c_int64, c_int64, c_int64, c_void_p, c_void_p,
                                     c_void_p, c_void_p, c_void_p]),
    "vp_dev_gemm_ffn2_abl": (c_int, [c_int, c_void_p, c_void_p, c_int64, c_int64, c_int64, c_void_p, c_void_p,
                                     c_void_p, c_void_p]),
}

_lib = None


def _diag() -> bool:
    return os.environ.get("VP_DIAG_LIB", "0") == "1"


def library_path() -> str:
    return _DIAG_LIB_PATH if _diag() else _LIB_PATH


def load() -> ctypes.CDLL:
    """Loads (once) and returns the library; raises NativeLibraryError if unavailable."""
    global _lib
    if _lib is not None:
        return _lib
    path = library_path()
    if not os.path.exists(path):
        raise NativeLibraryError(
            f"{path} not found: build it with `make -C videoprism-mlx_amd` "
            "(or __graft_entry__.build()); there is no CPU fallback.")
    try:
        import torch  # noqa: F401  (HIP runtime / RCCL of the process: torch's, loaded first)
    except ImportError:  # pragma: no cover
        pass
    try:
        lib = ctypes.CDLL(path)
    except OSError as e:
        raise NativeLibraryError(f"failed to load {path}: {e}") from e
    sigs = dict(_SIGNATURES, **(_DIAG_SIGNATURES if _diag() else {}))
    for name, (res, args) in sigs.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def exported_symbols():
    return list(_SIGNATURES)


def check(rc: int) -> None:
    if rc != VP_OK:
        msg = load().vp_last_error().decode("utf-8", "replace")
        if rc in (VP_EINVAL,):
            raise ValueError(msg)
        if rc == VP_ENOTSUP:
            raise NotImplementedError(msg)
        raise VPError(rc, msg)


def call(name: str, *args) -> None:
    fn = getattr(load(), name)
    # an undeclared signature would pass Python ints as 32-bit c_int: a device pointer truncated that way
    # is an illegal address on the GPU, so every entry point called here must be declared
    if getattr(fn, "argtypes", None) is None:
        raise TypeError(f"{name}: no ctypes signature declared in _native.py")
    check(fn(*args))


# ---------------------------------------------------------------------------------------
# torch-tensor helpers for the op-level entry points (used by kernel parity tests)
# ---------------------------------------------------------------------------------------
def _ptr(t):
    return None if t is None else c_void_p(t.data_ptr())


def _stream(stream=None):
    import torch
    s = stream if stream is not None else torch.cuda.current_stream()
    return c_void_p(s.cuda_stream)


def _prec(t):
    import torch
    if t.dtype == torch.bfloat16:
        return VP_BF16
    if t.dtype == torch.float32:
        return VP_F32
    if t.dtype == torch.uint8:
        return VP_U8
    raise TypeError(f"unsupported dtype {t.dtype}")


def op_gemm(a, w, bias, epilogue=EPI_STORE, out=None, resid=None, pos=None, rowpad=None,
            stream=None):
    """out = epilogue(a @ w.T + bias); a [M,K], w [N,K] (bf16 or fp32), bias fp32 [N]."""
    import torch
    M, K = a.shape
    N = w.shape[0]
    if out is None:
        odt = (a.dtype if epilogue in (EPI_STORE, EPI_GELU) else
               torch.bfloat16 if epilogue >= EPI_RESID_BF16 else torch.float32)
        out = torch.empty((M, N), dtype=odt, device=a.device)
    call("vp_op_gemm", _prec(a), epilogue, _ptr(a), a.stride(0), _ptr(w), w.stride(0), M, N, K,
         _ptr(out), out.stride(0), _ptr(bias), _ptr(resid),
         resid.stride(0) if resid is not None else 0, _ptr(pos),
         pos.shape[0] if pos is not None else 0, _ptr(rowpad), _stream(stream))
    return out


def dev_gemm_kernel(which, a, w, bias, epilogue, out, resid=None, pos=None, rowpad=None,
                    stream=None):
    """bf16 GEMM through one named kernel (4 = 4-wave, 8 = 8-wave); out/resid contiguous."""
    M, K = a.shape
    N = w.shape[0]
    call("vp_dev_gemm_kernel", which, epilogue, _ptr(a), _ptr(w), M, N, K, _ptr(out), _ptr(bias),
         _ptr(resid), _ptr(pos), pos.shape[0] if pos is not None else 0, _ptr(rowpad),
         _stream(stream))
    return out


EPI_BF16_LN, EPI_GELU_LN, EPI_RESID_BF16_ST, EPI_RESID_FFN_BF16_ST, EPI_POS_BF16_ST = 8, 9, 10, 11, 12
# the FFN pair over the row-blocked hidden activation [M/16][F/32][16][32] (vp_kernels.h EPI_*_BLK)
EPI_GELU_LN_BLK, EPI_RESID_FFN_BF16_ST_BLK, EPI_RESID_FFN_BF16_BLK, EPI_BF16_LN_BLK = 16, 17, 18, 19


def ffn1_blk_rows(F):
    """Row order of W1 / b' / c for EPI_GELU_LN_BLK (vp_internal.h pack_stack): packed row r holds
    natural row src[r] -- within each 32-row group, row 16 h + 4 g + i holds column 8 g + 4 h + i."""
    import numpy as np
    r = np.arange(F)
    w = r & 31
    return (r & ~31) + 8 * ((w >> 2) & 3) + 4 * (w >> 4) + (w & 3)


def to_row_blocked(h):
    """[M, F] row-major -> the [M/16][F/32][16][32] blocked layout, flattened back to [M, F] storage."""
    M, F = h.shape
    return h.reshape(M // 16, 16, F // 32, 32).permute(0, 2, 1, 3).reshape(M, F)


def dev_gemm_ln(a, w, bias, epilogue, out, resid=None, pos=None, rowpad=None, ln_rs=None,
                ln_c=None, st_part=None, stream=None):
    """bf16 w4 GEMM with a GEMM-folded LayerNorm epilogue (8, 9) or a row-statistics
    epilogue (10..12); all tensors contiguous on the device."""
    M, K = a.shape
    N = w.shape[0]
    call("vp_dev_gemm_ln", epilogue, _ptr(a), _ptr(w), M, N, K, _ptr(out), _ptr(bias), _ptr(resid),
         _ptr(pos), pos.shape[0] if pos is not None else 0, _ptr(rowpad), _ptr(ln_rs), _ptr(ln_c),
         _ptr(st_part), _stream(stream))
    return out


def dev_gemm_w4_abl(a, w, bias, out, abl, s3=False, stream=None):
    """Diag library only: an ablation build of the product 4-wave GEMM (EPI_BF16; abl 2 = no
    ds_reads, 4 = no staging loads, 8 = no epilogue) -- timing only, results garbage."""
    M, K = a.shape
    N = w.shape[0]
    call("vp_dev_gemm_w4_abl", abl, 1 if s3 else 0, _ptr(a), _ptr(w), M, N, K, _ptr(out), _ptr(bias),
         _stream(stream))
    return out


def dev_gemm_tattn(which, a, w, bias, ln_rs, ln_c, out, heads, cap, p=None, stream=None):
    """The fused temporal attention's launches: which 0 (w = [q_h | k_h] rows) -> P in `out`,
    which 1 (w = v rows, p = P) -> O [M, D] in `out`; all tensors contiguous on the device."""
    M, K = a.shape
    call("vp_dev_gemm_tattn", which, _ptr(a), _ptr(w), M, K, _ptr(out), _ptr(bias), _ptr(ln_rs), _ptr(ln_c),
         _ptr(p), heads, float(cap), _stream(stream))
    return out


def video_patch_w(k, P):
    """The fused patch embedding's weight layout (vp_kernels.h video_patch_k; packed the same way by
    vp_finalize): k [P*P*3, N] (the patch kernel) -> [N, 64 P]: patch pixel row py is K-tile py, read as
    cpr = ceil(3P/8) chunks of 8 values at value offsets min(8 j, 3P - 8) in slots j < cpr (columns
    64 py + 8 j ..); zero where a row's last chunk overlaps its predecessor and in the slots j >= cpr."""
    import torch
    cpr = (3 * P + 7) // 8
    kv = 64 * P
    out = torch.zeros(k.shape[1], kv, dtype=k.dtype)
    for py in range(P):
        for cr in range(cpr):
            vo = min(8 * cr, 3 * P - 8)
            for e in range(8):
                v = vo + e
                if cr == cpr - 1 and v < 8 * (cpr - 1):
                    continue
                out[:, 64 * py + 8 * cr + e] = k[py * 3 * P + v]
    return out


def dev_patch_embed(video, P, wv, bias, pos, out, stream=None):
    """Fused patch embedding (EPI_POS_BF16) straight from bf16 frames [F, 16P, 16P, 3]."""
    frames = video.shape[0]
    call("vp_dev_patch_embed", _ptr(video), frames, P, _ptr(wv), wv.shape[0], _ptr(bias), _ptr(pos), _ptr(out),
         _stream(stream))
    return out


def dev_ln_stats(src, M, D, out, from_partials, stream=None):
    """(rstd, -mean*rstd) per row from partial statistics (from_partials) or bf16 rows."""
    call("vp_dev_ln_stats", 0 if from_partials else 1, _ptr(src), M, D, _ptr(out), _stream(stream))
    return out


# The pooler, small GEMM and text kernels one at a time.  The caller provides every output and scratch
# tensor (contiguous, on the device), so a test can prefill them and see what a kernel leaves alone.
def dev_pool_split_u(U):
    """Host only: U [H, D] fp32 (NumPy) -> the logits kernel's bf16 operand [32, D] as uint16 bits,
    rows (U_hi | U_lo | 0), packed by the function the engines' finalize calls."""
    import numpy as np
    U = np.ascontiguousarray(U, dtype=np.float32)
    H, D = U.shape
    ut = np.full((32, D), 0xFFFF, np.uint16)
    call("vp_dev_pool_split_u", U.ctypes.data_as(c_void_p), H, D, ut.ctypes.data_as(c_void_p))
    return ut


def dev_pool_chunks(S) -> int:
    """Row chunks the weighted sum splits S rows into (zpart is [G][chunks][H][D])."""
    n = load().vp_dev_pool_chunks(S)
    if n < 0:
        raise ValueError(f"bad S {S}")
    return n


def dev_pool_logits(x, S, U, Ut, logits, stream=None, wide=False):
    """logits [rows/S][H][S] fp32 = x [rows, D] (fp32 / bf16) . U [H, D]; Ut: the uploaded split or None.
    wide: the entry point that takes D up to 1536 (the plain one stops at 1024)."""
    rows, D = x.shape
    call("vp_dev_pool_logits_wide" if wide else "vp_dev_pool_logits", _ptr(x), _prec(x), rows, S, D, _ptr(U), _ptr(Ut), U.shape[0], _ptr(logits),
         _stream(stream))
    return logits


def dev_pool_softmax_wsum(x, G, S, H, logits, stats, zpart, z, stream=None, wide=False):
    """stats [G*H, 2] = (max, 1/sum exp), z [G, H, D] = softmax(logits [G, H, S]) . x [G*S, D].
    wide: D = 128 k up to 1536 (the plain entry point: 256 k up to 1024)."""
    call("vp_dev_pool_softmax_wsum_wide" if wide else "vp_dev_pool_softmax_wsum", _ptr(x), _prec(x), G, S, x.shape[1], H, _ptr(logits), _ptr(stats), _ptr(zpart),
         _ptr(z), _stream(stream))
    return z


def dev_small_gemm(A, lda, sA, Wt, sW, bias, sB, out, ldo, sO, M, N, K, batch=1, splits=0, part=None, stream=None):
    """out[b][m][n] = A[b][m][:] . Wt[b][:][n] + bias[b][n] in fp32 (element strides); splits >= 1: the
    split-K path (batch 1, part [splits][M][N])."""
    call("vp_dev_small_gemm", _ptr(A), lda, sA, _ptr(Wt), sW, _ptr(bias), sB, _ptr(out), ldo, sO, M, N, K, batch,
         splits, _ptr(part), _stream(stream))
    return out


def dev_ln_l2_rows(x, stride, rows, D, gamma1p, beta, do_l2, out, stream=None, wide=False):
    """out [rows, D] fp32 = LayerNorm (skipped if gamma1p is None) and / or L2 of rows x[r * stride : +D].
    wide: D up to 1536 (the plain entry point stops at 1024)."""
    call("vp_dev_ln_l2_rows_wide" if wide else "vp_dev_ln_l2_rows", _ptr(x), _prec(x), stride, rows, D, _ptr(gamma1p), _ptr(beta), 1 if do_l2 else 0,
         _ptr(out), _stream(stream))
    return out


def dev_layernorm_residual(y, gamma1p, beta, xs, pad=None, stream=None):
    """norm_policy 'primer_hybrid': xs [rows, D] fp32 += LayerNorm(y [rows, D] (fp32 / bf16) * (1 - pad [rows])),
    in place; D = 128 k."""
    rows, D = y.shape
    call("vp_dev_layernorm_residual", _ptr(y), _prec(y), rows, D, _ptr(gamma1p), _ptr(beta), _ptr(pad), _ptr(xs),
         _stream(stream))
    return xs


def dev_text_embed(ids, table, cls, pos, scale, out, pad_in, pad_out, stream=None):
    """out [Q, L+1, D] = table[clamp(ids)] * scale + pos, CLS row appended; pad_out [Q, L+1] = [pad_in | 0]."""
    Q, L = ids.shape
    V, D = table.shape
    call("vp_dev_text_embed", _ptr(ids), Q, L, _ptr(table), _prec(table), V, _ptr(cls), _ptr(pos), float(scale), D,
         _ptr(out), _prec(out), _ptr(pad_in), _ptr(pad_out), _stream(stream))
    return out


def dev_pooler_scratch_bytes(kind, handle, G, S) -> int:
    n = c_size_t()
    call("vp_dev_pooler", kind, handle, None, G, S, 0, None, None, ctypes.byref(n), None)
    return n.value


def dev_pooler(kind, handle, feat, G, S, do_l2, dst, scratch, stream=None):
    """The whole pooler of a finalized vp_clip (kind 0) / vp_classifier (kind 1) handle over tokens
    feat [G*S, D] in the handle's fprop dtype -> dst [G, D] fp32; scratch: uint8, dev_pooler_scratch_bytes."""
    n = c_size_t(scratch.numel())
    call("vp_dev_pooler", kind, handle, _ptr(feat), G, S, 1 if do_l2 else 0, _ptr(dst), _ptr(scratch),
         ctypes.byref(n), _stream(stream))
    return dst


# The classifier head's training ops.  `tensors`: {member of vp_probe_params: contiguous fp32 tensor on the
# tokens' device}, the parameters or, for the backward, the gradients to fill.
def _probe_struct(tensors):
    return vp_probe_params(**{member: _ptr(tensors[member]) for member, _ in PROBE_LEAVES})


def op_probe_workspace_bytes(model_dim, num_heads, num_classes, B, S) -> int:
    dims = vp_probe_dims(model_dim, num_heads, num_classes)
    n = c_size_t()
    call("vp_op_probe_workspace_bytes", ctypes.byref(dims), B, S, ctypes.byref(n))
    return n.value


def _probe_paddings(entry, paddings, tokens):
    """(entry point, its paddings arguments): the *_masked call for token paddings (a contiguous fp32 [B, S] tensor
    on the tokens' device), the unmasked one for None."""
    if paddings is None:
        return entry, ()
    import torch
    if (paddings.dtype != torch.float32 or not paddings.is_contiguous() or paddings.device != tokens.device or
            tuple(paddings.shape) != tuple(tokens.shape[:2])):
        raise ValueError(f"paddings must be a contiguous fp32 {tuple(tokens.shape[:2])} tensor on {tokens.device}")
    return entry + "_masked", (_ptr(paddings),)


def op_probe_forward(dims, tensors, tokens, logits, emb, ws, ws_bytes=None, stream=None, paddings=None):
    """logits [B, C] (and emb [B, D] unless None) of the head over tokens [B, S, D]; fills the workspace `ws`
    (uint8, op_probe_workspace_bytes) with what op_probe_backward needs.  paddings: None, or fp32 [B, S] with
    > 0.5 at the padded tokens (vp_op_probe_forward_masked)."""
    import torch
    B, S, _ = tokens.shape
    d = vp_probe_dims(*dims)
    entry, pad = _probe_paddings("vp_op_probe_forward", paddings, tokens)
    with torch.cuda.device(tokens.device):  # no handle: the ops launch on the current device
        call(entry, ctypes.byref(d), ctypes.byref(_probe_struct(tensors)), _ptr(tokens), _prec(tokens),
             B, S, *pad, _ptr(logits), _ptr(emb), _ptr(ws), ws.numel() if ws_bytes is None else ws_bytes,
             _stream(stream))
    return logits


def op_probe_backward(dims, tensors, tokens, dlogits, grads, ws, ws_bytes=None, stream=None, paddings=None):
    """Fills `grads` (same members as `tensors`) from dlogits [B, C] and the workspace the forward filled;
    paddings: what that forward was given."""
    import torch
    B, S, _ = tokens.shape
    d = vp_probe_dims(*dims)
    entry, pad = _probe_paddings("vp_op_probe_backward", paddings, tokens)
    with torch.cuda.device(tokens.device):
        call(entry, ctypes.byref(d), ctypes.byref(_probe_struct(tensors)), _ptr(tokens),
             _prec(tokens), B, S, *pad, _ptr(dlogits), ctypes.byref(_probe_struct(grads)), _ptr(ws),
             ws.numel() if ws_bytes is None else ws_bytes, _stream(stream))
    return grads


def dev_probe_backward_pass(dims, tokens, which, ws, stream=None):
    """Pass 1 (which 1: dl from the tokens) or pass 2 (which 2: dU) of the backward alone, on a workspace
    op_probe_backward has run on; for timing."""
    import torch
    B, S, _ = tokens.shape
    d = vp_probe_dims(*dims)
    with torch.cuda.device(tokens.device):
        call("vp_dev_probe_backward_pass", ctypes.byref(d), _ptr(tokens), _prec(tokens), B, S, which, _ptr(ws),
             ws.numel(), _stream(stream))


# vp_dev_attention_choice: stack kinds (vp_internal.h AttnKind; ATT_OP: as vp_op_attention maps S and the key
# paddings) and the kernels it returns (AttnKernel)
ATT_OP, ATT_VIDEO, ATT_LONG, ATT_TEXT = -1, 0, 1, 2
ATTN_KERNELS = ("SPATIAL", "TEMPORAL", "SEQ", "LONG", "MASKED", "F32", "F32_MFMA")


def dev_attention_choice(kind, precision, S, cap, has_key_pad=False, dim_per_head=64) -> str:
    """Name of the attention kernel a stack of `kind` with heads of dim_per_head values gets (no GPU call, no
    device needed); NotImplementedError where the library has no kernel of that width in that precision."""
    k = load().vp_dev_attention_choice_dh(kind, precision, S, float(cap), 1 if has_key_pad else 0, dim_per_head)
    if k == -2:
        raise NotImplementedError(f"no attention kernel for dim_per_head {dim_per_head} in precision {precision}")
    if k < 0:
        raise ValueError(f"bad argument: kind {kind}, precision {precision}, S {S}")
    return ATTN_KERNELS[k]


def op_attention(qkv, num_seq, S, heads, cap, key_pad=None, out=None, stream=None, dim_per_head=64):
    import torch
    D = heads * dim_per_head
    if out is None:
        out = torch.empty((num_seq * S, D), dtype=qkv.dtype, device=qkv.device)
    call("vp_op_attention_dh", _prec(qkv), _ptr(qkv), _ptr(out), num_seq, S, heads, dim_per_head, float(cap),
         _ptr(key_pad), _stream(stream))
    return out


def op_attention_masked(qkv, num_seq, S, heads, cap, key_pad=None, causal=False, out=None,
                        stream=None, dim_per_head=64):
    """Generic fp32-math attention with key paddings and the causal merge (text tower)."""
    import torch
    D = heads * dim_per_head
    if out is None:
        out = torch.empty((num_seq * S, D), dtype=qkv.dtype, device=qkv.device)
    call("vp_op_attention_masked_dh", _prec(qkv), _ptr(qkv), _ptr(out), num_seq, S, heads, dim_per_head, float(cap),
         _ptr(key_pad), 1 if causal else 0, _stream(stream))
    return out


def op_similarity(video_emb, text_emb, stream=None):
    """video_emb [B, D] . text_emb [Q, D]^T (fp32)."""
    import torch
    B, D = video_emb.shape
    Q = text_emb.shape[0]
    out = torch.empty((B, Q), dtype=torch.float32, device=video_emb.device)
    call("vp_op_similarity", _ptr(video_emb), _ptr(text_emb), B, Q, D, _ptr(out), _stream(stream))
    return out


def op_topk_workspace_bytes(Q, k) -> int:
    n = c_size_t()
    call("vp_op_topk_workspace_bytes", Q, k, ctypes.byref(n))
    return n.value


def op_topk(queries, gallery, k, id_base=0, stream=None, ws=None):
    """The k rows of gallery [N, D] (fp32 or bf16, unit row stride along D, any row stride) with the largest dot
    product per row of queries [Q, D] (fp32): (scores [Q, k] fp32, ids [Q, k] int64 = id_base + row), score
    descending and equal scores by ascending id; fewer than k rows leave (-inf, -1).  `ws`: uint8 workspace of
    op_topk_workspace_bytes(Q, k) bytes (allocated when None)."""
    import torch
    Q, D = queries.shape
    N = gallery.shape[0]
    if gallery.dim() != 2 or gallery.shape[1] != D or (N > 1 and gallery.stride(1) != 1):
        raise ValueError(f"gallery must be [N, {D}] with contiguous rows, got {tuple(gallery.shape)}")
    if queries.dtype != torch.float32:
        raise TypeError("queries must be fp32")
    queries = queries.contiguous()
    ld = gallery.stride(0) if N > 1 else D
    scores = torch.empty((Q, k), dtype=torch.float32, device=queries.device)
    ids = torch.empty((Q, k), dtype=torch.int64, device=queries.device)
    if Q == 0:
        return scores, ids
    if ws is None:
        ws = torch.empty(op_topk_workspace_bytes(Q, k), dtype=torch.uint8, device=queries.device)
    with torch.cuda.device(queries.device):  # no handle: the op launches on the current device
        call("vp_op_topk", _ptr(queries), Q, _ptr(gallery), _prec(gallery), N, ld, D, k, id_base, _ptr(scores),
             _ptr(ids), _ptr(ws), ws.numel(), _stream(stream))
    return scores, ids


def op_topk_merge(scores, ids, k, stream=None):
    """The best k per query of sorted lists scores / ids [parts, Q, k_in] (op_topk's order; ids < 0 are padding)."""
    import torch
    parts, Q, k_in = scores.shape
    scores, ids = scores.contiguous(), ids.contiguous()
    out_s = torch.empty((Q, k), dtype=torch.float32, device=scores.device)
    out_i = torch.empty((Q, k), dtype=torch.int64, device=scores.device)
    with torch.cuda.device(scores.device):
        call("vp_op_topk_merge", _ptr(scores), _ptr(ids), parts, Q, k_in, k, _ptr(out_s), _ptr(out_i),
             _stream(stream))
    return out_s, out_i


def op_topk_groups_workspace_bytes(Q, k) -> int:
    n = c_size_t()
    call("vp_op_topk_groups_workspace_bytes", Q, k, ctypes.byref(n))
    return n.value


def op_topk_groups(queries, gallery, labels, k, id_base=0, stream=None, ws=None):
    """The k best groups of gallery rows per row of queries [Q, D] (fp32): labels [N] int64 names each row's group (a
    negative label blanks the row out), a group scores as its best row, and the result is (scores [Q, k] fp32,
    groups [Q, k] int64, ids [Q, k] int64 = id_base + best row), score descending and equal scores by ascending id;
    fewer than k groups leave (-inf, -1, -1).  Gallery and `ws` as op_topk (op_topk_groups_workspace_bytes)."""
    import torch
    Q, D = queries.shape
    N = gallery.shape[0]
    if gallery.dim() != 2 or gallery.shape[1] != D or (N > 1 and gallery.stride(1) != 1):
        raise ValueError(f"gallery must be [N, {D}] with contiguous rows, got {tuple(gallery.shape)}")
    if queries.dtype != torch.float32:
        raise TypeError("queries must be fp32")
    if labels.dtype != torch.int64 or tuple(labels.shape) != (N,):
        raise ValueError(f"labels must be int64 [{N}], got {labels.dtype} {tuple(labels.shape)}")
    queries, labels = queries.contiguous(), labels.contiguous()
    ld = gallery.stride(0) if N > 1 else D
    scores = torch.empty((Q, k), dtype=torch.float32, device=queries.device)
    groups = torch.empty((Q, k), dtype=torch.int64, device=queries.device)
    ids = torch.empty((Q, k), dtype=torch.int64, device=queries.device)
    if Q == 0:
        return scores, groups, ids
    if ws is None:
        ws = torch.empty(op_topk_groups_workspace_bytes(Q, k), dtype=torch.uint8, device=queries.device)
    with torch.cuda.device(queries.device):  # no handle: the op launches on the current device
        call("vp_op_topk_groups", _ptr(queries), Q, _ptr(gallery), _prec(gallery), N, ld, D, _ptr(labels), k, id_base,
             _ptr(scores), _ptr(groups), _ptr(ids), _ptr(ws), ws.numel(), _stream(stream))
    return scores, groups, ids


def op_topk_groups_merge(scores, groups, ids, k, stream=None):
    """The best k groups per query of lists scores / groups / ids [parts, Q, k_in] as op_topk_groups returns them; of a
    group's entries in several lists the one that comes first in the order stays."""
    import torch
    parts, Q, k_in = scores.shape
    scores, groups, ids = scores.contiguous(), groups.contiguous(), ids.contiguous()
    out_s = torch.empty((Q, k), dtype=torch.float32, device=scores.device)
    out_g = torch.empty((Q, k), dtype=torch.int64, device=scores.device)
    out_i = torch.empty((Q, k), dtype=torch.int64, device=scores.device)
    with torch.cuda.device(scores.device):
        call("vp_op_topk_groups_merge", _ptr(scores), _ptr(groups), _ptr(ids), parts, Q, k_in, k, _ptr(out_s),
             _ptr(out_g), _ptr(out_i), _stream(stream))
    return out_s, out_g, out_i


def rowmask_words(N) -> int:
    """Words of one packed row mask of N rows."""
    return (int(N) + 31) // 32


def _check_mask(mask, Q, N):
    """The query stride in words of a packed mask int32 [words] (shared, stride 0) or [Q, words]."""
    import torch
    W = rowmask_words(N)
    if mask.dtype != torch.int32:
        raise TypeError(f"mask must be packed int32 words, got {mask.dtype}")
    if mask.dim() == 1 and mask.shape[0] >= W:
        if mask.numel() > 1 and mask.stride(0) != 1:
            raise ValueError("mask words must be contiguous")
        return 0
    if mask.dim() == 2 and mask.shape[0] == Q and mask.shape[1] >= W:
        if mask.shape[1] > 1 and mask.stride(1) != 1:
            raise ValueError("mask words must be contiguous")
        return max(mask.stride(0), W) if Q > 1 else max(mask.shape[1], W)
    raise ValueError(f"mask must be int32 [>= {W}] or [{Q}, >= {W}], got {tuple(mask.shape)}")


def op_rowmask_pack(allow, and_words=None, out=None, stream=None):
    """Packed row masks, int32 [words] of allow [N] or [Q, words] of allow [Q, N] (bool or uint8, nonzero = allowed;
    words = ceil(N / 32), bit r & 31 of word r >> 5 is row r, bits past N zero), ANDed with and_words (packed int32
    [words], the same for every row of allow, or [Q, words]) where given."""
    import torch
    if allow.dtype not in (torch.bool, torch.uint8):
        raise TypeError(f"allow must be bool or uint8, got {allow.dtype}")
    if allow.dim() not in (1, 2):
        raise ValueError(f"allow must be [N] or [Q, N], got {tuple(allow.shape)}")
    shape = tuple(allow.shape)
    Q, N = (1 if len(shape) == 1 else shape[0]), shape[-1]
    a = allow.contiguous().view(torch.uint8).reshape(Q, N)
    W = rowmask_words(N)
    and_stride = 0
    if and_words is not None:
        and_stride = _check_mask(and_words, Q, N)
        if and_words.device != a.device:
            raise ValueError("and_words must be on allow's device")
    if out is None:
        out = torch.zeros((Q, W), dtype=torch.int32, device=a.device)
    elif out.dtype != torch.int32 or tuple(out.shape) != (Q, W) or not out.is_contiguous():
        raise ValueError(f"out must be contiguous int32 [{Q}, {W}]")
    if Q and N:
        with torch.cuda.device(a.device):
            call("vp_op_rowmask_pack", _ptr(a), Q, N, _ptr(and_words), and_stride, _ptr(out), W, _stream(stream))
    return out.view(W) if len(shape) == 1 else out


def op_topk_masked(queries, gallery, k, mask, id_base=0, stream=None, ws=None):
    """op_topk over the rows that `mask` allows: packed int32 words (op_rowmask_pack), [words] for all queries or
    [Q, words] for a mask per query.  The result is op_topk's on a gallery of the allowed rows alone, ids mapped
    back, scores bit for bit.  `ws` as op_topk's (op_topk_workspace_bytes)."""
    import torch
    Q, D = queries.shape
    N = gallery.shape[0]
    if gallery.dim() != 2 or gallery.shape[1] != D or (N > 1 and gallery.stride(1) != 1):
        raise ValueError(f"gallery must be [N, {D}] with contiguous rows, got {tuple(gallery.shape)}")
    if queries.dtype != torch.float32:
        raise TypeError("queries must be fp32")
    mstride = _check_mask(mask, Q, N)
    queries = queries.contiguous()
    ld = gallery.stride(0) if N > 1 else D
    scores = torch.empty((Q, k), dtype=torch.float32, device=queries.device)
    ids = torch.empty((Q, k), dtype=torch.int64, device=queries.device)
    if Q == 0:
        return scores, ids
    if ws is None:
        ws = torch.empty(op_topk_workspace_bytes(Q, k), dtype=torch.uint8, device=queries.device)
    with torch.cuda.device(queries.device):
        call("vp_op_topk_masked", _ptr(queries), Q, _ptr(gallery), _prec(gallery), N, ld, D, k, id_base, _ptr(mask),
             mstride, _ptr(scores), _ptr(ids), _ptr(ws), ws.numel(), _stream(stream))
    return scores, ids


def op_topk_groups_masked(queries, gallery, labels, k, mask, id_base=0, stream=None, ws=None):
    """op_topk_groups over the rows that `mask` allows (as op_topk_masked): a row that is not allowed never stands for
    its group.  `ws` as op_topk_groups's."""
    import torch
    Q, D = queries.shape
    N = gallery.shape[0]
    if gallery.dim() != 2 or gallery.shape[1] != D or (N > 1 and gallery.stride(1) != 1):
        raise ValueError(f"gallery must be [N, {D}] with contiguous rows, got {tuple(gallery.shape)}")
    if queries.dtype != torch.float32:
        raise TypeError("queries must be fp32")
    if labels.dtype != torch.int64 or tuple(labels.shape) != (N,):
        raise ValueError(f"labels must be int64 [{N}], got {labels.dtype} {tuple(labels.shape)}")
    mstride = _check_mask(mask, Q, N)
    queries, labels = queries.contiguous(), labels.contiguous()
    ld = gallery.stride(0) if N > 1 else D
    scores = torch.empty((Q, k), dtype=torch.float32, device=queries.device)
    groups = torch.empty((Q, k), dtype=torch.int64, device=queries.device)
    ids = torch.empty((Q, k), dtype=torch.int64, device=queries.device)
    if Q == 0:
        return scores, groups, ids
    if ws is None:
        ws = torch.empty(op_topk_groups_workspace_bytes(Q, k), dtype=torch.uint8, device=queries.device)
    with torch.cuda.device(queries.device):
        call("vp_op_topk_groups_masked", _ptr(queries), Q, _ptr(gallery), _prec(gallery), N, ld, D, _ptr(labels), k,
             id_base, _ptr(mask), mstride, _ptr(scores), _ptr(groups), _ptr(ids), _ptr(ws), ws.numel(),
             _stream(stream))
    return scores, groups, ids


def _codes_u8(codes):
    """An e4m3 code buffer as the bytes the library takes (torch.float8_e4m3fn or uint8, the same storage)."""
    import torch
    if codes.dtype == torch.float8_e4m3fn:
        return codes.view(torch.uint8)
    if codes.dtype != torch.uint8:
        raise TypeError(f"codes must be float8_e4m3fn or uint8, got {codes.dtype}")
    return codes


def op_quantize_rows_f8(x, codes=None, scales=None, stream=None):
    """x [N, D] (fp32 or bf16, unit stride along D, rows 16-byte aligned) as the fp8 gallery stores it: (codes [N, D]
    float8_e4m3fn, scales [N] fp32), row r standing for codes[r] * scales[r] with scales[r] the power of two that puts
    the row's largest finite magnitude in (224, 448].  `codes` / `scales`: where to write (codes with any row stride
    that is a multiple of 16 bytes; its columns past D keep what they hold); allocated when None."""
    import torch
    if x.dim() != 2 or (x.shape[0] > 1 and x.stride(1) != 1):
        raise ValueError(f"x must be [N, D] with contiguous rows, got {tuple(x.shape)}")
    if x.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError(f"x must be fp32 or bf16, got {x.dtype}")
    N, D = x.shape
    if codes is None:
        codes = torch.empty((N, D), dtype=torch.float8_e4m3fn, device=x.device)
    if scales is None:
        scales = torch.empty((N,), dtype=torch.float32, device=x.device)
    cb = _codes_u8(codes)
    if tuple(cb.shape) != (N, D) or (N > 1 and cb.stride(1) != 1):
        raise ValueError(f"codes must be [{N}, {D}] with contiguous rows, got {tuple(cb.shape)}")
    if scales.dtype != torch.float32 or tuple(scales.shape) != (N,) or not scales.is_contiguous():
        raise ValueError(f"scales must be contiguous fp32 [{N}], got {scales.dtype} {tuple(scales.shape)}")
    if N:
        ldx = x.stride(0) if N > 1 else D
        ldc = cb.stride(0) if N > 1 else D
        with torch.cuda.device(x.device):
            call("vp_op_quantize_rows_f8", _ptr(x), _prec(x), N, ldx, D, _ptr(cb), ldc, _ptr(scales), _stream(stream))
    return codes, scales


def _f8_gallery(queries, codes, scales):
    """(codes as bytes, N, ld in bytes) of an fp8 gallery after the shape checks the four searches share."""
    import torch
    Q, D = queries.shape
    cb = _codes_u8(codes)
    N = cb.shape[0]
    if cb.dim() != 2 or cb.shape[1] != D or (N > 1 and cb.stride(1) != 1):
        raise ValueError(f"codes must be [N, {D}] with contiguous rows, got {tuple(cb.shape)}")
    if scales.dtype != torch.float32 or tuple(scales.shape) != (N,) or (N > 1 and scales.stride(0) != 1):
        raise ValueError(f"scales must be contiguous fp32 [{N}], got {scales.dtype} {tuple(scales.shape)}")
    if queries.dtype != torch.float32:
        raise TypeError("queries must be fp32")
    return cb, N, (cb.stride(0) if N > 1 else D)


def op_topk_f8(queries, codes, scales, k, id_base=0, stream=None, ws=None):
    """op_topk over an fp8 gallery: codes [N, D] (float8_e4m3fn or its bytes, any row stride that is a multiple of 16)
    and scales [N] fp32, powers of two, as op_quantize_rows_f8 makes them.  Order, padding and `ws` as op_topk."""
    import torch
    Q, D = queries.shape
    cb, N, ld = _f8_gallery(queries, codes, scales)
    queries = queries.contiguous()
    out_s = torch.empty((Q, k), dtype=torch.float32, device=queries.device)
    ids = torch.empty((Q, k), dtype=torch.int64, device=queries.device)
    if Q == 0:
        return out_s, ids
    if ws is None:
        ws = torch.empty(op_topk_workspace_bytes(Q, k), dtype=torch.uint8, device=queries.device)
    with torch.cuda.device(queries.device):
        call("vp_op_topk_f8", _ptr(queries), Q, _ptr(cb), _ptr(scales), N, ld, D, k, id_base, _ptr(out_s), _ptr(ids),
             _ptr(ws), ws.numel(), _stream(stream))
    return out_s, ids


def op_topk_groups_f8(queries, codes, scales, labels, k, id_base=0, stream=None, ws=None):
    """op_topk_groups over an fp8 gallery (codes and scales as op_topk_f8)."""
    import torch
    Q, D = queries.shape
    cb, N, ld = _f8_gallery(queries, codes, scales)
    if labels.dtype != torch.int64 or tuple(labels.shape) != (N,):
        raise ValueError(f"labels must be int64 [{N}], got {labels.dtype} {tuple(labels.shape)}")
    queries, labels = queries.contiguous(), labels.contiguous()
    out_s = torch.empty((Q, k), dtype=torch.float32, device=queries.device)
    groups = torch.empty((Q, k), dtype=torch.int64, device=queries.device)
    ids = torch.empty((Q, k), dtype=torch.int64, device=queries.device)
    if Q == 0:
        return out_s, groups, ids
    if ws is None:
        ws = torch.empty(op_topk_groups_workspace_bytes(Q, k), dtype=torch.uint8, device=queries.device)
    with torch.cuda.device(queries.device):
        call("vp_op_topk_groups_f8", _ptr(queries), Q, _ptr(cb), _ptr(scales), N, ld, D, _ptr(labels), k, id_base,
             _ptr(out_s), _ptr(groups), _ptr(ids), _ptr(ws), ws.numel(), _stream(stream))
    return out_s, groups, ids


def op_topk_masked_f8(queries, codes, scales, k, mask, id_base=0, stream=None, ws=None):
    """op_topk_masked over an fp8 gallery (codes and scales as op_topk_f8)."""
    import torch
    Q, D = queries.shape
    cb, N, ld = _f8_gallery(queries, codes, scales)
    mstride = _check_mask(mask, Q, N)
    queries = queries.contiguous()
    out_s = torch.empty((Q, k), dtype=torch.float32, device=queries.device)
    ids = torch.empty((Q, k), dtype=torch.int64, device=queries.device)
    if Q == 0:
        return out_s, ids
    if ws is None:
        ws = torch.empty(op_topk_workspace_bytes(Q, k), dtype=torch.uint8, device=queries.device)
    with torch.cuda.device(queries.device):
        call("vp_op_topk_masked_f8", _ptr(queries), Q, _ptr(cb), _ptr(scales), N, ld, D, k, id_base, _ptr(mask),
             mstride, _ptr(out_s), _ptr(ids), _ptr(ws), ws.numel(), _stream(stream))
    return out_s, ids


def op_topk_groups_masked_f8(queries, codes, scales, labels, k, mask, id_base=0, stream=None, ws=None):
    """op_topk_groups_masked over an fp8 gallery (codes and scales as op_topk_f8)."""
    import torch
    Q, D = queries.shape
    cb, N, ld = _f8_gallery(queries, codes, scales)
    if labels.dtype != torch.int64 or tuple(labels.shape) != (N,):
        raise ValueError(f"labels must be int64 [{N}], got {labels.dtype} {tuple(labels.shape)}")
    mstride = _check_mask(mask, Q, N)
    queries, labels = queries.contiguous(), labels.contiguous()
    out_s = torch.empty((Q, k), dtype=torch.float32, device=queries.device)
    groups = torch.empty((Q, k), dtype=torch.int64, device=queries.device)
    ids = torch.empty((Q, k), dtype=torch.int64, device=queries.device)
    if Q == 0:
        return out_s, groups, ids
    if ws is None:
        ws = torch.empty(op_topk_groups_workspace_bytes(Q, k), dtype=torch.uint8, device=queries.device)
    with torch.cuda.device(queries.device):
        call("vp_op_topk_groups_masked_f8", _ptr(queries), Q, _ptr(cb), _ptr(scales), N, ld, D, _ptr(labels), k,
             id_base, _ptr(mask), mstride, _ptr(out_s), _ptr(groups), _ptr(ids), _ptr(ws), ws.numel(),
             _stream(stream))
    return out_s, groups, ids


def op_layernorm(x, gamma1p, beta, out_dtype=None, perm=PERM_NONE, T=1, Nsp=1, add=None,
                 stream=None):
    import torch
    rows, D = x.shape
    out_dtype = out_dtype or torch.float32
    out = torch.empty((rows, D), dtype=out_dtype, device=x.device)
    call("vp_op_layernorm", _ptr(x), _prec(x), rows, D, _ptr(gamma1p), _ptr(beta), _ptr(out),
         VP_BF16 if out_dtype == torch.bfloat16 else VP_F32, perm, T, Nsp, _ptr(add),
         _stream(stream))
    return out


def dev_gather_frames(states, frame_idx, out, stream=None):
    """out[s] = states[clamp(frame_idx[s], 0, F - 1)]: states [F, ...] contiguous, frame_idx int32 [nslots] on the
    device, out [nslots, ...] of the same dtype (written in place: the caller prefills it)."""
    F = states.shape[0]
    frame_bytes = states[0].numel() * states.element_size()
    call("vp_dev_gather_frames", _ptr(states), F, _ptr(frame_idx), frame_idx.numel(), frame_bytes, _ptr(out),
         _stream(stream))
    return out


def dev_layernorm_gather(states, frame_idx, T, gamma1p, beta, out, perm=PERM_NONE, add=None, out_rs=None,
                         stream=None):
    """gather_frames, then LayerNorm, as vp_forward_temporal launches them: states [F, Nsp, D], frame_idx int32
    [Wn*T] on the device (clamped to [0, F - 1] by the kernel), out [Wn*T*Nsp, D] bf16 / fp32 and out_rs (optional)
    fp32 [Wn*T*Nsp, 2] by output row, both written in place (the caller prefills them)."""
    import torch
    F, Nsp, D = states.shape
    rows = frame_idx.numel() * Nsp
    scratch = torch.empty((rows, D), dtype=states.dtype, device=states.device)
    call("vp_dev_layernorm_gather", _ptr(states), _prec(states), F, _ptr(frame_idx), rows, D, _ptr(gamma1p),
         _ptr(beta), _ptr(out), _prec(out), perm, T, Nsp, _ptr(add), _ptr(out_rs), _ptr(scratch), _stream(stream))
    return out


def op_patchify(video, P, kpad, out_dtype=None, stream=None):
    import torch
    BT, H, W, C = video.shape
    out_dtype = out_dtype or video.dtype
    out = torch.empty((BT * (H // P) * (W // P), kpad), dtype=out_dtype, device=video.device)
    call("vp_op_patchify", _ptr(video), _prec(video), _ptr(out),
         VP_BF16 if out_dtype == torch.bfloat16 else VP_F32, BT, H, W, C, P, kpad, _stream(stream))
    return out


def op_preprocess_frames(src, frame_idx=None, mode=VP_RESIZE_CENTER_CROP, swap_rb=False, size=288, out=None,
                         stream=None):
    """uint8 frames [N, H, W, 3] (any frame and row strides: views work) -> uint8 [F, size, size, 3],
    resized as cv2.resize does on uint8 and centre-cropped (or stretched); frame_idx int32 [F] on the
    device picks the frames (None: all N in order)."""
    import torch
    if src.dtype != torch.uint8 or src.dim() != 4 or src.shape[3] != 3:
        raise ValueError(f"frames must be uint8 [N, H, W, 3], got {src.dtype} {tuple(src.shape)}")
    N, H, W, _ = src.shape
    if src.stride(3) != 1 or (W > 1 and src.stride(2) != 3):
        raise ValueError("frames must have packed pixels (channel stride 1, pixel stride 3)")
    # a dimension of extent 1 may carry any stride: give the packed one
    row_stride = src.stride(1) if H > 1 else 3 * W
    frame_stride = src.stride(0) if N > 1 else H * row_stride
    if frame_idx is not None and (frame_idx.dtype != torch.int32 or frame_idx.dim() != 1 or
                                  not frame_idx.is_contiguous() or frame_idx.device != src.device):
        raise ValueError("frame_idx must be a contiguous int32 vector on the frames' device")
    F = N if frame_idx is None else frame_idx.shape[0]
    if out is None:
        out = torch.empty((F, size, size, 3), dtype=torch.uint8, device=src.device)
    elif out.dtype != torch.uint8 or tuple(out.shape) != (F, size, size, 3) or not out.is_contiguous():
        raise ValueError(f"out must be contiguous uint8 {(F, size, size, 3)}")
    with torch.cuda.device(src.device):  # the entry point has no handle: it launches on the current device
        call("vp_op_preprocess_frames", _ptr(src), N, H, W, row_stride, frame_stride, _ptr(frame_idx), F, int(mode),
             1 if swap_rb else 0, size, _ptr(out), _stream(stream))
    return out


def _views_args(views, frame_idx, N, size, out, device):
    """(V, T, out) of a view launch: views int32 [V, 9] and frame_idx int32 [V, T] (None: T = N, frame t of every
    view is source frame t), both contiguous on `device`; out uint8 [V * T, size, size, 3]."""
    import torch
    if (views.dtype != torch.int32 or views.dim() != 2 or views.shape[1] != 9 or views.shape[0] < 1 or
            not views.is_contiguous() or views.device != device):
        raise ValueError("views must be a contiguous int32 [V, 9] table on the frames' device")
    V = views.shape[0]
    if frame_idx is not None and (frame_idx.dtype != torch.int32 or frame_idx.dim() != 2 or frame_idx.shape[0] != V or
                                  not frame_idx.is_contiguous() or frame_idx.device != device):
        raise ValueError(f"frame_idx must be a contiguous int32 [{V}, T] matrix on the frames' device")
    T = N if frame_idx is None else frame_idx.shape[1]
    if out is None:
        out = torch.empty((V * T, size, size, 3), dtype=torch.uint8, device=device)
    elif out.dtype != torch.uint8 or tuple(out.shape) != (V * T, size, size, 3) or not out.is_contiguous():
        raise ValueError(f"out must be contiguous uint8 {(V * T, size, size, 3)}")
    return V, T, out


def op_preprocess_views(src, views, frame_idx=None, swap_rb=False, size=288, out=None, stream=None):
    """op_preprocess_frames with the geometry per output frame: views int32 [V, 9] on the device (rows box_y, box_x,
    box_h, box_w, new_h, new_w, win_y, win_x, flags; clamped by the kernel, see vp_op_preprocess_views), frame_idx
    int32 [V, T] on the device (None: all N frames for every view) -> uint8 [V * T, size, size, 3], view-major."""
    import torch
    if src.dtype != torch.uint8 or src.dim() != 4 or src.shape[3] != 3:
        raise ValueError(f"frames must be uint8 [N, H, W, 3], got {src.dtype} {tuple(src.shape)}")
    N, H, W, _ = src.shape
    if src.stride(3) != 1 or (W > 1 and src.stride(2) != 3):
        raise ValueError("frames must have packed pixels (channel stride 1, pixel stride 3)")
    # a dimension of extent 1 may carry any stride: give the packed one
    row_stride = src.stride(1) if H > 1 else 3 * W
    frame_stride = src.stride(0) if N > 1 else H * row_stride
    V, T, out = _views_args(views, frame_idx, N, size, out, src.device)
    with torch.cuda.device(src.device):  # the entry point has no handle: it launches on the current device
        call("vp_op_preprocess_views", _ptr(src), N, H, W, row_stride, frame_stride, _ptr(frame_idx), _ptr(views), V, T,
             1 if swap_rb else 0, size, _ptr(out), _stream(stream))
    return out


def op_pool_l2(emb, stream=None):
    import torch
    B, L, D = emb.shape
    out = torch.empty((B, D), dtype=torch.float32, device=emb.device)
    call("vp_op_pool_l2", _ptr(emb), _prec(emb), B, L, D, _ptr(out), _stream(stream))
    return out


def source_fingerprint() -> str:
    """sha256 over the product library's sources (the Makefile's SRC list, csrc/ headers and
    include/): bench.py only quotes PMC traffic measured on a build of exactly these sources.
    Files only the tools' diag library compiles (DIAG_SRC) do not count."""
    import hashlib
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc = os.path.join(root, "csrc")
    with open(os.path.join(root, "Makefile")) as fh:
        m = re.search(r"^SRC\s*:=\s*(.+)$", fh.read(), re.M)
    product = {os.path.basename(f) for f in m.group(1).split()} if m else None
    files = []
    for d in (csrc, os.path.join(os.path.dirname(root), "include")):
        if os.path.isdir(d):
            files += sorted(os.path.join(d, f) for f in os.listdir(d)
                            if f.endswith(".h") or (f.endswith((".hip", ".cpp")) and
                                                    (product is None or f in product)))
    h = hashlib.sha256()
    for f in files:
        h.update(os.path.basename(f).encode())
        with open(f, "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()[:16]


def kernel_short_name(symbol: str) -> str:
    """'void vp::(anonymous namespace)::gemm_bf16_w4_kernel<9, 512, 0>(...)' ->
    'gemm_bf16_w4_kernel<9, 512, 0>' (the same key tools/pmc_summary.py gives rocprof's names)."""
    import re
    m = re.search(r"(\w+_kernel\w*)<([^>]*)>", symbol)
    if m:
        return f"{m.group(1)}<{m.group(2)}>"
    m = re.search(r"(\w+_kernel\w*)\b", symbol)
    return m.group(1) if m else symbol


def profile_kernel_name(handle, cls_name: str) -> str:
    """Short symbol of the kernel last launched for profiler class `cls_name` on `handle`."""
    lib = load()
    for i in range(lib.vp_profile_class_count()):
        n = ctypes.c_char_p()
        call("vp_profile_class_name", i, ctypes.byref(n))
        if n.value.decode() == cls_name:
            k = ctypes.c_char_p()
            call("vp_profile_kernel_name", handle, i, ctypes.byref(k))
            return kernel_short_name(k.value.decode()) if k.value else ""
    return ""


def yuv_coefficients(matrix, color_range, bit_depth):
    """The 16.16 table of vp_op_preprocess_yuv: (int32 [3][3] rows R, G, B x (cy, cu, cv), yoff, coff)."""
    out = (c_int32 * 11)()
    call("vp_dev_yuv_coefficients", int(matrix), int(color_range), int(bit_depth), out)
    v = list(out)
    return [v[0:3], v[3:6], v[6:9]], v[9], v[10]


def yuv_frames(planes, pixel_format=VP_YUV_NV12, matrix=VP_YUV_BT601, color_range=VP_YUV_LIMITED):
    """(vp_yuv_frames, N, H, W) of device planes, which the struct points into: (y [N, H, W],
    uv [N, ceil(H/2), ceil(W/2), 2]) for NV12 (uint8) and P010 (int16 / uint16 words), (y, u [N, ceil(H/2),
    ceil(W/2)], v) for I420, with any frame and row strides (only the sample, or the U,V pair, must be contiguous)."""
    import torch
    nplanes = {VP_YUV_NV12: 2, VP_YUV_I420: 3, VP_YUV_P010: 2}.get(pixel_format)
    if nplanes is None:
        raise ValueError(f"Unknown pixel format: {pixel_format}")
    if len(planes) != nplanes:
        raise ValueError(f"pixel format {pixel_format} takes {nplanes} planes, got {len(planes)}")
    words = (torch.uint16, torch.int16) if pixel_format == VP_YUV_P010 else (torch.uint8,)
    y = planes[0]
    if y.dim() != 3:
        raise ValueError(f"the Y plane must be [N, H, W], got {tuple(y.shape)}")
    N, H, W = y.shape
    chroma = (N, (H + 1) // 2, (W + 1) // 2) + ((2,) if nplanes == 2 else ())
    src = vp_yuv_frames(format=int(pixel_format), matrix=int(matrix), range=int(color_range))
    for p, t in enumerate(planes):
        want = chroma if p else (N, H, W)
        if t.dtype not in words or tuple(t.shape) != want or t.device != y.device:
            raise ValueError(f"plane {p} must be {words[0]} {want} on the Y plane's device, got {t.dtype} {tuple(t.shape)}")
        inner = t.stride()[2:]
        if any(s != w for s, w, n in zip(inner, (2, 1) if len(inner) == 2 else (1,), want[2:]) if n > 1):
            raise ValueError(f"plane {p} must have contiguous samples" + (" (U,V pairs)" if len(inner) == 2 else ""))
        item = t.element_size()
        row_bytes = want[2] * (2 if len(inner) == 2 else 1) * item
        # a dimension of extent 1 may carry any stride: give the packed one
        row_stride = t.stride(1) * item if want[1] > 1 else row_bytes
        src.plane[p] = t.data_ptr()
        src.row_stride[p] = row_stride
        src.frame_stride[p] = t.stride(0) * item if N > 1 else want[1] * row_stride
    return src, N, H, W


def op_preprocess_yuv(planes, pixel_format=VP_YUV_NV12, matrix=VP_YUV_BT601, color_range=VP_YUV_LIMITED,
                      frame_idx=None, mode=VP_RESIZE_CENTER_CROP, size=288, out=None, stream=None):
    """4:2:0 decoder planes (see yuv_frames; read in place) -> uint8 RGB [F, size, size, 3]: op_preprocess_frames
    on the RGB frames the planes stand for, which are never stored."""
    import torch
    src, N, H, W = yuv_frames(planes, pixel_format, matrix, color_range)
    y = planes[0]
    if frame_idx is not None and (frame_idx.dtype != torch.int32 or frame_idx.dim() != 1 or
                                  not frame_idx.is_contiguous() or frame_idx.device != y.device):
        raise ValueError("frame_idx must be a contiguous int32 vector on the planes' device")
    F = N if frame_idx is None else frame_idx.shape[0]
    if out is None:
        out = torch.empty((F, size, size, 3), dtype=torch.uint8, device=y.device)
    elif out.dtype != torch.uint8 or tuple(out.shape) != (F, size, size, 3) or not out.is_contiguous():
        raise ValueError(f"out must be contiguous uint8 {(F, size, size, 3)}")
    with torch.cuda.device(y.device):  # the entry point has no handle: it launches on the current device
        call("vp_op_preprocess_yuv", ctypes.byref(src), N, H, W, _ptr(frame_idx), F, int(mode), size, _ptr(out),
             _stream(stream))
    return out


def op_preprocess_yuv_views(planes, views, pixel_format=VP_YUV_NV12, matrix=VP_YUV_BT601, color_range=VP_YUV_LIMITED,
                            frame_idx=None, size=288, out=None, stream=None):
    """op_preprocess_views on the RGB frames that 4:2:0 decoder planes stand for (see yuv_frames; read in place, the
    RGB frames are never stored): views int32 [V, 9], frame_idx int32 [V, T] or None -> uint8 [V * T, size, size, 3]."""
    import torch
    src, N, H, W = yuv_frames(planes, pixel_format, matrix, color_range)
    y = planes[0]
    V, T, out = _views_args(views, frame_idx, N, size, out, y.device)
    with torch.cuda.device(y.device):  # the entry point has no handle: it launches on the current device
        call("vp_op_preprocess_yuv_views", ctypes.byref(src), N, H, W, _ptr(frame_idx), _ptr(views), V, T, size,
             _ptr(out), _stream(stream))
    return out
