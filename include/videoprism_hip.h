/*
 * videoprism_hip.h — C-ABI of the MI355X (gfx950) VideoPrism video-encoder library
 * (libvideoprism_hip.so).
 *
 * The reference (tmoroney/videoprism-mlx) has no native FFI: its drop-in surface is the
 * Python API `models.get_model(name, fprop_dtype=...)` + `model.apply(variables, inputs,
 * train=False, return_intermediate=..., frame_paddings=...)` (videoprism/models.py:268-303,
 * videoprism/encoders.py:411-580) and `models_mlx.load_video_encoder(name, weights_path)`
 * (videoprism/models_mlx.py:146-210).  This header is the boundary those Python entry
 * points (videoprism-mlx_amd/videoprism/) bind through ctypes; any other host language
 * binds the same symbols.
 *
 * Conventions
 *  - Every function returns an int status (VP_OK == 0).  On failure a thread-local
 *    message is available from vp_last_error().  VP_EINVAL carries the same messages the
 *    reference raises as ValueError/AssertionError (e.g. encoders.py:86-90).
 *  - Plain pointers and sizes only.  Device pointers are HIP device memory of the handle's
 *    device; `stream` is a hipStream_t passed as void* (NULL = default stream).
 *  - Parameters are passed once, as HOST fp32 arrays in the reference's own Flax layout
 *    and names (scanned layers, leading L axis), and are repacked by the library into
 *    kernel-ready device buffers owned by the handle.
 *  - vp_forward never allocates, never synchronises: all activations live in the caller's
 *    workspace (size from vp_workspace_bytes); the call is asynchronous on `stream` and
 *    can be captured into a hipGraph.
 *  - A workspace is scratch: for every entry point that takes one, the bytes its *_workspace_bytes reports for the
 *    same arguments are enough (the call writes nothing outside [workspace, workspace + bytes) and refuses a shorter
 *    one with VP_EINVAL before its first launch), and no output bit depends on what the workspace held on entry.
 *  - A handle is bound to one device and is not thread-safe: calls on one handle must not overlap
 *    (in particular vp_prepare_geometry / vp_prepare_frames, which add to the handle's cached tables,
 *    must not run while vp_forward runs on the same handle).  Different handles -- on one device or
 *    several -- may be driven from different host threads at once: the library's launch state (kernel
 *    attributes, CU counts) is kept per device and set under a lock.
 */
#ifndef VIDEOPRISM_HIP_H_
#define VIDEOPRISM_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VP_ABI_VERSION 8

typedef struct vp_handle vp_handle;

enum vp_status {
  VP_OK = 0,
  VP_EINVAL = 1,   /* bad argument / shape (reference ValueError / assert) */
  VP_ENOMEM = 2,   /* device allocation failed */
  VP_EHIP = 3,     /* HIP runtime error */
  VP_ESTATE = 4,   /* handle not finalized / parameter missing */
  VP_ENOTSUP = 5,  /* valid for the reference but outside this library's kernels */
  VP_ECOMM = 6,    /* RCCL error (vp_comm_*, vp_allgather) */
};

/* VP_U8: video frames as uint8 [0, 255], normalised in the patchify kernel exactly as
 * video_utils.py:94 (float32(v) / 255.0) -- a quarter of the fp32 input bytes. */
enum vp_dtype { VP_F32 = 0, VP_BF16 = 1, VP_U8 = 2 };

/* FactorizedEncoder hyper-parameters: models.py:83-104 CONFIGS / encoders.py:399-408. */
typedef struct vp_config {
  int32_t patch_size;          /* 18 */
  int32_t pos_emb_t;           /* pos_emb_shape[0]: 16 (Base) / 8 (Large) */
  int32_t pos_emb_h;           /* pos_emb_shape[1]: 16 */
  int32_t pos_emb_w;           /* pos_emb_shape[2]: 16 */
  int32_t model_dim;           /* 768 / 1024 / 1408 (VP_F32: a multiple of 128; VP_BF16: of 256) */
  int32_t num_spatial_layers;  /* 12 / 24 */
  int32_t num_temporal_layers; /* 4 */
  int32_t num_heads;           /* 12 / 16 (dim_per_head 64; 88 -- Giant, 1408 / 16 -- with fprop_dtype VP_F32 only) */
  int32_t mlp_dim;             /* 3072 / 4096 */
  float atten_logit_cap;       /* 50.0 */
  int32_t fprop_dtype;         /* VP_F32 (reference default) or VP_BF16 (get_model(fprop_dtype=bf16)) */
} vp_config;

/* Last error message of the calling thread ("" if none). */
const char* vp_last_error(void);
int vp_abi_version(void);

/* Replaces models.get_model(...) (models.py:268-303): binds a config to a device. */
int vp_create(const vp_config* cfg, int device, vp_handle** out);
int vp_destroy(vp_handle* h);

/* One parameter leaf, by its Flax path under 'params' ('/'-joined, utils.py:84-105), e.g.
 *   "patch_projection/linear/kernel"                                    [P*P*3, D]
 *   "spatial_encoder/transformers_stack/x_layers/self_attention/query/w" [L, D, N, H]
 * host_data: fp32, C-contiguous.  Shapes are validated against the config. */
int vp_set_param(vp_handle* h, const char* name, const float* host_data, const int64_t* shape,
                 int ndim);
/* Number of leaves the config expects (40 for a scanned FactorizedEncoder,
 * encoders_test.py:170) and the i-th leaf's name. */
int vp_param_count(const vp_handle* h, int* count);
int vp_param_name(const vp_handle* h, int index, const char** name);
/* Validates that every leaf was set and uploads the packed weights (one-off). */
int vp_finalize(vp_handle* h);

/* Frames whose patch grid (H/P, W/P) differs from pos_emb_shape[1:]: interpolates the spatial
 * positional table the way encoders.py:497-512 does (_interpolate_emb_2d, jax.image.resize
 * 'bilinear', antialiased when shrinking) and caches it on the device (allocates; call once per
 * new frame size before vp_forward, which never allocates). */
int vp_prepare_geometry(vp_handle* h, int64_t H, int64_t W);

/* Clips of T frames: the temporal positional table resampled to T the way encoders.py:543-553
 * does (_interpolate_emb_1d, :107-130, jax.image.resize 'bilinear', antialiased when shrinking).
 * vp_finalize precomputes T = 1..32; any other T needs one call before vp_forward (allocates one
 * [T][D] fp32 table per distinct T, kept until vp_destroy; idempotent).  1 <= T <= 2^20. */
int vp_prepare_frames(vp_handle* h, int64_t T);

/* Workspace needed by vp_forward for inputs [B, T, H, W, 3]. */
int vp_workspace_bytes(const vp_handle* h, int64_t B, int64_t T, int64_t H, int64_t W,
                       size_t* bytes);

/* Replaces FactorizedEncoder.__call__ (encoders.py:411-456) / model.apply(..., train=False).
 *   video          device [B, T, H, W, 3], in_dtype VP_F32 or VP_BF16 (values as given) or VP_U8
 *   frame_paddings device [B, T] fp32 (1 = padded frame) or NULL (encoders.py:440-447)
 *   out            device [B, T*N, D] embeddings in out_dtype (token = t*N + n, :570-572)
 *   spatial_out    device [B, T*N, D] 'spatial_features' in out_dtype, or NULL (:574-578)
 */
int vp_forward(vp_handle* h, const void* video, int in_dtype, int64_t B, int64_t T, int64_t H,
               int64_t W, const float* frame_paddings, void* out, int out_dtype,
               void* spatial_out, void* workspace, size_t ws_bytes, void* stream);

/* ---------------- sliding windows: per-frame spatial states, computed once ----------------
 * FactorizedEncoder is factorized: the spatial layers see one frame at a time (encoders.py:459-478) and a frame
 * first meets its neighbours in the transpose to (b n) t (:535).  Overlapping windows of one long video therefore
 * share the spatial half: vp_forward_spatial runs it once per frame, vp_forward_temporal runs the rest over any
 * windows of those frames.  Neither allocates or synchronises.
 *
 * A frame state is the spatial residual stream after the last spatial layer, *before* spatial_ln: [F][N][D] in the
 * handle's fprop dtype, rows (frame, patch).  It depends on its frame's pixels and padding only: not on F, on the
 * frame's place in the batch, or on any T.  vp_forward_temporal copies the windows' frames out of the states (one
 * launch) and from there runs vp_forward's own launches, the fused spatial_ln + transpose + temporal pos-emb
 * included, which makes its outputs bitwise those of vp_forward on the gathered clips.
 *
 * vp_forward_spatial replaces encoders.py:436-514 and :459-478 (tokenisation, patch projection, spatial pos-emb,
 * spatial encoder) over F frames, exactly as vp_forward does for B = F, T = 1:
 *   video          device [F, H, W, 3], in_dtype VP_F32, VP_BF16 or VP_U8
 *   frame_paddings device [F] fp32 (1 = padded frame) or NULL
 *   states_out     device [F, N, D] in the fprop dtype */
int vp_spatial_workspace_bytes(const vp_handle* h, int64_t F, int64_t H, int64_t W, size_t* bytes);
int vp_forward_spatial(vp_handle* h, const void* video, int in_dtype, int64_t F, int64_t H, int64_t W,
                       const float* frame_paddings, void* states_out, void* workspace, size_t ws_bytes,
                       void* stream);
/* vp_forward_temporal replaces encoders.py:520-578 (spatial_ln, transpose, temporal pos-emb, temporal encoder,
 * temporal_ln) over Wn windows of T frames each:
 *   states         device [F, N, D] frame states in the fprop dtype (vp_forward_spatial)
 *   frame_idx      device int32 [Wn, T]: window w's frame t is state frame_idx[w][t].  The gather kernel clamps each
 *                  index to [0, F - 1]: an index out of range is the caller's error, but no read leaves `states`
 *   frame_paddings device [Wn, T] fp32 (the frames' paddings, gathered by the caller) or NULL
 *   out            device [Wn, T*N, D] embeddings in out_dtype
 *   spatial_out    device [Wn, T*N, D] 'spatial_features' in out_dtype, or NULL
 * A T without a temporal table gives VP_ESTATE (vp_prepare_frames), as in vp_forward.  Windows are processed in
 * chunks as vp_forward's clips are. */
int vp_temporal_workspace_bytes(const vp_handle* h, int64_t Wn, int64_t T, int64_t H, int64_t W, size_t* bytes);
int vp_forward_temporal(vp_handle* h, const void* states, int64_t F, const int32_t* frame_idx, int64_t Wn,
                        int64_t T, int64_t H, int64_t W, const float* frame_paddings, void* out, int out_dtype,
                        void* spatial_out, void* workspace, size_t ws_bytes, void* stream);

/* ---------------- HIP-event profiler (bench.py's live per-kernel timing) ----------------
 * vp_profile_enable(h, n): the next n kernel launches of vp_forward are bracketed by
 * hipEventRecord on the launch stream (0 disables).  vp_profile_read syncs on the last event
 * and returns, per kernel class (vp_profile_class_name), the summed milliseconds, algorithmic
 * FLOPs and bytes and the launch count since the previous read, then resets. */
int vp_profile_enable(vp_handle* h, int capacity);
int vp_profile_read(vp_handle* h, int nclass, double* ms, double* flops, double* bytes,
                    int64_t* launches);
/* Only launches of the classes whose bit is set in class_mask get events (default: all).  Each
 * event pair costs the stream a little, so bench.py times the dominant class alone in its timed
 * region and takes the per-class breakdown from a separate profiled step. */
int vp_profile_set_mask(vp_handle* h, uint32_t class_mask);
int vp_profile_class_count(void);
int vp_profile_class_name(int cls, const char** name);
/* Demangled symbol of the kernel most recently launched for class `cls` on this handle ("" if
 * none yet), e.g. "void vp::(anonymous namespace)::gemm_bf16_w4_kernel<9, 512, 0>(...)": bench.py
 * matches PMC traffic records to exactly this kernel.  Valid until the next call for `cls`. */
int vp_profile_kernel_name(vp_handle* h, int cls, const char** name);

/* ---------------- op-level entry points (kernel parity tests, benches) ---------------- */

/* C[M,N] = A[M,K].W[N,K]^T + bias with epilogue:
 *   0 store (out dtype = precision), 1 GELU(erf) [* (1-rowpad)], 2 out_f32 = resid_f32 + (.)*(1-rowpad),
 *   3 out_f32 = (.) + pos[m % pos_rows], 4 = 2 (separate kernel symbol used for ffn_layer2),
 *   5 / 6 / 7 = 2 / 3 / 4 with a bf16 residual stream (bf16 resid and out; precision VP_BF16 only).
 *   precision VP_BF16: A,W bf16; VP_F32: A,W fp32.
 * Replaces layers.py:273-313 (Dense) and :433-499 (einsum projections). */
int vp_op_gemm(int precision, int epilogue, const void* A, int64_t lda, const void* W, int64_t ldw,
               int64_t M, int64_t N, int64_t K, void* out, int64_t ldo, const float* bias,
               const void* resid, int64_t ldr, const float* pos, int64_t pos_rows,
               const float* rowpad, void* stream);

/* Capped attention over rows qkv[num_seq*S, 3*heads*64] = [q|k|v] (q pre-scaled), writing
 * o[num_seq*S, heads*64].  Replaces DotProductAttention._dot_atten (layers.py:601-661).
 * key_pad: [num_seq*S] (1 = padded key) or NULL.  Any S >= 1 in both precisions; the kernel is the one the
 * forward runs for such a stack (one dispatch serves both), first match:
 *   VP_BF16  cap outside (0, 50] (no capping, or a cap whose unnormalised fp32 numerators could overflow):
 *              the online-softmax kernel of vp_op_attention_masked
 *            S > 256 without key_pad: the long-sequence kernel of the LvT auxiliary encoder
 *            S == 256: the spatial kernel; S <= 16: the temporal kernel; 16 < S < 256: the sequence-packed
 *              kernel; S > 256 with key_pad: the online-softmax kernel
 *   VP_F32   S <= 256: the fp32 kernel (on the MFMA for S >= 128 with 0 < cap <= 50)
 *            S > 256: the fp32 MFMA kernel for 0 < cap <= 50, else the online-softmax kernel */
int vp_op_attention(int precision, const void* qkv, void* o, int64_t num_seq, int64_t S,
                    int64_t heads, float cap, const float* key_pad, void* stream);

/* vp_op_attention over heads of dim_per_head values: rows qkv[num_seq*S, 3*heads*dim_per_head], o[num_seq*S,
 * heads*dim_per_head].  64 is vp_op_attention itself.  88 (the Giant encoder's 1408 / 16) runs in VP_F32 only,
 * on the same fp32 kernels with one boundary moved: the fp32 kernel keeps K|V of a sequence in LDS, which
 * 88-wide heads fill at S = 224, so with a cap outside (0, 50] sequences of 224 < S <= 256 take the
 * online-softmax kernel.  Any other width, and 88 in VP_BF16, is VP_ENOTSUP. */
int vp_op_attention_dh(int precision, const void* qkv, void* o, int64_t num_seq, int64_t S, int64_t heads,
                       int64_t dim_per_head, float cap, const float* key_pad, void* stream);

/* LayerNorm (layers.py:208-270) of fp32 or bf16 rows (in_dtype) of D = 128 k values (k in 1..12, or 16; else
 * VP_ENOTSUP) with gamma = 1 + scale; optional
 * row permutation (0 none, 1 (b t n)->(b n t), 2 (b n t)->(b t n)) and fp32 add[t][D] by output t. */
int vp_op_layernorm(const void* x, int in_dtype, int64_t rows, int64_t D, const float* gamma,
                    const float* beta, void* out, int out_dtype, int perm, int64_t T, int64_t Nsp,
                    const float* add, void* stream);

/* _image_to_patch (encoders.py:70-104): video [BT,H,W,C] -> patches [BT*(H/P)*(W/P), kpad]
 * with features in (p, q, c) order and zero padding from P*P*C to kpad. */
int vp_op_patchify(const void* video, int in_dtype, void* patches, int out_dtype, int64_t BT,
                   int64_t H, int64_t W, int64_t C, int64_t P, int64_t kpad, void* stream);

enum vp_resize_mode { VP_RESIZE_CENTER_CROP = 0, VP_RESIZE_STRETCH = 1 };

/* Replaces video_utils.py:76-87, 97-127 (cv2 BGR->RGB, cv2.resize INTER_LINEAR on uint8, center crop).
 *   src        device uint8: frame n, row y, pixel x, channel c at n*frame_stride + y*row_stride + 3*x + c (bytes)
 *   frame_idx  device int32 [F] (indices into the N source frames, clamped to [0, N-1]), or NULL = 0..F-1 (then F <= N)
 *   dst        device uint8 [F, S, S, 3], contiguous
 * VP_RESIZE_CENTER_CROP resizes the short side to S and keeps the centre S x S window (only the window
 * is computed); VP_RESIZE_STRETCH resizes to S x S.  swap_rb != 0 swaps channels 0 and 2.  The arithmetic
 * is cv2's 11-bit fixed point (tests/preprocess_restatement.py states it).  No handle: the call is
 * asynchronous on `stream` on the current device, never allocates and never synchronises. */
int vp_op_preprocess_frames(const uint8_t* src, int64_t N, int64_t H, int64_t W, int64_t row_stride,
                            int64_t frame_stride, const int32_t* frame_idx, int64_t F, int mode,
                            int swap_rb, int64_t S, uint8_t* dst, void* stream);

/* The same step in front of a decoder's 4:2:0 surfaces, read in place (no decoder is part of this library).
 *   VP_YUV_NV12  8-bit: a Y plane and one plane of interleaved U,V byte pairs
 *   VP_YUV_I420  8-bit: separate Y, U and V planes
 *   VP_YUV_P010  NV12's layout in little-endian 16-bit words; the 10-bit sample is word >> 6
 * The Y plane is H x W samples, the chroma planes ceil(H/2) x ceil(W/2) (pairs, when interleaved): odd H
 * and W are legal.  Plane p holds frame n, row y at plane[p] + n*frame_stride[p] + y*row_stride[p]; no
 * byte outside those rows is read.  P010 bases and strides must be multiples of 2. */
enum vp_yuv_format { VP_YUV_NV12 = 0, VP_YUV_I420 = 1, VP_YUV_P010 = 2 };
enum vp_yuv_matrix { VP_YUV_BT601 = 0, VP_YUV_BT709 = 1 };
enum vp_yuv_range  { VP_YUV_LIMITED = 0, VP_YUV_FULL = 1 };
typedef struct {
  const void* plane[3];        /* Y, UV, NULL (NV12, P010) or Y, U, V (I420): device pointers */
  int64_t row_stride[3];       /* bytes */
  int64_t frame_stride[3];     /* bytes */
  int format, matrix, range;
} vp_yuv_frames;

/* dst = vp_op_preprocess_frames applied to the full-resolution RGB frame that is never stored: each tap
 * is converted to uint8 R, G, B first, then blended.  Chroma is not interpolated: luma (y, x) uses chroma
 * sample (y >> 1, x >> 1).  The conversion is 16.16 fixed point, clamped once at the end:
 *   out = clip((cy*(Y - yoff) + cu*(U - coff) + cv*(V - coff) + 32768) >> 16, 0, 255)
 * with the coefficients of vp_dev_yuv_coefficients (tests/yuv_restatement.py states it).  N, H, W, frame_idx,
 * F, mode, S, dst (R, G, B order) and the geometry limits are vp_op_preprocess_frames'.  Asynchronous on
 * `stream` on the current device; never allocates, never synchronises; argument errors are VP_EINVAL
 * before any device call. */
int vp_op_preprocess_yuv(const vp_yuv_frames* src, int64_t N, int64_t H, int64_t W, const int32_t* frame_idx,
                         int64_t F, int mode, int64_t S, uint8_t* dst, void* stream);

/* Both calls with the geometry per output frame (multi-view evaluation, crop and flip augmentation).
 *   views      device int32 [V, 9]: rows box_y, box_x, box_h, box_w, new_h, new_w, win_y, win_x, flags
 *   frame_idx  device int32 [V*T] (clamped to [0, N-1]), or NULL = frame t of every view is source frame t (then T <= N)
 *   dst        device uint8 [V*T, S, S, 3], contiguous; frame v*T + t belongs to view v
 * With img the source frame (for YUV the full-resolution RGB frame that is never stored), a view's picture is
 *   out = cv2.resize(img[box_y:box_y+box_h, box_x:box_x+box_w], (new_w, new_h))[win_y:win_y+S, win_x:win_x+S]
 *   out = out[:, ::-1] if flags & 1        (horizontal mirror; the other bits of flags must be 0)
 * in the arithmetic of vp_op_preprocess_frames: the taps clamp at the box's edges, not the frame's, and an
 * axis scale is the double 1.0 / ((double)new_w / (double)box_w), so the whole frame with the centre-crop
 * geometry gives vp_op_preprocess_frames' bits.  For YUV a tap at box-relative (y, x) is the luma sample
 * (box_y + y, box_x + x) with the chroma sample ((box_y + y) >> 1, (box_x + x) >> 1).
 * The table is never read on the host.  The kernel clamps each row, so that no table causes a read outside the
 * frames, and a valid row passes unchanged: box_y to [0, H-1], box_h to [1, H-box_y] (x likewise), new_h and
 * new_w to [S, 2^24-1], win_y to [0, new_h-S] and win_x to [0, new_w-S].
 * The size limits are vp_op_preprocess_frames' with F = V*T.  Asynchronous on `stream` on the current device;
 * never allocates, never synchronises; argument errors are VP_EINVAL before any device call. */
int vp_op_preprocess_views(const uint8_t* src, int64_t N, int64_t H, int64_t W, int64_t row_stride,
                           int64_t frame_stride, const int32_t* frame_idx, const int32_t* views, int64_t V,
                           int64_t T, int swap_rb, int64_t S, uint8_t* dst, void* stream);
int vp_op_preprocess_yuv_views(const vp_yuv_frames* src, int64_t N, int64_t H, int64_t W, const int32_t* frame_idx,
                               const int32_t* views, int64_t V, int64_t T, int64_t S, uint8_t* dst, void* stream);

/* The integer table vp_op_preprocess_yuv uses: out[0..8] = rows R, G, B x (cy, cu, cv), each
 * floor(x * 65536 + 0.5) of the real coefficient, out[9] = yoff, out[10] = coff; bit_depth 8 or 10.
 * No device needed. */
int vp_dev_yuv_coefficients(int matrix, int range, int bit_depth, int32_t out[11]);

/* Build-defined pooled clip embedding used by the multi-GPU gather (the video-only encoder
 * has no pooler in the reference): out[b] = l2norm(mean_l emb[b, l, :]) in fp32, with the
 * reference's _l2_normalize (encoders.py:50-67, eps 1e-12). */
int vp_op_pool_l2(const void* emb, int dtype, int64_t B, int64_t L, int64_t D, float* out,
                  void* stream);

/* Attention over rows qkv[num_seq*S, 3*heads*64] (q pre-scaled), any S, with key paddings
 * key_pad [num_seq*S] (nullable) and, if causal, the merged causal + padding mask of
 * layers.py:111-179 (a padded query row is fully masked -> uniform weights).  qkv / o in
 * `precision` (VP_F32 or VP_BF16).  cap <= 0 disables the tanh cap.  Used by the text tower: bf16
 * with 16 < S <= 256 and 0 < cap <= 50 on the sequence-packed MFMA kernel, otherwise fp32 math with an
 * online softmax. */
int vp_op_attention_masked(int precision, const void* qkv, void* o, int64_t num_seq, int64_t S,
                           int64_t heads, float cap, const float* key_pad, int causal, void* stream);

/* vp_op_attention_masked over heads of dim_per_head values (64, or 88 in VP_F32; else VP_ENOTSUP). */
int vp_op_attention_masked_dh(int precision, const void* qkv, void* o, int64_t num_seq, int64_t S, int64_t heads,
                              int64_t dim_per_head, float cap, const float* key_pad, int causal, void* stream);

/* video_emb [B, D] . text_emb [Q, D]^T -> out [B, Q] (fp32): the video-text similarity of the
 * LvT models (README / colab usage of FactorizedVideoCLIP's embeddings).  One workgroup per (video, text) pair:
 * meant for a batch's [B, Q] matrix; to search a gallery of embeddings use vp_op_topk below. */
int vp_op_similarity(const float* video_emb, const float* text_emb, int64_t B, int64_t Q, int64_t D,
                     float* out, void* stream);

/* ---------------- LvT video-text model: FactorizedVideoCLIP (encoders.py:762-910) ----------------
 * Replaces models.get_model('videoprism_lvt_public_v1_{base,large}') + model.apply(variables,
 * inputs, text_token_ids, text_paddings, train=False, normalize, return_intermediate,
 * frame_paddings) (models.py:116-212, 268-303).  Parameters are the Flax leaves under 'params':
 * 'vision_encoder/...' (the FactorizedEncoder leaves above), 'auxiliary_encoder/...',
 * 'contrastive_vision_pooler/...', 'text_encoder/...' (88 leaves for a scanned model,
 * encoders_test.py:339; 92 with norm_policy 1).  model_dim: a multiple of 128 up to 1536 (the pooler
 * kernels' range, VP_ENOTSUP past it), so videoprism_lvt_v1_giant (1408) runs with VP_F32; with VP_BF16 Giant's
 * widths get vp_create's dim_per_head refusal.  Same conventions as vp_handle (borrowed device pointers, async on
 * `stream`, no allocation in the encode calls, one device per handle, not thread-safe). */
typedef struct vp_clip vp_clip;

typedef struct vp_clip_config {
  vp_config video;               /* vision encoder hyper-parameters (models.py:116-145) */
  int32_t num_auxiliary_layers;  /* 2: VisionTransformer over all T*N tokens (:846-857) */
  int32_t vocabulary_size;       /* 32000 (c4_en, models.py:55-60) */
  int32_t num_unimodal_layers;   /* 12: text tower depth */
  int32_t enable_causal_atten;   /* 1 */
  int32_t norm_policy;           /* text tower only (encoders.py:899; the vision and auxiliary stacks are always
                                  * 'pre'): 0 'pre', 1 'primer_hybrid' (videoprism_lvt_v1_giant: a LayerNorm before
                                  * and after each sublayer, layers.py:388-430, :819-860; the scanned text stack
                                  * then has 20 leaves, pre_layer_norm / post_layer_norm in place of layer_norm);
                                  * any other value: VP_ENOTSUP */
} vp_clip_config;

int vp_clip_create(const vp_clip_config* cfg, int device, vp_clip** out);
int vp_clip_destroy(vp_clip* c);
int vp_clip_set_param(vp_clip* c, const char* name, const float* host_data, const int64_t* shape,
                      int ndim);
int vp_clip_param_count(const vp_clip* c, int* count);
int vp_clip_param_name(const vp_clip* c, int index, const char** name);
int vp_clip_finalize(vp_clip* c);
/* The vision tower's vp_handle (owned by the clip): vp_profile_* on it also covers the
 * auxiliary encoder and pooler launches of vp_clip_encode_video. */
int vp_clip_video_handle(vp_clip* c, vp_handle** video);

/* Video side of FactorizedVideoCLIP.__call__ (encoders.py:833-885):
 *   video_emb      device [B, D] fp32: contrastive_vision_pooler(auxiliary_encoder(features)),
 *                  L2-normalised if `normalize` (:859-872)
 *   frame_emb      device [B, T, D] fp32 'frame_embeddings' (pooler per frame, :874-885) or NULL
 *   spatial_out    device [B, T*N, D] 'spatial_features' in out_dtype, or NULL
 *   spatiotemporal_out device [B, T*N, D] 'spatiotemporal_features' (the vision encoder's output,
 *                  :844-845) in the handle's fprop dtype (out_dtype must match), or NULL */
int vp_clip_video_workspace_bytes(const vp_clip* c, int64_t B, int64_t T, int64_t H, int64_t W,
                                  size_t* bytes);
int vp_clip_encode_video(vp_clip* c, const void* video, int in_dtype, int64_t B, int64_t T,
                         int64_t H, int64_t W, const float* frame_paddings, int normalize,
                         float* video_emb, float* frame_emb, void* spatial_out,
                         void* spatiotemporal_out, int out_dtype, void* workspace,
                         size_t ws_bytes, void* stream);

/* vp_clip_encode_video over Wn windows of T frames of the vision tower's frame states (vp_forward_spatial on
 * vp_clip_video_handle; states, F, frame_idx and frame_paddings as in vp_forward_temporal): the vision features
 * (encoders.py:833-845) come from vp_forward_temporal, everything after them is vp_clip_encode_video's.  Outputs
 * are indexed by window where vp_clip_encode_video's are by clip. */
int vp_clip_video_windows_workspace_bytes(const vp_clip* c, int64_t Wn, int64_t T, int64_t H, int64_t W,
                                          size_t* bytes);
int vp_clip_encode_video_windows(vp_clip* c, const void* states, int64_t F, const int32_t* frame_idx, int64_t Wn,
                                 int64_t T, int64_t H, int64_t W, const float* frame_paddings, int normalize,
                                 float* video_emb, float* frame_emb, void* spatial_out, void* spatiotemporal_out,
                                 int out_dtype, void* workspace, size_t ws_bytes, void* stream);

/* Text side (encoders.py:887-908): ids device int32 [Q, L], paddings device fp32 [Q, L]
 * (1 = padded token); text_emb device [Q, D] fp32 = the CLS token after unimodal_ln,
 * L2-normalised if `normalize`.  Out-of-range ids are clamped (JAX gather semantics). */
int vp_clip_text_workspace_bytes(const vp_clip* c, int64_t Q, int64_t L, size_t* bytes);
int vp_clip_encode_text(vp_clip* c, const int32_t* ids, const float* paddings, int64_t Q,
                        int64_t L, int normalize, float* text_emb, void* workspace,
                        size_t ws_bytes, void* stream);

/* ---------------- video classifier: FactorizedVideoClassifier (encoders.py:583-653) ----------------
 * Replaces encoders.FactorizedVideoClassifier(encoder_params, num_classes).apply(...) and the
 * models.videoprism_vc_v1_{base,large}(num_classes) builders (models.py:195-216).  Leaves:
 * 'encoder/...' (the FactorizedEncoder leaves), 'atten_pooler/...' (AttenTokenPoolingLayer with
 * hidden D, 12 leaves), 'projection/linear/{kernel [D, C], bias [C]}': 54 in all
 * (encoders_test.py:224).
 *   logits      device [B, num_classes] fp32
 *   embeddings  device [B, D] fp32 'global_embeddings' (the pooled vector) or NULL
 *   spatial_out / spatiotemporal_out as vp_clip_encode_video */
typedef struct vp_classifier vp_classifier;
int vp_classifier_create(const vp_config* cfg, int num_classes, int device, vp_classifier** out);
int vp_classifier_destroy(vp_classifier* c);
int vp_classifier_set_param(vp_classifier* c, const char* name, const float* host_data,
                            const int64_t* shape, int ndim);
int vp_classifier_param_count(const vp_classifier* c, int* count);
int vp_classifier_param_name(const vp_classifier* c, int index, const char** name);
int vp_classifier_finalize(vp_classifier* c);
int vp_classifier_video_handle(vp_classifier* c, vp_handle** video);
int vp_classifier_workspace_bytes(const vp_classifier* c, int64_t B, int64_t T, int64_t H, int64_t W,
                                  size_t* bytes);
int vp_classifier_forward(vp_classifier* c, const void* video, int in_dtype, int64_t B, int64_t T,
                          int64_t H, int64_t W, const float* frame_paddings, float* logits,
                          float* embeddings, void* spatial_out, void* spatiotemporal_out,
                          int out_dtype, void* workspace, size_t ws_bytes, void* stream);

/* vp_classifier_forward over Wn windows of T frames of the encoder's frame states (vp_forward_spatial on
 * vp_classifier_video_handle; arguments as in vp_forward_temporal): the features of encoders.py:621-630 come from
 * vp_forward_temporal, the pooler and projection are vp_classifier_forward's. */
int vp_classifier_windows_workspace_bytes(const vp_classifier* c, int64_t Wn, int64_t T, int64_t H, int64_t W,
                                          size_t* bytes);
int vp_classifier_forward_windows(vp_classifier* c, const void* states, int64_t F, const int32_t* frame_idx,
                                  int64_t Wn, int64_t T, int64_t H, int64_t W, const float* frame_paddings,
                                  float* logits, float* embeddings, void* spatial_out, void* spatiotemporal_out,
                                  int out_dtype, void* workspace, size_t ws_bytes, void* stream);

/* ---------------- training the classifier's head on frozen tokens ----------------
 * The head of FactorizedVideoClassifier (encoders.py:634-652: atten_pooler, then projection) has no released
 * weights; VideoPrism is evaluated with a frozen backbone and a trained attentive probe.  These stateless ops are
 * the head's forward and backward over tokens [B, S, D] (the encoder's 'spatiotemporal_features', VP_F32 or
 * VP_BF16) that take no gradient.  Parameters and gradients are DEVICE fp32 arrays in the reference's own layouts;
 * dims: model_dim % 128 == 0, at most 1536, a multiple of num_heads <= 16 (else VP_ENOTSUP).  The calls are
 * asynchronous on `stream` on the current device, never allocate and never synchronise.
 *   vp_op_probe_forward   logits [B, C] fp32; emb [B, D] fp32 (the pooled embedding) or NULL.  Leaves in `ws` what
 *                         the backward needs.
 *   vp_op_probe_backward  dlogits [B, C] fp32 -> every member of `grads` (all required; key_b's gradient is
 *                         exactly zero: the key bias cancels in the softmax).  `ws` is the workspace the forward
 *                         of the same params, tokens, B and S filled; it may be called more than once on it.
 * Equal inputs give equal bits: no sum is formed with atomics.  The tokens are read twice by each call.
 *
 * Token paddings (vp_op_probe_forward_masked / vp_op_probe_backward_masked): `paddings` is a DEVICE fp32 [B, S], a
 * token is padded iff its value is > 0.5 (AttenTokenPoolingLayer's `paddings`, layers.py:1103-1106), in any pattern,
 * so clips of different lengths share one batch.  A padded token's logit becomes -0.7 * FLT_MAX in every head before
 * the fp32 softmax.  In a clip with a valid token its probability is exactly 0, its row of `tokens` is never read
 * (it may hold NaN or Inf) and it adds nothing to any gradient; a streaming pass costs about what the valid tokens
 * cost.  In a clip whose tokens are all padded the softmax is uniform over all S tokens, as the reference computes
 * it: every token counts in the embedding, and the key and query leaves get nothing from that clip (its logits are
 * constants).  NULL paddings are exactly the unmasked call: the same kernels, the same bits.  The
 * backward takes the paddings its forward took.  Workspace (vp_op_probe_workspace_bytes), stream and determinism are
 * those of the unmasked calls. */
typedef struct vp_probe_dims {
  int32_t model_dim;   /* D */
  int32_t num_heads;   /* H; dim_per_head dh = D / H */
  int32_t num_classes; /* C */
} vp_probe_dims;

typedef struct vp_probe_params {           /* leaf under 'params' */
  const float* query;                      /* atten_pooler/pooling_attention_query [1, D] */
  const float* per_dim_scale;              /* atten_pooler/pooling_attention/per_dim_scale/per_dim_scale [dh] */
  const float *query_w, *query_b;          /* .../pooling_attention/query/{w [D, H, dh], b [H, dh]} */
  const float *key_w, *key_b;              /* .../key/{w, b} */
  const float *value_w, *value_b;          /* .../value/{w, b} */
  const float *post_w, *post_b;            /* .../post/{w [D, H, dh], b [D]} */
  const float *ln_scale, *ln_bias;         /* atten_pooler/pooling_attention_layer_norm/{scale, bias} [D] */
  const float *proj_kernel, *proj_bias;    /* projection/linear/{kernel [D, C], bias [C]} */
} vp_probe_params;

typedef struct vp_probe_grads { /* member for member the gradient of vp_probe_params, same shapes */
  float* query;
  float* per_dim_scale;
  float *query_w, *query_b;
  float *key_w, *key_b;
  float *value_w, *value_b;
  float *post_w, *post_b;
  float *ln_scale, *ln_bias;
  float *proj_kernel, *proj_bias;
} vp_probe_grads;

int vp_op_probe_workspace_bytes(const vp_probe_dims* dims, int64_t B, int64_t S, size_t* bytes);
int vp_op_probe_forward(const vp_probe_dims* dims, const vp_probe_params* params, const void* tokens, int dtype,
                        int64_t B, int64_t S, float* logits, float* emb, void* ws, size_t ws_bytes, void* stream);
int vp_op_probe_backward(const vp_probe_dims* dims, const vp_probe_params* params, const void* tokens, int dtype,
                         int64_t B, int64_t S, const float* dlogits, const vp_probe_grads* grads, void* ws,
                         size_t ws_bytes, void* stream);
int vp_op_probe_forward_masked(const vp_probe_dims* dims, const vp_probe_params* params, const void* tokens, int dtype,
                               int64_t B, int64_t S, const float* paddings, float* logits, float* emb, void* ws,
                               size_t ws_bytes, void* stream);
int vp_op_probe_backward_masked(const vp_probe_dims* dims, const vp_probe_params* params, const void* tokens,
                                int dtype, int64_t B, int64_t S, const float* paddings, const float* dlogits,
                                const vp_probe_grads* grads, void* ws, size_t ws_bytes, void* stream);

/* ---------------- gallery search: fused scores and top-k ----------------
 * The retrieval step of the LvT models: for each query, the k gallery rows with the largest dot product.  Exact and
 * deterministic; the [N, Q] score matrix is never formed, the gallery is read once per group of 32 queries (16 where
 * D > 1024 or k is large), and a score depends on the two vectors alone (not on N, Q, ld, the row's position or the
 * grid), so a gallery searched in shards and merged gives the bits of the whole search.  Stateless and asynchronous on
 * `stream`: no allocation, no synchronisation.
 *   queries  device fp32 [Q, D], contiguous, 16-byte aligned
 *   gallery  device [N, D] with row stride ld elements (ld >= D, a multiple of 8), VP_F32 or VP_BF16, 16-byte aligned.
 *            VP_F32: exact fp32 products and sums.  VP_BF16: each query enters as two bf16 terms, so the stored
 *            gallery's rounding is the only quantisation.  D % 64 == 0, D <= 1536; k <= 128
 *   scores [Q, k] fp32, ids [Q, k] = id_base + row: score descending, equal scores by ascending id.  A row that scores
 *            NaN or -inf is never returned; with fewer than k rows the tail is (-inf, -1).  Q == 0 launches nothing.
 *   ws       vp_op_topk_workspace_bytes(Q, k) bytes (no device needed: the number of row ranges has a fixed bound)
 * vp_op_topk_merge: the best k <= k_in (<= 128) per query of `parts` lists scores_in / ids_in [parts, Q, k_in], each
 * in the order above (ids < 0 are padding): the step after per-shard searches with each shard's id_base. */
int vp_op_topk_workspace_bytes(int64_t Q, int64_t k, size_t* bytes);
int vp_op_topk(const float* queries, int64_t Q, const void* gallery, int gallery_dtype, int64_t N, int64_t ld, int64_t D,
               int64_t k, int64_t id_base, float* scores, int64_t* ids, void* ws, size_t ws_bytes, void* stream);
int vp_op_topk_merge(const float* scores_in, const int64_t* ids_in, int64_t parts, int64_t Q, int64_t k_in, int64_t k,
                     float* scores, int64_t* ids, void* stream);

/* ---------------- grouped gallery search: the k best groups, each with its best row ----------------
 * Several gallery rows may stand for one thing (the windows of a video, the views of a clip, the prompts of a class):
 * labels[r] (device int64 [N], 8-byte aligned) names row r's group.  A group's score is the largest score of its rows
 * and its best row is the row with that score, of equal scores the one with the smallest id.  The result lists the k
 * best groups per query, score descending and equal scores by ascending id of the best row:
 *   scores [Q, k] fp32, groups [Q, k] int64, ids [Q, k] int64 = id_base + best row; with fewer than k groups the tail
 *   is (-inf, -1, -1).  A row that scores NaN or -inf, or whose label is negative, is never returned and never stands
 *   for a group: a negative label blanks a row out.  Labels are arbitrary non-negative int64 (not dense, not sorted).
 * The selection happens in the scan's lists (one entry per group), so the result is exact for every k <= 128 however
 * many rows a group has.  Everything else is vp_op_topk's: the same scores bit for bit, the same limits on D, ld, k and
 * the dtypes, stateless, asynchronous on `stream`, Q == 0 launches nothing, N == 0 gives all padding (labels may then
 * be null).  The lists hold 16 B an entry, so a workgroup takes 32 queries only up to k = 63 at D = 1024.
 *   ws       vp_op_topk_groups_workspace_bytes(Q, k) bytes (no device needed)
 * vp_op_topk_groups_merge: the best k <= k_in (<= 128) groups per query of `parts` lists [parts, Q, k_in] as the search
 * writes them (sorted, one entry per group, ids < 0 are padding).  Two lists may hold the same group (groups may span
 * shards): of a group's entries the one that comes first in the order stays.  The result depends on the set of
 * (score, group, id) alone, so shards searched with their id_base and label slices merge to the bits of the whole. */
int vp_op_topk_groups_workspace_bytes(int64_t Q, int64_t k, size_t* bytes);
int vp_op_topk_groups(const float* queries, int64_t Q, const void* gallery, int gallery_dtype, int64_t N, int64_t ld,
                      int64_t D, const int64_t* labels, int64_t k, int64_t id_base, float* scores, int64_t* groups,
                      int64_t* ids, void* ws, size_t ws_bytes, void* stream);
int vp_op_topk_groups_merge(const float* scores_in, const int64_t* groups_in, const int64_t* ids_in, int64_t parts,
                            int64_t Q, int64_t k_in, int64_t k, float* scores, int64_t* groups, int64_t* ids,
                            void* stream);

/* ---------------- masked gallery search: a subset of the rows, and deleted rows ----------------
 * One bit per gallery row decides, inside the scan, whether the row may enter a query's list: the two searches above
 * over the allowed rows only.  The mask is packed bits in device uint32 words, 4-byte aligned: row r is allowed where
 * bit r & 31 of word r >> 5 is set.  A mask is ceil(N / 32) words; the spare bits of its last word are ignored
 * whatever they hold and nothing past those words is read.
 *   mask, mask_query_stride_words   stride 0: one mask [ceil(N / 32)] for all queries.  Otherwise query q's mask
 *            starts at word q * stride (stride >= ceil(N / 32)): each query searches its own subset.
 * The result is the best k of the allowed rows (groups: of the groups that have an allowed row, each with its best
 * allowed row), in the order and with the padding of the unmasked calls.  An allowed row's score has the bits the
 * unmasked search gives it, so the call returns what vp_op_topk / vp_op_topk_groups return on a gallery that holds the
 * allowed rows alone, ids mapped back, and masked shard lists merge with vp_op_topk_merge / vp_op_topk_groups_merge
 * to the bits of the whole gallery's masked search.  Rows that are not allowed may or may not be read; what they hold
 * (NaN, inf) does not matter.  Groups of 64 rows that no query of a workgroup allows cost neither loads nor MFMAs,
 * and the 512-row tiles are dealt to the workgroups in turn, so long runs of such rows shorten the whole search.
 * N < 2^32 - 1.  Everything else is the unmasked call's: limits, dtypes, alignment, stateless, asynchronous on `stream` with no
 * synchronisation and no launch elsewhere, Q == 0 launches nothing, N == 0 gives all padding (the mask may then be
 * null).  A null mask with N > 0 is VP_EINVAL: the unmasked call is the one for that.
 *   ws       the unmasked call's: vp_op_topk_workspace_bytes(Q, k) for vp_op_topk_masked,
 *            vp_op_topk_groups_workspace_bytes(Q, k) for vp_op_topk_groups_masked
 * vp_op_rowmask_pack: the words from one byte per row.  allow is device uint8 (or bool) [Q, N], contiguous, nonzero =
 * allowed; out[q * stride + w] (stride >= ceil(N / 32) words) gets the bits of rows 32 w .. 32 w + 31 of allow[q], zero
 * past N, ANDed with and_words[q * and_stride + w] where and_words is not null (and_stride 0: the same packed mask
 * for every q; else >= ceil(N / 32)): a caller's filter and a mask of rows not deleted combine in the one call.  Only
 * words that hold a row are written.  Q == 0 or N == 0 launches nothing. */
int vp_op_rowmask_pack(const uint8_t* allow, int64_t Q, int64_t N, const uint32_t* and_words, int64_t and_stride,
                       uint32_t* out_words, int64_t stride, void* stream);
int vp_op_topk_masked(const float* queries, int64_t Q, const void* gallery, int gallery_dtype, int64_t N, int64_t ld,
                      int64_t D, int64_t k, int64_t id_base, const uint32_t* mask, int64_t mask_query_stride_words,
                      float* scores, int64_t* ids, void* ws, size_t ws_bytes, void* stream);
int vp_op_topk_groups_masked(const float* queries, int64_t Q, const void* gallery, int gallery_dtype, int64_t N,
                             int64_t ld, int64_t D, const int64_t* labels, int64_t k, int64_t id_base,
                             const uint32_t* mask, int64_t mask_query_stride_words, float* scores, int64_t* groups,
                             int64_t* ids, void* ws, size_t ws_bytes, void* stream);

/* ---------------- fp8 gallery: rows quantised once, decoded in the search ----------------
 * An opt-in storage format of half bf16's width: D + 4 bytes a row (772 B at D = 768 against 1536 B), so a card holds
 * twice the rows and a search reads half the bytes.  Row r is stored as D codes in OCP e4m3 (torch.float8_e4m3fn: bias
 * 7, largest finite 448, subnormals down to 2^-9, NaN 0x7f / 0xff, no infinity; gfx950's fp8, not gfx942's fnuz) and one
 * fp32 scale, and stands for codes[r, :] * scales[r].  The scale MUST be a power of two (2^-100 .. 2^100): every stored
 * value is then exactly a bf16, the search decodes it exactly and runs the VP_BF16 arithmetic on it (queries as two bf16
 * terms), so the storage rounding is the only quantisation and a score depends on the two vectors alone, as above.
 * vp_op_quantize_rows_f8 makes no other scales; what a search returns with another scale is unspecified.
 * What the rounding costs (unit-norm random rows, the hard case): score error about 4e-3 max / 1e-3 rms at D = 768
 * (bf16: 3e-4 max), recall@10 against the exact search about 0.95; DESIGN.md §4 "fp8 gallery" has the table.
 * vp_op_quantize_rows_f8: x device fp32 or bf16 (x_dtype VP_F32 / VP_BF16) [N, D] with row stride ldx elements (ldx >= D,
 *   rows 16-byte aligned: x 16-byte aligned, ldx a multiple of 4 (fp32) or 8 (bf16)) -> codes [N, D] with row stride
 *   ldc bytes (ldc >= D, a multiple of 16; 16-byte aligned) and scales [N].  Per row: amax the largest magnitude of
 *   its finite elements, e the largest integer with amax * 2^e <= 448 clamped to [-100, 100] (0 for a row with no
 *   finite nonzero element), code = round-to-nearest-even e4m3 of x * 2^e (it never saturates), scale = 2^-e.  A NaN or
 *   infinite element becomes the NaN code.  Bytes of codes past column D and everything past row N keep what they
 *   held.  N == 0 launches nothing.
 * vp_op_topk_f8 / _groups_f8 / _masked_f8 / _groups_masked_f8: the four searches above, argument for argument, with
 *   `codes, scales` in place of `gallery, gallery_dtype` and ld in bytes (ld >= D, a multiple of 16; codes 16-byte
 *   aligned, scales 4-byte aligned).  Same limits (D % 64 == 0, D <= 1536, k <= 128, the N bounds), same order, padding,
 *   merges (vp_op_topk_merge / vp_op_topk_groups_merge) and workspaces (vp_op_topk_workspace_bytes /
 *   vp_op_topk_groups_workspace_bytes); stateless, no allocation, no synchronisation, every launch on `stream`; Q == 0
 *   launches nothing, N == 0 gives all padding (codes, scales, labels and mask may then be null).  Neither codes past
 *   column D or row N nor scales past row N are read.
 *   A row that holds a NaN code scores NaN and is never returned.  A VP_BF16 gallery can return a row that scores
 *   +inf; an fp8 gallery cannot hold an infinity, and a row quantised from one has the NaN code there.
 * The four calls above keep refusing every gallery_dtype but VP_F32 and VP_BF16. */
int vp_op_quantize_rows_f8(const void* x, int x_dtype, int64_t N, int64_t ldx, int64_t D, uint8_t* codes, int64_t ldc,
                           float* scales, void* stream);
int vp_op_topk_f8(const float* queries, int64_t Q, const uint8_t* codes, const float* scales, int64_t N, int64_t ld,
                  int64_t D, int64_t k, int64_t id_base, float* scores, int64_t* ids, void* ws, size_t ws_bytes,
                  void* stream);
int vp_op_topk_groups_f8(const float* queries, int64_t Q, const uint8_t* codes, const float* scales, int64_t N,
                         int64_t ld, int64_t D, const int64_t* labels, int64_t k, int64_t id_base, float* scores,
                         int64_t* groups, int64_t* ids, void* ws, size_t ws_bytes, void* stream);
int vp_op_topk_masked_f8(const float* queries, int64_t Q, const uint8_t* codes, const float* scales, int64_t N,
                         int64_t ld, int64_t D, int64_t k, int64_t id_base, const uint32_t* mask,
                         int64_t mask_query_stride_words, float* scores, int64_t* ids, void* ws, size_t ws_bytes,
                         void* stream);
int vp_op_topk_groups_masked_f8(const float* queries, int64_t Q, const uint8_t* codes, const float* scales, int64_t N,
                                int64_t ld, int64_t D, const int64_t* labels, int64_t k, int64_t id_base,
                                const uint32_t* mask, int64_t mask_query_stride_words, float* scores, int64_t* groups,
                                int64_t* ids, void* ws, size_t ws_bytes, void* stream);

/* ---------------- multi-GPU: RCCL all-gather of pooled clip embeddings ----------------
 * The reference runs on one device; its video-text usage scores every clip against every query,
 * `similarities = video_emb @ text_emb.T` (README.md:81, verify_clip_models.py:84).  With clips
 * sharded by batch over one process per GPU, that step needs every rank's
 * [b, D] video embeddings on every rank: one all-gather over xGMI.  The communicator is RCCL's:
 * rank 0 creates a unique id (vp_comm_unique_id, vp_comm_id_bytes() bytes), the host sends it to
 * every rank by any channel (videoprism/distributed.py uses torch.distributed), and every rank
 * calls vp_comm_init with it (collective: blocks until all nranks joined).
 * vp_allgather: recv[r*count .. (r+1)*count) = rank r's send[0 .. count) on every rank, dtype
 * VP_F32 / VP_BF16 / VP_U8, asynchronous on `stream` (device pointers of the comm's device).
 * `count` must be the same on every rank (RCCL's contract): hosts with uneven shards pad to the
 * largest (videoprism/distributed.py Communicator.all_gather_rows).  Every vp_comm_* entry point
 * leaves the calling thread's current HIP device as it found it. */
typedef struct vp_comm vp_comm;
int vp_comm_id_bytes(void);
int vp_comm_unique_id(uint8_t* id_out, int64_t nbytes);
int vp_comm_init(const uint8_t* id, int64_t nbytes, int nranks, int rank, int device, vp_comm** out);
int vp_comm_destroy(vp_comm* c);
int vp_allgather(vp_comm* c, const void* send, void* recv, int64_t count, int dtype, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* VIDEOPRISM_HIP_H_ */
