// Internal (C++) launch interface of the HIP kernels.  The public C-ABI lives in
// include/videoprism_hip.h and is implemented in vp_abi.cpp on top of these.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace vp {

typedef uint16_t bf16_t;

// host function of the kernel most recently launched by this thread through the launchers below
// (vp_profile_kernel_name names the kernel behind each profiled class, so bench.py can match the
// PMC traffic of exactly that kernel symbol)
extern thread_local const void* g_last_kernel;
#define VP_NOTE_KERNEL(fn) (::vp::g_last_kernel = reinterpret_cast<const void*>(fn))

enum Epilogue {
  EPI_BF16 = 0,       // out_bf16 = acc + bias                       (fused q|k|v projection)
  EPI_GELU_BF16 = 1,  // out_bf16 = gelu(acc + bias) * (1 - rowpad)  (ffn_layer1)
  EPI_RESID_F32 = 2,  // out_f32  = resid + (acc + bias) * (1 - rowpad)   (post, ffn_layer2)
  EPI_POS_F32 = 3,    // out_f32  = acc + bias + pos[m % pos_rows]   (patch_projection + pos emb)
  EPI_RESID_FFN = 4,  // = EPI_RESID_F32, separate kernel symbol for ffn_layer2 (profiling)
  // bf16 residual stream (bf16 GEMM only): same as 2 / 3 / 4 with bf16 resid and output
  EPI_RESID_BF16 = 5,
  EPI_POS_BF16 = 6,
  EPI_RESID_FFN_BF16 = 7,
  // LayerNorm folded into the consuming GEMM (bf16 path): A = the raw residual stream x,
  // W' = diag(1+scale) W, bias' = b + W.beta, and per row (rstd, -mean*rstd) from ln_rs:
  //   out = rstd * acc + (-mean*rstd) * c[n] + bias'[n],   c[n] = sum_k W'[n][k]
  EPI_BF16_LN = 8,       // as EPI_BF16   (q|k|v of LN1(x))
  EPI_GELU_BF16_LN = 9,  // as EPI_GELU   (ffn_layer1 of LN2(x))
  // residual-stream producers that also emit the row statistics of the bf16 values they
  // store: per 128-column partial p = (n / 128), st_part[p][row] = (sum, sum of squares about
  // the partial mean); ln_stats_finalize() combines them into ln_rs
  EPI_RESID_BF16_ST = 10,
  EPI_RESID_FFN_BF16_ST = 11,
  EPI_POS_BF16_ST = 12,
  // ReLU FFN of the text tower (encoders.py:743): out = relu(acc + bias) * (1 - rowpad);
  // bf16 out on the bf16 GEMM, fp32 out on the fp32 GEMM
  EPI_RELU_BF16 = 13,
  // temporal self-attention (T = 16 frames, dh = 64, no key paddings) fused into the LN1-folded
  // q|k|v projection of a temporal layer (layers.py:601-661 over sequences of 16 rows, which are
  // aligned 16-row blocks of the (b n) t row order): two launches over the same A = x2
  //  EPI_QK_TATTN_LN: W rows [q_h | k_h] per head (a 256-column tile = 2 heads); the epilogue
  //    rounds q, k to bf16 (as the reference's bf16 projections), forms the 16x16 logits of every
  //    (sequence, head) on MFMA, the capped softmax in fp32, and stores the normalised probabilities
  //    in bf16 -- P^T fragments, 512 B per (sequence, head) at out + ((seq * heads + h) * 256) --
  //    instead of q and k;
  //  EPI_V_TATTN_LN: W rows = the v projection; the epilogue rounds v to bf16 and stores
  //    O = P . V (P from `resid`, the first launch's output) in v's place, so the attention output
  //    [M][D] comes out of the GEMM and q|k|v never reach HBM.
  EPI_QK_TATTN_LN = 14,
  EPI_V_TATTN_LN = 15,
  // The FFN pair with the hidden activation h in a row-blocked layout [M/16][F/32][16][32] (4-wave
  // kernel, bf16): ffn_layer1's epilogue stores straight from the accumulator layout -- a lane's
  // 8 values of one row are 8 natural columns because W1's rows (and b', c) are permuted within each
  // 32-row group on the host (W-row 16h + 4g + i holds column 8g + 4h + i), and one store
  // instruction writes one whole 1 KiB block -- so no LDS transposition; ffn_layer2 stages its A
  // K-tiles from that layout.  Bitwise the row-major pair.
  EPI_GELU_BF16_LN_BLK = 16,       // ffn_layer1 (as EPI_GELU_BF16_LN), h blocked
  EPI_RESID_FFN_BF16_ST_BLK = 17,  // ffn_layer2 (as EPI_RESID_FFN_BF16_ST), A = blocked h
  EPI_RESID_FFN_BF16_BLK = 18,     // ffn_layer2 (as EPI_RESID_FFN_BF16), A = blocked h
  // the spatial layers' q|k|v projection (as EPI_BF16_LN) into the row-blocked layout [M/16][3D/32][16][32]
  // (Wqkv / b' / c rows permuted the same way, a separate copy), read by attention_spatial_bf16(blk)
  EPI_BF16_LN_BLK = 19,
};

struct EpiArgs {
  void* out = nullptr;
  int64_t ldo = 0;
  const float* bias = nullptr;    // [N]
  const void* resid = nullptr;    // EPI_RESID_*: fp32 or bf16 by epilogue (may alias out)
  int64_t ldr = 0;
  const float* pos = nullptr;     // EPI_POS_F32: [pos_rows][N]
  int pos_rows = 1;
  const float* rowpad = nullptr;  // optional [M], 1 = padded token
  const float* ln_rs = nullptr;   // EPI_*_LN: [M][2] (rstd, -mean*rstd)
  const float* ln_c = nullptr;    // EPI_*_LN: [N] column sums of W'
  float* st_part = nullptr;       // EPI_*_ST: [N/128][M][2] partial (sum, M2) of each row
  int64_t st_rows = 0;            // EPI_*_ST: M (partial stride)
  float cap = 0.0f;               // EPI_*_TATTN_LN: logit cap (0 < cap <= 50)
  // EPI_QK_TATTN_LN: 2 log2(e) / cap and cap log2(e), the capped-exp constants (host-computed: a
  // kernel argument lives in SGPRs, the in-kernel division's result in two VGPRs across the loop)
  float cap_c1 = 0.0f, cap_c2 = 0.0f;
  int heads = 0;                  // EPI_*_TATTN_LN: heads of the whole projection (P indexing)
};

// ---- bf16 MFMA GEMM (gemm_bf16.hip) ----
const char* gemm_bf16_check(int M, int N, int K, int64_t lda, int64_t ldw);
hipError_t gemm_bf16(int epi, const bf16_t* A, int64_t lda, const bf16_t* W, int64_t ldw, int M,
                     int N, int K, const EpiArgs& ep, hipStream_t s);

// small M (the text tower, gemm_bf16_small.hip): 64 x 64 tiles, K split over 4 waves; epilogues EPI_BF16,
// EPI_GELU_BF16, EPI_RELU_BF16, EPI_RESID_F32/_FFN, EPI_RESID_BF16/_FFN_BF16; M, N % 64 == 0, K % 256 == 0
bool gemm_bf16_small_ok(int epi, int M, int N, int K, int64_t lda, int64_t ldw);
hipError_t gemm_bf16_small(int epi, const bf16_t* A, int64_t lda, const bf16_t* W, int64_t ldw, int M, int N, int K,
                           const EpiArgs& ep, hipStream_t s);
// 4-wave (one wave per SIMD, 128x128 per wave, 16x16x32 MFMA, full-line buffer_load..lds
// staging) decomposition; needs N*ldw*2 < 4 GiB (32-bit buffer offsets); an A operand past that range
// runs as consecutive row ranges (gemm_bf16_w4.hip)
hipError_t gemm_bf16_w4(int epi, const bf16_t* A, int64_t lda, const bf16_t* W, int64_t ldw, int M,
                        int N, int K, const EpiArgs& ep, hipStream_t s);
// patch embedding straight from bf16 frames (no patch tensor): video [M/256 frames]
// [16P][16P][3] (a 16x16 patch grid, so one 256-row tile is one frame), 3 <= P <= 21, epi
// EPI_POS_BF16(_ST).  W [N][video_patch_k(P) = 64 P]: patch pixel row py is K-tile py, read as cpr =
// ceil(3P/8) chunks of 8 values at value offsets min(8 j, 3P - 8) in slots j < cpr; W holds the
// patch-kernel row (py, vo + e) at column 64 py + 8 j + e except where the last chunk overlaps its
// predecessor and in the slots j >= cpr (zeros; video_patch_w packs it)
inline int video_patch_cpr(int P) { return (3 * P + 7) / 8; }
inline int video_patch_k(int P) { return 64 * P; }
// patch sizes the fused path takes: a patch pixel row (3P values) fits one 64-wide K-tile, and P is
// even so every 16-B chunk starts 4-B aligned in the frame (byte offsets 6P px + 16 j and 6P - 16 for
// the overlapping last chunk; P = 18 is the models' size).  Odd P would put chunks at 2-B offsets:
// those grids take patchify + GEMM instead
inline bool video_patch_ok(int P) { return P >= 4 && P % 2 == 0 && 3 * P <= 64; }
hipError_t gemm_bf16_w4_video(int epi, const bf16_t* video, int P, const bf16_t* W, int M, int N, const EpiArgs& ep,
                              hipStream_t s);
// N-tile group size of the persistent tile order (gemm_bf16_w4.hip; shared by the diag kernels)
int w4_ngrp(int M, int N, int K, int grid);
// picks gemm_bf16_w4 or gemm_bf16 by epilogue and shape
hipError_t gemm_bf16_auto(int epi, const bf16_t* A, int64_t lda, const bf16_t* W, int64_t ldw, int M,
                          int N, int K, const EpiArgs& ep, hipStream_t s);

// ---- fp32 GEMM for fprop_dtype=float32 (gemm_f32.hip) ----
const char* gemm_f32_check(int M, int N, int K, int64_t lda, int64_t ldw);
// version 2 (default): the 32x32x2 kernel; 1: round 1's 16x16x4 kernel (A/B through vp_dev_gemm_kernel); 3: the
// 32x32x2 kernel with two accumulation chains per output (half the chain, about 1 / sqrt(2) the rounding error)
hipError_t gemm_f32(int epi, const float* A, int64_t lda, const float* W, int64_t ldw, int M,
                    int N, int K, const EpiArgs& ep, hipStream_t s, int version = 2);

// ---- attention (attention.hip) ----
// qkv: rows of [q(D) | k(D) | v(D)], row r = seq * S + s; q pre-scaled by dh^-0.5.
// o: rows of D = heads*dh (dh = 64 unless a launcher takes it).  key_pad: optional [num_seq * S] (1 = padded key).
// blk: qkv in the row-blocked layout of EPI_BF16_LN_BLK ([M/16][3D/32][16][32])
hipError_t attention_spatial_bf16(const bf16_t* qkv, bf16_t* o, int num_seq, int heads,
                                  float cap, const float* key_pad, hipStream_t s, bool blk = false);
// 16 < S <= 256 (temporal attention of clips longer than 16 frames, other patch grids, the text tower with
// causal = 1), key paddings optional (attention.hip)
hipError_t attention_seq_bf16(const bf16_t* qkv, bf16_t* o, int num_seq, int S, int heads, float cap,
                              const float* key_pad, hipStream_t s, int causal = 0);
hipError_t attention_temporal_bf16(const bf16_t* qkv, bf16_t* o, int num_seq, int S, int heads,
                                   float cap, const float* key_pad, hipStream_t s);
// The fp32 kernels below and attention_masked's fp32 instantiation take heads of dh = 64 or 88 floats (88: the
// Giant encoder, 1408 / 16); qkv rows are then [q|k|v] of D = heads * dh each and o rows of D.  The bf16
// kernels are dh = 64 only.
// longest sequence of attention_f32's generic kernel: K|V of one (sequence, head) in LDS, 8 S dh bytes of 160 KiB
constexpr int f32_generic_max_s(int dh) { return dh <= 64 ? 256 : 224; }
// fp32, S <= 256: S >= 128 with 0 < cap <= 50 on the MFMA (attention_f32_mfma), else the generic kernel
// (S <= f32_generic_max_s(dh))
hipError_t attention_f32(const float* qkv, float* o, int num_seq, int S, int heads, float cap,
                         const float* key_pad, hipStream_t s, int dh = 64);
// fp32 on v_mfma_f32_32x32x2f32, any S, no causal mask: hipErrorNotSupported unless 0 < cap <= 50 (the
// max-free softmax), which is when the host chooses it (vp_internal.h choose_attention); attention_f32 then
// takes its generic kernel
hipError_t attention_f32_mfma(const float* qkv, float* o, int num_seq, int S, int heads, float cap,
                              const float* key_pad, hipStream_t s, int dh = 64);

// ---- elementwise / normalisation (elementwise.hip) ----
enum RowPerm { PERM_NONE = 0, PERM_BTN_TO_BNT = 1, PERM_BNT_TO_BTN = 2 };
// video [BT, H, W, C] (in_dtype 0 f32, 1 bf16, 2 uint8 normalised /255) -> patches [BT*np, kpad]
// (bf16 or f32), zero-padded K.
hipError_t patchify(const void* video, int in_dtype, void* patches, int out_is_bf16, int BT,
                    int H, int W, int C, int P, int kpad, hipStream_t s);
// LayerNorm over D = 128 k (k in 1..12 or 16) of fp32 or bf16 rows; gamma already holds (1 + scale).  Output row r goes
// to row perm(r); `add` (optional, fp32 [add_rows][D]) is added by the *output* row's t index.
// out_rs (optional): (rstd, -mean*rstd) of each stored output row (as ln_rs above), by
// output row index
hipError_t layernorm(const void* x, int in_is_bf16, int rows, int D, const float* gamma,
                     const float* beta, void* out, int out_is_bf16, int perm, int T, int Nsp,
                     const float* add, hipStream_t s, float* out_rs = nullptr);
// The frames of a batch of windows picked out of per-frame states x [nframes] of frame_bytes each (a multiple of 16,
// x and out 16-byte aligned): out frame s = x frame clamp(frame_idx[s], 0, nframes - 1), s < nslots (frame_idx: int32
// [nslots] in device memory).  The clamp is part of the contract: an index out of range is the caller's error, but no
// read leaves x.  A copy, so whatever runs on `out` gives bitwise what it gives on the gathered frames themselves.
hipError_t gather_frames(const void* x, int64_t nframes, const int32_t* frame_idx, int64_t nslots, int64_t frame_bytes,
                         void* out, hipStream_t s);
// norm_policy 'primer_hybrid' (layers.py:409-425, :846-855): xs[r] += LayerNorm(y[r] * (1 - pad[r])) in place on the
// fp32 residual stream; y fp32 or bf16 rows of D = 128 k (layernorm's widths), gamma = 1 + scale, pad optional
// [rows] (1 = padded token: the row gets xs + beta)
hipError_t layernorm_residual(const void* y, int y_is_bf16, int rows, int D, const float* gamma, const float* beta,
                              const float* pad, float* xs, hipStream_t s);
// f32 (in_dtype 0) / uint8 (2, normalised /255) frames -> bf16 frames, n values, the patchify kernels'
// per-value conversion (for the fused patch embedding)
hipError_t video_to_bf16(const void* video, int in_dtype, bf16_t* out, int64_t n, hipStream_t s);
// fp32 -> bf16 cast (weights are pre-packed on the host; this is for activations)
hipError_t cast_f32_bf16(const float* x, bf16_t* y, int64_t n, hipStream_t s);
// per-token padding vector expansion: frame_pad [B*T] -> token pads in both orders
hipError_t expand_paddings(const float* frame_pad, int B, int T, int Nsp, float* pad_btn,
                           float* pad_bnt, hipStream_t s);

// (rstd, -mean*rstd) of every row from the P partial (sum, M2) pairs of 128 columns each
// (Chan's combination), D = 128 * P, LayerNorm eps 1e-6 (layers.py:240-243)
hipError_t ln_stats_finalize(const float* st_part, int P, int64_t M, float* ln_rs, hipStream_t s);
// same statistics straight from bf16 rows [M][D] (two-pass), for tests and the op API
hipError_t ln_row_stats(const bf16_t* x, int64_t M, int D, float* ln_rs, hipStream_t s);

// ---- LvT video-text path (attention_long.hip, clip_kernels.hip) ----
// auxiliary-encoder self-attention over S = T*N tokens (S % 256 == 0), capped, no masks
hipError_t attention_long_bf16(const bf16_t* qkv, bf16_t* o, int num_seq, int S, int heads, float cap,
                               hipStream_t s);
// generic fp32-math attention (any S) with key paddings and the causal merge of layers.py:111-179; qkv / o in
// bf16 (in_is_bf16, dh 64) or fp32 (dh 64 or 88)
hipError_t attention_masked(const void* qkv, void* o, int in_is_bf16, int num_seq, int S, int heads,
                            float cap, const float* key_pad, int causal, hipStream_t s, int dh = 64);
// widest rows the pooler kernels take (pool_logits: D = 64 k; pool_softmax_wsum: D = 128 k; ln_l2_rows: any D)
constexpr int kPoolMaxD = 1536;
constexpr int kPoolMaxH = 16;  // most heads they take (a thread of the weighted sum keeps every head's sums)
// contrastive pooler: logits[g][h][s] = x[g*S+s] . U[h]; then softmax per (g,h) and
// z[g][h][:] = sum_s p x (zpart scratch: [G][pool_chunks(S)][H][D], stats [G*H][2])
// (bf16 x with Ut = [32][D] bf16 (U_hi | U_lo | 0) and S % 32 == 0: MFMA kernel)
// pad: token paddings [G][S] fp32 (padded iff > 0.5; layers.py:1103-1106) or null: a padded token's logit is
// -0.7 * FLT_MAX, and its row of x is not read unless every token of its clip is padded (pool_stream.h).  Null
// launches the kernels that have no such parameter.
hipError_t pool_logits(const void* x, int in_bf16, int64_t rows, int S, int D, const float* U, const bf16_t* Ut,
                       int H, float* logits, hipStream_t s, const float* pad = nullptr);
hipError_t pool_softmax_wsum(const void* x, int in_bf16, int G, int S, int D, int H, const float* logits,
                             float* stats, float* zpart, float* z, hipStream_t s, const float* pad = nullptr);
int pool_chunks(int S);
// out[g][e] = sum_{i < n} part[g][i][e] in index order, e < HD, g < groups (chunk sums of a weighted-sum pass)
hipError_t pool_reduce(const float* part, int n, int64_t HD, int64_t groups, float* out, hipStream_t s);
// out[b][m][n] = A[b][m][:] . Wt[b][:][n] + bias[b][n] (fp32, small M), batch strides sA/sW/sB/sO
hipError_t small_gemm(const float* A, int64_t lda, int64_t sA, const float* Wt, int64_t sW, const float* bias,
                      int64_t sB, float* out, int64_t ldo, int64_t sO, int M, int N, int K, int batch,
                      hipStream_t s);
hipError_t small_gemm_splitk(const float* A, int64_t lda, const float* Wt, const float* bias, float* out, int64_t ldo,
                             int M, int N, int K, int splits, float* part, hipStream_t s);
// rows r of x (stride elements apart): optional LayerNorm (gamma = 1 + scale) then optional
// L2 normalisation, fp32 out [rows][D]
hipError_t ln_l2_rows(const void* x, int in_bf16, int64_t stride, int rows, int D, const float* gamma,
                      const float* beta, int do_l2, float* out, hipStream_t s);
// text tokens: out[q*(L+1)+t] = table[ids[q][t]]*scale + pos[t] (t < L), cls*scale (t = L);
// pad_out[q*(L+1)+t] = pad_in[q][t] (t < L), 0 (t = L)
hipError_t text_embed(const int32_t* ids, int Q, int L, const void* table, int table_bf16, int V, const float* cls,
                      const float* pos, float scale, int D, void* out, int out_bf16, const float* pad_in,
                      float* pad_out, hipStream_t s);
// out[i][j] = a[i] . b[j]
hipError_t similarity(const float* a, const float* b, int B, int Q, int D, float* out, hipStream_t s);

hipError_t pool_l2(const void* emb, int is_bf16, int B, int L, int D, float* out, hipStream_t s);

// ---- training the classifier head on frozen tokens (probe_kernels.hip; H heads of dh = D / H) ----
// qraw [H][dh] (= query . Wq on entry) += bq, q~ = qraw * 1.442695041/sqrt(dh) * softplus(pds), U [H][D] = Wk[:,h,:] q~[h];
// split (bf16 tokens): Ut [32][D] = (U_hi | U_lo | 0) as well, and U = U_hi + U_lo
hipError_t probe_fold(float* qraw, const float* bq, const float* pds, const float* Wk, int D, int H, int split,
                      float* qt, float* U, bf16_t* Ut, hipStream_t s);
// wvt [H][D][dh] and wpt [H*dh][D] from the reference's [D][H][dh] leaves (small_gemm's operands), gamma = 1 + scale
hipError_t probe_pack(const float* wv, const float* wp, const float* scale, int D, int H, float* wvt, float* wpt,
                      float* gamma, hipStream_t s);
// out[z][m * ldo + n] = sum_k A[z][m * am + k * ak] * Bm[z][k * bk + n] over `batch` matrices at element strides
// sA / sB / sO (products and sums over b of outer products of the backward); probe_dot: the same with both
// operands contiguous in k, out[z][m * ldo + n] = A[z][m * am + :] . Bm[z][n * bn + :]
hipError_t probe_gemm(const float* A, int64_t sA, int64_t am, int64_t ak, const float* Bm, int64_t sB, int64_t bk,
                      float* out, int64_t sO, int64_t ldo, int M, int N, int K, int batch, hipStream_t s);
hipError_t probe_dot(const float* A, int64_t sA, int64_t am, const float* Bm, int64_t sB, int64_t bn, float* out,
                     int64_t sO, int64_t ldo, int M, int N, int K, int batch, hipStream_t s);
// out[n] = sum_m x[m][n]
hipError_t probe_colsum(const float* x, int M, int N, float* out, hipStream_t s);
// LayerNorm backward over rows of x [rows][D]: dx, stats [rows][2] = (mean, rstd), dscale / dbias [D]
hipError_t probe_ln_bwd(const float* x, const float* dy, const float* gamma, int rows, int D, float* dx, float* stats,
                        float* dscale, float* dbias, hipStream_t s);
// r [B][H] = z . dz; split: dzt [B][32][D] = (dz_hi | dz_lo | 0) per clip and dz = dz_hi + dz_lo in place
hipError_t probe_dz_finish(const float* z, float* dz, int B, int H, int D, int split, bf16_t* dzt, float* r,
                           hipStream_t s);
// pass 1: dl [B][H][S] = p (x . dz - r), p from the forward's logits and stats (bf16 x with S % 32 == 0 and dzt:
// the MFMA kernel); pass 2: dU [H][D] = sum_{b,s} dl x through part [B][pool_chunks(S)][H][D] and dUclip [B][H][D].
// pad: the forward's token paddings [B][S] or null: dl is exactly 0 at a padded token and its row is never read
bool probe_dl_uses_mfma(int in_bf16, int S);
hipError_t probe_dl(const void* x, int in_bf16, int B, int S, int D, int H, const float* dz, const bf16_t* dzt,
                    const float* logits, const float* stats, const float* r, float* dl, hipStream_t s,
                    const float* pad = nullptr);
hipError_t probe_wsum(const void* x, int in_bf16, int B, int S, int D, int H, const float* dl, float* part,
                      float* dUclip, float* dU, hipStream_t s, const float* pad = nullptr);
// dwk [D][H][dh] = dU[h][d] q~[h][j]
hipError_t probe_fold_bwd(const float* dU, const float* qt, int D, int H, float* dwk, hipStream_t s);
// dqraw [H][dh] = dq~ c softplus(pds), dpds [dh] = c sigmoid(pds) sum_h dq~ qraw
hipError_t probe_dq(const float* dqt, const float* qraw, const float* pds, int D, int H, float* dqraw, float* dpds,
                    hipStream_t s);

// ---- gallery search (retrieval_kernels.hip) ----
constexpr int kTopkMaxK = 128;      // longest list a query keeps
constexpr int kTopkMaxParts = 256;  // most row ranges a search splits the gallery into (sizes the workspace)
// queries of a workgroup: 32, or 16 where 32 (with their lists) do not fit the LDS; scores do not depend on it
int topk_group(int D, int k);
// pass 1: per row range p < *parts_out (<= kTopkMaxParts) the best k of rows [p * n, (p + 1) * n) per query, sorted by
// (score descending, row ascending) and padded with (-inf, -1): ws_sc / ws_id [parts][Q][k], ids = id_base + row.
// queries fp32 [Q][D]; gallery fp32 or bf16 [N][ld]; D = 64 j <= kPoolMaxD; N = 0 gives one list of padding.
// `storage` says how the gallery is stored: kGalleryF32 (0) and kGalleryBF16 (1) as above, or kGalleryF8: e4m3 codes
// [N][ld] (ld in bytes, a multiple of 16) and `scales` fp32 [N], powers of two, row r standing for codes[r] * scales[r]
// (DESIGN.md §4 "fp8 gallery"); the other two do not look at `scales`
constexpr int kGalleryF32 = 0, kGalleryBF16 = 1, kGalleryF8 = 2;
hipError_t topk_scan(const float* queries, int64_t Q, const void* gallery, int storage, int64_t N, int64_t ld, int D,
                     int k, int64_t id_base, float* ws_sc, int64_t* ws_id, int* parts_out, hipStream_t s,
                     const float* scales = nullptr);
// pass 2: the best k <= k_in of `parts` such lists [parts][Q][k_in] per query, same order, ties between lists by id
hipError_t topk_merge(const float* sin, const int64_t* iin, int64_t parts, int64_t Q, int k_in, int k, float* so,
                      int64_t* io, hipStream_t s);
// the grouped search (DESIGN.md §4 "Grouped gallery search"): row r belongs to group labels[r] (int64; negative = the
// row is blanked out), a group scores as its best row, and the lists hold one entry per group: (score, id of the best
// row, group).  Same passes and the same scores as above; the lists carry an int64 label per entry in LDS, so the
// queries of a workgroup are chosen against 16 B an entry
int topk_groups_group(int D, int k);
hipError_t topk_groups_scan(const float* queries, int64_t Q, const void* gallery, int storage, int64_t N, int64_t ld,
                            int D, int k, const int64_t* labels, int64_t id_base, float* ws_sc, int64_t* ws_id,
                            int64_t* ws_gr, int* parts_out, hipStream_t s, const float* scales = nullptr);
// the merge drops an entry when another list holds its group with an entry that comes before it, so the result is a
// function of the set of (score, group, id) alone
hipError_t topk_groups_merge(const float* sin, const int64_t* gin, const int64_t* iin, int64_t parts, int64_t Q, int k_in,
                             int k, float* so, int64_t* go, int64_t* io, hipStream_t s);
// the masked search (DESIGN.md §4 "Masked search"): the two scans above over the rows whose bit of `mask` is set (bit
// r & 31 of word r >> 5; ceil(N / 32) words a mask, bits past N ignored).  mask_stride 0: one mask for all queries;
// else query q's mask starts at word q * mask_stride (>= ceil(N / 32)).  Lists, scores of allowed rows and the merges
// are the unmasked ones'; N = 0 takes a null mask
hipError_t topk_scan_masked(const float* queries, int64_t Q, const void* gallery, int storage, int64_t N, int64_t ld,
                            int D, int k, int64_t id_base, const uint32_t* mask, int64_t mask_stride, float* ws_sc,
                            int64_t* ws_id, int* parts_out, hipStream_t s, const float* scales = nullptr);
hipError_t topk_groups_scan_masked(const float* queries, int64_t Q, const void* gallery, int storage, int64_t N,
                                   int64_t ld, int D, int k, const int64_t* labels, int64_t id_base,
                                   const uint32_t* mask, int64_t mask_stride, float* ws_sc, int64_t* ws_id,
                                   int64_t* ws_gr, int* parts_out, hipStream_t s, const float* scales = nullptr);
// the fp8 gallery's rows from x fp32 or bf16 [N][ldx] (16-byte aligned rows): codes [N][ldc] e4m3 (ldc a multiple of
// 16 bytes; columns past D keep what they held) and scales [N], one power of two per row (retrieval_kernels.hip)
hipError_t quantize_rows_f8(const void* x, int x_bf16, int64_t N, int64_t ldx, int D, uint8_t* codes, int64_t ldc,
                            float* scales, hipStream_t s);
// out[q * stride + w] = the packed bits of allow[q][32 w ..] != 0 (uint8 [Q][N], rows past N zero), ANDed with
// and_words[q * and_stride + w] where and_words is given (and_stride 0: the same words for every q)
hipError_t rowmask_pack(const uint8_t* allow, int64_t Q, int64_t N, const uint32_t* and_words, int64_t and_stride,
                        uint32_t* out, int64_t stride, hipStream_t s);

// ---- frame ingest (preprocess.hip) ----
// video_utils.py:109-124: size of the resized frame and the crop window's origin in it (mode 0 centre
// crop, 1 stretch to S x S); a message if this library's kernel cannot take the geometry, else nullptr
const char* preprocess_geometry(int64_t H, int64_t W, int64_t S, int mode, int64_t* new_h, int64_t* new_w,
                                int64_t* y0, int64_t* x0);
// uint8 frames (frame n, row y, pixel x, channel c at n*frame_stride + y*row_stride + 3x + c) gathered by
// frame_idx (nullable: 0..F-1), resized as cv2.resize does on uint8 and cropped -> dst uint8 [F, S, S, 3]
hipError_t preprocess_frames(const uint8_t* src, int64_t N, int64_t H, int64_t W, int64_t row_stride,
                             int64_t frame_stride, const int32_t* frame_idx, int64_t F, int mode, int swap_rb,
                             int64_t S, uint8_t* dst, hipStream_t s);
// The same from a decoder's 4:2:0 planes (the values of vp_yuv_format): the taps are converted to uint8 RGB
// on the way, luma (y, x) with chroma (y >> 1, x >> 1), then resized as above.
enum { YUV_NV12 = 0, YUV_I420 = 1, YUV_P010 = 2 };
struct YuvPlanes {
  const void* plane[3];                    // Y, UV, - (NV12, P010: 16-bit words) or Y, U, V (I420)
  int64_t row_stride[3], frame_stride[3];  // bytes
  int format;
};
// out[0..8] = rows R, G, B x (cy, cu, cv) = floor(x * 65536 + 0.5), out[9] = yoff, out[10] = coff for
// matrix 0 (BT.601) / 1 (BT.709), range 0 (limited) / 1 (full), bit_depth 8 / 10; a message for anything else
const char* yuv_coefficients(int matrix, int range, int bit_depth, int32_t out[11]);
// coef: yuv_coefficients' table.  P010 planes and strides must be 2-byte aligned (hipErrorInvalidValue)
hipError_t preprocess_yuv(const YuvPlanes& src, const int32_t coef[11], int64_t N, int64_t H, int64_t W,
                          const int32_t* frame_idx, int64_t F, int mode, int64_t S, uint8_t* dst, hipStream_t s);
// Both once more with the geometry per output frame: views is a device table int32 [V, 9] of (box_y, box_x,
// box_h, box_w, new_h, new_w, win_y, win_x, flags) rows, which the kernel clamps; output frame v*T + t is
// cv2.resize(frame[box], (new_w, new_h))[win : win + S], mirrored along x where flags & 1, of source frame
// frame_idx[v*T + t] (nullable: t) -> dst uint8 [V*T, S, S, 3]
hipError_t preprocess_views(const uint8_t* src, int64_t N, int64_t H, int64_t W, int64_t row_stride,
                            int64_t frame_stride, const int32_t* frame_idx, const int32_t* views, int64_t V,
                            int64_t T, int swap_rb, int64_t S, uint8_t* dst, hipStream_t s);
hipError_t preprocess_yuv_views(const YuvPlanes& src, const int32_t coef[11], int64_t N, int64_t H, int64_t W,
                                const int32_t* frame_idx, const int32_t* views, int64_t V, int64_t T, int64_t S,
                                uint8_t* dst, hipStream_t s);

}  // namespace vp
