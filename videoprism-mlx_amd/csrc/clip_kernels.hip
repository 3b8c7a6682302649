// Kernels of the LvT video-text path besides attention.
//
// Contrastive pooler (AttenTokenPoolingLayer, layers.py:1044-1136; num_queries = 1, no logit
// cap, per-dim scale on; paddings None in the models, given to the *_masked kernels by the
// classifier head's training ops).  Its single query is a parameter, so the projected
// and scaled query q~[h] (layers.py:502-527, :676-681) is a constant and the key projection
// folds into it on the host:  logit[g,h,s] = x[g,s,:].U[h,:] + q~[h].bk[h], U[h] = Wk[:,h,:] q~[h].
// The constant q~[h].bk[h] shifts every logit of a row equally and cancels in the softmax, so
// the pooler never materialises K (B*S x 4D) or V: with p = softmax(logit) and sum_s p = 1,
//   enc[g,h,:] = sum_s p[g,h,s] (x[g,s,:] Wv[:,h,:] + bv[h]) = z[g,h,:] Wv[:,h,:] + bv[h],
//   z[g,h,:]   = sum_s p[g,h,s] x[g,s,:]
// which turns the two [S x D] x [D x 4D] projections per clip into two streaming passes over x
// (HBM-bound: pool_logits, pool_wsum) and [G x D] x [D x dh] matrix products (small_gemm).
//   pool_logits : logits[g][h][s] = x[g*S+s] . U[h]       (pool_stream.h pass 1, U shared by all clips)
//   pool_stats  : (max, 1/sum exp(l - max)) per (g, h)    (fp32 softmax, layers.py:650-654)
//   pool_wsum   : zpart[g][c][h][:] = sum over the c-th 256-row chunk of p * x   (pool_stream.h pass 2)
//   pool_reduce : z[g][h][:] = sum_c zpart
//   small_gemm  : out[m][n] = A[m][:] . Wt[:][n] + bias[n], batched (enc per head, then post)
//   ln_l2_rows  : LayerNorm (layers.py:208-270) and/or _l2_normalize (encoders.py:50-67), fp32
// Widths: D up to kPoolMaxD = 1536 (LayerNorm's range; Giant is 1408 = 22 x 64 = 5 x 256 + 128), at most kPoolMaxH
// heads.  The passes' own width rules are pool_stream.h's; ln_l2_rows takes any D up to the limit.  Every width up
// to 1024 runs the instantiation, grid and summation order it always ran.
// Text tower: text_embed = Embedding(ids)*sqrt(D) + sinusoidal PositionalEmbedding, with the
// CLS token appended (encoders.py:190-266, :700-740).  similarity = video_emb . text_emb^T.
#include "pool_stream.h"

namespace vp {

namespace {

struct StoreLogits {
  float* __restrict__ logits;
  __device__ __forceinline__ void operator()(int64_t, int64_t idx, float v) const { logits[idx] = v; }
  // a padded token (layers.py:51-72): exp(kPadLogit - max) is exactly 0 beside a valid token, and a clip of padded
  // tokens alone has max = kPadLogit and the uniform softmax, so pool_stats_kernel needs no mask
  __device__ __forceinline__ void dead(int64_t, int64_t idx) const { logits[idx] = kPadLogit; }
};

template <int NJ>
__global__ __launch_bounds__(256) void pool_logits_kernel(const void* __restrict__ x, int in_bf16, int64_t rows,
                                                          int S, int D, const float* __restrict__ U, int H,
                                                          float* __restrict__ logits) {
  pool_scalar_pass<NJ, false>(x, in_bf16, rows, S, D, U, H, StoreLogits{logits});
}

__global__ __launch_bounds__(256) void pool_logits_mfma_kernel(const bf16_t* __restrict__ x, int64_t rows, int S,
                                                               int D, const bf16_t* __restrict__ Ut, int H,
                                                               float* __restrict__ logits) {
  pool_mfma_pass<false>(x, rows, S, D, Ut, H, StoreLogits{logits});
}

// the same passes under token paddings pad [G][S] (pool_stream.h, PadRows)
template <int NJ>
__global__ __launch_bounds__(256) void pool_logits_masked_kernel(const void* __restrict__ x, int in_bf16,
                                                                 int64_t rows, int S, int D,
                                                                 const float* __restrict__ U, int H,
                                                                 const float* __restrict__ pad,
                                                                 float* __restrict__ logits) {
  pool_scalar_pass<NJ, false>(x, in_bf16, rows, S, D, U, H, StoreLogits{logits}, PadRows{pad});
}

__global__ __launch_bounds__(256) void pool_logits_mfma_masked_kernel(const bf16_t* __restrict__ x, int64_t rows,
                                                                      int S, int D, const bf16_t* __restrict__ Ut,
                                                                      int H, const float* __restrict__ pad,
                                                                      float* __restrict__ logits) {
  pool_mfma_pass<false>(x, rows, S, D, Ut, H, StoreLogits{logits}, PadRows{pad});
}

__global__ __launch_bounds__(256) void pool_stats_kernel(const float* __restrict__ logits, int S,
                                                         float* __restrict__ stats) {
  __shared__ float red[4];
  const float* l = logits + (int64_t)blockIdx.x * S;
  float m = -INFINITY;
  for (int s = threadIdx.x; s < S; s += 256) m = fmaxf(m, l[s]);
  m = block_max(m, red);
  float sum = 0.0f;
  for (int s = threadIdx.x; s < S; s += 256) sum += expf(l[s] - m);
  sum = block_sum(sum, red);
  if (threadIdx.x == 0) {
    stats[2 * blockIdx.x] = m;
    stats[2 * blockIdx.x + 1] = 1.0f / sum;
  }
}

// the softmax rebuilt from the logits and pool_stats, the [256][16] weights visited by row
struct FillSoftmax {
  static constexpr bool kByRow = true;
  const float* __restrict__ logits;
  const float* __restrict__ stats;
  __device__ __forceinline__ float operator()(int64_t gh, int64_t idx) const {
    return softmax_p(logits, stats, gh, idx);
  }
};

__global__ __launch_bounds__(128) void pool_wsum_kernel(const void* __restrict__ x, int in_bf16, int S, int D,
                                                        int H, const float* __restrict__ logits,
                                                        const float* __restrict__ stats, int C,
                                                        float* __restrict__ zpart) {
  pool_wsum_pass(x, in_bf16, S, D, H, C, FillSoftmax{logits, stats}, zpart);
}

// under token paddings: the dead rows (pool_stream.h, DeadRows) are neither loaded nor summed
__global__ __launch_bounds__(128) void pool_wsum_masked_kernel(const void* __restrict__ x, int in_bf16, int S, int D,
                                                               int H, const float* __restrict__ logits,
                                                               const float* __restrict__ stats,
                                                               const float* __restrict__ pad, int C,
                                                               float* __restrict__ zpart) {
  pool_wsum_pass(x, in_bf16, S, D, H, C, FillSoftmax{logits, stats}, zpart, DeadRows{pad, stats, H});
}

// out[g][e] = sum_{i < n} part[g][i][e] in index order
__global__ __launch_bounds__(256) void pool_reduce_kernel(const float* __restrict__ part, int n, int64_t HD,
                                                          int64_t total, float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int64_t g = i / HD, e = i % HD;
  const float* p = part + g * n * HD + e;
  float s = 0.0f;
#pragma unroll 8
  for (int c = 0; c < n; ++c) s += p[(int64_t)c * HD];
  out[i] = s;
}

// out[m][n] = A[m][:] . Wt[:][n] + bias[n] for small M (pooled vectors): a workgroup owns 64
// columns x 32 rows and splits K four ways (one quarter per wave, partial sums combined through
// LDS); A^T chunks are staged in LDS and read as float4 broadcasts, Wt rows are coalesced.
constexpr int kSgM = 32;
constexpr int kSgN = 64;
constexpr int kSgK = 128;

__global__ __launch_bounds__(256) void small_gemm_kernel(const float* __restrict__ A, int64_t lda, int64_t sA,
                                                         const float* __restrict__ Wt, int64_t sW,
                                                         const float* __restrict__ bias, int64_t sB,
                                                         float* __restrict__ out, int64_t ldo, int64_t sO, int M,
                                                         int N, int K) {
  __shared__ __attribute__((aligned(16))) float At[kSgK][kSgM];  // A^T chunk
  __shared__ float red[3][kSgM][kSgN];
  const int bz = blockIdx.z;
  A += bz * sA;
  Wt += bz * sW;
  out += bz * sO;
  const float* bb = bias ? bias + bz * sB : nullptr;
  const int col = threadIdx.x & 63;
  const int quarter = threadIdx.x >> 6;  // wave
  const int n = blockIdx.x * kSgN + col;
  const int m0 = blockIdx.y * kSgM;
  float acc[kSgM];
#pragma unroll
  for (int i = 0; i < kSgM; ++i) acc[i] = 0.0f;
  for (int k0 = 0; k0 < K; k0 += kSgK) {
    __syncthreads();
    for (int i = threadIdx.x; i < kSgM * kSgK; i += 256) {
      const int mi = i / kSgK, kk = i % kSgK;
      At[kk][mi] = (m0 + mi < M && k0 + kk < K) ? A[(int64_t)(m0 + mi) * lda + k0 + kk] : 0.0f;
    }
    __syncthreads();
    if (n < N) {
      const int kq0 = quarter * (kSgK / 4);
#pragma unroll 4
      for (int kk = kq0; kk < kq0 + kSgK / 4; ++kk) {
        const float w = k0 + kk < K ? Wt[(int64_t)(k0 + kk) * N + n] : 0.0f;
        const float4* ar = reinterpret_cast<const float4*>(At[kk]);
#pragma unroll
        for (int i4 = 0; i4 < kSgM / 4; ++i4) {
          const float4 a = ar[i4];
          acc[4 * i4] = fmaf(a.x, w, acc[4 * i4]);
          acc[4 * i4 + 1] = fmaf(a.y, w, acc[4 * i4 + 1]);
          acc[4 * i4 + 2] = fmaf(a.z, w, acc[4 * i4 + 2]);
          acc[4 * i4 + 3] = fmaf(a.w, w, acc[4 * i4 + 3]);
        }
      }
    }
  }
  if (quarter > 0) {
#pragma unroll
    for (int i = 0; i < kSgM; ++i) red[quarter - 1][i][col] = acc[i];
  }
  __syncthreads();
  if (quarter > 0 || n >= N) return;
  const float b = bb ? bb[n] : 0.0f;
#pragma unroll
  for (int i = 0; i < kSgM; ++i)
    if (m0 + i < M) out[(int64_t)(m0 + i) * ldo + n] = acc[i] + red[0][i][col] + red[1][i][col] + red[2][i][col] + b;
}

// out[m][n] = bias[n] + sum_z part[z][m][n] in z order (small_gemm_splitk)
__global__ __launch_bounds__(256) void splitk_reduce_kernel(const float* __restrict__ part, int splits, int64_t MN,
                                                            int N, const float* __restrict__ bias,
                                                            float* __restrict__ out, int64_t ldo) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= MN) return;
  float v = part[i];
  for (int z = 1; z < splits; ++z) v += part[z * MN + i];
  const int64_t m = i / N;
  const int n = (int)(i % N);
  out[m * ldo + n] = v + (bias ? bias[n] : 0.0f);
}

// NV: 256-column steps a thread keeps in registers: 4 (D <= 1024) or 6 (D <= 1536)
template <int NV>
__global__ __launch_bounds__(256) void ln_l2_rows_kernel(const void* __restrict__ x, int in_bf16, int64_t stride,
                                                         int D, const float* __restrict__ gamma,
                                                         const float* __restrict__ beta, int do_l2,
                                                         float* __restrict__ out) {
  __shared__ float red[4];
  const int64_t r = blockIdx.x;
  float v[NV];
  const int nj = (D + 255) >> 8;
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const int d = threadIdx.x + 256 * j;
    v[j] = (j < nj && d < D) ? ldx(x, in_bf16, r * stride + d) : 0.0f;
  }
  if (gamma) {
    float mean, rstd;
    ln_row_stats(v, D, red, mean, rstd);
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      const int d = threadIdx.x + 256 * j;
      if (j < nj && d < D) v[j] = (v[j] - mean) * rstd * gamma[d] + beta[d];
      else v[j] = 0.0f;
    }
  }
  if (do_l2) {
    float q = 0.0f;
#pragma unroll
    for (int j = 0; j < NV; ++j) q = fmaf(v[j], v[j], q);
    const float inv = 1.0f / sqrtf(block_sum(q, red) + 1e-12f);
#pragma unroll
    for (int j = 0; j < NV; ++j) v[j] *= inv;
  }
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const int d = threadIdx.x + 256 * j;
    if (j < nj && d < D) out[r * D + d] = v[j];
  }
}

__global__ __launch_bounds__(256) void text_embed_kernel(const int32_t* __restrict__ ids, int L, const void* table,
                                                         int table_bf16, int V, const float* __restrict__ cls,
                                                         const float* __restrict__ pos, float scale, int D,
                                                         void* out, int out_bf16, const float* __restrict__ pad_in,
                                                         float* __restrict__ pad_out) {
  const int64_t r = blockIdx.x;  // q * (L + 1) + t
  const int64_t q = r / (L + 1);
  const int t = (int)(r % (L + 1));
  // paddings with the CLS token's zero appended (encoders.py:737-740)
  if (threadIdx.x == 0) pad_out[r] = t < L ? pad_in[q * L + t] : 0.0f;
  int id = 0;
  if (t < L) {
    id = ids[q * L + t];
    id = id < 0 ? 0 : (id >= V ? V - 1 : id);  // jnp indexing clamps out-of-range ids
  }
  for (int d = threadIdx.x; d < D; d += 256) {
    const float e = t < L ? ldx(table, table_bf16, (int64_t)id * D + d) * scale + pos[(int64_t)t * D + d]
                          : cls[d] * scale;
    if (out_bf16) static_cast<bf16_t*>(out)[r * D + d] = f2bf(e);
    else static_cast<float*>(out)[r * D + d] = e;
  }
}

__global__ __launch_bounds__(256) void similarity_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                         int B, int Q, int D, float* __restrict__ out) {
  __shared__ float red[4];
  const int i = blockIdx.x / Q, j = blockIdx.x % Q;
  float s = 0.0f;
  for (int d = threadIdx.x; d < D; d += 256) s = fmaf(a[(int64_t)i * D + d], b[(int64_t)j * D + d], s);
  s = block_sum(s, red);
  if (threadIdx.x == 0) out[blockIdx.x] = s;
}

}  // namespace

hipError_t pool_logits(const void* x, int in_bf16, int64_t rows, int S, int D, const float* U, const bf16_t* Ut,
                       int H, float* logits, hipStream_t s, const float* pad) {
  if (D % 64 || D > kPoolMaxD || H < 1 || H > kPoolMaxH || rows % S) return hipErrorInvalidValue;
  if (in_bf16 && Ut && S % 32 == 0) {
    const int64_t grid = (rows / 32 + 3) / 4;
    if (pad)
      hipLaunchKernelGGL(pool_logits_mfma_masked_kernel, dim3((unsigned)grid), dim3(256), 0, s, (const bf16_t*)x,
                         rows, S, D, Ut, H, pad, logits);
    else
      hipLaunchKernelGGL(pool_logits_mfma_kernel, dim3((unsigned)grid), dim3(256), 0, s, (const bf16_t*)x, rows, S,
                         D, Ut, H, logits);
    return hipGetLastError();
  }
  const int64_t grid = (rows + kPlRows - 1) / kPlRows;
  if (pad)
    return launch_pool_scalar(&pool_logits_masked_kernel<16>, &pool_logits_masked_kernel<24>, dim3((unsigned)grid), D,
                              H, s, x, in_bf16, rows, S, D, U, H, pad, logits);
  return launch_pool_scalar(&pool_logits_kernel<16>, &pool_logits_kernel<24>, dim3((unsigned)grid), D, H, s, x, in_bf16,
                            rows, S, D, U, H, logits);
}

hipError_t pool_reduce(const float* part, int n, int64_t HD, int64_t groups, float* out, hipStream_t s) {
  const int64_t total = groups * HD;
  hipLaunchKernelGGL(pool_reduce_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, part, n, HD, total,
                     out);
  return hipGetLastError();
}

hipError_t pool_softmax_wsum(const void* x, int in_bf16, int G, int S, int D, int H, const float* logits,
                             float* stats, float* zpart, float* z, hipStream_t s, const float* pad) {
  if (D % 128 || D > kPoolMaxD || H < 1 || H > kPoolMaxH) return hipErrorInvalidValue;
  hipLaunchKernelGGL(pool_stats_kernel, dim3(G * H), dim3(256), 0, s, logits, S, stats);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const int C = (S + kPwRows - 1) / kPwRows;
  if (pad)
    hipLaunchKernelGGL(pool_wsum_masked_kernel, dim3(G * C * ((D + 255) / 256)), dim3(128), 0, s, x, in_bf16, S, D, H,
                       logits, stats, pad, C, zpart);
  else
    hipLaunchKernelGGL(pool_wsum_kernel, dim3(G * C * ((D + 255) / 256)), dim3(128), 0, s, x, in_bf16, S, D, H, logits, stats,
                       C, zpart);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  return pool_reduce(zpart, C, (int64_t)H * D, G, z, s);
}

int pool_chunks(int S) { return (S + kPwRows - 1) / kPwRows; }

hipError_t small_gemm(const float* A, int64_t lda, int64_t sA, const float* Wt, int64_t sW, const float* bias,
                      int64_t sB, float* out, int64_t ldo, int64_t sO, int M, int N, int K, int batch,
                      hipStream_t s) {
  if (M < 1 || N < 1 || K < 1 || batch < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(small_gemm_kernel, dim3((N + kSgN - 1) / kSgN, (M + kSgM - 1) / kSgM, batch), dim3(256), 0, s, A,
                     lda, sA, Wt, sW, bias, sB, out, ldo, sO, M, N, K);
  return hipGetLastError();
}

// K split `splits` ways as a batch of small_gemm over K slices (A columns / Wt rows), partials [splits][M][N]
// in `part`, then summed in slice order: the same bits for any M, and splits x the workgroups of one
// small_gemm (the pooler's output projection, K = heads x dim_per_head = 4096 on LvT-Large, otherwise ran on
// N / 64 = 16 workgroups)
hipError_t small_gemm_splitk(const float* A, int64_t lda, const float* Wt, const float* bias, float* out, int64_t ldo,
                             int M, int N, int K, int splits, float* part, hipStream_t s) {
  if (splits < 1 || K % splits) return hipErrorInvalidValue;
  const int Kc = K / splits;
  hipError_t e = small_gemm(A, lda, Kc, Wt, (int64_t)Kc * N, nullptr, 0, part, N, (int64_t)M * N, M, N, Kc, splits, s);
  if (e != hipSuccess) return e;
  const int64_t MN = (int64_t)M * N;
  hipLaunchKernelGGL(splitk_reduce_kernel, dim3((unsigned)((MN + 255) / 256)), dim3(256), 0, s, part, splits, MN, N,
                     bias, out, ldo);
  return hipGetLastError();
}

hipError_t ln_l2_rows(const void* x, int in_bf16, int64_t stride, int rows, int D, const float* gamma,
                      const float* beta, int do_l2, float* out, hipStream_t s) {
  if (D < 1 || D > kPoolMaxD || rows < 1) return hipErrorInvalidValue;
  if (D <= 1024)
    hipLaunchKernelGGL(ln_l2_rows_kernel<4>, dim3(rows), dim3(256), 0, s, x, in_bf16, stride, D, gamma, beta, do_l2,
                       out);
  else
    hipLaunchKernelGGL(ln_l2_rows_kernel<6>, dim3(rows), dim3(256), 0, s, x, in_bf16, stride, D, gamma, beta, do_l2,
                       out);
  return hipGetLastError();
}

hipError_t text_embed(const int32_t* ids, int Q, int L, const void* table, int table_bf16, int V, const float* cls,
                      const float* pos, float scale, int D, void* out, int out_bf16, const float* pad_in,
                      float* pad_out, hipStream_t s) {
  if (Q < 1 || L < 0 || V < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(text_embed_kernel, dim3(Q * (L + 1)), dim3(256), 0, s, ids, L, table, table_bf16, V, cls, pos,
                     scale, D, out, out_bf16, pad_in, pad_out);
  return hipGetLastError();
}

hipError_t similarity(const float* a, const float* b, int B, int Q, int D, float* out, hipStream_t s) {
  if (B < 1 || Q < 1 || D < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(similarity_kernel, dim3(B * Q), dim3(256), 0, s, a, b, B, Q, D, out);
  return hipGetLastError();
}

}  // namespace vp
