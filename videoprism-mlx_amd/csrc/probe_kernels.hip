// Training the classifier head (atten_pooler + projection, encoders.py:634-652) on frozen tokens: the
// device-side fold of the forward and the kernels of the backward (vp_probe.cpp drives them).
//
// The forward pooler folds the query into the key projection, U[h] = Wk[:,h,:] q~[h], and streams the tokens
// twice (the two passes of pool_stream.h).  An engine folds on the host once; a head that is being trained folds
// on the device every step:
//   probe_fold_q  : q~[h][j] = qraw[h][j] * c * softplus(pds[j]),  qraw = query . Wq + bq, c = 1.442695041/sqrt(dh)
//   probe_fold_u  : U[h][d] = Wk[d][h][:] . q~[h]; bf16 tokens: also Ut = (U_hi | U_lo | 0) as pool_split_u packs it,
//                   and U itself becomes U_hi + U_lo, so the MFMA and the scalar logits kernels see one and the same key
//   probe_pack    : Wv^T [H][D][dh], Wpost^T [H*dh][D] and gamma = 1 + scale, the layouts small_gemm / ln_l2_rows take
// With the tokens frozen there is no dX, and the backward folds the same way.  With p = softmax_s(x . U[h]),
// z = sum_s p x, enc = z Wv + bv and dz[b][h] = denc[b][h] Wv[:,h,:]^T:
//   dp[b,h,s] = x[b,s] . dz[b,h]         pass 1 over the tokens, the operand per clip
//   r[b,h]    = sum_s p dp = z[b,h] . dz[b,h]      (no pass: probe_dz_finish)
//   dl        = p (dp - r)               written by pass 1's store (probe_dl / probe_dl_mfma)
//   dU[h]     = sum_{b,s} dl x[b,s]      pass 2 with dl as the signed weights (probe_wsum), chunk
//                                        partials [B][C][H][D] summed over clips and chunks in index order
//   dWk[:,h,:] = dU[h] (x) q~[h],  dq~[h] = Wk[:,h,:]^T dU[h],  dbk = 0 (the key bias cancels in the softmax)
// Everything else is parameter-sized or [B][H][D]-sized: probe_gemm (strided, batched, the second operand's rows
// contiguous in n: products and the "sum over b of outer products" of dWc, dWp, dWv), probe_dot (both operands
// contiguous in k), probe_colsum (bias gradients), the LayerNorm and query backward kernels.  No atomics: every sum has one owner and a fixed order, so equal inputs give equal bits.
#include "pool_stream.h"

namespace vp {

namespace {

__device__ __forceinline__ float softplus(float x) { return x > 20.0f ? x : log1pf(expf(x)); }

// ---------------------------------------------------------------------------------------------------------
// forward fold
// ---------------------------------------------------------------------------------------------------------
// qraw += bq in place, q~ = qraw c softplus(pds)
__global__ __launch_bounds__(256) void probe_fold_q_kernel(float* __restrict__ qraw, const float* __restrict__ bq,
                                                           const float* __restrict__ pds, int n, int dh, float c,
                                                           float* __restrict__ qt) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float q = qraw[i] + bq[i];
  qraw[i] = q;
  qt[i] = q * c * softplus(pds[i % dh]);
}

// a workgroup owns one column d; wave w the heads w, w + 4, ...
__global__ __launch_bounds__(256) void probe_fold_u_kernel(const float* __restrict__ Wk,
                                                           const float* __restrict__ qt, int D, int H, int dh,
                                                           int split, float* __restrict__ U,
                                                           bf16_t* __restrict__ Ut) {
  const int d = blockIdx.x, lane = threadIdx.x & 63;
  for (int h = threadIdx.x >> 6; h < H; h += 4) {
    const float* wr = Wk + ((int64_t)d * H + h) * dh;
    float a = 0.0f;
    for (int j = lane; j < dh; j += 64) a = fmaf(wr[j], qt[h * dh + j], a);
    a = wave_sum(a);
    if (lane == 0) {
      if (split) {
        const bf16_t hi = f2bf(a), lo = f2bf(a - bf2f(hi));
        Ut[(int64_t)h * D + d] = hi;
        Ut[(int64_t)(H + h) * D + d] = lo;
        a = bf2f(hi) + bf2f(lo);
      }
      U[(int64_t)h * D + d] = a;
    }
  }
}

// i over D x (H*dh): wvt[h][d][j] = wv[d][h][j], wpt[(h,j)][d] = wp[d][(h,j)], gamma = 1 + scale
__global__ __launch_bounds__(256) void probe_pack_kernel(const float* __restrict__ wv, const float* __restrict__ wp,
                                                         const float* __restrict__ scale, int D, int H, int dh,
                                                         float* __restrict__ wvt, float* __restrict__ wpt,
                                                         float* __restrict__ gamma) {
  const int64_t HJ = (int64_t)H * dh;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= D * HJ) return;
  const int64_t d = i / HJ, hj = i % HJ;
  const int64_t h = hj / dh, j = hj % dh;
  wvt[(h * D + d) * dh + j] = wv[i];
  wpt[hj * D + d] = wp[i];
  if (i < D) gamma[i] = 1.0f + scale[i];
}

// ---------------------------------------------------------------------------------------------------------
// small products
// ---------------------------------------------------------------------------------------------------------
// out[z][m * ldo + n] = sum_k A[z][m * am + k * ak] * Bm[z][k * bk + n], Bm rows contiguous in n: a workgroup of 16
// waves owns 64 columns of four rows and splits K sixteen ways (one contiguous slice per wave, summed in k order;
// the slices are added in wave order through LDS).  These products have few outputs and a long K (M = 1 or B rows,
// K = D): the split is what keeps more than a dozen waves busy.  The A values are wave-uniform, the Bm reads coalesced.
constexpr int kPgM = 4;  // rows per workgroup
constexpr int kPgN = 64;
constexpr int kPgS = 16;  // K slices = waves per workgroup

__global__ __launch_bounds__(64 * kPgS) void probe_gemm_kernel(const float* __restrict__ A, int64_t sA, int64_t am,
                                                              int64_t ak, const float* __restrict__ Bm, int64_t sB,
                                                              int64_t bk, float* __restrict__ out, int64_t sO,
                                                              int64_t ldo, int M, int N, int K) {
  __shared__ float red[kPgS - 1][kPgM][kPgN];
  const int col = threadIdx.x & 63, slice = threadIdx.x >> 6;
  const int n = blockIdx.x * kPgN + col;
  const int m0 = blockIdx.y * kPgM;
  A += blockIdx.z * sA;
  Bm += blockIdx.z * sB + min(n, N - 1);  // columns past N read column N - 1 and are not stored
  out += blockIdx.z * sO;
  // rows past M read row M - 1 and are not stored
  const float* a0 = A + (int64_t)m0 * am;
  const float* a1 = A + (int64_t)min(m0 + 1, M - 1) * am;
  const float* a2 = A + (int64_t)min(m0 + 2, M - 1) * am;
  const float* a3 = A + (int64_t)min(m0 + 3, M - 1) * am;
  const int ks = (K + kPgS - 1) / kPgS;
  const int k1 = min(K, (slice + 1) * ks);
  float c0 = 0.0f, c1 = 0.0f, c2 = 0.0f, c3 = 0.0f;
#pragma unroll 8
  for (int k = slice * ks; k < k1; ++k) {
    const float b = Bm[(int64_t)k * bk];
    c0 = fmaf(a0[(int64_t)k * ak], b, c0);
    c1 = fmaf(a1[(int64_t)k * ak], b, c1);
    c2 = fmaf(a2[(int64_t)k * ak], b, c2);
    c3 = fmaf(a3[(int64_t)k * ak], b, c3);
  }
  if (slice > 0) {
    red[slice - 1][0][col] = c0;
    red[slice - 1][1][col] = c1;
    red[slice - 1][2][col] = c2;
    red[slice - 1][3][col] = c3;
  }
  __syncthreads();
  if (slice > 0 || n >= N) return;
  float c[kPgM] = {c0, c1, c2, c3};
#pragma unroll
  for (int i = 0; i < kPgM; ++i) {
#pragma unroll
    for (int w = 0; w < kPgS - 1; ++w) c[i] += red[w][i][col];
    if (m0 + i < M) out[(int64_t)(m0 + i) * ldo + n] = c[i];
  }
}

// out[z][m * ldo + n] = A[z][m * am + :] . Bm[z][n * bn + :], both operands contiguous in k: one wave per column n
// (a row of Bm), lanes over k, every row m in turn (the Bm row stays in L1)
__global__ __launch_bounds__(256) void probe_dot_kernel(const float* __restrict__ A, int64_t sA, int64_t am,
                                                        const float* __restrict__ Bm, int64_t sB, int64_t bn,
                                                        float* __restrict__ out, int64_t sO, int64_t ldo, int M, int N,
                                                        int K) {
  const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (n >= N) return;  // whole wave
  const int lane = threadIdx.x & 63;
  A += blockIdx.z * sA;
  const float* br = Bm + blockIdx.z * sB + (int64_t)n * bn;
  out += blockIdx.z * sO;
  for (int m = 0; m < M; ++m) {
    const float* ar = A + (int64_t)m * am;
    float a = 0.0f;
    for (int k = lane; k < K; k += 64) a = fmaf(ar[k], br[k], a);
    a = wave_sum(a);
    if (lane == 0) out[(int64_t)m * ldo + n] = a;
  }
}

// out[n] = sum_m x[m][n] in m order
__global__ __launch_bounds__(256) void probe_colsum_kernel(const float* __restrict__ x, int M, int N,
                                                           float* __restrict__ out) {
  const int n = blockIdx.x * 256 + threadIdx.x;
  if (n >= N) return;
  float s = 0.0f;
  for (int m = 0; m < M; ++m) s += x[(int64_t)m * N + n];
  out[n] = s;
}

// ---------------------------------------------------------------------------------------------------------
// LayerNorm backward (layers.py:208-270, eps 1e-6, gamma = 1 + scale): one workgroup per row
//   xh = (x - mean) rstd, g = dy gamma, dx = rstd (g - mean(g) - xh mean(g xh)); stats[row] = (mean, rstd)
// NV: 256-column steps a thread keeps in registers: 4 (D <= 1024) or 6 (D <= 1536), as ln_l2_rows
// ---------------------------------------------------------------------------------------------------------
template <int NV>
__global__ __launch_bounds__(256) void probe_ln_bwd_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                           const float* __restrict__ gamma, int D,
                                                           float* __restrict__ dx, float* __restrict__ stats) {
  __shared__ float red[4];
  const int64_t r = blockIdx.x;
  float v[NV], g[NV];
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const int d = threadIdx.x + 256 * j;
    const bool in = d < D;
    v[j] = in ? x[r * D + d] : 0.0f;
    g[j] = in ? dy[r * D + d] * gamma[d] : 0.0f;
  }
  float mean, rstd;
  ln_row_stats(v, D, red, mean, rstd);
  float sg = 0.0f, sgx = 0.0f;
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const int d = threadIdx.x + 256 * j;
    v[j] = d < D ? (v[j] - mean) * rstd : 0.0f;
    sg += g[j];
    sgx = fmaf(g[j], v[j], sgx);
  }
  const float mg = block_sum(sg, red) / (float)D;
  const float mgx = block_sum(sgx, red) / (float)D;
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const int d = threadIdx.x + 256 * j;
    if (d < D) dx[r * D + d] = rstd * (g[j] - mg - v[j] * mgx);
  }
  if (threadIdx.x == 0) {
    stats[2 * r] = mean;
    stats[2 * r + 1] = rstd;
  }
}

// dscale[d] = sum_b dy[b][d] xh[b][d], dbias[d] = sum_b dy[b][d], in b order
__global__ __launch_bounds__(256) void probe_ln_param_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                             const float* __restrict__ stats, int rows, int D,
                                                             float* __restrict__ dscale, float* __restrict__ dbias) {
  const int d = blockIdx.x * 256 + threadIdx.x;
  if (d >= D) return;
  float ds = 0.0f, db = 0.0f;
  for (int b = 0; b < rows; ++b) {
    const float g = dy[(int64_t)b * D + d];
    ds = fmaf(g, (x[(int64_t)b * D + d] - stats[2 * b]) * stats[2 * b + 1], ds);
    db += g;
  }
  dscale[d] = ds;
  dbias[d] = db;
}

// ---------------------------------------------------------------------------------------------------------
// r[b][h] = z[b][h] . dz[b][h], one wave per (b, h).  bf16 tokens: dz is split as U is (probe_fold_u): dzt
// [B][32][D] = (dz_hi | dz_lo | 0) per clip for the MFMA pass, dz itself becomes dz_hi + dz_lo
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void probe_dz_finish_kernel(const float* __restrict__ z, float* __restrict__ dz,
                                                              int BH, int H, int D, int split,
                                                              bf16_t* __restrict__ dzt, float* __restrict__ r) {
  const int bh = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (bh >= BH) return;  // whole wave
  const int lane = threadIdx.x & 63;
  const int b = bh / H, h = bh % H;
  float a = 0.0f;
  for (int d = lane; d < D; d += 64) {
    const int64_t i = (int64_t)bh * D + d;
    float v = dz[i];
    if (split) {
      const bf16_t hi = f2bf(v), lo = f2bf(v - bf2f(hi));
      dzt[((int64_t)b * 32 + h) * D + d] = hi;
      dzt[((int64_t)b * 32 + H + h) * D + d] = lo;
      v = bf2f(hi) + bf2f(lo);
      dz[i] = v;
    }
    a = fmaf(z[i], v, a);
  }
  a = wave_sum(a);
  if (lane == 0) r[bh] = a;
}

// ---------------------------------------------------------------------------------------------------------
// pass 1: dl[b][h][s] = p (x[b,s] . dz[b,h] - r[b,h]),  p = exp(logit - max) / sum as the forward forms it
// ---------------------------------------------------------------------------------------------------------
struct StoreDl {
  const float* __restrict__ logits;
  const float* __restrict__ stats;
  const float* __restrict__ r;
  float* __restrict__ dl;
  __device__ __forceinline__ void operator()(int64_t gh, int64_t idx, float dp) const {
    dl[idx] = softmax_p(logits, stats, gh, idx) * (dp - r[gh]);
  }
  // a padded token's logit is the constant kPadLogit: nothing flows through it to U, whatever p is (exactly 0
  // beside a valid token, 1 / S in a clip of padded tokens alone), and dp is never formed
  __device__ __forceinline__ void dead(int64_t, int64_t idx) const { dl[idx] = 0.0f; }
};

// pool_stream.h pass 1 with the operand of the workgroup's (wave's) clip: dz [B][H][D], dzt [B][32][D]
template <int NJ>
__global__ __launch_bounds__(256) void probe_dl_kernel(const void* __restrict__ x, int in_bf16, int S, int D,
                                                       const float* __restrict__ dz, int H,
                                                       const float* __restrict__ logits,
                                                       const float* __restrict__ stats, const float* __restrict__ r,
                                                       float* __restrict__ dl) {
  pool_scalar_pass<NJ, true>(x, in_bf16, 0, S, D, dz, H, StoreDl{logits, stats, r, dl});
}

__global__ __launch_bounds__(256) void probe_dl_mfma_kernel(const bf16_t* __restrict__ x, int64_t rows, int S, int D,
                                                            const bf16_t* __restrict__ dzt, int H,
                                                            const float* __restrict__ logits,
                                                            const float* __restrict__ stats,
                                                            const float* __restrict__ r, float* __restrict__ dl) {
  pool_mfma_pass<true>(x, rows, S, D, dzt, H, StoreDl{logits, stats, r, dl});
}

// the same under token paddings pad [B][S]: every padded row is dead in the backward (pool_stream.h, PadRows)
template <int NJ>
__global__ __launch_bounds__(256) void probe_dl_masked_kernel(const void* __restrict__ x, int in_bf16, int S, int D,
                                                              const float* __restrict__ dz, int H,
                                                              const float* __restrict__ logits,
                                                              const float* __restrict__ stats,
                                                              const float* __restrict__ r,
                                                              const float* __restrict__ pad,
                                                              float* __restrict__ dl) {
  pool_scalar_pass<NJ, true>(x, in_bf16, 0, S, D, dz, H, StoreDl{logits, stats, r, dl}, PadRows{pad});
}

__global__ __launch_bounds__(256) void probe_dl_mfma_masked_kernel(const bf16_t* __restrict__ x, int64_t rows, int S,
                                                                   int D, const bf16_t* __restrict__ dzt, int H,
                                                                   const float* __restrict__ logits,
                                                                   const float* __restrict__ stats,
                                                                   const float* __restrict__ r,
                                                                   const float* __restrict__ pad,
                                                                   float* __restrict__ dl) {
  pool_mfma_pass<true>(x, rows, S, D, dzt, H, StoreDl{logits, stats, r, dl}, PadRows{pad});
}

// ---------------------------------------------------------------------------------------------------------
// pass 2: part[g][c][h][d] = sum over the rows of chunk c of dl[g,h,s] x[g*S+s][d]: pool_stream.h pass 2 with the
// signed weights read as they are, the [256][16] weights visited by head (consecutive threads read consecutive s)
// ---------------------------------------------------------------------------------------------------------
struct FillDl {
  static constexpr bool kByRow = false;
  const float* __restrict__ dl;
  __device__ __forceinline__ float operator()(int64_t, int64_t idx) const { return dl[idx]; }
};

__global__ __launch_bounds__(128) void probe_wsum_kernel(const void* __restrict__ x, int in_bf16, int S, int D, int H,
                                                         const float* __restrict__ dl, int C,
                                                         float* __restrict__ part) {
  pool_wsum_pass(x, in_bf16, S, D, H, C, FillDl{dl}, part);
}

// under token paddings: dl is exactly 0 at the padded rows, which are neither loaded nor summed
__global__ __launch_bounds__(128) void probe_wsum_masked_kernel(const void* __restrict__ x, int in_bf16, int S, int D,
                                                                int H, const float* __restrict__ dl,
                                                                const float* __restrict__ pad, int C,
                                                                float* __restrict__ part) {
  pool_wsum_pass(x, in_bf16, S, D, H, C, FillDl{dl}, part, PadRows{pad});
}

// ---------------------------------------------------------------------------------------------------------
// fold backward
// ---------------------------------------------------------------------------------------------------------
// dWk[d][h][j] = dU[h][d] q~[h][j]
__global__ __launch_bounds__(256) void probe_dwk_kernel(const float* __restrict__ dU, const float* __restrict__ qt,
                                                        int D, int H, int dh, float* __restrict__ dwk) {
  const int64_t HJ = (int64_t)H * dh;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= D * HJ) return;
  const int64_t d = i / HJ, hj = i % HJ;
  dwk[i] = dU[(hj / dh) * D + d] * qt[hj];
}

// q~ = qraw c softplus(pds): dqraw[h][j] = dq~ c softplus(pds[j]) (= dbq), dpds[j] = c sigmoid(pds[j]) sum_h dq~ qraw
__global__ __launch_bounds__(256) void probe_dq_kernel(const float* __restrict__ dqt, const float* __restrict__ qraw,
                                                       const float* __restrict__ pds, int H, int dh, float c,
                                                       float* __restrict__ dqraw, float* __restrict__ dpds) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= dh) return;
  const float x = pds[j];
  const float sp = c * softplus(x);
  float s = 0.0f;
  for (int h = 0; h < H; ++h) {
    const float g = dqt[h * dh + j];
    dqraw[h * dh + j] = g * sp;
    s = fmaf(g, qraw[h * dh + j], s);
  }
  dpds[j] = c * s / (1.0f + expf(-x));
}

}  // namespace

hipError_t probe_fold(float* qraw, const float* bq, const float* pds, const float* Wk, int D, int H, int split,
                      float* qt, float* U, bf16_t* Ut, hipStream_t s) {
  if (D < 1 || H < 1 || D % H) return hipErrorInvalidValue;
  const int dh = D / H;
  const float c = (float)(1.442695041 / sqrt((double)dh));
  hipLaunchKernelGGL(probe_fold_q_kernel, dim3((D + 255) / 256), dim3(256), 0, s, qraw, bq, pds, D, dh, c, qt);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  if (split && (e = hipMemsetAsync(Ut, 0, (size_t)32 * D * sizeof(bf16_t), s)) != hipSuccess) return e;
  hipLaunchKernelGGL(probe_fold_u_kernel, dim3(D), dim3(256), 0, s, Wk, qt, D, H, dh, split, U, Ut);
  return hipGetLastError();
}

hipError_t probe_pack(const float* wv, const float* wp, const float* scale, int D, int H, float* wvt, float* wpt,
                      float* gamma, hipStream_t s) {
  if (D < 1 || H < 1 || D % H) return hipErrorInvalidValue;
  const int64_t n = (int64_t)D * D;
  hipLaunchKernelGGL(probe_pack_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, wv, wp, scale, D, H, D / H,
                     wvt, wpt, gamma);
  return hipGetLastError();
}

hipError_t probe_gemm(const float* A, int64_t sA, int64_t am, int64_t ak, const float* Bm, int64_t sB, int64_t bk,
                      float* out, int64_t sO, int64_t ldo, int M, int N, int K, int batch, hipStream_t s) {
  if (M < 1 || N < 1 || K < 1 || batch < 1 || batch > 65535 || (M + kPgM - 1) / kPgM > 65535)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(probe_gemm_kernel, dim3((N + kPgN - 1) / kPgN, (M + kPgM - 1) / kPgM, batch), dim3(64 * kPgS), 0, s,
                     A, sA, am, ak, Bm, sB, bk, out, sO, ldo, M, N, K);
  return hipGetLastError();
}

hipError_t probe_dot(const float* A, int64_t sA, int64_t am, const float* Bm, int64_t sB, int64_t bn, float* out,
                     int64_t sO, int64_t ldo, int M, int N, int K, int batch, hipStream_t s) {
  if (M < 1 || N < 1 || K < 1 || batch < 1 || batch > 65535) return hipErrorInvalidValue;
  hipLaunchKernelGGL(probe_dot_kernel, dim3((N + 3) / 4, 1, batch), dim3(256), 0, s, A, sA, am, Bm, sB, bn, out, sO, ldo,
                     M, N, K);
  return hipGetLastError();
}

hipError_t probe_colsum(const float* x, int M, int N, float* out, hipStream_t s) {
  if (M < 1 || N < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(probe_colsum_kernel, dim3((N + 255) / 256), dim3(256), 0, s, x, M, N, out);
  return hipGetLastError();
}

hipError_t probe_ln_bwd(const float* x, const float* dy, const float* gamma, int rows, int D, float* dx, float* stats,
                        float* dscale, float* dbias, hipStream_t s) {
  if (D < 1 || D > kPoolMaxD || rows < 1) return hipErrorInvalidValue;
  if (D <= 1024)
    hipLaunchKernelGGL(probe_ln_bwd_kernel<4>, dim3(rows), dim3(256), 0, s, x, dy, gamma, D, dx, stats);
  else
    hipLaunchKernelGGL(probe_ln_bwd_kernel<6>, dim3(rows), dim3(256), 0, s, x, dy, gamma, D, dx, stats);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(probe_ln_param_kernel, dim3((D + 255) / 256), dim3(256), 0, s, x, dy, stats, rows, D, dscale,
                     dbias);
  return hipGetLastError();
}

hipError_t probe_dz_finish(const float* z, float* dz, int B, int H, int D, int split, bf16_t* dzt, float* r,
                           hipStream_t s) {
  if (B < 1 || H < 1 || H > kPoolMaxH || D < 1) return hipErrorInvalidValue;
  hipError_t e;
  if (split && (e = hipMemsetAsync(dzt, 0, (size_t)B * 32 * D * sizeof(bf16_t), s)) != hipSuccess) return e;
  hipLaunchKernelGGL(probe_dz_finish_kernel, dim3((B * H + 3) / 4), dim3(256), 0, s, z, dz, B * H, H, D, split, dzt, r);
  return hipGetLastError();
}

bool probe_dl_uses_mfma(int in_bf16, int S) { return in_bf16 && S % 32 == 0; }

hipError_t probe_dl(const void* x, int in_bf16, int B, int S, int D, int H, const float* dz, const bf16_t* dzt,
                    const float* logits, const float* stats, const float* r, float* dl, hipStream_t s,
                    const float* pad) {
  if (D % 64 || D > kPoolMaxD || H < 1 || H > kPoolMaxH || B < 1 || S < 1 || B > 65535) return hipErrorInvalidValue;
  if (probe_dl_uses_mfma(in_bf16, S) && dzt) {
    const int64_t rows = (int64_t)B * S;
    const int64_t grid = (rows / 32 + 3) / 4;
    if (pad)
      hipLaunchKernelGGL(probe_dl_mfma_masked_kernel, dim3((unsigned)grid), dim3(256), 0, s, (const bf16_t*)x, rows, S,
                         D, dzt, H, logits, stats, r, pad, dl);
    else
      hipLaunchKernelGGL(probe_dl_mfma_kernel, dim3((unsigned)grid), dim3(256), 0, s, (const bf16_t*)x, rows, S, D, dzt,
                         H, logits, stats, r, dl);
    return hipGetLastError();
  }
  if (pad)
    return launch_pool_scalar(&probe_dl_masked_kernel<16>, &probe_dl_masked_kernel<24>,
                              dim3((S + kPlRows - 1) / kPlRows, B), D, H, s, x, in_bf16, S, D, dz, H, logits, stats, r,
                              pad, dl);
  return launch_pool_scalar(&probe_dl_kernel<16>, &probe_dl_kernel<24>, dim3((S + kPlRows - 1) / kPlRows, B), D, H, s, x,
                            in_bf16, S, D, dz, H, logits, stats, r, dl);
}

hipError_t probe_wsum(const void* x, int in_bf16, int B, int S, int D, int H, const float* dl, float* part,
                      float* dUclip, float* dU, hipStream_t s, const float* pad) {
  if (D % 128 || D > kPoolMaxD || H < 1 || H > kPoolMaxH || B < 1 || S < 1) return hipErrorInvalidValue;
  const int C = (S + kPwRows - 1) / kPwRows;
  if (pad)
    hipLaunchKernelGGL(probe_wsum_masked_kernel, dim3(B * C * ((D + 255) / 256)), dim3(128), 0, s, x, in_bf16, S, D, H,
                       dl, pad, C, part);
  else
    hipLaunchKernelGGL(probe_wsum_kernel, dim3(B * C * ((D + 255) / 256)), dim3(128), 0, s, x, in_bf16, S, D, H, dl, C,
                       part);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  // over the chunks of each clip, then over the clips: B times the workgroups of one sweep over all B * C partials
  const int64_t HD = (int64_t)H * D;
  if ((e = pool_reduce(part, C, HD, B, dUclip, s)) != hipSuccess) return e;
  return pool_reduce(dUclip, B, HD, 1, dU, s);
}

hipError_t probe_fold_bwd(const float* dU, const float* qt, int D, int H, float* dwk, hipStream_t s) {
  if (D < 1 || H < 1 || D % H) return hipErrorInvalidValue;
  const int64_t n = (int64_t)D * D;
  hipLaunchKernelGGL(probe_dwk_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, dU, qt, D, H, D / H, dwk);
  return hipGetLastError();
}

hipError_t probe_dq(const float* dqt, const float* qraw, const float* pds, int D, int H, float* dqraw, float* dpds,
                    hipStream_t s) {
  if (D < 1 || H < 1 || D % H) return hipErrorInvalidValue;
  const int dh = D / H;
  const float c = (float)(1.442695041 / sqrt((double)dh));
  hipLaunchKernelGGL(probe_dq_kernel, dim3((dh + 255) / 256), dim3(256), 0, s, dqt, qraw, pds, H, dh, c, dqraw, dpds);
  return hipGetLastError();
}

}  // namespace vp
