// The pooler's two streaming passes over the tokens, written once for the forward (clip_kernels.hip: logits, then
// the softmax-weighted sum z) and the head's backward (probe_kernels.hip: dl, then dU), with the reductions and the
// row statistics both files use.  A .hip file defines thin __global__ kernels that name a functor; the body, its
// width rules and its summation order are here and only here.
//
// Pass 1, out[g][h][s] = f(x[g*S+s] . B[h]) with B [H][D] shared by all clips (U) or one per clip (dz[g]):
//  * pool_mfma_pass (bf16 tokens, S % 32 == 0): a skinny GEMM on v_mfma_f32_32x32x16_bf16.  A wave owns 32 rows,
//    which lie in one clip; the B operand is Bt [32][D] bf16 = (B_hi | B_lo | 0) with B = B_hi + B_lo, so the fp32
//    operand survives bf16 to ~2^-16 relative.  Lane l has column i = l & 31 and half = l >> 5, and after the k loop
//    (D / 16 MFMAs in k order, loads batched 8 deep) acc[q] = C[row = (q&3) + 8(q>>2) + 4*half][col = i]; lane
//    i < H adds column H + i (the lo half) and stores.
//  * pool_scalar_pass (fp32 tokens, or S % 32 != 0): B [H][D] in dynamic LDS whole, D = 64 k; a workgroup owns
//    kPlRows rows (16 per wave), a lane keeps a row's NJ 64-column steps in registers (NJ = 16 up to D = 1024, the
//    kernel every width up to Large runs, or 24 up to kPoolMaxD; 22 steps at Giant's 1408) and sums each head as a
//    per-lane fmaf chain over j, then the wave_sum butterfly.  Past 64 KB (16 heads x 1408 columns are 90,112 B)
//    launch_pool_scalar opts in to the larger allocation, as the 88-wide fp32 attention kernel does.
// A store functor receives (gh = g*H + h, idx = gh*S + s, v) and writes what its pass writes.  Functors are plain
// structs passed by value and the operand's kind is a compile-time flag: with the kernels' own __restrict__
// parameters that leaves every kernel at or under its hand-written VGPR count (profiles/pool_stream/asm_identity.txt).
//
// Pass 2, part[g][c][h][d] = sum over the rows of chunk c of w[g,h,s] x[g*S+s][d] (pool_wsum_pass): a workgroup
// owns one (g, kPwRows-row chunk, 256-column block) with 128 threads; a thread owns two adjacent columns (one 4-byte
// bf16 pair / 8-byte fp32 pair per row) and all 16 head sums of each, the chunk's weights sit in LDS (float4
// broadcast reads), rows are loaded 16 deep and summed in row order.  D = 128 k; with k odd (1408 = 5 x 256 + 128)
// the last column block is 128 wide: its second wave fills its share of the weights and leaves, so no lane reads or
// writes a column past D and x is still read once.  A fill functor gives the weight of (gh, idx) and the order in
// which the [256][16] LDS entries are visited (by row: consecutive threads take the heads of one row; by head:
// consecutive threads read consecutive s).  The chunk sums are then added in index order (pool_reduce, vp_kernels.h).
//
// Token paddings (layers.py:1103-1106; pad [G][S] fp32, a token is padded iff its value is > 0.5) are a third
// compile-time piece, a row mask passed by value like the functors.  A masked pass asks it which rows are dead and
// never reads a dead row of x: pass 1 calls store.dead(gh, idx) for it instead of store(gh, idx, v) (a wave of the
// scalar pass skips the row's loads, a wave of the MFMA pass whose 32 rows are all dead skips its k loop), pass 2
// keeps one bit per row of the chunk beside the weights and skips the dead rows' loads and FMAs (a chunk with no live
// row fills no weights either and stores zeros), so NaN or Inf in a dead row reaches no sum.  The rows that are
// summed are summed in the row order of the unmasked pass.  PadRows calls every padded row dead; it serves
// the forward's pass 1 (a padded token's logit is the constant kPadLogit whatever the token holds)
// and both passes of the backward (nothing flows through a constant logit to U, so dl is exactly 0 there).  DeadRows
// (the forward's pass 2) calls a padded row dead only in a clip with a valid token, where its probability is
// exactly 0; in a clip whose tokens are all padded the softmax is uniform over all of them, as in the reference:
// every token counts in z and no row is dead.  NoMask is the unmasked pass, instruction for instruction the one
// without the parameter.
#pragma once
#include <type_traits>

#include "vp_common.h"
#include "vp_kernels.h"

namespace vp {

namespace {

__device__ __forceinline__ float ldx(const void* p, int in_bf16, int64_t i) {
  return in_bf16 ? bf2f(static_cast<const bf16_t*>(p)[i]) : static_cast<const float*>(p)[i];
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  return v;
}

// block (256 threads) reductions through LDS
__device__ __forceinline__ float block_sum(float v, float* red) {
  v = wave_sum(v);
  const int w = threadIdx.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[w] = v;
  __syncthreads();
  return red[0] + red[1] + red[2] + red[3];
}

__device__ __forceinline__ float block_max(float v, float* red) {
  v = wave_max(v);
  const int w = threadIdx.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[w] = v;
  __syncthreads();
  return fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

// LayerNorm's statistics (layers.py:208-270, eps 1e-6) of the row a 256-thread workgroup holds as v[j] = column
// threadIdx.x + 256 j, zero past D
template <int NV>
__device__ __forceinline__ void ln_row_stats(const float (&v)[NV], int D, float* red, float& mean, float& rstd) {
  float s = 0.0f;
#pragma unroll
  for (int j = 0; j < NV; ++j) s += v[j];
  mean = block_sum(s, red) / (float)D;
  float q = 0.0f;
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const int d = threadIdx.x + 256 * j;
    const float c = d < D ? v[j] - mean : 0.0f;
    q = fmaf(c, c, q);
  }
  rstd = rsqrtf(block_sum(q, red) / (float)D + 1e-6f);
}

// p[g,h,s] of the fp32 softmax (layers.py:650-654) from its logit and stats [G*H][2] = (max, 1 / sum exp(l - max))
__device__ __forceinline__ float softmax_p(const float* __restrict__ logits, const float* __restrict__ stats,
                                           int64_t gh, int64_t idx) {
  return __expf(logits[idx] - stats[2 * gh]) * stats[2 * gh + 1];
}

// what a padded token's logit becomes before the softmax: the reference's -0.7 * finfo(float32).max
constexpr float kPadLogit = -0.7f * 3.402823466e+38f;

__device__ __forceinline__ bool is_padded(const float* __restrict__ pad, int64_t row) { return !(pad[row] <= 0.5f); }

struct NoMask {
  static constexpr bool kMasked = false;
  __device__ __forceinline__ bool operator()(int64_t, int64_t) const { return false; }
};

// every padded row (g: clip, row = g*S + s)
struct PadRows {
  static constexpr bool kMasked = true;
  const float* __restrict__ pad;
  __device__ __forceinline__ bool operator()(int64_t, int64_t row) const { return is_padded(pad, row); }
};

// the padded rows of a clip with a valid token.  stats [G*H][2] are the forward's: the maximum of a clip's logits
// is kPadLogit, in every head, iff all of its tokens are padded
struct DeadRows {
  static constexpr bool kMasked = true;
  const float* __restrict__ pad;
  const float* __restrict__ stats;
  int H;
  __device__ __forceinline__ bool operator()(int64_t g, int64_t row) const {
    return is_padded(pad, row) && stats[2 * g * H] != kPadLogit;
  }
};

template <bool PER_CLIP, class Store, class Mask = NoMask>
__device__ __forceinline__ void pool_mfma_pass(const bf16_t* x, int64_t rows, int S, int D,
                                               const bf16_t* Bt, int H, Store store, Mask mask = {}) {
  const int lane = threadIdx.x & 63;
  const int64_t r0 = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * 32;
  if (r0 >= rows) return;  // whole wave
  const int i = lane & 31, half = lane >> 5;
  uint32_t dead = 0;  // bit j: row r0 + j
  if constexpr (Mask::kMasked) dead = (uint32_t)__ballot(mask(r0 / S, r0 + i));
  const bf16_t* ap = x + (r0 + i) * D + 8 * half;
  const bf16_t* bp = Bt + ((PER_CLIP ? r0 / S * 32 : 0) + i) * D + 8 * half;
  f32x16 acc = {};
  const int nt = D >> 4;
  int t = Mask::kMasked && dead == 0xffffffffu ? nt : 0;  // (uniform) no row of the wave is read
  for (; t + 8 <= nt; t += 8) {
    bf16x8 a[8], b[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      a[u] = *reinterpret_cast<const bf16x8*>(ap + 16 * (t + u));
      b[u] = *reinterpret_cast<const bf16x8*>(bp + 16 * (t + u));
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[u], b[u], acc, 0, 0, 0);
  }
  for (; t < nt; ++t) {
    const bf16x8 a = *reinterpret_cast<const bf16x8*>(ap + 16 * t);
    const bf16x8 b = *reinterpret_cast<const bf16x8*>(bp + 16 * t);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc, 0, 0, 0);
  }
  const int64_t g = r0 / S;
  const int64_t s0 = r0 % S;
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    const float v = acc[q] + __shfl_down(acc[q], H);
    if (i < H) {
      const int64_t gh = g * H + i;
      const int64_t idx = gh * S + s0 + (q & 3) + 8 * (q >> 2) + 4 * half;
      if constexpr (Mask::kMasked) {
        if (dead >> ((q & 3) + 8 * (q >> 2) + 4 * half) & 1) store.dead(gh, idx);
        else store(gh, idx, v);
      } else {
        store(gh, idx, v);
      }
    }
  }
}

constexpr int kPlRows = 64;  // rows per workgroup of the scalar pass (16 per wave)

// Shared B: a flat grid over the rows, and lane 0 stores each head's sum as it completes.  Per clip: grid
// (ceil(S / kPlRows), G), and lane h keeps head h's sum, so the H lanes run the store functor once per row.
template <int NJ, bool PER_CLIP, class Store, class Mask = NoMask>
__device__ __forceinline__ void pool_scalar_pass(const void* x, int in_bf16, int64_t rows, int S, int D,
                                                 const float* Bm, int H, Store store, Mask mask = {}) {
  extern __shared__ float Bs[];  // [H][D]
  if constexpr (PER_CLIP) Bm += (int64_t)blockIdx.y * H * D;
  for (int i = threadIdx.x; i < H * D; i += 256) Bs[i] = Bm[i];
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int w = threadIdx.x >> 6;
  const int nj = D >> 6;
  for (int rr = 0; rr < kPlRows / 4; ++rr) {
    const int64_t in = (int64_t)blockIdx.x * kPlRows + w * (kPlRows / 4) + rr;  // row of the clip / of x
    if (in >= (PER_CLIP ? S : rows)) break;  // uniform per wave
    const int64_t r = PER_CLIP ? (int64_t)blockIdx.y * S + in : in;
    if constexpr (Mask::kMasked) {
      const int64_t gm = PER_CLIP ? blockIdx.y : r / S;
      if (mask(gm, r)) {  // uniform per wave: the row is not loaded
        if (lane < H) store.dead(gm * H + lane, (gm * H + lane) * S + (PER_CLIP ? in : r % S));
        continue;
      }
    }
    float xv[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) xv[j] = j < nj ? ldx(x, in_bf16, r * D + lane + 64 * j) : 0.0f;
    const int64_t g = PER_CLIP ? blockIdx.y : r / S, s = PER_CLIP ? in : r % S;  // (the division under the loads)
    float mine = 0.0f;
    for (int h = 0; h < H; ++h) {
      float a = 0.0f;
#pragma unroll
      for (int j = 0; j < NJ; ++j)
        if (j < nj) a = fmaf(xv[j], Bs[h * D + lane + 64 * j], a);
      a = wave_sum(a);
      if constexpr (PER_CLIP) {
        if (lane == h) mine = a;
      } else if (lane == 0) {
        store(g * H + h, (g * H + h) * S + s, a);
      }
    }
    if (PER_CLIP && lane < H) store(g * H + lane, (g * H + lane) * S + s, mine);
  }
}

// launches k16 (NJ = 16) up to D = 1024 and k24 (NJ = 24) past it, B [H][D] in dynamic LDS
template <class K, class... Args>
hipError_t launch_pool_scalar(K k16, K k24, dim3 grid, int D, int H, hipStream_t s, Args... args) {
  const size_t lds = (size_t)H * D * 4;
  if (D > 1024 && lds > 65536) {  // up to 16 x 1536 x 4 = 98,304 B of the CU's 160 KB
    const hipError_t e = ensure_dyn_lds(reinterpret_cast<const void*>(k24), kPoolMaxH * kPoolMaxD * 4);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(D <= 1024 ? k16 : k24, grid, dim3(256), lds, s, args...);
  return hipGetLastError();
}

constexpr int kPwRows = 256;  // rows per chunk of pass 2

template <class Fill, class Mask = NoMask>
__device__ __forceinline__ void pool_wsum_pass(const void* x, int in_bf16, int S, int D, int H, int C,
                                               Fill fill, float* part, Mask mask = {}) {
  __shared__ __attribute__((aligned(16))) float ws[kPwRows][kPoolMaxH];
  uint64_t* dead = nullptr;  // bit r & 63 of dead[r >> 6]: row r of the chunk
  if constexpr (Mask::kMasked) {
    __shared__ uint64_t bits[kPwRows / 64];
    dead = bits;
  }
  const int nq = (D + 255) >> 8;
  const int q = blockIdx.x % nq;
  const int gc = blockIdx.x / nq;
  const int g = gc / C;
  const int c = gc % C;
  const int r0 = c * kPwRows;
  const int nr = S - r0 < kPwRows ? S - r0 : kPwRows;
  bool live = true;  // (uniform) some row of the chunk is summed
  if constexpr (Mask::kMasked) {
    for (int r = threadIdx.x; r < kPwRows; r += 128) {
      const uint64_t m = __ballot(r < nr && mask(g, (int64_t)g * S + r0 + r));
      if ((threadIdx.x & 63) == 0) dead[r >> 6] = m;
    }
    __syncthreads();
    int some = 0;
#pragma unroll
    for (int j = 0; j < kPwRows / 64; ++j) {
      const int n = nr - 64 * j;  // rows of the chunk in word j
      some |= dead[j] != (n >= 64 ? ~0ull : n > 0 ? (1ull << n) - 1 : 0ull);
    }
    live = __builtin_amdgcn_readfirstlane(some);  // else: no weight is filled, no row is read, the sums are zeros
  }
  if (live) {
    for (int i = threadIdx.x; i < kPwRows * kPoolMaxH; i += 128) {
      const int r = Fill::kByRow ? i / kPoolMaxH : i % kPwRows;
      const int h = Fill::kByRow ? i % kPoolMaxH : i / kPwRows;
      float p = 0.0f;
      if (r < nr && h < H) {
        const int64_t gh = (int64_t)g * H + h;
        p = fill(gh, gh * S + r0 + r);
      }
      ws[r][h] = p;
    }
  }
  __syncthreads();
  const int d = q * 256 + 2 * threadIdx.x;
  if (d >= D) return;  // the half block's second wave, whole
  float acc0[kPoolMaxH], acc1[kPoolMaxH];
#pragma unroll
  for (int h = 0; h < kPoolMaxH; ++h) acc0[h] = acc1[h] = 0.0f;
  const int64_t rowbase = (int64_t)g * S + r0;
  auto ld2 = [&](int r) -> float2 {
    const int64_t i = (rowbase + r) * D + d;
    if (in_bf16) {
      const uint32_t u = *reinterpret_cast<const uint32_t*>(static_cast<const bf16_t*>(x) + i);
      return make_float2(__uint_as_float(u << 16), __uint_as_float(u & 0xffff0000u));
    }
    return *reinterpret_cast<const float2*>(static_cast<const float*>(x) + i);
  };
  auto row = [&](int r, float2 xv) {
    const float4* pr = reinterpret_cast<const float4*>(ws[r]);
#pragma unroll
    for (int h4 = 0; h4 < kPoolMaxH / 4; ++h4) {
      const float4 p = pr[h4];
      acc0[4 * h4] = fmaf(p.x, xv.x, acc0[4 * h4]);
      acc0[4 * h4 + 1] = fmaf(p.y, xv.x, acc0[4 * h4 + 1]);
      acc0[4 * h4 + 2] = fmaf(p.z, xv.x, acc0[4 * h4 + 2]);
      acc0[4 * h4 + 3] = fmaf(p.w, xv.x, acc0[4 * h4 + 3]);
      acc1[4 * h4] = fmaf(p.x, xv.y, acc1[4 * h4]);
      acc1[4 * h4 + 1] = fmaf(p.y, xv.y, acc1[4 * h4 + 1]);
      acc1[4 * h4 + 2] = fmaf(p.z, xv.y, acc1[4 * h4 + 2]);
      acc1[4 * h4 + 3] = fmaf(p.w, xv.y, acc1[4 * h4 + 3]);
    }
  };
  if constexpr (Mask::kMasked) {
    // The same row loops under the dead bits.  The bits of 16 rows sit in a scalar register, so the branches on them
    // are uniform; the token type is hoisted out of the loops and a row is converted where it is summed, not where it
    // is loaded, so the live loads of a batch are all in flight before the first wait, as in the unmasked loop.
    auto sweep = [&](auto bf) {
      constexpr bool kBf = decltype(bf)::value;
      auto dead16 = [&](int r) -> uint32_t {  // rows r .. r + 15, r % 16 == 0
        return __builtin_amdgcn_readfirstlane((uint32_t)(dead[r >> 6] >> (r & 63)) & 0xffffu);
      };
      auto ldr = [&](int r) -> uint2 {
        const int64_t i = (rowbase + r) * D + d;
        if constexpr (kBf) return make_uint2(*reinterpret_cast<const uint32_t*>(static_cast<const bf16_t*>(x) + i), 0u);
        else return *reinterpret_cast<const uint2*>(static_cast<const float*>(x) + i);
      };
      auto cvt = [&](uint2 u) -> float2 {
        if constexpr (kBf) return make_float2(__uint_as_float(u.x << 16), __uint_as_float(u.x & 0xffff0000u));
        else return make_float2(__uint_as_float(u.x), __uint_as_float(u.y));
      };
      int r = 0;
      for (; r + 16 <= nr; r += 16) {
        const uint32_t m = dead16(r);
        if (m == 0xffffu) continue;
        uint2 raw[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) raw[u] = m >> u & 1 ? make_uint2(0u, 0u) : ldr(r + u);
#pragma unroll
        for (int u = 0; u < 16; ++u)
          if (!(m >> u & 1)) row(r + u, cvt(raw[u]));
      }
      const uint32_t m = r < nr ? dead16(r) : 0;
      for (; r < nr; ++r)
        if (!(m >> (r & 15) & 1)) row(r, cvt(ldr(r)));
    };
    if (live) {
      if (in_bf16) sweep(std::true_type{});
      else sweep(std::false_type{});
    }
  } else {
    int r = 0;
    for (; r + 16 <= nr; r += 16) {
      float2 xv[16];
#pragma unroll
      for (int u = 0; u < 16; ++u) xv[u] = ld2(r + u);
#pragma unroll
      for (int u = 0; u < 16; ++u) row(r + u, xv[u]);
    }
    for (; r < nr; ++r) row(r, ld2(r));
  }
  float* zp = part + ((int64_t)g * C + c) * H * D + d;
#pragma unroll
  for (int h = 0; h < kPoolMaxH; ++h)
    if (h < H) *reinterpret_cast<float2*>(zp + (int64_t)h * D) = make_float2(acc0[h], acc1[h]);
}

}  // namespace

}  // namespace vp
