// Exact top-k search of a device-resident gallery of embeddings (vp_op_topk / vp_op_topk_merge; DESIGN.md §4
// "Gallery search").  Two kernels, no atomics, no [N, Q] matrix:
//
// topk_scan_kernel<BF16>: grid (parts, query groups), 512 threads.  A workgroup owns one group of G queries (32, or 16
// where 32 do not fit the 160 KB of LDS: topk_group) and one contiguous range of gallery rows, which it walks in
// ascending order in tiles of kTkRows = 512 rows (a wave: 64 rows as two 32-row MFMA tiles).
//  * Scores: the gallery tile is the A operand and the queries are B, so lane l = (i = l & 31, half = l >> 5) holds
//    query i's column and acc[q] = score(row (q & 3) + 8 (q >> 2) + 4 half, query i).  A lane loads 16 B of row i per
//    step straight from memory (the two halves cover 32 B of the row; 4 steps per batch, the next batch in flight under
//    the MFMAs); the queries sit in LDS in fragment order, written once per workgroup.
//      fp32 gallery: v_mfma_f32_32x32x2_f32, four per step, element e of the lane's 16 B against the same element of
//        the query's (k = 8 t + 4 half + e): an exact fmaf chain, the k order permuted alike for every pair.
//      bf16 gallery: v_mfma_f32_32x32x16_bf16 twice per step, against hi = bf16(q) and then lo = bf16(q - hi): the
//        gallery's rounding is the only quantisation left.
//    Every (query, row) pair gets the same instructions in the same order whatever N, Q, ld, the grid, the tile or the
//    lane, so a score is a function of the two vectors alone.  Rows past the range are never read (their lanes load
//    nothing and multiply zeros) and never selected.
//  * Selection: each query's best k so far in LDS, unordered but for the last slot, which holds the worst of them (the
//    k-th score).  A lane compares its 32 accumulators with its query's k-th score; a wave whose ballot finds no better
//    score is done with the tile.  Otherwise the waves insert one after the other (rows ascend from wave to wave), each
//    wave row by row (a ballot per 8 rows, then per row): a lane holding a better score overwrites the worst entry,
//    finds the new worst in one pass over the list and both of the query's lanes re-read it; the list is ordered once,
//    by counting, when it is written out.  Rows arrive in ascending
//    order, so `score > k-th` is the whole order rule: an equal score with a larger id never displaces, and a NaN or
//    -inf compares false against the initial -inf.  Expected inserts per query and range: about k ln(n / k).
//  * Output: lists [part][Q][k] of (score, id_base + row), padded with (-inf, -1).
//
// topk_merge_kernel: one workgroup per query merges `parts` sorted lists into the best k: L - 1 lists at a time join the
// running result in LDS and a tree of pairwise merges halves them; an element's place in a pair's output is its index
// plus the number of the other list's elements that come before it (binary search; on a full tie the even list first),
// so every output slot is written by exactly one thread.  The order (score descending, id ascending, padding last) is
// total, which makes the result independent of how the rows were split into lists.
//
// The grouped search (vp_op_topk_groups*; DESIGN.md §4 "Grouped gallery search") is topk_scan_kernel<BF16, true>, the
// same text with a label per list entry, and topk_groups_merge_kernel.  Scores, tiling, the pre-check against the k-th
// score and the waves' turns are shared; only the insert differs: a lane that beats the k-th score reads its row's
// label (a negative one is skipped) and looks for it in the list during the walk that finds the worst entry.  A group
// that is there with a score not smaller stays as it is, one with a smaller score is overwritten in place, and
// otherwise the worst entry goes, as above.  The k-th score only rises and a group leaves a list only when k others
// beat it, so the list is the best k groups of the rows seen, each with its best row (of equal scores the first).
// The labels of a lane's candidates in a tile are read together, and of candidates that follow one another in a lane
// with the same label only the best keeps its turn (tk_insert).
//
// The masked search (vp_op_topk_masked / vp_op_topk_groups_masked; DESIGN.md §4 "Masked search") is
// topk_scan_kernel<BF16, GROUPED, true>, again the same text.  The mask is packed bits, bit r & 31 of word r >> 5 set
// where row r is allowed; a 32-row MFMA tile is one word and a wave's 64 rows are two, read one tile ahead.  One mask
// serves all queries (stride 0: every lane reads the same two words) or each query has its own (lane l reads query
// l & 31's).  After the MFMAs and before the pre-check a lane sets the accumulators of rows its query does not allow
// to -inf, which no comparison of the selection passes; the instructions that form a score are the unmasked ones, so
// an allowed row's score has the unmasked search's bits and the lists are those of a gallery of the allowed rows
// alone.  A wave none of whose queries allows any of its 64 rows skips the tile's loads and MFMAs; under the shared
// mask a row that is not allowed is not loaded either.  So that such savings shorten the search and not only some
// workgroups' share of it, the masked scan deals the 512-row tiles to the workgroups in turn (workgroup x of P takes
// tiles x, x + P, ...) where the unmasked one gives each a contiguous range: a workgroup's rows still ascend, and the
// merge does not care how the rows were split.  Bits of rows past N are never looked at (every use of a score
// is behind `row < p1`) and no word past ceil(N / 32) per mask is read.  rowmask_pack_kernel makes the words from one
// byte per row, a ballot per 64 rows.
//
// The fp8 gallery (vp_op_topk*_f8; DESIGN.md §4 "fp8 gallery") is topk_scan_kernel<kTkF8, GROUPED, MASKED>: the first
// template argument names the storage, fp32, bf16 or fp8, where it was a bool.  A row is D OCP e4m3 codes and one fp32
// scale, a power of two, and stands for codes * scale, every value exactly a bf16.  A lane's 16-byte load is 16 codes of
// its row (a step is 32 elements, the query fragments are laid out for that), v_cvt_scalef32_pk_bf16_fp8 turns them and
// the row's scale into two bf16x8 operands exactly, and each goes through the bf16 gallery's two MFMAs against the hi
// and lo fragments: the storage rounding is again the only quantisation, and everything after the scores is the same
// text.  The scale is read with the row, once per tile, and not for rows that are not read.  quantize_rows_f8_kernel
// makes codes and scales from fp32 or bf16 rows.
#include "vp_common.h"
#include "vp_kernels.h"

#include <cmath>

namespace vp {

namespace {

constexpr int kTkWaves = 8;              // two per SIMD: the loads in flight, not the LDS, set the streaming rate
constexpr int kTkThreads = 64 * kTkWaves;
constexpr int kTkRows = 64 * kTkWaves;   // rows of a workgroup's tile: each wave 2 MFMA tiles of 32
constexpr int kTkLdsBytes = 160 * 1024;  // LDS of a CU; one workgroup may take all of it
constexpr uint32_t kTkNoRow = 0xffffffffu;

__device__ __forceinline__ uint32_t pack_bf2(bf16_t a, bf16_t b) {
  return (uint32_t)__builtin_bit_cast(uint16_t, a) | ((uint32_t)__builtin_bit_cast(uint16_t, b) << 16);
}

// 8 fp32 query values -> their 8 bf16 hi terms and 8 bf16 lo terms (q ~ hi + lo to about 2^-16 relative)
__device__ __forceinline__ void split8(const float (&v)[8], f32x4& hi, f32x4& lo) {
  uint32_t h[4], l[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const bf16_t h0 = f2bf(v[2 * e]), h1 = f2bf(v[2 * e + 1]);
    h[e] = pack_bf2(h0, h1);
    l[e] = pack_bf2(f2bf(v[2 * e] - bf2f(h0)), f2bf(v[2 * e + 1] - bf2f(h1)));
  }
  hi = f32x4{__uint_as_float(h[0]), __uint_as_float(h[1]), __uint_as_float(h[2]), __uint_as_float(h[3])};
  lo = f32x4{__uint_as_float(l[0]), __uint_as_float(l[1]), __uint_as_float(l[2]), __uint_as_float(l[3])};
}

// one batch of 4 steps for the wave's two row tiles; lanes of rows past the range load nothing
__device__ __forceinline__ void tk_load(f32x4 (&a)[2][4], const char* const (&rp)[2], const bool (&ok)[2], int t) {
#pragma unroll
  for (int rt = 0; rt < 2; ++rt)
#pragma unroll
    for (int u = 0; u < 4; ++u)
      a[rt][u] = ok[rt] ? *reinterpret_cast<const f32x4*>(rp[rt] + (int64_t)(t + u) * 32) : f32x4{0.f, 0.f, 0.f, 0.f};
}

template <bool BF16>
__device__ __forceinline__ void tk_mma(const f32x4 (&a)[2][4], const f32x4* bq, int t, int G, int i, int half,
                                       bool qlane, f32x16 (&acc)[2]) {
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int s = t + u;
    if constexpr (BF16) {
      const f32x4 bh = qlane ? bq[((s * 2 + 0) * 2 + half) * G + i] : zero;
      const f32x4 bl = qlane ? bq[((s * 2 + 1) * 2 + half) * G + i] : zero;
#pragma unroll
      for (int rt = 0; rt < 2; ++rt) {
        const bf16x8 av = __builtin_bit_cast(bf16x8, a[rt][u]);
        acc[rt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av, __builtin_bit_cast(bf16x8, bh), acc[rt], 0, 0, 0);
        acc[rt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av, __builtin_bit_cast(bf16x8, bl), acc[rt], 0, 0, 0);
      }
    } else {
      const f32x4 b = qlane ? bq[(s * 2 + half) * G + i] : zero;
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int rt = 0; rt < 2; ++rt)
          acc[rt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[rt][u][e], b[e], acc[rt], 0, 0, 0);
    }
  }
}

// The fp8 gallery's batch: as tk_load, a step being 32 codes of a row.  A row has D / 32 steps, a multiple of 2 only, so
// the last batch may hold two steps; its other two are neither loaded nor multiplied (the test is the wave's).
__device__ __forceinline__ void tk_load_f8(f32x4 (&a)[2][4], const char* const (&rp)[2], const bool (&ok)[2], int t,
                                           int nt) {
  const bool four = t + 2 < nt;
#pragma unroll
  for (int rt = 0; rt < 2; ++rt)
#pragma unroll
    for (int u = 0; u < 4; ++u)
      a[rt][u] = ok[rt] && (u < 2 || four) ? *reinterpret_cast<const f32x4*>(rp[rt] + (int64_t)(t + u) * 32)
                                           : f32x4{0.f, 0.f, 0.f, 0.f};
}

__device__ __forceinline__ const float* tk_scales(const float* scales) { return scales; }

typedef __bf16 tk_bf16x2 __attribute__((ext_vector_type(2)));

// 8 e4m3 codes (two words) times the row's scale, a power of two -> 8 bf16, exactly: a code has four significant bits
// and the product stays far inside bf16's exponent range (v_cvt_scalef32_pk_bf16_fp8, two codes an instruction)
__device__ __forceinline__ bf16x8 tk_decode8(float w0, float w1, float scale) {
  const uint32_t u0 = __float_as_uint(w0), u1 = __float_as_uint(w1);
  const tk_bf16x2 d[4] = {__builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(u0, scale, false),
                          __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(u0, scale, true),
                          __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(u1, scale, false),
                          __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(u1, scale, true)};
  return __builtin_bit_cast(bf16x8, d);
}

// fp8 gallery: the lane's 16 codes of a step are two bf16x8 operands (codes 0 .. 7 and 8 .. 15 of its 16), each against
// the hi and then the lo fragment of the same 8 query values: v_mfma_f32_32x32x16_bf16 four times a step and row tile
__device__ __forceinline__ void tk_mma_f8(const f32x4 (&a)[2][4], const float (&scale)[2], const f32x4* bq, int t, int nt,
                                          int G, int i, int half, bool qlane, f32x16 (&acc)[2]) {
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    if (u == 2 && t + 2 >= nt) break;
    const int s = t + u;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const f32x4 bh = qlane ? bq[(((s * 2 + j) * 2 + 0) * 2 + half) * G + i] : zero;
      const f32x4 bl = qlane ? bq[(((s * 2 + j) * 2 + 1) * 2 + half) * G + i] : zero;
#pragma unroll
      for (int rt = 0; rt < 2; ++rt) {
        const bf16x8 av = tk_decode8(a[rt][u][2 * j], a[rt][u][2 * j + 1], scale[rt]);
        acc[rt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av, __builtin_bit_cast(bf16x8, bh), acc[rt], 0, 0, 0);
        acc[rt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av, __builtin_bit_cast(bf16x8, bl), acc[rt], 0, 0, 0);
      }
    }
  }
}

// The wave's rows that beat their query's k-th score enter its list, in row order (see the file comment).  GROUPED: the
// list holds one entry per group (llb: the entries' labels; labels: the rows' labels in memory).
template <bool GROUPED>
__device__ __forceinline__ void tk_insert(const f32x16 (&acc)[2], int64_t r0, int64_t p0, int64_t p1, int k, int i,
                                          int half, bool qlane, float* lsc, uint32_t* lid, int64_t* llb,
                                          const int64_t* __restrict__ labels) {
  float* sc = lsc + i * k;
  uint32_t* id = lid + i * k;
  __threadfence_block();
  float thr = qlane ? sc[k - 1] : INFINITY;
#pragma unroll
  for (int rt = 0; rt < 2; ++rt) {
    // GROUPED: the labels of the lane's rows of this tile that beat the k-th score, read together before the rows take
    // their turns (one latency a tile, not one a candidate; the k-th score only rises, so no later candidate is missed)
    int64_t lab[GROUPED ? 16 : 1];
    if constexpr (GROUPED) {
      bool c16 = false;
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int64_t row = r0 + 32 * rt + (q & 3) + 8 * (q >> 2) + 4 * half;
        const bool ok = row < p1 && acc[rt][q] > thr;
        c16 |= ok;
        lab[q] = ok ? labels[row] : (int64_t)-1;
      }
      if (__ballot(c16) == 0) continue;
      // Of the lane's candidates that follow one another with the same label only the best can be its group's best row
      // (of equal scores the first), so the others give up their turn: forwards a row that an earlier one of its run
      // equals or beats, backwards a row that a later one beats.  With a video's windows in neighbouring rows this
      // leaves one candidate a lane instead of 16; what the lists end up holding does not depend on it.
      {
        int64_t cl = -1;
        float cs = 0.f;
#pragma unroll
        for (int q = 0; q < 16; ++q) {
          if (lab[q] < 0) continue;
          if (lab[q] != cl) cl = lab[q], cs = acc[rt][q];
          else if (acc[rt][q] > cs) cs = acc[rt][q];
          else lab[q] = -1;
        }
        cl = -1;
#pragma unroll
        for (int q = 15; q >= 0; --q) {
          if (lab[q] < 0) continue;
          if (lab[q] != cl) cl = lab[q], cs = acc[rt][q];
          else if (acc[rt][q] >= cs) cs = acc[rt][q];
          else lab[q] = -1;
        }
      }
    }
    auto live = [&](int q) {  // GROUPED: the candidate kept its turn (and its label is not negative)
      if constexpr (GROUPED) return lab[q] >= 0;
      else return true;
    };
#pragma unroll
    for (int qb = 0; qb < 4; ++qb) {  // rows 8 qb .. 8 qb + 7 of the tile: acc[4 qb .. 4 qb + 3] of both halves
      bool c4 = false;
#pragma unroll
      for (int e = 0; e < 4; ++e)
        c4 |= r0 + 32 * rt + 8 * qb + 4 * half + e < p1 && acc[rt][4 * qb + e] > thr && live(4 * qb + e);
      if (__ballot(c4) == 0) continue;
#pragma unroll
      for (int jj = 8 * qb; jj < 8 * qb + 8; ++jj) {
        const int q = (jj & 3) + 4 * (jj >> 3);  // row jj is acc[q] of the lanes with half == (jj >> 2) & 1
        const int64_t row = r0 + 32 * rt + jj;
        const float v = acc[rt][q];
        const bool c = half == ((jj >> 2) & 1) && row < p1 && v > thr && live(q);
        if (__ballot(c) != 0) {
          if constexpr (GROUPED) {
            // the same walk also looks for the row's group in slots 0 .. k - 2.  Found there with a score not smaller:
            // nothing changes (rows ascend, so an equal score has the smaller row already).  Found with a smaller
            // score: overwritten in place, and slot k - 1 is still the worst.  Not found, or found in slot k - 1 (whose
            // score v beats): the new entry takes slot k - 1 and trades places with the worst, as in the ungrouped path
            const int64_t g = lab[q];
            if (c) {
              int64_t* lb = llb + i * k;
              const uint32_t rr = (uint32_t)(row - p0);
              float ws = v;
              uint32_t wr = rr;
              int64_t wl = g;
              int wp = k - 1, mp = -1;
              for (int p = 0; p < k - 1; ++p) {
                const float s = sc[p];
                const uint32_t r = id[p];
                const int64_t l = lb[p];
                if (l == g) mp = p;
                if (s < ws || (s == ws && r > wr)) ws = s, wr = r, wl = l, wp = p;
              }
              if (mp >= 0) {
                if (sc[mp] < v) sc[mp] = v, id[mp] = rr;
              } else {
                sc[wp] = v;
                id[wp] = rr;
                lb[wp] = g;
                sc[k - 1] = ws;
                id[k - 1] = wr;
                lb[k - 1] = wl;
              }
            }
          } else if (c) {
            // the new entry evicts slot k - 1, the worst; the worst of the k now there (lowest score, of equal scores
            // the largest row) trades places with it
            const uint32_t rr = (uint32_t)(row - p0);
            float ws = v;
            uint32_t wr = rr;
            int wp = k - 1;
            for (int p = 0; p < k - 1; ++p) {
              const float s = sc[p];
              const uint32_t r = id[p];
              if (s < ws || (s == ws && r > wr)) ws = s, wr = r, wp = p;
            }
            sc[wp] = v;
            id[wp] = rr;
            sc[k - 1] = ws;
            id[k - 1] = wr;
          }
          __threadfence_block();  // the query's other half-lane reads the new k-th score
          thr = qlane ? sc[k - 1] : INFINITY;
        }
      }
    }
  }
}

// the two mask words of the wave's rows r0 .. r0 + 63 (r0 a multiple of 64); a word whose rows all lie past the range
// is not read, and lanes without a query hold zeros
__device__ __forceinline__ void tk_mask_load(uint32_t (&m)[2], const uint32_t* mq, bool mlane, int64_t r0, int64_t p1) {
#pragma unroll
  for (int rt = 0; rt < 2; ++rt) m[rt] = mlane && r0 + 32 * rt < p1 ? mq[(r0 >> 5) + rt] : 0u;
}

// how the gallery is stored, the kernel's first template argument: vp_kernels.h's kGalleryF32 / BF16 / F8
constexpr int kTkF32 = kGalleryF32, kTkBF16 = kGalleryBF16, kTkF8 = kGalleryF8;

// MASKED: a row enters a list only where its bit of `mask` is set (see the file comment); the other instantiations do
// not look at the two arguments.  ST == kTkF8: `gallery` holds e4m3 codes, ld in bytes, and row r stands for its codes
// times scales[r].  That pointer is the one trailing argument `sc` of the fp8 instantiations alone, so the others keep
// the argument list, and with it the code object, they had before there was an fp8 gallery.
template <int ST, bool GROUPED, bool MASKED, typename... SC>
__global__ __launch_bounds__(kTkThreads) void topk_scan_kernel(const float* __restrict__ queries, int64_t Q,
                                                        const void* __restrict__ gallery, int64_t N, int64_t ld, int D,
                                                        int k, int G, int64_t rows_per_part, int64_t id_base,
                                                        float* __restrict__ ws_sc, int64_t* __restrict__ ws_id,
                                                        const int64_t* __restrict__ labels,
                                                        int64_t* __restrict__ ws_gr,
                                                        const uint32_t* __restrict__ mask, int64_t mask_stride,
                                                        SC... sc) {
  constexpr bool BF16 = ST == kTkBF16, F8 = ST == kTkF8;
  static_assert(sizeof...(SC) == (F8 ? 1 : 0), "the scales come with the fp8 gallery and with no other");
  extern __shared__ __attribute__((aligned(16))) char tk_smem[];
  f32x4* bq = reinterpret_cast<f32x4*>(tk_smem);                          // D * G * 4 bytes, fragment order
  float* lsc = reinterpret_cast<float*>(tk_smem + (size_t)D * G * 4);     // [G][k]
  uint32_t* lid = reinterpret_cast<uint32_t*>(lsc + G * k);               // [G][k] row - p0
  volatile int* flags = reinterpret_cast<volatile int*>(lid + G * k);     // [2][kTkWaves]
  // GROUPED: [G][k] labels behind the flags (a multiple of 8 bytes from the start)
  int64_t* llb = GROUPED ? reinterpret_cast<int64_t*>(const_cast<int*>(flags) + 2 * kTkWaves) : nullptr;
  const int tid = threadIdx.x;
  const int lane = tid & 63, w = tid >> 6, i = lane & 31, half = lane >> 5;
  const int64_t q0 = (int64_t)blockIdx.y * G;

  for (int e = tid; e < G * k; e += kTkThreads) {
    lsc[e] = -INFINITY;
    lid[e] = kTkNoRow;
    if constexpr (GROUPED) llb[e] = -1;  // matches no row's label: a lane skips a negative one
  }
  if constexpr (BF16 || F8) {
    const int nc = D >> 3;  // chunks of 8 values: step c >> 1, half c & 1 (fp8: step c >> 2, half, then operand c & 1)
    for (int e = tid; e < G * nc; e += kTkThreads) {
      const int qi = e / nc, c = e % nc;
      float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      if (q0 + qi < Q) {
        const float4* src = reinterpret_cast<const float4*>(queries + (q0 + qi) * D + 8 * c);
        const float4 x = src[0], y = src[1];
        v[0] = x.x, v[1] = x.y, v[2] = x.z, v[3] = x.w, v[4] = y.x, v[5] = y.y, v[6] = y.z, v[7] = y.w;
      }
      f32x4 hi, lo;
      split8(v, hi, lo);
      if constexpr (F8) {
        const int s = c >> 2, h = (c >> 1) & 1, j = c & 1;
        bq[(((s * 2 + j) * 2 + 0) * 2 + h) * G + qi] = hi;
        bq[(((s * 2 + j) * 2 + 1) * 2 + h) * G + qi] = lo;
      } else {
        const int s = c >> 1, h = c & 1;
        bq[((s * 2 + 0) * 2 + h) * G + qi] = hi;
        bq[((s * 2 + 1) * 2 + h) * G + qi] = lo;
      }
    }
  } else {
    const int nc = D >> 2;  // chunks of 4 values
    for (int e = tid; e < G * nc; e += kTkThreads) {
      const int qi = e / nc, c = e % nc;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (q0 + qi < Q) v = *reinterpret_cast<const f32x4*>(queries + (q0 + qi) * D + 4 * c);
      bq[((c >> 1) * 2 + (c & 1)) * G + qi] = v;
    }
  }
  __syncthreads();

  // the workgroup's rows: [p0, p1), tile after tile.  MASKED: the tiles are dealt to the workgroups in turn instead
  // (workgroup x takes tiles x, x + gridDim.x, ... to the gallery's end: rows_per_part is then the step, gridDim.x
  // tiles), so a long run of rows that are not allowed shortens every workgroup's walk a little and no workgroup's
  // not at all; the rows still ascend, and the lists count them from the workgroup's first tile
  const int64_t p0 = (int64_t)blockIdx.x * (MASKED ? (int64_t)kTkRows : rows_per_part);
  const int64_t p1 = MASKED ? N : p0 + rows_per_part < N ? p0 + rows_per_part : N;
  const int tstep = MASKED ? (int)rows_per_part : kTkRows;  // at most kTopkMaxParts tiles
  const int64_t row_bytes = ld * (F8 ? 1 : BF16 ? 2 : 4);
  const int nt = (D * (F8 ? 1 : BF16 ? 2 : 4)) >> 5;  // 32-byte steps of a row: a multiple of 4 (fp8: of 2)
  const bool qlane = i < G;
  // MASKED: the lane's mask (its query's, or the shared one in every lane) and the words of the wave's 64 rows of the
  // tile to come, two 32-row words read one tile ahead; a tile starts at a multiple of 512, so r0 is one of 64
  const uint32_t* mq = nullptr;
  bool mlane = false, mshared = false;
  uint32_t mnext[2] = {0u, 0u};
  if constexpr (MASKED) {
    mshared = mask_stride == 0;
    mlane = mshared || (qlane && q0 + i < Q);
    mq = mask + (mlane ? (q0 + i) * mask_stride : 0);
    tk_mask_load(mnext, mq, mlane, p0 + 64 * w, p1);
  }
  int par = 0;
  for (int64_t tb = p0; tb < p1; tb += tstep, par ^= 1) {
    const int64_t r0 = tb + 64 * w;
    f32x16 acc[2] = {};
    uint32_t mw[2] = {mnext[0], mnext[1]};
    bool wave = r0 < p1;
    bool need[2] = {true, true};  // the lane's row of each 32-row tile is read
    if constexpr (MASKED) {
      if (tb + tstep < p1) tk_mask_load(mnext, mq, mlane, r0 + tstep, p1);
      // no query of the wave allows any of its 64 rows: neither loads nor MFMAs (the branch is the wave's; the loads
      // of a tile are all issued inside it, so a skipped tile leaves none in flight).  Under the shared mask every
      // lane holds the rows' own bits and a row that is not allowed is not read either; per query, a 32-row tile
      // that no query allows is not read
      wave = wave && __ballot((mw[0] | mw[1]) != 0) != 0;
#pragma unroll
      for (int rt = 0; rt < 2; ++rt) need[rt] = mshared ? (mw[rt] >> i) & 1 : __ballot(mw[rt] != 0) != 0;
    }
    if (wave) {  // whole wave
      const char* rp[2];
      bool ok[2];
#pragma unroll
      for (int rt = 0; rt < 2; ++rt) {
        const int64_t row = r0 + 32 * rt + i;
        ok[rt] = row < p1 && need[rt];
        rp[rt] = static_cast<const char*>(gallery) + row * row_bytes + 16 * half;
      }
      f32x4 a0[2][4], a1[2][4];
      if constexpr (F8) {
        // the scale of the lane's row comes with the row: not read where the row is not (its codes are zeros then)
        const float* scales = tk_scales(sc...);
        float scale[2];
#pragma unroll
        for (int rt = 0; rt < 2; ++rt) scale[rt] = ok[rt] ? scales[r0 + 32 * rt + i] : 1.f;
        tk_load_f8(a0, rp, ok, 0, nt);
        for (int t = 0; t < nt; t += 8) {
          const bool more = t + 4 < nt;
          if (more) tk_load_f8(a1, rp, ok, t + 4, nt);
          tk_mma_f8(a0, scale, bq, t, nt, G, i, half, qlane, acc);
          if (more) {
            if (t + 8 < nt) tk_load_f8(a0, rp, ok, t + 8, nt);
            tk_mma_f8(a1, scale, bq, t + 4, nt, G, i, half, qlane, acc);
          }
        }
      } else {
        tk_load(a0, rp, ok, 0);
        for (int t = 0; t < nt; t += 8) {
          const bool more = t + 4 < nt;
          if (more) tk_load(a1, rp, ok, t + 4);
          tk_mma<BF16>(a0, bq, t, G, i, half, qlane, acc);
          if (more) {
            if (t + 8 < nt) tk_load(a0, rp, ok, t + 8);
            tk_mma<BF16>(a1, bq, t + 4, G, i, half, qlane, acc);
          }
        }
      }
    }
    if constexpr (MASKED) {
      // a row that the lane's query does not allow scores -inf from here on: it fails the pre-check and every
      // comparison of tk_insert; an allowed row's score is what the MFMAs left
#pragma unroll
      for (int rt = 0; rt < 2; ++rt) {
        const uint32_t mh = mw[rt] >> (4 * half);
#pragma unroll
        for (int q = 0; q < 16; ++q)
          if (!((mh >> ((q & 3) + 8 * (q >> 2))) & 1)) acc[rt][q] = -INFINITY;
      }
    }
    // lists last changed before the previous tile's final barrier
    const float thr = qlane ? lsc[i * k + k - 1] : INFINITY;
    bool any = false;
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int64_t row = r0 + 32 * rt + (q & 3) + 8 * (q >> 2) + 4 * half;
        any |= row < p1 && acc[rt][q] > thr;
      }
    const bool wany = __ballot(any) != 0;
    if (lane == 0) flags[par * kTkWaves + w] = wany;
    __syncthreads();
#pragma unroll
    for (int ww = 0; ww < kTkWaves; ++ww) {
      if (flags[par * kTkWaves + ww]) {  // the same for every thread
        if (w == ww) tk_insert<GROUPED>(acc, r0, p0, p1, k, i, half, qlane, lsc, lid, llb, labels);
        __syncthreads();
      }
    }
  }
  __syncthreads();
  const int64_t part = blockIdx.x;
  for (int e = tid; e < G * k; e += kTkThreads) {
    const int qi = e / k, j = e % k;
    if (q0 + qi >= Q) continue;
    // the lists are unordered but for their last slot: an entry goes where the count of entries that beat it says
    // (score descending, row ascending; among the padding, slot order)
    const float s = lsc[e];
    const uint32_t r = lid[e];
    int rank = 0;
    for (int p = 0; p < k; ++p) {
      const float s2 = lsc[qi * k + p];
      const uint32_t r2 = lid[qi * k + p];
      rank += s2 > s || (s2 == s && (r2 < r || (r2 == r && p < j)));
    }
    const int64_t o = (part * Q + q0 + qi) * k + rank;
    ws_sc[o] = s;
    ws_id[o] = r == kTkNoRow ? (int64_t)-1 : id_base + p0 + (int64_t)r;
    if constexpr (GROUPED) ws_gr[o] = llb[e];  // -1 where the slot was never filled
  }
}

// the order: score descending, id ascending, padding (id < 0) last
__device__ __forceinline__ bool tk_beats(float s1, int64_t i1, float s2, int64_t i2) {
  if (i1 < 0) return false;
  if (i2 < 0) return true;
  return s1 > s2 || (s1 == s2 && i1 < i2);
}

__global__ __launch_bounds__(256) void topk_merge_kernel(const float* __restrict__ sin, const int64_t* __restrict__ iin,
                                                         int64_t parts, int64_t Q, int k_in, int k, int L,
                                                         float* __restrict__ so, int64_t* __restrict__ io) {
  extern __shared__ __attribute__((aligned(16))) char mg_smem[];
  // two buffers of L lists of k_in entries
  int64_t* idb = reinterpret_cast<int64_t*>(mg_smem);
  float* scb = reinterpret_cast<float*>(idb + 2 * L * k_in);
  const int tid = threadIdx.x;
  const int64_t q = blockIdx.x;
  const int LK = L * k_in;
  int cur = 0;
  for (int e = tid; e < k_in; e += 256) {  // list 0: the running result
    scb[e] = -INFINITY;
    idb[e] = -1;
  }
  for (int64_t base = 0; base < parts; base += L - 1) {
    for (int e = tid; e < LK - k_in; e += 256) {
      const int64_t p = base + e / k_in;
      float s = -INFINITY;
      int64_t id = -1;
      if (p < parts) {
        const int64_t o = (p * Q + q) * k_in + e % k_in;
        s = sin[o];
        id = iin[o];
        if (!(s > -INFINITY) || id < 0) s = -INFINITY, id = -1;  // NaN and -inf never rank
      }
      scb[cur * LK + k_in + e] = s;
      idb[cur * LK + k_in + e] = id;
    }
    __syncthreads();
    for (int n = L; n > 1; n >>= 1) {
      const float* cs = scb + cur * LK;
      const int64_t* ci = idb + cur * LK;
      float* ns = scb + (cur ^ 1) * LK;
      int64_t* ni = idb + (cur ^ 1) * LK;
      for (int e = tid; e < n * k_in; e += 256) {
        const int l = e / k_in, j = e % k_in;
        const float s = cs[e];
        const int64_t id = ci[e];
        const float* os = cs + (l ^ 1) * k_in;
        const int64_t* oi = ci + (l ^ 1) * k_in;
        int lo = 0, hi = k_in;  // entries of the other list that come before this one
        while (lo < hi) {
          const int mid = (lo + hi) >> 1;
          const bool before = (l & 1) ? !tk_beats(s, id, os[mid], oi[mid]) : tk_beats(os[mid], oi[mid], s, id);
          if (before) lo = mid + 1;
          else hi = mid;
        }
        const int rank = j + lo;
        if (rank < k_in) {
          ns[(l >> 1) * k_in + rank] = s;
          ni[(l >> 1) * k_in + rank] = id;
        }
      }
      __syncthreads();
      cur ^= 1;
    }
  }
  __syncthreads();
  for (int e = tid; e < k; e += 256) {
    so[q * k + e] = scb[cur * LK + e];
    io[q * k + e] = idb[cur * LK + e];
  }
}

// The grouped merge: topk_merge_kernel's rounds and pairwise tree over lists of (score, group, id), one entry per group.
// At a pairwise step an entry is dropped when the other list holds its group with an entry that comes before it (of
// two identical entries the odd list's goes); a survivor's place is the number of survivors before it in its own list
// plus the number of the other list's survivors that come before it.  The dropped entries leave holes, so both numbers
// are counted, not searched; the output list is cleared first and every survivor writes its own slot.
__global__ __launch_bounds__(256) void topk_groups_merge_kernel(const float* __restrict__ sin,
                                                                const int64_t* __restrict__ gin,
                                                                const int64_t* __restrict__ iin, int64_t parts,
                                                                int64_t Q, int k_in, int k, int L,
                                                                float* __restrict__ so, int64_t* __restrict__ go,
                                                                int64_t* __restrict__ io) {
  extern __shared__ __attribute__((aligned(16))) char mg_smem[];
  // two buffers of L lists of k_in entries, and one flag per entry of a buffer
  int64_t* idb = reinterpret_cast<int64_t*>(mg_smem);
  int64_t* grb = idb + 2 * L * k_in;
  float* scb = reinterpret_cast<float*>(grb + 2 * L * k_in);
  int* live = reinterpret_cast<int*>(scb + 2 * L * k_in);
  const int tid = threadIdx.x;
  const int64_t q = blockIdx.x;
  const int LK = L * k_in;
  int cur = 0;
  for (int e = tid; e < k_in; e += 256) {  // list 0: the running result
    scb[e] = -INFINITY;
    idb[e] = -1;
    grb[e] = -1;
  }
  for (int64_t base = 0; base < parts; base += L - 1) {
    for (int e = tid; e < LK - k_in; e += 256) {
      const int64_t p = base + e / k_in;
      float s = -INFINITY;
      int64_t id = -1, g = -1;
      if (p < parts) {
        const int64_t o = (p * Q + q) * k_in + e % k_in;
        s = sin[o];
        id = iin[o];
        g = gin[o];
        if (!(s > -INFINITY) || id < 0 || g < 0) s = -INFINITY, id = -1, g = -1;  // NaN, -inf and blanks never rank
      }
      scb[cur * LK + k_in + e] = s;
      idb[cur * LK + k_in + e] = id;
      grb[cur * LK + k_in + e] = g;
    }
    __syncthreads();
    for (int n = L; n > 1; n >>= 1) {
      const float* cs = scb + cur * LK;
      const int64_t* ci = idb + cur * LK;
      const int64_t* cg = grb + cur * LK;
      float* ns = scb + (cur ^ 1) * LK;
      int64_t* ni = idb + (cur ^ 1) * LK;
      int64_t* ng = grb + (cur ^ 1) * LK;
      for (int e = tid; e < n * k_in; e += 256) {
        const int l = e / k_in;
        const float s = cs[e];
        const int64_t id = ci[e], g = cg[e];
        bool alive = id >= 0;
        if (alive) {
          const int ob = (l ^ 1) * k_in;
          for (int p = 0; p < k_in; ++p) {
            if (cg[ob + p] != g) continue;
            const float s2 = cs[ob + p];
            const int64_t i2 = ci[ob + p];
            if (tk_beats(s2, i2, s, id) || ((l & 1) && s2 == s && i2 == id)) alive = false;
          }
        }
        live[e] = alive;
        if (e < (n >> 1) * k_in) {
          ns[e] = -INFINITY;
          ni[e] = -1;
          ng[e] = -1;
        }
      }
      __syncthreads();
      for (int e = tid; e < n * k_in; e += 256) {
        if (!live[e]) continue;
        const int l = e / k_in, j = e % k_in;
        const float s = cs[e];
        const int64_t id = ci[e];
        int rank = 0;
        for (int p = 0; p < j; ++p) rank += live[l * k_in + p];
        const int ob = (l ^ 1) * k_in;
        for (int p = 0; p < k_in; ++p) {
          const float s2 = cs[ob + p];
          const int64_t i2 = ci[ob + p];
          const bool before = (l & 1) ? !tk_beats(s, id, s2, i2) : tk_beats(s2, i2, s, id);
          rank += live[ob + p] && before;
        }
        if (rank < k_in) {
          ns[(l >> 1) * k_in + rank] = s;
          ni[(l >> 1) * k_in + rank] = id;
          ng[(l >> 1) * k_in + rank] = cg[e];
        }
      }
      __syncthreads();
      cur ^= 1;
    }
  }
  __syncthreads();
  for (int e = tid; e < k; e += 256) {
    so[q * k + e] = scb[cur * LK + e];
    io[q * k + e] = idb[cur * LK + e];
    go[q * k + e] = grb[cur * LK + e];
  }
}

// The row mask of the masked search from one byte per row (vp_op_rowmask_pack): a wave takes 64 rows of one mask, a
// lane reads its row's byte, the ballot of `nonzero` is the two words, and lanes 0 and 1 store one each, after the AND
// with the same word of `andw` where that is given (and_stride 0: one such mask for all Q).  Rows past N give zero
// bits; a word is written only where it holds a row, and every word that does is written by exactly one lane.
constexpr int kPackRows = 256;  // rows of a workgroup: 4 waves

__global__ __launch_bounds__(kPackRows) void rowmask_pack_kernel(const uint8_t* __restrict__ allow, int64_t Q, int64_t N,
                                                                 const uint32_t* __restrict__ andw, int64_t and_stride,
                                                                 uint32_t* __restrict__ out, int64_t stride) {
  const int lane = threadIdx.x & 63;
  const int64_t r0 = (int64_t)blockIdx.x * kPackRows + (threadIdx.x & ~63);  // the wave's first row
  if (r0 >= N) return;
  for (int64_t q = blockIdx.y; q < Q; q += gridDim.y) {
    const int64_t row = r0 + lane;
    const bool on = row < N && allow[q * N + row] != 0;
    const uint64_t b = __ballot(on);
    const int64_t wd = (r0 >> 5) + lane;  // lanes 0 and 1: the word this lane stores
    if (lane < 2 && r0 + 32 * lane < N) {
      uint32_t v = (uint32_t)(b >> (32 * lane));
      if (andw) v &= andw[q * and_stride + wd];
      out[q * stride + wd] = v;
    }
  }
}

// Rows to the fp8 gallery's storage (vp_op_quantize_rows_f8; DESIGN.md §4 "fp8 gallery"): row r becomes D e4m3 codes
// and one scale 2^-e, e the largest integer with amax * 2^e <= 448 (amax over the row's finite elements), clamped to
// +-100 and 0 for a row without a finite nonzero element; code = RNE_e4m3(x * 2^e), the NaN code for a non-finite x.
// A wave takes a row and reads it once: a lane keeps up to two chunks of 16 values in registers, the wave reduces the
// largest magnitude as an integer (the bits of |x| order as the values do), e comes from its exponent and mantissa
// fields (amax = m * 2^p, m in [0.5, 1): 9 - p where m <= 0.875, else 8 - p), the products are exact and
// v_cvt_pk_fp8_f32 rounds them; no product passes 448 (but where e was clamped, which plain C++ handles), so the
// instruction never saturates, and it never sees a non-finite value either.  A lane stores its chunk's 16 codes as one
// 16-byte word and lane 0 the scale; columns past D and rows past N are not written.
constexpr int kQzRows = 4;  // rows of a workgroup: a wave each

template <bool XBF16>
__global__ __launch_bounds__(64 * kQzRows) void quantize_rows_f8_kernel(const void* __restrict__ x, int64_t N,
                                                                        int64_t ldx, int D, uint8_t* __restrict__ codes,
                                                                        int64_t ldc, float* __restrict__ scales) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * kQzRows + (threadIdx.x >> 6);
  if (row >= N) return;  // the whole wave
  const int nch = D >> 4;  // chunks of 16 values: at most 96
  float v[2][16];
  uint32_t amax = 0;
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    const int ch = lane + 64 * c;
    if (ch < nch) {
      if constexpr (XBF16) {
        const f32x4* src = reinterpret_cast<const f32x4*>(static_cast<const bf16_t*>(x) + row * ldx + 16 * ch);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const f32x4 p = src[h];
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const uint32_t u = __float_as_uint(p[e]);
            v[c][8 * h + 2 * e] = __uint_as_float(u << 16);
            v[c][8 * h + 2 * e + 1] = __uint_as_float(u & 0xffff0000u);
          }
        }
      } else {
        const f32x4* src = reinterpret_cast<const f32x4*>(static_cast<const float*>(x) + row * ldx + 16 * ch);
#pragma unroll
        for (int h = 0; h < 4; ++h) {
          const f32x4 p = src[h];
#pragma unroll
          for (int e = 0; e < 4; ++e) v[c][4 * h + e] = p[e];
        }
      }
    } else {
#pragma unroll
      for (int e = 0; e < 16; ++e) v[c][e] = 0.f;
    }
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const uint32_t u = __float_as_uint(v[c][e]) & 0x7fffffffu;
      if (u < 0x7f800000u && u > amax) amax = u;
    }
  }
#pragma unroll
  for (int m = 32; m > 0; m >>= 1) {
    const uint32_t o = (uint32_t)__shfl_xor((int)amax, m);
    amax = o > amax ? o : amax;
  }
  int e = 0;
  if (amax != 0) {
    const int E = (int)(amax >> 23);  // 0: a denormal, p <= -126, and e clamps
    e = E == 0 ? 100 : ((amax & 0x7fffffu) <= 0x600000u ? 135 : 134) - E;
    e = e < -100 ? -100 : e > 100 ? 100 : e;
  }
  const float mul = __uint_as_float((uint32_t)(127 + e) << 23);
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    const int ch = lane + 64 * c;
    if (ch >= nch) continue;
    uint32_t w[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      float y[4];
      uint32_t nanb = 0;  // the NaN code in the bytes of non-finite elements, whatever the instruction makes of them
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const float xv = v[c][4 * g + b];
        float p = xv * mul;
        // only where e was clamped at -100 (amax above 448 * 2^100) can a product pass 448: from 464, the tie with
        // the absent next value, the format's round-to-nearest gives the NaN code, below it 448
        const bool fin = (__float_as_uint(xv) & 0x7fffffffu) < 0x7f800000u && fabsf(p) < 464.f;
        p = fabsf(p) > 448.f ? copysignf(448.f, p) : p;
        y[b] = fin ? p : 0.f;
        nanb |= fin ? 0u : 0xffu << (8 * b);
      }
      int pk = __builtin_amdgcn_cvt_pk_fp8_f32(y[0], y[1], 0, false);
      pk = __builtin_amdgcn_cvt_pk_fp8_f32(y[2], y[3], pk, true);
      w[g] = ((uint32_t)pk & ~nanb) | (0x7f7f7f7fu & nanb);
    }
    *reinterpret_cast<f32x4*>(codes + row * ldc + 16 * ch) =
        f32x4{__uint_as_float(w[0]), __uint_as_float(w[1]), __uint_as_float(w[2]), __uint_as_float(w[3])};
  }
  if (lane == 0) scales[row] = __uint_as_float((uint32_t)(127 - e) << 23);
}

}  // namespace

int topk_group(int D, int k) {
  return D <= 1024 && (size_t)D * 32 * 4 + (size_t)32 * k * 8 + 64 <= (size_t)kTkLdsBytes ? 32 : 16;
}

// the grouped lists hold an int64 label per entry: 16 B instead of 8
int topk_groups_group(int D, int k) {
  return D <= 1024 && (size_t)D * 32 * 4 + (size_t)32 * k * 16 + 64 <= (size_t)kTkLdsBytes ? 32 : 16;
}

namespace {

// both searches: labels == nullptr is the ungrouped one (ws_gr unused); MASKED: mask / mask_stride as the kernel's
template <bool GROUPED, bool MASKED>
hipError_t topk_scan_launch(const float* queries, int64_t Q, const void* gallery, int st, const float* scales, int64_t N,
                            int64_t ld, int D, int k, const int64_t* labels, int64_t id_base, float* ws_sc,
                            int64_t* ws_id, int64_t* ws_gr, const uint32_t* mask, int64_t mask_stride, int* parts_out,
                            hipStream_t s) {
  if (st < kGalleryF32 || st > kGalleryF8 || (st == kGalleryF8 && !scales && N > 0)) return hipErrorInvalidValue;
  if (Q < 1 || N < 0 || D < 64 || D % 64 || D > kPoolMaxD || k < 1 || k > kTopkMaxK || ld < D) return hipErrorInvalidValue;
  if (MASKED && ((!mask && N > 0) || mask_stride < 0 || (mask_stride > 0 && mask_stride < (N + 31) / 32)))
    return hipErrorInvalidValue;
  const int G = GROUPED ? topk_groups_group(D, k) : topk_group(D, k);
  const int64_t groups = (Q + G - 1) / G;
  if (groups > 65535) return hipErrorInvalidValue;
  // about one workgroup per CU (each takes most of a CU's LDS), every range a whole number of tiles
  const int64_t tiles = (N + kTkRows - 1) / kTkRows;
  int64_t parts = device_cu_count() / groups;
  parts = parts < 1 ? 1 : parts > kTopkMaxParts ? kTopkMaxParts : parts;
  parts = tiles < 1 ? 1 : parts > tiles ? tiles : parts;
  int64_t rows_per_part = tiles < 1 ? kTkRows : (tiles + parts - 1) / parts * kTkRows;
  if (MASKED) {
    // the tiles go to the workgroups in turn (see the kernel): the kernel's rows_per_part is the step from one of a
    // workgroup's tiles to its next, and a list counts rows from the workgroup's first tile to the gallery's end
    rows_per_part = parts * kTkRows;
    if (N >= (int64_t)kTkNoRow) return hipErrorInvalidValue;
  } else {
    if (rows_per_part >= (int64_t)kTkNoRow) return hipErrorInvalidValue;
    parts = tiles < 1 ? 1 : (N + rows_per_part - 1) / rows_per_part;
  }
  const int lds = D * G * 4 + G * k * (GROUPED ? 16 : 8) + 2 * kTkWaves * 4;
  const void* fn = st == kTkF8     ? reinterpret_cast<const void*>(&topk_scan_kernel<kTkF8, GROUPED, MASKED, const float*>)
                   : st == kTkBF16 ? reinterpret_cast<const void*>(&topk_scan_kernel<kTkBF16, GROUPED, MASKED>)
                                   : reinterpret_cast<const void*>(&topk_scan_kernel<kTkF32, GROUPED, MASKED>);
  hipError_t e = ensure_dyn_lds(fn, kTkLdsBytes);
  if (e != hipSuccess) return e;
  const dim3 grid((unsigned)parts, (unsigned)groups);
  if (st == kTkF8)
    hipLaunchKernelGGL((topk_scan_kernel<kTkF8, GROUPED, MASKED, const float*>), grid, dim3(kTkThreads), lds, s, queries,
                       Q, gallery, N, ld, D, k, G, rows_per_part, id_base, ws_sc, ws_id, labels, ws_gr, mask, mask_stride,
                       scales);
  else if (st == kTkBF16)
    hipLaunchKernelGGL((topk_scan_kernel<kTkBF16, GROUPED, MASKED>), grid, dim3(kTkThreads), lds, s, queries, Q, gallery,
                       N, ld, D, k, G, rows_per_part, id_base, ws_sc, ws_id, labels, ws_gr, mask, mask_stride);
  else
    hipLaunchKernelGGL((topk_scan_kernel<kTkF32, GROUPED, MASKED>), grid, dim3(kTkThreads), lds, s, queries, Q, gallery,
                       N, ld, D, k, G, rows_per_part, id_base, ws_sc, ws_id, labels, ws_gr, mask, mask_stride);
  *parts_out = (int)parts;
  return hipGetLastError();
}

}  // namespace

hipError_t topk_scan(const float* queries, int64_t Q, const void* gallery, int storage, int64_t N, int64_t ld, int D,
                     int k, int64_t id_base, float* ws_sc, int64_t* ws_id, int* parts_out, hipStream_t s,
                     const float* scales) {
  return topk_scan_launch<false, false>(queries, Q, gallery, storage, scales, N, ld, D, k, nullptr, id_base, ws_sc, ws_id,
                                        nullptr, nullptr, 0, parts_out, s);
}

hipError_t topk_groups_scan(const float* queries, int64_t Q, const void* gallery, int storage, int64_t N, int64_t ld,
                            int D, int k, const int64_t* labels, int64_t id_base, float* ws_sc, int64_t* ws_id,
                            int64_t* ws_gr, int* parts_out, hipStream_t s, const float* scales) {
  if (!labels && N > 0) return hipErrorInvalidValue;
  return topk_scan_launch<true, false>(queries, Q, gallery, storage, scales, N, ld, D, k, labels, id_base, ws_sc, ws_id,
                                       ws_gr, nullptr, 0, parts_out, s);
}

hipError_t topk_scan_masked(const float* queries, int64_t Q, const void* gallery, int storage, int64_t N, int64_t ld,
                            int D, int k, int64_t id_base, const uint32_t* mask, int64_t mask_stride, float* ws_sc,
                            int64_t* ws_id, int* parts_out, hipStream_t s, const float* scales) {
  return topk_scan_launch<false, true>(queries, Q, gallery, storage, scales, N, ld, D, k, nullptr, id_base, ws_sc, ws_id,
                                       nullptr, mask, mask_stride, parts_out, s);
}

hipError_t topk_groups_scan_masked(const float* queries, int64_t Q, const void* gallery, int storage, int64_t N,
                                   int64_t ld, int D, int k, const int64_t* labels, int64_t id_base,
                                   const uint32_t* mask, int64_t mask_stride, float* ws_sc, int64_t* ws_id,
                                   int64_t* ws_gr, int* parts_out, hipStream_t s, const float* scales) {
  if (!labels && N > 0) return hipErrorInvalidValue;
  return topk_scan_launch<true, true>(queries, Q, gallery, storage, scales, N, ld, D, k, labels, id_base, ws_sc, ws_id,
                                      ws_gr, mask, mask_stride, parts_out, s);
}

hipError_t quantize_rows_f8(const void* x, int x_bf16, int64_t N, int64_t ldx, int D, uint8_t* codes, int64_t ldc,
                            float* scales, hipStream_t s) {
  if (N < 0 || D < 64 || D % 64 || D > kPoolMaxD || ldx < D || ldc < D || ldc % 16 || ldx % (x_bf16 ? 8 : 4))
    return hipErrorInvalidValue;
  if (N == 0) return hipSuccess;
  if (!x || !codes || !scales) return hipErrorInvalidValue;
  const int64_t bx = (N + kQzRows - 1) / kQzRows;
  if (bx > 0x7fffffff) return hipErrorInvalidValue;
  if (x_bf16)
    hipLaunchKernelGGL(quantize_rows_f8_kernel<true>, dim3((unsigned)bx), dim3(64 * kQzRows), 0, s, x, N, ldx, D, codes,
                       ldc, scales);
  else
    hipLaunchKernelGGL(quantize_rows_f8_kernel<false>, dim3((unsigned)bx), dim3(64 * kQzRows), 0, s, x, N, ldx, D, codes,
                       ldc, scales);
  return hipGetLastError();
}

hipError_t rowmask_pack(const uint8_t* allow, int64_t Q, int64_t N, const uint32_t* and_words, int64_t and_stride,
                        uint32_t* out, int64_t stride, hipStream_t s) {
  const int64_t words = (N + 31) / 32;
  if (Q < 0 || N < 0 || !allow || !out || stride < words || and_stride < 0 || (and_stride > 0 && and_stride < words))
    return hipErrorInvalidValue;
  if (Q == 0 || N == 0) return hipSuccess;
  const int64_t bx = (N + kPackRows - 1) / kPackRows;
  if (bx > 0x7fffffff) return hipErrorInvalidValue;
  hipLaunchKernelGGL(rowmask_pack_kernel, dim3((unsigned)bx, (unsigned)(Q < 65535 ? Q : 65535)), dim3(kPackRows), 0, s,
                     allow, Q, N, and_words, and_stride, out, stride);
  return hipGetLastError();
}

hipError_t topk_merge(const float* sin, const int64_t* iin, int64_t parts, int64_t Q, int k_in, int k, float* so,
                      int64_t* io, hipStream_t s) {
  if (parts < 1 || Q < 1 || Q > 0x7fffffff || k_in < 1 || k_in > kTopkMaxK || k < 1 || k > k_in)
    return hipErrorInvalidValue;
  // as many lists at a time as 48 KB of LDS hold twice (16 at k_in = 128), no more than there are
  int L = 2;
  while (L < 256 && L < parts + 1 && (size_t)2 * (2 * L) * k_in * 12 <= 48 * 1024) L *= 2;
  hipLaunchKernelGGL(topk_merge_kernel, dim3((unsigned)Q), dim3(256), (size_t)2 * L * k_in * 12, s, sin, iin, parts, Q,
                     k_in, k, L, so, io);
  return hipGetLastError();
}

hipError_t topk_groups_merge(const float* sin, const int64_t* gin, const int64_t* iin, int64_t parts, int64_t Q, int k_in,
                             int k, float* so, int64_t* go, int64_t* io, hipStream_t s) {
  if (parts < 1 || Q < 1 || Q > 0x7fffffff || k_in < 1 || k_in > kTopkMaxK || k < 1 || k > k_in)
    return hipErrorInvalidValue;
  // an entry takes 20 B in each of the two buffers and a 4 B flag: as many lists at a time as 48 KB hold (8 at
  // k_in = 128), no more than there are
  int L = 2;
  while (L < 256 && L < parts + 1 && (size_t)(2 * L) * k_in * 44 <= 48 * 1024) L *= 2;
  hipLaunchKernelGGL(topk_groups_merge_kernel, dim3((unsigned)Q), dim3(256), (size_t)L * k_in * 44, s, sin, gin, iin,
                     parts, Q, k_in, k, L, so, go, io);
  return hipGetLastError();
}

}  // namespace vp
