// The 32x32x16 bf16 attention tile shared by attn_spatial_kernel and attn_seq_kernel (attention.hip), attn_long_kernel
// (attention_long_kernel.h) and the diag library's attn_long_pp_kernel: its constants, address maps and register-level
// steps, and its description, written once.  A kernel owns its staging schedule (which piece when, its waits and
// barriers), its masks and its store; the form (ii) asm loads of Q and the waits that retire them stay in the kernel
// bodies, where tools/check_kernels.py audits them.  No kernels and no inline-asm loads here.
// Each kernel calls the helpers that leave its device assembly as it was (tools/asm_identity.py against the parent
// commit; a helper that replaces the last use of a lane index inside a lambda changes what the lambda captures, and
// with it the schedule); where one does not, the kernel keeps the expression written out, with a pointer here.
//
// Geometry (dh = 64: a K or V row is 64 bf16 = 128 B = 8 chunks of 16 B):
//  * A wave owns 32 queries, one per lane column of v_mfma_f32_32x32x16_bf16; lane l has query l & 31 and
//    half = l >> 5.  Q is the B operand of S^T = K.Q^T: fragment kd (0..3) of lane l is the 8 dims
//    16 kd + 8 half .. + 7 of its query (q_frag_row, q_frag_ptr).
//  * K and V are staged in pieces of 8 rows x 128 B = 1 KiB, one global_load_lds of 16 B per lane: lane l lands
//    row l >> 3, LDS chunk l & 7.  The LDS-DMA image is lane-linear, so the bank swizzle goes on the global source
//    -- lane l fetches source chunk (l & 7) ^ swz(row) (stage_chunk, stage_src) -- and every read undoes it:
//    swzK(row) = (row >> 1) & 7 for the ds_read_b128 of K, swzV(row) = ((row >> 1) & 1) << 2 for the
//    ds_read_b64_tr_b16 of V.
//  * S^T tile kt: the A operand of lane l is chunk 2 kd + half of K row 32 kt + (l & 31) (k_read_at).  Output
//    register i of lane l is the logit of key 32 kt + (i & 3) + 8 (i >> 2) + 4 half against query l & 31, so a
//    query's row sum is lane-local up to one exchange between the lane halves.
//  * O^T = V^T.P^T: the numerators, rounded to bf16, are the B operand as they stand (pack_numerators:
//    pf[s] = registers 8 s .. 8 s + 7, the tile's keys 16 s .. 16 s + 15), so P never touches LDS.  The A operand
//    V^T comes from transposed reads: with g = l >> 4, trq = (l & 15) >> 2, trp = l & 3, lane l reads at key row
//    32 kt + 16 s + 4 half + trq, column 32 dh + 16 (g & 1) + 4 trp (v_read_at), and again 8 rows (1024 B) further;
//    v_frag joins the two reads, pv_mfma runs the tile's four MFMAs.  swzV of that key row is ((trq >> 1) & 1) << 2
//    whatever kt and s are, so the unrolled kernels keep per-lane bases of tile 0 and add 4096 kt + 2048 s (+ 1024)
//    as immediates (lds_tr_read8_o).
//  * y_dh[4 g4 + c] = O^T[d = 32 dh + 8 g4 + 4 half + c][query l & 31]: a register quad is 4 consecutive dims, one
//    uint2 of bf16 (pack_o_quad).
#pragma once
#include "vp_common.h"

namespace vp {

namespace {

constexpr float kLog2e = 1.4426950408889634f;

// capped_exp_exact's / capped_exp16's constants c1 = 2 log2(e) / cap, c2 = cap log2(e).  The kernels (on the device)
// and the fused temporal attention's launch arguments (on the host, vp_internal.h set_tattn_cap) both take them from
// here: the same IEEE fp32 operations
__host__ __device__ __forceinline__ float cap_c1(float cap) { return 2.0f * kLog2e / cap; }
__host__ __device__ __forceinline__ float cap_c2(float cap) { return cap * kLog2e; }

__device__ __forceinline__ int swzK(int row) { return (row >> 1) & 7; }
__device__ __forceinline__ int swzV(int row) { return ((row >> 1) & 1) << 2; }

// staging: the source chunk lane `lane` fetches for row `row` of a K (isV = 0) or V piece, and its address in a
// row-major q|k|v (base + col0: the head's q columns of row 0; ld: row stride; sec: the k section's offset, v at
// twice that)
__device__ __forceinline__ int stage_chunk(int row, int lane, int isV) {
  return (lane & 7) ^ (isV ? swzV(row) : swzK(row));
}
template <typename SEC>
__device__ __forceinline__ const bf16_t* stage_src(const bf16_t* base, int64_t row, int64_t ld, SEC sec, int isV,
                                                   int col0, int chunk) {
  return base + row * ld + (isV ? 2 * sec : sec) + col0 + chunk * 8;
}

// LDS address of a pointer into LDS
__device__ __forceinline__ uint32_t lds_addr(const char* p) { return (uint32_t)(uintptr_t)VP_LDS_PTR(p); }

// Q fragment kd of a lane (half = lane >> 5): 8 bf16 of row q_frag_row at q_frag_ptr, given the start of the head's
// q columns in that row
__device__ __forceinline__ int q_frag_row(int q0, int lane) { return q0 + (lane & 31); }
__device__ __forceinline__ const bf16_t* q_frag_ptr(const bf16_t* qrow, int kd, int half) {
  return qrow + 8 * half + 16 * kd;
}

// K and V reads.  B is a pointer into LDS or an LDS address (uint32_t); the sums keep the kernels' grouping
// (base + row, + chunk, + element), which the compiler's address arithmetic follows.
// the 16 B of row krow of the K region at ks that the S^T MFMA step kd takes
template <typename B>
__device__ __forceinline__ B k_read_at(B ks, int krow, int kd, int half) {
  return ks + krow * 128 + (((2 * kd + half) ^ swzK(krow)) << 4);
}

// a lane's transposed read of the V region at vs at key row `key`, dims 32 dh ..
template <typename B>
__device__ __forceinline__ B v_read_at(B vs, int key, int dh, int lane) {
  const int g = lane >> 4, trp = (lane & 15) & 3;
  const int col = 32 * dh + 16 * (g & 1) + 4 * trp;
  return vs + key * 128 + (((col >> 3) ^ swzV(key)) << 4) + (col & 7) * 2;
}

// the 16 numerators of a lane, rounded to bf16, as the two B operands of O^T = V^T.P^T
__device__ __forceinline__ void pack_numerators(const float (&p)[16], bf16x8 (&pf)[2]) {
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    uint32_t u[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) u[j] = pack_bf16x2(p[8 * s + 2 * j], p[8 * s + 2 * j + 1]);
    pf[s] = *reinterpret_cast<bf16x8*>(u);
  }
}

// the A operand V^T from a transposed read and the one 8 rows further
__device__ __forceinline__ bf16x8 v_frag(const s16x4 (&v)[2]) {
  const s16x4 lo = v[0], hi = v[1];
  return bf16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
}

// O^T += V^T.P^T over one 32-key tile: y0 = dims 0..31, y1 = dims 32..63
__device__ __forceinline__ void pv_mfma(const s16x4 (&vr)[2][2][2], const bf16x8 (&pf)[2], f32x16& y0, f32x16& y1) {
#pragma unroll
  for (int s = 0; s < 2; ++s) {
#pragma unroll
    for (int dh = 0; dh < 2; ++dh) {
      const s16x4 lo = vr[s][dh][0], hi = vr[s][dh][1];
      const bf16x8 vf = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
      if (dh == 0) y0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf, pf[s], y0, 0, 0, 0);
      else y1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf, pf[s], y1, 0, 0, 0);
    }
  }
}

// register quad g4 of y, scaled by 1 / row sum, as 4 bf16
__device__ __forceinline__ uint2 pack_o_quad(const f32x16& y, int g4, float inv) {
  return make_uint2(pack_bf16x2(y[4 * g4] * inv, y[4 * g4 + 1] * inv),
                    pack_bf16x2(y[4 * g4 + 2] * inv, y[4 * g4 + 3] * inv));
}

}  // namespace

}  // namespace vp
