// C-ABI of the gallery search (vp_op_topk*, vp_op_rowmask_pack, vp_op_quantize_rows_f8): argument checks, the workspace
// layout and the two passes of retrieval_kernels.hip (per-range candidate lists, then their merge).  The masked calls
// share the unmasked ones' checks, workspace and merge; only the scan differs.  The _f8 calls are the same four with
// the gallery given as e4m3 codes and per-row scales.
#include "vp_internal.h"

using namespace vpi;

namespace {

// candidate lists of the most row ranges a search uses: scores [parts][Q][k] fp32, then ids [parts][Q][k] int64
struct TopkWs {
  size_t scores = 0, ids = 0, total = 0;
};

TopkWs topk_ws(int64_t Q, int64_t k) {
  TopkWs L;
  const size_t n = (size_t)vp::kTopkMaxParts * (size_t)Q * (size_t)k;
  L.ids = align256(n * 4);
  L.total = align256(L.ids + n * 8);
  return L;
}

// the grouped search's lists: the same two arrays, then groups [parts][Q][k] int64
struct TopkGroupsWs {
  size_t scores = 0, ids = 0, groups = 0, total = 0;
};

TopkGroupsWs topk_groups_ws(int64_t Q, int64_t k) {
  TopkGroupsWs L;
  const size_t n = (size_t)vp::kTopkMaxParts * (size_t)Q * (size_t)k;
  L.ids = align256(n * 4);
  L.groups = align256(L.ids + n * 8);
  L.total = align256(L.groups + n * 8);
  return L;
}

int check_topk_k(int64_t Q, int64_t k, const char* op = "topk") {
  const std::string o = std::string(op) + ": ";
  if (Q < 0) return fail(VP_EINVAL, o + "Q must be >= 0");
  if (k < 1) return fail(VP_EINVAL, o + "k must be >= 1");
  if (k > vp::kTopkMaxK) return fail(VP_ENOTSUP, o + "k must be <= 128");
  if (Q > (int64_t)16 * 65535) return fail(VP_ENOTSUP, o + "Q must be <= 1048560");
  return VP_OK;
}

bool misaligned(const void* p) { return reinterpret_cast<uintptr_t>(p) & 15; }

// the masked calls' two arguments: a mask wherever there are rows, 4-byte aligned; stride 0 (one mask for all queries)
// or at least a mask's words
int check_mask(const std::string& o, const uint32_t* mask, int64_t mask_stride, int64_t N) {
  if (!mask && N != 0) return fail(VP_EINVAL, o + "null mask (the unmasked call searches every row)");
  if (reinterpret_cast<uintptr_t>(mask) & 3) return fail(VP_EINVAL, o + "mask must be 4-byte aligned");
  if (mask_stride < 0 || (mask_stride > 0 && mask_stride < (N + 31) / 32))
    return fail(VP_EINVAL, o + "mask_query_stride_words must be 0 or >= ceil(N / 32)");
  // a list of the masked scan counts rows from its first tile to the gallery's end, in 32 bits
  if (N >= (int64_t)0xffffffff) return fail(VP_ENOTSUP, o + "N must be < 2^32 - 1");
  return VP_OK;
}

// the gallery of a call: fp32 or bf16 rows (gallery_dtype), or with f8 the e4m3 codes in `gallery` and their scales
struct Gallery {
  const void* gallery;
  int gallery_dtype;
  const float* scales;
  bool f8;
};

// the gallery's own argument checks, after the null checks of the call's other pointers
int check_gallery(const std::string& o, const Gallery& g, int64_t N) {
  if (!g.gallery && N != 0) return fail(VP_EINVAL, o + (g.f8 ? "null codes" : "null gallery"));
  if (g.f8 && !g.scales && N != 0) return fail(VP_EINVAL, o + "null scales");
  return VP_OK;
}

int check_gallery_layout(const std::string& o, const Gallery& g, int64_t ld, int64_t D) {
  if (!g.f8 && g.gallery_dtype != VP_F32 && g.gallery_dtype != VP_BF16)
    return fail(VP_ENOTSUP, o + "gallery_dtype must be VP_F32 or VP_BF16");
  if (D < 64 || D % 64) return fail(VP_ENOTSUP, o + "D must be a positive multiple of 64");
  if (D > vp::kPoolMaxD) return fail(VP_ENOTSUP, o + "D must be <= 1536");
  if (ld < D) return fail(VP_EINVAL, o + "ld must be >= D");
  if (g.f8) {
    if (ld % 16) return fail(VP_EINVAL, o + "ld must be a multiple of 16 bytes");
  } else if (ld % 8) {
    return fail(VP_EINVAL, o + "ld must be a multiple of 8 elements");
  }
  return VP_OK;
}

int gallery_storage(const Gallery& g) {
  return g.f8 ? vp::kGalleryF8 : g.gallery_dtype == VP_BF16 ? vp::kGalleryBF16 : vp::kGalleryF32;
}

// vp_op_topk (masked false: mask and mask_stride unused), vp_op_topk_masked and their _f8 forms; `op` names the call
// in messages
int topk_call(const char* op, bool masked, const float* queries, int64_t Q, const Gallery& g, int64_t N, int64_t ld,
              int64_t D, int64_t k, int64_t id_base, const uint32_t* mask, int64_t mask_stride, float* scores,
              int64_t* ids, void* ws, size_t ws_bytes, void* stream) {
  const std::string o = std::string(op) + ": ";
  const void* gallery = g.gallery;
  if (!queries) return fail(VP_EINVAL, o + "null queries");
  if (int rc = check_gallery(o, g, N)) return rc;
  if (!scores) return fail(VP_EINVAL, o + "null scores");
  if (!ids) return fail(VP_EINVAL, o + "null ids");
  if (!ws) return fail(VP_EINVAL, o + "null ws");
  if (N < 0) return fail(VP_EINVAL, o + "N must be >= 0");
  if (masked) {
    if (int rc = check_mask(o, mask, mask_stride, N)) return rc;
  }
  if (int rc = check_topk_k(Q, k, op)) return rc;
  if (int rc = check_gallery_layout(o, g, ld, D)) return rc;
  if (misaligned(queries)) return fail(VP_EINVAL, o + "queries must be 16-byte aligned");
  if (misaligned(gallery)) return fail(VP_EINVAL, o + (g.f8 ? "codes" : "gallery") + " must be 16-byte aligned");
  if (g.f8 && (reinterpret_cast<uintptr_t>(g.scales) & 3)) return fail(VP_EINVAL, o + "scales must be 4-byte aligned");
  if (misaligned(ws)) return fail(VP_EINVAL, o + "ws must be 16-byte aligned");
  const TopkWs L = topk_ws(Q, k);
  if (ws_bytes < L.total) return fail(VP_EINVAL, o + "ws_bytes too small: need " + std::to_string(L.total));
  if (Q == 0) return VP_OK;
  hipStream_t s = static_cast<hipStream_t>(stream);
  char* w = static_cast<char*>(ws);
  float* ws_sc = reinterpret_cast<float*>(w + L.scores);
  int64_t* ws_id = reinterpret_cast<int64_t*>(w + L.ids);
  int parts = 0;
  if (masked)
    VP_HIP(vp::topk_scan_masked(queries, Q, gallery, gallery_storage(g), N, ld, (int)D, (int)k, id_base, mask,
                                mask_stride, ws_sc, ws_id, &parts, s, g.scales));
  else
    VP_HIP(vp::topk_scan(queries, Q, gallery, gallery_storage(g), N, ld, (int)D, (int)k, id_base, ws_sc, ws_id, &parts,
                         s, g.scales));
  VP_HIP(vp::topk_merge(ws_sc, ws_id, parts, Q, (int)k, (int)k, scores, ids, s));
  return VP_OK;
}

// vp_op_topk_groups, vp_op_topk_groups_masked and their _f8 forms, as topk_call
int topk_groups_call(const char* op, bool masked, const float* queries, int64_t Q, const Gallery& g, int64_t N,
                     int64_t ld, int64_t D, const int64_t* labels, int64_t k, int64_t id_base, const uint32_t* mask,
                     int64_t mask_stride, float* scores, int64_t* groups, int64_t* ids, void* ws, size_t ws_bytes,
                     void* stream) {
  const std::string o = std::string(op) + ": ";
  const void* gallery = g.gallery;
  if (!queries) return fail(VP_EINVAL, o + "null queries");
  if (int rc = check_gallery(o, g, N)) return rc;
  if (!labels && N != 0) return fail(VP_EINVAL, o + "null labels");
  if (!scores) return fail(VP_EINVAL, o + "null scores");
  if (!groups) return fail(VP_EINVAL, o + "null groups");
  if (!ids) return fail(VP_EINVAL, o + "null ids");
  if (!ws) return fail(VP_EINVAL, o + "null ws");
  if (N < 0) return fail(VP_EINVAL, o + "N must be >= 0");
  if (masked) {
    if (int rc = check_mask(o, mask, mask_stride, N)) return rc;
  }
  if (int rc = check_topk_k(Q, k, op)) return rc;
  if (int rc = check_gallery_layout(o, g, ld, D)) return rc;
  if (misaligned(queries)) return fail(VP_EINVAL, o + "queries must be 16-byte aligned");
  if (misaligned(gallery)) return fail(VP_EINVAL, o + (g.f8 ? "codes" : "gallery") + " must be 16-byte aligned");
  if (g.f8 && (reinterpret_cast<uintptr_t>(g.scales) & 3)) return fail(VP_EINVAL, o + "scales must be 4-byte aligned");
  if (reinterpret_cast<uintptr_t>(labels) & 7) return fail(VP_EINVAL, o + "labels must be 8-byte aligned");
  if (misaligned(ws)) return fail(VP_EINVAL, o + "ws must be 16-byte aligned");
  const TopkGroupsWs L = topk_groups_ws(Q, k);
  if (ws_bytes < L.total) return fail(VP_EINVAL, o + "ws_bytes too small: need " + std::to_string(L.total));
  if (Q == 0) return VP_OK;
  hipStream_t s = static_cast<hipStream_t>(stream);
  char* w = static_cast<char*>(ws);
  float* ws_sc = reinterpret_cast<float*>(w + L.scores);
  int64_t* ws_id = reinterpret_cast<int64_t*>(w + L.ids);
  int64_t* ws_gr = reinterpret_cast<int64_t*>(w + L.groups);
  int parts = 0;
  if (masked)
    VP_HIP(vp::topk_groups_scan_masked(queries, Q, gallery, gallery_storage(g), N, ld, (int)D, (int)k, labels, id_base,
                                       mask, mask_stride, ws_sc, ws_id, ws_gr, &parts, s, g.scales));
  else
    VP_HIP(vp::topk_groups_scan(queries, Q, gallery, gallery_storage(g), N, ld, (int)D, (int)k, labels, id_base, ws_sc,
                                ws_id, ws_gr, &parts, s, g.scales));
  VP_HIP(vp::topk_groups_merge(ws_sc, ws_gr, ws_id, parts, Q, (int)k, (int)k, scores, groups, ids, s));
  return VP_OK;
}

}  // namespace

extern "C" {

int vp_op_topk_workspace_bytes(int64_t Q, int64_t k, size_t* bytes) {
  if (!bytes) return fail(VP_EINVAL, "topk: null bytes");
  if (int rc = check_topk_k(Q, k)) return rc;
  *bytes = topk_ws(Q, k).total;
  return VP_OK;
}

int vp_op_topk(const float* queries, int64_t Q, const void* gallery, int gallery_dtype, int64_t N, int64_t ld, int64_t D,
               int64_t k, int64_t id_base, float* scores, int64_t* ids, void* ws, size_t ws_bytes, void* stream) {
  return topk_call("topk", false, queries, Q, {gallery, gallery_dtype, nullptr, false}, N, ld, D, k, id_base, nullptr, 0, scores, ids, ws,
                   ws_bytes, stream);
}

int vp_op_topk_masked(const float* queries, int64_t Q, const void* gallery, int gallery_dtype, int64_t N, int64_t ld,
                      int64_t D, int64_t k, int64_t id_base, const uint32_t* mask, int64_t mask_query_stride_words,
                      float* scores, int64_t* ids, void* ws, size_t ws_bytes, void* stream) {
  return topk_call("topk_masked", true, queries, Q, {gallery, gallery_dtype, nullptr, false}, N, ld, D, k, id_base, mask,
                   mask_query_stride_words, scores, ids, ws, ws_bytes, stream);
}

int vp_op_rowmask_pack(const uint8_t* allow, int64_t Q, int64_t N, const uint32_t* and_words, int64_t and_stride,
                       uint32_t* out_words, int64_t stride, void* stream) {
  if (Q < 0) return fail(VP_EINVAL, "rowmask_pack: Q must be >= 0");
  if (N < 0) return fail(VP_EINVAL, "rowmask_pack: N must be >= 0");
  const int64_t words = (N + 31) / 32;
  if (stride < words) return fail(VP_EINVAL, "rowmask_pack: stride must be >= ceil(N / 32) words");
  if (and_stride < 0 || (and_words && and_stride > 0 && and_stride < words))
    return fail(VP_EINVAL, "rowmask_pack: and_stride must be 0 or >= ceil(N / 32) words");
  if (Q == 0 || N == 0) return VP_OK;
  if (!allow) return fail(VP_EINVAL, "rowmask_pack: null allow");
  if (!out_words) return fail(VP_EINVAL, "rowmask_pack: null out_words");
  if (reinterpret_cast<uintptr_t>(out_words) & 3) return fail(VP_EINVAL, "rowmask_pack: out_words must be 4-byte aligned");
  if (reinterpret_cast<uintptr_t>(and_words) & 3) return fail(VP_EINVAL, "rowmask_pack: and_words must be 4-byte aligned");
  if (N > ((int64_t)1 << 38)) return fail(VP_ENOTSUP, "rowmask_pack: N must be <= 2^38");
  VP_HIP(vp::rowmask_pack(allow, Q, N, and_words, and_words ? and_stride : 0, out_words, stride,
                          static_cast<hipStream_t>(stream)));
  return VP_OK;
}

int vp_op_topk_merge(const float* scores_in, const int64_t* ids_in, int64_t parts, int64_t Q, int64_t k_in, int64_t k,
                     float* scores, int64_t* ids, void* stream) {
  if (!scores_in) return fail(VP_EINVAL, "topk_merge: null scores_in");
  if (!ids_in) return fail(VP_EINVAL, "topk_merge: null ids_in");
  if (!scores) return fail(VP_EINVAL, "topk_merge: null scores");
  if (!ids) return fail(VP_EINVAL, "topk_merge: null ids");
  if (parts < 1) return fail(VP_EINVAL, "topk_merge: parts must be >= 1");
  if (Q < 0 || Q > 0x7fffffff) return fail(VP_EINVAL, "topk_merge: Q must be in [0, 2^31)");
  if (k < 1) return fail(VP_EINVAL, "topk_merge: k must be >= 1");
  if (k > k_in) return fail(VP_EINVAL, "topk_merge: k must be <= k_in");
  if (k_in > vp::kTopkMaxK) return fail(VP_ENOTSUP, "topk_merge: k_in must be <= 128");
  if (Q == 0) return VP_OK;
  VP_HIP(vp::topk_merge(scores_in, ids_in, parts, Q, (int)k_in, (int)k, scores, ids, static_cast<hipStream_t>(stream)));
  return VP_OK;
}

int vp_op_topk_groups_workspace_bytes(int64_t Q, int64_t k, size_t* bytes) {
  if (!bytes) return fail(VP_EINVAL, "topk_groups: null bytes");
  if (int rc = check_topk_k(Q, k, "topk_groups")) return rc;
  *bytes = topk_groups_ws(Q, k).total;
  return VP_OK;
}

int vp_op_topk_groups(const float* queries, int64_t Q, const void* gallery, int gallery_dtype, int64_t N, int64_t ld,
                      int64_t D, const int64_t* labels, int64_t k, int64_t id_base, float* scores, int64_t* groups,
                      int64_t* ids, void* ws, size_t ws_bytes, void* stream) {
  return topk_groups_call("topk_groups", false, queries, Q, {gallery, gallery_dtype, nullptr, false}, N, ld, D, labels, k, id_base,
                          nullptr, 0, scores, groups, ids, ws, ws_bytes, stream);
}

int vp_op_topk_groups_masked(const float* queries, int64_t Q, const void* gallery, int gallery_dtype, int64_t N,
                             int64_t ld, int64_t D, const int64_t* labels, int64_t k, int64_t id_base,
                             const uint32_t* mask, int64_t mask_query_stride_words, float* scores, int64_t* groups,
                             int64_t* ids, void* ws, size_t ws_bytes, void* stream) {
  return topk_groups_call("topk_groups_masked", true, queries, Q, {gallery, gallery_dtype, nullptr, false}, N, ld, D, labels, k, id_base,
                          mask, mask_query_stride_words, scores, groups, ids, ws, ws_bytes, stream);
}

int vp_op_topk_groups_merge(const float* scores_in, const int64_t* groups_in, const int64_t* ids_in, int64_t parts,
                            int64_t Q, int64_t k_in, int64_t k, float* scores, int64_t* groups, int64_t* ids,
                            void* stream) {
  if (!scores_in) return fail(VP_EINVAL, "topk_groups_merge: null scores_in");
  if (!groups_in) return fail(VP_EINVAL, "topk_groups_merge: null groups_in");
  if (!ids_in) return fail(VP_EINVAL, "topk_groups_merge: null ids_in");
  if (!scores) return fail(VP_EINVAL, "topk_groups_merge: null scores");
  if (!groups) return fail(VP_EINVAL, "topk_groups_merge: null groups");
  if (!ids) return fail(VP_EINVAL, "topk_groups_merge: null ids");
  if (parts < 1) return fail(VP_EINVAL, "topk_groups_merge: parts must be >= 1");
  if (Q < 0 || Q > 0x7fffffff) return fail(VP_EINVAL, "topk_groups_merge: Q must be in [0, 2^31)");
  if (k < 1) return fail(VP_EINVAL, "topk_groups_merge: k must be >= 1");
  if (k > k_in) return fail(VP_EINVAL, "topk_groups_merge: k must be <= k_in");
  if (k_in > vp::kTopkMaxK) return fail(VP_ENOTSUP, "topk_groups_merge: k_in must be <= 128");
  if (Q == 0) return VP_OK;
  VP_HIP(vp::topk_groups_merge(scores_in, groups_in, ids_in, parts, Q, (int)k_in, (int)k, scores, groups, ids,
                               static_cast<hipStream_t>(stream)));
  return VP_OK;
}

// ---- the fp8 gallery (DESIGN.md §4 "fp8 gallery"): the quantiser and the four searches over codes and scales ----
int vp_op_quantize_rows_f8(const void* x, int x_dtype, int64_t N, int64_t ldx, int64_t D, uint8_t* codes, int64_t ldc,
                           float* scales, void* stream) {
  const std::string o = "quantize_rows_f8: ";
  if (N < 0) return fail(VP_EINVAL, o + "N must be >= 0");
  if (!x && N != 0) return fail(VP_EINVAL, o + "null x");
  if (!codes && N != 0) return fail(VP_EINVAL, o + "null codes");
  if (!scales && N != 0) return fail(VP_EINVAL, o + "null scales");
  if (x_dtype != VP_F32 && x_dtype != VP_BF16) return fail(VP_ENOTSUP, o + "x_dtype must be VP_F32 or VP_BF16");
  if (D < 64 || D % 64) return fail(VP_ENOTSUP, o + "D must be a positive multiple of 64");
  if (D > vp::kPoolMaxD) return fail(VP_ENOTSUP, o + "D must be <= 1536");
  if (ldx < D) return fail(VP_EINVAL, o + "ldx must be >= D");
  if (ldx % (x_dtype == VP_BF16 ? 8 : 4)) return fail(VP_EINVAL, o + "ldx must be a multiple of 16 bytes");
  if (ldc < D) return fail(VP_EINVAL, o + "ldc must be >= D");
  if (ldc % 16) return fail(VP_EINVAL, o + "ldc must be a multiple of 16 bytes");
  if (misaligned(x)) return fail(VP_EINVAL, o + "x must be 16-byte aligned");
  if (misaligned(codes)) return fail(VP_EINVAL, o + "codes must be 16-byte aligned");
  if (reinterpret_cast<uintptr_t>(scales) & 3) return fail(VP_EINVAL, o + "scales must be 4-byte aligned");
  if (N > ((int64_t)1 << 32)) return fail(VP_ENOTSUP, o + "N must be <= 2^32");
  if (N == 0) return VP_OK;
  VP_HIP(vp::quantize_rows_f8(x, x_dtype == VP_BF16, N, ldx, (int)D, codes, ldc, scales,
                              static_cast<hipStream_t>(stream)));
  return VP_OK;
}

int vp_op_topk_f8(const float* queries, int64_t Q, const uint8_t* codes, const float* scales, int64_t N, int64_t ld,
                  int64_t D, int64_t k, int64_t id_base, float* scores, int64_t* ids, void* ws, size_t ws_bytes,
                  void* stream) {
  return topk_call("topk_f8", false, queries, Q, {codes, 0, scales, true}, N, ld, D, k, id_base, nullptr, 0, scores, ids,
                   ws, ws_bytes, stream);
}

int vp_op_topk_groups_f8(const float* queries, int64_t Q, const uint8_t* codes, const float* scales, int64_t N,
                         int64_t ld, int64_t D, const int64_t* labels, int64_t k, int64_t id_base, float* scores,
                         int64_t* groups, int64_t* ids, void* ws, size_t ws_bytes, void* stream) {
  return topk_groups_call("topk_groups_f8", false, queries, Q, {codes, 0, scales, true}, N, ld, D, labels, k, id_base,
                          nullptr, 0, scores, groups, ids, ws, ws_bytes, stream);
}

int vp_op_topk_masked_f8(const float* queries, int64_t Q, const uint8_t* codes, const float* scales, int64_t N,
                         int64_t ld, int64_t D, int64_t k, int64_t id_base, const uint32_t* mask,
                         int64_t mask_query_stride_words, float* scores, int64_t* ids, void* ws, size_t ws_bytes,
                         void* stream) {
  return topk_call("topk_masked_f8", true, queries, Q, {codes, 0, scales, true}, N, ld, D, k, id_base, mask,
                   mask_query_stride_words, scores, ids, ws, ws_bytes, stream);
}

int vp_op_topk_groups_masked_f8(const float* queries, int64_t Q, const uint8_t* codes, const float* scales, int64_t N,
                                int64_t ld, int64_t D, const int64_t* labels, int64_t k, int64_t id_base,
                                const uint32_t* mask, int64_t mask_query_stride_words, float* scores, int64_t* groups,
                                int64_t* ids, void* ws, size_t ws_bytes, void* stream) {
  return topk_groups_call("topk_groups_masked_f8", true, queries, Q, {codes, 0, scales, true}, N, ld, D, labels, k,
                          id_base, mask, mask_query_stride_words, scores, groups, ids, ws, ws_bytes, stream);
}

// Not in the public header: the queries a workgroup of the search takes at (D, k), for tools/retrieval_bench.py's
// traffic (the gallery is read once per such group).  No device call.
int vp_dev_topk_group(int64_t D, int64_t k) { return vp::topk_group((int)D, (int)k); }
// ... and of the grouped search, whose lists hold 16 B an entry (tools/retrieval_groups_bench.py and the tests)
int vp_dev_topk_groups_group(int64_t D, int64_t k) { return vp::topk_groups_group((int)D, (int)k); }

}  // extern "C"
