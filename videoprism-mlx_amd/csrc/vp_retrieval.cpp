// C-ABI of the gallery search (vp_op_topk*): argument checks, the workspace layout and the two passes of
// retrieval_kernels.hip (per-range candidate lists, then their merge).
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
  if (!queries) return fail(VP_EINVAL, "topk: null queries");
  if (!gallery && N != 0) return fail(VP_EINVAL, "topk: null gallery");
  if (!scores) return fail(VP_EINVAL, "topk: null scores");
  if (!ids) return fail(VP_EINVAL, "topk: null ids");
  if (!ws) return fail(VP_EINVAL, "topk: null ws");
  if (N < 0) return fail(VP_EINVAL, "topk: N must be >= 0");
  if (int rc = check_topk_k(Q, k)) return rc;
  if (gallery_dtype != VP_F32 && gallery_dtype != VP_BF16)
    return fail(VP_ENOTSUP, "topk: gallery_dtype must be VP_F32 or VP_BF16");
  if (D < 64 || D % 64) return fail(VP_ENOTSUP, "topk: D must be a positive multiple of 64");
  if (D > vp::kPoolMaxD) return fail(VP_ENOTSUP, "topk: D must be <= 1536");
  if (ld < D) return fail(VP_EINVAL, "topk: ld must be >= D");
  if (ld % 8) return fail(VP_EINVAL, "topk: ld must be a multiple of 8 elements");
  if (misaligned(queries)) return fail(VP_EINVAL, "topk: queries must be 16-byte aligned");
  if (misaligned(gallery)) return fail(VP_EINVAL, "topk: gallery must be 16-byte aligned");
  if (misaligned(ws)) return fail(VP_EINVAL, "topk: ws must be 16-byte aligned");
  const TopkWs L = topk_ws(Q, k);
  if (ws_bytes < L.total) return fail(VP_EINVAL, "topk: ws_bytes too small: need " + std::to_string(L.total));
  if (Q == 0) return VP_OK;
  hipStream_t s = static_cast<hipStream_t>(stream);
  char* w = static_cast<char*>(ws);
  float* ws_sc = reinterpret_cast<float*>(w + L.scores);
  int64_t* ws_id = reinterpret_cast<int64_t*>(w + L.ids);
  int parts = 0;
  VP_HIP(vp::topk_scan(queries, Q, gallery, gallery_dtype == VP_BF16, N, ld, (int)D, (int)k, id_base, ws_sc, ws_id,
                       &parts, s));
  VP_HIP(vp::topk_merge(ws_sc, ws_id, parts, Q, (int)k, (int)k, scores, ids, s));
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
  if (!queries) return fail(VP_EINVAL, "topk_groups: null queries");
  if (!gallery && N != 0) return fail(VP_EINVAL, "topk_groups: null gallery");
  if (!labels && N != 0) return fail(VP_EINVAL, "topk_groups: null labels");
  if (!scores) return fail(VP_EINVAL, "topk_groups: null scores");
  if (!groups) return fail(VP_EINVAL, "topk_groups: null groups");
  if (!ids) return fail(VP_EINVAL, "topk_groups: null ids");
  if (!ws) return fail(VP_EINVAL, "topk_groups: null ws");
  if (N < 0) return fail(VP_EINVAL, "topk_groups: N must be >= 0");
  if (int rc = check_topk_k(Q, k, "topk_groups")) return rc;
  if (gallery_dtype != VP_F32 && gallery_dtype != VP_BF16)
    return fail(VP_ENOTSUP, "topk_groups: gallery_dtype must be VP_F32 or VP_BF16");
  if (D < 64 || D % 64) return fail(VP_ENOTSUP, "topk_groups: D must be a positive multiple of 64");
  if (D > vp::kPoolMaxD) return fail(VP_ENOTSUP, "topk_groups: D must be <= 1536");
  if (ld < D) return fail(VP_EINVAL, "topk_groups: ld must be >= D");
  if (ld % 8) return fail(VP_EINVAL, "topk_groups: ld must be a multiple of 8 elements");
  if (misaligned(queries)) return fail(VP_EINVAL, "topk_groups: queries must be 16-byte aligned");
  if (misaligned(gallery)) return fail(VP_EINVAL, "topk_groups: gallery must be 16-byte aligned");
  if (reinterpret_cast<uintptr_t>(labels) & 7) return fail(VP_EINVAL, "topk_groups: labels must be 8-byte aligned");
  if (misaligned(ws)) return fail(VP_EINVAL, "topk_groups: ws must be 16-byte aligned");
  const TopkGroupsWs L = topk_groups_ws(Q, k);
  if (ws_bytes < L.total) return fail(VP_EINVAL, "topk_groups: ws_bytes too small: need " + std::to_string(L.total));
  if (Q == 0) return VP_OK;
  hipStream_t s = static_cast<hipStream_t>(stream);
  char* w = static_cast<char*>(ws);
  float* ws_sc = reinterpret_cast<float*>(w + L.scores);
  int64_t* ws_id = reinterpret_cast<int64_t*>(w + L.ids);
  int64_t* ws_gr = reinterpret_cast<int64_t*>(w + L.groups);
  int parts = 0;
  VP_HIP(vp::topk_groups_scan(queries, Q, gallery, gallery_dtype == VP_BF16, N, ld, (int)D, (int)k, labels, id_base,
                              ws_sc, ws_id, ws_gr, &parts, s));
  VP_HIP(vp::topk_groups_merge(ws_sc, ws_gr, ws_id, parts, Q, (int)k, (int)k, scores, groups, ids, s));
  return VP_OK;
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

// Not in the public header: the queries a workgroup of the search takes at (D, k), for tools/retrieval_bench.py's
// traffic (the gallery is read once per such group).  No device call.
int vp_dev_topk_group(int64_t D, int64_t k) { return vp::topk_group((int)D, (int)k); }
// ... and of the grouped search, whose lists hold 16 B an entry (tools/retrieval_groups_bench.py and the tests)
int vp_dev_topk_groups_group(int64_t D, int64_t k) { return vp::topk_groups_group((int)D, (int)k); }

}  // extern "C"
