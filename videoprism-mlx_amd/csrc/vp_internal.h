// Host-side internals shared by the C-ABI translation units (vp_abi.cpp: FactorizedEncoder,
// vp_clip.cpp: FactorizedVideoCLIP): parameter intake, weight packing, workspace layout and the
// pre-LN transformer-stack schedule over the HIP kernels.
#pragma once
#include "../../include/videoprism_hip.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "attention_tile.h"
#include "vp_kernels.h"
#include "vp_params.h"

namespace vpi {

// jax.image.resize(method='bilinear') weights W[in][out] (restated in oracle/ and DESIGN.md:
// triangle kernel, half-pixel centres, antialiased when downsampling, normalised columns).
inline std::vector<double> resize_weights(int in_size, int out_size) {
  std::vector<double> w((size_t)in_size * out_size, 0.0);
  const double scale = (double)out_size / in_size;
  const double inv_scale = 1.0 / scale;
  const double kscale = std::max(inv_scale, 1.0);
  for (int o = 0; o < out_size; ++o) {
    const double sf = (o + 0.5) * inv_scale - 0.5;
    double tot = 0.0;
    for (int i = 0; i < in_size; ++i) {
      const double x = std::fabs(sf - i) / kscale;
      const double v = std::max(0.0, 1.0 - x);
      w[(size_t)i * out_size + o] = v;
      tot += v;
    }
    const bool inside = sf >= -0.5 && sf <= in_size - 0.5;
    for (int i = 0; i < in_size; ++i) {
      double& v = w[(size_t)i * out_size + o];
      if (!inside || !(std::fabs(tot) > 1000.0 * 1.1920928955078125e-07)) v = 0.0;
      else v = v / (tot != 0.0 ? tot : 1.0);
    }
  }
  return w;
}

struct LayerW {  // one transformer layer, packed
  void* wqkv = nullptr;  // [3D][D]   rows (q|k|v, head, dh); q rows scaled by dh^-0.5
  float* bqkv = nullptr; // [3D]
  void* wpost = nullptr; // [D][D]    (out d, in n*H+h)
  float* bpost = nullptr;
  float *ln1_g = nullptr, *ln1_b = nullptr, *ln2_g = nullptr, *ln2_b = nullptr;
  // norm_policy 'primer_hybrid': ln1 / ln2 are the pre_layer_norms, these the post_layer_norms of the attention
  // and FFN sublayers (gamma = 1 + scale), applied before the residual (layernorm_residual)
  float *pn1_g = nullptr, *pn1_b = nullptr, *pn2_g = nullptr, *pn2_b = nullptr;
  void* w1 = nullptr;    // [F][D]
  float* b1 = nullptr;
  // bf16 handles fold LN1 / LN2 into the consuming GEMM (EPI_*_LN): wqkv / w1 hold
  // W' = W diag(1+scale), bqkv / b1 hold b + W beta, and c = row sums of bf16(W')
  float* cqkv = nullptr;
  float* c1 = nullptr;
  void* w2 = nullptr;    // [D][F]
  float* b2 = nullptr;
  // temporal layers (bf16, folded): the q and k rows of wqkv regrouped per head, [q_h | k_h] for
  // h = 0..heads-1 ([2D][D]), with their b' and c -- the first launch of the fused temporal
  // attention (EPI_QK_TATTN_LN); the v rows stay at wqkv + 2 D rows
  void* wqk = nullptr;
  float* bqk = nullptr;
  float* cqk = nullptr;
  // bf16, folded, F % 256 == 0: w1 / b1 / c1 rows permuted within each 32-row group (W row 16h + 4g + i
  // holds column 8g + 4h + i) for the FFN pair over the row-blocked hidden activation (EPI_*_BLK)
  bool ffn_blk = false;
  // spatial stacks (bf16, folded, 3D % 256 == 0): a copy of wqkv / b' / c with the rows permuted the same
  // way, for the q|k|v projection into the row-blocked layout the spatial attention reads (EPI_BF16_LN_BLK)
  void* wqkv_blk = nullptr;
  float* bqkv_blk = nullptr;
  float* cqkv_blk = nullptr;
};

// temporal positional tables precomputed by vp_finalize (T = 1..kPrecomputedT); longer clips get
// theirs from vp_prepare_frames (encoders.py:543-553 interpolates to any T)
constexpr int kPrecomputedT = 32;

enum ProfClass {
  PC_PATCHIFY = 0, PC_GEMM_PATCH, PC_LAYERNORM, PC_GEMM_QKV, PC_ATTN_SPATIAL, PC_ATTN_TEMPORAL,
  PC_GEMM_POST, PC_GEMM_FFN1, PC_GEMM_FFN2, PC_ATTN_AUX, PC_ATTN_TEXT, PC_POOL, PC_MISC,
  PC_GEMM_QKV_TATTN, PC_COUNT
};
inline const char* kProfNames[PC_COUNT] = {"patchify", "gemm_patch_embed", "layernorm", "gemm_qkv",
                                    "attention_spatial", "attention_temporal", "gemm_post",
                                    "gemm_ffn1_gelu", "gemm_ffn2", "attention_aux", "text_tower",
                                    "pooler", "misc", "gemm_qkv_temporal_attn"};

// HIP-event profiler: start/stop events around each launch on the launch stream.
struct Profiler {
  const void* kfn[PC_COUNT] = {};  // host function of the last kernel launched per class
  std::string kname[PC_COUNT];    // its demangled name (vp_profile_kernel_name)
  int cap = 0, used = 0;
  uint32_t mask = 0xffffffffu;  // kernel classes that get events (vp_profile_set_mask)
  std::vector<hipEvent_t> ev;
  std::vector<int> cls;
  std::vector<double> flops, bytes;
};

}  // namespace

struct vp_handle : vpi::ParamStore {
  vp_config cfg;
  std::string prefix;  // "" for a FactorizedEncoder, "vision_encoder/" inside a vp_clip, "encoder/" inside a vp_classifier
  bool bf16() const { return cfg.fprop_dtype == VP_BF16; }
  // packed device weights
  int kpad = 0;
  void* wpatch = nullptr;      // [D][kpad]
  void* wpatch_v = nullptr;    // bf16, vp::video_patch_ok(P) (even P, 4..20): [D][video_patch_k(P)] in the frames' chunk order (fused
                               // patch embedding straight from the frames, gemm_bf16_w4_video)
  float* bpatch = nullptr;
  float* spatial_pos = nullptr;    // [pos_h*pos_w][D]
  std::vector<float> spatial_pos_host;                   // kept for other patch grids
  std::map<std::pair<int, int>, float*> grid_pos;        // interpolated tables (vp_prepare_geometry)
  std::vector<float> temporal_pos_host;                  // temporal_pos_emb/emb_var [pos_t][D]
  std::map<int, float*> temporal_pos;                    // T -> [T][D] (resampled when T != pos_t)
  std::vector<vpi::LayerW> spatial, temporal;
  float *sln_g = nullptr, *sln_b = nullptr, *tln_g = nullptr, *tln_b = nullptr;
  vpi::Profiler prof;
};

namespace vpi {

inline bool is_bf16(const vp_handle* h) { return h->bf16(); }

// the 16 leaves of a scanned StackedTransformer (layers.py:940-1041) under `pre` (".../x_layers/"); primer
// (norm_policy 'primer_hybrid', layers.py:347-351): 20, a pre_layer_norm and a post_layer_norm pair in place of each
// layer_norm pair
inline void add_stack_expected(ParamStore& ps, const std::string& pre, int64_t L, int64_t D, int64_t F, int64_t NH,
                               bool primer = false) {
  const int64_t DH = D / NH;
  auto add_ln = [&](const std::string& at) {
    for (const char* ln : {"pre_layer_norm", "post_layer_norm", "layer_norm"}) {
      if (primer == !std::strcmp(ln, "layer_norm")) continue;
      ps.expect(at + ln + "/scale", {L, D});
      ps.expect(at + ln + "/bias", {L, D});
    }
  };
  add_ln(pre);
  for (const char* qkv : {"query", "key", "value"}) {
    ps.expect(pre + "self_attention/" + qkv + "/w", {L, D, NH, DH});
    ps.expect(pre + "self_attention/" + qkv + "/b", {L, NH, DH});
  }
  ps.expect(pre + "self_attention/post/w", {L, D, NH, DH});
  ps.expect(pre + "self_attention/post/b", {L, D});
  add_ln(pre + "ff_layer/");
  ps.expect(pre + "ff_layer/ffn_layer1/linear/kernel", {L, D, F});
  ps.expect(pre + "ff_layer/ffn_layer1/linear/bias", {L, F});
  ps.expect(pre + "ff_layer/ffn_layer2/linear/kernel", {L, F, D});
  ps.expect(pre + "ff_layer/ffn_layer2/linear/bias", {L, D});
}

// A FactorizedEncoder handle whose leaves are named under `prefix` (vp_abi.cpp): vp_create's own with "",
// the encoder wrapped by a vp_clip / vp_classifier with theirs.
int create_encoder(const vp_config* cfg, int device, const std::string& prefix, vp_handle** out);

// LayerNorm folded into the following GEMM (bf16 handles): w [N][K] *= gamma[k],
// b[n] += sum_k w[n][k] beta[k] (before scaling, fp64), c[n] = sum_k bf16(w'[n][k]) (fp64).
// LN(x).W + b = rstd * (x.W') - mean*rstd * c + b'   (layers.py:208-270 with :273-313)
inline std::vector<float> fold_ln(std::vector<float>& w, std::vector<float>& b, const std::vector<float>& gamma,
                           const std::vector<float>& beta, int64_t N, int64_t K) {
  std::vector<float> c(N);
  for (int64_t n = 0; n < N; ++n) {
    double bb = b[n], cs = 0.0;
    float* row = w.data() + (size_t)n * K;
    for (int64_t k = 0; k < K; ++k) {
      bb += (double)row[k] * beta[k];
      row[k] = row[k] * gamma[k];
      const uint16_t r = host_f2bf(row[k]);
      uint32_t u = (uint32_t)r << 16;
      float rf;
      std::memcpy(&rf, &u, 4);
      cs += rf;
    }
    b[n] = (float)bb;
    c[n] = (float)cs;
  }
  return c;
}

// extra copies of the folded q|k|v rows a stack's attention path reads (pack_stack)
enum QkvExtra {
  QKV_PLAIN = 0,    // row-major [3D][D] only (auxiliary / text stacks)
  QKV_PER_HEAD = 1, // + [q_h | k_h] per head (temporal stacks: the fused temporal attention)
  QKV_BLOCKED = 2,  // + the row-blocked copy (spatial stacks: EPI_BF16_LN_BLK -> attn_spatial<.., true>)
};

// one scanned stack `pre` (".../x_layers/") -> L packed layers.  fold: LayerNorms folded into
// the consuming GEMMs (bf16 handles, EPI_*_LN); otherwise W / b are the plain projections and the
// LayerNorms run as kernels (ln*_g / ln*_b).  The row-major q|k|v copy is always kept: it serves the
// unfused attention paths (other patch grids, frame paddings, caps outside the fast range).
inline int pack_stack(ParamStore& ps, bool bf16, const std::string& pre, int L, int64_t D, int64_t F, int NH, bool fold,
                      std::vector<LayerW>& out, QkvExtra extra = QKV_PLAIN, bool primer = false) {
  const bool qk_perm = extra == QKV_PER_HEAD;
  const float qscale = 1.0f / std::sqrt((float)(D / NH));  // layers.py:576-583
  if (primer && fold) return fail(VP_ENOTSUP, "norm_policy 'primer_hybrid' runs with unfolded LayerNorms only");
  const std::string ln = primer ? "pre_layer_norm/" : "layer_norm/";
  const auto& lng = ps.data(pre + ln + "scale");
  const auto& lnb = ps.data(pre + ln + "bias");
  const auto& ln2g = ps.data(pre + "ff_layer/" + ln + "scale");
  const auto& ln2b = ps.data(pre + "ff_layer/" + ln + "bias");
  const std::vector<float>* wq[3] = {&ps.data(pre + "self_attention/query/w"),
                                     &ps.data(pre + "self_attention/key/w"),
                                     &ps.data(pre + "self_attention/value/w")};
  const std::vector<float>* bq[3] = {&ps.data(pre + "self_attention/query/b"),
                                     &ps.data(pre + "self_attention/key/b"),
                                     &ps.data(pre + "self_attention/value/b")};
  const auto& wpost = ps.data(pre + "self_attention/post/w");
  const auto& bpost = ps.data(pre + "self_attention/post/b");
  const auto& w1 = ps.data(pre + "ff_layer/ffn_layer1/linear/kernel");
  const auto& b1 = ps.data(pre + "ff_layer/ffn_layer1/linear/bias");
  const auto& w2 = ps.data(pre + "ff_layer/ffn_layer2/linear/kernel");
  const auto& b2 = ps.data(pre + "ff_layer/ffn_layer2/linear/bias");
  out.resize(L);
  for (int l = 0; l < L; ++l) {
    LayerW& lw = out[l];
    std::vector<float> t((size_t)3 * D * D), tb((size_t)3 * D);
    for (int which = 0; which < 3; ++which) {
      const float sc = which == 0 ? qscale : 1.0f;
      const float* w = wq[which]->data() + (size_t)l * D * D;  // [D_in][N*H]
      for (int64_t k = 0; k < D; ++k)
        for (int64_t n = 0; n < D; ++n) t[((size_t)which * D + n) * D + k] = w[k * D + n] * sc;
      const float* b = bq[which]->data() + (size_t)l * D;
      for (int64_t n = 0; n < D; ++n) tb[(size_t)which * D + n] = b[n] * sc;
    }
    int rc;
    std::vector<float> g1(D), be1(D), g2(D), be2(D);
    for (int64_t i = 0; i < D; ++i) {
      g1[i] = lng[(size_t)l * D + i] + 1.0f;   // direct_scale=False (layers.py:259-260)
      be1[i] = lnb[(size_t)l * D + i];
      g2[i] = ln2g[(size_t)l * D + i] + 1.0f;
      be2[i] = ln2b[(size_t)l * D + i];
    }
    if (fold) {
      const std::vector<float> c = fold_ln(t, tb, g1, be1, 3 * D, D);
      if ((rc = ps.upload_f32(c, &lw.cqkv))) return rc;
      if (extra == QKV_BLOCKED && (3 * D) % 256 == 0) {  // the row-blocked copy (LayerW::wqkv_blk)
        const int64_t N3 = 3 * D;
        std::vector<float> pt((size_t)N3 * D), pb(N3), pc(N3);
        for (int64_t r = 0; r < N3; ++r) {
          const int64_t w = r & 31, src = (r & ~31LL) + 8 * ((w >> 2) & 3) + 4 * (w >> 4) + (w & 3);
          std::memcpy(pt.data() + (size_t)r * D, t.data() + (size_t)src * D, (size_t)D * 4);
          pb[r] = tb[src];
          pc[r] = c[src];
        }
        if ((rc = ps.upload_mat(pt, bf16, &lw.wqkv_blk)) || (rc = ps.upload_f32(pb, &lw.bqkv_blk)) ||
            (rc = ps.upload_f32(pc, &lw.cqkv_blk)))
          return rc;
      }
      if (qk_perm) {  // [q_h | k_h] per head (rows of the folded t, b', c)
        const int64_t DH = D / NH;
        std::vector<float> tq((size_t)2 * D * D), bq((size_t)2 * D), cq((size_t)2 * D);
        for (int64_t hh = 0; hh < NH; ++hh)
          for (int which = 0; which < 2; ++which)
            for (int64_t i = 0; i < DH; ++i) {
              const int64_t src = which * D + hh * DH + i, dst = hh * 2 * DH + which * DH + i;
              std::memcpy(tq.data() + (size_t)dst * D, t.data() + (size_t)src * D, (size_t)D * 4);
              bq[dst] = tb[src];
              cq[dst] = c[src];
            }
        if ((rc = ps.upload_mat(tq, bf16, &lw.wqk)) || (rc = ps.upload_f32(bq, &lw.bqk)) ||
            (rc = ps.upload_f32(cq, &lw.cqk)))
          return rc;
      }
    }
    if ((rc = ps.upload_mat(t, bf16, &lw.wqkv)) || (rc = ps.upload_f32(tb, &lw.bqkv))) return rc;
    // post: w[d][n][h] is already [out D][in N*H]
    std::vector<float> wp(wpost.begin() + (size_t)l * D * D, wpost.begin() + (size_t)(l + 1) * D * D);
    std::vector<float> bp(bpost.begin() + (size_t)l * D, bpost.begin() + (size_t)(l + 1) * D);
    if ((rc = ps.upload_mat(wp, bf16, &lw.wpost)) || (rc = ps.upload_f32(bp, &lw.bpost))) return rc;
    if ((rc = ps.upload_f32(g1, &lw.ln1_g)) || (rc = ps.upload_f32(be1, &lw.ln1_b)) ||
        (rc = ps.upload_f32(g2, &lw.ln2_g)) || (rc = ps.upload_f32(be2, &lw.ln2_b)))
      return rc;
    if (primer) {
      const std::string post[2] = {pre + "post_layer_norm/", pre + "ff_layer/post_layer_norm/"};
      float** dst[2][2] = {{&lw.pn1_g, &lw.pn1_b}, {&lw.pn2_g, &lw.pn2_b}};
      for (int i = 0; i < 2; ++i) {
        const auto& sc = ps.data(post[i] + "scale");
        const auto& bi = ps.data(post[i] + "bias");
        std::vector<float> g(D), b(bi.begin() + (size_t)l * D, bi.begin() + (size_t)(l + 1) * D);
        for (int64_t d = 0; d < D; ++d) g[d] = sc[(size_t)l * D + d] + 1.0f;
        if ((rc = ps.upload_f32(g, dst[i][0])) || (rc = ps.upload_f32(b, dst[i][1]))) return rc;
      }
    }
    std::vector<float> t1((size_t)F * D), t2((size_t)D * F);
    const float* w1l = w1.data() + (size_t)l * D * F;  // [D][F]
    for (int64_t k = 0; k < D; ++k)
      for (int64_t n = 0; n < F; ++n) t1[(size_t)n * D + k] = w1l[k * F + n];
    const float* w2l = w2.data() + (size_t)l * F * D;  // [F][D]
    for (int64_t k = 0; k < F; ++k)
      for (int64_t n = 0; n < D; ++n) t2[(size_t)n * F + k] = w2l[k * D + n];
    std::vector<float> bb1(b1.begin() + (size_t)l * F, b1.begin() + (size_t)(l + 1) * F);
    std::vector<float> bb2(b2.begin() + (size_t)l * D, b2.begin() + (size_t)(l + 1) * D);
    if (fold) {
      std::vector<float> c = fold_ln(t1, bb1, g2, be2, F, D);
      if (F % 256 == 0) {  // rows of W', b', c in the blocked FFN pair's order (LayerW::ffn_blk)
        std::vector<float> pt((size_t)F * D), pb(F), pc(F);
        for (int64_t r = 0; r < F; ++r) {
          const int64_t w = r & 31, src = (r & ~31LL) + 8 * ((w >> 2) & 3) + 4 * (w >> 4) + (w & 3);
          std::memcpy(pt.data() + (size_t)r * D, t1.data() + (size_t)src * D, (size_t)D * 4);
          pb[r] = bb1[src];
          pc[r] = c[src];
        }
        t1.swap(pt);
        bb1.swap(pb);
        c.swap(pc);
        lw.ffn_blk = true;
      }
      if ((rc = ps.upload_f32(c, &lw.c1))) return rc;
    }
    if ((rc = ps.upload_mat(t1, bf16, &lw.w1)) || (rc = ps.upload_f32(bb1, &lw.b1)) ||
        (rc = ps.upload_mat(t2, bf16, &lw.w2)) || (rc = ps.upload_f32(bb2, &lw.b2)))
      return rc;
  }
  return VP_OK;
}

// workspace carve-up (all offsets 256-B aligned)
struct WsLayout {
  size_t x = 0, x2 = 0, hbuf = 0, big = 0, pad_btn = 0, pad_bnt = 0, st_part = 0, ln_rs = 0, total = 0;
};

inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

// ---- the attention pooler's forward (AttenTokenPoolingLayer; pool_stream.h, clip_kernels.hip), as the video-text
// and classifier engines run it on packed weights and as the head's training op runs it on weights it folds ----
// what the pooler kernels take: whole 128-column blocks up to vp::kPoolMaxD, at most vp::kPoolMaxH heads
inline int check_pooler_heads(int64_t num_heads) {
  if (num_heads > vp::kPoolMaxH)
    return fail(VP_ENOTSUP, "pooler kernels support up to " + std::to_string(vp::kPoolMaxH) + " heads");
  return VP_OK;
}
inline int check_pooler_dims(int64_t model_dim, int64_t num_heads) {
  if (int rc = check_pooler_heads(num_heads)) return rc;
  if (model_dim % 128 || model_dim > vp::kPoolMaxD)
    return fail(VP_ENOTSUP, "pooler kernels need model_dim % 128 == 0, at most " + std::to_string(vp::kPoolMaxD));
  return VP_OK;
}

// The weights in the layouts the kernels take (device pointers): U [H][D] (query folded into the key projection),
// Ut = bf16 hi|lo halves of U for the MFMA logits, Wv^T [H][D][dp], bv [H][dp], Wpost^T [H*dp][D], bpost [D],
// LayerNorm gamma (1 + scale) / beta
struct PoolerW {
  const void* Ut = nullptr;
  const float *U = nullptr, *WvT = nullptr, *bv = nullptr, *WpT = nullptr, *bp = nullptr;
  const float *ln_g = nullptr, *ln_b = nullptr;
  int dp = 0;
};

// scratch of one forward over G groups: logits [rows][H], stats [G][H][2], zpart (the chunk sums; the output
// projection's split-K partials reuse it), z [G][H][D], enc [G][H*dp], pooled [G][D]
struct PoolScratch {
  float *logits, *stats, *zpart, *z, *enc, *pooled;
  size_t zpart_floats;  // capacity of zpart
};

// its byte offsets in a workspace, carved from `off` on in that order
struct PoolWs {
  size_t logits = 0, stats = 0, zpart = 0, z = 0, enc = 0, pooled = 0;
  PoolScratch at(void* base) const {
    auto f32 = [&](size_t o) { return reinterpret_cast<float*>(static_cast<char*>(base) + o); };
    return PoolScratch{f32(logits), f32(stats), f32(zpart), f32(z), f32(enc), f32(pooled), (z - zpart) / 4};
  }
};
inline PoolWs carve_pool_ws(size_t& off, int64_t rows, int64_t G, int64_t D, int64_t NH, int64_t dp,
                            size_t zpart_floats) {
  PoolWs L;
  L.logits = off; off = align256(off + (size_t)rows * NH * 4);
  L.stats = off; off = align256(off + (size_t)G * NH * 8);
  L.zpart = off; off = align256(off + zpart_floats * 4);
  L.z = off; off = align256(off + (size_t)G * NH * D * 4);
  L.enc = off; off = align256(off + (size_t)G * NH * dp * 4);
  L.pooled = off; off = align256(off + (size_t)G * D * 4);
  return L;
}

// The two streaming passes over feat [G*Sg][D] (bf: bf16, else fp32): logits, softmax statistics, z (vp_clip.cpp);
// pad: token paddings [G][Sg] or null (vp_kernels.h, pool_logits)
hipError_t pooler_stream(hipStream_t s, int bf, const PoolerW& pw, const void* feat, int G, int Sg, int D, int NH,
                         const PoolScratch& sc, const float* pad = nullptr);
// ... then the value projection per head, the output projection over K = NH * dp (split 8 ways into zpart, free
// again once z is summed, where that fills the device), LayerNorm and, if do_l2, L2 -> dst [G][D]
hipError_t pooler_project(hipStream_t s, const PoolerW& pw, int G, int D, int NH, const PoolScratch& sc, int do_l2,
                          float* dst);

// GEMM row count: B*T*N padded to the GEMM tile (256 rows bf16, 128 fp32); the padding rows
// ride through the row-independent GEMM / LayerNorm kernels and are never read back
inline int64_t padded_rows(const vp_handle* h, int64_t M) {
  const int64_t t = is_bf16(h) ? 256 : 128;
  return (M + t - 1) / t * t;
}

inline WsLayout ws_layout(const vp_handle* h, int64_t B, int64_t T, int64_t H, int64_t W) {
  const int64_t P = h->cfg.patch_size;
  const int64_t Nsp = (H / P) * (W / P);
  const int64_t M = padded_rows(h, B * T * Nsp);
  const int64_t D = h->cfg.model_dim, F = h->cfg.mlp_dim;
  const size_t es = is_bf16(h) ? 2 : 4;
  const int64_t kpad = ((P * P * 3 + 63) / 64) * 64;
  const int64_t bigcols = std::max(std::max(3 * D, F), kpad);
  WsLayout L;
  size_t off = 0;
  // residual streams: fp32, or bf16 when fprop_dtype is bf16 (Flax keeps activations in
  // fprop_dtype between layers, models.py:301-302)
  L.x = off; off = align256(off + (size_t)M * D * es);
  L.x2 = off; off = align256(off + (size_t)M * D * es);
  L.hbuf = off; off = align256(off + (size_t)M * D * es);
  L.big = off; off = align256(off + (size_t)M * bigcols * es);
  L.pad_btn = off; off = align256(off + (size_t)M * 4);
  L.pad_bnt = off; off = align256(off + (size_t)M * 4);
  // GEMM-folded LayerNorm (bf16): per-row partial statistics and (rstd, -mean*rstd)
  L.st_part = off; off = align256(off + (size_t)(D / 128) * M * 8);
  L.ln_rs = off; off = align256(off + (size_t)M * 8);
  L.total = off;
  return L;
}

// Clips per forward chunk: the forward entry points process any B as consecutive chunks of at most this
// many clips (clips are independent, encoders.py:411-580), each in the same workspace, which bounds the
// workspace at about 4 GiB of FFN hidden activation (170 clips of 16 x 288 x 288).  A single clip always
// fits a chunk: the GEMMs walk an operand past the 32-bit buffer range in row ranges (gemm_bf16_w4.hip),
// so clip length is bounded by device memory only.
inline int64_t chunk_clips(const vp_config& c, int64_t T, int64_t H, int64_t W) {
  const int64_t P = c.patch_size;
  const int64_t tok = T * (H / P) * (W / P);
  const int64_t kpad = ((P * P * 3 + 63) / 64) * 64;
  const int64_t lda = std::max<int64_t>(std::max<int64_t>(c.model_dim, c.mlp_dim), kpad);
  const int64_t max_rows = (int64_t)(0xFFFFFFF0ull / (uint64_t)(2 * lda)) / 256 * 256;
  return tok > 0 ? std::max<int64_t>(1, max_rows / tok) : 1;
}

// the reference's message for frames the patch grid does not divide (encoders.py:86-89)
inline std::string patch_size_message(int64_t H, int64_t W, int64_t P) {
  return "Image height (" + std::to_string(H) + ") and width (" + std::to_string(W) +
         ") should be multiples of patch_size (" + std::to_string(P) + ").";
}

inline int check_geometry(const vp_handle* h, int64_t B, int64_t T, int64_t H, int64_t W) {
  const int64_t P = h->cfg.patch_size;
  if (B < 1 || T < 1 || H < 1 || W < 1) return fail(VP_EINVAL, "inputs must be [B, T, H, W, 3] with positive sizes");
  if (H != W) return fail(VP_EINVAL, "assert h == w failed (encoders.py:435)");
  if (H % P || W % P) return fail(VP_EINVAL, patch_size_message(H, W, P));
  if (T * (H / P) * (W / P) > ((int64_t)1 << 30))
    return fail(VP_EINVAL, "one clip of " + std::to_string(T) + "x" + std::to_string(H) + "x" + std::to_string(W) +
                               " has more than 2^30 tokens (32-bit row indices)");
  return VP_OK;
}

// clips per chunk for a forward over B clips
inline int64_t chunk_of(const vp_handle* h, int64_t B, int64_t T, int64_t H, int64_t W) {
  return std::min<int64_t>(B, chunk_clips(h->cfg, T, H, W));
}

inline size_t dtype_bytes(int dtype) { return dtype == VP_U8 ? 1 : dtype == VP_BF16 ? 2 : 4; }

// dtype codes of a forward entry point; spatiotemporal features are the encoder's output itself, so they
// come in the handle's fprop dtype only
inline int check_dtypes(int in_dtype, int out_dtype, bool spatiotemporal_out, int fprop_dtype) {
  if (spatiotemporal_out && out_dtype != fprop_dtype)
    return fail(VP_EINVAL, "spatiotemporal_features are returned in the fprop dtype");
  if ((in_dtype != VP_F32 && in_dtype != VP_BF16 && in_dtype != VP_U8) || (out_dtype != VP_F32 && out_dtype != VP_BF16))
    return fail(VP_EINVAL, "bad dtype");
  return VP_OK;
}

// bytes of one clip of the caller's frames
inline size_t video_clip_bytes(int64_t T, int64_t H, int64_t W, int in_dtype) {
  return (size_t)(T * H * W * 3) * dtype_bytes(in_dtype);
}

// the caller's workspace against `need`; *feat_clip: bytes of one clip of features [T*N][D] in feat_dtype
inline int check_workspace(const vp_handle* h, int64_t T, int64_t H, int64_t W, size_t ws_bytes, size_t need,
                           int feat_dtype, size_t* feat_clip) {
  if (ws_bytes < need) return fail(VP_EINVAL, "workspace too small: need " + std::to_string(need));
  const int64_t P = h->cfg.patch_size;
  *feat_clip = (size_t)(T * (H / P) * (W / P) * h->cfg.model_dim) * dtype_bytes(feat_dtype);
  return VP_OK;
}

// fn(b0, nb) over B clips in consecutive chunks of at most chunk_of(...) clips; stops at the first error
template <class Fn>
int for_each_chunk(const vp_handle* h, int64_t B, int64_t T, int64_t H, int64_t W, Fn&& fn) {
  const int64_t Bc = chunk_of(h, B, T, H, W);
  for (int64_t b0 = 0; b0 < B; b0 += Bc) {
    const int rc = fn(b0, std::min(Bc, B - b0));
    if (rc) return rc;
  }
  return VP_OK;
}

// a caller's buffer `bytes` further on; an absent (null) buffer stays absent
template <class T>
T* advance(T* p, size_t bytes) {
  return p ? reinterpret_cast<T*>(reinterpret_cast<uintptr_t>(p) + bytes) : nullptr;
}

// algorithmic bytes of a GEMM [M][K] . [N][K]^T with es-byte operands (the profiler's roofline input)
inline double gemm_bytes(double M, double K, double N, double es, double out_bytes, double resid_bytes) {
  return M * K * es + N * K * es + M * N * out_bytes + M * N * resid_bytes;
}

inline vp::EpiArgs epi_args(void* out, int64_t ldo, const float* bias, const void* resid, int64_t ldr, const float* pos,
                            int64_t pos_rows, const float* rowpad) {
  vp::EpiArgs ep;
  ep.out = out; ep.ldo = ldo; ep.bias = bias; ep.resid = resid; ep.ldr = ldr;
  ep.pos = pos; ep.pos_rows = (int)pos_rows; ep.rowpad = rowpad;
  return ep;
}

// The bf16 attention kernels compute the capped softmax without a running max: every numerator
// is exp(l) with |l| <= cap, and both the row sum and the unnormalised O = sum_s exp(l_s) v_s are
// accumulated in fp32.  With cap <= 50 (the reference's value for every VideoPrism config,
// models.py:91) and S keys, |O| <= e^50 * S * max|v| stays below FLT_MAX for any |v| < 1.6e13 at
// S = 4096 (16 frames) and |v| < 1e12 at S = 65536 (256 frames of the auxiliary encoder) --
// bf16 activations of a trained model are nowhere near.  (Round 2 allowed 80,
// priced on the row sum alone: e^80 * S * |v| overflows for |v| > ~1.5 at S = 4096.)  Any other
// cap (<= 0: no capping, layers.py:586-589; > 50) takes the online-softmax kernel.
constexpr float kMaxFastCap = 50.0f;
inline bool fast_cap(float cap) { return cap > 0.0f && cap <= kMaxFastCap; }

// what a stack's attention is for (the rest of the pre-LN layer is shared); choose_attention picks the kernel
enum AttnKind {
  ATT_VIDEO = 0,  // factorized encoder: spatial (S = the patch grid) and temporal (S = T) stacks, key paddings
  ATT_LONG = 1,   // auxiliary encoder over T*N tokens, no masks
  ATT_TEXT = 2,   // text tower: causal + key paddings (layers.py:155-179)
};

// the attention kernels (vp_kernels.h)
enum AttnKernel {
  ATTN_SPATIAL = 0,   // attention_spatial_bf16: S == 256
  ATTN_TEMPORAL = 1,  // attention_temporal_bf16: S <= 16
  ATTN_SEQ = 2,       // attention_seq_bf16: 16 < S <= 256, optionally causal
  ATTN_LONG = 3,      // attention_long_bf16: any S, no masks
  ATTN_MASKED = 4,    // attention_masked: online softmax, any S, cap, masks and dtype
  ATTN_F32 = 5,       // attention_f32: S <= 256 (88-wide heads outside the fast cap range: S <= f32_generic_max_s)
  ATTN_F32_MFMA = 6,  // attention_f32_mfma: any S, 0 < cap <= kMaxFastCap
};

// The one choice of attention kernel: the forward (run_stack) and the op-level entry points (vp_op_attention*,
// which the kernel parity tests call) all come through here.  Every kernel but ATTN_MASKED and ATTN_F32 has the
// max-free softmax only, hence fast_cap.  No tier depends on key paddings: ATT_LONG has none by contract and
// every kernel an ATT_VIDEO / ATT_TEXT stack can get takes them.  dh: head width, 64, or 88 in fp32 (supported_dh);
// it moves one boundary: attention_f32's generic kernel keeps K|V of a sequence in LDS, which 88-wide heads fill at
// S = f32_generic_max_s(88) = 224, so without a fast cap (no MFMA kernel from S = 128) longer sequences go to ATTN_MASKED.
inline bool supported_dh(bool bf16, int64_t dh) { return dh == 64 || (!bf16 && dh == 88); }

inline AttnKernel choose_attention(int kind, bool bf16, int64_t S, float cap, bool /*has_key_pad*/, int dh = 64) {
  const bool fast = fast_cap(cap);
  if (kind == ATT_TEXT) return bf16 && fast && S > 16 && S <= 256 ? ATTN_SEQ : ATTN_MASKED;
  if (bf16 && !fast) return ATTN_MASKED;
  if (kind == ATT_LONG) {
    if (!bf16) return fast ? ATTN_F32_MFMA : ATTN_MASKED;
    return S >= 256 ? ATTN_LONG : S > 16 ? ATTN_SEQ : ATTN_TEMPORAL;
  }
  if (!bf16) {
    if (S <= 256 && (S <= vp::f32_generic_max_s(dh) || (fast && S >= 128))) return ATTN_F32;
    return fast ? ATTN_F32_MFMA : ATTN_MASKED;
  }
  return S == 256 ? ATTN_SPATIAL : S <= 16 ? ATTN_TEMPORAL : S < 256 ? ATTN_SEQ : ATTN_MASKED;
}

// vp_op_attention has no kind: sequences past 256 keys without paddings are the auxiliary encoder's
inline int op_attention_kind(int64_t S, bool has_key_pad) { return S > 256 && !has_key_pad ? ATT_LONG : ATT_VIDEO; }

// Launches choose_attention's kernel over qkv [num_seq * S][3 * heads * dh] -> o.  ATT_LONG passes no key
// paddings, only ATT_TEXT a causal mask; blk: q|k|v in the row-blocked layout (ATTN_SPATIAL only).
inline hipError_t launch_attention(int kind, bool bf16, const void* qkv, void* o, int num_seq, int S, int heads, float cap,
                                   const float* key_pad, int causal, bool blk, hipStream_t s, int dh = 64) {
  using namespace vp;
  if (!supported_dh(bf16, dh)) return hipErrorNotSupported;
  if (kind == ATT_LONG) key_pad = nullptr;
  if (kind != ATT_TEXT) causal = 0;
  const bf16_t* qb = static_cast<const bf16_t*>(qkv);
  bf16_t* ob = static_cast<bf16_t*>(o);
  switch (choose_attention(kind, bf16, S, cap, key_pad != nullptr, dh)) {
    case ATTN_SPATIAL: return attention_spatial_bf16(qb, ob, num_seq, heads, cap, key_pad, s, blk);
    case ATTN_TEMPORAL: return attention_temporal_bf16(qb, ob, num_seq, S, heads, cap, key_pad, s);
    case ATTN_SEQ: return attention_seq_bf16(qb, ob, num_seq, S, heads, cap, key_pad, s, causal);
    case ATTN_LONG: return attention_long_bf16(qb, ob, num_seq, S, heads, cap, s);
    case ATTN_MASKED: return attention_masked(qkv, o, bf16, num_seq, S, heads, cap, key_pad, causal, s, dh);
    case ATTN_F32: return attention_f32((const float*)qkv, (float*)o, num_seq, S, heads, cap, key_pad, s, dh);
    case ATTN_F32_MFMA: return attention_f32_mfma((const float*)qkv, (float*)o, num_seq, S, heads, cap, key_pad, s, dh);
  }
  return hipErrorInvalidValue;
}

// the fused temporal attention's cap arguments (EPI_*_TATTN_LN): cap_c1 / cap_c2 are the capped-exp constants
// 2 log2(e) / cap and cap log2(e), the same IEEE division the unfused kernels do on the device: the one expression
// both evaluate (attention_tile.h cap_c1 / cap_c2)
inline void set_tattn_cap(vp::EpiArgs& ep, float cap, int heads) {
  ep.cap = cap; ep.heads = heads;
  ep.cap_c1 = vp::cap_c1(cap);
  ep.cap_c2 = vp::cap_c2(cap);
}

// The fp32 GEMM sums each output in one k-ordered chain, whose rounding error grows as sqrt(K): at Base's and
// Large's widths (K <= 4096) the forward stays at 6e-6 - 7e-6 of the fp64 oracle, at Giant's (K = 1408 and 6144
// in every layer) it reaches the project's 1e-5 bar.  Configurations that are new with Giant -- 88-wide heads, or a
// model_dim that is no multiple of 256 -- run the two-chain kernel (gemm_f32 version 3); every configuration the
// library took before keeps its sums bitwise.
inline bool f32_two_chains(const vp_config& c) {
  return c.fprop_dtype == VP_F32 && (c.model_dim / c.num_heads != 64 || c.model_dim % 256 != 0);
}

// One forward pass's launch context: stream, dtype, row count, scratch buffers and the profiler.
// hipEventRecord on `s`; inside a stream capture an event-record node of the graph instead (a
// plain record during capture only orders the capture, so a replay would not re-record it)
inline hipError_t record_event(hipEvent_t ev, hipStream_t s) {
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  hipGraph_t g = nullptr;
  const hipGraphNode_t* deps = nullptr;
  size_t nd = 0;
  hipError_t e = hipStreamGetCaptureInfo_v2(s, &cs, nullptr, &g, &deps, &nd);
  if (e != hipSuccess) return e;
  if (cs != hipStreamCaptureStatusActive) return hipEventRecord(ev, s);
  hipGraphNode_t node = nullptr;
  e = hipGraphAddEventRecordNode(&node, g, deps, nd, ev);
  if (e != hipSuccess) return e;
  return hipStreamUpdateCaptureDependencies(s, &node, 1, hipStreamSetCaptureDependencies);
}

struct Fwd {
  hipStream_t s = nullptr;
  bool bf = false;
  int M = 0, D = 0, NH = 0;
  float cap = 0.0f;
  int causal = 1;            // ATT_TEXT: merged causal + padding mask (enable_causal_atten)
  bool xs_f32 = false;       // bf16 GEMMs over an fp32 residual stream (text tower; no folding)
  bool small_m = false;      // few rows (text tower): 64 x 64-tile GEMM, K split over the waves (gemm_bf16_small.hip)
  bool f32_two_chains = false;  // fp32 GEMMs with two accumulation chains per output (f32_two_chains(cfg))
  void* hb = nullptr;        // [M][D] LayerNorm / attention output
  void* big = nullptr;       // [M][max(3D, F)] q|k|v, FFN hidden
  float* st_part = nullptr;  // [D/128][M][2] partial row statistics (folded LayerNorm)
  float* ln_rs = nullptr;    // [M][2] (rstd, -mean*rstd)
  Profiler* pf = nullptr;
  int cls_all = -1;          // >= 0: every launch of this context counts in that class (the text tower)

  // profiled launch: records events around `fn` when vp_profile_enable() is active
  template <class Fn>
  hipError_t rec(int cls, double flops, double bytes, Fn&& fn) {
    if (cls_all >= 0) cls = cls_all;
    auto launch = [&]() {
      vp::g_last_kernel = nullptr;
      const hipError_t e = fn();
      if (pf && vp::g_last_kernel) pf->kfn[cls] = vp::g_last_kernel;
      return e;
    };
    if (!pf || pf->used >= pf->cap || !((pf->mask >> cls) & 1u)) return launch();
    const int i = pf->used++;
    hipError_t e = record_event(pf->ev[2 * i], s);
    if (e != hipSuccess) return e;
    e = launch();
    if (e != hipSuccess) return e;
    pf->cls[i] = cls; pf->flops[i] = flops; pf->bytes[i] = bytes;
    return record_event(pf->ev[2 * i + 1], s);
  }

  hipError_t gemm(int epi, const void* A, int K, const void* Wt, int N, void* o, int64_t ldo, const float* bias,
                  const void* resid, const float* pos, int pos_rows, const float* rowpad,
                  const float* lnc = nullptr) const {
    vp::EpiArgs ep = epi_args(o, ldo, bias, resid, ldo, pos, pos_rows, rowpad);
    ep.ln_rs = ln_rs; ep.ln_c = lnc; ep.st_part = st_part; ep.st_rows = M;
    if (bf && small_m) {
      // the text tower's rows are padded to 64 only (clip_text_ws): the 256-row kernels cannot take
      // them, so an epilogue the small-M kernel lacks is an error here, not a fallback
      if (!vp::gemm_bf16_small_ok(epi, M, N, K, K, K)) return hipErrorNotSupported;
      return vp::gemm_bf16_small(epi, (const vp::bf16_t*)A, K, (const vp::bf16_t*)Wt, K, M, N, K, ep, s);
    }
    if (bf) return vp::gemm_bf16_auto(epi, (const vp::bf16_t*)A, K, (const vp::bf16_t*)Wt, K, M, N, K, ep, s);
    return vp::gemm_f32(epi, (const float*)A, K, (const float*)Wt, K, M, N, K, ep, s, f32_two_chains ? 3 : 2);
  }

  // (rstd, -mean*rstd) of the residual stream from the producers' partial statistics
  hipError_t finalize() {
    const double b = (double)M * (D / 128) * 8.0 + (double)M * 8.0;
    return rec(PC_LAYERNORM, 0.0, b, [&] { return vp::ln_stats_finalize(st_part, D / 128, M, ln_rs, s); });
  }

  // pre-LN transformer layers (layers.py:749-872) over num_seq contiguous sequences of S rows of
  // the residual stream xs (in place).  fold: LN1/LN2 folded into the q|k|v / ffn1 GEMMs, with
  // (rstd, -mean*rstd) of xs already in ln_rs on entry.  relu: ReLU FFN (text tower), else GELU.
  // primer: norm_policy 'primer_hybrid' (layers.py:388-430, :819-860) over an fp32 residual stream, unfolded: each
  // sublayer is xs += post_layer_norm(f(pre_layer_norm(xs))), so the post and ffn_layer2 GEMMs store plainly (the
  // q|k|v projection's epilogue) and layernorm_residual adds the normalised result to xs.
  int run_stack(std::vector<LayerW>& layers, void* xs, int num_seq, int S, const float* pad, int F, int acls,
                int kind, bool fold, bool relu, bool primer = false) {
    using namespace vp;
    const double dM = M, dD = D, dF = F, dE = bf ? 2.0 : 4.0;
    auto gbytes = [&](double K, double N, double outb, double resid) { return gemm_bytes(dM, K, N, dE, outb, resid); };
    const double aflops = 4.0 * num_seq * (double)S * S * dD;
    const double abytes = dM * 3 * dD * dE + dM * dD * dE;
    const double ln_bytes = 2.0 * dM * dD * dE;
    const bool xbf = bf && !xs_f32;  // residual stream dtype
    const int epi_resid = xbf ? EPI_RESID_BF16 : EPI_RESID_F32;
    const int epi_resid_ffn = xbf ? EPI_RESID_FFN_BF16 : EPI_RESID_FFN;
    if (primer && (fold || xbf)) return fail(VP_ENOTSUP, "primer_hybrid needs an unfolded stack over an fp32 stream");
    // temporal attention fused into the q|k|v projection (vp_kernels.h EPI_*_TATTN_LN): T = 16
    // frames (one 16-row MFMA block per sequence), dh = 64, no key paddings, max-free cap; the
    // unfused pair stays for every other temporal case (frame paddings, T != 16, other caps)
    const bool tattn = fold && xbf && kind == ATT_VIDEO && S == 16 && !pad && fast_cap(cap) && D == NH * 64 &&
                       !layers.empty() && layers[0].wqk && M % 256 == 0;
    for (size_t li = 0; li < layers.size(); ++li) {
      LayerW& lw = layers[li];
      const bool last = li + 1 == layers.size();
      // spatial layers: q|k|v in the row-blocked layout for the spatial attention kernel
      const bool sblk = fold && xbf && lw.wqkv_blk && kind == ATT_VIDEO && S == 256 && fast_cap(cap) && !tattn;
      if (tattn) {
        // P (normalised bf16 probabilities, 512 B per (sequence, head)) goes to `big`; O to hb
        vp::EpiArgs ep;
        set_tattn_cap(ep, cap, NH);
        ep.ln_rs = ln_rs; ep.out = big; ep.bias = lw.bqk; ep.ln_c = lw.cqk;
        VP_HIP(rec(PC_GEMM_QKV_TATTN, 2.0 * dM * dD * 2 * dD + 4.0 * num_seq * (double)S * S * dD,
                   gbytes(dD, 2 * dD, 0, 0) + dM * NH * 32.0, [&] {
          return gemm_bf16_w4(EPI_QK_TATTN_LN, (const bf16_t*)xs, D, (const bf16_t*)lw.wqk, D, M, 2 * D, D, ep, s); }));
        vp::EpiArgs ev;
        set_tattn_cap(ev, cap, NH);
        ev.ln_rs = ln_rs; ev.out = hb; ev.ldo = D; ev.resid = big;
        ev.bias = lw.bqkv + 2 * D; ev.ln_c = lw.cqkv + 2 * D;
        const bf16_t* wv = static_cast<const bf16_t*>(lw.wqkv) + (size_t)2 * D * D;
        VP_HIP(rec(PC_GEMM_QKV_TATTN, 2.0 * dM * dD * dD, gbytes(dD, dD, dE, 0) + dM * NH * 32.0, [&] {
          return gemm_bf16_w4(EPI_V_TATTN_LN, (const bf16_t*)xs, D, wv, D, M, D, D, ev, s); }));
      } else if (fold) {  // LN1 folded: A = the residual stream, (rstd, -mean*rstd) in ln_rs
        VP_HIP(rec(PC_GEMM_QKV, 2.0 * dM * dD * 3 * dD, gbytes(dD, 3 * dD, dE, 0), [&] {
          if (sblk) return gemm(EPI_BF16_LN_BLK, xs, D, lw.wqkv_blk, 3 * D, big, 3 * D, lw.bqkv_blk, nullptr, nullptr, 1,
                                nullptr, lw.cqkv_blk);
          return gemm(EPI_BF16_LN, xs, D, lw.wqkv, 3 * D, big, 3 * D, lw.bqkv, nullptr, nullptr, 1, nullptr,
                      lw.cqkv); }));
      } else {
        VP_HIP(rec(PC_LAYERNORM, 0.0, ln_bytes, [&] {
          return layernorm(xs, xbf, M, D, lw.ln1_g, lw.ln1_b, hb, bf, PERM_NONE, 1, 1, nullptr, s); }));
        VP_HIP(rec(PC_GEMM_QKV, 2.0 * dM * dD * 3 * dD, gbytes(dD, 3 * dD, dE, 0), [&] {
          return gemm(EPI_BF16, hb, D, lw.wqkv, 3 * D, big, 3 * D, lw.bqkv, nullptr, nullptr, 1, nullptr); }));
      }
      if (!tattn) VP_HIP(rec(acls, aflops, abytes, [&] {
        return launch_attention(kind, bf, big, hb, num_seq, S, NH, cap, pad, causal, sblk, s, D / NH); }));
      if (primer) {
        // the attention output is this GEMM's A, so its result goes to `big` (q|k|v are consumed); no paddings
        // on the attention sublayer (layers.py:846-855)
        VP_HIP(rec(PC_GEMM_POST, 2.0 * dM * dD * dD, gbytes(dD, dD, dE, 0), [&] {
          return gemm(EPI_BF16, hb, D, lw.wpost, D, big, D, lw.bpost, nullptr, nullptr, 1, nullptr); }));
        VP_HIP(rec(PC_LAYERNORM, 0.0, dM * dD * (dE + 8.0), [&] {
          return layernorm_residual(big, bf, M, D, lw.pn1_g, lw.pn1_b, nullptr, static_cast<float*>(xs), s); }));
      } else {
        VP_HIP(rec(PC_GEMM_POST, 2.0 * dM * dD * dD, gbytes(dD, dD, dE, dE), [&] {
          return gemm(fold ? EPI_RESID_BF16_ST : epi_resid, hb, D, lw.wpost, D, xs, D, lw.bpost, xs, nullptr, 1,
                      nullptr); }));
      }
      if (fold) {  // LN2 folded into ffn_layer1
        VP_HIP(finalize());
        VP_HIP(rec(PC_GEMM_FFN1, 2.0 * dM * dD * dF, gbytes(dD, dF, dE, 0), [&] {
          return gemm(lw.ffn_blk ? EPI_GELU_BF16_LN_BLK : EPI_GELU_BF16_LN, xs, D, lw.w1, F, big, F, lw.b1, nullptr,
                      nullptr, 1, pad, lw.c1); }));
      } else {
        VP_HIP(rec(PC_LAYERNORM, 0.0, ln_bytes, [&] {
          return layernorm(xs, xbf, M, D, lw.ln2_g, lw.ln2_b, hb, bf, PERM_NONE, 1, 1, nullptr, s); }));
        VP_HIP(rec(PC_GEMM_FFN1, 2.0 * dM * dD * dF, gbytes(dD, dF, dE, 0), [&] {
          return gemm(relu ? EPI_RELU_BF16 : EPI_GELU_BF16, hb, D, lw.w1, F, big, F, lw.b1, nullptr, nullptr, 1,
                      pad); }));
      }
      if (primer) {
        // ffn_layer2 into hb (ffn_layer1 has consumed the pre_layer_norm output there); the padding multiply
        // (layers.py:409-410) is layernorm_residual's, ahead of its LayerNorm
        VP_HIP(rec(PC_GEMM_FFN2, 2.0 * dM * dF * dD, gbytes(dF, dD, dE, 0), [&] {
          return gemm(EPI_BF16, big, F, lw.w2, D, hb, D, lw.b2, nullptr, nullptr, 1, nullptr); }));
        VP_HIP(rec(PC_LAYERNORM, 0.0, dM * dD * (dE + 8.0), [&] {
          return layernorm_residual(hb, bf, M, D, lw.pn2_g, lw.pn2_b, pad, static_cast<float*>(xs), s); }));
        continue;
      }
      const bool st = fold && !last;  // the next layer's LN1 statistics
      const int epi_ffn2 = lw.ffn_blk && fold ? (st ? EPI_RESID_FFN_BF16_ST_BLK : EPI_RESID_FFN_BF16_BLK)
                                              : st ? EPI_RESID_FFN_BF16_ST : epi_resid_ffn;
      VP_HIP(rec(PC_GEMM_FFN2, 2.0 * dM * dF * dD, gbytes(dF, dD, dE, dE), [&] {
        return gemm(epi_ffn2, big, F, lw.w2, D, xs, D, lw.b2, xs, nullptr, 1, pad); }));
      if (st) VP_HIP(finalize());
    }
    return VP_OK;
  }
};

}  // namespace vpi
