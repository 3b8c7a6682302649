// C-ABI of the LvT video-text model, FactorizedVideoCLIP (encoders.py:762-910), on top of the
// FactorizedEncoder handle (vp_abi.cpp) and the shared layer schedule (vp_internal.h).
//
//   video: vision encoder (vp_forward) -> auxiliary encoder (2 pre-LN layers over all T*N
//          tokens, attention_long_bf16) -> contrastive pooler (query folded into the key
//          projection, clip_kernels.hip) -> LayerNorm -> L2 normalise
//   text:  token embedding * sqrt(D) + sinusoidal positions, CLS appended -> 12 causal pre-LN
//          ReLU layers (attention_masked) -> unimodal_ln on the CLS row -> L2 normalise
//          (norm_policy 1, Giant: 16 'primer_hybrid' layers, a LayerNorm before and after each sublayer)
#include "vp_internal.h"

using namespace vpi;

namespace {
constexpr int kMaxTextLen = 1024;  // L + 1 (CLS) tokens; TEXT_MAX_LEN is 64 (models.py:53)
}

namespace vpi {

hipError_t pooler_stream(hipStream_t s, int bf, const PoolerW& pw, const void* feat, int G, int Sg, int D, int NH,
                         const PoolScratch& sc, const float* pad) {
  const hipError_t e = vp::pool_logits(feat, bf, (int64_t)G * Sg, Sg, D, pw.U, bf ? (const vp::bf16_t*)pw.Ut : nullptr,
                                       NH, sc.logits, s, pad);
  if (e != hipSuccess) return e;
  return vp::pool_softmax_wsum(feat, bf, G, Sg, D, NH, sc.logits, sc.stats, sc.zpart, sc.z, s, pad);
}

hipError_t pooler_project(hipStream_t s, const PoolerW& pw, int G, int D, int NH, const PoolScratch& sc, int do_l2,
                          float* dst) {
  using namespace vp;
  const int dp = pw.dp, K = NH * dp;
  hipError_t e = small_gemm(sc.z, (int64_t)NH * D, D, pw.WvT, (int64_t)D * dp, pw.bv, dp, sc.enc, K, dp, G, dp, D, NH, s);
  if (e != hipSuccess) return e;
  const int splits = NH >= 8 && K % (8 * 128) == 0 && (size_t)8 * G * D <= sc.zpart_floats ? 8 : 1;
  e = splits > 1 ? small_gemm_splitk(sc.enc, K, pw.WpT, pw.bp, sc.pooled, D, G, D, K, splits, sc.zpart, s)
                 : small_gemm(sc.enc, K, 0, pw.WpT, 0, pw.bp, 0, sc.pooled, D, 0, G, D, K, 1, s);
  if (e != hipSuccess) return e;
  return ln_l2_rows(sc.pooled, 0, D, G, D, pw.ln_g, pw.ln_b, do_l2, dst, s);
}

}  // namespace vpi

// What the two handles that wrap a FactorizedEncoder share: their own leaves (the ParamStore), the wrapped
// handle and the prefix its leaves carry.  The wrapped encoder's leaves come first in the enumeration.
struct WrapHandle : vpi::ParamStore {
  vp_handle* video = nullptr;
  PoolerW pool;         // the AttenTokenPoolingLayer over the encoder's features, packed (pack_pooler)
  int64_t pool_dp = 0;  // its dim_per_head, set by *_create (pool.dp only once packed)
  bool bf16() const { return video->bf16(); }
  virtual ~WrapHandle() = default;

  int init(const vp_config* cfg, int dev, const char* prefix) {
    device = dev;
    return create_encoder(cfg, dev, prefix, &video);
  }
  // every leaf set -> the encoder packed, this handle's device current: the caller packs its own leaves next
  int begin_finalize() {
    if (const std::string* n = first_missing()) return fail(VP_ESTATE, "missing parameter: " + *n);
    int rc = vp_finalize(video);
    if (rc) return rc;
    VP_HIP(hipSetDevice(device));
    return VP_OK;
  }
};

namespace {

int wrap_destroy(WrapHandle* w) {
  if (!w) return VP_OK;
  vp_destroy(w->video);
  w->free_all();
  delete w;
  return VP_OK;
}

// a leaf under the wrapped encoder's prefix is the encoder's
int wrap_set_param(WrapHandle* w, const char* name, const float* data, const int64_t* shape, int ndim) {
  if (!w) return fail(VP_EINVAL, "null argument");
  const std::string& px = w->video->prefix;
  const bool inner = name && !w->finalized && !std::strncmp(name, px.c_str(), px.size());
  return (inner ? static_cast<ParamStore*>(w->video) : w)->set(name, data, shape, ndim);
}

int wrap_param_count(const WrapHandle* w, int* count) {
  if (!w || !count) return fail(VP_EINVAL, "null argument");
  *count = (int)(w->video->names.size() + w->names.size());
  return VP_OK;
}

int wrap_param_name(const WrapHandle* w, int index, const char** name) {
  if (!w || !name || index < 0) return fail(VP_EINVAL, "bad index");
  const std::vector<std::string>&inner = w->video->names, &own = w->names;
  if (index >= (int)(inner.size() + own.size())) return fail(VP_EINVAL, "bad index");
  *name = (index < (int)inner.size() ? inner[index] : own[index - inner.size()]).c_str();
  return VP_OK;
}

int wrap_video_handle(WrapHandle* w, vp_handle** video) {
  if (!w || !video) return fail(VP_EINVAL, "null argument");
  *video = w->video;
  return VP_OK;
}

}  // namespace

struct vp_clip : WrapHandle {  // 'vision_encoder/' leaves in `video`
  vp_clip_config cfg;
  std::vector<vpi::LayerW> aux, text;  // `pool`: contrastive_vision_pooler (hidden 4D)
  // text tower: token table [V][D] (fprop dtype), cls [D], sinusoidal table [kMaxTextLen][D]
  void* tok = nullptr;
  float *cls = nullptr, *tpos = nullptr, *uln_g = nullptr, *uln_b = nullptr;
};

struct vp_classifier : WrapHandle {  // 'encoder/' leaves in `video`
  vp_config cfg;
  int num_classes = 0;                       // `pool`: atten_pooler (hidden D)
  float *wproj = nullptr, *bproj = nullptr;  // projection kernel [D][C] (= Wt of small_gemm), bias [C]
};

namespace {

struct ClipVideoWs {
  size_t inner_bytes = 0;  // the wrapped encoder's own workspace, at `inner`
  size_t inner = 0, feat = 0, total = 0;
  PoolWs pool;
};

// vision features + pooler scratch for G <= B*T groups; dp = the pooler's dim_per_head
ClipVideoWs pool_video_ws(const vp_config& v, int64_t B, int64_t T, int64_t H, int64_t W, size_t inner_bytes,
                          int64_t dp) {
  const int64_t P = v.patch_size, N = (H / P) * (W / P), M = B * T * N;
  const int64_t Mp = (M + 255) / 256 * 256;  // the auxiliary encoder's GEMM rows (clip_video_chunk)
  const int64_t D = v.model_dim, NH = v.num_heads;
  const size_t es = v.fprop_dtype == VP_BF16 ? 2 : 4;
  const int64_t gc = std::max<int64_t>(B * vp::pool_chunks((int)(T * N)), B * T * vp::pool_chunks((int)N));
  ClipVideoWs L;
  L.inner_bytes = inner_bytes;
  size_t off = 0;
  L.inner = off; off = align256(off + inner_bytes);
  L.feat = off; off = align256(off + (size_t)Mp * D * es);
  L.pool = carve_pool_ws(off, M, B * T, D, NH, dp, (size_t)gc * NH * D);
  L.total = off;
  return L;
}

// the layout for a forward over B clips: that of its (largest) chunk
int pool_video_ws(const WrapHandle* w, int64_t B, int64_t T, int64_t H, int64_t W, ClipVideoWs* L) {
  size_t inner = 0;
  int rc = vp_workspace_bytes(w->video, B, T, H, W, &inner);
  if (rc) return rc;
  *L = pool_video_ws(w->video->cfg, chunk_of(w->video, B, T, H, W), T, H, W, inner, w->pool_dp);
  return VP_OK;
}

struct ClipTextWs {
  size_t x = 0, hb = 0, big = 0, pad = 0, total = 0;
  int64_t Mt = 0;
  bool small = false;  // bf16 GEMMs on the small-M kernel (64-row tiles)
};

ClipTextWs clip_text_ws(const vp_clip* c, int64_t Q, int64_t L) {
  const int64_t D = c->cfg.video.model_dim;
  const size_t es = c->bf16() ? 2 : 4;
  ClipTextWs w;
  // up to 4096 rows (63 queries) the bf16 GEMMs take the small-M kernel, whose tiles are 64 rows; the
  // 256 x 256-tile kernels would leave at least three quarters of the CUs idle
  w.small = c->bf16() && Q * (L + 1) <= 4096 && D % 256 == 0;
  const int64_t rt = w.small ? 64 : 256;
  w.Mt = (Q * (L + 1) + rt - 1) / rt * rt;
  size_t off = 0;
  w.x = off; off = align256(off + (size_t)w.Mt * D * 4);  // fp32 residual stream
  w.hb = off; off = align256(off + (size_t)w.Mt * D * es);
  w.big = off; off = align256(off + (size_t)w.Mt * 4 * D * es);
  w.pad = off; off = align256(off + (size_t)w.Mt * 4);
  w.total = off;
  return w;
}

// the 12 leaves of an AttenTokenPoolingLayer (layers.py:1044-1136, layers_test.py:283)
void add_pooler_expected(ParamStore& c, const std::string& pre, int64_t D, int64_t NH, int64_t dp) {
  c.expect(pre + "pooling_attention_query", {1, D});
  c.expect(pre + "pooling_attention/per_dim_scale/per_dim_scale", {dp});
  for (const char* q : {"query", "key", "value"}) {
    c.expect(pre + "pooling_attention/" + q + "/w", {D, NH, dp});
    c.expect(pre + "pooling_attention/" + q + "/b", {NH, dp});
  }
  c.expect(pre + "pooling_attention/post/w", {D, NH, dp});
  c.expect(pre + "pooling_attention/post/b", {D});
  c.expect(pre + "pooling_attention_layer_norm/scale", {D});
  c.expect(pre + "pooling_attention_layer_norm/bias", {D});
}

void build_clip_expected(vp_clip& c) {
  const vp_clip_config& cc = c.cfg;
  const int64_t D = cc.video.model_dim, NH = cc.video.num_heads;
  if (cc.num_auxiliary_layers > 0)
    add_stack_expected(c, "auxiliary_encoder/transformers_stack/x_layers/", cc.num_auxiliary_layers, D,
                       cc.video.mlp_dim, NH);
  add_pooler_expected(c, "contrastive_vision_pooler/", D, NH, c.pool_dp);
  c.expect("text_encoder/token_emb/emb_var", {(int64_t)cc.vocabulary_size, D});
  c.expect("text_encoder/cls_emb", {1, 1, D});
  add_stack_expected(c, "text_encoder/unimodal_transformer/x_layers/", cc.num_unimodal_layers, D, 4 * D, NH,
                     cc.norm_policy == 1);
  c.expect("text_encoder/unimodal_ln/scale", {D});
  c.expect("text_encoder/unimodal_ln/bias", {D});
}

// bf16 hi/lo split of U [H][D] for the MFMA logits kernel: ut [32][D] = (U_hi | U_lo | 0), U_hi the bf16 of
// U and U_lo the bf16 of U - U_hi (pack_pooler, and vp_dev_pool_split_u for the tests)
void pool_split_u(const float* U, int64_t H, int64_t D, uint16_t* ut) {
  std::fill(ut, ut + (size_t)32 * D, (uint16_t)0);
  for (int64_t h = 0; h < H; ++h)
    for (int64_t d = 0; d < D; ++d) {
      const float u = U[(size_t)h * D + d];
      const uint16_t hi = host_f2bf(u);
      uint32_t hb = (uint32_t)hi << 16;
      float hf;
      std::memcpy(&hf, &hb, 4);
      ut[(size_t)h * D + d] = hi;
      ut[(size_t)(H + h) * D + d] = host_f2bf(u - hf);
    }
}

// AttenTokenPoolingLayer (layers.py:1044-1136) with the query folded into the key projection
// (see clip_kernels.hip): host packing in fp64.
int pack_pooler(ParamStore& c, const std::string& root, int64_t D, int64_t H, int64_t dp, PoolerW& pw) {
  const std::string pre = root + "pooling_attention/";
  pw.dp = (int)dp;
  const auto& query = c.data(root + "pooling_attention_query");
  const auto& wq = c.data(pre + "query/w");
  const auto& bq = c.data(pre + "query/b");
  const auto& wk = c.data(pre + "key/w");
  const auto& wv = c.data(pre + "value/w");
  const auto& bv = c.data(pre + "value/b");
  const auto& wp = c.data(pre + "post/w");
  const auto& bp = c.data(pre + "post/b");
  const auto& pds = c.data(pre + "per_dim_scale/per_dim_scale");
  // q~[h][j] = (query . Wq[:, h, j] + bq[h][j]) * 1.442695041/sqrt(dp) * softplus(pds[j])  (:502-527)
  std::vector<double> qt((size_t)H * dp);
  const double r_softplus_0 = 1.442695041 / std::sqrt((double)dp);
  for (int64_t h = 0; h < H; ++h)
    for (int64_t j = 0; j < dp; ++j) {
      double a = bq[(size_t)h * dp + j];
      for (int64_t d = 0; d < D; ++d) a += (double)query[d] * wq[((size_t)d * H + h) * dp + j];
      const double x = pds[j];
      const double sp = x > 30.0 ? x : std::log1p(std::exp(x));
      qt[(size_t)h * dp + j] = a * r_softplus_0 * sp;
    }
  std::vector<float> U((size_t)H * D), wvt((size_t)H * D * dp), wpt((size_t)H * dp * D);
  for (int64_t h = 0; h < H; ++h)
    for (int64_t d = 0; d < D; ++d) {
      double a = 0.0;
      for (int64_t j = 0; j < dp; ++j) a += (double)wk[((size_t)d * H + h) * dp + j] * qt[(size_t)h * dp + j];
      U[(size_t)h * D + d] = (float)a;
      for (int64_t j = 0; j < dp; ++j) wvt[((size_t)h * D + d) * dp + j] = wv[((size_t)d * H + h) * dp + j];
    }
  for (int64_t n = 0; n < D; ++n)
    for (int64_t k = 0; k < H * dp; ++k) wpt[(size_t)k * D + n] = wp[(size_t)n * H * dp + k];
  std::vector<float> g(D);
  const auto& sc = c.data(root + "pooling_attention_layer_norm/scale");
  for (int64_t d = 0; d < D; ++d) g[d] = sc[d] + 1.0f;
  std::vector<uint16_t> ut((size_t)32 * D);
  pool_split_u(U.data(), H, D, ut.data());
  int rc;
  void* utd = nullptr;
  if ((rc = c.upload(ut.data(), ut.size() * 2, &utd))) return rc;
  pw.Ut = utd;
  auto up = [&](const std::vector<float>& v, const float** out) {
    float* p = nullptr;
    const int r = c.upload_f32(v, &p);
    *out = p;
    return r;
  };
  if ((rc = up(U, &pw.U)) || (rc = up(wvt, &pw.WvT)) || (rc = up(bv, &pw.bv)) || (rc = up(wpt, &pw.WpT)) ||
      (rc = up(bp, &pw.bp)) || (rc = up(g, &pw.ln_g)) ||
      (rc = up(c.data(root + "pooling_attention_layer_norm/bias"), &pw.ln_b)))
    return rc;
  return VP_OK;
}

// pooler over G groups of Sg rows of feat [G*Sg][D] -> dst [G][D] fp32 (LayerNorm, then L2 if do_l2)
int run_pooler(Fwd& f, const PoolerW& pw, const void* feat, int M, int G, int Sg, int D, int NH,
               const PoolScratch& sc, int do_l2, float* dst) {
  const int dp = pw.dp;
  const double bytes = 2.0 * M * D * (f.bf ? 2 : 4);  // two streaming passes over the tokens
  VP_HIP(f.rec(PC_POOL, 2.0 * 2.0 * M * D * NH, bytes,
               [&] { return pooler_stream(f.s, f.bf, pw, feat, G, Sg, D, NH, sc); }));
  VP_HIP(f.rec(PC_POOL, 2.0 * G * D * (double)dp * NH * 2.0, 4.0 * (double)NH * D * dp * 2.0,
               [&] { return pooler_project(f.s, pw, G, D, NH, sc, do_l2, dst); }));
  return VP_OK;
}

// What clip_video_chunk and classifier_chunk start with, over one chunk of B <= chunk_clips clips: the wrapped
// encoder's features [B, T*N, D] in the fprop dtype (encoders.py:833-845, :621-630) land in the pooler
// workspace, a copy goes to spatiotemporal_out if asked, and the pooler's scratch is carved out.
struct VisionFeat {
  ClipVideoWs L;
  void* feat = nullptr;
  int M = 0;  // B*T*N tokens
  PoolScratch sc;
};

// Where vision_features takes its B clips from: frames [B, T, H, W, 3] (vp_forward), or, with states set, B windows
// of T frames picked by frame_idx [B, T] out of the encoder's F frame states (vp_forward_temporal)
struct VideoSrc {
  const void* video = nullptr;
  int in_dtype = VP_F32;
  const void* states = nullptr;
  int64_t F = 0;
  const int32_t* frame_idx = nullptr;

  // the source of the clips from b0 on
  VideoSrc from(int64_t b0, int64_t T, size_t clip_bytes) const {
    VideoSrc s = *this;
    s.video = advance(video, b0 * clip_bytes);
    s.frame_idx = frame_idx ? frame_idx + b0 * T : nullptr;
    return s;
  }
};

int vision_features(WrapHandle* w, const VideoSrc& src, int64_t B, int64_t T, int64_t H, int64_t W,
                    const float* frame_paddings, void* spatial_out, void* spatiotemporal_out, void* workspace,
                    void* stream, VisionFeat* vf) {
  ClipVideoWs& L = vf->L;
  int rc = pool_video_ws(w, B, T, H, W, &L);
  if (rc) return rc;
  const vp_config& v = w->video->cfg;
  const int64_t N = (H / v.patch_size) * (W / v.patch_size), M64 = B * T * N;
  if (M64 > 0x7fffffff) return fail(VP_ENOTSUP, "too many tokens");
  vf->M = (int)M64;
  char* ws = static_cast<char*>(workspace);
  vf->feat = ws + L.feat;
  rc = src.states ? vp_forward_temporal(w->video, src.states, src.F, src.frame_idx, B, T, H, W, frame_paddings, vf->feat,
                                        v.fprop_dtype, spatial_out, ws + L.inner, L.inner_bytes, stream)
                  : vp_forward(w->video, src.video, src.in_dtype, B, T, H, W, frame_paddings, vf->feat, v.fprop_dtype,
                               spatial_out, ws + L.inner, L.inner_bytes, stream);
  if (rc) return rc;
  VP_HIP(hipSetDevice(w->device));
  if (spatiotemporal_out)
    VP_HIP(hipMemcpyAsync(spatiotemporal_out, vf->feat, (size_t)M64 * v.model_dim * dtype_bytes(v.fprop_dtype),
                          hipMemcpyDeviceToDevice, static_cast<hipStream_t>(stream)));
  vf->sc = L.pool.at(ws);
  return VP_OK;
}

int pack_text(vp_clip* c) {
  const int64_t D = c->cfg.video.model_dim;
  int rc;
  if ((rc = c->upload_mat(c->data("text_encoder/token_emb/emb_var"), c->bf16(), &c->tok))) return rc;
  if ((rc = c->upload_f32(c->data("text_encoder/cls_emb"), &c->cls))) return rc;
  // PositionalEmbedding (encoders.py:190-224): [sin(t * inv) | cos(t * inv)], zero column for odd D
  std::vector<float> pos((size_t)kMaxTextLen * D, 0.0f);
  const int64_t nts = D / 2;
  const double inc = std::log(10000.0) / std::max<double>((double)nts - 1.0, 1.0);
  for (int t = 0; t < kMaxTextLen; ++t)
    for (int64_t i = 0; i < nts; ++i) {
      const double st = t * std::exp(-(double)i * inc);
      pos[(size_t)t * D + i] = (float)std::sin(st);
      pos[(size_t)t * D + nts + i] = (float)std::cos(st);
    }
  if ((rc = c->upload_f32(pos, &c->tpos))) return rc;
  std::vector<float> g(D);
  const auto& sc = c->data("text_encoder/unimodal_ln/scale");
  for (int64_t d = 0; d < D; ++d) g[d] = sc[d] + 1.0f;
  if ((rc = c->upload_f32(g, &c->uln_g)) || (rc = c->upload_f32(c->data("text_encoder/unimodal_ln/bias"), &c->uln_b)))
    return rc;
  const int NH = c->cfg.video.num_heads;
  return pack_stack(*c, c->bf16(), "text_encoder/unimodal_transformer/x_layers/", c->cfg.num_unimodal_layers, D, 4 * D, NH,
                    false, c->text, QKV_PLAIN, c->cfg.norm_policy == 1);
}

}  // namespace

extern "C" {

int vp_clip_create(const vp_clip_config* cfg, int device, vp_clip** out) {
  if (!cfg || !out) return fail(VP_EINVAL, "null argument");
  *out = nullptr;
  if (cfg->num_auxiliary_layers < 0 || cfg->num_unimodal_layers < 0 || cfg->vocabulary_size < 1)
    return fail(VP_EINVAL, "bad LvT configuration");
  if (int rc = check_pooler_heads(cfg->video.num_heads)) return rc;
  if (cfg->norm_policy != 0 && cfg->norm_policy != 1)
    return fail(VP_ENOTSUP, "norm_policy must be 0 ('pre') or 1 ('primer_hybrid', the text tower's)");
  vp_clip* c = new vp_clip();
  int rc = c->init(&cfg->video, device, "vision_encoder/");
  // after the encoder's own refusals (dim_per_head, bf16 widths)
  if (!rc) rc = check_pooler_dims(cfg->video.model_dim, cfg->video.num_heads);
  if (rc) {
    wrap_destroy(c);
    return rc;
  }
  c->cfg = *cfg;
  c->pool_dp = 4 * cfg->video.model_dim / cfg->video.num_heads;
  build_clip_expected(*c);
  *out = c;
  return VP_OK;
}

int vp_clip_destroy(vp_clip* c) { return wrap_destroy(c); }
int vp_clip_set_param(vp_clip* c, const char* name, const float* host_data, const int64_t* shape, int ndim) {
  return wrap_set_param(c, name, host_data, shape, ndim);
}
int vp_clip_param_count(const vp_clip* c, int* count) { return wrap_param_count(c, count); }
int vp_clip_param_name(const vp_clip* c, int index, const char** name) { return wrap_param_name(c, index, name); }
int vp_clip_video_handle(vp_clip* c, vp_handle** video) { return wrap_video_handle(c, video); }

int vp_clip_finalize(vp_clip* c) {
  if (!c) return fail(VP_EINVAL, "null handle");
  if (c->finalized) return VP_OK;
  int rc = c->begin_finalize();
  if (rc) return rc;
  const vp_config& v = c->cfg.video;
  if (c->cfg.num_auxiliary_layers > 0 &&
      (rc = pack_stack(*c, c->bf16(), "auxiliary_encoder/transformers_stack/x_layers/", c->cfg.num_auxiliary_layers,
                       v.model_dim, v.mlp_dim, v.num_heads, c->bf16(), c->aux)))
    return rc;
  if ((rc = pack_pooler(*c, "contrastive_vision_pooler/", v.model_dim, v.num_heads, c->pool_dp, c->pool)) ||
      (rc = pack_text(c)))
    return rc;
  c->seal();
  return VP_OK;
}

int vp_clip_video_workspace_bytes(const vp_clip* c, int64_t B, int64_t T, int64_t H, int64_t W, size_t* bytes) {
  if (!c || !bytes) return fail(VP_EINVAL, "null argument");
  ClipVideoWs L;
  int rc = pool_video_ws(c, B, T, H, W, &L);
  if (rc) return rc;
  *bytes = L.total;
  return VP_OK;
}

}  // extern "C"

namespace {

// video side of FactorizedVideoCLIP over one chunk of B <= chunk_clips clips
int clip_video_chunk(vp_clip* c, const VideoSrc& src, int64_t B, int64_t T, int64_t H, int64_t W,
                     const float* frame_paddings, int normalize, float* video_emb, float* frame_emb,
                     void* spatial_out, void* spatiotemporal_out, void* workspace, void* stream) {
  using namespace vp;
  // 1. vision encoder -> vision_features [B, T*N, D] (encoders.py:833-845)
  VisionFeat vf;
  int rc = vision_features(c, src, B, T, H, W, frame_paddings, spatial_out, spatiotemporal_out, workspace, stream, &vf);
  if (rc) return rc;
  const bool bf = c->bf16();
  const vp_config& v = c->cfg.video;
  const int D = v.model_dim, NH = v.num_heads, M = vf.M;
  const int N = (int)(M / (B * T)), S = (int)T * N;
  void* feat = vf.feat;
  // the auxiliary encoder's GEMM rows: B*T*N padded to the tile (as the vision encoder's, vp_internal.h
  // padded_rows); the padding rows of feat are zeroed, ride through the row-independent GEMM / LayerNorm
  // kernels and are never attended to or pooled (every sequence and pooling group is a block of M rows)
  const int Mp = (int)padded_rows(c->video, M);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const size_t es = bf ? 2 : 4;
  // the vision encoder's scratch regions are free again (stream order): reuse them
  const WsLayout Lv = ws_layout(c->video, B, T, H, W);
  char* wsv = static_cast<char*>(workspace) + vf.L.inner;
  Fwd f;
  f.s = s; f.bf = bf; f.M = Mp; f.D = D; f.NH = NH; f.cap = v.atten_logit_cap;
  f.f32_two_chains = f32_two_chains(v);
  f.hb = wsv + Lv.hbuf; f.big = wsv + Lv.big;
  f.st_part = reinterpret_cast<float*>(wsv + Lv.st_part);
  f.ln_rs = reinterpret_cast<float*>(wsv + Lv.ln_rs);
  f.pf = &c->video->prof;
  // 2. auxiliary encoder over all T*N tokens of each clip (encoders.py:846-857; paddings None)
  if (c->cfg.num_auxiliary_layers > 0) {
    if (Mp > M) VP_HIP(hipMemsetAsync(static_cast<char*>(feat) + (size_t)M * D * es, 0, (size_t)(Mp - M) * D * es, s));
    if (bf)
      VP_HIP(f.rec(PC_LAYERNORM, 0.0, (double)M * D * 2, [&] {
        return ln_row_stats((const bf16_t*)feat, Mp, D, f.ln_rs, s); }));
    rc = f.run_stack(c->aux, feat, (int)B, S, nullptr, v.mlp_dim, PC_ATTN_AUX, ATT_LONG, bf, false);
    if (rc) return rc;
  }
  // 3. contrastive pooler + L2 (encoders.py:859-872), and per frame (:874-885)
  auto pool = [&](int G, int Sg, float* dst) -> int {
    return run_pooler(f, c->pool, feat, M, G, Sg, D, NH, vf.sc, normalize, dst);
  };
  if ((rc = pool((int)B, S, video_emb))) return rc;
  if (frame_emb && (rc = pool((int)(B * T), N, frame_emb))) return rc;
  return VP_OK;
}

// vp_clip_encode_video / vp_clip_encode_video_windows over the B clips of `src`
int clip_encode(vp_clip* c, const VideoSrc& src, int64_t B, int64_t T, int64_t H, int64_t W, const float* frame_paddings,
                int normalize, float* video_emb, float* frame_emb, void* spatial_out, void* spatiotemporal_out,
                int out_dtype, void* workspace, size_t ws_bytes, void* stream) {
  if (!c->finalized) return fail(VP_ESTATE, "vp_clip_finalize has not been called");
  size_t need = 0, st_clip = 0;
  int rc = check_dtypes(src.in_dtype, out_dtype, spatiotemporal_out != nullptr, c->video->cfg.fprop_dtype);
  if (rc || (rc = vp_clip_video_workspace_bytes(c, B, T, H, W, &need)) ||
      (rc = check_workspace(c->video, T, H, W, ws_bytes, need, c->video->cfg.fprop_dtype, &st_clip)))
    return rc;
  const size_t in_clip = video_clip_bytes(T, H, W, src.in_dtype);
  const int64_t D = c->cfg.video.model_dim;
  return for_each_chunk(c->video, B, T, H, W, [&](int64_t b0, int64_t nb) {
    return clip_video_chunk(c, src.from(b0, T, in_clip), nb, T, H, W, advance(frame_paddings, b0 * T * 4),
                            normalize, video_emb + b0 * D, advance(frame_emb, b0 * T * D * 4),
                            advance(spatial_out, b0 * st_clip), advance(spatiotemporal_out, b0 * st_clip), workspace,
                            stream);
  });
}

}  // namespace

extern "C" {

int vp_clip_encode_video(vp_clip* c, const void* video, int in_dtype, int64_t B, int64_t T, int64_t H, int64_t W,
                         const float* frame_paddings, int normalize, float* video_emb, float* frame_emb,
                         void* spatial_out, void* spatiotemporal_out, int out_dtype, void* workspace,
                         size_t ws_bytes, void* stream) {
  if (!c || !video || !video_emb || !workspace) return fail(VP_EINVAL, "null argument");
  VideoSrc src;
  src.video = video;
  src.in_dtype = in_dtype;
  return clip_encode(c, src, B, T, H, W, frame_paddings, normalize, video_emb, frame_emb, spatial_out,
                     spatiotemporal_out, out_dtype, workspace, ws_bytes, stream);
}

int vp_clip_video_windows_workspace_bytes(const vp_clip* c, int64_t Wn, int64_t T, int64_t H, int64_t W,
                                          size_t* bytes) {
  return vp_clip_video_workspace_bytes(c, Wn, T, H, W, bytes);
}

int vp_clip_encode_video_windows(vp_clip* c, const void* states, int64_t F, const int32_t* frame_idx, int64_t Wn,
                                 int64_t T, int64_t H, int64_t W, const float* frame_paddings, int normalize,
                                 float* video_emb, float* frame_emb, void* spatial_out, void* spatiotemporal_out,
                                 int out_dtype, void* workspace, size_t ws_bytes, void* stream) {
  if (!c || !states || !frame_idx || !video_emb || !workspace) return fail(VP_EINVAL, "null argument");
  VideoSrc src;
  src.in_dtype = c->video->cfg.fprop_dtype;
  src.states = states;
  src.F = F;
  src.frame_idx = frame_idx;
  return clip_encode(c, src, Wn, T, H, W, frame_paddings, normalize, video_emb, frame_emb, spatial_out,
                     spatiotemporal_out, out_dtype, workspace, ws_bytes, stream);
}

int vp_clip_text_workspace_bytes(const vp_clip* c, int64_t Q, int64_t L, size_t* bytes) {
  if (!c || !bytes) return fail(VP_EINVAL, "null argument");
  if (Q < 1 || L < 1 || L + 1 > kMaxTextLen) return fail(VP_EINVAL, "text ids must be [Q, L] with 1 <= L < 1024");
  *bytes = clip_text_ws(c, Q, L).total;
  return VP_OK;
}

int vp_clip_encode_text(vp_clip* c, const int32_t* ids, const float* paddings, int64_t Q, int64_t L, int normalize,
                        float* text_emb, void* workspace, size_t ws_bytes, void* stream) {
  using namespace vp;
  if (!c || !ids || !paddings || !text_emb || !workspace) return fail(VP_EINVAL, "null argument");
  if (!c->finalized) return fail(VP_ESTATE, "vp_clip_finalize has not been called");
  if (Q < 1 || L < 1 || L + 1 > kMaxTextLen) return fail(VP_EINVAL, "text ids must be [Q, L] with 1 <= L < 1024");
  const ClipTextWs w = clip_text_ws(c, Q, L);
  if (ws_bytes < w.total) return fail(VP_EINVAL, "workspace too small: need " + std::to_string(w.total));
  if (w.Mt > 0x7fffffff) return fail(VP_ENOTSUP, "too many text tokens");
  VP_HIP(hipSetDevice(c->device));
  hipStream_t s = static_cast<hipStream_t>(stream);
  const bool bf = c->bf16();
  const vp_config& v = c->cfg.video;
  const int D = v.model_dim;
  char* ws = static_cast<char*>(workspace);
  void* x = ws + w.x;
  float* pad = reinterpret_cast<float*>(ws + w.pad);
  // The text tower keeps its residual stream in fp32 in both modes (bf16 GEMM operands, fp32
  // sums): its Q*(L+1) rows cost nothing, and it removes the stream's per-layer bf16 rounding.
  // Rows past Q*(L+1) only pad the GEMMs' M to a tile multiple: keep them finite.
  VP_HIP(hipMemsetAsync(x, 0, (size_t)w.Mt * D * 4, s));
  VP_HIP(hipMemsetAsync(pad, 0, (size_t)w.Mt * 4, s));
  VP_HIP(text_embed(ids, (int)Q, (int)L, c->tok, bf, c->cfg.vocabulary_size, c->cls, c->tpos, std::sqrt((float)D), D,
                    x, 0, paddings, pad, s));
  Fwd f;
  f.s = s; f.bf = bf; f.M = (int)w.Mt; f.D = D; f.NH = v.num_heads; f.cap = v.atten_logit_cap;
  f.causal = c->cfg.enable_causal_atten ? 1 : 0;
  f.xs_f32 = true;
  f.f32_two_chains = f32_two_chains(v);
  f.small_m = w.small;
  f.hb = ws + w.hb; f.big = ws + w.big;
  f.pf = &c->video->prof;
  f.cls_all = PC_ATTN_TEXT;  // the whole text tower in one profiler class ("text_tower"), so the vision GEMM
                             // classes (and bench.py's dominant-kernel roofline) hold the vision launches only
  int rc = f.run_stack(c->text, x, (int)Q, (int)L + 1, pad, 4 * D, PC_ATTN_TEXT, ATT_TEXT, false, true,
                       c->cfg.norm_policy == 1);
  if (rc) return rc;
  // unimodal_ln on the CLS rows, then L2 (encoders.py:752-758, :905-908)
  VP_HIP(ln_l2_rows(static_cast<float*>(x) + (size_t)L * D, 0, (int64_t)(L + 1) * D, (int)Q, D, c->uln_g,
                    c->uln_b, normalize, text_emb, s));
  return VP_OK;
}

}  // extern "C"

// ------------------------------------------------------------------------------------------
// FactorizedVideoClassifier (encoders.py:583-653): encoder -> AttenTokenPoolingLayer(hidden D,
// dim_per_head D/heads, paddings None) -> Dense(num_classes)
// ------------------------------------------------------------------------------------------
extern "C" {

int vp_classifier_create(const vp_config* cfg, int num_classes, int device, vp_classifier** out) {
  if (!cfg || !out) return fail(VP_EINVAL, "null argument");
  *out = nullptr;
  if (num_classes < 1) return fail(VP_EINVAL, "num_classes must be positive");
  if (int rc = check_pooler_heads(cfg->num_heads)) return rc;
  vp_classifier* c = new vp_classifier();
  int rc = c->init(cfg, device, "encoder/");
  if (!rc) rc = check_pooler_dims(cfg->model_dim, cfg->num_heads);
  if (rc) {
    wrap_destroy(c);
    return rc;
  }
  c->cfg = *cfg;
  c->num_classes = num_classes;
  const int64_t D = cfg->model_dim, NH = cfg->num_heads;
  c->pool_dp = D / NH;
  add_pooler_expected(*c, "atten_pooler/", D, NH, c->pool_dp);
  c->expect("projection/linear/kernel", {D, (int64_t)num_classes});
  c->expect("projection/linear/bias", {(int64_t)num_classes});
  *out = c;
  return VP_OK;
}

int vp_classifier_destroy(vp_classifier* c) { return wrap_destroy(c); }
int vp_classifier_set_param(vp_classifier* c, const char* name, const float* host_data, const int64_t* shape,
                            int ndim) {
  return wrap_set_param(c, name, host_data, shape, ndim);
}
int vp_classifier_param_count(const vp_classifier* c, int* count) { return wrap_param_count(c, count); }
int vp_classifier_param_name(const vp_classifier* c, int index, const char** name) {
  return wrap_param_name(c, index, name);
}
int vp_classifier_video_handle(vp_classifier* c, vp_handle** video) { return wrap_video_handle(c, video); }

int vp_classifier_finalize(vp_classifier* c) {
  if (!c) return fail(VP_EINVAL, "null handle");
  if (c->finalized) return VP_OK;
  int rc = c->begin_finalize();
  if (rc) return rc;
  const int64_t D = c->cfg.model_dim, NH = c->cfg.num_heads;
  if ((rc = pack_pooler(*c, "atten_pooler/", D, NH, c->pool_dp, c->pool)) ||
      (rc = c->upload_f32(c->data("projection/linear/kernel"), &c->wproj)) ||
      (rc = c->upload_f32(c->data("projection/linear/bias"), &c->bproj)))
    return rc;
  c->seal();
  return VP_OK;
}

int vp_classifier_workspace_bytes(const vp_classifier* c, int64_t B, int64_t T, int64_t H, int64_t W,
                                  size_t* bytes) {
  if (!c || !bytes) return fail(VP_EINVAL, "null argument");
  ClipVideoWs L;
  int rc = pool_video_ws(c, B, T, H, W, &L);
  if (rc) return rc;
  // + the pooled embeddings of one chunk, when the caller does not ask for them
  *bytes = L.total + align256((size_t)chunk_of(c->video, B, T, H, W) * c->cfg.model_dim * 4);
  return VP_OK;
}

}  // extern "C"

namespace {

// FactorizedVideoClassifier over one chunk of B <= chunk_clips clips
int classifier_chunk(vp_classifier* c, const VideoSrc& src, int64_t B, int64_t T, int64_t H,
                     int64_t W, const float* frame_paddings, float* logits, float* embeddings,
                     void* spatial_out, void* spatiotemporal_out, void* workspace, void* stream) {
  using namespace vp;
  // 1. encoder -> features [B, T*N, D] (encoders.py:621-630)
  VisionFeat vf;
  int rc = vision_features(c, src, B, T, H, W, frame_paddings, spatial_out, spatiotemporal_out, workspace, stream, &vf);
  if (rc) return rc;
  const vp_config& v = c->cfg;
  const int D = v.model_dim, NH = v.num_heads, M = vf.M;
  hipStream_t s = static_cast<hipStream_t>(stream);
  Fwd f;
  f.s = s; f.bf = c->bf16(); f.M = M; f.D = D; f.NH = NH; f.cap = v.atten_logit_cap;
  f.pf = &c->video->prof;
  // 2. atten_pooler over all T*N tokens, paddings None (:634-641); 3. projection (:646-652)
  float* emb = embeddings ? embeddings : reinterpret_cast<float*>(static_cast<char*>(workspace) + vf.L.total);
  if ((rc = run_pooler(f, c->pool, vf.feat, M, (int)B, (int)(M / B), D, NH, vf.sc, 0, emb))) return rc;
  VP_HIP(small_gemm(emb, D, 0, c->wproj, 0, c->bproj, 0, logits, c->num_classes, 0, (int)B, c->num_classes, D, 1, s));
  return VP_OK;
}

// vp_classifier_forward / vp_classifier_forward_windows over the B clips of `src`
int classifier_run(vp_classifier* c, const VideoSrc& src, int64_t B, int64_t T, int64_t H, int64_t W,
                   const float* frame_paddings, float* logits, float* embeddings, void* spatial_out,
                   void* spatiotemporal_out, int out_dtype, void* workspace, size_t ws_bytes, void* stream) {
  if (!c->finalized) return fail(VP_ESTATE, "vp_classifier_finalize has not been called");
  size_t need = 0, st_clip = 0;
  int rc = check_dtypes(src.in_dtype, out_dtype, spatiotemporal_out != nullptr, c->cfg.fprop_dtype);
  if (rc || (rc = vp_classifier_workspace_bytes(c, B, T, H, W, &need)) ||
      (rc = check_workspace(c->video, T, H, W, ws_bytes, need, c->video->cfg.fprop_dtype, &st_clip)))
    return rc;
  const size_t in_clip = video_clip_bytes(T, H, W, src.in_dtype);
  const int64_t D = c->cfg.model_dim;
  return for_each_chunk(c->video, B, T, H, W, [&](int64_t b0, int64_t nb) {
    return classifier_chunk(c, src.from(b0, T, in_clip), nb, T, H, W, advance(frame_paddings, b0 * T * 4),
                            logits + b0 * c->num_classes, advance(embeddings, b0 * D * 4),
                            advance(spatial_out, b0 * st_clip), advance(spatiotemporal_out, b0 * st_clip), workspace,
                            stream);
  });
}

}  // namespace

extern "C" {

int vp_classifier_forward(vp_classifier* c, const void* video, int in_dtype, int64_t B, int64_t T, int64_t H,
                          int64_t W, const float* frame_paddings, float* logits, float* embeddings,
                          void* spatial_out, void* spatiotemporal_out, int out_dtype, void* workspace,
                          size_t ws_bytes, void* stream) {
  if (!c || !video || !logits || !workspace) return fail(VP_EINVAL, "null argument");
  VideoSrc src;
  src.video = video;
  src.in_dtype = in_dtype;
  return classifier_run(c, src, B, T, H, W, frame_paddings, logits, embeddings, spatial_out, spatiotemporal_out,
                        out_dtype, workspace, ws_bytes, stream);
}

int vp_classifier_windows_workspace_bytes(const vp_classifier* c, int64_t Wn, int64_t T, int64_t H, int64_t W,
                                          size_t* bytes) {
  return vp_classifier_workspace_bytes(c, Wn, T, H, W, bytes);
}

int vp_classifier_forward_windows(vp_classifier* c, const void* states, int64_t F, const int32_t* frame_idx,
                                  int64_t Wn, int64_t T, int64_t H, int64_t W, const float* frame_paddings,
                                  float* logits, float* embeddings, void* spatial_out, void* spatiotemporal_out,
                                  int out_dtype, void* workspace, size_t ws_bytes, void* stream) {
  if (!c || !states || !frame_idx || !logits || !workspace) return fail(VP_EINVAL, "null argument");
  VideoSrc src;
  src.in_dtype = c->video->cfg.fprop_dtype;
  src.states = states;
  src.F = F;
  src.frame_idx = frame_idx;
  return classifier_run(c, src, Wn, T, H, W, frame_paddings, logits, embeddings, spatial_out, spatiotemporal_out,
                        out_dtype, workspace, ws_bytes, stream);
}

}  // extern "C"

// ------------------------------------------------------------------------------------------
// Not in the public header: the pooler, small GEMM and text kernels of clip_kernels.hip one at a time, and
// run_pooler on caller-supplied tokens, for the op-level fp64 parity tests (tests/test_gpu_clip_kernels.py,
// tests/test_pool_split_cpu.py).  Every shape a launcher would refuse is refused here first, with a message.
// ------------------------------------------------------------------------------------------
namespace {

bool float_dtype(int dtype) { return dtype == VP_F32 || dtype == VP_BF16; }

}  // namespace

extern "C" {

// Host only, no GPU call: the production packing of U [H][D] fp32 into ut [32][D] bf16 bits (pool_split_u).
int vp_dev_pool_split_u(const float* U_host, int64_t H, int64_t D, uint16_t* ut_host) {
  if (!U_host || !ut_host) return fail(VP_EINVAL, "null argument");
  if (H < 1 || H > vp::kPoolMaxH || D < 1)
    return fail(VP_EINVAL, "pool_split_u: 1 <= H <= " + std::to_string(vp::kPoolMaxH) + " and D >= 1");
  pool_split_u(U_host, H, D, ut_host);
  return VP_OK;
}

int vp_dev_pool_chunks(int64_t S) { return S < 1 || S > 0x7fffffff ? -1 : vp::pool_chunks((int)S); }

// The three entry points below come in two ranges of D: the plain names stop at 1024, as they always have (their
// refusals are pinned by tests), the *_wide names at vp::kPoolMaxD (Giant's 1408 = 11 x 128).
static int dev_pool_logits(const void* x, int in_dtype, int64_t rows, int64_t S, int64_t D, const float* U,
                           const void* Ut, int64_t H, float* logits, void* stream, int64_t max_d) {
  if (!x || !U || !logits) return fail(VP_EINVAL, "null argument");
  if (!float_dtype(in_dtype)) return fail(VP_EINVAL, "bad dtype");
  if (rows < 1 || S < 1 || rows % S) return fail(VP_EINVAL, "pool_logits: rows must be a positive multiple of S");
  if (D < 64 || D % 64 || D > max_d)
    return fail(VP_EINVAL, "pool_logits: D must be a multiple of 64, at most " + std::to_string(max_d));
  if (H < 1 || H > vp::kPoolMaxH) return fail(VP_EINVAL, "pool_logits: 1 <= H <= " + std::to_string(vp::kPoolMaxH));
  if (rows / 64 + 1 > 0x7fffffff) return fail(VP_EINVAL, "pool_logits: too many rows");
  VP_HIP(vp::pool_logits(x, in_dtype == VP_BF16, rows, (int)S, (int)D, U, (const vp::bf16_t*)Ut, (int)H, logits,
                         static_cast<hipStream_t>(stream)));
  return VP_OK;
}

// logits [rows/S][H][S] = x [rows][D] . U [H][D]; Ut: the split of vp_dev_pool_split_u on the device, or NULL
int vp_dev_pool_logits(const void* x, int in_dtype, int64_t rows, int64_t S, int64_t D, const float* U,
                       const void* Ut, int64_t H, float* logits, void* stream) {
  return dev_pool_logits(x, in_dtype, rows, S, D, U, Ut, H, logits, stream, 1024);
}
int vp_dev_pool_logits_wide(const void* x, int in_dtype, int64_t rows, int64_t S, int64_t D, const float* U,
                            const void* Ut, int64_t H, float* logits, void* stream) {
  return dev_pool_logits(x, in_dtype, rows, S, D, U, Ut, H, logits, stream, vp::kPoolMaxD);
}

static int dev_pool_softmax_wsum(const void* x, int in_dtype, int64_t G, int64_t S, int64_t D, int64_t H,
                                 const float* logits, float* stats, float* zpart, float* z, void* stream,
                                 int64_t block, int64_t max_d) {
  if (!x || !logits || !stats || !zpart || !z) return fail(VP_EINVAL, "null argument");
  if (!float_dtype(in_dtype)) return fail(VP_EINVAL, "bad dtype");
  if (G < 1 || S < 1 || G * S > 0x7fffffff) return fail(VP_EINVAL, "pool_softmax_wsum: bad G or S");
  if (D < block || D % block || D > max_d)
    return fail(VP_EINVAL, "pool_softmax_wsum: D must be a multiple of " + std::to_string(block) + ", at most " +
                               std::to_string(max_d));
  if (H < 1 || H > vp::kPoolMaxH)
    return fail(VP_EINVAL, "pool_softmax_wsum: 1 <= H <= " + std::to_string(vp::kPoolMaxH));
  VP_HIP(vp::pool_softmax_wsum(x, in_dtype == VP_BF16, (int)G, (int)S, (int)D, (int)H, logits, stats, zpart, z,
                               static_cast<hipStream_t>(stream)));
  return VP_OK;
}

// stats [G*H][2] = (max, 1/sum exp(l - max)), z [G][H][D] = sum_s softmax(logits)[g][h][s] x[g*S+s];
// zpart: scratch of [G][vp_dev_pool_chunks(S)][H][D] floats
int vp_dev_pool_softmax_wsum(const void* x, int in_dtype, int64_t G, int64_t S, int64_t D, int64_t H,
                             const float* logits, float* stats, float* zpart, float* z, void* stream) {
  return dev_pool_softmax_wsum(x, in_dtype, G, S, D, H, logits, stats, zpart, z, stream, 256, 1024);
}
// D = 128 k: an odd k ends in a 128-wide column block
int vp_dev_pool_softmax_wsum_wide(const void* x, int in_dtype, int64_t G, int64_t S, int64_t D, int64_t H,
                                  const float* logits, float* stats, float* zpart, float* z, void* stream) {
  return dev_pool_softmax_wsum(x, in_dtype, G, S, D, H, logits, stats, zpart, z, stream, 128, vp::kPoolMaxD);
}

// splits == 0: small_gemm (batch matrices at strides sA / sW / sB / sO); splits >= 1: small_gemm_splitk
// (batch == 1, part [splits][M][N] floats of scratch)
int vp_dev_small_gemm(const float* A, int64_t lda, int64_t sA, const float* Wt, int64_t sW, const float* bias,
                      int64_t sB, float* out, int64_t ldo, int64_t sO, int64_t M, int64_t N, int64_t K,
                      int64_t batch, int64_t splits, float* part, void* stream) {
  if (!A || !Wt || !out) return fail(VP_EINVAL, "null argument");
  if (M < 1 || N < 1 || K < 1 || batch < 1) return fail(VP_EINVAL, "small_gemm: M, N, K and batch must be positive");
  if ((M + 31) / 32 > 65535 || batch > 65535 || N > 0x7fffffff || K > 0x7fffffff)
    return fail(VP_EINVAL, "small_gemm: shape out of range");
  if (lda < K || ldo < N) return fail(VP_EINVAL, "small_gemm: lda >= K and ldo >= N");
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (splits == 0) {
    VP_HIP(vp::small_gemm(A, lda, sA, Wt, sW, bias, sB, out, ldo, sO, (int)M, (int)N, (int)K, (int)batch, s));
    return VP_OK;
  }
  if (splits < 0 || splits > 65535) return fail(VP_EINVAL, "small_gemm: bad splits");
  if (batch != 1 || !part) return fail(VP_EINVAL, "small_gemm: split-K needs batch == 1 and the partials buffer");
  if (K % splits) return fail(VP_EINVAL, "small_gemm: K must be a multiple of splits");
  VP_HIP(vp::small_gemm_splitk(A, lda, Wt, bias, out, ldo, (int)M, (int)N, (int)K, (int)splits, part, s));
  return VP_OK;
}

static int dev_ln_l2_rows(const void* x, int in_dtype, int64_t stride, int64_t rows, int64_t D, const float* gamma,
                          const float* beta, int do_l2, float* out, void* stream, int64_t max_d) {
  if (!x || !out || (gamma && !beta)) return fail(VP_EINVAL, "null argument");
  if (!float_dtype(in_dtype)) return fail(VP_EINVAL, "bad dtype");
  if (D < 1 || D > max_d) return fail(VP_EINVAL, "ln_l2_rows: 1 <= D <= " + std::to_string(max_d));
  if (rows < 1 || rows > 0x7fffffff || stride < D) return fail(VP_EINVAL, "ln_l2_rows: rows >= 1 and stride >= D");
  VP_HIP(vp::ln_l2_rows(x, in_dtype == VP_BF16, stride, (int)rows, (int)D, gamma, beta, do_l2, out,
                        static_cast<hipStream_t>(stream)));
  return VP_OK;
}

// out [rows][D] fp32 = LayerNorm (gamma = 1 + scale, beta; skipped when gamma is NULL) then L2 (if do_l2) of
// the rows x + r * stride
int vp_dev_ln_l2_rows(const void* x, int in_dtype, int64_t stride, int64_t rows, int64_t D, const float* gamma,
                      const float* beta, int do_l2, float* out, void* stream) {
  return dev_ln_l2_rows(x, in_dtype, stride, rows, D, gamma, beta, do_l2, out, stream, 1024);
}
int vp_dev_ln_l2_rows_wide(const void* x, int in_dtype, int64_t stride, int64_t rows, int64_t D, const float* gamma,
                           const float* beta, int do_l2, float* out, void* stream) {
  return dev_ln_l2_rows(x, in_dtype, stride, rows, D, gamma, beta, do_l2, out, stream, vp::kPoolMaxD);
}

// norm_policy 'primer_hybrid': xs [rows][D] fp32 += LayerNorm(y [rows][D] (fp32 / bf16) * (1 - pad [rows])) in
// place; gamma = 1 + scale; pad may be NULL; D = 128 k as vp_op_layernorm takes
int vp_dev_layernorm_residual(const void* y, int y_dtype, int64_t rows, int64_t D, const float* gamma,
                              const float* beta, const float* pad, float* xs, void* stream) {
  if (!y || !gamma || !beta || !xs) return fail(VP_EINVAL, "null argument");
  if (!float_dtype(y_dtype)) return fail(VP_EINVAL, "bad dtype");
  if (rows < 1 || rows > 0x7fffffff) return fail(VP_EINVAL, "layernorm_residual: bad rows");
  if (D < 128 || D % 128 || (D > 1536 && D != 2048))
    return fail(VP_ENOTSUP, "layernorm_residual: D must be a multiple of 128 up to 1536, or 2048");
  VP_HIP(vp::layernorm_residual(y, y_dtype == VP_BF16, (int)rows, (int)D, gamma, beta, pad, xs,
                                static_cast<hipStream_t>(stream)));
  return VP_OK;
}

// out [Q][L+1][D] = table[clamp(ids)] * scale + pos[t] for t < L, cls * scale at t = L; pad_out [Q][L+1] =
// [pad_in | 0].  ids, pad_in and pos are not read when L == 0.
int vp_dev_text_embed(const int32_t* ids, int64_t Q, int64_t L, const void* table, int table_dtype, int64_t V,
                      const float* cls, const float* pos, float scale, int64_t D, void* out, int out_dtype,
                      const float* pad_in, float* pad_out, void* stream) {
  if (!table || !cls || !out || !pad_out || (L > 0 && (!ids || !pos || !pad_in))) return fail(VP_EINVAL, "null argument");
  if (!float_dtype(table_dtype) || !float_dtype(out_dtype)) return fail(VP_EINVAL, "bad dtype");
  if (Q < 1 || L < 0 || V < 1 || D < 1 || V > 0x7fffffff || D > 0x7fffffff || Q * (L + 1) > 0x7fffffff)
    return fail(VP_EINVAL, "text_embed: Q >= 1, L >= 0, V >= 1, D >= 1");
  VP_HIP(vp::text_embed(ids, (int)Q, (int)L, table, table_dtype == VP_BF16, (int)V, cls, pos, scale, (int)D, out,
                        out_dtype == VP_BF16, pad_in, pad_out, static_cast<hipStream_t>(stream)));
  return VP_OK;
}

// run_pooler with the packed weights of a finalized vp_clip (kind 0) or vp_classifier (kind 1) over caller
// tokens feat [G*S][D] in the handle's fprop dtype -> dst [G][D] fp32.  scratch == NULL: only writes the
// bytes it needs to *scratch_bytes.
int vp_dev_pooler(int kind, void* handle, const void* feat, int64_t G, int64_t S, int do_l2, float* dst,
                  void* scratch, size_t* scratch_bytes, void* stream) {
  if (!handle || !scratch_bytes) return fail(VP_EINVAL, "null argument");
  if (kind != 0 && kind != 1) return fail(VP_EINVAL, "kind must be 0 (vp_clip) or 1 (vp_classifier)");
  WrapHandle* w = kind == 0 ? static_cast<WrapHandle*>(static_cast<vp_clip*>(handle))
                            : static_cast<WrapHandle*>(static_cast<vp_classifier*>(handle));
  if (!w->finalized) return fail(VP_ESTATE, "the handle has not been finalized");
  if (G < 1 || S < 1 || G * S > 0x7fffffff) return fail(VP_EINVAL, "pooler: bad G or S");
  const vp_config& v = w->video->cfg;
  const int D = v.model_dim, NH = v.num_heads;
  if (int rc = check_pooler_dims(D, NH)) return rc;
  // zpart holds the G * pool_chunks(S) chunk sums (as pool_video_ws sizes it for its larger grouping)
  size_t total = 0;
  const PoolWs L = carve_pool_ws(total, G * S, G, D, NH, w->pool.dp, (size_t)G * vp::pool_chunks((int)S) * NH * D);
  if (!scratch) {
    *scratch_bytes = total;
    return VP_OK;
  }
  if (!feat || !dst) return fail(VP_EINVAL, "null argument");
  if (*scratch_bytes < total) return fail(VP_EINVAL, "scratch too small: need " + std::to_string(total));
  VP_HIP(hipSetDevice(w->device));
  Fwd f;
  f.s = static_cast<hipStream_t>(stream); f.bf = w->bf16(); f.M = (int)(G * S); f.D = D; f.NH = NH;
  return run_pooler(f, w->pool, feat, (int)(G * S), (int)G, (int)S, D, NH, L.at(scratch), do_l2, dst);
}

}  // extern "C"
