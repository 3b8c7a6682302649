// C-ABI of the classifier head's training ops (vp_op_probe_*): forward and backward of atten_pooler + projection
// (encoders.py:634-652) over frozen tokens.  The forward folds the query into the key projection on the device
// (probe_kernels.hip) and then runs the engines' pooler forward (pooler_stream, pooler_project) and the projection;
// the backward is steps 1-8 below, two streaming passes over the tokens and parameter-sized products.  The
// *_masked entry points take token paddings [B][S] as well (pool_stream.h says what the passes do with them); the
// unmasked ones are their paddings = NULL case, which launches the kernels without the parameter.  The mask needs no
// workspace of its own.
#include "vp_internal.h"

using namespace vpi;

namespace {

// forward state the backward reads (the folded weights, the pooler's scratch, emb), then the backward's own
// scratch (offsets in bytes)
struct ProbeWs {
  size_t qraw = 0, qt = 0, U = 0, Ut = 0, wvt = 0, wpt = 0, gamma = 0;
  PoolWs fw;
  size_t emb = 0;
  size_t demb = 0, dpooled = 0, lnst = 0, denc = 0, dz = 0, dzt = 0, r = 0, dl = 0, dUclip = 0, dU = 0, dqt = 0;
  size_t total = 0;
};

ProbeWs probe_ws(int64_t D, int64_t H, int64_t B, int64_t S) {
  ProbeWs L;
  size_t off = 0;
  auto take = [&](size_t bytes) {
    const size_t at = off;
    off = align256(off + bytes);
    return at;
  };
  const size_t f = 4;
  L.qraw = take(D * f);
  L.qt = take(D * f);
  L.U = take(H * D * f);
  L.Ut = take((size_t)32 * D * 2);
  L.wvt = take((size_t)D * D * f);
  L.wpt = take((size_t)D * D * f);
  L.gamma = take(D * f);
  // zpart: chunk sums of both weighted-sum passes; the output projection's 8 split-K partials reuse it
  L.fw = carve_pool_ws(off, B * S, B, D, H, D / H,
                       std::max<size_t>((size_t)B * vp::pool_chunks((int)S) * H * D, (size_t)8 * B * D));
  L.emb = take((size_t)B * D * f);
  L.demb = take((size_t)B * D * f);
  L.dpooled = take((size_t)B * D * f);
  L.lnst = take((size_t)B * 2 * f);
  L.denc = take((size_t)B * D * f);
  L.dz = take((size_t)B * H * D * f);
  L.dzt = take((size_t)B * 32 * D * 2);
  L.r = take((size_t)B * H * f);
  L.dl = take((size_t)B * H * S * f);
  L.dUclip = take((size_t)B * H * D * f);
  L.dU = take(H * D * f);
  L.dqt = take(D * f);
  L.total = off;
  return L;
}

int check_probe_shape(const vp_probe_dims* dims, int64_t B, int64_t S) {
  if (!dims) return fail(VP_EINVAL, "null argument");
  if (B < 1 || S < 1) return fail(VP_EINVAL, "probe: tokens must be [B, S, D] with B >= 1 and S >= 1");
  if (dims->model_dim < 1 || dims->num_heads < 1 || dims->num_classes < 1)
    return fail(VP_EINVAL, "probe: model_dim, num_heads and num_classes must be positive");
  if (int rc = check_pooler_dims(dims->model_dim, dims->num_heads)) return rc;
  if (dims->model_dim % dims->num_heads)
    return fail(VP_ENOTSUP, "probe: model_dim must be a multiple of num_heads");
  if (B > 65535 || B * S > 0x7fffffff) return fail(VP_ENOTSUP, "probe: at most 65535 clips and 2^31 - 1 tokens");
  return VP_OK;
}

template <class Leaves>  // vp_probe_params or vp_probe_grads: the same 14 names
bool any_null(const Leaves& p) {
  return !p.query || !p.per_dim_scale || !p.query_w || !p.query_b || !p.key_w || !p.key_b || !p.value_w ||
         !p.value_b || !p.post_w || !p.post_b || !p.ln_scale || !p.ln_bias || !p.proj_kernel || !p.proj_bias;
}

int check_probe_call(const vp_probe_dims* dims, int dtype, int64_t B, int64_t S, size_t ws_bytes, ProbeWs* L) {
  if (int rc = check_probe_shape(dims, B, S)) return rc;
  if (dtype != VP_F32 && dtype != VP_BF16) return fail(VP_EINVAL, "probe: tokens must be VP_F32 or VP_BF16");
  *L = probe_ws(dims->model_dim, dims->num_heads, B, S);
  if (ws_bytes < L->total) return fail(VP_EINVAL, "workspace too small: need " + std::to_string(L->total));
  return VP_OK;
}

}  // namespace

extern "C" {

int vp_op_probe_workspace_bytes(const vp_probe_dims* dims, int64_t B, int64_t S, size_t* bytes) {
  if (!dims || !bytes) return fail(VP_EINVAL, "null argument");
  if (int rc = check_probe_shape(dims, B, S)) return rc;
  *bytes = probe_ws(dims->model_dim, dims->num_heads, B, S).total;
  return VP_OK;
}

int vp_op_probe_forward(const vp_probe_dims* dims, const vp_probe_params* params, const void* tokens, int dtype,
                        int64_t B, int64_t S, float* logits, float* emb, void* ws, size_t ws_bytes, void* stream) {
  return vp_op_probe_forward_masked(dims, params, tokens, dtype, B, S, nullptr, logits, emb, ws, ws_bytes, stream);
}

int vp_op_probe_forward_masked(const vp_probe_dims* dims, const vp_probe_params* params, const void* tokens, int dtype,
                               int64_t B, int64_t S, const float* paddings, float* logits, float* emb, void* ws,
                               size_t ws_bytes, void* stream) {
  using namespace vp;
  if (!dims || !params || !tokens || !logits || !ws || any_null(*params)) return fail(VP_EINVAL, "null argument");
  ProbeWs L;
  if (int rc = check_probe_call(dims, dtype, B, S, ws_bytes, &L)) return rc;
  const vp_probe_params& p = *params;
  const int D = dims->model_dim, H = dims->num_heads, C = dims->num_classes, dh = D / H, G = (int)B;
  const int bf = dtype == VP_BF16;
  hipStream_t s = static_cast<hipStream_t>(stream);
  char* w = static_cast<char*>(ws);
  auto f32 = [&](size_t off) { return reinterpret_cast<float*>(w + off); };
  bf16_t* Ut = reinterpret_cast<bf16_t*>(w + L.Ut);
  // the fold an engine's finalize does on the host (pack_pooler), on the device: the weights change every step
  VP_HIP(probe_gemm(p.query, 0, 0, 1, p.query_w, 0, D, f32(L.qraw), 0, D, 1, D, D, 1, s));
  VP_HIP(probe_fold(f32(L.qraw), p.query_b, p.per_dim_scale, p.key_w, D, H, bf, f32(L.qt), f32(L.U), Ut, s));
  VP_HIP(probe_pack(p.value_w, p.post_w, p.ln_scale, D, H, f32(L.wvt), f32(L.wpt), f32(L.gamma), s));
  // the pooler's forward on the folded weights, then the projection
  const PoolerW pw{Ut, f32(L.U), f32(L.wvt), p.value_b, f32(L.wpt), p.post_b, f32(L.gamma), p.ln_bias, dh};
  const PoolScratch sc = L.fw.at(ws);
  VP_HIP(pooler_stream(s, bf, pw, tokens, G, (int)S, D, H, sc, paddings));
  VP_HIP(pooler_project(s, pw, G, D, H, sc, 0, f32(L.emb)));
  VP_HIP(small_gemm(f32(L.emb), D, 0, p.proj_kernel, 0, p.proj_bias, 0, logits, C, 0, G, C, D, 1, s));
  if (emb) VP_HIP(hipMemcpyAsync(emb, f32(L.emb), (size_t)B * D * 4, hipMemcpyDeviceToDevice, s));
  return VP_OK;
}

int vp_op_probe_backward(const vp_probe_dims* dims, const vp_probe_params* params, const void* tokens, int dtype,
                         int64_t B, int64_t S, const float* dlogits, const vp_probe_grads* grads, void* ws,
                         size_t ws_bytes, void* stream) {
  return vp_op_probe_backward_masked(dims, params, tokens, dtype, B, S, nullptr, dlogits, grads, ws, ws_bytes, stream);
}

int vp_op_probe_backward_masked(const vp_probe_dims* dims, const vp_probe_params* params, const void* tokens,
                                int dtype, int64_t B, int64_t S, const float* paddings, const float* dlogits,
                                const vp_probe_grads* grads, void* ws, size_t ws_bytes, void* stream) {
  using namespace vp;
  if (!dims || !params || !tokens || !dlogits || !grads || !ws || any_null(*params) || any_null(*grads))
    return fail(VP_EINVAL, "null argument");
  ProbeWs L;
  if (int rc = check_probe_call(dims, dtype, B, S, ws_bytes, &L)) return rc;
  const vp_probe_params& p = *params;
  const vp_probe_grads& g = *grads;
  const int D = dims->model_dim, H = dims->num_heads, C = dims->num_classes, dh = D / H, G = (int)B;
  const int64_t HD = (int64_t)H * D;
  const int bf = dtype == VP_BF16;
  hipStream_t s = static_cast<hipStream_t>(stream);
  char* w = static_cast<char*>(ws);
  auto f32 = [&](size_t off) { return reinterpret_cast<float*>(w + off); };
  bf16_t* dzt = reinterpret_cast<bf16_t*>(w + L.dzt);
  // 1. projection: demb = dlogits Wc^T, dWc = emb^T dlogits, dbc = sum_b dlogits
  VP_HIP(probe_dot(dlogits, 0, C, p.proj_kernel, 0, C, f32(L.demb), 0, D, G, D, C, 1, s));
  VP_HIP(probe_gemm(f32(L.emb), 0, 1, D, dlogits, 0, C, g.proj_kernel, 0, C, D, C, G, 1, s));
  VP_HIP(probe_colsum(dlogits, G, C, g.proj_bias, s));
  // 2. LayerNorm
  VP_HIP(probe_ln_bwd(f32(L.fw.pooled), f32(L.demb), f32(L.gamma), G, D, f32(L.dpooled), f32(L.lnst), g.ln_scale,
                      g.ln_bias, s));
  // 3. post projection: dWp[d][h][j] = sum_b dpooled[b][d] enc[b][h][j], denc = dpooled Wp (small_gemm takes this
  // layout too, but its 12 workgroups run the K = D loop in 55 us at B = 32 where the 16-way K split takes a fifth)
  VP_HIP(probe_gemm(f32(L.dpooled), 0, 1, D, f32(L.fw.enc), 0, D, g.post_w, 0, D, D, D, G, 1, s));
  VP_HIP(probe_colsum(f32(L.dpooled), G, D, g.post_b, s));
  VP_HIP(probe_gemm(f32(L.dpooled), 0, D, 1, p.post_w, 0, D, f32(L.denc), 0, D, G, D, D, 1, s));
  // 4. value projection, per head: dWv[:,h,:] = sum_b z[b,h]^T denc[b,h], dz[b,h] = denc[b,h] Wv[:,h,:]^T
  VP_HIP(probe_gemm(f32(L.fw.z), D, 1, HD, f32(L.denc), dh, D, g.value_w, dh, D, D, dh, G, H, s));
  VP_HIP(probe_colsum(f32(L.denc), G, D, g.value_b, s));
  VP_HIP(probe_dot(f32(L.denc), dh, D, p.value_w, dh, D, f32(L.dz), D, HD, G, D, dh, H, s));
  // 5. r = z . dz (the softmax term needs no pass) and, for bf16 tokens, the hi | lo operand of each clip; pass 1
  VP_HIP(probe_dz_finish(f32(L.fw.z), f32(L.dz), G, H, D, bf, dzt, f32(L.r), s));
  VP_HIP(probe_dl(tokens, bf, G, (int)S, D, H, f32(L.dz), bf ? dzt : nullptr, f32(L.fw.logits), f32(L.fw.stats), f32(L.r),
                  f32(L.dl), s, paddings));
  // 6. pass 2
  VP_HIP(probe_wsum(tokens, bf, G, (int)S, D, H, f32(L.dl), f32(L.fw.zpart), f32(L.dUclip), f32(L.dU), s, paddings));
  // 7. fold: dWk = dU (x) q~, dq~[h] = Wk[:,h,:]^T dU[h], dbk = 0
  VP_HIP(probe_fold_bwd(f32(L.dU), f32(L.qt), D, H, g.key_w, s));
  VP_HIP(hipMemsetAsync(g.key_b, 0, (size_t)D * 4, s));
  VP_HIP(probe_gemm(f32(L.dU), D, 0, 1, p.key_w, dh, D, f32(L.dqt), dh, dh, 1, dh, D, H, s));
  // 8. query: dbq = dqraw, dWq = query^T (x) dqraw, dquery = Wq dqraw
  VP_HIP(probe_dq(f32(L.dqt), f32(L.qraw), p.per_dim_scale, D, H, g.query_b, g.per_dim_scale, s));
  VP_HIP(probe_gemm(p.query, 0, 1, 0, g.query_b, 0, 0, g.query_w, 0, D, D, D, 1, 1, s));
  VP_HIP(probe_dot(g.query_b, 0, 0, p.query_w, 0, D, g.query, 0, D, 1, D, D, 1, s));
  return VP_OK;
}

// Not in the public header: one streaming pass of the backward on its own, for tools/probe_bench.py.  which 1: pass 1
// (dl from the tokens), 2: pass 2 (dU with its reduction), on a workspace vp_op_probe_backward has run on (each pass
// rewrites what that call left there, from the same inputs).
int vp_dev_probe_backward_pass(const vp_probe_dims* dims, const void* tokens, int dtype, int64_t B, int64_t S,
                               int which, void* ws, size_t ws_bytes, void* stream) {
  using namespace vp;
  if (!dims || !tokens || !ws) return fail(VP_EINVAL, "null argument");
  if (which != 1 && which != 2) return fail(VP_EINVAL, "which must be 1 (pass 1) or 2 (pass 2)");
  ProbeWs L;
  if (int rc = check_probe_call(dims, dtype, B, S, ws_bytes, &L)) return rc;
  const int D = dims->model_dim, H = dims->num_heads;
  const int bf = dtype == VP_BF16;
  hipStream_t s = static_cast<hipStream_t>(stream);
  char* w = static_cast<char*>(ws);
  auto f32 = [&](size_t off) { return reinterpret_cast<float*>(w + off); };
  if (which == 1)
    VP_HIP(probe_dl(tokens, bf, (int)B, (int)S, D, H, f32(L.dz), bf ? reinterpret_cast<bf16_t*>(w + L.dzt) : nullptr,
                    f32(L.fw.logits), f32(L.fw.stats), f32(L.r), f32(L.dl), s));
  else
    VP_HIP(probe_wsum(tokens, bf, (int)B, (int)S, D, H, f32(L.dl), f32(L.fw.zpart), f32(L.dUclip), f32(L.dU), s));
  return VP_OK;
}

}  // extern "C"
