// C-ABI implementation (include/videoprism_hip.h): parameter intake in the reference's
// Flax layout, packing into kernel-ready device buffers, and the FactorizedEncoder
// forward schedule (encoders.py:411-580) over the HIP kernels.
#include "../../include/videoprism_hip.h"

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdlib>
#include <cxxabi.h>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "vp_kernels.h"

#include "vp_internal.h"

using namespace vpi;

namespace {

// the temporal positional table for T frames, [T][D]: temporal_pos_emb/emb_var itself when T ==
// pos_emb_t, else _interpolate_emb_1d (encoders.py:107-130: jax.image.resize 'bilinear', antialiased
// when shrinking), fp64 on the host
std::vector<float> temporal_table(const vp_handle* h, int T) {
  const int64_t D = h->cfg.model_dim;
  const int Tp = h->cfg.pos_emb_t;
  const std::vector<float>& e = h->temporal_pos_host;
  std::vector<float> dst((size_t)T * D);
  if (T == Tp) {
    std::memcpy(dst.data(), e.data(), (size_t)T * D * 4);
    return dst;
  }
  const auto w = resize_weights(Tp, T);
  for (int t = 0; t < T; ++t)
    for (int64_t d = 0; d < D; ++d) {
      double s = 0.0;
      for (int i = 0; i < Tp; ++i) s += w[(size_t)i * T + t] * e[(size_t)i * D + d];
      dst[(size_t)t * D + d] = (float)s;
    }
  return dst;
}

// the encoder's leaves under h->prefix (encoders.py:391-580)
void build_expected(vp_handle* h) {
  const vp_config& c = h->cfg;
  const int64_t D = c.model_dim, F = c.mlp_dim, NH = c.num_heads;
  const int64_t P = c.patch_size;
  const std::string& px = h->prefix;
  h->expect(px + "patch_projection/linear/kernel", {P * P * 3, D});
  h->expect(px + "patch_projection/linear/bias", {D});
  h->expect(px + "spatial_pos_emb/emb_var", {(int64_t)c.pos_emb_h * c.pos_emb_w, D});
  add_stack_expected(*h, px + "spatial_encoder/transformers_stack/x_layers/", c.num_spatial_layers, D, F, NH);
  h->expect(px + "spatial_ln/scale", {D});
  h->expect(px + "spatial_ln/bias", {D});
  h->expect(px + "temporal_pos_emb/emb_var", {(int64_t)c.pos_emb_t, D});
  add_stack_expected(*h, px + "temporal_encoder/transformers_stack/x_layers/", c.num_temporal_layers, D, F, NH);
  h->expect(px + "temporal_ln/scale", {D});
  h->expect(px + "temporal_ln/bias", {D});
}

}  // namespace

int vpi::create_encoder(const vp_config* cfg, int device, const std::string& prefix, vp_handle** out) {
  if (!cfg || !out) return fail(VP_EINVAL, "null argument");
  *out = nullptr;
  if (cfg->num_heads <= 0 || cfg->model_dim % cfg->num_heads)
    return fail(VP_EINVAL, "model_dim must be divisible by num_heads");
  if (cfg->fprop_dtype != VP_F32 && cfg->fprop_dtype != VP_BF16)
    return fail(VP_EINVAL, "fprop_dtype must be VP_F32 or VP_BF16");
  // fp32 runs 64- and 88-wide heads (88: the Giant encoder, 1408 / 16) at any model_dim % 128 == 0; the bf16
  // attention kernels and 256-wide GEMM tiles are 64-wide heads and model_dim % 256 == 0 only
  const bool f32 = cfg->fprop_dtype == VP_F32;
  const int dph = cfg->model_dim / cfg->num_heads;
  if (!supported_dh(!f32, dph))
    return fail(VP_ENOTSUP, dph == 88 ? "dim_per_head 88 needs fprop_dtype float32 (bfloat16 runs dim_per_head 64 only)"
                                      : "dim_per_head must be 64, or 88 with fprop_dtype float32");
  if (cfg->model_dim % (f32 ? 128 : 256) || cfg->mlp_dim % 256)
    return fail(VP_ENOTSUP, f32 ? "model_dim must be a multiple of 128 and mlp_dim of 256"
                                : "model_dim and mlp_dim must be multiples of 256 with fprop_dtype bfloat16");
  if (cfg->patch_size <= 0 || cfg->pos_emb_t <= 0 || cfg->pos_emb_h <= 0 || cfg->pos_emb_w <= 0)
    return fail(VP_EINVAL, "bad patch_size / pos_emb_shape");
  if (cfg->num_spatial_layers < 0 || cfg->num_temporal_layers < 0)
    return fail(VP_EINVAL, "negative layer count");
  if (!std::isfinite(cfg->atten_logit_cap)) return fail(VP_EINVAL, "atten_logit_cap must be finite");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev)
    return fail(VP_EINVAL, "invalid HIP device " + std::to_string(device));
  vp_handle* h = new vp_handle();
  h->cfg = *cfg;
  h->device = device;
  h->prefix = prefix;
  build_expected(h);
  *out = h;
  return VP_OK;
}

extern "C" {

const char* vp_last_error(void) { return g_err.c_str(); }
int vp_abi_version(void) { return VP_ABI_VERSION; }

int vp_create(const vp_config* cfg, int device, vp_handle** out) { return create_encoder(cfg, device, "", out); }

int vp_destroy(vp_handle* h) {
  if (!h) return VP_OK;
  h->free_all();
  for (auto& e : h->prof.ev) hipEventDestroy(e);
  delete h;
  return VP_OK;
}

int vp_param_count(const vp_handle* h, int* count) {
  if (!h || !count) return fail(VP_EINVAL, "null argument");
  *count = (int)h->names.size();
  return VP_OK;
}

int vp_param_name(const vp_handle* h, int index, const char** name) {
  if (!h || !name || index < 0 || index >= (int)h->names.size()) return fail(VP_EINVAL, "bad index");
  *name = h->names[index].c_str();
  return VP_OK;
}

int vp_set_param(vp_handle* h, const char* name, const float* host_data, const int64_t* shape, int ndim) {
  return h ? h->set(name, host_data, shape, ndim) : fail(VP_EINVAL, "null argument");
}

int vp_finalize(vp_handle* h) {
  if (!h) return fail(VP_EINVAL, "null handle");
  if (h->finalized) return VP_OK;
  if (const std::string* n = h->first_missing()) return fail(VP_ESTATE, "missing parameter: " + *n);
  VP_HIP(hipSetDevice(h->device));
  const vp_config& c = h->cfg;
  const bool bf = h->bf16();
  const int64_t D = c.model_dim, P = c.patch_size;
  const int64_t kreal = P * P * 3;
  h->kpad = (int)(((kreal + 63) / 64) * 64);
  int rc;
  const std::string& px = h->prefix;
  {  // patch projection: kernel [kreal][D] -> [D][kpad]
    const auto& k = h->data(px + "patch_projection/linear/kernel");
    std::vector<float> t((size_t)D * h->kpad, 0.0f);
    for (int64_t i = 0; i < kreal; ++i)
      for (int64_t n = 0; n < D; ++n) t[(size_t)n * h->kpad + i] = k[(size_t)i * D + n];
    if ((rc = h->upload_mat(t, bf, &h->wpatch))) return rc;
    if (bf && vp::video_patch_ok((int)P)) {  // the frames' chunk order (gemm_bf16_w4_video, vp_kernels.h)
      const int64_t cpr = vp::video_patch_cpr((int)P), kv = vp::video_patch_k((int)P);
      std::vector<float> tv((size_t)D * kv, 0.0f);
      for (int64_t py = 0; py < P; ++py)
        for (int64_t cr = 0; cr < cpr; ++cr) {
          const int64_t vo = std::min<int64_t>(8 * cr, 3 * P - 8);
          for (int64_t e = 0; e < 8; ++e) {
            const int64_t v = vo + e;
            if (cr == cpr - 1 && v < 8 * (cpr - 1)) continue;  // overlap with the row's previous chunk
            for (int64_t n = 0; n < D; ++n) tv[(size_t)n * kv + 64 * py + 8 * cr + e] = k[(size_t)(py * 3 * P + v) * D + n];
          }
        }
      if ((rc = h->upload_mat(tv, bf, &h->wpatch_v))) return rc;
    }
    if ((rc = h->upload_f32(h->data(px + "patch_projection/linear/bias"), &h->bpatch))) return rc;
  }
  if ((rc = h->upload_f32(h->data(px + "spatial_pos_emb/emb_var"), &h->spatial_pos))) return rc;
  h->spatial_pos_host = h->data(px + "spatial_pos_emb/emb_var");
  {  // temporal positional tables for T = 1..kPrecomputedT in one buffer (encoders.py:543-553)
    h->temporal_pos_host = h->data(px + "temporal_pos_emb/emb_var");
    std::vector<float> tab;
    std::vector<size_t> off(kPrecomputedT + 1);
    for (int T = 1; T <= kPrecomputedT; ++T) {
      off[T] = tab.size();
      const std::vector<float> t = temporal_table(h, T);
      tab.insert(tab.end(), t.begin(), t.end());
    }
    float* dev = nullptr;
    if ((rc = h->upload_f32(tab, &dev))) return rc;
    for (int T = 1; T <= kPrecomputedT; ++T) h->temporal_pos[T] = dev + off[T];
  }
  const bool fold = bf;  // LayerNorms folded into the consuming GEMMs
  if ((rc = pack_stack(*h, bf, px + "spatial_encoder/transformers_stack/x_layers/", c.num_spatial_layers, D, c.mlp_dim,
                       c.num_heads, fold, h->spatial, QKV_BLOCKED)))
    return rc;
  if ((rc = pack_stack(*h, bf, px + "temporal_encoder/transformers_stack/x_layers/", c.num_temporal_layers, D,
                       c.mlp_dim, c.num_heads, fold, h->temporal,
                       fold && c.model_dim == c.num_heads * 64 ? QKV_PER_HEAD : QKV_PLAIN)))
    return rc;
  std::vector<float> g(D);
  const char* lns[2] = {"spatial_ln", "temporal_ln"};
  for (int i = 0; i < 2; ++i) {
    const auto& sc = h->data(px + lns[i] + "/scale");
    for (int64_t d = 0; d < D; ++d) g[d] = sc[d] + 1.0f;
    float** gp = i == 0 ? &h->sln_g : &h->tln_g;
    float** bp = i == 0 ? &h->sln_b : &h->tln_b;
    if ((rc = h->upload_f32(g, gp)) || (rc = h->upload_f32(h->data(px + lns[i] + "/bias"), bp)))
      return rc;
  }
  h->seal();
  return VP_OK;
}

int vp_prepare_geometry(vp_handle* h, int64_t H, int64_t W) {
  if (!h) return fail(VP_EINVAL, "null handle");
  if (!h->finalized) return fail(VP_ESTATE, "vp_finalize has not been called");
  const vp_config& c = h->cfg;
  const int64_t P = c.patch_size, D = c.model_dim;
  if (H < 1 || W < 1 || H % P || W % P) return fail(VP_EINVAL, patch_size_message(H, W, P));
  const int gm = (int)(H / P), gn = (int)(W / P);
  if ((gm == c.pos_emb_h && gn == c.pos_emb_w) || h->grid_pos.count({gm, gn})) return VP_OK;
  // _interpolate_emb_2d (encoders.py:133-165): separable jax.image.resize 'bilinear' (antialiased
  // when shrinking) of the [pos_h, pos_w, D] table, fp64 on the host
  const int ph = c.pos_emb_h, pw = c.pos_emb_w;
  const auto wh = resize_weights(ph, gm), ww = resize_weights(pw, gn);
  const auto& e = h->spatial_pos_host;
  std::vector<float> out((size_t)gm * gn * D);
  std::vector<double> acc(D);
  for (int i = 0; i < gm; ++i)
    for (int j = 0; j < gn; ++j) {
      std::fill(acc.begin(), acc.end(), 0.0);
      for (int a = 0; a < ph; ++a) {
        const double wa = wh[(size_t)a * gm + i];
        if (wa == 0.0) continue;
        for (int b = 0; b < pw; ++b) {
          const double w = wa * ww[(size_t)b * gn + j];
          if (w == 0.0) continue;
          const float* src = e.data() + ((size_t)a * pw + b) * D;
          for (int64_t d = 0; d < D; ++d) acc[d] += w * src[d];
        }
      }
      for (int64_t d = 0; d < D; ++d) out[((size_t)i * gn + j) * D + d] = (float)acc[d];
    }
  VP_HIP(hipSetDevice(h->device));
  float* dev = nullptr;
  int rc = h->upload_f32(out, &dev);
  if (rc) return rc;
  h->grid_pos[{gm, gn}] = dev;
  return VP_OK;
}

int vp_prepare_frames(vp_handle* h, int64_t T) {
  if (!h) return fail(VP_EINVAL, "null handle");
  if (!h->finalized) return fail(VP_ESTATE, "vp_finalize has not been called");
  if (T < 1 || T > (int64_t)1 << 20) return fail(VP_EINVAL, "T must be in [1, 2^20]");
  if (h->temporal_pos.count((int)T)) return VP_OK;
  VP_HIP(hipSetDevice(h->device));
  float* dev = nullptr;
  int rc = h->upload_f32(temporal_table(h, (int)T), &dev);
  if (rc) return rc;
  h->temporal_pos[(int)T] = dev;
  return VP_OK;
}

int vp_workspace_bytes(const vp_handle* h, int64_t B, int64_t T, int64_t H, int64_t W,
                       size_t* bytes) {
  if (!h || !bytes) return fail(VP_EINVAL, "null argument");
  int rc = check_geometry(h, B, T, H, W);
  if (rc) return rc;
  *bytes = ws_layout(h, chunk_of(h, B, T, H, W), T, H, W).total;
  return VP_OK;
}

}  // extern "C"

namespace {

// What the two halves of a forward chunk share: the workspace carve-up for B x T frames of H x W, the launch
// context and the token paddings in both row orders.
struct Chunk {
  WsLayout L;
  hipStream_t s = nullptr;
  bool bf = false;
  int Nsp = 0, M = 0, Mp = 0;  // patches per frame, tokens, GEMM rows
  char* ws = nullptr;
  float* pad_btn = nullptr;
  float* pad_bnt = nullptr;
  Fwd f;
};

// the spatial positional table for frames of H x W (encoders.py:497-512)
int find_spatial_pos(const vp_handle* h, int64_t H, int64_t W, const float** sp_pos) {
  const vp_config& c = h->cfg;
  const int P_ = c.patch_size;
  const int Nsp = (int)((H / P_) * (W / P_));
  *sp_pos = h->spatial_pos;
  if (Nsp != c.pos_emb_h * c.pos_emb_w || H / P_ != c.pos_emb_h) {
    auto it = h->grid_pos.find({(int)(H / P_), (int)(W / P_)});
    if (it == h->grid_pos.end())
      return fail(VP_ESTATE, "patch grid differs from pos_emb_shape[1:]: call vp_prepare_geometry first");
    *sp_pos = it->second;
  }
  return VP_OK;
}

// the temporal positional table for clips of T frames (encoders.py:543-553)
int find_temporal_pos(const vp_handle* h, int64_t T, const float** tpos) {
  const auto tp = h->temporal_pos.find((int)T);
  if (tp == h->temporal_pos.end())
    return fail(VP_ESTATE, "no temporal positional table for T = " + std::to_string(T) + ": call vp_prepare_frames first");
  *tpos = tp->second;
  return VP_OK;
}

// Opens a chunk of B x T frames in `workspace`: sets the device, expands the frame paddings [B*T] to token paddings
// and fills the launch context.  The first launches of a forward chunk.
int begin_chunk(vp_handle* h, int64_t B, int64_t T, int64_t H, int64_t W, const float* frame_paddings,
                void* workspace, void* stream, Chunk* ck) {
  using namespace vp;
  ck->L = ws_layout(h, B, T, H, W);
  const WsLayout& L = ck->L;
  VP_HIP(hipSetDevice(h->device));
  hipStream_t s = static_cast<hipStream_t>(stream);
  const vp_config& c = h->cfg;
  const bool bf = is_bf16(h);
  const int P_ = c.patch_size;
  const int Nsp = (int)((H / P_) * (W / P_));
  const int M = (int)(B * T * Nsp);  // tokens
  const int Mp = (int)padded_rows(h, M);  // GEMM rows
  const int D = c.model_dim;
  char* ws = static_cast<char*>(workspace);
  ck->s = s; ck->bf = bf; ck->Nsp = Nsp; ck->M = M; ck->Mp = Mp; ck->ws = ws;
  const char* ge = bf ? gemm_bf16_check(Mp, 3 * D, D, D, D) : gemm_f32_check(Mp, 3 * D, D, D, D);
  if (ge) return fail(VP_ENOTSUP, ge);
  if (frame_paddings) {
    float* pad_btn = reinterpret_cast<float*>(ws + L.pad_btn);
    float* pad_bnt = reinterpret_cast<float*>(ws + L.pad_bnt);
    if (Mp > M) {
      VP_HIP(hipMemsetAsync(pad_btn + M, 0, (size_t)(Mp - M) * 4, s));
      VP_HIP(hipMemsetAsync(pad_bnt + M, 0, (size_t)(Mp - M) * 4, s));
    }
    VP_HIP(expand_paddings(frame_paddings, (int)B, (int)T, Nsp, pad_btn, pad_bnt, s));
    ck->pad_btn = pad_btn;
    ck->pad_bnt = pad_bnt;
  }
  // bf16: LayerNorms inside the layers are folded into the consuming GEMMs (EPI_*_LN); the
  // residual-stream producers emit row statistics (EPI_*_ST) that ln_stats_finalize turns into
  // (rstd, -mean*rstd) per row
  Fwd& f = ck->f;
  f.s = s; f.bf = bf; f.M = Mp; f.D = D; f.NH = c.num_heads; f.cap = c.atten_logit_cap;
  f.hb = ws + L.hbuf; f.big = ws + L.big;
  f.f32_two_chains = f32_two_chains(c);
  f.st_part = reinterpret_cast<float*>(ws + L.st_part);
  f.ln_rs = reinterpret_cast<float*>(ws + L.ln_rs);
  f.pf = &h->prof;
  return VP_OK;
}

// The spatial half of FactorizedEncoder.__call__ (encoders.py:436-514, :459-478) over the BT frames of an open chunk:
// leaves the spatial residual stream, before spatial_ln, in x [Mp][D] (the frame states)
int spatial_half(vp_handle* h, Chunk& ck, const void* video, int in_dtype, int64_t BT, int64_t H, int64_t W,
                 const float* sp_pos, void* x) {
  using namespace vp;
  int rc;
  hipStream_t s = ck.s;
  const vp_config& c = h->cfg;
  const bool bf = ck.bf;
  const int P_ = c.patch_size;
  const int Nsp = ck.Nsp, M = ck.M, Mp = ck.Mp;
  const int D = c.model_dim, F = c.mlp_dim;
  const size_t es = bf ? 2 : 4;
  Fwd& f = ck.f;
  void* big = f.big;
  const int epi_pos = bf ? EPI_POS_BF16 : EPI_POS_F32;
  const double dM = M, dD = D, dE = (double)es;
  auto gbytes = [&](double K, double N, double outb, double resid) { return gemm_bytes(dM, K, N, dE, outb, resid); };

  // 1. tokenisation + patch projection + spatial pos-emb (encoders.py:436-514)
  const double kreal = (double)P_ * P_ * 3;
  const double in_es = (double)dtype_bytes(in_dtype);
  const bool fold = bf && c.num_spatial_layers > 0;  // LN1 of spatial layer 0 folded
  // bf16 on a 16x16 patch grid: the patch embedding reads the frames themselves (no patch
  // tensor); f32 / uint8 frames are converted to bf16 frames first (the patchify kernels' per-value
  // conversion, so every input dtype gives bitwise the bf16 caller's result)
  // the fused path reads bf16 frames in 16-B chunks at 4-B granularity, and video_to_bf16 reads
  // float4 / uchar4: frames at a less aligned address (a sliced caller buffer) take patchify + GEMM
  const uintptr_t vmis = reinterpret_cast<uintptr_t>(video) & (in_dtype == VP_F32 ? 15 : 3);
  if (h->wpatch_v && H / P_ == 16 && W / P_ == 16 && Mp == M && vmis == 0) {
    const bf16_t* frames = static_cast<const bf16_t*>(video);
    if (in_dtype != VP_BF16) {
      VP_HIP(f.rec(PC_PATCHIFY, 0.0, dM * kreal * (in_es + dE), [&] {
        return video_to_bf16(video, in_dtype, static_cast<bf16_t*>(big), (int64_t)BT * H * W * 3, s); }));
      frames = static_cast<const bf16_t*>(big);
    }
    EpiArgs ep = epi_args(x, D, h->bpatch, nullptr, 0, sp_pos, Nsp, nullptr);
    ep.st_part = f.st_part; ep.st_rows = Mp;
    VP_HIP(f.rec(PC_GEMM_PATCH, 2.0 * dM * kreal * dD, gbytes(kreal, dD, dE, 0), [&] {
      return gemm_bf16_w4_video(fold ? EPI_POS_BF16_ST : EPI_POS_BF16, frames, P_, (const bf16_t*)h->wpatch_v, Mp, D,
                                ep, s); }));
  } else {
    if (Mp > M) VP_HIP(hipMemsetAsync(static_cast<char*>(big) + (size_t)M * h->kpad * es, 0,
                                      (size_t)(Mp - M) * h->kpad * es, s));
    VP_HIP(f.rec(PC_PATCHIFY, 0.0, dM * kreal * in_es + dM * h->kpad * dE, [&] {
      return patchify(video, in_dtype, big, bf, (int)BT, (int)H, (int)W, 3, P_, h->kpad, s); }));
    VP_HIP(f.rec(PC_GEMM_PATCH, 2.0 * dM * kreal * dD, gbytes(kreal, dD, dE, 0), [&] {
      return f.gemm(fold ? EPI_POS_BF16_ST : epi_pos, big, h->kpad, h->wpatch, D, x, D, h->bpatch, nullptr,
                    sp_pos, Nsp, nullptr); }));
  }
  if (fold) VP_HIP(f.finalize());
  // 2. spatial encoder over (b t) sequences of Nsp tokens
  if ((rc = f.run_stack(h->spatial, x, (int)BT, Nsp, ck.pad_btn, F, PC_ATTN_SPATIAL, ATT_VIDEO, bf, false))) return rc;
  return VP_OK;
}

// The temporal half (encoders.py:520-578) over the B clips of T frames of an open chunk.  frame_idx == nullptr
// (vp_forward): x is the chunk's own residual stream [B*T*Nsp][D], rows in place.  Else x holds the states of nframes frames and clip b's
// frame t is frame frame_idx[b*T + t] of them: one copy launch (gather_frames, vp_kernels.h) puts them into the
// chunk's residual stream, and from there on the launches are the same, kernel for kernel, which is what makes a
// window's output bitwise vp_forward's on the gathered clip.  (A LayerNorm that gathers as it loads would save that
// pass, but it is another kernel than layernorm's, and the compiler contracts multiplies and adds differently in the
// two: their outputs differ in the last bit of a few values.)
int temporal_half(vp_handle* h, Chunk& ck, const void* x, const int32_t* frame_idx, int64_t nframes, int64_t B,
                  int64_t T, const float* tpos, void* out, int out_dtype, void* spatial_out) {
  using namespace vp;
  int rc;
  hipStream_t s = ck.s;
  const vp_config& c = h->cfg;
  const bool bf = ck.bf;
  const int Nsp = ck.Nsp, M = ck.M;
  const int D = c.model_dim, F = c.mlp_dim;
  const size_t es = bf ? 2 : 4;
  Fwd& f = ck.f;
  void* x2 = ck.ws + ck.L.x2;
  float* ln_rs = bf && c.num_temporal_layers > 0 ? f.ln_rs : nullptr;
  const double dM = M, dD = D, dE = (double)es;
  const double ln_bytes = dM * dD * dE + dM * dD * dE;
  auto rec = [&](int cls, double flops, double bytes, auto&& fn) { return f.rec(cls, flops, bytes, fn); };
  if (frame_idx) {
    void* xg = ck.ws + ck.L.x;
    VP_HIP(rec(PC_MISC, 0.0, ln_bytes, [&] {
      return gather_frames(x, nframes, frame_idx, B * T, (int64_t)Nsp * D * (int64_t)es, xg, s); }));
    x = xg;
  }
  // 3. spatial_ln (+ optional spatial_features), transpose to (b n) t, + temporal pos-emb
  if (spatial_out)
    VP_HIP(rec(PC_LAYERNORM, 0.0, dM * dD * dE + dM * dD * (double)dtype_bytes(out_dtype), [&] {
      return layernorm(x, bf, M, D, h->sln_g, h->sln_b, spatial_out, out_dtype == VP_BF16, PERM_NONE, 1, 1, nullptr, s); }));
  VP_HIP(rec(PC_LAYERNORM, 0.0, ln_bytes, [&] {
    return layernorm(x, bf, M, D, h->sln_g, h->sln_b, x2, bf, PERM_BTN_TO_BNT, (int)T, Nsp, tpos, s, ln_rs); }));
  // 4. temporal encoder over (b n) sequences of T tokens
  if ((rc = f.run_stack(h->temporal, x2, (int)(B * Nsp), (int)T, ck.pad_bnt, F, PC_ATTN_TEMPORAL, ATT_VIDEO, bf, false)))
    return rc;
  // 5. temporal_ln and '(bn)td->b(tn)d'
  VP_HIP(rec(PC_LAYERNORM, 0.0, dM * dD * dE + dM * dD * (double)dtype_bytes(out_dtype), [&] {
    return layernorm(x2, bf, M, D, h->tln_g, h->tln_b, out, out_dtype == VP_BF16, PERM_BNT_TO_BTN, (int)T, Nsp, nullptr, s); }));
  return VP_OK;
}

// FactorizedEncoder.__call__ over one chunk of B clips (B <= chunk_clips: a workspace of about 4 GiB of
// FFN hidden activation); vp_forward below walks the batch chunk by chunk
int forward_chunk(vp_handle* h, const void* video, int in_dtype, int64_t B, int64_t T, int64_t H,
                  int64_t W, const float* frame_paddings, void* out, int out_dtype,
                  void* spatial_out, void* workspace, void* stream) {
  const float *sp_pos, *tpos;
  int rc;
  if ((rc = find_spatial_pos(h, H, W, &sp_pos)) || (rc = find_temporal_pos(h, T, &tpos))) return rc;
  Chunk ck;
  if ((rc = begin_chunk(h, B, T, H, W, frame_paddings, workspace, stream, &ck))) return rc;
  void* x = ck.ws + ck.L.x;
  if ((rc = spatial_half(h, ck, video, in_dtype, B * T, H, W, sp_pos, x))) return rc;
  return temporal_half(h, ck, x, nullptr, 0, B, T, tpos, out, out_dtype, spatial_out);
}

// vp_forward_spatial over one chunk of F frames: the chunk B = F, T = 1 of forward_chunk, stopped before spatial_ln
int spatial_chunk(vp_handle* h, const void* video, int in_dtype, int64_t F, int64_t H, int64_t W,
                  const float* frame_paddings, void* states_out, void* workspace, void* stream) {
  const float* sp_pos;
  int rc;
  if ((rc = find_spatial_pos(h, H, W, &sp_pos))) return rc;
  Chunk ck;
  if ((rc = begin_chunk(h, F, 1, H, W, frame_paddings, workspace, stream, &ck))) return rc;
  // F*N a multiple of the GEMM row tile: the residual stream lives in states_out from the patch embedding on
  const bool in_place = ck.Mp == ck.M;
  void* x = in_place ? states_out : ck.ws + ck.L.x;
  if ((rc = spatial_half(h, ck, video, in_dtype, F, H, W, sp_pos, x))) return rc;
  if (!in_place)
    VP_HIP(hipMemcpyAsync(states_out, x, (size_t)ck.M * h->cfg.model_dim * (ck.bf ? 2 : 4), hipMemcpyDeviceToDevice, ck.s));
  return VP_OK;
}

// vp_forward_temporal over one chunk of Wn windows
int temporal_chunk(vp_handle* h, const void* states, int64_t F, const int32_t* frame_idx, int64_t Wn, int64_t T,
                   int64_t H, int64_t W, const float* frame_paddings, void* out, int out_dtype, void* spatial_out,
                   void* workspace, void* stream) {
  const float* tpos;
  int rc;
  if ((rc = find_temporal_pos(h, T, &tpos))) return rc;
  Chunk ck;
  if ((rc = begin_chunk(h, Wn, T, H, W, frame_paddings, workspace, stream, &ck))) return rc;
  return temporal_half(h, ck, states, frame_idx, F, Wn, T, tpos, out, out_dtype, spatial_out);
}

}  // namespace

extern "C" {

int vp_forward(vp_handle* h, const void* video, int in_dtype, int64_t B, int64_t T, int64_t H,
               int64_t W, const float* frame_paddings, void* out, int out_dtype,
               void* spatial_out, void* workspace, size_t ws_bytes, void* stream) {
  if (!h || !video || !out || !workspace) return fail(VP_EINVAL, "null argument");
  if (!h->finalized) return fail(VP_ESTATE, "vp_finalize has not been called");
  size_t need = 0, out_clip = 0;
  int rc = check_dtypes(in_dtype, out_dtype, false, h->cfg.fprop_dtype);
  if (rc || (rc = vp_workspace_bytes(h, B, T, H, W, &need)) ||
      (rc = check_workspace(h, T, H, W, ws_bytes, need, out_dtype, &out_clip)))
    return rc;
  const size_t in_clip = video_clip_bytes(T, H, W, in_dtype);
  return for_each_chunk(h, B, T, H, W, [&](int64_t b0, int64_t nb) {
    return forward_chunk(h, advance(video, b0 * in_clip), in_dtype, nb, T, H, W, advance(frame_paddings, b0 * T * 4),
                         advance(out, b0 * out_clip), out_dtype, advance(spatial_out, b0 * out_clip), workspace, stream);
  });
}

int vp_spatial_workspace_bytes(const vp_handle* h, int64_t F, int64_t H, int64_t W, size_t* bytes) {
  return vp_workspace_bytes(h, F, 1, H, W, bytes);
}

int vp_forward_spatial(vp_handle* h, const void* video, int in_dtype, int64_t F, int64_t H, int64_t W,
                       const float* frame_paddings, void* states_out, void* workspace, size_t ws_bytes,
                       void* stream) {
  if (!h || !video || !states_out || !workspace) return fail(VP_EINVAL, "null argument");
  if (!h->finalized) return fail(VP_ESTATE, "vp_finalize has not been called");
  size_t need = 0, st_frame = 0;
  const int fd = h->cfg.fprop_dtype;
  int rc = check_dtypes(in_dtype, fd, false, fd);
  if (rc || (rc = vp_spatial_workspace_bytes(h, F, H, W, &need)) ||
      (rc = check_workspace(h, 1, H, W, ws_bytes, need, fd, &st_frame)))
    return rc;
  const size_t in_frame = video_clip_bytes(1, H, W, in_dtype);
  return for_each_chunk(h, F, 1, H, W, [&](int64_t f0, int64_t nf) {
    return spatial_chunk(h, advance(video, f0 * in_frame), in_dtype, nf, H, W, advance(frame_paddings, f0 * 4),
                         advance(states_out, f0 * st_frame), workspace, stream);
  });
}

int vp_temporal_workspace_bytes(const vp_handle* h, int64_t Wn, int64_t T, int64_t H, int64_t W, size_t* bytes) {
  return vp_workspace_bytes(h, Wn, T, H, W, bytes);
}

int vp_forward_temporal(vp_handle* h, const void* states, int64_t F, const int32_t* frame_idx, int64_t Wn,
                        int64_t T, int64_t H, int64_t W, const float* frame_paddings, void* out, int out_dtype,
                        void* spatial_out, void* workspace, size_t ws_bytes, void* stream) {
  if (!h || !states || !frame_idx || !out || !workspace) return fail(VP_EINVAL, "null argument");
  if (!h->finalized) return fail(VP_ESTATE, "vp_finalize has not been called");
  size_t need = 0, out_clip = 0;
  int rc = check_dtypes(h->cfg.fprop_dtype, out_dtype, false, h->cfg.fprop_dtype);
  if (rc || (rc = vp_temporal_workspace_bytes(h, Wn, T, H, W, &need)) ||
      (rc = check_workspace(h, T, H, W, ws_bytes, need, out_dtype, &out_clip)))
    return rc;
  const int64_t P = h->cfg.patch_size;
  if (F < 1 || F * (H / P) * (W / P) > 0x7fffffff)
    return fail(VP_EINVAL, "states must hold 1 <= F frames and fewer than 2^31 rows");
  return for_each_chunk(h, Wn, T, H, W, [&](int64_t w0, int64_t nw) {
    return temporal_chunk(h, states, F, frame_idx + w0 * T, nw, T, H, W, advance(frame_paddings, w0 * T * 4),
                          advance(out, w0 * out_clip), out_dtype, advance(spatial_out, w0 * out_clip), workspace, stream);
  });
}

// ----------------------------------- profiling ----------------------------------------

int vp_profile_enable(vp_handle* h, int capacity) {
  if (!h || capacity < 0) return fail(VP_EINVAL, "bad argument");
  VP_HIP(hipSetDevice(h->device));
  Profiler& p = h->prof;
  for (auto& e : p.ev) hipEventDestroy(e);
  p.ev.clear();
  p.cap = 0;
  p.used = 0;
  p.ev.resize((size_t)capacity * 2);
  for (auto& e : p.ev) VP_HIP(hipEventCreate(&e));
  p.cls.assign(capacity, PC_MISC);
  p.flops.assign(capacity, 0.0);
  p.bytes.assign(capacity, 0.0);
  p.cap = capacity;
  return VP_OK;
}

int vp_profile_set_mask(vp_handle* h, uint32_t class_mask) {
  if (!h) return fail(VP_EINVAL, "null handle");
  h->prof.mask = class_mask;
  return VP_OK;
}

int vp_profile_read(vp_handle* h, int nclass, double* ms, double* flops, double* bytes,
                    int64_t* launches) {
  if (!h || nclass < PC_COUNT || !ms || !flops || !bytes || !launches)
    return fail(VP_EINVAL, "bad argument");
  for (int c = 0; c < nclass; ++c) { ms[c] = 0; flops[c] = 0; bytes[c] = 0; launches[c] = 0; }
  Profiler& p = h->prof;
  if (p.used > 0) VP_HIP(hipEventSynchronize(p.ev[2 * p.used - 1]));
  for (int i = 0; i < p.used; ++i) {
    float t = 0.f;
    VP_HIP(hipEventElapsedTime(&t, p.ev[2 * i], p.ev[2 * i + 1]));
    ms[p.cls[i]] += t;
    flops[p.cls[i]] += p.flops[i];
    bytes[p.cls[i]] += p.bytes[i];
    launches[p.cls[i]] += 1;
  }
  p.used = 0;
  return VP_OK;
}

int vp_profile_class_name(int cls, const char** name) {
  if (cls < 0 || cls >= PC_COUNT || !name) return fail(VP_EINVAL, "bad class");
  *name = kProfNames[cls];
  return VP_OK;
}

int vp_profile_class_count(void) { return PC_COUNT; }

int vp_profile_kernel_name(vp_handle* h, int cls, const char** name) {
  if (!h || cls < 0 || cls >= PC_COUNT || !name) return fail(VP_EINVAL, "bad argument");
  Profiler& p = h->prof;
  p.kname[cls].clear();
  if (p.kfn[cls]) {
    const char* raw = hipKernelNameRefByPtr(p.kfn[cls], nullptr);
    if (raw) {
      int st = 0;
      char* dm = abi::__cxa_demangle(raw, nullptr, nullptr, &st);
      p.kname[cls] = (st == 0 && dm) ? dm : raw;
      std::free(dm);
    }
  }
  *name = p.kname[cls].c_str();
  return VP_OK;
}

// ----------------------------------- op level -----------------------------------------

int vp_op_gemm(int precision, int epilogue, const void* A, int64_t lda, const void* W, int64_t ldw,
               int64_t M, int64_t N, int64_t K, void* out, int64_t ldo, const float* bias,
               const void* resid, int64_t ldr, const float* pos, int64_t pos_rows,
               const float* rowpad, void* stream) {
  using namespace vp;
  if (!A || !W || !out || !bias) return fail(VP_EINVAL, "null argument");
  if (epilogue < 0 || epilogue > 7) return fail(VP_EINVAL, "bad epilogue");
  const bool needs_resid = epilogue == EPI_RESID_F32 || epilogue == EPI_RESID_FFN ||
                           epilogue == EPI_RESID_BF16 || epilogue == EPI_RESID_FFN_BF16;
  if (needs_resid && !resid) return fail(VP_EINVAL, "resid required");
  if ((epilogue == EPI_POS_F32 || epilogue == EPI_POS_BF16) && (!pos || pos_rows < 1))
    return fail(VP_EINVAL, "pos required");
  if (precision == VP_F32 && epilogue > 4) return fail(VP_EINVAL, "bf16 residual epilogues need precision VP_BF16");
  const EpiArgs ep = epi_args(out, ldo, bias, resid, ldr, pos, pos_rows, rowpad);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (precision == VP_BF16) {
    const char* e = gemm_bf16_check((int)M, (int)N, (int)K, lda, ldw);
    if (e) return fail(VP_EINVAL, e);
    VP_HIP(gemm_bf16_auto(epilogue, (const bf16_t*)A, lda, (const bf16_t*)W, ldw, (int)M, (int)N, (int)K, ep, s));
  } else if (precision == VP_F32) {
    const char* e = gemm_f32_check((int)M, (int)N, (int)K, lda, ldw);
    if (e) return fail(VP_EINVAL, e);
    VP_HIP(gemm_f32(epilogue, (const float*)A, lda, (const float*)W, ldw, (int)M, (int)N, (int)K, ep, s));
  } else {
    return fail(VP_EINVAL, "bad precision");
  }
  return VP_OK;
}

// Not in the public header: one named bf16 GEMM kernel (4: gemm_bf16_w4, 8: gemm_bf16) with any
// epilogue, for kernel A/B tests (tests/test_gpu_kernels.py) and tools/gemm_bench.py.
int vp_dev_gemm_kernel(int which, int epi, const void* A, const void* W, int64_t M, int64_t N,
                       int64_t K, void* out, const float* bias, const void* resid, const float* pos,
                       int64_t pos_rows, const float* rowpad, void* stream) {
  using namespace vp;
  const char* e = which == 1 ? nullptr : (which >= 32 && which <= 34) ? gemm_f32_check((int)M, (int)N, (int)K, K, K)
                                                                       : gemm_bf16_check((int)M, (int)N, (int)K, K, K);
  if (e) return fail(VP_EINVAL, e);
  const EpiArgs ep = epi_args(out, N, bias, resid, N, pos, pos_rows > 0 ? pos_rows : 1, rowpad);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (which == 4)
    VP_HIP(gemm_bf16_w4(epi, (const bf16_t*)A, K, (const bf16_t*)W, K, (int)M, (int)N, (int)K, ep, s));
  else if (which == 8)
    VP_HIP(gemm_bf16(epi, (const bf16_t*)A, K, (const bf16_t*)W, K, (int)M, (int)N, (int)K, ep, s));
  else if (which == 1) {  // the small-M kernel (text tower)
    if (!gemm_bf16_small_ok(epi, (int)M, (int)N, (int)K, K, K))
      return fail(VP_EINVAL, "small-M GEMM: epilogue 0, 1, 2, 4, 5, 7 or 13 and K % 256 == 0");
    VP_HIP(gemm_bf16_small(epi, (const bf16_t*)A, K, (const bf16_t*)W, K, (int)M, (int)N, (int)K, ep, s));
  } else if (which >= 32 && which <= 34) {  // fp32: round 1's 16x16x4 kernel (32) / the 32x32x2 kernel (33) / with two chains (34)
    VP_HIP(gemm_f32(epi, (const float*)A, K, (const float*)W, K, (int)M, (int)N, (int)K, ep, s, which - 31));
  } else
    return fail(VP_EINVAL, "which must be 1, 4, 8, 32, 33 or 34");
  return VP_OK;
}

// Not in the public header: the GEMM-folded LayerNorm pieces (tests/test_gpu_kernels.py).
// vp_dev_gemm_ln: EPI_BF16_LN / EPI_GELU_BF16_LN with (rstd, -mean*rstd) rows ln_rs and column
// sums ln_c, or EPI_*_ST writing partial row statistics to st_part ([N/128][M][2]); EPI_*_BLK: the FFN
// pair over the row-blocked hidden activation (vp_kernels.h).
int vp_dev_gemm_ln(int epi, const void* A, const void* W, int64_t M, int64_t N, int64_t K, void* out,
                   const float* bias, const void* resid, const float* pos, int64_t pos_rows,
                   const float* rowpad, const float* ln_rs, const float* ln_c, float* st_part,
                   void* stream) {
  using namespace vp;
  if (!((epi >= EPI_BF16_LN && epi <= EPI_POS_BF16_ST) || (epi >= EPI_GELU_BF16_LN_BLK && epi <= EPI_BF16_LN_BLK)))
    return fail(VP_EINVAL, "epilogue must be 8..12 or 16..19");
  const char* e = gemm_bf16_check((int)M, (int)N, (int)K, K, K);
  if (e) return fail(VP_EINVAL, e);
  EpiArgs ep = epi_args(out, N, bias, resid, N, pos, pos_rows > 0 ? pos_rows : 1, rowpad);
  ep.ln_rs = ln_rs; ep.ln_c = ln_c; ep.st_part = st_part; ep.st_rows = M;
  VP_HIP(gemm_bf16_w4(epi, (const bf16_t*)A, K, (const bf16_t*)W, K, (int)M, (int)N, (int)K, ep,
                      static_cast<hipStream_t>(stream)));
  return VP_OK;
}

// Not in the public header: the spatial attention (S = 256) over q|k|v in the row-blocked layout of
// EPI_BF16_LN_BLK (tests: bitwise the row-major path).
int vp_dev_attention_spatial_blk(const void* qkv, void* o, int64_t num_seq, int64_t heads, float cap,
                                 const float* key_pad, void* stream) {
  using namespace vp;
  if (!qkv || !o || num_seq < 1 || heads < 1) return fail(VP_EINVAL, "bad argument");
  VP_HIP(attention_spatial_bf16((const bf16_t*)qkv, (bf16_t*)o, (int)num_seq, (int)heads, cap, key_pad,
                                static_cast<hipStream_t>(stream), true));
  return VP_OK;
}

// Not in the public header: the two launches of the fused temporal attention (EPI_QK_TATTN_LN,
// EPI_V_TATTN_LN; vp_kernels.h) for kernel-level tests (tests/test_gpu_kernels.py).  which = 0: A = x
// [M][K], W = the [q_h | k_h]-regrouped LN-folded rows [2K][K] -> P (512 B per (sequence, head));
// which = 1: W = the v rows [K][K], p = P -> O [M][K].  K = heads * 64, M % 256 == 0.
int vp_dev_gemm_tattn(int which, const void* A, const void* W, int64_t M, int64_t K, void* out, const float* bias,
                      const float* ln_rs, const float* ln_c, const void* p, int64_t heads, float cap, void* stream) {
  using namespace vp;
  if (which < 0 || which > 1 || !A || !W || !out || !bias || !ln_rs || !ln_c || (which == 1 && !p))
    return fail(VP_EINVAL, "bad argument");
  if (K != heads * 64 || M % 256 || !vpi::fast_cap(cap)) return fail(VP_EINVAL, "needs K = heads*64, M % 256, 0 < cap <= 50");
  const int64_t N = which == 0 ? 2 * K : K;
  const char* e = gemm_bf16_check((int)M, (int)N, (int)K, K, K);
  if (e) return fail(VP_EINVAL, e);
  EpiArgs ep = epi_args(out, K, bias, p, 0, nullptr, 1, nullptr);
  ep.ln_rs = ln_rs; ep.ln_c = ln_c;
  set_tattn_cap(ep, cap, (int)heads);
  VP_HIP(gemm_bf16_w4(which == 0 ? EPI_QK_TATTN_LN : EPI_V_TATTN_LN, (const bf16_t*)A, K, (const bf16_t*)W, K, (int)M,
                      (int)N, (int)K, ep, static_cast<hipStream_t>(stream)));
  return VP_OK;
}

// Not in the public header: the fused patch embedding (gemm_bf16_w4_video, EPI_POS_BF16) for kernel
// tests: bf16 frames [frames][16P][16P][3], wv [N][video_patch_k(P)] in the frames' chunk order
// (vp_kernels.h), pos [256][N] fp32 -> out [frames*256][N] bf16.
int vp_dev_patch_embed(const void* video, int64_t frames, int64_t P, const void* wv, int64_t N, const float* bias,
                       const float* pos, void* out, void* stream) {
  using namespace vp;
  if (!video || !wv || !bias || !pos || !out || frames < 1 || N % 256) return fail(VP_EINVAL, "bad argument");
  if (!video_patch_ok((int)P)) return fail(VP_EINVAL, "fused patch embedding needs an even patch size, 4 <= P <= 21");
  const EpiArgs ep = epi_args(out, N, bias, nullptr, 0, pos, 256, nullptr);
  VP_HIP(gemm_bf16_w4_video(EPI_POS_BF16, (const bf16_t*)video, (int)P, (const bf16_t*)wv, (int)(frames * 256), (int)N,
                            ep, static_cast<hipStream_t>(stream)));
  return VP_OK;
}

// which = 0: ln_stats_finalize(src = st_part [D/128][M][2]); 1: ln_row_stats(src = bf16 [M][D])
int vp_dev_ln_stats(int which, const void* src, int64_t M, int64_t D, float* ln_rs, void* stream) {
  using namespace vp;
  if (D % 128 || D < 128) return fail(VP_EINVAL, "D must be a multiple of 128");
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (which == 0) VP_HIP(ln_stats_finalize((const float*)src, (int)(D / 128), M, ln_rs, s));
  else VP_HIP(ln_row_stats((const bf16_t*)src, M, (int)D, ln_rs, s));
  return VP_OK;
}

// Not in the public header: the kernel (vpi::AttnKernel) choose_attention gives a stack of `kind` (vpi::AttnKind;
// negative: whatever vp_op_attention makes of S and key paddings), or -1 for a bad argument.  No GPU call.
int vp_dev_attention_choice_dh(int kind, int precision, int64_t S, float cap, int has_key_pad, int64_t dim_per_head);

int vp_dev_attention_choice(int kind, int precision, int64_t S, float cap, int has_key_pad) {
  return vp_dev_attention_choice_dh(kind, precision, S, cap, has_key_pad, 64);
}

// ... for heads of dim_per_head values: -2 where no kernel takes that width in that precision (vp_op_attention_dh's
// VP_ENOTSUP)
int vp_dev_attention_choice_dh(int kind, int precision, int64_t S, float cap, int has_key_pad, int64_t dim_per_head) {
  if (kind > ATT_TEXT || (precision != VP_F32 && precision != VP_BF16) || S < 1) return -1;
  if (!supported_dh(precision == VP_BF16, dim_per_head)) return -2;
  if (kind < 0) kind = op_attention_kind(S, has_key_pad != 0);
  return choose_attention(kind, precision == VP_BF16, S, cap, has_key_pad != 0, (int)dim_per_head);
}

namespace {
int check_op_dh(int precision, int64_t dim_per_head) {
  if (supported_dh(precision == VP_BF16, dim_per_head)) return VP_OK;
  return fail(VP_ENOTSUP, precision == VP_BF16 ? "attention: bfloat16 runs dim_per_head 64 only"
                                               : "attention: dim_per_head must be 64 or 88");
}
}  // namespace

int vp_op_attention(int precision, const void* qkv, void* o, int64_t num_seq, int64_t S,
                    int64_t heads, float cap, const float* key_pad, void* stream) {
  return vp_op_attention_dh(precision, qkv, o, num_seq, S, heads, 64, cap, key_pad, stream);
}

int vp_op_attention_dh(int precision, const void* qkv, void* o, int64_t num_seq, int64_t S, int64_t heads,
                       int64_t dim_per_head, float cap, const float* key_pad, void* stream) {
  if (!qkv || !o || num_seq < 1 || heads < 1) return fail(VP_EINVAL, "bad argument");
  if (precision != VP_F32 && precision != VP_BF16) return fail(VP_EINVAL, "bad precision");
  if (S < 1) return fail(VP_EINVAL, "bad S");
  if (int rc = check_op_dh(precision, dim_per_head)) return rc;
  VP_HIP(launch_attention(op_attention_kind(S, key_pad != nullptr), precision == VP_BF16, qkv, o, (int)num_seq, (int)S,
                          (int)heads, cap, key_pad, 0, false, static_cast<hipStream_t>(stream), (int)dim_per_head));
  return VP_OK;
}

int vp_op_attention_masked(int precision, const void* qkv, void* o, int64_t num_seq, int64_t S,
                           int64_t heads, float cap, const float* key_pad, int causal, void* stream) {
  return vp_op_attention_masked_dh(precision, qkv, o, num_seq, S, heads, 64, cap, key_pad, causal, stream);
}

int vp_op_attention_masked_dh(int precision, const void* qkv, void* o, int64_t num_seq, int64_t S, int64_t heads,
                              int64_t dim_per_head, float cap, const float* key_pad, int causal, void* stream) {
  if (!qkv || !o || num_seq < 1 || heads < 1 || S < 1) return fail(VP_EINVAL, "bad argument");
  if (precision != VP_F32 && precision != VP_BF16) return fail(VP_EINVAL, "bad precision");
  if (int rc = check_op_dh(precision, dim_per_head)) return rc;
  VP_HIP(launch_attention(ATT_TEXT, precision == VP_BF16, qkv, o, (int)num_seq, (int)S, (int)heads, cap, key_pad,
                          causal ? 1 : 0, false, static_cast<hipStream_t>(stream), (int)dim_per_head));
  return VP_OK;
}

int vp_op_similarity(const float* video_emb, const float* text_emb, int64_t B, int64_t Q, int64_t D,
                     float* out, void* stream) {
  if (!video_emb || !text_emb || !out || B < 1 || Q < 1 || D < 1) return fail(VP_EINVAL, "bad argument");
  VP_HIP(vp::similarity(video_emb, text_emb, (int)B, (int)Q, (int)D, out, static_cast<hipStream_t>(stream)));
  return VP_OK;
}

int vp_op_layernorm(const void* x, int in_dtype, int64_t rows, int64_t D, const float* gamma,
                    const float* beta, void* out, int out_dtype, int perm, int64_t T, int64_t Nsp,
                    const float* add, void* stream) {
  using namespace vp;
  if (!x || !gamma || !beta || !out) return fail(VP_EINVAL, "null argument");
  if ((in_dtype != VP_F32 && in_dtype != VP_BF16) || (out_dtype != VP_F32 && out_dtype != VP_BF16))
    return fail(VP_EINVAL, "bad dtype");
  if (perm && (T < 1 || Nsp < 1 || rows % (T * Nsp))) return fail(VP_EINVAL, "bad permutation geometry");
  hipError_t e = layernorm(x, in_dtype == VP_BF16, (int)rows, (int)D, gamma, beta, out, out_dtype == VP_BF16,
                           perm, (int)T, (int)Nsp, add, static_cast<hipStream_t>(stream));
  if (e == hipErrorInvalidValue) return fail(VP_ENOTSUP, "layernorm: D must be 128*k, k in {1..12, 16}");
  VP_HIP(e);
  return VP_OK;
}

// Not in the public header: gather_frames (vp_kernels.h), the one launch vp_forward_temporal adds to vp_forward's, on
// its own for kernel tests (tests/test_gpu_windows.py): x = states [F] of frame_bytes each, frame_idx device int32
// [nslots] (clamped to [0, F - 1] by the kernel) -> out [nslots] frames.
int vp_dev_gather_frames(const void* x, int64_t F, const int32_t* frame_idx, int64_t nslots, int64_t frame_bytes,
                         void* out, void* stream) {
  if (!x || !frame_idx || !out) return fail(VP_EINVAL, "null argument");
  hipError_t e = vp::gather_frames(x, F, frame_idx, nslots, frame_bytes, out, static_cast<hipStream_t>(stream));
  if (e == hipErrorInvalidValue)
    return fail(VP_EINVAL, "gather_frames: 1 <= F, nslots < 2^31, frames of 16 k bytes (k <= 2^26), 16-byte aligned");
  VP_HIP(e);
  return VP_OK;
}

// Not in the public header: the two launches with which vp_forward_temporal enters the temporal half, gather_frames
// into `scratch` ([rows][D] in x's dtype) and then layernorm on it, for kernel tests (tests/test_gpu_windows.py):
// x = states [F][Nsp][D], frame_idx device int32 [rows / Nsp], rows = Wn*T*Nsp; perm 0 or 1; add (nullable) fp32
// [T][D] by the output row's t; out_rs (nullable) [rows][2], (rstd, -mean*rstd) of each stored row by output row.
int vp_dev_layernorm_gather(const void* x, int in_dtype, int64_t F, const int32_t* frame_idx, int64_t rows, int64_t D,
                            const float* gamma, const float* beta, void* out, int out_dtype, int perm, int64_t T,
                            int64_t Nsp, const float* add, float* out_rs, void* scratch, void* stream) {
  using namespace vp;
  if (!x || !frame_idx || !gamma || !beta || !out || !scratch) return fail(VP_EINVAL, "null argument");
  if ((in_dtype != VP_F32 && in_dtype != VP_BF16) || (out_dtype != VP_F32 && out_dtype != VP_BF16))
    return fail(VP_EINVAL, "bad dtype");
  if (F < 1 || T < 1 || Nsp < 1 || rows < 1 || rows > 0x7fffffff || rows % Nsp ||
      (perm != PERM_NONE && perm != PERM_BTN_TO_BNT) || (perm && rows % (T * Nsp)))
    return fail(VP_EINVAL, "bad gather geometry");
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipError_t e = gather_frames(x, F, frame_idx, rows / Nsp, Nsp * D * (int64_t)dtype_bytes(in_dtype), scratch, s);
  if (e == hipErrorInvalidValue) return fail(VP_EINVAL, "gather_frames: frames of 16 k bytes, 16-byte aligned");
  VP_HIP(e);
  e = layernorm(scratch, in_dtype == VP_BF16, (int)rows, (int)D, gamma, beta, out, out_dtype == VP_BF16, perm, (int)T,
                (int)Nsp, add, s, out_rs);
  if (e == hipErrorInvalidValue) return fail(VP_ENOTSUP, "layernorm: D must be 128*k, k in {1..12, 16}");
  VP_HIP(e);
  return VP_OK;
}

int vp_op_patchify(const void* video, int in_dtype, void* patches, int out_dtype, int64_t BT,
                   int64_t H, int64_t W, int64_t C, int64_t P, int64_t kpad, void* stream) {
  using namespace vp;
  if (!video || !patches || P <= 0) return fail(VP_EINVAL, "bad argument");
  if (H % P || W % P) return fail(VP_EINVAL, patch_size_message(H, W, P));
  if (kpad % 8 || kpad < P * P * C) return fail(VP_EINVAL, "kpad must be >= P*P*C and a multiple of 8");
  if (in_dtype != VP_F32 && in_dtype != VP_BF16 && in_dtype != VP_U8) return fail(VP_EINVAL, "bad dtype");
  VP_HIP(patchify(video, in_dtype, patches, out_dtype == VP_BF16, (int)BT, (int)H, (int)W,
                  (int)C, (int)P, (int)kpad, static_cast<hipStream_t>(stream)));
  return VP_OK;
}

int vp_op_preprocess_frames(const uint8_t* src, int64_t N, int64_t H, int64_t W, int64_t row_stride,
                            int64_t frame_stride, const int32_t* frame_idx, int64_t F, int mode,
                            int swap_rb, int64_t S, uint8_t* dst, void* stream) {
  using namespace vp;
  if (!src || !dst) return fail(VP_EINVAL, "null argument");
  if (N < 1 || H < 1 || W < 1 || F < 1 || S < 1) return fail(VP_EINVAL, "N, H, W, F and S must be at least 1");
  if (mode != VP_RESIZE_CENTER_CROP && mode != VP_RESIZE_STRETCH)
    return fail(VP_EINVAL, "Unknown resize_mode: " + std::to_string(mode));
  if (H >= (1 << 24) || W >= (1 << 24) || S > 16384 || N > INT32_MAX || F > INT32_MAX)
    return fail(VP_EINVAL, "frame geometry out of range (H, W < 2^24, S <= 16384, N, F < 2^31)");
  if (row_stride < 3 * W) return fail(VP_EINVAL, "row_stride must be at least 3*W bytes");
  if (frame_stride < H * row_stride) return fail(VP_EINVAL, "frame_stride must be at least H*row_stride bytes");
  if (!frame_idx && F > N)
    return fail(VP_EINVAL, "Video has only " + std::to_string(N) + " frames, but " + std::to_string(F) + " requested");
  int64_t nh, nw, y0, x0;
  if (const char* why = preprocess_geometry(H, W, S, mode, &nh, &nw, &y0, &x0)) return fail(VP_EINVAL, why);
  hipError_t e = preprocess_frames(src, N, H, W, row_stride, frame_stride, frame_idx, F, mode, swap_rb, S, dst,
                                   static_cast<hipStream_t>(stream));
  if (e == hipErrorInvalidValue) return fail(VP_EINVAL, "too many output pixels for one launch");
  VP_HIP(e);
  return VP_OK;
}

int vp_dev_yuv_coefficients(int matrix, int range, int bit_depth, int32_t out[11]) {
  if (!out) return fail(VP_EINVAL, "null argument");
  if (const char* why = vp::yuv_coefficients(matrix, range, bit_depth, out)) return fail(VP_EINVAL, why);
  return VP_OK;
}

namespace {
// The checks vp_op_preprocess_yuv and vp_op_preprocess_yuv_views share, in the former's order: the planes of a
// vp_yuv_frames for N frames of H x W, F output frames of S x S (mode: the resize mode where the call has one)
// -> the kernel's planes and coefficient table, or the error
int yuv_source(const vp_yuv_frames* src, int64_t N, int64_t H, int64_t W, int64_t F, int64_t S, const int* mode,
               const uint8_t* dst, vp::YuvPlanes& pl, int32_t coef[11]) {
  using namespace vp;
  if (!src || !src->plane[0] || !dst) return fail(VP_EINVAL, "null argument");
  const int fmt = src->format;
  if (fmt != VP_YUV_NV12 && fmt != VP_YUV_I420 && fmt != VP_YUV_P010)
    return fail(VP_EINVAL, "Unknown pixel format: " + std::to_string(fmt));
  if (const char* why = yuv_coefficients(src->matrix, src->range, fmt == VP_YUV_P010 ? 10 : 8, coef))
    return fail(VP_EINVAL, why);
  const int planes = fmt == VP_YUV_I420 ? 3 : 2;
  for (int p = 1; p < planes; ++p)
    if (!src->plane[p]) return fail(VP_EINVAL, "missing chroma plane");
  if (N < 1 || H < 1 || W < 1 || F < 1 || S < 1) return fail(VP_EINVAL, "N, H, W, F and S must be at least 1");
  if (mode && *mode != VP_RESIZE_CENTER_CROP && *mode != VP_RESIZE_STRETCH)
    return fail(VP_EINVAL, "Unknown resize_mode: " + std::to_string(*mode));
  if (H >= (1 << 24) || W >= (1 << 24) || S > 16384 || N > INT32_MAX || F > INT32_MAX)
    return fail(VP_EINVAL, "frame geometry out of range (H, W < 2^24, S <= 16384, N, F < 2^31)");
  const int64_t sample = fmt == VP_YUV_P010 ? 2 : 1, ch = (H + 1) / 2, cw = (W + 1) / 2;
  pl.format = fmt;
  for (int p = 0; p < 3; ++p) {
    pl.plane[p] = p < planes ? src->plane[p] : nullptr;
    pl.row_stride[p] = p < planes ? src->row_stride[p] : 0;
    pl.frame_stride[p] = p < planes ? src->frame_stride[p] : 0;
    if (p >= planes) continue;
    const int64_t rows = p ? ch : H, row_bytes = (p == 0 ? W : fmt == VP_YUV_I420 ? cw : 2 * cw) * sample;
    if (pl.row_stride[p] < row_bytes)
      return fail(VP_EINVAL, "row_stride[" + std::to_string(p) + "] must be at least " + std::to_string(row_bytes) + " bytes");
    if (pl.frame_stride[p] < rows * pl.row_stride[p])
      return fail(VP_EINVAL, "frame_stride[" + std::to_string(p) + "] must be at least its rows times row_stride bytes");
    if (fmt == VP_YUV_P010 && (((uintptr_t)pl.plane[p] | (uintptr_t)pl.row_stride[p] | (uintptr_t)pl.frame_stride[p]) & 1))
      return fail(VP_EINVAL, "P010 plane bases and strides must be multiples of 2 bytes");
  }
  return VP_OK;
}

// V views of T frames each: the arguments the two view calls add
int check_views(const int32_t* views, int64_t V, int64_t T) {
  if (!views) return fail(VP_EINVAL, "null argument");
  if (V < 1 || T < 1) return fail(VP_EINVAL, "V and T must be at least 1");
  if (V > INT32_MAX || T > INT32_MAX || V * T > INT32_MAX)
    return fail(VP_EINVAL, "frame geometry out of range (V * T < 2^31)");
  return VP_OK;
}

// without frame_idx, frame t of every view is source frame t
int check_view_frames(const int32_t* frame_idx, int64_t N, int64_t T) {
  if (!frame_idx && T > N)
    return fail(VP_EINVAL, "Video has only " + std::to_string(N) + " frames, but " + std::to_string(T) + " requested");
  return VP_OK;
}
}  // namespace

int vp_op_preprocess_views(const uint8_t* src, int64_t N, int64_t H, int64_t W, int64_t row_stride,
                           int64_t frame_stride, const int32_t* frame_idx, const int32_t* views, int64_t V,
                           int64_t T, int swap_rb, int64_t S, uint8_t* dst, void* stream) {
  using namespace vp;
  if (!src || !dst) return fail(VP_EINVAL, "null argument");
  if (int rc = check_views(views, V, T)) return rc;
  if (N < 1 || H < 1 || W < 1 || S < 1) return fail(VP_EINVAL, "N, H, W and S must be at least 1");
  if (H >= (1 << 24) || W >= (1 << 24) || S > 16384 || N > INT32_MAX)
    return fail(VP_EINVAL, "frame geometry out of range (H, W < 2^24, S <= 16384, N < 2^31)");
  if (row_stride < 3 * W) return fail(VP_EINVAL, "row_stride must be at least 3*W bytes");
  if (frame_stride < H * row_stride) return fail(VP_EINVAL, "frame_stride must be at least H*row_stride bytes");
  if (int rc = check_view_frames(frame_idx, N, T)) return rc;
  hipError_t e = preprocess_views(src, N, H, W, row_stride, frame_stride, frame_idx, views, V, T, swap_rb, S, dst,
                                  static_cast<hipStream_t>(stream));
  if (e == hipErrorInvalidValue) return fail(VP_EINVAL, "too many output pixels for one launch");
  VP_HIP(e);
  return VP_OK;
}

int vp_op_preprocess_yuv_views(const vp_yuv_frames* src, int64_t N, int64_t H, int64_t W, const int32_t* frame_idx,
                               const int32_t* views, int64_t V, int64_t T, int64_t S, uint8_t* dst, void* stream) {
  using namespace vp;
  if (int rc = check_views(views, V, T)) return rc;
  YuvPlanes pl;
  int32_t coef[11];
  if (int rc = yuv_source(src, N, H, W, V * T, S, nullptr, dst, pl, coef)) return rc;
  if (int rc = check_view_frames(frame_idx, N, T)) return rc;
  hipError_t e = preprocess_yuv_views(pl, coef, N, H, W, frame_idx, views, V, T, S, dst, static_cast<hipStream_t>(stream));
  if (e == hipErrorInvalidValue) return fail(VP_EINVAL, "too many output pixels for one launch");
  VP_HIP(e);
  return VP_OK;
}

int vp_op_preprocess_yuv(const vp_yuv_frames* src, int64_t N, int64_t H, int64_t W, const int32_t* frame_idx,
                         int64_t F, int mode, int64_t S, uint8_t* dst, void* stream) {
  using namespace vp;
  YuvPlanes pl;
  int32_t coef[11];
  if (int rc = yuv_source(src, N, H, W, F, S, &mode, dst, pl, coef)) return rc;
  if (!frame_idx && F > N)
    return fail(VP_EINVAL, "Video has only " + std::to_string(N) + " frames, but " + std::to_string(F) + " requested");
  int64_t nh, nw, y0, x0;
  if (const char* why = preprocess_geometry(H, W, S, mode, &nh, &nw, &y0, &x0)) return fail(VP_EINVAL, why);
  hipError_t e = preprocess_yuv(pl, coef, N, H, W, frame_idx, F, mode, S, dst, static_cast<hipStream_t>(stream));
  if (e == hipErrorInvalidValue) return fail(VP_EINVAL, "too many output pixels for one launch");
  VP_HIP(e);
  return VP_OK;
}

int vp_op_pool_l2(const void* emb, int dtype, int64_t B, int64_t L, int64_t D, float* out,
                  void* stream) {
  using namespace vp;
  if (!emb || !out || B < 1 || L < 1 || D < 1) return fail(VP_EINVAL, "bad argument");
  VP_HIP(pool_l2(emb, dtype == VP_BF16, (int)B, (int)L, (int)D, out, static_cast<hipStream_t>(stream)));
  return VP_OK;
}

}  // extern "C"
