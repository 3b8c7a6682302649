// Frame ingest in front of the encoder (video_utils.py:76-87, 97-127): gather a frame by index, resize
// it the way cv2.resize(frame, (new_w, new_h)) does on uint8 (INTER_LINEAR in 11-bit fixed point),
// keep the centre-crop window, optionally swap R and B, and store uint8 [F, S, S, 3].  Only the window
// is computed; the resized full frame never exists.
//
// Memory-bound (a 720p source is 2.7 MB per frame in, 0.25 MB out).  One thread produces 4
// consecutive output pixels of the frame taken as a flat pixel array (12 bytes = three dword stores
// when the frame's base is 4-byte aligned, byte stores otherwise), so a wave covers 256 consecutive
// pixels of an output row and its taps fall in two contiguous source row segments.  The source is
// read with byte loads only: a tap is 3 bytes at a 3-byte pitch behind an arbitrary base and row
// stride, and a wider load would leave [src, src + extent) at a row's end.
//
// preprocess_yuv_kernel is the same kernel in front of a decoder's 4:2:0 planes (NV12, I420, P010): each
// of a pixel's 4 taps is converted to uint8 R, G, B first, in 16.16 fixed point with the coefficients
// of yuv_coefficients (tests/yuv_restatement.py states the arithmetic), and the blend runs on those.  A
// tap is one luma sample and one chroma pair; luma (y, x) uses chroma (y >> 1, x >> 1), so a pixel's
// taps share their pair along an axis whenever both fall in one chroma cell (always when s0 is even).
//
// VIEWS is the same body once more with the geometry read per output frame from a device table [V, 9]
// (box_y, box_x, box_h, box_w, new_h, new_w, win_y, win_x, flags): output frame f is frame f % T of view
// f / T, the picture cv2.resize(img[box], (new_w, new_h))[win : win + S], mirrored along x where flags & 1.
// A block never spans two frames, so the nine ints are wave-uniform loads.  The taps are formed against the
// box (they clamp at its edges) and then moved by the box origin, so the YUV chroma cell is the absolute
// one.  load_view clamps the table: no table can make a tap leave the frame.
#include "vp_common.h"
#include "vp_kernels.h"

namespace vp {

namespace {

struct Tap {
  int s0, s1;  // the two source indices (s1 clamped to the last)
  int a0, a1;  // their weights, scaled by 2048
};

// One axis of cv2's linear resize table for output index d of `dst`, source size `src`, scale =
// 1 / (dst / src) in double.  The coordinate is a double product, a double difference, then one
// rounding to float32: a fused multiply-add gives other coefficients, hence no contraction here.
__device__ __forceinline__ Tap axis_tap(int d, double scale, int src) {
#pragma clang fp contract(off)
  const double prod = ((double)d + 0.5) * scale;
  float f = (float)(prod - 0.5);
  const float fl = floorf(f);
  int s = (int)fl;
  f -= fl;
  if (s < 0) { s = 0; f = 0.0f; }
  if (s >= src - 1) { s = src - 1; f = 0.0f; }
  Tap t;
  t.s0 = s;
  t.s1 = min(s + 1, src - 1);
  t.a1 = (int)rintf(f * 2048.0f);           // round half to even
  t.a0 = (int)rintf((1.0f - f) * 2048.0f);
  return t;
}

// cv2's vertical pass over the two horizontal sums h0 (row s0) and h1 (row s1)
__device__ __forceinline__ uint32_t blend_rows(const Tap& ty, int h0, int h1) {
  return (uint32_t)((((ty.a0 * (h0 >> 4)) >> 16) + ((ty.a1 * (h1 >> 4)) >> 16) + 2) >> 2);
}

// What an output frame is cut from: the source box that is resized, the scales of that resize, the
// window's origin in it and the mirror.  Without a view table the box is the frame and nothing is mirrored.
struct Geometry {
  int by, bx, bh, bw;       // source box
  int y0, x0;               // window origin in the resized box
  double scale_y, scale_x;  // 1 / (new / box), cv2's double
  bool flip;
};

// One row of the view table, clamped: the box lies inside the H x W frame and holds a pixel, the resize is
// S .. 2^24 - 1 a side, the window lies inside the resize.  A valid row passes through unchanged.
__device__ __forceinline__ Geometry load_view(const int32_t* __restrict__ v, int H, int W, int S) {
  Geometry w;
  w.by = min(max(v[0], 0), H - 1);
  w.bx = min(max(v[1], 0), W - 1);
  w.bh = min(max(v[2], 1), H - w.by);
  w.bw = min(max(v[3], 1), W - w.bx);
  const int nh = min(max(v[4], S), (1 << 24) - 1);
  const int nw = min(max(v[5], S), (1 << 24) - 1);
  w.y0 = min(max(v[6], 0), nh - S);
  w.x0 = min(max(v[7], 0), nw - S);
  w.flip = (v[8] & 1) != 0;
  w.scale_y = 1.0 / ((double)nh / (double)w.bh);  // the host's expression: correctly rounded divisions
  w.scale_x = 1.0 / ((double)nw / (double)w.bw);
  return w;
}

// Geometry of output frame f: row f / T of the table (wave-uniform: a block lies in one frame), or the
// launch's own.
template <bool VIEWS, typename Args>
__device__ __forceinline__ Geometry frame_geometry(const Args& a, int f) {
  if constexpr (VIEWS) {
    return load_view(a.views + (int64_t)(f / a.T) * 9, a.H, a.W, a.S);
  } else {
    return Geometry{0, 0, a.H, a.W, a.y0, a.x0, a.scale_y, a.scale_x, false};
  }
}

// The taps of output row oy / column ox in frame coordinates: formed against the box, so they clamp at its
// edges, then moved by its origin.  A mirrored frame's column ox shows the window's column S - 1 - ox.
__device__ __forceinline__ Tap row_tap(const Geometry& g, int oy) {
  Tap t = axis_tap(g.y0 + oy, g.scale_y, g.bh);
  t.s0 += g.by;
  t.s1 += g.by;
  return t;
}
__device__ __forceinline__ Tap col_tap(const Geometry& g, int ox, int S) {
  Tap t = axis_tap(g.x0 + (g.flip ? S - 1 - ox : ox), g.scale_x, g.bw);
  t.s0 += g.bx;
  t.s1 += g.bx;
  return t;
}

// The 4 pixels p0 .. p0+3 of a frame's flat pixel array `out` (SS pixels): three dword stores when the
// frame's base is 4-byte aligned and the group is whole, byte stores otherwise.
__device__ __forceinline__ void store_group(uint8_t* __restrict__ out, int p0, int SS, const uint32_t (&px)[4][3]) {
  uint8_t* o = out + (int64_t)p0 * 3;
  const bool aligned = ((uintptr_t)out & 3) == 0;  // the same for every thread of the block
  if (aligned && p0 + 4 <= SS) {
    uint32_t* o4 = reinterpret_cast<uint32_t*>(o);
    o4[0] = px[0][0] | (px[0][1] << 8) | (px[0][2] << 16) | (px[1][0] << 24);
    o4[1] = px[1][1] | (px[1][2] << 8) | (px[2][0] << 16) | (px[2][1] << 24);
    o4[2] = px[2][2] | (px[3][0] << 8) | (px[3][1] << 16) | (px[3][2] << 24);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (p0 + j < SS) {
#pragma unroll
        for (int c = 0; c < 3; ++c) o[3 * j + c] = (uint8_t)px[j][c];
      }
  }
}

struct PreArgs {
  const uint8_t* src;
  const int32_t* frame_idx;  // nullable
  uint8_t* dst;
  int64_t row_stride, frame_stride;
  double scale_x, scale_y;
  int N, H, W, S;
  int x0, y0;        // crop window origin in the resized frame
  int swap_rb;
  int groups;        // 4-pixel groups per frame = ceil(S*S / 4)
  int blocks_per_frame;
};

// The view variants' arguments behind the plain ones', whose layout stays as it is.
struct ViewTable {
  const int32_t* views;  // [V, 9]
  int T;                 // output frames per view
};
struct PreViewArgs : PreArgs, ViewTable {};

template <bool VIEWS>
__global__ __launch_bounds__(256) void preprocess_frames_kernel(const std::conditional_t<VIEWS, PreViewArgs, PreArgs> a) {
  const int f = blockIdx.x / a.blocks_per_frame;
  const int g = (blockIdx.x - f * a.blocks_per_frame) * 256 + threadIdx.x;
  if (g >= a.groups) return;
  int n = f;
  if constexpr (VIEWS) n = f % a.T;
  if (a.frame_idx) n = min(max(a.frame_idx[f], 0), a.N - 1);
  const uint8_t* __restrict__ frame = a.src + (int64_t)n * a.frame_stride;
  const int SS = a.S * a.S;
  uint8_t* __restrict__ out = a.dst + (int64_t)f * SS * 3;
  const int p0 = 4 * g;
  int oy = p0 / a.S, ox = p0 - oy * a.S;
  const int c0 = a.swap_rb ? 2 : 0, c2 = 2 - c0;
  const Geometry geo = frame_geometry<VIEWS>(a, f);

  uint32_t px[4][3];
  Tap ty = row_tap(geo, oy);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (p0 + j < SS) {
      const Tap tx = col_tap(geo, ox, a.S);
      const uint8_t* r0 = frame + (int64_t)ty.s0 * a.row_stride;
      const uint8_t* r1 = frame + (int64_t)ty.s1 * a.row_stride;
      const int o0 = 3 * tx.s0, o1 = 3 * tx.s1;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const int sc = c == 0 ? c0 : c == 1 ? 1 : c2;
        const int h0 = (int)r0[o0 + sc] * tx.a0 + (int)r0[o1 + sc] * tx.a1;
        const int h1 = (int)r1[o0 + sc] * tx.a0 + (int)r1[o1 + sc] * tx.a1;
        px[j][c] = blend_rows(ty, h0, h1);
      }
    } else {
      px[j][0] = px[j][1] = px[j][2] = 0;
    }
    if (j < 3 && ++ox == a.S) {  // the group runs over a row's end (S % 4 != 0 only)
      ox = 0;
      ++oy;
      if (p0 + j + 1 < SS) ty = row_tap(geo, oy);
    }
  }
  store_group(out, p0, SS, px);
}

// ---- 4:2:0 planes in (NV12, I420, P010) ----

struct YuvArgs {
  const uint8_t* plane[3];   // Y, UV, - (NV12, P010) or Y, U, V (I420)
  int64_t row_stride[3], frame_stride[3];  // bytes
  const int32_t* frame_idx;  // nullable
  uint8_t* dst;
  double scale_x, scale_y;
  int32_t coef[3][3];        // rows R, G, B x (cy, cu, cv), 16.16
  int32_t yoff, coff;
  int N, H, W, S;
  int x0, y0;
  int groups, blocks_per_frame;
};
struct YuvViewArgs : YuvArgs, ViewTable {};

// What one chroma sample adds to R, G, B before the shift: cu*(U - coff) + cv*(V - coff) + 32768.
struct Chroma {
  int t[3];
};

// One sample by a load of its own: the compiler fuses two plain loads of neighbouring samples into one
// unaligned load of twice the width, a relaxed wave-scope atomic load is the same instruction and stays single.
template <typename T>
__device__ __forceinline__ int load_single(const T* p) {
  return (int)__hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
}

// The chroma sample (cy, cx) of frame-relative planes pu / pv (pv unused with interleaved chroma).  PAIR:
// the interleaved U,V pair is one aligned load (2 bytes for NV12, 4 for P010), else one load per sample.
template <int FMT, bool PAIR>
__device__ __forceinline__ Chroma load_chroma(const YuvArgs& a, const uint8_t* __restrict__ pu,
                                              const uint8_t* __restrict__ pv, int cy, int cx) {
  int u, v;
  if (FMT == YUV_I420) {
    u = pu[(int64_t)cy * a.row_stride[1] + cx];
    v = pv[(int64_t)cy * a.row_stride[2] + cx];
  } else if (FMT == YUV_NV12) {
    const uint8_t* p = pu + (int64_t)cy * a.row_stride[1] + 2 * cx;
    if (PAIR) {
      const uint32_t w = *reinterpret_cast<const uint16_t*>(p);
      u = (int)(w & 0xff);
      v = (int)(w >> 8);
    } else {
      u = load_single(p);
      v = load_single(p + 1);
    }
  } else {  // P010: little-endian words, the sample in the high 10 bits
    const uint8_t* p = pu + (int64_t)cy * a.row_stride[1] + 4 * cx;
    if (PAIR) {
      const uint32_t w = *reinterpret_cast<const uint32_t*>(p);
      u = (int)((w & 0xffff) >> 6);
      v = (int)(w >> 22);
    } else {
      const uint16_t* q = reinterpret_cast<const uint16_t*>(p);
      u = load_single(q) >> 6;
      v = load_single(q + 1) >> 6;
    }
  }
  u -= a.coff;
  v -= a.coff;
  Chroma c;
#pragma unroll
  for (int k = 0; k < 3; ++k) c.t[k] = a.coef[k][1] * u + a.coef[k][2] * v + 32768;
  return c;
}

// Luma sample x of row `row`, less yoff
template <int FMT>
__device__ __forceinline__ int load_luma(const YuvArgs& a, const uint8_t* __restrict__ row, int x) {
  if (FMT == YUV_P010) return (int)(reinterpret_cast<const uint16_t*>(row)[x] >> 6) - a.yoff;
  return (int)row[x] - a.yoff;
}

// uint8 channel k of a tap: luma (less yoff) and its chroma term, clamped once, after the shift
__device__ __forceinline__ int yuv_channel(const YuvArgs& a, int k, int luma, const Chroma& c) {
  return min(max((a.coef[k][0] * luma + c.t[k]) >> 16, 0), 255);
}

template <int FMT, bool PAIR, bool VIEWS>
__global__ __launch_bounds__(256) void preprocess_yuv_kernel(const std::conditional_t<VIEWS, YuvViewArgs, YuvArgs> a) {
  const int f = blockIdx.x / a.blocks_per_frame;
  const int g = (blockIdx.x - f * a.blocks_per_frame) * 256 + threadIdx.x;
  if (g >= a.groups) return;
  int n = f;
  if constexpr (VIEWS) n = f % a.T;
  if (a.frame_idx) n = min(max(a.frame_idx[f], 0), a.N - 1);
  const uint8_t* __restrict__ py = a.plane[0] + (int64_t)n * a.frame_stride[0];
  const uint8_t* __restrict__ pu = a.plane[1] + (int64_t)n * a.frame_stride[1];
  const uint8_t* __restrict__ pv = FMT == YUV_I420 ? a.plane[2] + (int64_t)n * a.frame_stride[2] : nullptr;
  const int SS = a.S * a.S;
  uint8_t* __restrict__ out = a.dst + (int64_t)f * SS * 3;
  const int p0 = 4 * g;
  int oy = p0 / a.S, ox = p0 - oy * a.S;
  const Geometry geo = frame_geometry<VIEWS>(a, f);

  uint32_t px[4][3];
  Tap ty = row_tap(geo, oy);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (p0 + j < SS) {
      const Tap tx = col_tap(geo, ox, a.S);
      const uint8_t* r0 = py + (int64_t)ty.s0 * a.row_stride[0];
      const uint8_t* r1 = py + (int64_t)ty.s1 * a.row_stride[0];
      const int l00 = load_luma<FMT>(a, r0, tx.s0), l01 = load_luma<FMT>(a, r0, tx.s1);
      const int l10 = load_luma<FMT>(a, r1, tx.s0), l11 = load_luma<FMT>(a, r1, tx.s1);
      // taps in one chroma cell share its pair: along x whenever s0 is even (or s1 is clamped), same along y
      const int cy0 = ty.s0 >> 1, cy1 = ty.s1 >> 1, cx0 = tx.s0 >> 1, cx1 = tx.s1 >> 1;
      const Chroma c00 = load_chroma<FMT, PAIR>(a, pu, pv, cy0, cx0);
      Chroma c01 = c00;
      if (cx1 != cx0) c01 = load_chroma<FMT, PAIR>(a, pu, pv, cy0, cx1);
      Chroma c10 = c00, c11 = c01;
      if (cy1 != cy0) {
        c10 = load_chroma<FMT, PAIR>(a, pu, pv, cy1, cx0);
        c11 = c10;
        if (cx1 != cx0) c11 = load_chroma<FMT, PAIR>(a, pu, pv, cy1, cx1);
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const int h0 = yuv_channel(a, c, l00, c00) * tx.a0 + yuv_channel(a, c, l01, c01) * tx.a1;
        const int h1 = yuv_channel(a, c, l10, c10) * tx.a0 + yuv_channel(a, c, l11, c11) * tx.a1;
        px[j][c] = blend_rows(ty, h0, h1);
      }
    } else {
      px[j][0] = px[j][1] = px[j][2] = 0;
    }
    if (j < 3 && ++ox == a.S) {  // the group runs over a row's end (S % 4 != 0 only)
      ox = 0;
      ++oy;
      if (p0 + j + 1 < SS) ty = row_tap(geo, oy);
    }
  }
  store_group(out, p0, SS, px);
}

template <int FMT, bool PAIR, typename Args>
hipError_t launch_yuv(const Args& a, int64_t blocks, hipStream_t s) {
  constexpr bool VIEWS = std::is_same<Args, YuvViewArgs>::value;
  VP_NOTE_KERNEL((preprocess_yuv_kernel<FMT, PAIR, VIEWS>));
  hipLaunchKernelGGL((preprocess_yuv_kernel<FMT, PAIR, VIEWS>), dim3((unsigned)blocks), dim3(256), 0, s, a);
  return hipGetLastError();
}

// The kernel for the planes' format and alignment (PAIR where every interleaved pair is one aligned load)
template <typename Args>
hipError_t launch_yuv_format(const YuvPlanes& src, const Args& a, int64_t blocks, hipStream_t s) {
  // the low bits every interleaved pair's address shares: a pair is one load only where these make it aligned
  const uintptr_t chroma_bits = (uintptr_t)src.plane[1] | (uintptr_t)src.row_stride[1] | (uintptr_t)src.frame_stride[1];
  switch (src.format) {
    case YUV_NV12:
      return (chroma_bits & 1) == 0 ? launch_yuv<YUV_NV12, true>(a, blocks, s) : launch_yuv<YUV_NV12, false>(a, blocks, s);
    case YUV_I420:
      return launch_yuv<YUV_I420, false>(a, blocks, s);
    case YUV_P010:
      if (((uintptr_t)src.plane[0] | (uintptr_t)src.row_stride[0] | (uintptr_t)src.frame_stride[0] | chroma_bits) & 1)
        return hipErrorInvalidValue;
      return (chroma_bits & 3) == 0 ? launch_yuv<YUV_P010, true>(a, blocks, s) : launch_yuv<YUV_P010, false>(a, blocks, s);
  }
  return hipErrorInvalidValue;
}

// groups and blocks per frame of S x S output; false if F frames are more than one launch takes
bool launch_shape(int64_t N, int64_t H, int64_t W, int64_t S, int64_t F, int64_t* groups, int64_t* bpf) {
  *groups = (S * S + 3) / 4;
  *bpf = (*groups + 255) / 256;
  return !(N > INT32_MAX || H >= (1 << 24) || W >= (1 << 24) || S > 16384 || *bpf * F > INT32_MAX);
}

void fill_yuv_args(YuvArgs& a, const YuvPlanes& src, const int32_t coef[11], const int32_t* frame_idx, uint8_t* dst,
                   int64_t N, int64_t H, int64_t W, int64_t S, int64_t groups, int64_t bpf) {
  for (int p = 0; p < 3; ++p) {
    a.plane[p] = static_cast<const uint8_t*>(src.plane[p]);
    a.row_stride[p] = src.row_stride[p];
    a.frame_stride[p] = src.frame_stride[p];
  }
  a.frame_idx = frame_idx; a.dst = dst;
  for (int i = 0; i < 9; ++i) a.coef[i / 3][i % 3] = coef[i];
  a.yoff = coef[9]; a.coff = coef[10];
  a.N = (int)N; a.H = (int)H; a.W = (int)W; a.S = (int)S;
  a.groups = (int)groups;
  a.blocks_per_frame = (int)bpf;
}

}  // namespace

const char* preprocess_geometry(int64_t H, int64_t W, int64_t S, int mode, int64_t* new_h, int64_t* new_w,
                                int64_t* y0, int64_t* x0) {
  if (mode == 1) {
    *new_h = *new_w = S;
  } else if (H < W) {  // video_utils.py:112-117: Python doubles, int() truncation
    *new_h = S;
    *new_w = (int64_t)((double)W * ((double)S / (double)H));
  } else {
    *new_w = S;
    *new_h = (int64_t)((double)H * ((double)S / (double)W));
  }
  *y0 = (*new_h - S) / 2;
  *x0 = (*new_w - S) / 2;
  if (*new_h < S || *new_w < S) return "resized frame smaller than the crop window";
  if (*new_h >= (int64_t)1 << 24 || *new_w >= (int64_t)1 << 24) return "resized frame of 2^24 pixels or more a side";
  return nullptr;
}

hipError_t preprocess_frames(const uint8_t* src, int64_t N, int64_t H, int64_t W, int64_t row_stride,
                             int64_t frame_stride, const int32_t* frame_idx, int64_t F, int mode, int swap_rb,
                             int64_t S, uint8_t* dst, hipStream_t s) {
  int64_t new_h, new_w, y0, x0, groups, bpf;
  if (preprocess_geometry(H, W, S, mode, &new_h, &new_w, &y0, &x0)) return hipErrorInvalidValue;
  if (!launch_shape(N, H, W, S, F, &groups, &bpf)) return hipErrorInvalidValue;
  PreArgs a;
  a.src = src; a.frame_idx = frame_idx; a.dst = dst;
  a.row_stride = row_stride; a.frame_stride = frame_stride;
  // cv2: inv_scale = dsize / ssize, scale = 1 / inv_scale (not ssize / dsize)
  a.scale_x = 1.0 / ((double)new_w / (double)W);
  a.scale_y = 1.0 / ((double)new_h / (double)H);
  a.N = (int)N; a.H = (int)H; a.W = (int)W; a.S = (int)S;
  a.x0 = (int)x0; a.y0 = (int)y0;
  a.swap_rb = swap_rb ? 1 : 0;
  a.groups = (int)groups;
  a.blocks_per_frame = (int)bpf;
  VP_NOTE_KERNEL(preprocess_frames_kernel<false>);
  hipLaunchKernelGGL(preprocess_frames_kernel<false>, dim3((unsigned)(bpf * F)), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t preprocess_views(const uint8_t* src, int64_t N, int64_t H, int64_t W, int64_t row_stride,
                            int64_t frame_stride, const int32_t* frame_idx, const int32_t* views, int64_t V,
                            int64_t T, int swap_rb, int64_t S, uint8_t* dst, hipStream_t s) {
  int64_t groups, bpf;
  if (V * T > INT32_MAX || !launch_shape(N, H, W, S, V * T, &groups, &bpf)) return hipErrorInvalidValue;
  PreViewArgs a;
  a.src = src; a.frame_idx = frame_idx; a.dst = dst;
  a.row_stride = row_stride; a.frame_stride = frame_stride;
  a.scale_x = a.scale_y = 0.0;  // the table's
  a.N = (int)N; a.H = (int)H; a.W = (int)W; a.S = (int)S;
  a.x0 = a.y0 = 0;
  a.swap_rb = swap_rb ? 1 : 0;
  a.groups = (int)groups;
  a.blocks_per_frame = (int)bpf;
  a.views = views; a.T = (int)T;
  VP_NOTE_KERNEL(preprocess_frames_kernel<true>);
  hipLaunchKernelGGL(preprocess_frames_kernel<true>, dim3((unsigned)(bpf * V * T)), dim3(256), 0, s, a);
  return hipGetLastError();
}

const char* yuv_coefficients(int matrix, int range, int bit_depth, int32_t out[11]) {
  if (matrix != 0 && matrix != 1) return "unknown YUV matrix";
  if (range != 0 && range != 1) return "unknown YUV range";
  if (bit_depth != 8 && bit_depth != 10) return "bit_depth must be 8 or 10";
  const double kr = matrix == 0 ? 0.299 : 0.2126, kb = matrix == 0 ? 0.114 : 0.0722, kg = 1.0 - kr - kb;
  const double s = (double)(1 << (bit_depth - 8)), full = (double)((1 << bit_depth) - 1);
  const double ygain = range == 0 ? 255.0 / (219.0 * s) : 255.0 / full;
  const double cgain = range == 0 ? 255.0 / (224.0 * s) : 255.0 / full;
  const double real[9] = {ygain, 0.0, cgain * 2.0 * (1.0 - kr),
                          ygain, -(cgain * 2.0 * (1.0 - kb) * kb / kg), -(cgain * 2.0 * (1.0 - kr) * kr / kg),
                          ygain, cgain * 2.0 * (1.0 - kb), 0.0};
  for (int i = 0; i < 9; ++i) out[i] = (int32_t)std::floor(real[i] * 65536.0 + 0.5);
  out[9] = range == 0 ? 16 << (bit_depth - 8) : 0;
  out[10] = 128 << (bit_depth - 8);
  return nullptr;
}

hipError_t preprocess_yuv(const YuvPlanes& src, const int32_t coef[11], int64_t N, int64_t H, int64_t W,
                          const int32_t* frame_idx, int64_t F, int mode, int64_t S, uint8_t* dst, hipStream_t s) {
  int64_t new_h, new_w, y0, x0, groups, bpf;
  if (preprocess_geometry(H, W, S, mode, &new_h, &new_w, &y0, &x0)) return hipErrorInvalidValue;
  if (!launch_shape(N, H, W, S, F, &groups, &bpf)) return hipErrorInvalidValue;
  YuvArgs a;
  fill_yuv_args(a, src, coef, frame_idx, dst, N, H, W, S, groups, bpf);
  a.scale_x = 1.0 / ((double)new_w / (double)W);
  a.scale_y = 1.0 / ((double)new_h / (double)H);
  a.x0 = (int)x0; a.y0 = (int)y0;
  return launch_yuv_format(src, a, bpf * F, s);
}

hipError_t preprocess_yuv_views(const YuvPlanes& src, const int32_t coef[11], int64_t N, int64_t H, int64_t W,
                                const int32_t* frame_idx, const int32_t* views, int64_t V, int64_t T, int64_t S,
                                uint8_t* dst, hipStream_t s) {
  int64_t groups, bpf;
  if (V * T > INT32_MAX || !launch_shape(N, H, W, S, V * T, &groups, &bpf)) return hipErrorInvalidValue;
  YuvViewArgs a;
  fill_yuv_args(a, src, coef, frame_idx, dst, N, H, W, S, groups, bpf);
  a.scale_x = a.scale_y = 0.0;  // the table's
  a.x0 = a.y0 = 0;
  a.views = views; a.T = (int)T;
  return launch_yuv_format(src, a, bpf * V * T, s);
}

}  // namespace vp
