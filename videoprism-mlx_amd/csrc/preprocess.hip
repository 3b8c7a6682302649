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

__global__ __launch_bounds__(256) void preprocess_frames_kernel(const PreArgs a) {
  const int f = blockIdx.x / a.blocks_per_frame;
  const int g = (blockIdx.x - f * a.blocks_per_frame) * 256 + threadIdx.x;
  if (g >= a.groups) return;
  int n = f;
  if (a.frame_idx) n = min(max(a.frame_idx[f], 0), a.N - 1);
  const uint8_t* __restrict__ frame = a.src + (int64_t)n * a.frame_stride;
  const int SS = a.S * a.S;
  uint8_t* __restrict__ out = a.dst + (int64_t)f * SS * 3;
  const int p0 = 4 * g;
  int oy = p0 / a.S, ox = p0 - oy * a.S;
  const int c0 = a.swap_rb ? 2 : 0, c2 = 2 - c0;

  uint32_t px[4][3];
  Tap ty = axis_tap(a.y0 + oy, a.scale_y, a.H);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (p0 + j < SS) {
      const Tap tx = axis_tap(a.x0 + ox, a.scale_x, a.W);
      const uint8_t* r0 = frame + (int64_t)ty.s0 * a.row_stride;
      const uint8_t* r1 = frame + (int64_t)ty.s1 * a.row_stride;
      const int o0 = 3 * tx.s0, o1 = 3 * tx.s1;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const int sc = c == 0 ? c0 : c == 1 ? 1 : c2;
        const int h0 = (int)r0[o0 + sc] * tx.a0 + (int)r0[o1 + sc] * tx.a1;
        const int h1 = (int)r1[o0 + sc] * tx.a0 + (int)r1[o1 + sc] * tx.a1;
        px[j][c] = (uint32_t)((((ty.a0 * (h0 >> 4)) >> 16) + ((ty.a1 * (h1 >> 4)) >> 16) + 2) >> 2);
      }
    } else {
      px[j][0] = px[j][1] = px[j][2] = 0;
    }
    if (j < 3 && ++ox == a.S) {  // the group runs over a row's end (S % 4 != 0 only)
      ox = 0;
      ++oy;
      if (p0 + j + 1 < SS) ty = axis_tap(a.y0 + oy, a.scale_y, a.H);
    }
  }

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
  int64_t new_h, new_w, y0, x0;
  if (preprocess_geometry(H, W, S, mode, &new_h, &new_w, &y0, &x0)) return hipErrorInvalidValue;
  const int64_t groups = (S * S + 3) / 4;
  const int64_t bpf = (groups + 255) / 256;
  if (N > INT32_MAX || H >= (1 << 24) || W >= (1 << 24) || S > 16384 || bpf * F > INT32_MAX) return hipErrorInvalidValue;
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
  VP_NOTE_KERNEL(preprocess_frames_kernel);
  hipLaunchKernelGGL(preprocess_frames_kernel, dim3((unsigned)(bpf * F)), dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace vp
