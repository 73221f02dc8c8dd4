// Flow consistency masks: Flow.compute_flow_masks, reference flow.py:180-209 and utils/consistency.py:8-67.
//
// For a frame pair (a, b) with flows Fab, Fba [h][w][2] (pixels) and colours Ca, Cb [h][w][C], direction a -> b, pixel (x, y):
//   target (tx, ty) = (x + Fab.x, y + Fab.y) in f64 (numpy promotes f32 + int64); in bounds iff 0 <= tx <= w - 1 and
//   0 <= ty <= h - 1.  Sampling position gx = f32(2 tx / w - 1), gy likewise (f64, rounded once), then grid_sample's
//   bilinear / align_corners = false / border rule in f32: px = ((gx + 1) w - 1) / 2 clamped to [0, w - 1] (NaN -> 0), taps
//   floor(px) and floor(px) + 1, a tap outside the image contributes 0.  px = tx - 0.5: the reference samples the target
//   image half a pixel up and left of x + flow, and so does this kernel.
//   ef = sum_c (Fab[c] + S(Fba)[c])^2, ec = sum_c (Ca[c] - S(Cb)[c])^2, S = that sample; f32, left to right.
//   mask = in bounds && ef < flowT && ec < colorT (a NaN fails a comparison).  Direction b -> a swaps the roles.
//
// k_flow_masks<C, PIX>: one launch for P pairs, blockIdx.y = pair, blockIdx.z = direction, 256-thread workgroups over the
// image's linear pixel index, PIX consecutive pixels of a row per thread.
//   PIX = 1  any raster: the own flow is one 8-byte load per lane (a wave reads 512 contiguous bytes), the own colour C
//            dword loads, the mask a byte store.
//   PIX = 4  w % 4 == 0 (every image base is then 16-byte aligned and a thread's pixels share a row): the own flow is two
//            16-byte loads, the own colour C of them, the mask one packed 4-byte store, the errors two 16-byte stores.
// The other flow and colour are gathered with four taps per pixel straight from global memory: neighbouring lanes hit
// neighbouring texels, so the taps are served by the caches.  No LDS, no scratch.  The per-direction kept counts are wave
// reductions (ballot + popcount) and one integer atomic per wave: integer adds commute, so every output repeats bit for bit.
#pragma once
#include <hip/hip_runtime.h>

namespace cvd {

constexpr int kFlowMaskThreads = 256;

struct FlowMaskArgs {
  int w, h;
  float flowT, colorT;               // f32(flow_thresh^2), f32(C color_thresh^2), each computed in double and rounded once
  const float* color;                // [frames][h][w][C]
  const int2* pairs;                 // [P] (a, b), indices into color
  const float2 *flowAB, *flowBA;     // [P][h][w]
  unsigned char *maskAB, *maskBA;    // [P][h][w], 255 / 0
  int* kept;                         // [P][2], zero before the launch
  float2* errors;                    // [P][2][h][w] (ef, ec), or null
};

// One pixel of one direction: f = own flow, cOwn = own colour, other* = the target frame's images.  err = (ef, ec).
template <int C>
__device__ __forceinline__ bool flowMaskPixel(const FlowMaskArgs& A, int x, int y, float2 f, const float* cOwn,
                                              const float2* otherFlow, const float* otherColor, float2& err) {
#pragma clang fp contract(off)
  const double tx = static_cast<double>(x) + static_cast<double>(f.x);
  const double ty = static_cast<double>(y) + static_cast<double>(f.y);
  const bool inBounds = tx >= 0.0 && tx <= static_cast<double>(A.w - 1) && ty >= 0.0 && ty <= static_cast<double>(A.h - 1);
  const float gx = static_cast<float>(2.0 * tx / static_cast<double>(A.w) - 1.0);
  const float gy = static_cast<float>(2.0 * ty / static_cast<double>(A.h) - 1.0);
  float px = ((gx + 1.f) * static_cast<float>(A.w) - 1.f) / 2.f;
  float py = ((gy + 1.f) * static_cast<float>(A.h) - 1.f) / 2.f;
  px = fminf(fmaxf(px, 0.f), static_cast<float>(A.w - 1));  // (fmaxf(NaN, 0) = 0, as grid_sample's clamp)
  py = fminf(fmaxf(py, 0.f), static_cast<float>(A.h - 1));
  const float fx0 = floorf(px), fy0 = floorf(py);
  const int x0 = static_cast<int>(fx0), y0 = static_cast<int>(fy0);
  const float wx = px - fx0, ex = 1.f - wx, wy = py - fy0, ey = 1.f - wy;
  const float w00 = ey * ex, w01 = ey * wx, w10 = wy * ex, w11 = wy * wx;
  // after the clamp only the +1 tap at the last column / row can lie outside (its weight is 0): it contributes 0 and is
  // read from the clamped texel
  const bool xin = x0 + 1 < A.w, yin = y0 + 1 < A.h;
  const int x1 = xin ? x0 + 1 : x0, y1 = yin ? y0 + 1 : y0;
  const int i00 = y0 * A.w + x0, i01 = y0 * A.w + x1, i10 = y1 * A.w + x0, i11 = y1 * A.w + x1;
  const bool in01 = xin, in10 = yin, in11 = xin && yin;

  const float2 f00 = otherFlow[i00], f01 = otherFlow[i01], f10 = otherFlow[i10], f11 = otherFlow[i11];
  const float sx = f00.x * w00 + (in01 ? f01.x : 0.f) * w01 + (in10 ? f10.x : 0.f) * w10 + (in11 ? f11.x : 0.f) * w11;
  const float sy = f00.y * w00 + (in01 ? f01.y : 0.f) * w01 + (in10 ? f10.y : 0.f) * w10 + (in11 ? f11.y : 0.f) * w11;
  const float dx = f.x + sx, dy = f.y + sy;
  const float ef = dx * dx + dy * dy;

  float ec = 0.f;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const float c00 = otherColor[i00 * C + c], c01 = otherColor[i01 * C + c];
    const float c10 = otherColor[i10 * C + c], c11 = otherColor[i11 * C + c];
    const float sc = c00 * w00 + (in01 ? c01 : 0.f) * w01 + (in10 ? c10 : 0.f) * w10 + (in11 ? c11 : 0.f) * w11;
    const float d = cOwn[c] - sc;
    ec = c == 0 ? d * d : ec + d * d;
  }
  err = make_float2(ef, ec);
  return inBounds && ef < A.flowT && ec < A.colorT;
}

template <int C, int PIX>
inline __global__ __launch_bounds__(kFlowMaskThreads) void k_flow_masks(FlowMaskArgs A) {
  static_assert(PIX == 1 || PIX == 4, "one pixel or four consecutive pixels of a row per thread");
  const int pair = blockIdx.y, dir = blockIdx.z;
  const size_t npx = static_cast<size_t>(A.w) * A.h;
  const int2 ab = A.pairs[pair];
  const int own = dir ? ab.y : ab.x, other = dir ? ab.x : ab.y;
  const float2* ownFlow = (dir ? A.flowBA : A.flowAB) + pair * npx;
  const float2* otherFlow = (dir ? A.flowAB : A.flowBA) + pair * npx;
  const float* ownColor = A.color + own * npx * C;
  const float* otherColor = A.color + other * npx * C;
  unsigned char* mask = (dir ? A.maskBA : A.maskAB) + pair * npx;
  float2* errors = A.errors ? A.errors + (static_cast<size_t>(pair) * 2 + dir) * npx : nullptr;
  const size_t i0 = (static_cast<size_t>(blockIdx.x) * kFlowMaskThreads + threadIdx.x) * PIX;
  const bool active = i0 < npx;  // (PIX = 4: npx % 4 == 0, a thread's four pixels are all inside or all outside)
  int count = 0;
  if constexpr (PIX == 1) {
    bool keep = false;
    if (active) {
      const int y = static_cast<int>(i0 / A.w), x = static_cast<int>(i0 - static_cast<size_t>(y) * A.w);
      const float2 f = ownFlow[i0];
      float cOwn[C];
#pragma unroll
      for (int c = 0; c < C; ++c) cOwn[c] = ownColor[i0 * C + c];
      float2 err;
      keep = flowMaskPixel<C>(A, x, y, f, cOwn, otherFlow, otherColor, err);
      mask[i0] = keep ? 255 : 0;
      if (errors) errors[i0] = err;
    }
    count = __popcll(__ballot(keep));
  } else {
    bool keep[4] = {false, false, false, false};
    if (active) {
      const int y = static_cast<int>(i0 / A.w), x = static_cast<int>(i0 - static_cast<size_t>(y) * A.w);
      const float4* fp = reinterpret_cast<const float4*>(ownFlow + i0);
      const float4 fa = fp[0], fb = fp[1];
      const float2 f[4] = {make_float2(fa.x, fa.y), make_float2(fa.z, fa.w), make_float2(fb.x, fb.y), make_float2(fb.z, fb.w)};
      const float4* cp = reinterpret_cast<const float4*>(ownColor + i0 * C);
      float cOwn[4 * C];
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const float4 v = cp[c];
        cOwn[4 * c] = v.x;
        cOwn[4 * c + 1] = v.y;
        cOwn[4 * c + 2] = v.z;
        cOwn[4 * c + 3] = v.w;
      }
      float2 err[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) keep[k] = flowMaskPixel<C>(A, x + k, y, f[k], cOwn + k * C, otherFlow, otherColor, err[k]);
      *reinterpret_cast<uchar4*>(mask + i0) =
          make_uchar4(keep[0] ? 255 : 0, keep[1] ? 255 : 0, keep[2] ? 255 : 0, keep[3] ? 255 : 0);
      if (errors) {
        float4* ep = reinterpret_cast<float4*>(errors + i0);
        ep[0] = make_float4(err[0].x, err[0].y, err[1].x, err[1].y);
        ep[1] = make_float4(err[2].x, err[2].y, err[3].x, err[3].y);
      }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) count += __popcll(__ballot(keep[k]));
  }
  if ((threadIdx.x & 63) == 0 && count) atomicAdd(A.kept + pair * 2 + dir, count);
}

}  // namespace cvd
