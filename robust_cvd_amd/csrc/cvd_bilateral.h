// Bilateral depth filter: DepthVideoProcessor::bilateralFilter, reference lib/Processor.cpp:183-313 (defaults
// lib/Processor.h:64-70).
//
// For every output pixel (x, y) of frame f the reference visits the samples of the spatio-temporal window
// [f - frameRadius, f + frameRadius] x [y - r, y + r] x [x - r, x + r] clipped to the video / image (frame ascending, then
// row, then column), weights each sample by exp(-(d - dref)^2 / depthSigma^2 - |c - cref|^2 / colorSigma^2) (a term only
// when its sigma is > 0; weight 1 when the exponent is exactly 0) and takes the weighted mean, or the weighted median:
// the first sample, in (depth, weight) lexicographic order, whose running weight sum reaches half the total.
// f32 in the reference's operation order, no FMA contraction; the only non-reproducible operation is the device expf.
//
// Layout: 256-thread workgroups, blockIdx.z = output frame.
//   k_bilateral_mean<COLOR, LDS>   one thread per output pixel, the workgroup a 32 x 8 tile (a wave = two 128-byte rows).
//       LDS = true (spatialRadius > 0 and the tile fits): each window frame's tile plus a halo of r is staged in LDS one
//       frame at a time (depth, and BGR colour when COLOR), so every input texel is fetched about once per frame of the
//       window instead of (2r + 1)^2 times.  LDS = false (r = 0, the default; or a halo too large for 64 KB): samples
//       stream straight from global memory, the neighbouring frames' reads hitting the caches.
//   k_bilateral_median_small<CAP, COLOR>  one thread per output pixel (same tile), for windows of <= CAP samples
//       (CAP = 16 / 64): the samples live in two VGPR arrays of CAP entries.  The gather is unrolled over the CAP slots
//       with wave-uniform window counters, so every array index is a compile-time constant; slots outside the clipped
//       window hold the pad (+inf, 0).  A bitonic sorting network over the CAP slots (static indices again) sorts them
//       and an unrolled scan picks the median.  Pads sort after every finite sample and add exactly 0 to either sum.
//   k_bilateral_median_wave<COLOR>  one WAVE per output pixel (4 pixels per workgroup), for windows of up to
//       kBilateralMaxSamples (2048) samples: the window's (depth, weight) pairs, padded with (+inf, 0) to the power of two
//       P2, are held in LDS (8 P2 bytes per wave, <= 64 KB per workgroup), spread over the 64 lanes; a bitonic sort in
//       LDS (one workgroup barrier per stage, every wave of the workgroup has the same P2) orders them, and lane 0 runs
//       the two sequential f32 sums (total weight in window order, running weight in sorted order) of the reference.
#pragma once
#include <hip/hip_runtime.h>

namespace cvd {

constexpr int kBilateralTileW = 32, kBilateralTileH = 8;   // 256 threads
constexpr int kBilateralMaxSamples = 2048;                 // median: largest window (samples per pixel) supported
constexpr int kBilateralMaxLds = 64 * 1024;                // LDS staging / wave median: bytes per workgroup

struct BilateralArgs {
  int n;                    // frames in the batch (consecutive); temporal windows are clipped to [0, n)
  int first;                // batch frame of output frame 0 of this launch (output frame = first + blockIdx.z)
  int w, h;                 // raster of depth, colour and output
  int frameRadius, spatialRadius;
  int useDepth, useColor;   // depthSigma > 0, colorSigma > 0
  float depthSigma2, colorSigma2;  // sqr(sigma) in f32, as the reference squares them
  const float* depth;       // [n][h][w]
  const float* color;       // [n][h][w][3] BGR (null when !useColor)
  float* out;               // [launch frames][h][w]
};

template <bool COLOR>  // COLOR == A.useColor (the launch picks the instantiation)
__device__ __forceinline__ float bilateralWeight(const BilateralArgs& A, float d, float dref, const float* c,
                                                 const float* cref) {
#pragma clang fp contract(off)
  float exponent = 0.f;
  if (A.useDepth) {
    const float diff = d - dref;
    const float diff2 = diff * diff;
    exponent += -diff2 / A.depthSigma2;
  }
  if constexpr (COLOR) {
    const float e0 = c[0] - cref[0], e1 = c[1] - cref[1], e2 = c[2] - cref[2];
    const float diff2 = e0 * e0 + e1 * e1 + e2 * e2;
    exponent += -diff2 / A.colorSigma2;
  }
  return exponent != 0.f ? expf(exponent) : 1.f;
}

// std::pair<float, float> order (depth, then weight)
__device__ __forceinline__ bool bilateralPairGreater(float a, float aw, float b, float bw) {
  return a > b || (a == b && aw > bw);
}

template <bool COLOR>
__device__ __forceinline__ void bilateralRef(const BilateralArgs& A, int kf, int x, int y, float& dref, float* cref) {
  const size_t at = (static_cast<size_t>(kf) * A.h + y) * A.w + x;
  dref = A.depth[at];
  if constexpr (COLOR) {
#pragma unroll
    for (int i = 0; i < 3; ++i) cref[i] = A.color[at * 3 + i];
  }
}

template <bool COLOR, bool LDS>
inline __global__ __launch_bounds__(256) void k_bilateral_mean(BilateralArgs A) {
#pragma clang fp contract(off)
  extern __shared__ float bilateralLds[];
  const int tx = threadIdx.x % kBilateralTileW, ty = threadIdx.x / kBilateralTileW;
  const int bx = blockIdx.x * kBilateralTileW, by = blockIdx.y * kBilateralTileH;
  const int x = bx + tx, y = by + ty;
  const bool inside = x < A.w && y < A.h;
  const int kf = A.first + blockIdx.z;
  const int r = A.spatialRadius;
  const int k0 = max(0, kf - A.frameRadius), k1 = min(A.n - 1, kf + A.frameRadius);
  float dref = 0.f, cref[3] = {0.f, 0.f, 0.f};
  if (inside) bilateralRef<COLOR>(A, kf, x, y, dref, cref);
  const int y0 = max(0, y - r), y1 = min(A.h - 1, y + r);
  const int x0 = max(0, x - r), x1 = min(A.w - 1, x + r);
  const size_t px = static_cast<size_t>(A.w) * A.h;
  float sumDepth = 0.f, sumWeight = 0.f;
  if constexpr (LDS) {
    // tile + halo of frame k: rows by - r .. by + 7 + r, columns bx - r .. bx + 31 + r
    const int TW = kBilateralTileW + 2 * r, TH = kBilateralTileH + 2 * r, T = TW * TH;
    float* sd = bilateralLds;
    float* sc = bilateralLds + T;  // [T][3] when COLOR
    for (int k = k0; k <= k1; ++k) {
      const float* fd = A.depth + static_cast<size_t>(k) * px;
      const float* fc = COLOR ? A.color + static_cast<size_t>(k) * px * 3 : nullptr;
      for (int t = threadIdx.x; t < T; t += 256) {
        const int gx = bx - r + t % TW, gy = by - r + t / TW;
        const bool in = gx >= 0 && gx < A.w && gy >= 0 && gy < A.h;
        const size_t g = static_cast<size_t>(gy) * A.w + gx;
        float d = 0.f, c[3] = {0.f, 0.f, 0.f};  // (halo texels outside the image are never read back)
        if (in) {
          d = fd[g];
          if constexpr (COLOR) {
#pragma unroll
            for (int i = 0; i < 3; ++i) c[i] = fc[g * 3 + i];
          }
        }
        sd[t] = d;
        if constexpr (COLOR) {
#pragma unroll
          for (int i = 0; i < 3; ++i) sc[t * 3 + i] = c[i];
        }
      }
      __syncthreads();
      if (inside) {
        for (int wy = y0; wy <= y1; ++wy) {
          const int row = (wy - by + r) * TW - bx + r;
          for (int wx = x0; wx <= x1; ++wx) {
            const int t = row + wx;
            const float d = sd[t];
            const float wgt = bilateralWeight<COLOR>(A, d, dref, sc + t * 3, cref);
            sumDepth += d * wgt;
            sumWeight += wgt;
          }
        }
      }
      __syncthreads();
    }
  } else {
    if (!inside) return;
    for (int k = k0; k <= k1; ++k) {
      const float* fd = A.depth + static_cast<size_t>(k) * px;
      const float* fc = COLOR ? A.color + static_cast<size_t>(k) * px * 3 : nullptr;
      for (int wy = y0; wy <= y1; ++wy) {
        for (int wx = x0; wx <= x1; ++wx) {
          const size_t g = static_cast<size_t>(wy) * A.w + wx;
          float c[3] = {0.f, 0.f, 0.f};
          if constexpr (COLOR) {
#pragma unroll
            for (int i = 0; i < 3; ++i) c[i] = fc[g * 3 + i];
          }
          const float d = fd[g];
          const float wgt = bilateralWeight<COLOR>(A, d, dref, c, cref);
          sumDepth += d * wgt;
          sumWeight += wgt;
        }
      }
    }
  }
  if (inside) A.out[(static_cast<size_t>(blockIdx.z) * A.h + y) * A.w + x] = sumWeight > 0.f ? sumDepth / sumWeight : 0.f;
}

template <int CAP, bool COLOR>
inline __global__ __launch_bounds__(256) void k_bilateral_median_small(BilateralArgs A) {
#pragma clang fp contract(off)
  const int x = blockIdx.x * kBilateralTileW + threadIdx.x % kBilateralTileW;
  const int y = blockIdx.y * kBilateralTileH + threadIdx.x / kBilateralTileW;
  if (x >= A.w || y >= A.h) return;
  const int kf = A.first + blockIdx.z;
  const int r = A.spatialRadius, R = A.frameRadius;
  float dref, cref[3] = {0.f, 0.f, 0.f};
  bilateralRef<COLOR>(A, kf, x, y, dref, cref);
  const int side = 2 * r + 1;
  const int total = side * side * (2 * R + 1);  // unclipped window (<= CAP, checked by the host)
  const size_t px = static_cast<size_t>(A.w) * A.h;
  float ds[CAP], ws[CAP];
  float sumWeight = 0.f;
  int k = kf - R, dy = -r, dx = -r;  // window counters in the reference's order, uniform over the workgroup
#pragma unroll
  for (int i = 0; i < CAP; ++i) {
    const int wx = x + dx, wy = y + dy;
    const bool valid = i < total && k >= 0 && k < A.n && wx >= 0 && wx < A.w && wy >= 0 && wy < A.h;
    float d = __builtin_inff(), wgt = 0.f;
    if (valid) {
      const size_t g = static_cast<size_t>(k) * px + static_cast<size_t>(wy) * A.w + wx;
      float c[3] = {0.f, 0.f, 0.f};
      if constexpr (COLOR) {
#pragma unroll
        for (int j = 0; j < 3; ++j) c[j] = A.color[g * 3 + j];
      }
      d = A.depth[g];
      wgt = bilateralWeight<COLOR>(A, d, dref, c, cref);
    }
    sumWeight += wgt;  // (+0 for a skipped sample: the sum is unchanged)
    ds[i] = d;
    ws[i] = wgt;
    if (++dx > r) {
      dx = -r;
      if (++dy > r) { dy = -r; ++k; }
    }
  }
#pragma unroll
  for (int kk = 2; kk <= CAP; kk <<= 1) {
#pragma unroll
    for (int j = kk >> 1; j > 0; j >>= 1) {
#pragma unroll
      for (int i = 0; i < CAP; ++i) {
        const int l = i ^ j;
        if (l > i) {
          const bool up = (i & kk) == 0;
          const bool swap = bilateralPairGreater(ds[i], ws[i], ds[l], ws[l]) == up;
          const float a = ds[i], b = ds[l], aw = ws[i], bw = ws[l];
          ds[i] = swap ? b : a;
          ds[l] = swap ? a : b;
          ws[i] = swap ? bw : aw;
          ws[l] = swap ? aw : bw;
        }
      }
    }
  }
  const float half = sumWeight / 2.f;
  float cum = 0.f, result = 0.f;  // (the reference leaves the pixel unwritten if no sample reaches half, e.g. NaN weights)
  bool found = false;
#pragma unroll
  for (int i = 0; i < CAP; ++i) {
    cum += ws[i];
    const bool hit = !found && cum >= half;
    result = hit ? ds[i] : result;
    found = found || hit;
  }
  A.out[(static_cast<size_t>(blockIdx.z) * A.h + y) * A.w + x] = result;
}

// dynamic LDS: 4 waves x P2 x (depth, weight)
template <bool COLOR>
inline __global__ __launch_bounds__(256) void k_bilateral_median_wave(BilateralArgs A, int P2) {
#pragma clang fp contract(off)
  extern __shared__ float bilateralLds[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float* keys = bilateralLds + static_cast<size_t>(wave) * 2 * P2;
  float* wts = keys + P2;
  const int p = blockIdx.x * 4 + wave;
  const bool inside = p < A.w * A.h;  // (a wave past the last pixel sorts pads: every wave must reach the barriers)
  const int x = inside ? p % A.w : 0, y = inside ? p / A.w : 0;
  const int kf = A.first + blockIdx.z;
  const int r = A.spatialRadius, R = A.frameRadius, side = 2 * r + 1, plane = side * side;
  const int total = plane * (2 * R + 1);
  float dref = 0.f, cref[3] = {0.f, 0.f, 0.f};
  if (inside) bilateralRef<COLOR>(A, kf, x, y, dref, cref);
  const size_t px = static_cast<size_t>(A.w) * A.h;
  for (int j = lane; j < P2; j += 64) {
    const int fi = j / plane, rem = j - fi * plane;
    const int k = kf - R + fi, wy = y - r + rem / side, wx = x - r + rem % side;
    const bool valid = inside && j < total && k >= 0 && k < A.n && wx >= 0 && wx < A.w && wy >= 0 && wy < A.h;
    float d = __builtin_inff(), wgt = 0.f;
    if (valid) {
      const size_t g = static_cast<size_t>(k) * px + static_cast<size_t>(wy) * A.w + wx;
      float c[3] = {0.f, 0.f, 0.f};
      if constexpr (COLOR) {
#pragma unroll
        for (int i = 0; i < 3; ++i) c[i] = A.color[g * 3 + i];
      }
      d = A.depth[g];
      wgt = bilateralWeight<COLOR>(A, d, dref, c, cref);
    }
    keys[j] = d;
    wts[j] = wgt;
  }
  __syncthreads();
  float sumWeight = 0.f;
  if (lane == 0)
    for (int j = 0; j < total; ++j) sumWeight += wts[j];  // window order (a skipped sample adds +0)
  __syncthreads();
  for (int kk = 2; kk <= P2; kk <<= 1) {
    for (int jj = kk >> 1; jj > 0; jj >>= 1) {
      for (int i = lane; i < P2; i += 64) {
        const int l = i ^ jj;
        if (l > i) {
          const float a = keys[i], b = keys[l], aw = wts[i], bw = wts[l];
          if (bilateralPairGreater(a, aw, b, bw) == ((i & kk) == 0)) {
            keys[i] = b;
            keys[l] = a;
            wts[i] = bw;
            wts[l] = aw;
          }
        }
      }
      __syncthreads();
    }
  }
  if (inside && lane == 0) {
    const float half = sumWeight / 2.f;
    float cum = 0.f, result = 0.f;
    for (int j = 0; j < P2; ++j) {
      cum += wts[j];
      if (cum >= half) { result = keys[j]; break; }
    }
    A.out[(static_cast<size_t>(blockIdx.z) * A.h + y) * A.w + x] = result;
  }
}

}  // namespace cvd
