// Device building blocks the fine-tuning losses share (cvd_consistency.h, cvd_sceneflow.h, cvd_spatial.h):
// the math overloads, the one- / four-pixel loads, the robust distance, the bilinear tap rule, the per-workgroup fold into a slab
// slot with its finishing pass, and the ordered tap additions of the deterministic build.  Each decision lives here once.
//
// lossBilinearTaps       grid_sample (bilinear, align_corners = false, border): g = 2 m / (size - 1) - 1, u = ((g + 1) size - 1) / 2
//                        clamped to [0, size - 1], taps floor / floor + 1; the +1 tap at the last column / row has weight 0 and is
//                        read from the clamped texel.
// lossFoldWorkgroup<N>   a thread's double acc[N] summed over the workgroup for its slot[0..N) of a slab: lanes by a shuffle tree,
//                        waves in index order.  Nothing is accumulated atomically.
// lossFinishPairs<C>    the body of k_cons_finish_pairs / k_sf_finish_pairs: one wave per pair sums the pair's C classes of slab
//                        slots in a fixed order.
// lossOrderedTaps        CVD_DETERMINISTIC: the taps of one lane at a time, in lane order.
#pragma once
#include <hip/hip_runtime.h>
#include <type_traits>

#ifndef CVD_DETERMINISTIC
#define CVD_DETERMINISTIC 0
#endif

namespace cvd {

constexpr int kConsThreads = 256;
constexpr int kConsDetThreads = 64;

enum ConsRho { CONS_RHO_L1 = 0, CONS_RHO_TWO = 1, CONS_RHO_ZERO = 2, CONS_RHO_GENERAL = 3 };

__device__ __forceinline__ bool consPairOk(int2 ab, int F) {
  return ab.x >= 0 && ab.x < F && ab.y >= 0 && ab.y < F && ab.x != ab.y;
}

__device__ __forceinline__ float consAbs(float v) { return fabsf(v); }
__device__ __forceinline__ double consAbs(double v) { return fabs(v); }
__device__ __forceinline__ float consSqrt(float v) { return sqrtf(v); }
__device__ __forceinline__ double consSqrt(double v) { return sqrt(v); }
__device__ __forceinline__ float consLog(float v) { return logf(v); }
__device__ __forceinline__ double consLog(double v) { return log(v); }
__device__ __forceinline__ float consLog1p(float v) { return log1pf(v); }
__device__ __forceinline__ double consLog1p(double v) { return log1p(v); }
__device__ __forceinline__ float consPow(float a, float b) { return powf(a, b); }
__device__ __forceinline__ double consPow(double a, double b) { return pow(a, b); }
__device__ __forceinline__ float consFloor(float v) { return floorf(v); }
__device__ __forceinline__ double consFloor(double v) { return floor(v); }
__device__ __forceinline__ float consClamp(float v, float hi) { return fminf(fmaxf(v, 0.f), hi); }  // (NaN -> 0, as grid_sample)
__device__ __forceinline__ double consClamp(double v, double hi) { return fmin(fmax(v, 0.0), hi); }

// one robust distance: kind (ConsRho), scale, and the constants of the general branch (beta = max(eps32, |alpha - 2|),
// alphaSafe = sign(alpha) max(eps32, |alpha|))
template <typename T>
struct ConsDistance {
  int kind;
  T scale, alpha, beta, alphaSafe;
};

// rho(e) and d rho / d e of the distance R
template <typename T>
__device__ __forceinline__ T consRhoOf(const ConsDistance<T>& R, T e, T& d) {
  const T q = e / R.scale;
  if (R.kind == CONS_RHO_L1) {
    d = (e > T(0) ? T(1) : (e < T(0) ? T(-1) : T(0))) / R.scale;
    return consAbs(q);
  }
  const T s = q * q, hs = T(0.5) * s;
  if (R.kind == CONS_RHO_TWO) {
    d = q / R.scale;
    return hs;
  }
  if (R.kind == CONS_RHO_ZERO) {
    const T cap = T(33e37);
    d = hs < cap ? (q / R.scale) / (T(1) + hs) : T(0);
    return consLog1p(hs < cap ? hs : cap);
  }
  const T base = s / R.beta + T(1);
  const T pw = consPow(base, T(0.5) * R.alpha);
  d = (R.alpha / R.alphaSafe) * (pw / base) * (q / R.scale);
  return (R.beta / R.alphaSafe) * (pw - T(1));
}

// the four bilinear taps of the sampling position (mx, my) in a W x H map: columns x[0] / x[1] and rows y[0] / y[1], index and
// weight of the taps (x0, y0), (x1, y0), (x0, y1), (x1, y1)
template <typename T>
struct LossTaps {
  int x[2], y[2];
  int idx[4];
  T wt[4];
};

template <typename T>
__device__ __forceinline__ LossTaps<T> lossBilinearTaps(int W, int H, T mx, T my) {
  const T gx = T(2) * mx / static_cast<T>(W - 1) - T(1), gy = T(2) * my / static_cast<T>(H - 1) - T(1);
  const T u = consClamp(((gx + T(1)) * static_cast<T>(W) - T(1)) / T(2), static_cast<T>(W - 1));
  const T v = consClamp(((gy + T(1)) * static_cast<T>(H) - T(1)) / T(2), static_cast<T>(H - 1));
  const T fu = consFloor(u), fv = consFloor(v);
  const int x0 = static_cast<int>(fu), y0 = static_cast<int>(fv);
  const T tx = u - fu, ex = T(1) - tx, ty = v - fv, ey = T(1) - ty;
  // after the clamp only the +1 tap at the last column / row can lie outside: it contributes nothing and is read from the
  // clamped texel
  const bool xin = x0 + 1 < W, yin = y0 + 1 < H;
  const int x1 = xin ? x0 + 1 : x0, y1 = yin ? y0 + 1 : y0;
  LossTaps<T> t;
  t.x[0] = x0; t.x[1] = x1; t.y[0] = y0; t.y[1] = y1;
  t.idx[0] = y0 * W + x0; t.idx[1] = y0 * W + x1; t.idx[2] = y1 * W + x0; t.idx[3] = y1 * W + x1;
  t.wt[0] = ey * ex; t.wt[1] = xin ? ey * tx : T(0); t.wt[2] = yin ? ty * ex : T(0); t.wt[3] = (xin && yin) ? ty * tx : T(0);
  return t;
}

// f(k) for k = 0 .. PIX - 1 with k a compile-time constant: the per-pixel arrays stay in registers
template <int K, int PIX, typename Fn>
__device__ __forceinline__ void consEachPixel(Fn&& f) {
  if constexpr (K < PIX) {
    f(std::integral_constant<int, K>{});
    consEachPixel<K + 1, PIX>(f);
  }
}

template <typename T> struct ConsVec4;
template <> struct ConsVec4<float> { using type = float4; };
template <> struct ConsVec4<double> { using type = double4; };

// PIX consecutive values at p[i] (PIX = 4: one 16 / 32-byte aligned vector load), returned by value
template <typename T, int PIX>
struct ConsVals {
  T v[PIX];
};

template <typename T, int PIX>
__device__ __forceinline__ ConsVals<T, PIX> consLoad(const T* __restrict__ p, size_t i) {
  ConsVals<T, PIX> out;
  if constexpr (PIX == 1) {
    out.v[0] = p[i];
  } else {
    const typename ConsVec4<T>::type q = *reinterpret_cast<const typename ConsVec4<T>::type*>(p + i);
    out.v[0] = q.x; out.v[1] = q.y; out.v[2] = q.z; out.v[3] = q.w;
  }
  return out;
}

// acc[0..N) of every thread of a kConsThreads workgroup summed: a shuffle tree over the lanes, then the waves in index order.
// Every thread of the workgroup calls it; true in the threads q < N, which hold the sum of acc[q] in s and write it to their
// workgroup's slot of the slab.
template <int N>
__device__ __forceinline__ bool lossFoldWorkgroup(double (&acc)[N], double& s) {
  __shared__ double part[kConsThreads / 64][N];
#pragma unroll
  for (int q = 0; q < N; ++q)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc[q] += __shfl_down(acc[q], o);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int q = 0; q < N; ++q) part[wave][q] = acc[q];
  }
  __syncthreads();
  if (threadIdx.x >= N) return false;
  s = part[0][threadIdx.x];
#pragma unroll
  for (int k = 1; k < kConsThreads / 64; ++k) s += part[k][threadIdx.x];
  return true;
}

// The body of a loss's finish-pairs kernel, one wave per pair: sums[pair][class][q] = the nb slots of slab [P][CLASSES][nb][4],
// lane-strided in index order, then a shuffle tree.
template <int CLASSES>
__device__ __forceinline__ void lossFinishPairs(const double* slab, double* sums, int nb) {
  const int pair = blockIdx.x, lane = threadIdx.x;
#pragma unroll
  for (int cq = 0; cq < CLASSES * 4; ++cq) {
    const int cls = cq >> 2, q = cq & 3;
    const double* s = slab + (static_cast<size_t>(pair) * CLASSES + cls) * nb * 4 + q;
    double a = 0.0;
    for (int b = lane; b < nb; b += 64) a += s[static_cast<size_t>(b) * 4];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) a += __shfl_down(a, o);
    if (lane == 0) sums[(static_cast<size_t>(pair) * CLASSES + cls) * 4 + q] = a;
  }
}

// sum of one double per thread over the workgroup, in a fixed order; every thread returns the sum
__device__ __forceinline__ double consBlockSum(double v, double* red) {
  __syncthreads();
  red[threadIdx.x] = v;
  __syncthreads();
  for (int o = kConsThreads / 2; o > 0; o >>= 1) {
    if (static_cast<int>(threadIdx.x) < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  return red[0];
}

__device__ __forceinline__ void consAtomicAdd(float* p, float v) { atomicAdd(p, v); }
__device__ __forceinline__ void consAtomicAdd(double* p, double v) { atomicAdd(p, v); }

// adds gTap[j] to gf[idx[j]] for the four taps of every lane of the wave: the taps of one lane at a time, in lane order (taps of
// different lanes may coincide)
template <typename T>
__device__ __forceinline__ void lossOrderedTaps(T* gf, int lane, const int* idx, const T* gTap) {
  unsigned long long todo = __ballot(gTap[0] != T(0) || gTap[1] != T(0) || gTap[2] != T(0) || gTap[3] != T(0));
  while (todo) {
    const int l = __ffsll(static_cast<long long>(todo)) - 1;
    todo &= todo - 1;
    if (lane == l) {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (gTap[j] != T(0)) consAtomicAdd(gf + idx[j], gTap[j]);
    }
  }
}

}  // namespace cvd
