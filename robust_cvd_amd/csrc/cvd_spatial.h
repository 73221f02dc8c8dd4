// The two spatial terms of the reference's fine-tuning criterion and their gradient with respect to the depth maps, in one walk:
// DisparitySmoothLoss (loss/disparity_smooth_loss.py:15-56), the edge-aware L1 on the disparity gradient, and ContrastLoss
// (loss/contrast_loss.py:13-79), which keeps the depth ratio across the original estimator's depth edges above a threshold
// (DESIGN.md §3.12).  Templated on the precision T (float / double) of every real array.  The lane / vector-load helpers are
// those of cvd_loss_common.h.
//
// Tables, contiguous, F = B N frames, frame f of sample b = f / N: depth [F][H][W], depth_orig [F][H][W] (read only with the
// contrast term), image [F][3][H][W] (read only with the smoothness term).  With d = 1 / D:
//   x-edge (x < W-1):  w_x = exp(-mean_c |I_c(x,y) - I_c(x+1,y)| / sigma),  s_x = w_x |d(x,y) - d(x+1,y)|;  y-edge likewise
//   S_b    = lambda_s [ sum_{f in b} sum s_x / (N H (W-1)) + sum_{f in b} sum s_y / (N (H-1) W) ],   smooth = mean_b S_b
//   r(a, b) = max(a, b) / (min(a, b) + 1e-10)                                  (the 1e-10 is added in T, as the reference does)
//   h-edge (x < W-1):  c_h = [ r(Do(x+1,y), Do(x,y)) > tau ] (tau - r(D(x+1,y), D(x,y)))^2;  v-edge likewise with (x, y+1)
//   contrast = lambda_c (sum c_h + sum c_v) / F,   total = smooth + contrast   (a term exists only when its lambda is > 0)
// The reference's last column / row (a ratio against a zero pad, overwritten with 0 in place) contributes no value and no
// gradient; its torch.max(square, zeros) is a no-op; sign(0) = 0; min / max of two equal depths pass half the gradient each.
//
// k_sp_pass<T, PIX, GRAD>  grid (nb F), 256 threads: workgroup (f, tile) covers 256 PIX consecutive pixels of frame f, a thread
//                          PIX consecutive pixels of one row (PIX = 4: W % 4 == 0 and 16 / 32-byte aligned tables, the rule of
//                          k_cons_forward).  A pixel accumulates the right and the bottom edge it owns; with GRAD it also forms
//                          d total / d D(x, y) from its four incident edges of both terms and writes it with one plain store: the
//                          normalisers are pixel counts, so d total / d (edge value) is a constant per term the host computes
//                          (kx, ky, kc) and no finishing pass comes first.  Row neighbours: registers inside a thread's group,
//                          lane exchange across lanes (a load at either end of a wave); the rows above and below are read
//                          from the cache.  Per-workgroup f64 sums (sum s_x, sum s_y, sum c_h + sum c_v) go to a slot of a slab:
//                          shuffle tree over the lanes, waves in index order.  No atomics: value and gradient repeat bit for
//                          bit on every build.  The per-pixel arithmetic is compiled without contraction, so the one- and the
//                          four-pixel path give the same bits.
// k_sp_finish              one workgroup: a wave per sample sums its frames' slots in a fixed order into S_b; thread 0 then
//                          forms smooth, contrast and total.
#pragma once
#include "cvd_loss_common.h"

namespace cvd {

constexpr int kSpFinishThreads = 1024;

template <typename T>
struct SpArgs {
  int F, W, H;
  int nb;                       // workgroups per frame
  int useSmooth, useContrast;   // the term's lambda is > 0
  T sigma, tau;
  T kx, ky, kc;                 // d total / d s_x, d s_y, d c (GRAD only)
  const T* depth;
  const T* depthOrig;           // or null (no contrast term)
  const T* image;               // or null (no smoothness term)
  double* slab;                 // [F][nb][3]
  T* grad;                      // [F][H][W]; GRAD only
};

struct SpFinishArgs {
  int F, N, nb;
  int useSmooth, useContrast;
  double lamS, nx, ny;          // lambda_s, N H (W-1), N (H-1) W
  double lamC;
  const double* slab;           // [F][nb][3]
  double* cpart;                // [B]: a sample's sum c
  double* total;                // [1]
  double* smooth;               // [B]
  double* contrast;             // [1]
};

__device__ __forceinline__ float spExp(float v) { return expf(v); }
__device__ __forceinline__ double spExp(double v) { return exp(v); }

// a pixel: depth, original depth, disparity, colour (fields the enabled terms do not read hold 1 / 0)
template <typename T>
struct SpPx {
  T D, Do, d, c0, c1, c2;
};

template <typename T, int PIX>
struct SpGroup {
  SpPx<T> p[PIX];
};

// PIX consecutive pixels of frame f at pixel index i (PIX = 4: aligned vector loads)
template <typename T, int PIX>
__device__ __forceinline__ SpGroup<T, PIX> spLoad(const SpArgs<T>& A, int f, size_t npx, size_t i) {
#pragma clang fp contract(off)
  SpGroup<T, PIX> g;
  const ConsVals<T, PIX> D = consLoad<T, PIX>(A.depth + static_cast<size_t>(f) * npx, i);
#pragma unroll
  for (int k = 0; k < PIX; ++k) {
    g.p[k].D = D.v[k];
    g.p[k].Do = T(1);
    g.p[k].d = g.p[k].c0 = g.p[k].c1 = g.p[k].c2 = T(0);
  }
  if (A.useContrast) {
    const ConsVals<T, PIX> Do = consLoad<T, PIX>(A.depthOrig + static_cast<size_t>(f) * npx, i);
#pragma unroll
    for (int k = 0; k < PIX; ++k) g.p[k].Do = Do.v[k];
  }
  if (A.useSmooth) {
    const T* im = A.image + static_cast<size_t>(f) * 3 * npx;
    const ConsVals<T, PIX> c0 = consLoad<T, PIX>(im, i), c1 = consLoad<T, PIX>(im + npx, i), c2 = consLoad<T, PIX>(im + 2 * npx, i);
#pragma unroll
    for (int k = 0; k < PIX; ++k) {
      g.p[k].d = T(1) / D.v[k];
      g.p[k].c0 = c0.v[k]; g.p[k].c1 = c1.v[k]; g.p[k].c2 = c2.v[k];
    }
  }
  return g;
}

template <typename T>
__device__ __forceinline__ SpPx<T> spDefault() {
  return {T(1), T(1), T(0), T(0), T(0), T(0)};
}

// lane exchange of a pixel: the value of lane (lane + delta); delta = -1 / +1
template <typename T>
__device__ __forceinline__ SpPx<T> spShift(const SpPx<T>& v, int delta) {
  SpPx<T> o;
  if (delta < 0) {
    o.D = __shfl_up(v.D, 1); o.Do = __shfl_up(v.Do, 1); o.d = __shfl_up(v.d, 1);
    o.c0 = __shfl_up(v.c0, 1); o.c1 = __shfl_up(v.c1, 1); o.c2 = __shfl_up(v.c2, 1);
  } else {
    o.D = __shfl_down(v.D, 1); o.Do = __shfl_down(v.Do, 1); o.d = __shfl_down(v.d, 1);
    o.c0 = __shfl_down(v.c0, 1); o.c1 = __shfl_down(v.c1, 1); o.c2 = __shfl_down(v.c2, 1);
  }
  return o;
}

// the smoothness value of the edge (p, q), s = w |d_p - d_q|; gp = d s / d D_p
template <typename T, bool GRAD>
__device__ __forceinline__ T spSmoothEdge(const SpArgs<T>& A, const SpPx<T>& p, const SpPx<T>& q, T& gp) {
#pragma clang fp contract(off)
  const T gm = ((consAbs(p.c0 - q.c0) + consAbs(p.c1 - q.c1)) + consAbs(p.c2 - q.c2)) / T(3);
  const T w = spExp(-gm / A.sigma);
  const T e = p.d - q.d;
  if (GRAD) {
    const T sg = e > T(0) ? T(1) : (e < T(0) ? T(-1) : T(0));
    gp = -(w * sg) * (p.d * p.d);   // d (1 / D) / d D = -d^2
  }
  return w * consAbs(e);
}

// the contrast value of the edge (p, q), c = [r(Do_p, Do_q) > tau] (tau - r(D_p, D_q))^2; gp = d c / d D_p
template <typename T, bool GRAD>
__device__ __forceinline__ T spContrastEdge(const SpArgs<T>& A, const SpPx<T>& p, const SpPx<T>& q, T& gp) {
#pragma clang fp contract(off)
  const T eps = T(1e-10);
  if (GRAD) gp = T(0);
  const T olo = p.Do < q.Do ? p.Do : q.Do, ohi = p.Do < q.Do ? q.Do : p.Do;
  if (!(ohi / (olo + eps) > A.tau)) return T(0);
  const T lo = p.D < q.D ? p.D : q.D, hi = p.D < q.D ? q.D : p.D;
  const T den = lo + eps;
  const T t = A.tau - hi / den;
  if (GRAD) {
    const T up = T(1) / den, dn = -(hi / den) / den;   // d r / d max, d r / d min
    const T dr = p.D > q.D ? up : (p.D < q.D ? dn : T(0.5) * (up + dn));
    gp = (T(-2) * t) * dr;
  }
  return t * t;
}

template <typename T, int PIX, bool GRAD>
inline __global__ __launch_bounds__(kConsThreads) void k_sp_pass(SpArgs<T> A) {
#pragma clang fp contract(off)
  static_assert(PIX == 1 || PIX == 4, "one pixel or four consecutive pixels of a row per thread");
  const int f = static_cast<int>(blockIdx.x / A.nb), tile = static_cast<int>(blockIdx.x - static_cast<unsigned>(f) * A.nb);
  const size_t npx = static_cast<size_t>(A.W) * A.H;
  const size_t i0 = (static_cast<size_t>(tile) * kConsThreads + threadIdx.x) * PIX;
  const int lane = threadIdx.x & 63;
  // (PIX = 4: npx % 4 == 0 and W % 4 == 0, a thread's four pixels are all inside or all outside and share a row)
  const bool in = i0 < npx;
  const int y = in ? static_cast<int>(i0 / A.W) : 0, x = in ? static_cast<int>(i0 - static_cast<size_t>(y) * A.W) : 0;
  const bool hasL = in && x > 0, hasR = in && x + PIX < A.W, hasU = in && y > 0, hasD = in && y + 1 < A.H;
  SpGroup<T, PIX> v, up, dn;
#pragma unroll
  for (int k = 0; k < PIX; ++k) v.p[k] = up.p[k] = dn.p[k] = spDefault<T>();
  if (in) v = spLoad<T, PIX>(A, f, npx, i0);
  if (hasD) dn = spLoad<T, PIX>(A, f, npx, i0 + A.W);
  if (GRAD && hasU) up = spLoad<T, PIX>(A, f, npx, i0 - A.W);
  // the pixels left and right of the group: the neighbouring lane's (every lane takes part in the exchange), a load at a wave's end
  SpPx<T> R = spShift(v.p[0], +1), L = spDefault<T>();
  if (hasR && lane == 63) R = spLoad<T, 1>(A, f, npx, i0 + PIX).p[0];
  if (GRAD) {
    L = spShift(v.p[PIX - 1], -1);
    if (hasL && lane == 0) L = spLoad<T, 1>(A, f, npx, i0 - 1).p[0];
  }
  double acc[3] = {0.0, 0.0, 0.0};
  T g[PIX];
  consEachPixel<0, PIX>([&](auto kc) {
    constexpr int k = decltype(kc)::value;
    const SpPx<T>& p = v.p[k];
    const SpPx<T>& right = k + 1 < PIX ? v.p[k + 1 < PIX ? k + 1 : k] : R;
    const SpPx<T>& left = k > 0 ? v.p[k > 0 ? k - 1 : k] : L;
    const bool eR = k + 1 < PIX ? in : hasR, eL = k > 0 ? in : hasL;
    T gsx = T(0), gsy = T(0), gc = T(0), gp;
    if (A.useSmooth) {
      if (eR) {
        acc[0] += static_cast<double>(spSmoothEdge<T, GRAD>(A, p, right, gp));
        if (GRAD) gsx = gp;
      }
      if (hasD) {
        acc[1] += static_cast<double>(spSmoothEdge<T, GRAD>(A, p, dn.p[k], gp));
        if (GRAD) gsy = gp;
      }
      if (GRAD && eL) {
        (void)spSmoothEdge<T, true>(A, p, left, gp);
        gsx = gp + gsx;
      }
      if (GRAD && hasU) {
        (void)spSmoothEdge<T, true>(A, p, up.p[k], gp);
        gsy = gp + gsy;
      }
    }
    if (A.useContrast) {
      if (GRAD && eL) {
        (void)spContrastEdge<T, true>(A, p, left, gp);
        gc = gp;
      }
      if (eR) {
        acc[2] += static_cast<double>(spContrastEdge<T, GRAD>(A, p, right, gp));
        if (GRAD) gc = gc + gp;
      }
      if (GRAD && hasU) {
        (void)spContrastEdge<T, true>(A, p, up.p[k], gp);
        gc = gc + gp;
      }
      if (hasD) {
        acc[2] += static_cast<double>(spContrastEdge<T, GRAD>(A, p, dn.p[k], gp));
        if (GRAD) gc = gc + gp;
      }
    }
    if (GRAD) g[k] = (A.kx * gsx + A.ky * gsy) + A.kc * gc;
  });
  if (GRAD && in) {
    T* out = A.grad + static_cast<size_t>(f) * npx + i0;
    if constexpr (PIX == 1) {
      out[0] = g[0];
    } else {
      typename ConsVec4<T>::type q;
      q.x = g[0]; q.y = g[1]; q.z = g[2]; q.w = g[3];
      *reinterpret_cast<typename ConsVec4<T>::type*>(out) = q;
    }
  }
  double s;
  if (lossFoldWorkgroup(acc, s)) A.slab[(static_cast<size_t>(f) * A.nb + tile) * 3 + threadIdx.x] = s;
}

// One workgroup.  Wave w takes the samples w, w + 16, ...: per frame of the sample, in frame order, the lanes stride over the
// frame's slots in index order and fold with a shuffle tree (a frame's sum does not depend on which call it is part of).
inline __global__ __launch_bounds__(kSpFinishThreads) void k_sp_finish(SpFinishArgs A) {
  const int B = A.F / A.N, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int b = wave; b < B; b += kSpFinishThreads / 64) {
    double s[3] = {0.0, 0.0, 0.0};
    for (int k = 0; k < A.N; ++k) {
      const double* sl = A.slab + (static_cast<size_t>(b) * A.N + k) * A.nb * 3;
      double a[3] = {0.0, 0.0, 0.0};
      for (int j = lane; j < A.nb; j += 64) {
#pragma unroll
        for (int q = 0; q < 3; ++q) a[q] += sl[static_cast<size_t>(j) * 3 + q];
      }
#pragma unroll
      for (int q = 0; q < 3; ++q) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) a[q] += __shfl_down(a[q], o);
        s[q] += a[q];
      }
    }
    if (lane == 0) {
      A.smooth[b] = A.useSmooth ? A.lamS * (s[0] / A.nx + s[1] / A.ny) : 0.0;
      A.cpart[b] = s[2];
    }
  }
  __threadfence_block();
  __syncthreads();
  if (threadIdx.x == 0) {
    double sm = 0.0, c = 0.0;
    for (int b = 0; b < B; ++b) {
      sm += A.smooth[b];
      c += A.cpart[b];
    }
    sm /= static_cast<double>(B);
    c = A.useContrast ? A.lamC * (c / static_cast<double>(A.F)) : 0.0;
    A.contrast[0] = c;
    A.total[0] = sm + c;
  }
}

}  // namespace cvd
