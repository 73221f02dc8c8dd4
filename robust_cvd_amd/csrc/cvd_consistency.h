// Geometric consistency loss of flow pairs and its gradient with respect to the depth maps: the static terms of the reference's
// fine-tuning loss, loss/consistency_loss.py:92-182, 219-239 with utils/geometry.py:9-165, 238-245 and utils/loss.py:62-80
// (DESIGN.md §3.10).  Templated on the precision T (float / double) of every real array.
//
// Tables: depth [F][H][W], extrinsics [F][3][4] = [R | t] (columns right / up / backward), intrinsics [F][4] = (fx, fy, cx, cy),
// optional warp [F][2][H][W] (pixel offsets, planar), pairs [P] = (a, b), and per direction k one planar flow [P][2][H][W] and
// one weight map [P][H][W]: k = 0 is a -> b on a's raster, k = 1 is b -> a on b's raster.  With ref frame r and target frame t
// of (pair, direction), at pixel (x, y):
//   pix   = (x, y) + warp_r(x, y)
//   X_r   = ((pix.x - cx_r) / fx_r, -(pix.y - cy_r) / fy_r, -1) D_r(x, y)
//   X_t   = R_t^T (R_r X_r + t_r - t_t)                  formed as M X_r + b with M = R_t^T R_r, b = R_t^T (t_r - t_t)
//   proj  = (cx_t + fx_t X_t.x / (-X_t.z), cy_t - fy_t X_t.y / (-X_t.z))
//   m     = pix + flow_k(x, y),   e_rep = |proj - m|
//   z_w   = -bilinear(D_t; m): the tap rule of cvd_loss_common.h (grid_sample, bilinear, align_corners = false, border)
//   e_dsp = 1 / X_t.z - 1 / z_w,   e_rat = lambda_ratio log(min(|z_w|, |X_t.z|) / max(|z_w|, |X_t.z|))
//   term(e) = sum_px w rho(e) / max(sum_px w, 1e-6)
// rho: |e / scale| (l1) or the exact branch of the general robust loss (Barron 2019) at alpha = 2, alpha = 0 or any other finite
// alpha, with its clamps to f32 machine epsilon.
//
// k_cons_forward<T, PIX>   grid (blocks, P, 2), 256 threads, PIX = 1 or 4 consecutive pixels of a row per thread (4: W % 4 == 0 and
//                          16 / 32-byte aligned tables).  The cameras of (pair, direction) are the same for the whole workgroup.
//                          Every workgroup folds (sum w, sum w rho_rep, sum w rho_dsp, sum w rho_rat) in f64 into its slot of a
//                          slab (lossFoldWorkgroup): nothing is accumulated atomically.
// k_cons_finish_pairs      one wave per pair: sums the pair's slab slots in a fixed order (lossFinishPairs<2>).
// k_cons_finish_total      one workgroup: the mean focal lengths, the per-pair terms, the total, and for the backward pass the
//                          factor d total / d (sum w rho) of every (pair, direction, term).  The forward result repeats bit for bit.
// k_cons_backward<T, PIX>  the same walk; recomputes the sample and adds d total / d depth to the gradient table [F][H][W] (zero
//                          before the launch): one hardware float atomic for D_r(x, y), up to four for the bilinear taps of D_t.
//                          The sampling position depends on no depth.  sign(0) = 0 and the norm of the zero vector has gradient 0.
// k_cons_backward_det<T>   CVD_DETERMINISTIC: one wave per DESTINATION frame walks the (pair, direction)s that name the frame, in
//                          pair order; the taps of one lane at a time (lossOrderedTaps).  All additions to a frame's table come
//                          from one wave in program order, so the gradient repeats bit for bit.  Slow; for tests.
// A pair that names a frame outside [0, F), or one frame twice, is never dereferenced: its terms and the total come back NaN.
#pragma once
#include "cvd_loss_common.h"

namespace cvd {

template <typename T>
struct ConsArgs {
  int F, P, W, H;
  int useRep, useDsp, useRat;   // the term's lambda is > 0
  int nb;                       // workgroups per (pair, direction)
  T lamRat;
  ConsDistance<T> rho;          // the loss's one distance
  const T* depth;
  const T* ext;
  const T* intr;
  const T* warp;                // or null
  const int2* pairs;
  const T* flow[2];
  const T* weight[2];
  double* slab;                 // [P][2][nb][4]
  const double* coef;           // [P][2][3]: d total / d (sum w rho) of (rep, dsp, rat); backward only
  T* grad;                      // [F][H][W]; backward only
};

struct ConsFinishArgs {
  int F, P, nb;
  double lamRep, lamDsp, lamRat;  // lamRat: only its sign matters here (the ratio's lambda sits inside the distance)
  const int2* pairs;
  double* slab;    // [P][2][nb][4]
  double* sums;    // [P][2][4]
  double* coef;    // [P][2][3]
  double* terms;   // [P][3]
  double* total;   // [1]
};

template <typename T>
struct ConsCam {
  T M[9], b[3];
  T fxr, fyr, cxr, cyr, fxt, fyt, cxt, cyt;
};

template <typename T>
__device__ __forceinline__ ConsCam<T> consCam(const ConsArgs<T>& A, int r, int t) {
  const T* Er = A.ext + static_cast<size_t>(r) * 12;
  const T* Et = A.ext + static_cast<size_t>(t) * 12;
  ConsCam<T> c;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j) c.M[i * 3 + j] = Et[i] * Er[j] + Et[4 + i] * Er[4 + j] + Et[8 + i] * Er[8 + j];
    c.b[i] = Et[i] * (Er[3] - Et[3]) + Et[4 + i] * (Er[7] - Et[7]) + Et[8 + i] * (Er[11] - Et[11]);
  }
  const T* Ir = A.intr + static_cast<size_t>(r) * 4;
  const T* It = A.intr + static_cast<size_t>(t) * 4;
  c.fxr = Ir[0]; c.fyr = Ir[1]; c.cxr = Ir[2]; c.cyr = Ir[3];
  c.fxt = It[0]; c.fyt = It[1]; c.cxt = It[2]; c.cyt = It[3];
  return c;
}

// One sample.  Forward (GRAD = false): adds (w, w rho_rep, w rho_dsp, w rho_rat) to acc.  Backward: cf = the three factors
// d total / d (sum w rho); gD = d total / d D_r(x, y), tap[k] / gTap[k] = index into the target's depth map and its share
// (gTap = 0 for a tap outside the image).
template <typename T, bool GRAD>
__device__ __forceinline__ void consSample(const ConsArgs<T>& A, const ConsCam<T>& c, const T* __restrict__ Dt, int x, int y, T D,
                                           T wx, T wy, T fx, T fy, T w, const T* cf, double* acc, T& gD, int* tap, T* gTap) {
  const T px = static_cast<T>(x) + wx, py = static_cast<T>(y) + wy;
  const T rx = (px - c.cxr) / c.fxr, ry = -(py - c.cyr) / c.fyr;
  const T Xr = rx * D, Yr = ry * D, Zr = -D;
  const T X = c.M[0] * Xr + c.M[1] * Yr + c.M[2] * Zr + c.b[0];
  const T Y = c.M[3] * Xr + c.M[4] * Yr + c.M[5] * Zr + c.b[1];
  const T Z = c.M[6] * Xr + c.M[7] * Yr + c.M[8] * Zr + c.b[2];
  const T mx = px + fx, my = py + fy;
  T g = T(0), gz = T(0);  // d total / d D_r, d total / d z_w
  if (GRAD) gD = T(0);
  // d X_t / d D_r
  const T ax = c.M[0] * rx + c.M[1] * ry - c.M[2], ay = c.M[3] * rx + c.M[4] * ry - c.M[5], az = c.M[6] * rx + c.M[7] * ry - c.M[8];
  const T iz2 = T(1) / (Z * Z);
  if (A.useRep) {
    const T nz = -Z;
    const T dx = (X / nz) * c.fxt + c.cxt - mx;
    const T dy = -((Y / nz) * c.fyt) + c.cyt - my;
    const T e = consSqrt(dx * dx + dy * dy);
    T dr;
    const T r = consRhoOf(A.rho, e, dr);
    if (!GRAD) acc[1] += static_cast<double>(w * r);
    else if (e > T(0)) {
      const T dpx = -c.fxt * (ax * Z - X * az) * iz2, dpy = c.fyt * (ay * Z - Y * az) * iz2;
      g += cf[0] * w * dr * ((dx * dpx + dy * dpy) / e);
    }
  }
  if (A.useDsp || A.useRat) {
    const LossTaps<T> tp = lossBilinearTaps(A.W, A.H, mx, my);
    const T zw = -(Dt[tp.idx[0]] * tp.wt[0] + Dt[tp.idx[1]] * tp.wt[1] + Dt[tp.idx[2]] * tp.wt[2] + Dt[tp.idx[3]] * tp.wt[3]);
    if (A.useDsp) {
      const T e = T(1) / Z - T(1) / zw;
      T dr;
      const T r = consRhoOf(A.rho, e, dr);
      if (!GRAD) acc[2] += static_cast<double>(w * r);
      else {
        const T k = cf[1] * w * dr;
        g += k * (-az * iz2);
        gz += k / (zw * zw);
      }
    }
    if (A.useRat) {
      const T p = consAbs(zw), q = consAbs(Z);
      const T e = A.lamRat * consLog((p < q ? p : q) / (p < q ? q : p));
      T dr;
      const T r = consRhoOf(A.rho, e, dr);
      if (!GRAD) acc[3] += static_cast<double>(w * r);
      else {
        const T sg = p < q ? T(1) : (p > q ? T(-1) : T(0));
        const T k = cf[2] * w * dr * sg * A.lamRat;
        g += -k * az / Z;
        gz += k / zw;
      }
    }
    if (GRAD) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        tap[j] = tp.idx[j];
        gTap[j] = -tp.wt[j] * gz;
      }
    }
  } else if (GRAD) {
    tap[0] = tap[1] = tap[2] = tap[3] = 0;
    gTap[0] = gTap[1] = gTap[2] = gTap[3] = T(0);
  }
  if (!GRAD) acc[0] += static_cast<double>(w);
  else gD = g;
}

// The inputs of a thread's PIX pixels of (pair, dir); ref frame r.
template <typename T, int PIX>
struct ConsPixels {
  ConsVals<T, PIX> D, wx, wy, fx, fy, w;
};

template <typename T, int PIX>
__device__ __forceinline__ ConsPixels<T, PIX> consLoadPixels(const ConsArgs<T>& A, int pair, int dir, int r, size_t npx, size_t i0) {
  ConsPixels<T, PIX> v;
  v.D = consLoad<T, PIX>(A.depth + static_cast<size_t>(r) * npx, i0);
  const T* fl = A.flow[dir] + static_cast<size_t>(pair) * 2 * npx;
  v.fx = consLoad<T, PIX>(fl, i0);
  v.fy = consLoad<T, PIX>(fl + npx, i0);
  v.w = consLoad<T, PIX>(A.weight[dir] + static_cast<size_t>(pair) * npx, i0);
  ConsVals<T, PIX> zero;
#pragma unroll
  for (int k = 0; k < PIX; ++k) zero.v[k] = T(0);
  v.wx = v.wy = zero;
  if (A.warp) {
    const T* wp = A.warp + static_cast<size_t>(r) * 2 * npx;
    v.wx = consLoad<T, PIX>(wp, i0);
    v.wy = consLoad<T, PIX>(wp + npx, i0);
  }
  return v;
}

template <typename T, int PIX>
inline __global__ __launch_bounds__(kConsThreads) void k_cons_forward(ConsArgs<T> A) {
  static_assert(PIX == 1 || PIX == 4, "one pixel or four consecutive pixels of a row per thread");
  const int pair = blockIdx.y, dir = blockIdx.z;
  const size_t npx = static_cast<size_t>(A.W) * A.H;
  double* slot = A.slab + ((static_cast<size_t>(pair) * 2 + dir) * A.nb + blockIdx.x) * 4;
  const int2 ab = A.pairs[pair];
  if (!consPairOk(ab, A.F)) {  // (the whole workgroup)
    if (threadIdx.x < 4) slot[threadIdx.x] = __builtin_nan("");
    return;
  }
  const int r = dir ? ab.y : ab.x, t = dir ? ab.x : ab.y;
  const ConsCam<T> c = consCam(A, r, t);
  const T* Dt = A.depth + static_cast<size_t>(t) * npx;
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  const size_t i0 = (static_cast<size_t>(blockIdx.x) * kConsThreads + threadIdx.x) * PIX;
  if (i0 < npx) {  // (PIX = 4: npx % 4 == 0, a thread's four pixels are all inside or all outside and share a row)
    const int y = static_cast<int>(i0 / A.W), x = static_cast<int>(i0 - static_cast<size_t>(y) * A.W);
    const ConsPixels<T, PIX> v = consLoadPixels<T, PIX>(A, pair, dir, r, npx, i0);
    consEachPixel<0, PIX>([&](auto kc) {
      constexpr int k = decltype(kc)::value;
      T gD;
      consSample<T, false>(A, c, Dt, x + k, y, v.D.v[k], v.wx.v[k], v.wy.v[k], v.fx.v[k], v.fy.v[k], v.w.v[k], nullptr, acc, gD, nullptr, nullptr);
    });
  }
  double s;
  if (lossFoldWorkgroup(acc, s)) slot[threadIdx.x] = s;
}

inline __global__ __launch_bounds__(64) void k_cons_finish_pairs(ConsFinishArgs A) { lossFinishPairs<2>(A.slab, A.sums, A.nb); }

template <typename T>
inline __global__ __launch_bounds__(kConsThreads) void k_cons_finish_total(ConsFinishArgs A, const T* __restrict__ intr) {
  __shared__ double red[kConsThreads];
  // fbar[k]: mean of (fx, fy) over the ref frames of ALL pairs in direction k (the reference's torch.mean over the batch)
  double f0 = 0.0, f1 = 0.0;
  for (int p = threadIdx.x; p < A.P; p += kConsThreads) {
    const int2 ab = A.pairs[p];
    if (!consPairOk(ab, A.F)) continue;  // (its terms are NaN through the slab)
    f0 += static_cast<double>(intr[static_cast<size_t>(ab.x) * 4]) + static_cast<double>(intr[static_cast<size_t>(ab.x) * 4 + 1]);
    f1 += static_cast<double>(intr[static_cast<size_t>(ab.y) * 4]) + static_cast<double>(intr[static_cast<size_t>(ab.y) * 4 + 1]);
  }
  const double fbar[2] = {consBlockSum(f0, red) / (2.0 * A.P), consBlockSum(f1, red) / (2.0 * A.P)};
  double sum = 0.0;
  for (int p = threadIdx.x; p < A.P; p += kConsThreads) {
    double term[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const double* s = A.sums + (static_cast<size_t>(p) * 2 + k) * 4;
      const double n = fmax(s[0], 1e-6);
      const double lam[3] = {A.lamRep, A.lamDsp * fbar[k], A.lamRat > 0.0 ? 1.0 : 0.0};
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        term[q] += 0.5 * lam[q] * (s[1 + q] / n);
        A.coef[(static_cast<size_t>(p) * 2 + k) * 3 + q] = 0.5 * lam[q] / (n * A.P);
      }
    }
#pragma unroll
    for (int q = 0; q < 3; ++q) A.terms[static_cast<size_t>(p) * 3 + q] = term[q];
    sum += term[0] + term[1] + term[2];
  }
  const double total = consBlockSum(sum, red) / A.P;
  if (threadIdx.x == 0) A.total[0] = total;
}

template <typename T, int PIX>
inline __global__ __launch_bounds__(kConsThreads) void k_cons_backward(ConsArgs<T> A) {
  static_assert(PIX == 1 || PIX == 4, "one pixel or four consecutive pixels of a row per thread");
  const int pair = blockIdx.y, dir = blockIdx.z;
  const size_t npx = static_cast<size_t>(A.W) * A.H;
  const int2 ab = A.pairs[pair];
  if (!consPairOk(ab, A.F)) return;
  const double* cd = A.coef + (static_cast<size_t>(pair) * 2 + dir) * 3;
  const T cf[3] = {static_cast<T>(cd[0]), static_cast<T>(cd[1]), static_cast<T>(cd[2])};
  const int r = dir ? ab.y : ab.x, t = dir ? ab.x : ab.y;
  const ConsCam<T> c = consCam(A, r, t);
  const T* Dt = A.depth + static_cast<size_t>(t) * npx;
  T* gr = A.grad + static_cast<size_t>(r) * npx;
  T* gt = A.grad + static_cast<size_t>(t) * npx;
  const size_t i0 = (static_cast<size_t>(blockIdx.x) * kConsThreads + threadIdx.x) * PIX;
  if (i0 >= npx) return;
  const int y = static_cast<int>(i0 / A.W), x = static_cast<int>(i0 - static_cast<size_t>(y) * A.W);
  const ConsPixels<T, PIX> v = consLoadPixels<T, PIX>(A, pair, dir, r, npx, i0);
  consEachPixel<0, PIX>([&](auto kc) {
    constexpr int k = decltype(kc)::value;
    if (v.w.v[k] == T(0)) return;
    T gD, gTap[4];
    int tap[4];
    consSample<T, true>(A, c, Dt, x + k, y, v.D.v[k], v.wx.v[k], v.wy.v[k], v.fx.v[k], v.fy.v[k], v.w.v[k], cf, nullptr, gD, tap, gTap);
    if (gD != T(0)) consAtomicAdd(gr + i0 + k, gD);
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (gTap[j] != T(0)) consAtomicAdd(gt + tap[j], gTap[j]);
  });
}

template <typename T>
inline __global__ __launch_bounds__(kConsDetThreads) void k_cons_backward_det(ConsArgs<T> A) {
  const int f = blockIdx.x, lane = threadIdx.x;
  const size_t npx = static_cast<size_t>(A.W) * A.H;
  T* gf = A.grad + static_cast<size_t>(f) * npx;
  for (int pair = 0; pair < A.P; ++pair) {
    const int2 ab = A.pairs[pair];
    if (!consPairOk(ab, A.F) || (ab.x != f && ab.y != f)) continue;
    for (int dir = 0; dir < 2; ++dir) {
      const double* cd = A.coef + (static_cast<size_t>(pair) * 2 + dir) * 3;
      const T cf[3] = {static_cast<T>(cd[0]), static_cast<T>(cd[1]), static_cast<T>(cd[2])};
      const int r = dir ? ab.y : ab.x, t = dir ? ab.x : ab.y;
      const ConsCam<T> c = consCam(A, r, t);
      const T* Dt = A.depth + static_cast<size_t>(t) * npx;
      for (size_t base = 0; base < npx; base += kConsDetThreads) {
        const size_t i = base + lane;
        T gD = T(0), gTap[4] = {T(0), T(0), T(0), T(0)};
        int tap[4] = {0, 0, 0, 0};
        if (i < npx) {
          const ConsPixels<T, 1> v = consLoadPixels<T, 1>(A, pair, dir, r, npx, i);
          if (v.w.v[0] != T(0)) {
            const int y = static_cast<int>(i / A.W), x = static_cast<int>(i - static_cast<size_t>(y) * A.W);
            consSample<T, true>(A, c, Dt, x, y, v.D.v[0], v.wx.v[0], v.wy.v[0], v.fx.v[0], v.fy.v[0], v.w.v[0], cf, nullptr, gD, tap, gTap);
          }
        }
        if (r == f) {  // the lanes' pixels are distinct
          if (gD != T(0)) consAtomicAdd(gf + i, gD);
        } else {
          lossOrderedTaps(gf, lane, tap, gTap);
        }
      }
    }
  }
}

}  // namespace cvd
