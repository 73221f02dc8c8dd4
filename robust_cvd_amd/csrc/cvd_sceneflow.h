// Scene-flow loss of flow pairs and its gradient with respect to the depth maps: the reference's fine-tuning term SceneFlowLoss,
// loss/scene_flow_loss.py:31-356 with utils/geometry.py:38-137, 238-245 and utils/loss.py:62-80.  Templated on
// the precision T (float / double) of every real array.  The sibling of cvd_consistency.h; both build on cvd_loss_common.h.
//
// Tables: depth [F][H][W], extrinsics [F][3][4] = [R | t], intrinsics [F][4] = (fx, fy, cx, cy), optional warp [F][2][H][W] (pixel
// offsets, planar), pairs [P] = (a, b).  Static part, per direction k (0: a -> b on a's raster, 1: b -> a on b's): flow_k
// [P][2][H][W], mask_k [P][H][W].  Smooth part: neighbours [P][4] = (a-1, a+1, b-1, b+1) (a boundary anchor names itself), four
// flows nflow_j [P][2][H][W] and masks nmask_j [P][H][W] in that order, valid [P][2].
//   pix_f(x, y) = (x, y) + warp_f(x, y)
//   X_f(x, y)   = ray_f(pix_f) D_f(x, y),  ray = ((pix.x - cx) / fx, -(pix.y - cy) / fy, -1);   Xw_f = R_f X_f + t_f
//   S_f(m)      = bilinear sample of the three-channel map X_f at m (the tap rule of cvd_loss_common.h applied to ray(tap) D(tap))
//   term(rho, w) = sum_px w rho / max(sum_px w, 1e-6)
// Static, (pair, direction k), ref r, target t:  Y = R_t S_t(pix_r + flow_k) + t_t,  d = |Xw_r - Y|,  w = mask_k / |D_r|  (the
// weight depends on the depth and is differentiated),  static = lambda_static mean_k term(rho_s(d), w).
// Smooth, (pair, anchor al), frame r, neighbours n-, n+ (j = 2 al, 2 al + 1):  Y+- = R_n S_n(pix_r + nflow+-) + t_n,
// X_s = R_r^T (Y+ + Y- - Xw_r - t_r),  w = valid nmask- nmask+,  e_rep = |proj_r(X_s) - pix_r|,  e_dsp = 1 / X_s.z - 1 / X_r.z,
// e_rat = lambda_ratio log(min / max of |X_r.z|, |X_s.z|);  reproj = lambda mean_al term(rho_m(e_rep), w), disparity = lambda
// mean_al (fbar_al term(.)), depth ratio = mean_al term(.);  fbar_al = mean focal length of anchor al's frames over all pairs.
//
// k_sf_forward<T, PIX>    grid (blocks, P, 4), 256 threads; the classes z are static direction 0 / 1 and smooth anchor 0 / 1.  The
//                         cameras of (pair, class) are the same for the whole workgroup.  Per-workgroup f64 sums (sum w and up to
//                         three sum w rho) go to a slot of a slab; nothing is accumulated atomically.  With A.maps the six
//                         visualisation maps [6][P][3][H][W] are written (zeros for a class that does not exist).
// k_sf_finish_pairs       one wave per pair: sums the pair's slab slots in a fixed order (lossFinishPairs<4>).
// k_sf_finish_total       one workgroup: mean focal lengths, per-pair terms, total, and per (pair, class) the backward factors
//                         (static: d total / d sum w rho and d total / d sum w; smooth: d total / d sum w rho of the three terms).
// k_sf_backward<T, PIX>   the same walk; one hardware float atomic for D_r(x, y) (both paths of the static term in one add), one
//                         per bilinear tap of a sampled frame: the scalar weight_tap ray(tap) . (R^T g).
// k_sf_backward_det<T>    CVD_DETERMINISTIC: one wave per DESTINATION frame, (pair, class)s in order, taps one lane at a time.
// A pair or neighbour index outside [0, F), or a == b, is never dereferenced: its terms and the total come back NaN.
#pragma once
#include "cvd_loss_common.h"

namespace cvd {

template <typename T>
struct SfArgs {
  int F, P, W, H;
  int useStatic, useRep, useDsp, useRat;  // the term's lambda is > 0
  int nb;                                 // workgroups per (pair, class)
  T lamRat;
  ConsDistance<T> rhoS, rhoM;             // static / smooth distance
  const T* depth;
  const T* ext;
  const T* intr;
  const T* warp;                          // or null
  const int2* pairs;
  const int* nbrs;                        // [P][4]; null when no smooth term exists
  const T* flow[2];
  const T* mask[2];
  const T* nflow[4];
  const T* nmask[4];
  const T* valid;                         // [P][2]
  double* slab;                           // [P][4][nb][4]
  const double* coef;                     // [P][4][3]; backward only
  T* grad;                                // [F][H][W]; backward only
  T* maps;                                // [6][P][3][H][W] or null; forward only
};

struct SfFinishArgs {
  int F, P, nb;
  double lamStatic, lamRep, lamDsp, lamRat;  // lamRat: only its sign matters here
  const int2* pairs;
  const int* nbrs;
  double* slab;    // [P][4][nb][4]
  double* sums;    // [P][4][4]
  double* coef;    // [P][4][3]
  double* terms;   // [P][4]: static, smooth reproj, smooth disparity, smooth depth ratio
  double* total;   // [1]
};

// a frame's camera: [R | t] rows and (fx, fy, cx, cy)
template <typename T>
struct SfCam {
  T E[12];
  T fx, fy, cx, cy;
};

template <typename T>
__device__ __forceinline__ SfCam<T> sfCam(const SfArgs<T>& A, int f) {
  SfCam<T> c;
  const T* E = A.ext + static_cast<size_t>(f) * 12;
#pragma unroll
  for (int i = 0; i < 12; ++i) c.E[i] = E[i];
  const T* I = A.intr + static_cast<size_t>(f) * 4;
  c.fx = I[0]; c.fy = I[1]; c.cx = I[2]; c.cy = I[3];
  return c;
}

template <typename T>
struct SfVec3 {
  T x, y, z;
};

template <typename T>
__device__ __forceinline__ SfVec3<T> sfRot(const SfCam<T>& c, SfVec3<T> v) {  // R v
  return {c.E[0] * v.x + c.E[1] * v.y + c.E[2] * v.z, c.E[4] * v.x + c.E[5] * v.y + c.E[6] * v.z,
          c.E[8] * v.x + c.E[9] * v.y + c.E[10] * v.z};
}
template <typename T>
__device__ __forceinline__ SfVec3<T> sfRotT(const SfCam<T>& c, SfVec3<T> v) {  // R^T v
  return {c.E[0] * v.x + c.E[4] * v.y + c.E[8] * v.z, c.E[1] * v.x + c.E[5] * v.y + c.E[9] * v.z,
          c.E[2] * v.x + c.E[6] * v.y + c.E[10] * v.z};
}

// the four bilinear taps of one sampled point: index into the frame's maps, weight (0 outside the image), ray (x, y; z = -1)
template <typename T>
struct SfTaps {
  int idx[4];
  T wt[4], rx[4], ry[4];
};

// S_f(m) of frame f with camera c; Df / wf = the frame's depth map / warp planes (wf may be null)
template <typename T>
__device__ __forceinline__ SfVec3<T> sfSample(const SfArgs<T>& A, const SfCam<T>& c, const T* __restrict__ Df,
                                               const T* __restrict__ wf, T mx, T my, SfTaps<T>& tp) {
  const LossTaps<T> bt = lossBilinearTaps(A.W, A.H, mx, my);
  const int xs[4] = {bt.x[0], bt.x[1], bt.x[0], bt.x[1]}, ys[4] = {bt.y[0], bt.y[0], bt.y[1], bt.y[1]};
  const size_t npx = static_cast<size_t>(A.W) * A.H;
  SfVec3<T> S{T(0), T(0), T(0)};
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int i = bt.idx[j];
    tp.idx[j] = i;
    tp.wt[j] = bt.wt[j];
    T px = static_cast<T>(xs[j]), py = static_cast<T>(ys[j]);
    if (wf) {
      px += wf[i];
      py += wf[npx + i];
    }
    tp.rx[j] = (px - c.cx) / c.fx;
    tp.ry[j] = -(py - c.cy) / c.fy;
    const T wd = tp.wt[j] * Df[i];
    S.x += tp.rx[j] * wd;
    S.y += tp.ry[j] * wd;
    S.z -= wd;
  }
  return S;
}

// d total / d D_f(tap j) for the gradient u (in f's camera) of the sampled point
template <typename T>
__device__ __forceinline__ T sfTapGrad(const SfTaps<T>& tp, int j, SfVec3<T> u) {
  return tp.wt[j] * (tp.rx[j] * u.x + tp.ry[j] * u.y - u.z);
}

// The frames of (pair, class): r = ref / anchor, s0 = target or n-, s1 = n+ (smooth only).  false: an index is out of range.
struct SfFrames {
  int r, s0, s1;
};

template <typename T>
__device__ __forceinline__ bool sfFrames(const SfArgs<T>& A, int pair, int cls, SfFrames& f) {
  const int2 ab = A.pairs[pair];
  if (!consPairOk(ab, A.F)) return false;
  if (cls < 2) {
    f.r = cls ? ab.y : ab.x;
    f.s0 = f.s1 = cls ? ab.x : ab.y;
    return true;
  }
  const int al = cls - 2;
  f.r = al ? ab.y : ab.x;
  f.s0 = A.nbrs[pair * 4 + 2 * al];
  f.s1 = A.nbrs[pair * 4 + 2 * al + 1];
  return f.s0 >= 0 && f.s0 < A.F && f.s1 >= 0 && f.s1 < A.F;
}

template <typename T>
__device__ __forceinline__ bool sfClassOn(const SfArgs<T>& A, int cls) {
  return cls < 2 ? A.useStatic != 0 : (A.useRep | A.useDsp | A.useRat) != 0;
}

// Static sample.  Forward (GRAD = false): adds (w, w rho) to acc and writes the map entry.  Backward: cf = (d total / d sum w rho,
// d total / d sum w); gD = d total / d D_r(x, y) through X_r and through w; gTap[j] for the taps tp of the target frame.
template <typename T, bool GRAD>
__device__ __forceinline__ void sfStatic(const SfArgs<T>& A, const SfCam<T>& cr, const SfCam<T>& ct, const T* __restrict__ Dt,
                                         const T* __restrict__ wt, int x, int y, T D, T wx, T wy, T fx, T fy, T m, const T* cf,
                                         double* acc, T* map, size_t npx, T& gD, SfTaps<T>& tp, T* gTap) {
  const T px = static_cast<T>(x) + wx, py = static_cast<T>(y) + wy;
  const SfVec3<T> ray{(px - cr.cx) / cr.fx, -(py - cr.cy) / cr.fy, T(-1)};
  const SfVec3<T> a = sfRot(cr, ray);  // d Xw_r / d D_r
  const SfVec3<T> S = sfSample(A, ct, Dt, wt, px + fx, py + fy, tp);
  const SfVec3<T> Y = sfRot(ct, S);
  const SfVec3<T> v{a.x * D + cr.E[3] - (Y.x + ct.E[3]), a.y * D + cr.E[7] - (Y.y + ct.E[7]), a.z * D + cr.E[11] - (Y.z + ct.E[11])};
  const T d = consSqrt(v.x * v.x + v.y * v.y + v.z * v.z);
  const T w = m * consAbs(T(1) / (-D));
  T dr;
  const T r = consRhoOf(A.rhoS, d, dr);
  if (!GRAD) {
    acc[0] += static_cast<double>(w);
    acc[1] += static_cast<double>(w * r);
    if (map) {
      map[0] = w * v.x; map[npx] = w * v.y; map[2 * npx] = w * v.z;
    }
  } else {
    const T dw = -w / D;  // d (m / |D|) / d D
    T g = (cf[0] * r + cf[1]) * dw;
    SfVec3<T> u{T(0), T(0), T(0)};
    if (d > T(0)) {
      const T k = cf[0] * w * dr / d;
      const SfVec3<T> gv{k * v.x, k * v.y, k * v.z};
      g += gv.x * a.x + gv.y * a.y + gv.z * a.z;
      u = sfRotT(ct, gv);
    }
    gD = g;
#pragma unroll
    for (int j = 0; j < 4; ++j) gTap[j] = -sfTapGrad(tp, j, u);
  }
}

// Smooth sample of one anchor.  Forward: adds (w, w rho_rep, w rho_dsp, w rho_rat) to acc, writes both map entries (mapF: n+,
// mapB: n-).  Backward: cf = the three factors; gD, and gTap0 / gTap1 for the taps tp0 / tp1 of n- / n+.
template <typename T, bool GRAD>
__device__ __forceinline__ void sfSmooth(const SfArgs<T>& A, const SfCam<T>& cr, const SfCam<T>& c0, const SfCam<T>& c1,
                                         const T* __restrict__ D0, const T* __restrict__ w0, const T* __restrict__ D1,
                                         const T* __restrict__ w1, int x, int y, T D, T wx, T wy, T f0x, T f0y, T f1x, T f1y, T w,
                                         const T* cf, double* acc, T* mapF, T* mapB, size_t npx, T& gD, SfTaps<T>& tp0, T* gTap0,
                                         SfTaps<T>& tp1, T* gTap1) {
  const T px = static_cast<T>(x) + wx, py = static_cast<T>(y) + wy;
  const SfVec3<T> ray{(px - cr.cx) / cr.fx, -(py - cr.cy) / cr.fy, T(-1)};
  const SfVec3<T> Xr{ray.x * D, ray.y * D, -D};
  const SfVec3<T> RX = sfRot(cr, Xr);
  const SfVec3<T> Xw{RX.x + cr.E[3], RX.y + cr.E[7], RX.z + cr.E[11]};
  const SfVec3<T> S0 = sfSample(A, c0, D0, w0, px + f0x, py + f0y, tp0);
  const SfVec3<T> S1 = sfSample(A, c1, D1, w1, px + f1x, py + f1y, tp1);
  const SfVec3<T> R0 = sfRot(c0, S0), R1 = sfRot(c1, S1);
  const SfVec3<T> Ym{R0.x + c0.E[3], R0.y + c0.E[7], R0.z + c0.E[11]}, Yp{R1.x + c1.E[3], R1.y + c1.E[7], R1.z + c1.E[11]};
  const SfVec3<T> sp{Yp.x - Xw.x, Yp.y - Xw.y, Yp.z - Xw.z}, sm{Ym.x - Xw.x, Ym.y - Xw.y, Ym.z - Xw.z};  // scene flow fw / bw
  // Xw + (sp + sm) - t_r, back in r's camera
  const SfVec3<T> Q{Xw.x + (sp.x + sm.x) - cr.E[3], Xw.y + (sp.y + sm.y) - cr.E[7], Xw.z + (sp.z + sm.z) - cr.E[11]};
  const SfVec3<T> Xs = sfRotT(cr, Q);
  const T Z = Xs.z, Zr = Xr.z;
  if (!GRAD) {
    acc[0] += static_cast<double>(w);
    if (mapF) {
      mapF[0] = w * sp.x; mapF[npx] = w * sp.y; mapF[2 * npx] = w * sp.z;
      mapB[0] = w * sm.x; mapB[npx] = w * sm.y; mapB[2 * npx] = w * sm.z;
    }
  }
  T g = T(0);                        // d total / d D_r not through X_s
  SfVec3<T> gs{T(0), T(0), T(0)};    // d total / d X_s
  if (A.useRep) {
    const T nz = -Z;
    const T dx = (Xs.x / nz) * cr.fx + cr.cx - px;
    const T dy = -((Xs.y / nz) * cr.fy) + cr.cy - py;
    const T e = consSqrt(dx * dx + dy * dy);
    T dr;
    const T r = consRhoOf(A.rhoM, e, dr);
    if (!GRAD) acc[1] += static_cast<double>(w * r);
    else if (e > T(0)) {
      const T k = cf[0] * w * dr / e;
      const T kx = k * dx * cr.fx, ky = k * dy * cr.fy;
      gs.x += -kx / Z;
      gs.y += ky / Z;
      gs.z += (kx * Xs.x - ky * Xs.y) / (Z * Z);
    }
  }
  if (A.useDsp) {
    const T e = T(1) / Z - T(1) / Zr;
    T dr;
    const T r = consRhoOf(A.rhoM, e, dr);
    if (!GRAD) acc[2] += static_cast<double>(w * r);
    else {
      const T k = cf[1] * w * dr;
      gs.z += -k / (Z * Z);
      g += -k / (Zr * Zr);   // d (-1 / Zr) / d D = -1 / D^2
    }
  }
  if (A.useRat) {
    const T p = consAbs(Zr), q = consAbs(Z);
    const T e = A.lamRat * consLog((p < q ? p : q) / (p < q ? q : p));
    T dr;
    const T r = consRhoOf(A.rhoM, e, dr);
    if (!GRAD) acc[3] += static_cast<double>(w * r);
    else {
      const T sg = p < q ? T(1) : (p > q ? T(-1) : T(0));
      const T k = cf[2] * w * dr * sg * A.lamRat;
      g += k / D;
      gs.z += -k / Z;
    }
  }
  if (GRAD) {
    const SfVec3<T> gw = sfRot(cr, gs);  // d total / d Y+ = d total / d Y-
    const SfVec3<T> a = sfRot(cr, ray);  // d X_s / d D_r = -R_r^T R_r ray (R_r as given: not assumed orthogonal to rounding)
    gD = g - (gw.x * a.x + gw.y * a.y + gw.z * a.z);
    const SfVec3<T> u0 = sfRotT(c0, gw), u1 = sfRotT(c1, gw);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      gTap0[j] = sfTapGrad(tp0, j, u0);
      gTap1[j] = sfTapGrad(tp1, j, u1);
    }
  }
}

// The inputs of a thread's PIX pixels of (pair, class); ref frame r.  Static: f0 = flow, m0 = mask.  Smooth: f0 / f1 = nflow-/+,
// m0 = valid nmask- nmask+.
template <typename T, int PIX>
struct SfPixels {
  ConsVals<T, PIX> D, wx, wy, f0x, f0y, f1x, f1y, m0;
};

template <typename T, int PIX>
__device__ __forceinline__ SfPixels<T, PIX> sfLoadPixels(const SfArgs<T>& A, int pair, int cls, int r, size_t npx, size_t i0) {
  SfPixels<T, PIX> v;
  v.D = consLoad<T, PIX>(A.depth + static_cast<size_t>(r) * npx, i0);
  ConsVals<T, PIX> zero;
#pragma unroll
  for (int k = 0; k < PIX; ++k) zero.v[k] = T(0);
  v.wx = v.wy = v.f1x = v.f1y = zero;
  if (A.warp) {
    const T* wp = A.warp + static_cast<size_t>(r) * 2 * npx;
    v.wx = consLoad<T, PIX>(wp, i0);
    v.wy = consLoad<T, PIX>(wp + npx, i0);
  }
  if (cls < 2) {
    const T* fl = A.flow[cls] + static_cast<size_t>(pair) * 2 * npx;
    v.f0x = consLoad<T, PIX>(fl, i0);
    v.f0y = consLoad<T, PIX>(fl + npx, i0);
    v.m0 = consLoad<T, PIX>(A.mask[cls] + static_cast<size_t>(pair) * npx, i0);
  } else {
    const int j = 2 * (cls - 2);
    const T* f0 = A.nflow[j] + static_cast<size_t>(pair) * 2 * npx;
    const T* f1 = A.nflow[j + 1] + static_cast<size_t>(pair) * 2 * npx;
    v.f0x = consLoad<T, PIX>(f0, i0);
    v.f0y = consLoad<T, PIX>(f0 + npx, i0);
    v.f1x = consLoad<T, PIX>(f1, i0);
    v.f1y = consLoad<T, PIX>(f1 + npx, i0);
    const ConsVals<T, PIX> ma = consLoad<T, PIX>(A.nmask[j] + static_cast<size_t>(pair) * npx, i0);
    const ConsVals<T, PIX> mb = consLoad<T, PIX>(A.nmask[j + 1] + static_cast<size_t>(pair) * npx, i0);
    const T vl = A.valid[pair * 2 + (cls - 2)];
#pragma unroll
    for (int k = 0; k < PIX; ++k) v.m0.v[k] = vl * ma.v[k] * mb.v[k];
  }
  return v;
}

template <typename T, int PIX>
inline __global__ __launch_bounds__(kConsThreads) void k_sf_forward(SfArgs<T> A) {
  static_assert(PIX == 1 || PIX == 4, "one pixel or four consecutive pixels of a row per thread");
  const int pair = blockIdx.y, cls = blockIdx.z;
  const size_t npx = static_cast<size_t>(A.W) * A.H;
  double* slot = A.slab + ((static_cast<size_t>(pair) * 4 + cls) * A.nb + blockIdx.x) * 4;
  const size_t i0 = (static_cast<size_t>(blockIdx.x) * kConsThreads + threadIdx.x) * PIX;
  // the maps of this class: static k -> map k; anchor al -> maps 2 + 2 al (n+) and 3 + 2 al (n-)
  const size_t mapStride = static_cast<size_t>(A.P) * 3 * npx;
  T* mapA = A.maps ? A.maps + (cls < 2 ? cls : 2 * cls - 2) * mapStride + static_cast<size_t>(pair) * 3 * npx : nullptr;
  T* mapB = A.maps ? mapA + mapStride : nullptr;
  SfFrames fr;
  const bool on = sfClassOn(A, cls);
  if (!on || !sfFrames(A, pair, cls, fr)) {  // (the whole workgroup)
    if (threadIdx.x < 4) slot[threadIdx.x] = on ? __builtin_nan("") : 0.0;
    if (mapA && i0 < npx) {
      const T fill = on ? static_cast<T>(__builtin_nan("")) : T(0);
#pragma unroll
      for (int k = 0; k < PIX; ++k)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          mapA[c * npx + i0 + k] = fill;
          if (cls >= 2) mapB[c * npx + i0 + k] = fill;
        }
    }
    return;
  }
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  if (i0 < npx) {  // (PIX = 4: npx % 4 == 0, a thread's four pixels are all inside or all outside and share a row)
    const int y = static_cast<int>(i0 / A.W), x = static_cast<int>(i0 - static_cast<size_t>(y) * A.W);
    const SfPixels<T, PIX> v = sfLoadPixels<T, PIX>(A, pair, cls, fr.r, npx, i0);
    const SfCam<T> cr = sfCam(A, fr.r), c0 = sfCam(A, fr.s0);
    const T* D0 = A.depth + static_cast<size_t>(fr.s0) * npx;
    const T* w0 = A.warp ? A.warp + static_cast<size_t>(fr.s0) * 2 * npx : nullptr;
    if (cls < 2) {
      consEachPixel<0, PIX>([&](auto kc) {
        constexpr int k = decltype(kc)::value;
        T gD;
        SfTaps<T> tp;
        sfStatic<T, false>(A, cr, c0, D0, w0, x + k, y, v.D.v[k], v.wx.v[k], v.wy.v[k], v.f0x.v[k], v.f0y.v[k], v.m0.v[k], nullptr,
                           acc, mapA ? mapA + i0 + k : nullptr, npx, gD, tp, nullptr);
      });
    } else {
      const SfCam<T> c1 = sfCam(A, fr.s1);
      const T* D1 = A.depth + static_cast<size_t>(fr.s1) * npx;
      const T* w1 = A.warp ? A.warp + static_cast<size_t>(fr.s1) * 2 * npx : nullptr;
      consEachPixel<0, PIX>([&](auto kc) {
        constexpr int k = decltype(kc)::value;
        T gD;
        SfTaps<T> tp0, tp1;
        sfSmooth<T, false>(A, cr, c0, c1, D0, w0, D1, w1, x + k, y, v.D.v[k], v.wx.v[k], v.wy.v[k], v.f0x.v[k], v.f0y.v[k],
                           v.f1x.v[k], v.f1y.v[k], v.m0.v[k], nullptr, acc, mapA ? mapA + i0 + k : nullptr,
                           mapB ? mapB + i0 + k : nullptr, npx, gD, tp0, nullptr, tp1, nullptr);
      });
    }
  }
  double s;
  if (lossFoldWorkgroup(acc, s)) slot[threadIdx.x] = s;
}

inline __global__ __launch_bounds__(64) void k_sf_finish_pairs(SfFinishArgs A) { lossFinishPairs<4>(A.slab, A.sums, A.nb); }

template <typename T>
inline __global__ __launch_bounds__(kConsThreads) void k_sf_finish_total(SfFinishArgs A, const T* __restrict__ intr) {
  __shared__ double red[kConsThreads];
  // fbar[al]: mean of (fx, fy) over anchor al's frames of ALL pairs (the reference's torch.mean over the batch)
  double f0 = 0.0, f1 = 0.0;
  for (int p = threadIdx.x; p < A.P; p += kConsThreads) {
    const int2 ab = A.pairs[p];
    if (!consPairOk(ab, A.F)) {  // its terms are NaN through the slab; the mean focal length does not exist either, so the
      f0 = f1 = __builtin_nan("");  // disparity term of every pair is NaN rather than scaled by a mean over the other pairs
      continue;
    }
    f0 += static_cast<double>(intr[static_cast<size_t>(ab.x) * 4]) + static_cast<double>(intr[static_cast<size_t>(ab.x) * 4 + 1]);
    f1 += static_cast<double>(intr[static_cast<size_t>(ab.y) * 4]) + static_cast<double>(intr[static_cast<size_t>(ab.y) * 4 + 1]);
  }
  const double fbar[2] = {consBlockSum(f0, red) / (2.0 * A.P), consBlockSum(f1, red) / (2.0 * A.P)};
  double sum = 0.0;
  for (int p = threadIdx.x; p < A.P; p += kConsThreads) {
    double term[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const double* s = A.sums + (static_cast<size_t>(p) * 4 + k) * 4;
      double* cf = A.coef + (static_cast<size_t>(p) * 4 + k) * 3;
      const double n = fmax(s[0], 1e-6);
      term[0] += 0.5 * A.lamStatic * (s[1] / n);
      cf[0] = 0.5 * A.lamStatic / (n * A.P);
      cf[1] = s[0] >= 1e-6 ? -cf[0] * (s[1] / n) : 0.0;  // (the clamp passes no gradient to sum w)
      cf[2] = 0.0;
    }
#pragma unroll
    for (int al = 0; al < 2; ++al) {
      const double* s = A.sums + (static_cast<size_t>(p) * 4 + 2 + al) * 4;
      double* cf = A.coef + (static_cast<size_t>(p) * 4 + 2 + al) * 3;
      const double n = fmax(s[0], 1e-6);
      const double lam[3] = {A.lamRep, A.lamDsp > 0.0 ? A.lamDsp * fbar[al] : 0.0, A.lamRat > 0.0 ? 1.0 : 0.0};
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        term[1 + q] += 0.5 * lam[q] * (s[1 + q] / n);
        cf[q] = 0.5 * lam[q] / (n * A.P);
      }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) A.terms[static_cast<size_t>(p) * 4 + q] = term[q];
    sum += term[0] + term[1] + term[2] + term[3];
  }
  const double total = consBlockSum(sum, red) / A.P;
  if (threadIdx.x == 0) A.total[0] = total;
}

// The gradient of one sample of (pair, class) at pixel i = (x, y): gD for D_r(i), gTap0 / gTap1 for the taps of s0 / s1 (gTap1 = 0
// for a static class).  All zero for a zero-weight sample.
template <typename T>
__device__ __forceinline__ void sfSampleGrad(const SfArgs<T>& A, int cls, const SfFrames& fr, const T* cf, size_t npx, int x,
                                             int y, T D, T wx, T wy, T f0x, T f0y, T f1x, T f1y, T m, T& gD, SfTaps<T>& tp0,
                                             T* gTap0, SfTaps<T>& tp1, T* gTap1) {
  gD = T(0);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    gTap0[j] = gTap1[j] = T(0);
    tp0.idx[j] = tp1.idx[j] = 0;
  }
  if (m == T(0)) return;
  const SfCam<T> cr = sfCam(A, fr.r), c0 = sfCam(A, fr.s0);
  const T* D0 = A.depth + static_cast<size_t>(fr.s0) * npx;
  const T* w0 = A.warp ? A.warp + static_cast<size_t>(fr.s0) * 2 * npx : nullptr;
  if (cls < 2) {
    sfStatic<T, true>(A, cr, c0, D0, w0, x, y, D, wx, wy, f0x, f0y, m, cf, nullptr, nullptr, npx, gD, tp0, gTap0);
  } else {
    const SfCam<T> c1 = sfCam(A, fr.s1);
    const T* D1 = A.depth + static_cast<size_t>(fr.s1) * npx;
    const T* w1 = A.warp ? A.warp + static_cast<size_t>(fr.s1) * 2 * npx : nullptr;
    sfSmooth<T, true>(A, cr, c0, c1, D0, w0, D1, w1, x, y, D, wx, wy, f0x, f0y, f1x, f1y, m, cf, nullptr, nullptr, nullptr, npx,
                      gD, tp0, gTap0, tp1, gTap1);
  }
}

template <typename T, int PIX>
inline __global__ __launch_bounds__(kConsThreads) void k_sf_backward(SfArgs<T> A) {
  static_assert(PIX == 1 || PIX == 4, "one pixel or four consecutive pixels of a row per thread");
  const int pair = blockIdx.y, cls = blockIdx.z;
  const size_t npx = static_cast<size_t>(A.W) * A.H;
  SfFrames fr;
  if (!sfClassOn(A, cls) || !sfFrames(A, pair, cls, fr)) return;
  const double* cd = A.coef + (static_cast<size_t>(pair) * 4 + cls) * 3;
  const T cf[3] = {static_cast<T>(cd[0]), static_cast<T>(cd[1]), static_cast<T>(cd[2])};
  T* gr = A.grad + static_cast<size_t>(fr.r) * npx;
  T* g0 = A.grad + static_cast<size_t>(fr.s0) * npx;
  T* g1 = A.grad + static_cast<size_t>(fr.s1) * npx;
  const size_t i0 = (static_cast<size_t>(blockIdx.x) * kConsThreads + threadIdx.x) * PIX;
  if (i0 >= npx) return;
  const int y = static_cast<int>(i0 / A.W), x = static_cast<int>(i0 - static_cast<size_t>(y) * A.W);
  const SfPixels<T, PIX> v = sfLoadPixels<T, PIX>(A, pair, cls, fr.r, npx, i0);
  consEachPixel<0, PIX>([&](auto kc) {
    constexpr int k = decltype(kc)::value;
    if (v.m0.v[k] == T(0)) return;
    T gD, gTap0[4], gTap1[4];
    SfTaps<T> tp0, tp1;
    sfSampleGrad(A, cls, fr, cf, npx, x + k, y, v.D.v[k], v.wx.v[k], v.wy.v[k], v.f0x.v[k], v.f0y.v[k], v.f1x.v[k], v.f1y.v[k],
                 v.m0.v[k], gD, tp0, gTap0, tp1, gTap1);
    if (gD != T(0)) consAtomicAdd(gr + i0 + k, gD);
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (gTap0[j] != T(0)) consAtomicAdd(g0 + tp0.idx[j], gTap0[j]);
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (gTap1[j] != T(0)) consAtomicAdd(g1 + tp1.idx[j], gTap1[j]);
  });
}

template <typename T>
inline __global__ __launch_bounds__(kConsDetThreads) void k_sf_backward_det(SfArgs<T> A) {
  const int f = blockIdx.x, lane = threadIdx.x;
  const size_t npx = static_cast<size_t>(A.W) * A.H;
  T* gf = A.grad + static_cast<size_t>(f) * npx;
  for (int pair = 0; pair < A.P; ++pair) {
    for (int cls = 0; cls < 4; ++cls) {
      SfFrames fr;
      if (!sfClassOn(A, cls) || !sfFrames(A, pair, cls, fr)) continue;
      if (fr.r != f && fr.s0 != f && fr.s1 != f) continue;
      const double* cd = A.coef + (static_cast<size_t>(pair) * 4 + cls) * 3;
      const T cf[3] = {static_cast<T>(cd[0]), static_cast<T>(cd[1]), static_cast<T>(cd[2])};
      for (size_t base = 0; base < npx; base += kConsDetThreads) {
        const size_t i = base + lane;
        T gD = T(0), gTap0[4] = {T(0), T(0), T(0), T(0)}, gTap1[4] = {T(0), T(0), T(0), T(0)};
        SfTaps<T> tp0, tp1;
#pragma unroll
        for (int j = 0; j < 4; ++j) tp0.idx[j] = tp1.idx[j] = 0;
        if (i < npx) {
          const SfPixels<T, 1> v = sfLoadPixels<T, 1>(A, pair, cls, fr.r, npx, i);
          const int y = static_cast<int>(i / A.W), x = static_cast<int>(i - static_cast<size_t>(y) * A.W);
          sfSampleGrad(A, cls, fr, cf, npx, x, y, v.D.v[0], v.wx.v[0], v.wy.v[0], v.f0x.v[0], v.f0y.v[0], v.f1x.v[0], v.f1y.v[0],
                       v.m0.v[0], gD, tp0, gTap0, tp1, gTap1);
        }
        if (fr.r == f && gD != T(0)) consAtomicAdd(gf + i, gD);  // the lanes' pixels are distinct
        if (fr.s0 == f) lossOrderedTaps(gf, lane, tp0.idx, gTap0);
        if (cls >= 2 && fr.s1 == f) lossOrderedTaps(gf, lane, tp1.idx, gTap1);
      }
    }
  }
}

}  // namespace cvd
