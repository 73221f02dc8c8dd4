// cvd_cost.h -- candidate-point cost of an LM step and the step's statistics (kernel map: cvd_kernels.h).
#pragma once

#include "cvd_kernels.h"

namespace cvd {

// ---------------------------------------------------------------------------------------------------
// candidate-point cost: pair-major over work items
// ---------------------------------------------------------------------------------------------------
template <int KD, int KS>
inline __global__ __launch_bounds__(256) void k_cost_items(Layout L, Table T, Items it, const double* __restrict__ x,
                                                    const FrameConst* __restrict__ fc, double* __restrict__ costItem) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  const int B = L.B;
  double* xa = sm;
  double* xb = sm + B;
  FrameConst* fcs = reinterpret_cast<FrameConst*>(sm + 2 * B);
  double* red = reinterpret_cast<double*>(fcs + 2);
  const int item = blockIdx.x;
  const int fa = it.fa[item], fb = it.fb[item];
  for (int i = threadIdx.x; i < B; i += blockDim.x) {
    xa[i] = x[static_cast<size_t>(fa) * B + i];
    xb[i] = x[static_cast<size_t>(fb) * B + i];
  }
  if (threadIdx.x < 2 * (sizeof(FrameConst) / 8)) {
    const int which = threadIdx.x / (sizeof(FrameConst) / 8);
    const int k = threadIdx.x % (sizeof(FrameConst) / 8);
    reinterpret_cast<double*>(fcs + which)[k] = reinterpret_cast<const double*>(fc + (which ? fb : fa))[k];
  }
  __syncthreads();
  double acc = 0.0;
  for (int dir = 0; dir < 2; ++dir) {
    const long long cb = it.range[item * 4 + dir * 2], ce = it.range[item * 4 + dir * 2 + 1];
    const FrameConst& Fs = fcs[dir];
    const FrameConst& Ft = fcs[dir ^ 1];
    const double* xs = dir ? xb : xa;
    const double* xt = dir ? xa : xb;
    for (long long c = cb + threadIdx.x; c < ce; c += blockDim.x) {
      const float2 d = T.dsrc[c];
      if (d.x > 0.f) {
        Sample<KD, KS> s;
        evalSample<KD, KS, false>(L, Fs, Ft, xs, xt, T.ndc[c], d, s);
        acc += s.rho0;
      }
    }
  }
  acc = waveSum(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
    for (int w = 0; w < (blockDim.x >> 6); ++w) t += red[w];
    costItem[item] = 0.5 * t;
  }
}

template <int KD>
inline __global__ __launch_bounds__(256) void k_cost_frames(Layout L, const double* __restrict__ x,
                                                     const float* __restrict__ median,
                                                     const unsigned char* __restrict__ inRange,
                                                     const unsigned char* __restrict__ rangeFlags,
                                                     double* __restrict__ costFrame) {
  // (the frame's parameters go through LDS: every residual would otherwise start with its own dependent global load)
  extern __shared__ __attribute__((aligned(16))) double sm[];
  __shared__ double red[4];
  const int f = blockIdx.x;
  double acc = 0.0;
  if (threadIdx.x == 0 && L.positionRegSqrt > 0.0) {
    double o3[3] = {0, 0, 0}, dg = 0.0, cst = 0.0;
    if (posRegValid(L, rangeFlags, f)) posRegFrame(L, rangeFlags, f, x, nullptr, o3, dg, cst);
    acc += cst;
  }
  const bool active = inRange[f] != 0;
  if (active)
    for (int i = threadIdx.x; i < L.B; i += 256) sm[i] = x[static_cast<size_t>(f) * L.B + i];
  __syncthreads();
  if (active) {
    const float med = median[f];
    const int nr = numRegResiduals<KD>(L);
    for (int i = threadIdx.x; i < nr; i += 256) {
      double r;
      int n;
      int cols[2 * KD + 2];
      double jac[2 * KD + 2];
      regResidual<KD>(L, f, i, sm, med, r, n, cols, jac);
      acc += r * r;
    }
  }
  acc = waveSum(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) costFrame[f] = 0.5 * ((red[0] + red[1]) + (red[2] + red[3]));
}

// deterministic final sum: out[slot] = sum(a[0..na)) + sum(b[0..nb))
inline __global__ __launch_bounds__(256) void k_sum2(const double* __restrict__ a, int na, const double* __restrict__ b,
                                              int nb, double* __restrict__ out, int slot) {
  __shared__ double red[4];
  double acc = 0.0;
  for (int i = threadIdx.x; i < na; i += 256) acc += a[i];
  for (int i = threadIdx.x; i < nb; i += 256) acc += b[i];
  acc = waveSum(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) out[slot] = red[0] + red[1] + red[2] + red[3];
}

// Candidate-point cost on the fast path (same scope as k_matvec_pairs_fast: identity spatial transform, reprojection
// losses): the residual chain of the fast kernels with register-resident taps.  The generic k_cost_items keeps the taps
// of Sample<KD, KS> in dynamically indexed arrays, i.e. in scratch memory (672 B per lane, stores and dependent reloads
// per constraint): 53 us for 1.09 M constraints where the arithmetic needs ~10.
template <int KD, bool DENSE = false>
inline __global__ __launch_bounds__(256) void k_cost_items_fast(Layout L, Table T, Items it, const double* __restrict__ x,
                                                         const FrameConst* __restrict__ fc, double* __restrict__ costItem) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  const int B = L.B;
  double* xa = sm;
  double* xb = sm + B;
  FrameConst* fcs = reinterpret_cast<FrameConst*>(sm + 2 * B);
  double* red = reinterpret_cast<double*>(fcs + 2);
  const int item = blockIdx.x;
  const int tid = threadIdx.x;
  const int fa = it.fa[item], fb = it.fb[item];
  for (int i = tid; i < B; i += 256) {
    xa[i] = x[static_cast<size_t>(fa) * B + i];
    xb[i] = x[static_cast<size_t>(fb) * B + i];
  }
  constexpr int FCW = sizeof(FrameConst) / 8;
  if (tid < 2 * FCW) {
    const int which = tid / FCW, k = tid % FCW;
    reinterpret_cast<double*>(fcs + which)[k] = reinterpret_cast<const double*>(fc + (which ? fb : fa))[k];
  }
  __syncthreads();
  const int N = L.N;
  const double A = L.aspect;
  double acc = 0.0;
  for (int dir = 0; dir < 2; ++dir) {
    const long long cb = it.range[item * 4 + dir * 2], ce = it.range[item * 4 + dir * 2 + 1];
    const FrameConst& Fa = fcs[dir];
    const FrameConst& Fb = fcs[dir ^ 1];
    const double* xs = dir ? xb : xa;
    const double* xt = dir ? xa : xb;
    const double fya = Fa.fy, fxa = Fa.fy * A;
    const double fyb = Fb.fy;
    const double ifyb = 1.0 / fyb, ifxb = 1.0 / (fyb * A);
    const int fsrc = dir ? fb : fa, ftgt = dir ? fa : fb;
    const long long pixBase = DENSE ? (cb / (static_cast<long long>(T.W) * T.H)) * (static_cast<long long>(T.W) * T.H) : 0;
    std::conditional_t<DENSE, DenseStreamAhead, RecordStream<false>> rs;
    const int nDir = static_cast<int>(ce - cb);
    if constexpr (DENSE) rs.prime(T, cb, tid, 256, nDir, pixBase, fsrc, ftgt);
    else rs.prime(T, cb, tid, nDir);
    for (int ci = tid; ci < nDir; ci += 256) {
      float4 nd;
      float2 d;
      if (!rs.take(T, cb, ci, 256, nDir, pixBase, fsrc, ftgt, nd, d)) continue;
      const double da = static_cast<double>(d.x), db = static_cast<double>(d.y);
      double Da, Db;
      if (N == 0) {
        Da = da;
        Db = db;
      } else {
        FastTaps<KD> ta, tb;
        fastGather<KD>(L, nd.x, nd.y, ta);
        fastGather<KD>(L, nd.z, nd.w, tb);
        Da = 0.0;
        Db = 0.0;
#pragma unroll
        for (int k = 0; k < KD; ++k) {
          if (ta.ok(k)) {
            const int ia = ta.I(k);
            const double wa = ta.Wt(k);
            Da += (N == 2 ? da * xs[7 + ia * 2] + xs[7 + ia * 2 + 1] : da * xs[7 + ia]) * wa;
          }
          if (tb.ok(k)) {
            const int ib = tb.I(k);
            const double wb = tb.Wt(k);
            Db += (N == 2 ? db * xt[7 + ib * 2] + xt[7 + ib * 2 + 1] : db * xt[7 + ib]) * wb;
          }
        }
      }
      const double pax = static_cast<double>(nd.x), pay = static_cast<double>(nd.y);
      const double pbx = static_cast<double>(nd.z), pby = static_cast<double>(nd.w);
      double ca[3], Rca[3];
      fastRay(Fa.R, pax, pay, fxa, fya, ca, Rca);
      const double v[3] = {Fa.t[0] + Rca[0] * Da - Fb.t[0], Fa.t[1] + Rca[1] * Da - Fb.t[1], Fa.t[2] + Rca[2] * Da - Fb.t[2]};
      double zz, iz, u, vv, r0, r1, r2, dr2dA, dr2dDb;
      fastProject<false>(L, Fb.R, v, ifxb, ifyb, pbx, pby, zz, iz, u, vv, r0, r1);
      fastDepthResidual<false>(L, L.lossType, zz, iz, Db, r2, dr2dA, dr2dDb);  // (value only: the derivatives drop out)
      double rho0, rho1;
      robustRho(L, r0 * r0 + r1 * r1 + r2 * r2, rho0, rho1);
      acc += rho0;
    }
  }
  acc = waveSum(acc);
  if ((tid & 63) == 0) red[tid >> 6] = acc;
  __syncthreads();
  if (tid == 0) costItem[item] = 0.5 * ((red[0] + red[1]) + (red[2] + red[3]));
}

// Step statistics (one block): d.g, d.r, d.(lam d), |d|^2, |x|^2 (active unknowns), max |g|, and the number of active unknowns
// (entries of diag(H) that are not zero: what the host used to count from a downloaded copy at the start of every solve).
inline __global__ __launch_bounds__(256) void k_step_stats(size_t n, const double* __restrict__ dx,
                                                    const double* __restrict__ g, const double* __restrict__ r,
                                                    const double* __restrict__ lam, const double* __restrict__ x,
                                                    const double* __restrict__ hdiagActive, double* __restrict__ scal,
                                                    double* __restrict__ part, unsigned int* __restrict__ counter) {
  // gridDim.x workgroups stride over the vector; the last one to arrive folds the per-workgroup partials
  constexpr int NQ = 7;   // sums 0..4 and 6, maximum 5
  __shared__ double red[NQ][4];
  __shared__ int flag;
  const int G = gridDim.x;
  double a[NQ] = {0, 0, 0, 0, 0, 0, 0};
  for (size_t i = static_cast<size_t>(blockIdx.x) * 256 + threadIdx.x; i < n; i += static_cast<size_t>(G) * 256) {
    const double d = dx[i];
    a[0] += d * g[i];
    a[1] += d * r[i];
    a[2] += d * lam[i] * d;
    a[3] += d * d;
    if (hdiagActive[i] != 0.0) { a[4] += x[i] * x[i]; a[6] += 1.0; }
    a[5] = fmax(a[5], fabs(g[i]));
  }
#pragma unroll
  for (int k = 0; k < NQ; ++k)
    if (k != 5) a[k] = waveSum(a[k]);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) a[5] = fmax(a[5], __shfl_xor(a[5], off, 64));
  if ((threadIdx.x & 63) == 0)
    for (int k = 0; k < NQ; ++k) red[k][threadIdx.x >> 6] = a[k];
  __syncthreads();
  if (threadIdx.x < NQ) {
    const int k = threadIdx.x;
    part[k * G + blockIdx.x] = (k != 5) ? (red[k][0] + red[k][1]) + (red[k][2] + red[k][3])
                                        : fmax(fmax(red[5][0], red[5][1]), fmax(red[5][2], red[5][3]));
  }
  if (!lastBlockArrives(counter, G, &flag)) return;
  double t[NQ] = {0, 0, 0, 0, 0, 0, 0};
  for (int b = threadIdx.x; b < G; b += 256) {
#pragma unroll
    for (int k = 0; k < NQ; ++k)
      if (k != 5) t[k] += part[k * G + b];
    t[5] = fmax(t[5], part[5 * G + b]);
  }
#pragma unroll
  for (int k = 0; k < NQ; ++k)
    if (k != 5) t[k] = waveSum(t[k]);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) t[5] = fmax(t[5], __shfl_xor(t[5], off, 64));
  if ((threadIdx.x & 63) == 0)
    for (int k = 0; k < NQ; ++k) red[k][threadIdx.x >> 6] = t[k];
  __syncthreads();
  if (threadIdx.x == 0) {
    scal[S_DG] = red[0][0] + red[0][1] + red[0][2] + red[0][3];
    scal[S_DR] = red[1][0] + red[1][1] + red[1][2] + red[1][3];
    scal[S_DLD] = red[2][0] + red[2][1] + red[2][2] + red[2][3];
    scal[S_DD] = red[3][0] + red[3][1] + red[3][2] + red[3][3];
    scal[S_XX] = red[4][0] + red[4][1] + red[4][2] + red[4][3];
    scal[S_GMAX] = fmax(fmax(red[5][0], red[5][1]), fmax(red[5][2], red[5][3]));
    scal[S_NACTIVE] = red[6][0] + red[6][1] + red[6][2] + red[6][3];
  }
}

}  // namespace cvd
