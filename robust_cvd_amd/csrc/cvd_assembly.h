// cvd_assembly.h -- gradient J^T r and the frame-diagonal blocks of J^T J, generic and fast path (kernel map: cvd_kernels.h).
#pragma once

#include "cvd_kernels.h"
#include "cvd_asm_segments.h"

namespace cvd {

// ---------------------------------------------------------------------------------------------------
// Frame-major assembly: one workgroup owns frame f, walks every pair it takes part in (as source or as
// target), and accumulates g_f = J_f^T r and H_ff = J_f^T J_f in LDS (packed lower triangle), then adds the
// frame's regularisers.  No global atomics, no partial buffers, output written exactly once.
// ---------------------------------------------------------------------------------------------------
template <int KD, int KS>
inline __global__ __launch_bounds__(256) void k_assemble(Layout L, Table T, const double* __restrict__ x,
                                                  const FrameConst* __restrict__ fc, const double* __restrict__ mask,
                                                  const float* __restrict__ median,
                                                  const unsigned char* __restrict__ inRange,
                                                  const unsigned char* __restrict__ rangeFlags,
                                                  const int* __restrict__ fpOff, const int* __restrict__ fpList,
                                                  double* __restrict__ gOut, double* __restrict__ hOut,
                                                  double* __restrict__ costFrame, double* __restrict__ focalG,
                                                  double* __restrict__ focalH, AsmPanels panels, int panelCap) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  const int B = L.B;
  double* Hs = sm;             // one row panel of the packed lower triangle (panelCap doubles)
  double* gs = Hs + panelCap;  // B
  double* xf = gs + B;         // B
  double* xo = xf + B;         // B
  FrameConst* fcs = reinterpret_cast<FrameConst*>(xo + B);  // [0] = own frame, [1] = other frame
  double* red = reinterpret_cast<double*>(fcs + 2);          // 4 * 36
  const int f = blockIdx.x;
  const int tid = threadIdx.x;
  for (int i = tid; i < B; i += 256) {
    gs[i] = 0.0;
    xf[i] = x[static_cast<size_t>(f) * B + i];
  }
  constexpr int FCW = sizeof(FrameConst) / 8;
  if (tid < FCW) reinterpret_cast<double*>(fcs)[tid] = reinterpret_cast<const double*>(fc + f)[tid];
  const double* mf = mask + static_cast<size_t>(f) * B;
  double* hf = hOut + static_cast<size_t>(f) * B * B;
  double staticCost = 0.0, regCostTotal = 0.0;

  for (int pass = 0; pass < panels.n; ++pass) {
  const int r0 = panels.row[pass], r1 = panels.row[pass + 1];
  const int base = r0 * (r0 + 1) / 2, npk = r1 * (r1 + 1) / 2 - base;
  const bool first = pass == 0;  // gradient, cost and the shared-focal sums are taken in the first pass only
  // entry (hi, lo), hi >= lo, of the triangle: in this panel iff r0 <= hi < r1
#define CVD_PANEL_ADD(hi_, lo_, val_)                                                       \
  do {                                                                                      \
    const int hi__ = (hi_);                                                                 \
    if (hi__ >= r0 && hi__ < r1) atomicAdd(&Hs[packedIdx(hi__, (lo_)) - base], (val_));     \
  } while (0)
  __syncthreads();
  for (int i = tid; i < npk; i += 256) Hs[i] = 0.0;
  __syncthreads();

  // register accumulators of the pose-like 7x7 block + gradient (all lanes hit the same addresses)
  double PP[28];
  double gp[7];
  double cost = 0.0;
  double shG = 0.0, shH = 0.0;  // IntrinsicsOptimization::Shared: focal gradient / squared column norm
#pragma unroll
  for (int i = 0; i < 28; ++i) PP[i] = 0.0;
#pragma unroll
  for (int i = 0; i < 7; ++i) gp[i] = 0.0;

  if (L.includeStatic) {
    for (int e = fpOff[f]; e < fpOff[f + 1]; ++e) {
      const int code = fpList[e];
      const int p = code >> 1;
      const int side = code & 1;  // 0: f is the source (a) of pair p, 1: f is the target (b)
      const int o = side ? T.pairA[p] : T.pairB[p];
      __syncthreads();
      for (int i = tid; i < B; i += 256) xo[i] = x[static_cast<size_t>(o) * B + i];
      if (tid < FCW) reinterpret_cast<double*>(fcs + 1)[tid] = reinterpret_cast<const double*>(fc + o)[tid];
      __syncthreads();
      const FrameConst& fa = side ? fcs[1] : fcs[0];
      const FrameConst& fb = side ? fcs[0] : fcs[1];
      const double* xa = side ? xo : xf;
      const double* xb = side ? xf : xo;
      for (long long c = T.pairOff[p] + tid; c < T.pairOff[p + 1]; c += 256) {
        const float2 d = T.dsrc[c];
        if (!(d.x > 0.f)) continue;
        Sample<KD, KS> s;
        evalSample<KD, KS, true>(L, fa, fb, xa, xb, T.ndc[c], d, s);
        const double w = s.rho1;
        if (L.intrOpt == kIntrShared) {
          // one focal length: the focal column of this constraint is (d r / d f_a + d r / d f_b); its gradient and
          // squared norm are taken once per constraint (source visit) for frame 0's slot
#pragma unroll
          for (int rr = 0; rr < 3; ++rr) {
            const double tot = s.a.Jp[rr][6] + s.b.Jp[rr][6];
            s.a.Jp[rr][6] = tot;
            s.b.Jp[rr][6] = tot;
          }
          if (!side && first) {
            shG += w * (s.a.Jp[0][6] * s.r[0] + s.a.Jp[1][6] * s.r[1] + s.a.Jp[2][6] * s.r[2]);
            shH += w * (s.a.Jp[0][6] * s.a.Jp[0][6] + s.a.Jp[1][6] * s.a.Jp[1][6] + s.a.Jp[2][6] * s.a.Jp[2][6]);
          }
        }
        const Side<KD, KS>& me = side ? s.b : s.a;
        if (!side && first) cost += s.rho0;  // count every constraint once
        // pose-like block (rows 0..6: first panel)
        if (first) {
          int q = 0;
#pragma unroll
          for (int i = 0; i < 7; ++i) {
            gp[i] += w * (me.Jp[0][i] * s.r[0] + me.Jp[1][i] * s.r[1] + me.Jp[2][i] * s.r[2]);
#pragma unroll
            for (int j = 0; j <= i; ++j) {
              PP[q] += w * (me.Jp[0][i] * me.Jp[0][j] + me.Jp[1][i] * me.Jp[1][j] + me.Jp[2][i] * me.Jp[2][j]);
              ++q;
            }
          }
        }
        // tap columns
        const int nt = sideNumTapCols(L, me);
        for (int t = 0; t < nt; ++t) {
          int ct;
          double Jt[3];
          sideTapCol(L, me, t, ct, Jt);
          const double wj0 = w * Jt[0], wj1 = w * Jt[1], wj2 = w * Jt[2];
          if (first) atomicAdd(&gs[ct], wj0 * s.r[0] + wj1 * s.r[1] + wj2 * s.r[2]);
          if (ct >= r0 && ct < r1) {
            const int rowBase = ct * (ct + 1) / 2 - base;
#pragma unroll
            for (int i = 0; i < 7; ++i)
              atomicAdd(&Hs[rowBase + i], wj0 * me.Jp[0][i] + wj1 * me.Jp[1][i] + wj2 * me.Jp[2][i]);
          }
          for (int t2 = 0; t2 <= t; ++t2) {
            int c2;
            double J2[3];
            sideTapCol(L, me, t2, c2, J2);
            const double val = wj0 * J2[0] + wj1 * J2[1] + wj2 * J2[2];
            // tap columns of one sample are distinct but not sorted (border folding keeps row-major order,
            // spatial columns follow depth columns) -> order the pair
            const int hi = ct > c2 ? ct : c2, lo = ct > c2 ? c2 : ct;
            CVD_PANEL_ADD(hi, lo, val);
          }
        }
      }
    }
  }
  __syncthreads();
  if (first) {
    // block reduction of the register accumulators
    {
#pragma unroll
      for (int i = 0; i < 28; ++i) PP[i] = waveSum(PP[i]);
#pragma unroll
      for (int i = 0; i < 7; ++i) gp[i] = waveSum(gp[i]);
      cost = waveSum(cost);
      const int wv = tid >> 6;
      if ((tid & 63) == 0) {
#pragma unroll
        for (int i = 0; i < 28; ++i) red[wv * 36 + i] = PP[i];
#pragma unroll
        for (int i = 0; i < 7; ++i) red[wv * 36 + 28 + i] = gp[i];
        red[wv * 36 + 35] = cost;
      }
    }
    __syncthreads();
    if (tid < 28) {
      int i = 0;
      while ((i + 1) * (i + 2) / 2 <= tid) ++i;
      const int j = tid - i * (i + 1) / 2;
      Hs[packedIdx(i, j)] += red[tid] + red[36 + tid] + red[72 + tid] + red[108 + tid];  // (rows 0..6 are in panel 0: r1 >= 7)
    } else if (tid < 35) {
      gs[tid - 28] += red[tid] + red[36 + tid] + red[72 + tid] + red[108 + tid];
    }
    __syncthreads();
    staticCost = 0.5 * (red[35] + red[36 + 35] + red[72 + 35] + red[108 + 35]);
    __syncthreads();
  }
  if (L.intrOpt == kIntrShared) {
    // The focal column of every constraint belongs to frame 0's slot: publish this frame's static focal
    // gradient / diagonal for k_shared_focal_fixup and drop the entries from the frame's own block (for f != 0
    // they are off-diagonal couplings with frame 0, which the block-Jacobi preconditioner does not hold).
    if (first) {
      shG = waveSum(shG);
      shH = waveSum(shH);
      if ((tid & 63) == 0) { red[tid >> 6] = shG; red[4 + (tid >> 6)] = shH; }
      __syncthreads();
      if (tid == 0) {
        focalG[f] = red[0] + red[1] + red[2] + red[3];
        focalH[f] = red[4] + red[5] + red[6] + red[7];
        gs[6] = 0.0;
        Hs[packedIdx(6, 6)] = 0.0;
      }
    }
    if (f != 0) {
      for (int j = tid; j < B; j += 256) {
        if (j == 6) continue;
        const int hi = j > 6 ? j : 6, lo = j > 6 ? 6 : j;
        if (hi >= r0 && hi < r1) Hs[packedIdx(hi, lo) - base] = 0.0;
      }
    }
    __syncthreads();
  }

  // regularisers of this frame
  double regCost = 0.0;
  if (inRange[f]) {
    const int nr = numRegResiduals<KD>(L);
    for (int i = tid; i < nr; i += 256) {
      double r;
      int n;
      int cols[2 * KD + 2];
      double jac[2 * KD + 2];
      regResidual<KD>(L, f, i, xf, median[f], r, n, cols, jac);
      if (first) regCost += r * r;
      for (int a = 0; a < n; ++a) {
        if (first) atomicAdd(&gs[cols[a]], jac[a] * r);
        for (int b = 0; b <= a; ++b) {
          const int hi = cols[a] > cols[b] ? cols[a] : cols[b];
          const int lo = cols[a] > cols[b] ? cols[b] : cols[a];
          CVD_PANEL_ADD(hi, lo, jac[a] * jac[b]);
        }
      }
    }
  }
  if (tid == 0 && L.positionRegSqrt > 0.0 && first) {
    double o3[3] = {0, 0, 0}, dg = 0.0, cst = 0.0;
    posRegFrame(L, rangeFlags, f, x, nullptr, o3, dg, cst);
    for (int i = 0; i < 3; ++i) {
      atomicAdd(&gs[i], o3[i]);
      atomicAdd(&Hs[packedIdx(i, i)], dg);
    }
    regCost += cst;
  }
  if (first) {
    regCost = waveSum(regCost);
    __syncthreads();
    if ((tid & 63) == 0) red[tid >> 6] = regCost;
    __syncthreads();
    regCostTotal = 0.5 * (red[0] + red[1] + red[2] + red[3]);
  }
  __syncthreads();
  // write-out of this panel with the constant-parameter mask applied (constant columns drop out of J): entry (i, j),
  // j <= i, goes to both triangles of the full block
  for (int idx = tid; idx < npk; idx += 256) {
    int i = static_cast<int>((sqrt(8.0 * static_cast<double>(idx + base) + 1.0) - 1.0) * 0.5);
    while (i * (i + 1) / 2 > idx + base) --i;
    while ((i + 1) * (i + 2) / 2 <= idx + base) ++i;
    const int j = idx + base - i * (i + 1) / 2;
    const double v = Hs[idx] * mf[i] * mf[j];
    hf[static_cast<size_t>(i) * B + j] = v;
    hf[static_cast<size_t>(j) * B + i] = v;
  }
#undef CVD_PANEL_ADD
  }  // pass
  if (tid == 0) costFrame[f] = staticCost + regCostTotal;
  __syncthreads();
  for (int i = tid; i < B; i += 256) gOut[static_cast<size_t>(f) * B + i] = gs[i] * mf[i];
}

// IntrinsicsOptimization::Shared: frame 0's focal slot receives the static focal gradient / diagonal of all frames.
inline __global__ __launch_bounds__(256) void k_shared_focal_fixup(Layout L, const double* __restrict__ focalG,
                                                            const double* __restrict__ focalH,
                                                            const double* __restrict__ mask, double* __restrict__ g,
                                                            double* __restrict__ hBlocks) {
  __shared__ double red[8];
  double a = 0.0, b = 0.0;
  for (int f = threadIdx.x; f < L.F; f += 256) { a += focalG[f]; b += focalH[f]; }
  a = waveSum(a);
  b = waveSum(b);
  if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6] = a; red[4 + (threadIdx.x >> 6)] = b; }
  __syncthreads();
  if (threadIdx.x == 0) {
    const double m = mask[6];
    g[6] += (red[0] + red[1] + red[2] + red[3]) * m;
    hBlocks[static_cast<size_t>(6) * L.B + 6] += (red[4] + red[5] + red[6] + red[7]) * m * m;
  }
}

inline __global__ void k_extract_diag(Layout L, const double* __restrict__ hBlocks, double* __restrict__ out) {
  const size_t n = static_cast<size_t>(L.F) * L.B;
  const size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const size_t f = i / L.B, c = i - f * L.B;
  out[i] = hBlocks[(f * L.B + c) * L.B + c];
}

// =====================================================================================================
// Fast path of the frame-major assembly (same scope as k_matvec_pairs_fast: identity spatial transform,
// reprojection losses, Identity / Global / bilinear depth transform).  Only the OWN side's Jacobian is formed
// (3x7 pose-like columns + the 3-vector d r / d D); taps are unrolled, nothing is indexed dynamically.
// Accumulation: 7x7 + gradient in registers (wave-reduced at the end), pose x grid and grid x grid through LDS
// f64 atomics into the packed lower triangle.
// Register state (KD = 4, list mode, STAGE; DESIGN_LOG has the history): the runtime-variant walk (SPEC = 0) sits at
// its 256-VGPR budget with a few spilled values; the specialised walk (SPEC = 1 / 2, asmWalkSpec below) needs no
// scratch -- tests/test_codegen_assembly.py pins that.
// =====================================================================================================

#ifdef CVD_ASM_PROFILE
__device__ unsigned long long g_asmProf[2048 * 16];
#define ASM_STAMP(slot) do { if (lane == 0) g_asmProf[(blockIdx.x & 2047) * 16 + (slot)] = wall_clock64(); } while (0)
// Per-wave sums over the wave's units of the specialised walk (the 16 slots above are all taken): [0] the wait for the unit descriptor,
// [1] for the pair's frames and offsets, [2] for the other frame's constants, the staged parameters and the first record, [3] the walk
// itself, [4] the number of units.  Every stamp waits for all outstanding loads first, so the phases do not overlap: the build measures
// how the loop's time divides, it is not the product's schedule.
__device__ unsigned long long g_asmWait[2048 * 8 * 8];
#define ASM_WAIT_DECL unsigned long long asmT[5] = {0, 0, 0, 0, 0}; unsigned long long asmT0 = 0
#define ASM_WAIT_BEGIN() do { asmT0 = wall_clock64(); } while (0)
#define ASM_WAIT_LAP(k) do { asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory"); const unsigned long long t_ = wall_clock64(); \
                             asmT[k] += t_ - asmT0; asmT0 = t_; } while (0)
#define ASM_WAIT_MARK(k) do { const unsigned long long t_ = wall_clock64(); asmT[k] += t_ - asmT0; asmT0 = t_; } while (0)
#define ASM_WAIT_FLUSH() do { if (lane == 0) for (int k_ = 0; k_ < 5; ++k_) g_asmWait[((blockIdx.x & 2047) * 8 + (wv & 7)) * 8 + k_] = asmT[k_]; } while (0)
#define ASM_WAIT_PARAMS , unsigned long long (&asmT)[5], unsigned long long& asmT0
#define ASM_WAIT_ARGS , asmT, asmT0
#else
#define ASM_STAMP(slot) do {} while (0)
#define ASM_WAIT_DECL
#define ASM_WAIT_BEGIN() do {} while (0)
#define ASM_WAIT_LAP(k) do {} while (0)
#define ASM_WAIT_MARK(k) do {} while (0)
#define ASM_WAIT_FLUSH() do {} while (0)
#define ASM_WAIT_PARAMS
#define ASM_WAIT_ARGS
#endif
// Every instantiation runs kAsmThreads per workgroup.  The packed triangle leaves room for ONE workgroup per CU, so the waves per
// SIMD are the workgroup's waves / 4: 8 waves need <= 256 VGPRs, 12 would need <= 168 (the specialised walk then spills 102), 16 <= 128.

// The frame scalars of a (pair, side) entry: they hold for every constraint of the entry, whichever unit or segment it is walked in.
struct AsmEntryScalars {
  double RaU[9], RbU[9], dTU[3];
  double fxa, fya, ifxb, ifyb;
  __device__ __forceinline__ void form(const Layout& L, const FrameConst& Fa, const FrameConst& Fb) {
    const double A = L.aspect;
#pragma unroll
    for (int i = 0; i < 9; ++i) { RaU[i] = uniformValue(Fa.R[i]); RbU[i] = uniformValue(Fb.R[i]); }
#pragma unroll
    for (int i = 0; i < 3; ++i) dTU[i] = uniformValue(Fa.t[i] - Fb.t[i]);
    fya = uniformValue(Fa.fy);
    fxa = fya * A;
    const double fyb = uniformValue(Fb.fy);
    ifyb = uniformValue(1.0 / fyb);
    ifxb = uniformValue(1.0 / (fyb * A));
  }
};

// The walk of one unit with the variant fixed at compile time (k_assemble_fast's SPEC = 1 / 2: one value parameter per vertex,
// ReproDisparity, Cauchy / Huber -- the rule of k_matvec_pairs_fast).  `side` is the own frame's role in the pair (0: the source,
// 1: the target): wave-uniform, a scalar branch where the two Jacobians differ.  (Two copies of the loop, one per role, were tried: the
// register allocator then keeps the 35 accumulators twice and the kernel spills.)
//  * Frame constants are scalars for the whole unit (R_a, R_b, t_a - t_b, the focals and their reciprocals): nothing of FrameConst is
//    read inside the constraint loop.
//  * Rotation columns in the frame's LOCAL basis.  dR/dw_i = [a_i]x R (a_i = row i of FrameConst::Jl), so with G = M R_b^T, the rows
//    of the translation columns,
//      source:  G_rr . dR_a,i (D_a c_a) = a_i . (X x G_rr),  X = D_a R_a c_a
//      target:  M_rr . dR_b,i^T v       = a_i . (G_rr x v)
//    i.e. every rotation column is Jl applied to ONE cross product per residual row.  The loop accumulates with that 3-vector in
//    columns 3..5 (no dR, no Jl) and the kernel applies T = diag(I_3, Jl^T, I) to the sums afterwards: H <- T^T H T, g <- T^T g
//    (asmLocalToAxisAngle).
//  * Hardware reciprocals with two Newton steps (rcpFast / rsqrtFast) instead of IEEE divisions; rho and rho' written out.
//  * The next trip's table record is in flight during this trip's arithmetic (RecordStream, primed by the caller before it stages).
// asmConstraintSpec is one valid constraint (table record nd, d) of that walk: residual, the own side's Jacobian, its share of the sums.
template <int KD, int SPEC>
__device__ __forceinline__ void asmConstraintSpec(const Layout& L, const AsmEntryScalars& S, const float4 nd, const float2 d,
                                                  const bool side, const double* __restrict__ xa, const double* __restrict__ xb,
                                                  double* Hs, double* gs, double (&PP)[28], double (&gp)[7], double (&GD)[19],
                                                  double& cost) {
  const double A = L.aspect;
  const double (&RaU)[9] = S.RaU;
  const double (&RbU)[9] = S.RbU;
  const double (&dTU)[3] = S.dTU;
  const double fxa = S.fxa, fya = S.fya, ifxb = S.ifxb, ifyb = S.ifyb;
  const double da = static_cast<double>(d.x), db = static_cast<double>(d.y);
  // The own side's taps are kept for the accumulation; the other side's only interpolate its depth and are formed first, so the two
  // sets and a selected copy are never held together (bicubic: 8 weights a side).  own = xf's side: `side` picks which of a / b.
  FastTaps<KD> tm;
  double Dm = 0.0, Do = 0.0;
  {
    FastTaps<KD> to;
    fastGather<KD>(L, side ? nd.x : nd.z, side ? nd.y : nd.w, to);
    const double* __restrict__ xo_ = side ? xa : xb;
#pragma unroll
    for (int k = 0; k < KD; ++k)
      if (to.ok(k)) Do += xo_[7 + to.I(k)] * to.Wt(k);
  }
  fastGather<KD>(L, side ? nd.z : nd.x, side ? nd.w : nd.y, tm);
  {
    const double* __restrict__ xm_ = side ? xb : xa;
#pragma unroll
    for (int k = 0; k < KD; ++k)
      if (tm.ok(k)) Dm += xm_[7 + tm.I(k)] * tm.Wt(k);
  }
  const double Da = (side ? Do : Dm) * da;
  const double Db = (side ? Dm : Do) * db;
  const double pax = static_cast<double>(nd.x), pay = static_cast<double>(nd.y);
  const double pbx = static_cast<double>(nd.z), pby = static_cast<double>(nd.w);
  double ca[3], Rca[3];
  fastRay(RaU, pax, pay, fxa, fya, ca, Rca);
  const double v[3] = {dTU[0] + Rca[0] * Da, dTU[1] + Rca[1] * Da, dTU[2] + Rca[2] * Da};
  double zz, iz, u, vv, r[3], dr2dA, dr2dDb;
  fastProject<true>(L, RbU, v, ifxb, ifyb, pbx, pby, zz, iz, u, vv, r[0], r[1]);
  fastDepthResidual<true>(L, kLossDisparity, zz, iz, Db, r[2], dr2dA, dr2dDb);
  const double sq = r[0] * r[0] + r[1] * r[1] + r[2] * r[2];
  const double w = fastRobustRho1<SPEC>(L, sq);     // rho'
  if (!side) cost += fastRobustRho0<SPEC>(L, sq);  // rho: on the source visit (every constraint is counted once)

  // d r / d q (rows, fastRows);  G = M R_b^T
  double m00, m11, m02, m12;
  fastRows(L, iz, u, vv, ifxb, ifyb, m00, m11, m02, m12);
  const double m22 = -dr2dA;
  double G[3][3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    G[0][i] = m00 * RbU[i * 3 + 0] + m02 * RbU[i * 3 + 2];
    G[1][i] = m11 * RbU[i * 3 + 1] + m12 * RbU[i * 3 + 2];
    G[2][i] = m22 * RbU[i * 3 + 2];
  }
  double Jp[3][7];  // columns 3..5: local basis (see above)
  double JD[3];
  if (!side) {
    const double X[3] = {Da * Rca[0], Da * Rca[1], Da * Rca[2]};
    const double cf0 = pax * A, cf1 = pay;
    const double dXdf[3] = {Da * (RaU[0] * cf0 + RaU[1] * cf1), Da * (RaU[3] * cf0 + RaU[4] * cf1),
                            Da * (RaU[6] * cf0 + RaU[7] * cf1)};
#pragma unroll
    for (int rr = 0; rr < 3; ++rr) {
      Jp[rr][0] = G[rr][0]; Jp[rr][1] = G[rr][1]; Jp[rr][2] = G[rr][2];
      Jp[rr][3] = X[1] * G[rr][2] - X[2] * G[rr][1];
      Jp[rr][4] = X[2] * G[rr][0] - X[0] * G[rr][2];
      Jp[rr][5] = X[0] * G[rr][1] - X[1] * G[rr][0];
      Jp[rr][6] = dot3(G[rr], dXdf);
      JD[rr] = dot3(G[rr], Rca);
    }
  } else {
#pragma unroll
    for (int rr = 0; rr < 3; ++rr) {
      Jp[rr][0] = -G[rr][0]; Jp[rr][1] = -G[rr][1]; Jp[rr][2] = -G[rr][2];
      Jp[rr][3] = G[rr][1] * v[2] - G[rr][2] * v[1];
      Jp[rr][4] = G[rr][2] * v[0] - G[rr][0] * v[2];
      Jp[rr][5] = G[rr][0] * v[1] - G[rr][1] * v[0];
    }
    Jp[0][6] = -L.ws * u * ifyb;
    Jp[1][6] = -L.ws * vv * ifyb;
    Jp[2][6] = 0.0;
    JD[0] = 0.0; JD[1] = 0.0; JD[2] = dr2dDb;
  }
  // ---- accumulate
  int qi = 0;
#pragma unroll
  for (int i = 0; i < 7; ++i) {
    gp[i] += w * (Jp[0][i] * r[0] + Jp[1][i] * r[1] + Jp[2][i] * r[2]);
#pragma unroll
    for (int j = 0; j <= i; ++j) {
      PP[qi] += w * (Jp[0][i] * Jp[0][j] + Jp[1][i] * Jp[1][j] + Jp[2][i] * Jp[2][j]);
      ++qi;
    }
  }
  double v7[7];
#pragma unroll
  for (int i = 0; i < 7; ++i) v7[i] = w * (Jp[0][i] * JD[0] + Jp[1][i] * JD[1] + Jp[2][i] * JD[2]);
  const double sDD = w * (JD[0] * JD[0] + JD[1] * JD[1] + JD[2] * JD[2]);
  const double sDr = w * (JD[0] * r[0] + JD[1] * r[1] + JD[2] * r[2]);
  const double dm = side ? db : da;  // d D / d theta_k = w_k d
  if constexpr (KD == 1) {
    // (Global / Identity: the single depth block is hit by every sample -> the kernel's register accumulators)
    const double fac = tm.Wt(0) * dm;
#pragma unroll
    for (int i = 0; i < 7; ++i) GD[i] += v7[i] * fac;
    GD[17] += sDr * fac;
    GD[14] += sDD * fac * fac;
  } else {
#pragma unroll
    for (int ka = 0; ka < KD; ++ka) {
      if (!tm.ok(ka)) continue;
      const double fa = tm.Wt(ka) * dm;
      const int ct = 7 + tm.I(ka);
      const int rowBase = ct * (ct + 1) / 2;
      atomicAdd(&gs[ct], sDr * fa);
#pragma unroll
      for (int i = 0; i < 7; ++i) atomicAdd(&Hs[rowBase + i], v7[i] * fa);
      const double sfa = sDD * fa;
#pragma unroll
      for (int kb = 0; kb <= ka; ++kb) {
        if (!tm.ok(kb)) continue;
        const int c2 = 7 + tm.I(kb);
        // (bilinear taps at gx = 1 are not in index order: order the pair; the bicubic taps are)
        const int hi = (KD == 16 || ct > c2) ? ct : c2, lo = (KD == 16 || ct > c2) ? c2 : ct;
        atomicAdd(&Hs[packedIdx(hi, lo)], sfa * (tm.Wt(kb) * dm));
      }
    }
  }
}

template <int KD, int SPEC>
__device__ __forceinline__ void asmWalkSpec(const Layout& L, const Table& T, RecordStream<false>& rs, long long cBegin, int n,
                                            int lane, const bool side, const FrameConst& Fa, const FrameConst& Fb,
                                            const double* __restrict__ xa, const double* __restrict__ xb, double* Hs,
                                            double* gs, double (&PP)[28], double (&gp)[7], double (&GD)[19], double& cost ASM_WAIT_PARAMS) {
  AsmEntryScalars S;
  S.form(L, Fa, Fb);
  ASM_WAIT_LAP(2);
  for (int ci = lane; ci < n; ci += 64) {
    float4 nd;
    float2 d;
    if (!rs.take(T, cBegin, ci, 64, n, 0, 0, 0, nd, d)) continue;
    asmConstraintSpec<KD, SPEC>(L, S, nd, d, side, xa, xb, Hs, gs, PP, gp, GD, cost);
  }
}

// B doubles from global memory straight into an LDS row, no register in between (LDS-DMA, one dword per lane and instruction: the rows
// are 8-byte aligned, B may be odd).  The destination of an instruction is the wave-uniform address in M0 plus 4 bytes per lane; M0
// is the compiler's, so it is saved and restored within the statement.  The compiler does not count these loads: the caller waits for
// them with an `s_waitcnt vmcnt(0)` of its own before it reads the row (asmWalkSegments, at the switch of segments).
__device__ __forceinline__ void asmStageAhead(const double* __restrict__ src, double* dstRow, int B, int lane) {
  const unsigned int* g = reinterpret_cast<const unsigned int*>(src);
  const unsigned int lds = static_cast<unsigned int>(reinterpret_cast<uintptr_t>(
      (__attribute__((address_space(3))) void*)dstRow));  // (the row's byte address within the workgroup's LDS)
  const int nDw = 2 * B;
  for (int k0 = 0; k0 < nDw; k0 += 64) {
    if (k0 + lane < nDw) {
      unsigned int keep;
      const unsigned int dst = __builtin_amdgcn_readfirstlane(lds + 4u * static_cast<unsigned int>(k0));
      asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dword %1, off\n\ts_mov_b32 m0, %0"
                   : "=&s"(keep) : "v"(g + k0 + lane), "s"(dst) : "memory");
    }
  }
}

// How a launch's segment list reaches the kernel.  k_assemble_fast's parameter list is fixed (tests/test_codegen_assembly.py
// instantiates it by its argument types), and cvd_kernels.h, where AsmWork lives, is tied to the committed counter files by its hash.
// A list-mode launch has no dense records, so the list travels in that argument: records = the segments, recOff = the (part, wave)
// offsets, fpOff = the staging depth as an integer in a pointer's bits.  Only these two functions know.
inline DenseRecords asmSegsAsArgument(const AsmSegs& s) {
  return DenseRecords{reinterpret_cast<const double*>(s.seg), s.waveOff,
                      reinterpret_cast<const int*>(static_cast<uintptr_t>(s.depth)), nullptr};
}
__host__ __device__ __forceinline__ AsmSegs asmSegsFromArgument(const DenseRecords& d) {
  return AsmSegs{reinterpret_cast<const AsmSegment*>(d.records), d.recOff,
                 static_cast<int32_t>(reinterpret_cast<uintptr_t>(d.fpOff))};
}

// The walk of a wave's SEGMENTS (cvd_asm_segments.h; the multi-wave build's SPEC = 1 / 2): what asmWalkSpec does per unit is done
// once per segment, and what a segment needs is requested while the one before it is walked.
//  * The segment record is one scalar load; the next one is read while this one is walked.
//  * The frame scalars are formed and the other frame's parameters staged once per segment.
//  * The record stream runs through: every trip requests the next trip's record, the last trip of a segment the first record of the
//    next segment.
//  * segs.depth = 2: two staging rows per wave.  The last trip of a segment also requests the next segment's other-frame parameters
//    into the row that is not in use (asmStageAhead), so the switch only waits for what has been in flight for a trip.  depth = 1:
//    one row, copied through registers at the switch.  STAGE = false (depth 0): the other frame's parameters are read from memory.
// One copy of the trip loop for both roles and all segments (the accumulators must not be kept twice: asmWalkSpec's note).
template <int KD, int SPEC, bool STAGE>
__device__ __forceinline__ void asmWalkSegments(const Layout& L, const Table& T, const double* __restrict__ x,
                                                const FrameConst* __restrict__ fc, const int f, const AsmSegs& segs, const int wv,
                                                const int lane, const double* xf, double* xstage, double* Hs, double* gs,
                                                double (&PP)[28], double (&gp)[7], double (&GD)[19], double& cost) {
  const int B = L.B;
  const int slot = static_cast<int>(blockIdx.x) * (kAsmThreads / 64) + wv;
  int si = __builtin_amdgcn_readfirstlane(segs.waveOff[slot]);
  const int sEnd = __builtin_amdgcn_readfirstlane(segs.waveOff[slot + 1]);
  if (si >= sEnd) return;  // (a part with fewer units than waves)
  ASM_WAIT_DECL;
  ASM_WAIT_BEGIN();
  const bool ahead = STAGE && segs.depth == 2;
  double* rows = xstage + static_cast<size_t>(wv) * (ahead ? 2 : 1) * B;
  int row = 0;
  AsmSegment cur = segs.seg[si];
  bool fresh = true;  // nothing of `cur` has been requested yet (the wave's first segment)
  float4 ndNext = make_float4(0.f, 0.f, 0.f, 0.f);
  float2 dNext = make_float2(0.f, 0.f);
  for (;;) {
    // What `cur` still needs before it can be walked.  Its first record and, with two rows, its staged parameters were requested
    // in the last trip of the segment before it; the wave's first segment requests everything here, and with one row the copy is
    // made here, through registers (a wave's LDS operations execute in order: its reads of the row in the last trip are done before
    // these writes land).  One wait for all of it.
    if (fresh && lane < cur.count) { dNext = (T.dsrc + cur.first)[lane]; ndNext = (T.ndc + cur.first)[lane]; }
    if constexpr (STAGE) {
      if (fresh || !ahead) {
        const double* __restrict__ xo = x + static_cast<size_t>(cur.other) * B;
        double* xw = rows + static_cast<size_t>(row) * B;
        for (int i = lane; i < B; i += 64) xw[i] = xo[i];
      }
    }
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    fresh = false;
    const bool more = cur.last == 0;
    AsmSegment nxt = cur;
    if (more) nxt = segs.seg[si + 1];  // (one scalar load, in flight while this segment is walked; needed in its last trip)
    const bool side = cur.side != 0;
    AsmEntryScalars S;
    S.form(L, side ? fc[cur.other] : fc[f], side ? fc[f] : fc[cur.other]);
    const double* xov = STAGE ? rows + static_cast<size_t>(row) * B : x + static_cast<size_t>(cur.other) * B;
    const double* xa = side ? xov : xf;
    const double* xb = side ? xf : xov;
    const int n = cur.count;
    ASM_WAIT_LAP(2);
    for (int base = 0; base < n; base += 64) {  // (every lane runs every trip: the last one requests for the next segment)
      const int ci = base + lane;
      const float4 nd = ndNext;
      const float2 d = dNext;
      // the next record of the wave's stream: this segment's next trip, or the next segment's first (one load site, scalar selects;
      // 32-bit offsets from the scalar base)
      const bool within = base + 64 < n;
      const long long rb = within ? cur.first : nxt.first;
      const int ri = within ? ci + 64 : lane;
      const int rn = within ? n : (more ? nxt.count : 0);
      if (ri < rn) {
        dNext = *reinterpret_cast<const float2*>(reinterpret_cast<const char*>(T.dsrc + rb) + static_cast<unsigned int>(ri) * 8u);
        ndNext = *reinterpret_cast<const float4*>(reinterpret_cast<const char*>(T.ndc + rb) + static_cast<unsigned int>(ri) * 16u);
      }
      if (!within && more && ahead)
        asmStageAhead(x + static_cast<size_t>(nxt.other) * B, rows + static_cast<size_t>(row ^ 1) * B, B, lane);
      if (ci < n && d.x > 0.f) asmConstraintSpec<KD, SPEC>(L, S, nd, d, side, xa, xb, Hs, gs, PP, gp, GD, cost);
    }
    ASM_WAIT_MARK(3);  // (no wait here: what the next segment waits for at its top counts as its wait)
#ifdef CVD_ASM_PROFILE
    ++asmT[4];
#endif
    if (!more) break;
    if (ahead) row ^= 1;
    ++si;
    cur = nxt;
  }
  ASM_WAIT_FLUSH();
}

// Rotation rows / columns of a frame's sums from the local basis of asmWalkSpec to the axis-angle parameters: with J = Jl (row i =
// a_i) every triple (H[3][j], H[4][j], H[5][j]), j outside 3..5, becomes J times itself, the 3 x 3 block S becomes J S J^T and the
// gradient triple J g.  Linear, so it commutes with the fold of a split frame's parts: every part transforms its own sums, BEFORE
// the regularisers (which are in axis-angle terms) are added.  Each entry is read and written by one thread; the caller's barriers
// separate it from the accumulation before and the regularisers after.
template <int NT>
__device__ __forceinline__ void asmLocalToAxisAngle(const double* __restrict__ Jl, int B, int tid, double* Hs, double* gs) {
  double J[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) J[i] = Jl[i];
  for (int j = tid; j < B; j += NT) {
    if (j >= 3 && j <= 5) continue;
    const int i0 = j < 3 ? packedIdx(3, j) : packedIdx(j, 3);
    const int i1 = j < 3 ? packedIdx(4, j) : packedIdx(j, 4);
    const int i2 = j < 3 ? packedIdx(5, j) : packedIdx(j, 5);
    const double h0 = Hs[i0], h1 = Hs[i1], h2 = Hs[i2];
    Hs[i0] = J[0] * h0 + J[1] * h1 + J[2] * h2;
    Hs[i1] = J[3] * h0 + J[4] * h1 + J[5] * h2;
    Hs[i2] = J[6] * h0 + J[7] * h1 + J[8] * h2;
  }
  if (tid == NT - 1) {
    double S[3][3], JS[3][3];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int b = 0; b < 3; ++b) S[a][b] = Hs[a >= b ? packedIdx(3 + a, 3 + b) : packedIdx(3 + b, 3 + a)];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int b = 0; b < 3; ++b) JS[a][b] = J[a * 3] * S[0][b] + J[a * 3 + 1] * S[1][b] + J[a * 3 + 2] * S[2][b];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int b = 0; b <= a; ++b)
        Hs[packedIdx(3 + a, 3 + b)] = JS[a][0] * J[b * 3] + JS[a][1] * J[b * 3 + 1] + JS[a][2] * J[b * 3 + 2];
    const double g0 = gs[3], g1 = gs[4], g2 = gs[5];
    gs[3] = J[0] * g0 + J[1] * g1 + J[2] * g2;
    gs[4] = J[3] * g0 + J[4] * g1 + J[5] * g2;
    gs[5] = J[6] * g0 + J[7] * g1 + J[8] * g2;
  }
}

// The frame's regularisers for the specialised walk (N = 1, 2-D grid or Global): same residuals as regResidual, with nothing indexed
// dynamically.  The scale regulariser's taps are unrolled (FastTaps); the others (focal, grid deformation, spatial: one or two columns)
// go through regResidual with the scale term switched off, which leaves only constant indices into its column arrays.  Returns
// this thread's sum of squared residuals.
template <int KD, int NT>
__device__ __forceinline__ double asmRegularisersSpec(const Layout& L, int f, int tid, const double* __restrict__ xf, float median,
                                                      double* Hs, double* gs) {
  constexpr double eps = 1e-6;
  double regCost = 0.0;
  if (L.scaleRegSqrt > 0.0) {
    const int ns = L.sregX * L.sregY;
    const bool taps = KD > 1 || L.depthType == kDepthGlobal;  // (depthGather: one tap exists for the Global transform only)
    for (int i = tid; i < ns; i += NT) {
      const int y = i / L.sregX, x = i - y * L.sregX;
      // float arithmetic of reference lib/PoseOptimizer.cpp:1384-1385
      const float lx = __fadd_rn(-1.f, __fdiv_rn(__fmul_rn(2.f, static_cast<float>(x)), static_cast<float>(L.sregX - 1)));
      const float ly = __fadd_rn(-1.f, __fdiv_rn(__fmul_rn(2.f, static_cast<float>(y)), static_cast<float>(L.sregY - 1)));
      FastTaps<KD> t;
      fastGather<KD>(L, lx, ly, t);
      const double d = static_cast<double>(median);
      double D = (L.depthType == kDepthIdentity) ? d : 0.0;
#pragma unroll
      for (int k = 0; k < KD; ++k)
        if (taps && t.ok(k)) D += d * xf[7 + t.I(k)] * t.Wt(k);
      const bool o = !(D < eps);
      const double dd = o ? D : eps;
      const double r = L.scaleRegSqrt * (1.0 / dd - 1.0);
      const double drdD = o ? (-L.scaleRegSqrt / (dd * dd)) : 0.0;
      regCost += r * r;
#pragma unroll
      for (int ka = 0; ka < KD; ++ka) {
        if (!(taps && t.ok(ka))) continue;
        const int ca = 7 + t.I(ka);
        const double ja = drdD * t.Wt(ka) * d;
        atomicAdd(&gs[ca], ja * r);
#pragma unroll
        for (int kb = 0; kb <= ka; ++kb) {
          if (!t.ok(kb)) continue;
          const int cb = 7 + t.I(kb);
          const int hi = ca > cb ? ca : cb, lo = ca > cb ? cb : ca;
          atomicAdd(&Hs[packedIdx(hi, lo)], ja * (drdD * t.Wt(kb) * d));
        }
      }
    }
  }
  Layout Lr = L;
  Lr.scaleRegSqrt = 0.0;
  const int nr = numRegResiduals<KD>(Lr);
  for (int i = tid; i < nr; i += NT) {
    double r;
    int n;
    int cols[2 * KD + 2];
    double jac[2 * KD + 2];
    regResidual<KD>(Lr, f, i, xf, median, r, n, cols, jac);
    regCost += r * r;
    if (n >= 1) {
      atomicAdd(&gs[cols[0]], jac[0] * r);
      atomicAdd(&Hs[packedIdx(cols[0], cols[0])], jac[0] * jac[0]);
    }
    if (n >= 2) {
      atomicAdd(&gs[cols[1]], jac[1] * r);
      const int hi = cols[1] > cols[0] ? cols[1] : cols[0], lo = cols[1] > cols[0] ? cols[0] : cols[1];
      atomicAdd(&Hs[packedIdx(hi, lo)], jac[1] * jac[0]);
      atomicAdd(&Hs[packedIdx(cols[1], cols[1])], jac[1] * jac[1]);
    }
  }
  return regCost;
}

// STAGE (round 5): the OTHER frame's parameters of the unit a wave walks are copied into a per-wave LDS buffer first.  Without it
// the taps of the other side are 4-tap gathers from global memory -- a dependent round trip in every trip of a kernel that runs
// two waves per SIMD -- and, since `side` selects between an LDS and a global pointer at run time, every parameter read of the
// loop is a FLAT load.  With it both sides are LDS reads.  Needs 8 B more doubles of LDS: on whenever that fits (cvd_eval.hip).
// FOLD (round 6, dense mode inside the explicit-block scope): the constraints were walked by k_dense_walk (cvd_dense_walk.h); a
// frame's workgroup sums its records -- a gather over (pair, side) entries, no atomics -- in place of the walk, and continues with
// the regularisers and the write-out as ever.  One workgroup per frame (blockIdx.x = frame; the work list is not used).
// SPEC (as on k_matvec_pairs_fast, chosen by the same rule): 1 = one value parameter per vertex, ReproDisparity, Cauchy; 2 = the same
// with Huber; 0 = the runtime-variant walk below (everything else, shared intrinsics -- their extra focal column sits in the loop --
// and the DENSE / FOLD instantiations).  SPEC != 0 walks segments through asmWalkSegments (the list arrives in `dr`:
// asmSegsAsArgument; the one-wave deterministic build walks its units through asmWalkSpec).
template <int KD, bool DENSE = false, bool STAGE = false, bool FOLD = false, int SPEC = 0>
inline __global__ __launch_bounds__(kAsmThreads) void k_assemble_fast(Layout L, Table T, const double* __restrict__ x,
                                                       const FrameConst* __restrict__ fc,
                                                       const double* __restrict__ mask, const float* __restrict__ median,
                                                       const unsigned char* __restrict__ regOwner,
                                                       const unsigned char* __restrict__ rangeFlags,
                                                       AsmWork work,
                                                       double* __restrict__ gOut, double* __restrict__ hOut,
                                                       double* __restrict__ costFrame, double* __restrict__ focalG,
                                                       double* __restrict__ focalH, DenseRecords dr = DenseRecords{}) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  constexpr double eps = 1e-6;
  const int B = L.B;
  const int npk = B * (B + 1) / 2;
  // LDS holds only what is accumulated into: the packed block, the gradient, this frame's parameters and the
  // reduction scratch ((B(B+1)/2 + 2B + 144) doubles: B = 199, the 16x12 grid, still fits 160 KiB).  The other
  // frame's parameters and both frames' FrameConst are read through L1/L2 (wave-uniform or 4-tap gathers).
  double* Hs = sm;
  double* gs = Hs + npk;
  double* xf = gs + B;
  double* red = xf + B;  // 36 workgroup sums (LDS atomics, one set per wave) + scratch
  double* xstage = red + 4 * 36;  // STAGE: NT / 64 x B doubles
  const AsmPart me = FOLD ? AsmPart{static_cast<int>(blockIdx.x), 0, 0, 0, 1, 0} : work.parts[blockIdx.x];
  const int f = me.frame;
  const int tid = threadIdx.x;
  static_assert(SPEC == 0 || (!DENSE && !FOLD), "the specialised walk is list mode only");
  constexpr int NT = kAsmThreads;
  // wave-uniform wave index (scalar register: the per-entry frame constants below become scalar loads)
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lane = tid & 63;
  if (tid == 0) ASM_STAMP(0);
  for (int i = tid; i < npk; i += NT) Hs[i] = 0.0;
  if (tid < 48) red[tid] = 0.0;
  for (int i = tid; i < B; i += NT) {
    gs[i] = 0.0;
    xf[i] = x[static_cast<size_t>(f) * B + i];
  }
  __syncthreads();
  if (tid == 0) ASM_STAMP(1);

  double PP[28], gp[7];
  // KD == 1 (Global / Identity): the single depth block is hit by every sample -> register accumulators
  // [0..13] pose x theta (7 x N), [14..16] theta x theta (lower), [17..18] gradient
  double GD[19];
#pragma unroll
  for (int i = 0; i < 19; ++i) GD[i] = 0.0;
  double cost = 0.0;
  double shG = 0.0, shH = 0.0;  // IntrinsicsOptimization::Shared: focal gradient / squared column norm
#pragma unroll
  for (int i = 0; i < 28; ++i) PP[i] = 0.0;
#pragma unroll
  for (int i = 0; i < 7; ++i) gp[i] = 0.0;
  const int N = SPEC ? 1 : L.N;
  const double A = L.aspect;

  if constexpr (FOLD) {
    if (L.includeStatic) {
      // output o: [0, 28) pose x pose (lower), [28, 35) pose gradient, 35 cost, then 36 + c G + v: c < 7 theta[v] x pose[c],
      // c = 7 gradient of theta[v], c = 8 + d band d of theta x theta.  Side 0 (source) / 1 (target) read different parts of a record.
      const int G = L.nD;
      const int recN = dwRecordDoubles(G);
      const int e0 = dr.fpOff[f], e1 = dr.fpOff[f + 1];
      const int nOut = 36 + 13 * G;
      for (int o = tid; o < nOut; o += NT) {
        int off0, off1, c = -1, v = 0;
        if (o < 28) {
          int i = 0;
          while ((i + 1) * (i + 2) / 2 <= o) ++i;
          const int j = o - i * (i + 1) / 2;
          off0 = i * 16 + j;
          off1 = (7 + i) * 16 + 7 + j;
        } else if (o < 35) {
          off0 = (o - 28) * 16 + 14;
          off1 = (7 + o - 28) * 16 + 14;
        } else if (o == 35) {
          off0 = 256 + 40 * G;
          off1 = -1;
        } else {
          const int e = o - 36;
          c = e / G;
          v = e - c * G;
          if (c < 7) { off0 = 256 + c * G + v; off1 = 256 + 15 * G + (7 + c) * G + v; }
          else if (c == 7) { off0 = 256 + 14 * G + v; off1 = 256 + 29 * G + v; }
          else { off0 = 256 + 30 * G + (c - 8) * G + v; off1 = 256 + 35 * G + (c - 8) * G + v; }
        }
        double s = 0.0;
        for (int e = e0; e < e1; ++e) {
          const int code = dr.fpList[e];
          const int off = (code & 1) ? off1 : off0;
          if (off < 0) continue;
          for (int q = dr.recOff[code >> 1]; q < dr.recOff[(code >> 1) + 1]; ++q) s += dr.records[static_cast<size_t>(q) * recN + off];
        }
        if (o < 36) atomicAdd(&red[o], s);
        else if (c < 7) Hs[packedIdx(7 + v, c)] = s;
        else if (c == 7) gs[7 + v] = s;
        else {
          const int d = c - 8;
          const int v2 = v + (d == 0 ? 0 : (d == 1 ? 1 : L.gx + d - 3));
          if (v2 < G) atomicAdd(&Hs[packedIdx(7 + v2, 7 + v)], s);  // (gx = 2: bands 1 and 2 are the same vertex pair)
        }
      }
    }
  } else
  if (L.includeStatic) {
    // one unit (slice of a (pair, side) entry) per WAVE at a time: the waves run through their units independently
    // (no barrier until the end), 64 lanes over the slice's constraints
    if constexpr (SPEC != 0 && NT > 64) {
      // segments, one contiguous run of the part's units per wave (the one-wave deterministic build keeps the unit loop below)
      const AsmSegs segs = asmSegsFromArgument(dr);
      asmWalkSegments<KD, SPEC, STAGE>(L, T, x, fc, f, segs, wv, lane, xf, xstage, Hs, gs, PP, gp, GD, cost);
    } else {
    ASM_WAIT_DECL;
    for (int u = me.u0 + wv; u < me.u1; u += NT / 64) {
      if constexpr (SPEC != 0) ASM_WAIT_BEGIN();
      const int2 unit = work.units[u];
      const int code = __builtin_amdgcn_readfirstlane(unit.x);
      if constexpr (SPEC != 0) ASM_WAIT_LAP(0);
      const int p = code >> 1;
      const int side = code & 1;  // 0: f is the source of pair p, 1: f is the target
      const int o = side ? T.pairA[p] : T.pairB[p];
      const double* __restrict__ xo = x + static_cast<size_t>(o) * B;
      const FrameConst& Fa = side ? fc[o] : fc[f];
      const FrameConst& Fb = side ? fc[f] : fc[o];
      double* xw = xstage + wv * B;
      if constexpr (SPEC != 0) {
        const long long pOff = T.pairOff[p];
        const long long cb = pOff + __builtin_amdgcn_readfirstlane(unit.y);
        const long long pEnd = T.pairOff[p + 1];
        const int n = static_cast<int>((cb + kAsmUnit < pEnd ? cb + kAsmUnit : pEnd) - cb);
#ifdef CVD_ASM_PROFILE
        asm volatile("" :: "s"(o), "s"(n));  // (the header's values are formed in front of the stamp)
#endif
        ASM_WAIT_LAP(1);
        RecordStream<false> rs;
        rs.prime(T, cb, lane, n);
        // (the unit's first record is requested before the staging copy: one round trip for both; LDS ordering as below)
        if constexpr (STAGE) {
          for (int i = lane; i < B; i += 64) xw[i] = xo[i];
          asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        }
        const double* xov = STAGE ? xw : xo;
        asmWalkSpec<KD, SPEC>(L, T, rs, cb, n, lane, side != 0, Fa, Fb, side ? xov : xf,
                              side ? xf : xov, Hs, gs, PP, gp, GD, cost ASM_WAIT_ARGS);
        ASM_WAIT_LAP(3);
#ifdef CVD_ASM_PROFILE
        ++asmT[4];
#endif
        continue;
      }
      if constexpr (STAGE) {
        // (a wave's LDS operations execute in order: its own earlier reads of the buffer are done before these writes land, and
        // the reads below see them -- no workgroup barrier, the waves walk their units independently)
        for (int i = lane; i < B; i += 64) xw[i] = xo[i];
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
      }
      const double* xa = STAGE ? (side ? xw : xf) : (side ? xo : xf);
      const double* xb = STAGE ? (side ? xf : xw) : (side ? xf : xo);
      const double fya = Fa.fy, fxa = Fa.fy * A;
      const double fyb = Fb.fy;
      const double ifyb = 1.0 / fyb, ifxb = 1.0 / (fyb * A);
      const long long cBegin = T.pairOff[p] + __builtin_amdgcn_readfirstlane(unit.y);
      constexpr int kUnit = DENSE ? kAsmUnitDense : kAsmUnit;
      const long long cEnd = cBegin + kUnit < T.pairOff[p + 1] ? cBegin + kUnit : T.pairOff[p + 1];
      const int fsrc = side ? o : f, ftgt = side ? f : o;
      // list mode: lane = constraint, stride 64; dense mode: every lane walks its own run of kDenseRun pixels
      const long long cFirst = DENSE ? cBegin + static_cast<long long>(lane) * kDenseRun : cBegin + lane;
      const long long cStop = DENSE ? (cFirst + kDenseRun < cEnd ? cFirst + kDenseRun : cEnd) : cEnd;
      constexpr long long cStep = DENSE ? 1 : 64;
      // (list mode: no RecordStream -- a unit is two trips per lane and the kernel sits at its 256-register budget, the six
      // registers of a record in flight spill: 0.33 -> 0.35 ms.  Dense mode: mask and flow of the lane's next pixel in flight)
      RecordStream<true> rs;
      const int iFirst = static_cast<int>(cFirst - cBegin), iStop = static_cast<int>(cStop - cBegin);
      if constexpr (DENSE) rs.prime(T, cBegin, iFirst, iStop);
      for (long long c = cFirst; c < cStop; c += cStep) {
        float4 nd;
        float2 d;
        if constexpr (DENSE) {
          if (!rs.take(T, cBegin, static_cast<int>(c - cBegin), 1, iStop, T.pairOff[p], fsrc, ftgt, nd, d)) continue;
        } else {
          if (!loadConstraint<false>(T, c, T.pairOff[p], fsrc, ftgt, nd, d)) continue;
        }
        const double da = static_cast<double>(d.x), db = static_cast<double>(d.y);
        FastTaps<KD> ta, tb;
        fastGather<KD>(L, nd.x, nd.y, ta);
        fastGather<KD>(L, nd.z, nd.w, tb);
        double Da, Db;
        if (N == 0) {
          Da = da; Db = db;
        } else {
          Da = 0.0; Db = 0.0;
#pragma unroll
          for (int k = 0; k < KD; ++k) {
            if (ta.ok(k)) {
              const int ia = ta.I(k);
              if (N == 2) Da += (da * xa[7 + ia * 2] + xa[7 + ia * 2 + 1]) * ta.Wt(k);
              else Da += da * xa[7 + ia] * ta.Wt(k);
            }
            if (tb.ok(k)) {
              const int ib = tb.I(k);
              if (N == 2) Db += (db * xb[7 + ib * 2] + xb[7 + ib * 2 + 1]) * tb.Wt(k);
              else Db += db * xb[7 + ib] * tb.Wt(k);
            }
          }
        }
        const double pax = static_cast<double>(nd.x), pay = static_cast<double>(nd.y);
        const double pbx = static_cast<double>(nd.z), pby = static_cast<double>(nd.w);
        const double ca[3] = {pax * fxa, pay * fya, -1.0};
        const double Rca[3] = {dot3(Fa.R, ca), dot3(Fa.R + 3, ca), dot3(Fa.R + 6, ca)};
        const double v[3] = {Fa.t[0] + Rca[0] * Da - Fb.t[0], Fa.t[1] + Rca[1] * Da - Fb.t[1],
                             Fa.t[2] + Rca[2] * Da - Fb.t[2]};
        const double q0 = Fb.R[0] * v[0] + Fb.R[3] * v[1] + Fb.R[6] * v[2];
        const double q1 = Fb.R[1] * v[0] + Fb.R[4] * v[1] + Fb.R[7] * v[2];
        const double q2 = Fb.R[2] * v[0] + Fb.R[5] * v[1] + Fb.R[8] * v[2];
        const double zz = -q2;
        const double iz = 1.0 / zz;
        const double u = q0 * iz * ifxb;
        const double vv = q1 * iz * ifyb;
        double r[3];
        r[0] = (u - pbx) * L.ws;
        r[1] = (vv - pby) * L.ws;
        double dr2dA, dr2dDb;
        if (L.lossType == kLossDisparity) {
          const bool zo = !(zz < eps), bo = !(Db < eps);
          const double izc = zo ? iz : 1.0 / eps, ibc = 1.0 / (bo ? Db : eps);
          r[2] = (izc - ibc) * L.wd;
          dr2dA = zo ? (-L.wd * izc * izc) : 0.0;
          dr2dDb = bo ? (L.wd * ibc * ibc) : 0.0;
        } else {
          const bool zIsMax = !(zz < Db), zIsMin = !(Db < zz);
          const double mx = zIsMax ? zz : Db, mn = zIsMin ? zz : Db;
          if (L.lossType == kLossRatio) {
            r[2] = (mx / mn - 1.0) * L.wd;
            const double dmx = 1.0 / mn, dmn = -mx / (mn * mn);
            dr2dA = ((zIsMax ? dmx : 0.0) + (zIsMin ? dmn : 0.0)) * L.wd;
            dr2dDb = ((zIsMax ? 0.0 : dmx) + (zIsMin ? 0.0 : dmn)) * L.wd;
          } else {
            r[2] = log(mn / mx) * L.wd;
            const double dmn = 1.0 / mn, dmx = -1.0 / mx;
            dr2dA = ((zIsMax ? dmx : 0.0) + (zIsMin ? dmn : 0.0)) * L.wd;
            dr2dDb = ((zIsMax ? 0.0 : dmx) + (zIsMin ? 0.0 : dmn)) * L.wd;
          }
        }
        double rho0, w;  // rho, rho'
        robustRho(L, r[0] * r[0] + r[1] * r[1] + r[2] * r[2], rho0, w);
        if (!side) cost += rho0;

        // d r / d q (rows): M0 = (m00, 0, m02), M1 = (0, m11, m12), M2 = (0, 0, m22)
        const double wiz = L.ws * iz;
        const double m00 = wiz * ifxb, m11 = wiz * ifyb, m02 = wiz * u, m12 = wiz * vv, m22 = -dr2dA;
        double Jp[3][7];
        double JD[3];
        const FastTaps<KD>& tm = side ? tb : ta;
        const double dm = side ? db : da;
        if (!side) {
          // G = M R_b^T ; columns: t -> G, w_i -> G (D_a dR_a,i c_a), fy -> G (D_a R_a cf), D -> G R c_a
          double G[3][3];
#pragma unroll
          for (int i = 0; i < 3; ++i) {
            G[0][i] = m00 * Fb.R[i * 3 + 0] + m02 * Fb.R[i * 3 + 2];
            G[1][i] = m11 * Fb.R[i * 3 + 1] + m12 * Fb.R[i * 3 + 2];
            G[2][i] = m22 * Fb.R[i * 3 + 2];
          }
          const double cf[3] = {pax * A, pay, 0.0};
          const double dXdf[3] = {Da * (Fa.R[0] * cf[0] + Fa.R[1] * cf[1]), Da * (Fa.R[3] * cf[0] + Fa.R[4] * cf[1]),
                                  Da * (Fa.R[6] * cf[0] + Fa.R[7] * cf[1])};
#pragma unroll
          for (int rr = 0; rr < 3; ++rr) {
            Jp[rr][0] = G[rr][0]; Jp[rr][1] = G[rr][1]; Jp[rr][2] = G[rr][2];
            Jp[rr][6] = dot3(G[rr], dXdf);
            JD[rr] = dot3(G[rr], Rca);
          }
#pragma unroll
          for (int i = 0; i < 3; ++i) {
            const double dX[3] = {Da * dot3(Fa.dR[i], ca), Da * dot3(Fa.dR[i] + 3, ca), Da * dot3(Fa.dR[i] + 6, ca)};
            Jp[0][3 + i] = dot3(G[0], dX);
            Jp[1][3 + i] = dot3(G[1], dX);
            Jp[2][3 + i] = dot3(G[2], dX);
          }
        } else {
#pragma unroll
          for (int i = 0; i < 3; ++i) {
            Jp[0][i] = -(m00 * Fb.R[i * 3 + 0] + m02 * Fb.R[i * 3 + 2]);
            Jp[1][i] = -(m11 * Fb.R[i * 3 + 1] + m12 * Fb.R[i * 3 + 2]);
            Jp[2][i] = -(m22 * Fb.R[i * 3 + 2]);
            const double* D = Fb.dR[i];  // d q / d w_b,i = dR_b,i^T v
            const double dq0 = D[0] * v[0] + D[3] * v[1] + D[6] * v[2];
            const double dq1 = D[1] * v[0] + D[4] * v[1] + D[7] * v[2];
            const double dq2 = D[2] * v[0] + D[5] * v[1] + D[8] * v[2];
            Jp[0][3 + i] = m00 * dq0 + m02 * dq2;
            Jp[1][3 + i] = m11 * dq1 + m12 * dq2;
            Jp[2][3 + i] = m22 * dq2;
          }
          Jp[0][6] = -L.ws * u * ifyb;
          Jp[1][6] = -L.ws * vv * ifyb;
          Jp[2][6] = 0.0;
          JD[0] = 0.0; JD[1] = 0.0; JD[2] = dr2dDb;
        }
        if (L.intrOpt == kIntrShared) {
          // one focal length: column = d r / d f_a + d r / d f_b (the other side's part is added here)
          if (!side) {
            Jp[0][6] += -L.ws * u * ifyb;
            Jp[1][6] += -L.ws * vv * ifyb;
          } else {
            const double cf[3] = {pax * A, pay, 0.0};
            const double dXdf[3] = {Da * (Fa.R[0] * cf[0] + Fa.R[1] * cf[1]), Da * (Fa.R[3] * cf[0] + Fa.R[4] * cf[1]),
                                    Da * (Fa.R[6] * cf[0] + Fa.R[7] * cf[1])};
#pragma unroll
            for (int i = 0; i < 3; ++i) {
              Jp[0][6] += (m00 * Fb.R[i * 3 + 0] + m02 * Fb.R[i * 3 + 2]) * dXdf[i];
              Jp[1][6] += (m11 * Fb.R[i * 3 + 1] + m12 * Fb.R[i * 3 + 2]) * dXdf[i];
              Jp[2][6] += (m22 * Fb.R[i * 3 + 2]) * dXdf[i];
            }
          }
          if (!side) {
            shG += w * (Jp[0][6] * r[0] + Jp[1][6] * r[1] + Jp[2][6] * r[2]);
            shH += w * (Jp[0][6] * Jp[0][6] + Jp[1][6] * Jp[1][6] + Jp[2][6] * Jp[2][6]);
          }
        }
        // ---- accumulate
        int qi = 0;
#pragma unroll
        for (int i = 0; i < 7; ++i) {
          gp[i] += w * (Jp[0][i] * r[0] + Jp[1][i] * r[1] + Jp[2][i] * r[2]);
#pragma unroll
          for (int j = 0; j <= i; ++j) {
            PP[qi] += w * (Jp[0][i] * Jp[0][j] + Jp[1][i] * Jp[1][j] + Jp[2][i] * Jp[2][j]);
            ++qi;
          }
        }
        if (N > 0) {
          double v7[7];
#pragma unroll
          for (int i = 0; i < 7; ++i) v7[i] = w * (Jp[0][i] * JD[0] + Jp[1][i] * JD[1] + Jp[2][i] * JD[2]);
          const double sDD = w * (JD[0] * JD[0] + JD[1] * JD[1] + JD[2] * JD[2]);
          const double sDr = w * (JD[0] * r[0] + JD[1] * r[1] + JD[2] * r[2]);
          if constexpr (KD == 16) {
            // bicubic: column factors come straight from the separable weights, taps outside the folded
            // footprint are skipped (d/d theta_k[0] = w_k d, d/d theta_k[1] = w_k)
#pragma unroll
            for (int ka = 0; ka < 16; ++ka) {
              if (!tm.ok(ka)) continue;
              const double wa = tm.Wt(ka);
              const int ia = tm.I(ka);
#pragma unroll
              for (int na = 0; na < 2; ++na) {
                if (na >= N) continue;
                const int ct = 7 + ia * N + na;
                const double fa = (N == 2 && na == 1) ? wa : wa * dm;
                const int rowBase = ct * (ct + 1) / 2;
                atomicAdd(&gs[ct], sDr * fa);
#pragma unroll
                for (int i = 0; i < 7; ++i) atomicAdd(&Hs[rowBase + i], v7[i] * fa);
#pragma unroll
                for (int kb = 0; kb <= ka; ++kb) {
                  if (!tm.ok(kb)) continue;
                  const double wb = tm.Wt(kb);
                  const int ib = tm.I(kb);
#pragma unroll
                  for (int nb = 0; nb < 2; ++nb) {
                    if (nb >= N || (kb == ka && nb > na)) continue;
                    const int c2 = 7 + ib * N + nb;
                    const double fb = (N == 2 && nb == 1) ? wb : wb * dm;
                    atomicAdd(&Hs[rowBase + c2], sDD * fa * fb);  // tap order is index order: c2 <= ct
                  }
                }
              }
            }
          } else {
          // tap column factors: value params (d/d theta_k[0] = w_k d, d/d theta_k[1] = w_k)
          double fac[KD * 2];
          int col[KD * 2];
#pragma unroll
          for (int k = 0; k < KD; ++k) {
            if (N == 2) {
              col[2 * k] = 7 + tm.I(k) * 2;       fac[2 * k] = tm.Wt(k) * dm;
              col[2 * k + 1] = col[2 * k] + 1;    fac[2 * k + 1] = tm.Wt(k);
            } else {
              col[k] = 7 + tm.I(k);               fac[k] = tm.Wt(k) * dm;
            }
          }
          const int nt = (N == 2) ? 2 * KD : KD;
          if constexpr (KD == 1) {
#pragma unroll
            for (int a = 0; a < 2; ++a) {
              if (a < nt) {
#pragma unroll
                for (int i = 0; i < 7; ++i) GD[a * 7 + i] += v7[i] * fac[a];
                GD[17 + a] += sDr * fac[a];
              }
            }
            GD[14] += sDD * fac[0] * fac[0];
            if (N == 2) { GD[15] += sDD * fac[1] * fac[0]; GD[16] += sDD * fac[1] * fac[1]; }
          } else {
#pragma unroll
          for (int a = 0; a < KD * 2; ++a) {
            if (a < nt) {
              const int ct = col[a];
              const int rowBase = ct * (ct + 1) / 2;
              atomicAdd(&gs[ct], sDr * fac[a]);
#pragma unroll
              for (int i = 0; i < 7; ++i) atomicAdd(&Hs[rowBase + i], v7[i] * fac[a]);
#pragma unroll
              for (int b = 0; b < KD * 2; ++b) {
                if (b <= a) {
                  const int c2 = col[b];
                  const int hi = ct > c2 ? ct : c2, lo = ct > c2 ? c2 : ct;
                  atomicAdd(&Hs[packedIdx(hi, lo)], sDD * fac[a] * fac[b]);
                }
              }
            }
          }
          }
          }
        }
      }
    }
    if constexpr (SPEC != 0) ASM_WAIT_FLUSH();
    }
  }
  ASM_STAMP(4 + wv);  // each wave's end of the constraint loop
  __syncthreads();
  if (tid == 0) ASM_STAMP(2);
  {
#pragma unroll
    for (int i = 0; i < 28; ++i) PP[i] = waveSum(PP[i]);
#pragma unroll
    for (int i = 0; i < 7; ++i) gp[i] = waveSum(gp[i]);
    cost = waveSum(cost);
    if constexpr (KD == 1) {
      if (N > 0) {
#pragma unroll
        for (int i = 0; i < 19; ++i) GD[i] = waveSum(GD[i]);
        if (lane == 0) {
          for (int a = 0; a < N; ++a) {
            const int ct = 7 + a;
            for (int i = 0; i < 7; ++i) atomicAdd(&Hs[ct * (ct + 1) / 2 + i], GD[a * 7 + i]);
            atomicAdd(&gs[ct], GD[17 + a]);
          }
          atomicAdd(&Hs[packedIdx(7, 7)], GD[14]);
          if (N == 2) { atomicAdd(&Hs[packedIdx(8, 7)], GD[15]); atomicAdd(&Hs[packedIdx(8, 8)], GD[16]); }
        }
      }
    }
    if (lane == 0) {
#pragma unroll
      for (int i = 0; i < 28; ++i) atomicAdd(&red[i], PP[i]);
#pragma unroll
      for (int i = 0; i < 7; ++i) atomicAdd(&red[28 + i], gp[i]);
      atomicAdd(&red[35], cost);
    }
  }
  __syncthreads();
  if (tid < 28) {
    int i = 0;
    while ((i + 1) * (i + 2) / 2 <= tid) ++i;
    const int j = tid - i * (i + 1) / 2;
    Hs[packedIdx(i, j)] += red[tid];
  } else if (tid < 35) {
    gs[tid - 28] += red[tid];
  }
  __syncthreads();
  const double staticCost = 0.5 * red[35];
  __syncthreads();
  if constexpr (SPEC != 0) {
    asmLocalToAxisAngle<NT>(fc[f].Jl, B, tid, Hs, gs);
    __syncthreads();
  }
  if (tid == 0) ASM_STAMP(13);
  if (L.intrOpt == kIntrShared) {
    // The focal column of every constraint belongs to frame 0's slot: publish this frame's static focal
    // gradient / diagonal for k_shared_focal_fixup and drop the entries from the frame's own block (for f != 0
    // they are off-diagonal couplings with frame 0, which the block-Jacobi preconditioner does not hold).
    shG = waveSum(shG);
    shH = waveSum(shH);
    if (lane == 0) { red[wv] = shG; red[16 + wv] = shH; }
    __syncthreads();
    if (tid == 0) {
      double sg = 0.0, sh = 0.0;
      for (int w = 0; w < NT / 64; ++w) { sg += red[w]; sh += red[16 + w]; }
      focalG[f] = sg;  // (a split frame: overwritten with the sum over the parts below)
      focalH[f] = sh;
      red[42] = sg;
      red[43] = sh;
      gs[6] = 0.0;
      Hs[packedIdx(6, 6)] = 0.0;
    }
    if (f != 0) {
      for (int j = tid; j < B; j += NT)
        if (j != 6) Hs[j > 6 ? packedIdx(j, 6) : packedIdx(6, j)] = 0.0;
    }
    __syncthreads();
  }

  if (tid == 0) ASM_STAMP(14);
  double regCost = 0.0;
  if constexpr (SPEC != 0) {
    if (regOwner[f] && me.part == 0) regCost = asmRegularisersSpec<KD, NT>(L, f, tid, xf, median[f], Hs, gs);
  } else
  if (regOwner[f] && me.part == 0) {
    const int nr = numRegResiduals<KD>(L);
    for (int i = tid; i < nr; i += NT) {
      double r;
      int n;
      int cols[2 * KD + 2];
      double jac[2 * KD + 2];
      regResidual<KD>(L, f, i, xf, median[f], r, n, cols, jac);
      regCost += r * r;
      for (int a = 0; a < n; ++a) {
        atomicAdd(&gs[cols[a]], jac[a] * r);
        for (int b = 0; b <= a; ++b) {
          const int hi = cols[a] > cols[b] ? cols[a] : cols[b];
          const int lo = cols[a] > cols[b] ? cols[b] : cols[a];
          atomicAdd(&Hs[packedIdx(hi, lo)], jac[a] * jac[b]);
        }
      }
    }
  }
  if (tid == 0 && L.positionRegSqrt > 0.0 && me.part == 0) {
    double o3[3] = {0, 0, 0}, dg = 0.0, cst = 0.0;
    posRegFrame(L, rangeFlags, f, x, nullptr, o3, dg, cst);
    for (int i = 0; i < 3; ++i) {
      atomicAdd(&gs[i], o3[i]);
      atomicAdd(&Hs[packedIdx(i, i)], dg);
    }
    regCost += cst;
  }
  regCost = waveSum(regCost);
  __syncthreads();
  if (tid == 0) ASM_STAMP(15);
  if (lane == 0) red[wv] = regCost;
  __syncthreads();
  if (tid == 0) {
    double rc = 0.0;
    for (int w = 0; w < NT / 64; ++w) rc += red[w];
    if (me.nParts == 1) costFrame[f] = staticCost + 0.5 * rc;
    red[40] = staticCost + 0.5 * rc;
  }
  if (me.nParts > 1) {
    // split frame: publish this part's packed block / gradient / cost; the last part to arrive folds the others in
    __syncthreads();
    const size_t stride = static_cast<size_t>(npk) + B + 4;
    double* mine = work.scratch + static_cast<size_t>(me.slot0 + me.part) * stride;
    for (int i = tid; i < npk; i += NT) mine[i] = Hs[i];
    for (int i = tid; i < B; i += NT) mine[npk + i] = gs[i];
    if (tid == 0) {
      mine[npk + B] = red[40];
      if (L.intrOpt == kIntrShared) { mine[npk + B + 1] = red[42]; mine[npk + B + 2] = red[43]; }
    }
    if (!lastBlockArrives(work.counters + f, static_cast<unsigned int>(me.nParts), reinterpret_cast<int*>(red + 41))) return;
#if CVD_DETERMINISTIC
    // (which part arrives last is a matter of timing: fold ALL parts in index order, this one's from its published copy)
    double costSum = 0.0, sgSum = 0.0, shSum = 0.0;
    for (int i = tid; i < npk; i += NT) Hs[i] = 0.0;
    for (int i = tid; i < B; i += NT) gs[i] = 0.0;
    for (int q = 0; q < me.nParts; ++q) {
#else
    double costSum = red[40];
    double sgSum = red[42], shSum = red[43];
    for (int q = 0; q < me.nParts; ++q) {
      if (q == me.part) continue;
#endif
      const double* other = work.scratch + static_cast<size_t>(me.slot0 + q) * stride;
      for (int i = tid; i < npk; i += NT) Hs[i] += other[i];
      for (int i = tid; i < B; i += NT) gs[i] += other[npk + i];
      costSum += other[npk + B];
      if (L.intrOpt == kIntrShared) { sgSum += other[npk + B + 1]; shSum += other[npk + B + 2]; }
    }
    if (tid == 0) {
      costFrame[f] = costSum;
      if (L.intrOpt == kIntrShared) { focalG[f] = sgSum; focalH[f] = shSum; }
    }
    __syncthreads();
  }

  if (tid == 0) ASM_STAMP(3);
  const double* mf = mask + static_cast<size_t>(f) * B;
  for (int i = tid; i < B; i += NT) gOut[static_cast<size_t>(f) * B + i] = gs[i] * mf[i];
  double* hf = hOut + static_cast<size_t>(f) * B * B;
  for (int idx = tid; idx < B * B; idx += NT) {
    const int i = idx / B, j = idx - i * B;
    const int hi = i > j ? i : j, lo = i > j ? j : i;
    hf[idx] = Hs[packedIdx(hi, lo)] * mf[i] * mf[j];
  }
  if (tid == 0) ASM_STAMP(12);
}

}  // namespace cvd
