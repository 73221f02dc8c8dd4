// cvd_pcg.h -- the per-frame kernels of a PCG iteration and of the LM step around it (kernel map: cvd_kernels.h, which
// also holds the pair product and pcgFinishScalars, shared with the levels' headers).
#pragma once

#include "cvd_kernels.h"

namespace cvd {

// ---------------------------------------------------------------------------------------------------
// LM diagonal (Ceres LevenbergMarquardtStrategy::ComputeStep in the unscaled variables):
//   scale_j = 1 / (1 + sqrt(h_jj)) from the FIRST Jacobian; lam_j = clamp(scale_j^2 h_jj) / (radius scale_j^2).
// Unknowns nothing depends on (h_jj == 0: constant or absent parameter blocks) get lam = 1, so that the
// damped system is the identity on them and their step is exactly 0.
// ---------------------------------------------------------------------------------------------------
// hdiag = diag(H_ff) of every frame as a flat F x B vector (k_extract_diag; all-gathered from the frames' owners in the
// pair-sharded multi-GPU mode, where a rank holds the reduced H_ff of its own frames only).
inline __global__ void k_lm_diag(Layout L, const double* __restrict__ hdiag, double* __restrict__ scale,
                          int computeScale, double radius, double* __restrict__ lam) {
  const size_t n = static_cast<size_t>(L.F) * L.B;
  const size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double h = hdiag[i];
  if (computeScale) scale[i] = 1.0 / (1.0 + sqrt(h));
  const double s = scale[i];
  if (h == 0.0) {
    lam[i] = 1.0;
  } else {
    const double d = fmin(fmax(s * s * h, 1e-6), 1e32);
    lam[i] = d / (radius * s * s);
  }
}

template <int KD>
inline __global__ __launch_bounds__(256) void k_reg_cache(Layout L, const double* __restrict__ x,
                                                   const float* __restrict__ median,
                                                   const unsigned char* __restrict__ owner, RegCache rc) {
  extern __shared__ __attribute__((aligned(16))) double sm[];  // the frame's parameters (see k_cost_frames)
  const int f = blockIdx.x;
  if (!owner[f]) return;
  for (int i = threadIdx.x; i < L.B; i += 256) sm[i] = x[static_cast<size_t>(f) * L.B + i];
  __syncthreads();
  const float med = median[f];
  for (int i = threadIdx.x; i < rc.nr; i += 256) {
    double r;
    int n;
    int cols[2 * KD + 2];
    double jac[2 * KD + 2];
    regResidual<KD>(L, f, i, sm, med, r, n, cols, jac);
    rc.cnt[static_cast<size_t>(f) * rc.nr + i] = static_cast<unsigned char>(n);
    for (int a = 0; a < n; ++a) {
      const size_t e = (static_cast<size_t>(f) * rc.stride + a) * rc.nr + i;
      rc.jac[e] = jac[a];
      rc.col[e] = static_cast<unsigned short>(cols[a]);
    }
  }
}

// Direction and product element `tid` of the frame (B <= 256), handed from the finish half to the update half of the fused
// tail kernel (k_pcg_tail) in registers.
struct TailCarry {
  double pv, qv;
};

// Per frame: p_f = z + beta p_old (stored for the next iteration), q_f = mask * (sum of partials +
// regulariser J^T J p) + lam * p_f, and the frame's share of p.q.
// Body of k_matvec_finish.  FUSED = false: the kernel of that name (256 threads per frame).  FUSED = true: the first half of
// k_pcg_tail -- the workgroup may be larger than 256 threads (threads beyond B idle through the barriers), nothing is handed to
// a last workgroup (the caller's grid barrier follows), Z^T q is PUBLISHED (agent-scope stores: other workgroups of the same
// launch read it), and the direction / product of element tid stay in registers (carry).  Returns false when the PCG has
// converged already (uniform over the launch; nothing was written).
template <int KD, bool FUSED>
__device__ __forceinline__ bool matvecFinishBody(const Layout& L, const double* __restrict__ x,
                                                 const double* __restrict__ mask,
                                                 const double* __restrict__ lam, const float* __restrict__ median,
                                                 const unsigned char* __restrict__ inRange,
                                                 const unsigned char* __restrict__ rangeFlags,
                                                 const int* __restrict__ fiOff, const int* __restrict__ fiList,
                                                 const double* __restrict__ qPart, const double* __restrict__ z,
                                                 const double* __restrict__ pOld, double* __restrict__ pNew,
                                                 double* __restrict__ scal, unsigned int* __restrict__ counter,
                                                 int useBeta, double* __restrict__ q, double* __restrict__ fdot,
                                                 int distMode, int nRows, const RegCache& rc, const CoarseView& V,
                                                 double* __restrict__ qc, const CoarseColumns& cc,
                                                 const double* __restrict__ Hdiag, double* __restrict__ pqOut,
                                                 int ownFirst, int ownCount, double* __restrict__ sm, TailCarry& carry,
                                                 const TlStep* __restrict__ tsp, double* __restrict__ tlPart) {
  // Hdiag != nullptr (explicit cross blocks, cvd_cross.h): the partial rows hold the OFF-diagonal blocks' products only;
  // the frame-diagonal part, regularisers included, is H_ff p_f with the assembled H_ff.
  const double sDone = scal[S_DONE];  // PCG already converged (iterations enqueued ahead): tested after the input loads
  const int nT = FUSED ? static_cast<int>(blockDim.x) : 256;  // stride of the loops that are not bounded by B
  const int B = L.B;
  double* xf = sm;
  double* pf = xf + B;   // masked direction
  double* qf = pf + B;
  double* red = qf + B;
  double* cl = red + 8;  // kCB coarse corrections of this frame
  const int f = blockIdx.x;
  const int tid = threadIdx.x;
  const double beta = useBeta ? scal[S_BETA] : 0.0;
  const size_t base = static_cast<size_t>(f) * B;
  // (FUSED: the row range first -- it is the one address the row walk below waits for -- and whether the frame has regulariser rows:
  // asked here, not behind the barriers; k_matvec_finish asks where it always did)
  int e0 = 0, e1 = 0;
  bool regRowsOn = false;
  if constexpr (FUSED) {
    e0 = fiOff[f];
    e1 = fiOff[f + 1];
    regRowsOn = Hdiag == nullptr && inRange[f];
  }
  // One global round trip for the inputs (B <= 256: one element per thread): the loads of z / mask / p_old / x / lam
  // are issued together with the coarse correction's, the direction is formed after the barrier and stays in a
  // register for the damping term and p.q at the end.
  if (V.Wb != nullptr) {
    if (tid < 64) coarseFrameCorrection(V, f, tid, cl);
  } else if (tid < kCB) {
    cl[tid] = (V.cF != nullptr) ? V.cF[f * kCB + tid] : 0.0;
  }
  // (two elements per thread: B <= 512; the fused kernel's scope ends at B = 256: one)
  constexpr int EPT = FUSED ? 1 : 2;
  double vz[2] = {0.0, 0.0}, vm[2] = {0.0, 0.0}, vp[2] = {0.0, 0.0}, vlam[2] = {0.0, 0.0}, pvReg[2] = {0.0, 0.0};
  // third level (CoarseView::tl): the frame's coefficients to LDS (behind the row walk's partial sums), the vertex taps to registers
  const bool tlOn = V.tl != nullptr;
  double* tls = cl + kCB + (FUSED ? ((nT >> 8) - 1) * 256 : 0);
  TlTaps tt[EPT];
  // (... and the thread's first entry of the transposed table for the restriction at the end: no load left behind the product)
  float tlW0 = 0.f;
  int tlV0 = 0, tlEntries = 0;
  if (tlOn) {
    if (tid < V.tlS) tls[tid] = V.tl[static_cast<size_t>(f) * V.tlS + tid];
#pragma unroll
    for (int e = 0; e < EPT; ++e) tlLoadTaps(V, tid + e * 256, L.nD, tt[e]);
  }
  if (tsp != nullptr) {
    tlEntries = tsp->S * tsp->width;
    if (tid < tlEntries) {
      tlW0 = tsp->elW[tid];
      tlV0 = tsp->elV[tid];
    }
  }
#pragma unroll
  for (int e = 0; e < EPT; ++e) {
    const int i = tid + e * 256;
    if (i < B) {
      vz[e] = z[base + i];
      vm[e] = mask[base + i];
      if (useBeta) vp[e] = pOld[base + i];
      vlam[e] = lam[base + i];
      xf[i] = x[base + i];
    }
  }
  if constexpr (!FUSED) {
    e0 = fiOff[f];
    e1 = fiOff[f + 1];
  }
  // The frame's partial rows (contiguous; independent streaming loads, four in flight per thread) are summed BEFORE the
  // barrier: they depend on nothing but the row range, so their way from L2 overlaps the vector loads above instead of
  // following them (this kernel is a chain of dependent round trips, not a bandwidth problem).
  double rowSum[2] = {0.0, 0.0};
  double* psum = cl + kCB;  // FUSED: (blockDim / 256 - 1) x 256 partial sums of the row walk
  if (L.includeStatic) {
    if constexpr (FUSED) {
      // every 256 threads of the (larger) workgroup walk their own residue class of the rows: the walk is a chain of dependent
      // round trips -- 40 rows of a hub frame of the hierarchical flow list = 10 trips of 4 loads -- and that chain, not the
      // bytes, was the fused kernel's critical path (the slowest frame reached the grid barrier after 25 us)
      const int nParts = nT >> 8, part = tid >> 8, i = tid & 255;
      if (i < B && part < nParts) {
        const size_t step = static_cast<size_t>(nParts) * B;
        const double* rowp = qPart + static_cast<size_t>(e0 + part) * B + i;
        double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
        int r = e0 + part;
        for (; r + 3 * nParts < e1; r += 4 * nParts, rowp += 4 * step) {
          a0 += rowp[0];
          a1 += rowp[step];
          a2 += rowp[2 * step];
          a3 += rowp[3 * step];
        }
        for (; r < e1; r += nParts, rowp += step) a0 += rowp[0];
        const double t = (a0 + a1) + (a2 + a3);
        if (part == 0) rowSum[0] = t;
        else psum[(part - 1) * 256 + i] = t;
      }
    } else {
#pragma unroll
      for (int e = 0; e < EPT; ++e) {
        const int i = tid + e * 256;
        if (i >= B) continue;
        const double* rowp = qPart + static_cast<size_t>(e0) * B + i;
        double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
        int r = e0;
        for (; r + 3 < e1; r += 4, rowp += 4 * B) {
          a0 += rowp[0];
          a1 += rowp[B];
          a2 += rowp[2 * B];
          a3 += rowp[3 * B];
        }
        for (; r < e1; ++r, rowp += B) a0 += rowp[0];
        rowSum[e] = (a0 + a1) + (a2 + a3);
      }
    }
  }
  __syncthreads();
  if (sDone != 0.0) return false;  // uniform; nothing has been written to global memory yet
  if constexpr (FUSED) {
    if (L.includeStatic && tid < B)
      for (int k = 0; k + 1 < (nT >> 8); ++k) rowSum[0] += psum[k * 256 + tid];
  }
#pragma unroll
  for (int e = 0; e < EPT; ++e) {
    const int i = tid + e * 256;
    if (i >= B) continue;
    // search direction from the two-level preconditioned residual z + Z c (coarse part only on active unknowns)
    const double pv = vz[e] + (coarseAtLds(cl, L, i) + (tlOn ? tlAt(tls, tt[e]) : 0.0)) * vm[e] + (useBeta ? beta * vp[e] : 0.0);
    if constexpr (!FUSED) pNew[base + i] = pv;  // (FUSED: the caller stores carry.pv / carry.qv behind its arrival at the grid barrier)
    pvReg[e] = pv;
    pf[i] = pv * vm[e];
    // (no pair kernel ran: the partial buffer is stale; shared focal: frame 0's slot collects every row's entry below)
    qf[i] = (L.includeStatic && !(L.intrOpt == kIntrShared && i == 6)) ? rowSum[e] : 0.0;
  }
  __syncthreads();
  if (L.intrOpt == kIntrShared && f == 0 && L.includeStatic) {
    // shared focal: frame 0's slot collects the focal adjoint of EVERY partial row (both sides of every pair item, the
    // three rows of every triplet group)
    double a = 0.0;
    for (int k = tid; k < nRows; k += nT) a += qPart[static_cast<size_t>(k) * B + 6];
    a = waveSum(a);
    if ((tid & 63) == 0) atomicAdd(&qf[6], a);
    __syncthreads();
  }
  // (pair-sharded run: the reduced H_ff lives on the frame's OWNER rank only -- the others contribute the cross blocks of
  // their pairs and nothing else for this frame)
  if (Hdiag != nullptr && f >= ownFirst && f < ownFirst + ownCount) {
    // symmetric block: column access, coalesced over the row index; four independent loads in flight
    const double* Hf = Hdiag + static_cast<size_t>(f) * B * B;
    for (int i = tid; i < B; i += 256) {
      double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
      int j = 0;
      for (; j + 3 < B; j += 4) {
        a0 += Hf[static_cast<size_t>(j) * B + i] * pf[j];
        a1 += Hf[static_cast<size_t>(j + 1) * B + i] * pf[j + 1];
        a2 += Hf[static_cast<size_t>(j + 2) * B + i] * pf[j + 2];
        a3 += Hf[static_cast<size_t>(j + 3) * B + i] * pf[j + 3];
      }
      for (; j < B; ++j) a0 += Hf[static_cast<size_t>(j) * B + i] * pf[j];
      qf[i] += (a0 + a1) + (a2 + a3);
    }
    __syncthreads();
  } else if (FUSED ? regRowsOn : (Hdiag == nullptr && inRange[f])) {
    // J_reg^T (J_reg p) from the cached rows (k_reg_cache)
    // (deterministic build: the first wave alone -- the rows' LDS atomics then land in program order)
    const int regStride = CVD_DETERMINISTIC ? 64 : nT;
    for (int i = tid; i < rc.nr && tid < regStride; i += regStride) {
      const int n = rc.cnt[static_cast<size_t>(f) * rc.nr + i];
      const size_t e0 = static_cast<size_t>(f) * rc.stride * rc.nr + i;
      double t = 0.0;
      for (int a = 0; a < n; ++a) t += rc.jac[e0 + static_cast<size_t>(a) * rc.nr] * pf[rc.col[e0 + static_cast<size_t>(a) * rc.nr]];
      for (int a = 0; a < n; ++a)
        atomicAdd(&qf[rc.col[e0 + static_cast<size_t>(a) * rc.nr]], rc.jac[e0 + static_cast<size_t>(a) * rc.nr] * t);
    }
  }
  if (L.positionRegSqrt > 0.0 && tid < 3) {
    // neighbours' directions are re-formed from z / p_old (their pNew rows are being written concurrently)
    const double w = L.positionRegSqrt * L.positionRegSqrt;
    const double cf[3] = {1.0, -2.0, 1.0};
    double acc = 0.0;
    for (int o = 0; o < 3; ++o) {
      const int k = f - o;
      if (k < 0 || !posRegValid(L, rangeFlags, k)) continue;
      double a = 0.0;
      for (int j = 0; j < 3; ++j) {
        const size_t idx = static_cast<size_t>(k + j) * B + tid;
        a += cf[j] * (z[idx] + coarseAt(V.cF, L, k + j, tid) + (useBeta ? beta * pOld[idx] : 0.0)) * mask[idx];
      }
      acc += w * cf[o] * a;
    }
    atomicAdd(&qf[tid], acc);
  }
  __syncthreads();
  // distMode (pair-sharded multi-GPU): 1 = this rank adds the damping term, 2 = it does not; q is all-reduced afterwards.
  // pqOut == nullptr: p.q / alpha are formed by k_dot_pq on the reduced vector.  pqOut != nullptr (FUSED exchange): the
  // product, its restriction Z^T q and p.q are all linear in q, so this rank's shares of the three travel in ONE
  // all-reduce ([q | Z^T q | p.q] contiguous) and k_cg_update forms alpha from the reduced p.q itself.
  if (!FUSED && distMode && pqOut == nullptr) {
#pragma unroll
    for (int e = 0; e < EPT; ++e) {
      const int i = tid + e * 256;
      if (i < B) q[base + i] = qf[i] * vm[e] + (distMode == 1 ? vlam[e] * pvReg[e] : 0.0);
    }
    return true;
  }
  double dot = 0.0;
#pragma unroll
  for (int e = 0; e < EPT; ++e) {
    const int i = tid + e * 256;
    if (i >= B) continue;
    const double pv = pvReg[e];
    const double qv = qf[i] * vm[e] + (distMode == 2 ? 0.0 : vlam[e] * pv);
    if constexpr (!FUSED) q[base + i] = qv;
    qf[i] = qv;
    dot += pv * qv;
    if (e == 0) { carry.pv = pv; carry.qv = qv; }
  }
  dot = waveSum(dot);
  if ((tid & 63) == 0 && tid < 256) red[tid >> 6] = dot;  // (waves beyond the first four hold no element: B <= 256 when FUSED)
  __syncthreads();
  if (tid == 0) publishPartial(fdot + f, red[0] + red[1] + red[2] + red[3]);
  if (qc != nullptr) {  // Z^T q and this frame's column of W (Z^T q) for the fused y update (CoarseStep)
    coarseRestrict<FUSED>(L, qf, f, tid, V.modeActive, qc);
    if constexpr (!FUSED) {
      __syncthreads();
      coarseColumnProducts(cc, qc + f * kCB, f, tid, 256);
    }
  }
  if (tsp != nullptr) {
    // third level: spatial restriction of this frame's product, sq[f][s] = sum_v Hs[v][s] q_f[7 + v], by the transposed vertex
    // table (entry k of hat s; fixed summation order).  (The level's descriptor is read where it is used: as a kernel argument
    // its 24 scalar registers stayed live through both halves of k_pcg_tail and cost the update half spilled operands.)
    const TlStep ts = *tsp;
    if (tid < tlEntries) tlPart[tid] = static_cast<double>(tlW0) * qf[7 + tlV0];
    for (int e = tid + nT; e < tlEntries; e += nT) tlPart[e] = static_cast<double>(ts.elW[e]) * qf[7 + ts.elV[e]];
    __syncthreads();
    if (tid < ts.S) {
      double a = 0.0;
      for (int k = 0; k < ts.width; ++k) a += tlPart[k * ts.S + tid];
      storeMaybePublished(ts.sq + static_cast<size_t>(f) * ts.S + tid, a, FUSED);
    }
  }
  if constexpr (!FUSED) {
    // the last workgroup to arrive reduces p.q over the frames and publishes alpha for k_cg_update
    if (lastBlockArrivesLite(counter, L.F, reinterpret_cast<int*>(red + 6))) {
      const double pq = blockSumPartials(fdot, L.F, red);
      if (tid == 0) {
        if (pqOut != nullptr) {
          *pqOut = pq;  // (this rank's share: reduced with q)
        } else {
          scal[S_PQ] = pq;
          scal[S_ALPHA] = scal[S_RZ] / pq;
        }
      }
    }
  }
  return true;
}

template <int KD>
inline __global__ __launch_bounds__(256) void k_matvec_finish(Layout L, const double* __restrict__ x,
                                                       const double* __restrict__ mask,
                                                       const double* __restrict__ lam, const float* __restrict__ median,
                                                       const unsigned char* __restrict__ inRange,
                                                       const unsigned char* __restrict__ rangeFlags,
                                                       const int* __restrict__ fiOff, const int* __restrict__ fiList,
                                                       const double* __restrict__ qPart, const double* __restrict__ z,
                                                       const double* __restrict__ pOld, double* __restrict__ pNew,
                                                       double* __restrict__ scal, unsigned int* __restrict__ counter,
                                                       int useBeta, double* __restrict__ q, double* __restrict__ fdot,
                                                       int distMode, int nRows, RegCache rc, CoarseView V,
                                                       double* __restrict__ qc, CoarseColumns cc,
                                                       const double* __restrict__ Hdiag, double* __restrict__ pqOut,
                                                       int ownFirst, int ownCount, const TlStep* __restrict__ tsp) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  TailCarry carry;
  // (third level: its coefficients behind the coarse corrections, the restriction's products behind those)
  (void)matvecFinishBody<KD, false>(L, x, mask, lam, median, inRange, rangeFlags, fiOff, fiList, qPart, z, pOld, pNew, scal, counter,
                                    useBeta, q, fdot, distMode, nRows, rc, V, qc, cc, Hdiag, pqOut, ownFirst, ownCount, sm, carry, tsp,
                                    sm + 3 * L.B + 8 + kCB + kTlMaxS);
}

// p.q of the all-reduced product (multi-GPU only) + alpha, same last-workgroup pattern as k_matvec_finish.
inline __global__ __launch_bounds__(256) void k_dot_pq(Layout L, const double* __restrict__ p, const double* __restrict__ q,
                                                double* __restrict__ scal, unsigned int* __restrict__ counter,
                                                double* __restrict__ fdot, double* __restrict__ qc,
                                                const unsigned char* __restrict__ modeActive, CoarseColumns cc,
                                                const TlStep* __restrict__ tsp) {
  if (scal[S_DONE] != 0.0) return;  // PCG already converged (iterations enqueued ahead)
  __shared__ double red[8];
  __shared__ double prod[kTlMaxS * kTlMaxWidth];
  const int f = blockIdx.x, tid = threadIdx.x;
  const size_t base = static_cast<size_t>(f) * L.B;
  if (tsp != nullptr) {  // third level: spatial restriction of the all-reduced product (matvecFinishBody does it on the other paths)
    const TlStep ts = *tsp;
    const int nE = ts.S * ts.width;
    for (int e = tid; e < nE; e += 256) prod[e] = static_cast<double>(ts.elW[e]) * q[base + 7 + ts.elV[e]];
    __syncthreads();
    if (tid < ts.S) {
      double a = 0.0;
      for (int k = 0; k < ts.width; ++k) a += prod[k * ts.S + tid];
      ts.sq[static_cast<size_t>(f) * ts.S + tid] = a;
    }
  }
  if (qc != nullptr) {  // on the all-reduced q
    coarseRestrict(L, q + base, f, tid, modeActive, qc);
    __syncthreads();
    coarseColumnProducts(cc, qc + f * kCB, f, tid, 256);
  }
  double dot = 0.0;
  for (int i = tid; i < L.B; i += 256) dot += p[base + i] * q[base + i];
  dot = waveSum(dot);
  if ((tid & 63) == 0) red[tid >> 6] = dot;
  __syncthreads();
  if (tid == 0) publishPartial(fdot + f, red[0] + red[1] + red[2] + red[3]);
  if (lastBlockArrivesLite(counter, L.F, reinterpret_cast<int*>(red + 6))) {
    const double pq = blockSumPartials(fdot, L.F, red);
    if (tid == 0) {
      scal[S_PQ] = pq;
      scal[S_ALPHA] = scal[S_RZ] / pq;
    }
  }
}

// LDS doubles of k_cg_update's partial row sums (host and device agree on the layout)
__host__ __device__ inline int cgUpdatePartDoubles(int B, int nThreads) {
  return B > 256 ? nThreads : max(nThreads, 16 * ((B + 3) & ~3));
}

// Workgroup of the third level (TlStep) for coarse hat s: q_T = R_t sq over the frames of every temporal node (all NT entries: the
// rows need them all), the hat's nn rows of the inverse (one wave per row), t <- t - alpha A_T^-1 q_T, r_T <- r_T - alpha q_T, the
// hat's share of r^T P t, and the temporal interpolation of the new t for every frame (tl).  init: t = A_T^-1 q_T, r_T = q_T with
// sq = the restriction of the first residual.  LDS: NT + 2 nn doubles at sm.  Returns false when nothing was written.
#ifdef CVD_TAIL_PROFILE  // tools/tail_profile.py: wall-clock (100 MHz) stamps of k_pcg_tail's workgroups
// slots: 0 start, 1 finish half done, 2 operands requested, 3 released, 4 end, 5-7 levels (node sums, rows, interpolation),
// 8 levels: rows staged, 10 arrival done (first wave: ticket in hand; the releasing workgroup: records written)
__device__ unsigned long long g_tailProf[1024 * 16];
#define TAIL_STAMP(slot) do { if (threadIdx.x == 0) g_tailProf[(blockIdx.x & 1023) * 16 + (slot)] = wall_clock64(); } while (0)
#else
#define TAIL_STAMP(slot) do {} while (0)
#endif

struct NoMid {  // (the kernels that are not k_pcg_tail: nothing happens between the halves)
  __device__ bool first(double&, double&) { return true; }
  __device__ bool second(double&) { return true; }
  __device__ unsigned int generation() { return 0u; }
  __device__ bool stageRows() { return false; }
  // (k_pcg_tail's shares mode, below: the launch closes r^T z itself / a level's share goes where its descriptor says / no flag)
  __device__ bool closes() { return true; }
  __device__ double* levelShare(double* fromDescriptor) { return fromDescriptor; }
  __device__ void gaveUp() {}
};
// LDS doubles of a temporal level's workgroup in k_pcg_tail that stages its rows of the inverse in front of the grid barrier
// (tlLevelRows): the kTlSpan + 1 rows of NT doubles behind its tlRowsLds(NT) (host and device agree on the layout)
__host__ __device__ inline int tlStagedLds(int NT) { return tlRowsLds(NT) + (kTlSpan + 1) * NT; }
typedef unsigned int cvd_u32x4 __attribute__((ext_vector_type(4)));
template <bool FUSED, typename Mid>
__device__ __forceinline__ bool tlLevelRows(const TlStep* __restrict__ tsp, int wg, int F, double& alpha, int init, double sDone,
                                            const double* __restrict__ scal, double* __restrict__ sm, Mid& mid) {
  const TlStep ts = *tsp;
  const int tid = threadIdx.x, nThreads = blockDim.x;
  const int wv = tid >> 6, lane = tid & 63, nW = nThreads >> 6;
  // Workgroup = (hat s, node range): nodes [aLo, aHi] with aHi shared with the next range (both walk its row -- the frames between
  // two nodes need both coefficients -- the next range OWNS it: writes it, counts it).  One row per wave: span + 1 <= waves.
  const int s = wg / ts.parts, part = wg - s * ts.parts;
  const int aLo = part * ts.span, aHi = min(ts.nn - 1, aLo + ts.span), nA = aHi - aLo + 1;
  const bool ownsLast = part == ts.parts - 1;
  // t is double-buffered (a shared row's old coefficient is read by two workgroups while its owner writes the new one): iteration
  // k (S_ITERS = k - 1 applied) reads buffer (k - 1) & 1 and writes the other; the first residual writes buffer 0
  const int par = init ? 1 : (static_cast<int>(scal[S_ITERS]) & 1);
  const double* tin = ts.t + static_cast<size_t>(par) * ts.NT;
  double* tout = ts.t + static_cast<size_t>(par ^ 1) * ts.NT;
  double* qT = sm;                 // [S][nn]
  double* tn = qT + ts.NT;         // span + 1 new coefficients of this hat
  double* red = tn + ts.span + 1;  // span + 1 products t r_T, [span + 1 .. ]: flag
  // (the coefficients the wave's first row updates depend on nothing this launch computes: requested before the grid barrier.
  // The row itself -- 8 doubles per lane -- would spill at the 80 registers of k_pcg_tail if held across the barrier: the fused
  // kernel stages it in LDS instead, below.)
  double rOldPre = 0.0, tOldPre = 0.0;
  if (lane == 0 && !init) {
    const int e = s * ts.nn + aLo + (wv < nA ? wv : 0);
    rOldPre = ts.rT[e];
    tOldPre = tin[e];
  }
  // FUSED, staged: the rows themselves wait in LDS.  Every wave copies the row(s) it will walk -- they depend on nothing this
  // launch computes, and the workgroup idles in front of the barrier -- eight loads per lane in flight, stored as they are
  // consumed: nothing is held in registers across the barrier.  The product below reads the same entries in the same order.
  double* stage = sm + tlRowsLds(ts.NT);  // [span + 1][NT]
  bool staged = false;
  if constexpr (FUSED) {
    staged = mid.stageRows();
    if (staged) {
      constexpr int kStageBatch = 8;
      for (int k = wv; k < nA; k += nW) {
        const double* row = ts.Ainv + static_cast<size_t>(s * ts.nn + aLo + k) * ts.ld;
        double* dst = stage + static_cast<size_t>(k) * ts.NT;
        for (int c0 = 0; c0 < ts.NT; c0 += 64 * kStageBatch) {
          double v[kStageBatch];
#pragma unroll
          for (int u = 0; u < kStageBatch; ++u) {
            const int c = c0 + u * 64 + lane;
            v[u] = row[min(c, ts.NT - 1)];
          }
#pragma unroll
          for (int u = 0; u < kStageBatch; ++u) {
            const int c = c0 + u * 64 + lane;
            if (c < ts.NT) dst[c] = v[u];
          }
        }
      }
    }
    TAIL_STAMP(8);
  }
  bool on = false;
  if constexpr (FUSED) {
    on = *ts.fail == 0;  // (set when the level was built: asked in front of the grid barrier, not behind the node sums)
    if (!mid.second(alpha)) return false;
  }
  const double inv = 1.0 / static_cast<double>(ts.step);
  bool direct = true;
  if constexpr (FUSED) {
    if (ts.rec != nullptr) {
      // Node sums through the other workgroups of the level: every hat's workgroup sums ITS hat over the frames of each node (one
      // load per lane, one wave per node), the first range's publishes the nn sums as 16-byte records {generation, value,
      // generation}, and everybody collects the NT records -- 1 + 1 round trips instead of (2 step - 1) / 8 batches of loads
      // of the whole sq.  The generation is the grid barrier's (unique per launch; records zeroed with the barrier's words).
      direct = false;
      const unsigned int gen = mid.generation() + 1u;
      cvd_u32x4* rec = reinterpret_cast<cvd_u32x4*>(ts.rec);
      for (int a = wv; a < ts.nn; a += nW) {
        const int f = (a - 1) * ts.step + 1 + lane;
        const bool in = lane < 2 * ts.step - 1 && f >= 0 && f < F;
        double v = in ? readPartial(ts.sq + static_cast<size_t>(f) * ts.S + s) : 0.0;
        v *= 1.0 - fabs(static_cast<double>(f - a * ts.step)) * inv;
        v = waveSum(in ? v : 0.0);
        if (lane == 0 && part == 0) {
          cvd_u32x4 r4;
          r4.x = gen;
          r4.y = static_cast<unsigned int>(__double2loint(v));
          r4.z = static_cast<unsigned int>(__double2hiint(v));
          r4.w = gen;
          *reinterpret_cast<volatile cvd_u32x4*>(rec + s * ts.nn + a) = r4;
        }
      }
      int* bad = reinterpret_cast<int*>(red + ts.span + 1);
      if (tid == 0) *bad = 0;
      __syncthreads();
      for (int e = tid; e < ts.NT; e += nThreads) {
        const volatile cvd_u32x4* src = reinterpret_cast<const volatile cvd_u32x4*>(rec + e);
        cvd_u32x4 r4;
        unsigned int spins = 0;
        for (;;) {
          r4 = *src;
          if (r4.x == gen && r4.w == gen) break;
          __builtin_amdgcn_s_sleep(4);
          if (++spins > (1u << 20)) {  // (a workgroup of the level is not resident: give up, the host reports the stalled PCG)
            *bad = 1;
            break;
          }
        }
        qT[e] = __hiloint2double(static_cast<int>(r4.z), static_cast<int>(r4.y));
      }
      __syncthreads();
      if (*bad) {
        mid.gaveUp();
        return false;
      }
    }
  }
  if (direct) {
    for (int e = tid; e < ts.NT; e += nThreads) {  // e = a * S + s': neighbouring lanes read neighbouring words of a frame's row
      const int a = e / ts.S, sp = e - a * ts.S;
      const int fLo = max(0, (a - 1) * ts.step + 1), fHi = min(F - 1, (a + 1) * ts.step - 1);
      // (a node has up to 2 step - 1 frames: eight independent loads per batch, the walk is latency, not bytes)
      constexpr int kTlBatch = 8;
      double acc[4] = {0.0, 0.0, 0.0, 0.0};
      for (int f = fLo; f <= fHi; f += kTlBatch) {
        double v[kTlBatch];
#pragma unroll
        for (int u = 0; u < kTlBatch; ++u) {
          const double* src = ts.sq + static_cast<size_t>(min(f + u, fHi)) * ts.S + sp;
          v[u] = FUSED ? readPartial(src) : *src;
        }
#pragma unroll
        for (int u = 0; u < kTlBatch; ++u) {
          const double w = 1.0 - fabs(static_cast<double>(f + u - a * ts.step)) * inv;
          acc[u & 3] += (f + u <= fHi) ? w * v[u] : 0.0;
        }
      }
      qT[sp * ts.nn + a] = (acc[0] + acc[1]) + (acc[2] + acc[3]);
    }
    __syncthreads();
  }
  if (sDone != 0.0) return false;  // uniform; nothing written yet
  if constexpr (FUSED) TAIL_STAMP(5);
  if constexpr (!FUSED) on = *ts.fail == 0;
  for (int k = wv; k < nA; k += nW) {
    const int a = aLo + k, e = s * ts.nn + a;
    const double* row = ts.Ainv + static_cast<size_t>(e) * ts.ld;
    const bool owned = ownsLast || a < aHi;
    // (what the row's update needs besides the product: requested with the row)
    double rOld = rOldPre, tOld = tOldPre;
    double acc0 = 0.0, acc1 = 0.0;
    int c = lane;
    if (k != wv && lane == 0 && !init) {
      rOld = ts.rT[e];
      tOld = tin[e];
    }
    if (staged) {  // (the wave's own copy: LDS operations of a wave complete in order, and two workgroup barriers lie between)
      const double* srow = stage + static_cast<size_t>(k) * ts.NT;
      for (; c + 64 < ts.NT; c += 128) {
        acc0 += srow[c] * qT[c];
        acc1 += srow[c + 64] * qT[c + 64];
      }
      if (c < ts.NT) acc0 += srow[c] * qT[c];
    } else {
      for (; c + 64 < ts.NT; c += 128) {
        acc0 += row[c] * qT[c];
        acc1 += row[c + 64] * qT[c + 64];
      }
      if (c < ts.NT) acc0 += row[c] * qT[c];
    }
    const double d = ts.weight * waveSum(acc0 + acc1);
    if (lane == 0) {
      const double rn = init ? qT[e] : rOld - alpha * qT[e];
      const double tv = on ? (init ? d : tOld - alpha * d) : 0.0;
      if (owned) {
        ts.rT[e] = rn;
        tout[e] = tv;
      }
      tn[k] = tv;
      red[k] = owned ? tv * rn : 0.0;
    }
  }
  __syncthreads();
  if constexpr (FUSED) TAIL_STAMP(6);
  const int fLo = aLo * ts.step, fHi = ownsLast ? F : min(F, aHi * ts.step);
  for (int f = fLo + tid; f < fHi; f += nThreads) {
    const int a0 = f / ts.step, k0 = a0 - aLo;
    const double tau = static_cast<double>(f - a0 * ts.step) * inv;
    ts.tl[static_cast<size_t>(f) * ts.S + s] = (1.0 - tau) * tn[k0] + tau * tn[min(k0 + 1, nA - 1)];
  }
  if (tid == 0) {
    double d = 0.0;
    for (int k = 0; k < nA; ++k) d += red[k];
    storeMaybePublished(mid.levelShare(ts.dotPart + wg), d, mid.closes());
  }
  if constexpr (FUSED) TAIL_STAMP(7);
  return true;
}

// alpha = rz / sum(p.q) (published by k_matvec_finish); dx += alpha p; r -= alpha q; z = Minv_f r;
// partial r.z and r.r.  One workgroup per frame with 256 threads per 64-row chunk (blockDim = 256 * ceil(B/64),
// B <= 256): thread = (row, j-segment); the 4 segments of a row split the block mat-vec and are combined in LDS.
// 256 < B <= 512: 128 threads per chunk (two segments per row), same layout otherwise.
// init != 0: dx = 0, r = -g (already masked), z = Minv r.
// Body of k_cg_update.  FUSED = false: the kernel of that name.  FUSED = true: the second half of k_pcg_tail -- the caller's
// `mid.first(pv, qv)` runs the finish half of the frame first (direction / product element handed over in registers; false =
// converged already), then the loads that depend on nothing this launch computes are requested (the thread's share of M_f^-1
// resp. of A_c^-1, r, dx) and `mid.second(alpha)` -- the grid barrier and alpha = r^T z / sum p.q -- runs while they are in
// flight (held across the finish half as well they cost 32 spilled registers at the 80 a 768-thread workgroup pair allows).
template <bool FUSED, typename Mid>
__device__ __forceinline__ void cgUpdateBody(const Layout& L, int init, const double* __restrict__ g,
                                             const float* __restrict__ minv, const double* __restrict__ p,
                                             const double* __restrict__ q, double* __restrict__ scal,
                                             unsigned int* __restrict__ counter, double* __restrict__ dx,
                                             double* __restrict__ r, double* __restrict__ z,
                                             double* __restrict__ fdotRZ, double* __restrict__ fdotRR,
                                             double tol2, double* __restrict__ rc,
                                             const unsigned char* __restrict__ modeActive,
                                             double* __restrict__ hostMirror, const CoarseStep& cs, const DenseStep& ds,
                                             const double* __restrict__ pqReduced, double* __restrict__ sm, Mid& mid,
                                             int f0, int nF, double* __restrict__ partOut, const TlStep* __restrict__ tsp,
                                             const TlStep* __restrict__ tpp) {
  // [f0, f0 + nF): the frames this launch updates -- all of them, or (owner-sharded multi-GPU iteration) the calling rank's own
  // chunk; workgroups beyond nF are the dense coarse level's, two frames of the window each.  partOut != nullptr: the last
  // workgroup leaves THIS RANK's shares {r^T z, r^T r} there instead of finishing the PCG scalars (k_pcg_scalars_dist does).
  const double sDone = (init || FUSED) ? 0.0 : scal[S_DONE];  // converged earlier: the iterations enqueued ahead are no-ops (tested below)
  const int B = L.B;
  const int nThreads = blockDim.x;
  double* rf = sm;                 // B
  double* part = rf + B;           // partial row sums: nThreads (B > 256) or 16 segments x 4 ceil(B / 4) rows
  double* red = part + cgUpdatePartDoubles(B, nThreads);   // 2 * 16 wave partials + 10
  double* ypart = red + 48;        // 16 waves x kCB partial sums of the fused y update + kCB squares
  const bool fusedY = !init && cs.Wb != nullptr;
  const bool fusedDense = !init && ds.Ainv != nullptr;  // (the grid then has F extra workgroups)
  const int nWaves = nThreads >> 6;
  // closes: the last workgroup to leave sums the shares of r^T z and finishes the PCG scalars (below).  false (k_pcg_tail's shares
  // mode, chosen per launch): the shares are stored plainly -- nobody in the launch reads them -- into ONE array the caller laid out
  // (fdotRZ / fdotRR, ds.dotPart, ds.dotPart2 and mid.levelShare point into it), no ticket is drawn, and the next product's prologue
  // (k_matvec_pairs_fast<..., SHARES>) or k_pcg_close sums them: the launch ends when its slowest workgroup has stored its share.
  const bool closes = mid.closes();
  // Logical workgroup index: [0, nF) the frames, then the levels' workgroups.  A launch of its own (not the fused tail, whose
  // workgroups are all resident) dispatches the LEVELS' workgroups first: theirs is the longest dependent chain of the launch, and
  // behind a thousand frame workgroups -- four rounds of the device at configs[4] -- it started when everything else was done.
  const int nExtraWg = static_cast<int>(gridDim.x) - nF;
  const int bid = FUSED ? static_cast<int>(blockIdx.x)
                        : (static_cast<int>(blockIdx.x) < nExtraWg ? nF + static_cast<int>(blockIdx.x) : static_cast<int>(blockIdx.x) - nExtraWg);
  const bool denseWg = bid >= nF;
  const int f = denseWg ? L.F + (bid - nF) : f0 + bid;
  // (third level: its S workgroups follow the dense level's)
  const int nDenseWg = (fusedDense && ds.rowSplit > 0) ? (nF + kDenseFramesPerGroup - 1) / kDenseFramesPerGroup : 0;
  // (... and the kCB of the temporal pose level, coarse_level 3, follow those: same rows routine, its own descriptor)
  const bool tlOn = !init && tsp != nullptr, tpOn = !init && tpp != nullptr;
  const bool tlWg = (tlOn || tpOn) && bid >= nF + nDenseWg;
  const int tid = threadIdx.x;
  const size_t base = static_cast<size_t>(f) * B;
  // (pqReduced: the fused exchange of the pair-sharded mode left the all-reduced p.q there; S_RZ is rewritten only by the
  // last workgroup to arrive, i.e. after every workgroup has read it here)
  double alpha = (init || FUSED) ? 0.0 : (pqReduced != nullptr ? scal[S_RZ] / *pqReduced : scal[S_ALPHA]);
  double pvCarry = 0.0, qvCarry = 0.0;
  if constexpr (FUSED) {
    // the finish half of this frame (dense-level workgroups: only the convergence flag); its registers are dead before the
    // update half requests its operands below
    if (!mid.first(pvCarry, qvCarry)) return;
  }
#ifndef CVD_DENSE_LOADS
#define CVD_DENSE_LOADS 4
#endif
  // (7 in the fused kernel -- two round trips per row instead of four -- spills at its 80-register budget: 12.9 -> 16.9 us)
  constexpr int kDenseLoads = CVD_DENSE_LOADS;
  const size_t nC = static_cast<size_t>(L.F) * kCB;   // coarse unknowns
  const int n2 = static_cast<int>(nC / 2);
  // ---- dense coarse level, rows [r0, r0 + nR) of frame g: d = (A_c^-1 Z^T q) (nThreads / nR threads per row; every thread's
  // <= kDenseLoads 16-byte loads of the (f64) inverse are issued at once, qc comes from LDS, the row sums are folded in LDS),
  // c <- c - alpha d, rc <- rc - alpha qc, and the rows' share of the coarse part of r^T z into *dotSlot.  All threads of the
  // workgroup call it.  w: the first batch of the first row walk when preloaded.
  auto denseRows = [&](int g, int r0, int nR, const double* qcs, double* psum, bool on0, double2 (&w)[kDenseLoads], bool preloaded,
                       double* dotSlot) {
    const int per = nThreads / nR, m = tid / per, part = tid - m * per;
    const bool active = m < nR;
    const double2* row = reinterpret_cast<const double2*>(ds.Ainv + (static_cast<size_t>(g) * kCB + r0 + (active ? m : 0)) * nC);
    const int e = g * kCB + r0 + (tid < nR ? tid : 0);
    const double qcv = qcs[e], rcOld = ds.rc[e], cOld = ds.c[e];
    const bool on = on0 && ds.modeActive[e];
    double acc0 = 0.0, acc1 = 0.0;
    // the row in BATCHES of kDenseLoads loads per thread, every batch's loads issued together
    for (int base = 0; base < n2; base += kDenseLoads * per) {
      if (!preloaded || base > 0) {
#pragma unroll
        for (int u = 0; u < kDenseLoads; ++u) {
          const int j = base + part + u * per;
          w[u] = row[j < n2 ? j : 0];
          if (j >= n2 || !active) w[u] = make_double2(0.0, 0.0);
        }
      }
#pragma unroll
      for (int u = 0; u < kDenseLoads; ++u) {
        const int j = base + part + u * per;
        const double2 qq = *reinterpret_cast<const double2*>(qcs + 2 * (j < n2 ? j : 0));
        acc0 += w[u].x * qq.x;
        acc1 += w[u].y * qq.y;
      }
    }
    psum[tid] = active ? acc0 + acc1 : 0.0;
    __syncthreads();
    if (tid < nR * 8) {  // 8 lanes per row fold its `per` partials, then three shuffle steps
      const int r = tid >> 3, l = tid & 7;
      double t = 0.0;
      for (int k = l; k < per; k += 8) t += psum[r * per + k];
      t += __shfl_xor(t, 1, 64);
      t += __shfl_xor(t, 2, 64);
      t += __shfl_xor(t, 4, 64);
      if (l == 0) psum[nThreads + r] = t;
    }
    __syncthreads();
    if (tid < 8) {  // (8 lanes shuffle together; rows beyond nR contribute nothing)
      double t = 0.0;
      if (tid < nR) {
        const double d = psum[nThreads + tid];
        const double rcn = rcOld - alpha * qcv;
        const double cn = on ? cOld - alpha * d : 0.0;
        ds.rc[e] = rcn;
        ds.c[e] = cn;
        t = cn * rcn;
      }
      t += __shfl_xor(t, 1, 64);
      t += __shfl_xor(t, 2, 64);
      t += __shfl_xor(t, 4, 64);
      if (tid == 0) storeMaybePublished(dotSlot, t, closes);
    }
    __syncthreads();  // (psum is reused)
  };
  if (f >= L.F) {
    if (tlWg) {  // third level's workgroup (one coarse hat) or the temporal pose level's (one mode)
      const int k = bid - nF - nDenseWg, nTl = tlOn ? tsp->S * tsp->parts : 0;
      if (!tlLevelRows<FUSED>(k < nTl ? tsp : tpp, k < nTl ? k : k - nTl, L.F, alpha, 0, sDone, scal, sm, mid)) return;
    } else {
    // ---- dense-level workgroup: rows [0, rowSplit) of kDenseFramesPerGroup frames, one frame after the other (F + F / 2
    // workgroups of 768 threads still fit the device in ONE round, two per CU; F + F do not)
    const int nR = ds.rowSplit;
    double* qcs = sm;                       // nC doubles (the frame workgroups' layout is not used here)
    double* psum = sm + nC;                 // nThreads partial sums + 8 row sums
    const int g0 = f0 + (f - L.F) * kDenseFramesPerGroup;
    double2 w[kDenseLoads];
    {
      const int per = nThreads / nR, m = tid / per, part = tid - m * per;
      const double2* row = reinterpret_cast<const double2*>(ds.Ainv + (static_cast<size_t>(g0) * kCB + (m < nR ? m : 0)) * nC);
#pragma unroll
      for (int u = 0; u < kDenseLoads; ++u) {
        const int j = part + u * per;
        w[u] = row[j < n2 ? j : 0];
        if (j >= n2 || m >= nR) w[u] = make_double2(0.0, 0.0);
      }
    }
    if constexpr (FUSED) {  // (the first batch of the inverse's row is in flight across the grid barrier)
      if (!mid.second(alpha)) return;
      for (int i = tid; i < static_cast<int>(nC); i += nThreads) qcs[i] = readPartial(ds.qc + i);  // (published by the finish halves)
    } else {
      for (int i = tid; i < static_cast<int>(nC); i += nThreads) qcs[i] = ds.qc[i];
    }
    const bool on0 = *ds.fail == 0;
    __syncthreads();
    if (sDone != 0.0) return;  // uniform; nothing written yet
    for (int rep = 0; rep < kDenseFramesPerGroup; ++rep) {
      const int g = g0 + rep;
      if (g >= f0 + nF) break;
      denseRows(g, 0, nR, qcs, psum, on0, w, rep == 0, ds.dotPart + g);
    }
    }  // dense-level workgroup
  } else {
  // B <= 256: the thread's share of the f32 block M_f^-1 (see the mat-vec below) is requested FIRST -- it depends on nothing
  // this launch computes, so its way from L2 / MALL overlaps the vector loads, the update and the barrier
  struct __attribute__((packed, aligned(4))) F4u { float x, y, z, w; };
  constexpr int kMinvLoads = 8;   // rows j = sg, sg + nSeg, ...: the first 8 of up to ceil(256 / 16) = 16 (16 spill at the
                                  // 128 registers a 1024-thread workgroup leaves a wave; the rest follows after the barrier)
  const bool wide = B > 256;  // (two segments per row: blockDim = 128 * ceil(B / 64) <= 1024)
  const float* Mf = minv + static_cast<size_t>(f) * B * B;
  const int nQ = (B + 3) >> 2;
  const int nSeg = min(16, nThreads / nQ);
  const int q4 = tid % nQ, sg = tid / nQ;
  F4u mreg[kMinvLoads];
  if (!wide && sg < nSeg) {
    const float* col = Mf + 4 * q4;
#pragma unroll
    for (int u = 0; u < kMinvLoads; ++u) {
      const int j = sg + u * nSeg;
      if (u * nSeg < B) mreg[u] = *reinterpret_cast<const F4u*>(col + static_cast<size_t>(min(j, B - 1)) * B);  // (uniform test)
    }
  }
  {
    // one element per thread (blockDim = 256 * ceil(B / 64) >= B).  The vector loads are issued together with the
    // scalars' and the convergence flag is tested once they are back: one dependent global round trip instead of two
    const int j = tid;
    double pv = 0.0, qv = 0.0, rv = 0.0, dv = 0.0;
    if (j < B) {
      if (init) {
        rv = -g[base + j];
      } else {
        if constexpr (!FUSED) {
          pv = p[base + j];
          qv = q[base + j];
        }
        rv = r[base + j];
        dv = dx[base + j];
      }
    }
    if constexpr (!FUSED) asm volatile("" : "+v"(pv), "+v"(qv), "+v"(rv), "+v"(dv));  // (keeps the loads above the early exit)
    if constexpr (FUSED) {
      pv = pvCarry;
      qv = qvCarry;
      if (!mid.second(alpha)) return;  // grid barrier + alpha (the loads above are in flight meanwhile)
    } else {
      if (sDone != 0.0) return;  // uniform; nothing written yet
    }
    if (j < B) {
      if (!init) {
        dv += alpha * pv;
        rv -= alpha * qv;
      }
      dx[base + j] = dv;
      r[base + j] = rv;
      rf[j] = rv;
    }
  }
  __syncthreads();
  if (rc != nullptr) coarseRestrict(L, rf, f, tid, modeActive, rc);  // Z_f^T r_f (first residual: k_coarse_apply_w)
  if (fusedY) {
    // row f of W (Z^T q): the 8-vectors W_block (Z^T q)_column were left in row order by coarseColumnProducts (in the
    // kernel that completed q), so the row is a contiguous run: a wave sums eight entries per load, lane = (entry, mode)
    const int wv = tid >> 6, lane = tid & 63, nWv = nThreads >> 6;
    const size_t e0 = static_cast<size_t>(cs.wtPtr[f]) * kCB, e1 = static_cast<size_t>(cs.wtPtr[f + 1]) * kCB;
    double a0 = 0.0, a1 = 0.0;
    size_t e = e0 + static_cast<size_t>(wv) * 64 + lane;
    const size_t stride = static_cast<size_t>(nWv) * 64;
    for (; e + stride < e1; e += 2 * stride) {
      a0 += cs.wq[e];
      a1 += cs.wq[e + stride];
    }
    if (e < e1) a0 += cs.wq[e];
    double ya = a0 + a1;
    ya += __shfl_xor(ya, 8, 64);
    ya += __shfl_xor(ya, 16, 64);
    ya += __shfl_xor(ya, 32, 64);
    if (lane < kCB) ypart[wv * kCB + lane] = ya;
  }
  // preconditioner blocks are stored in f32 (an SPD approximation is all PCG needs; halves the traffic),
  // applied with f64 accumulation.  Symmetric block: column access, coalesced over the row index.
  const int chunk = wide ? tid >> 7 : tid >> 8, row = tid & 63, seg = wide ? (tid >> 6) & 1 : (tid >> 6) & 3;
  const int i = chunk * 64 + row;
  double acc = 0.0;
  if (wide) {
    if (i < B) {
      double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
      const float* col = Mf + i;
      int j = seg;
      for (; j + 6 < B; j += 8) {
        a0 += static_cast<double>(col[static_cast<size_t>(j) * B]) * rf[j];
        a1 += static_cast<double>(col[static_cast<size_t>(j + 2) * B]) * rf[j + 2];
        a2 += static_cast<double>(col[static_cast<size_t>(j + 4) * B]) * rf[j + 4];
        a3 += static_cast<double>(col[static_cast<size_t>(j + 6) * B]) * rf[j + 6];
      }
      for (; j < B; j += 2) a0 += static_cast<double>(col[static_cast<size_t>(j) * B]) * rf[j];
      acc = (a0 + a1) + (a2 + a3);
    }
  } else {
    // Thread = (QUAD of rows 4 q .. 4 q + 3, j-segment): one 16-byte load fetches the quad's entries of block row j (the
    // block is symmetric: row j = column j; consecutive lanes = consecutive quads, so a wave reads contiguous bytes of a
    // row), up to 16 independent loads per thread all in flight.  4 B per lane and load (thread = one row) made this half of
    // the launch latency-bound at 2.4 TB/s of L2/MALL-resident data.  The rows are only 4-byte aligned (B is odd in every
    // level of the default schedule): global dwordx4 loads need no more.  A quad that reaches past the end of a row reads
    // the head of the next one (past the last frame: the allocation's slack) into lanes whose sums are never used.
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    if (sg < nSeg) {
#pragma unroll
      for (int u = 0; u < kMinvLoads; ++u) {
        const int j = sg + u * nSeg;
        if (u * nSeg < B) {
          const double rj = j < B ? rf[j] : 0.0;
          a0 += static_cast<double>(mreg[u].x) * rj;
          a1 += static_cast<double>(mreg[u].y) * rj;
          a2 += static_cast<double>(mreg[u].z) * rj;
          a3 += static_cast<double>(mreg[u].w) * rj;
        }
      }
      if (kMinvLoads * nSeg < B) {  // (uniform: B > 128 at 16 segments) second batch, again all loads first
        const float* col = Mf + 4 * q4;
#pragma unroll
        for (int u = 0; u < kMinvLoads; ++u) {
          const int j = sg + (kMinvLoads + u) * nSeg;
          if ((kMinvLoads + u) * nSeg < B) mreg[u] = *reinterpret_cast<const F4u*>(col + static_cast<size_t>(min(j, B - 1)) * B);
        }
#pragma unroll
        for (int u = 0; u < kMinvLoads; ++u) {
          const int j = sg + (kMinvLoads + u) * nSeg;
          if ((kMinvLoads + u) * nSeg < B) {
            const double rj = j < B ? rf[j] : 0.0;
            a0 += static_cast<double>(mreg[u].x) * rj;
            a1 += static_cast<double>(mreg[u].y) * rj;
            a2 += static_cast<double>(mreg[u].z) * rj;
            a3 += static_cast<double>(mreg[u].w) * rj;
          }
        }
      }
      double* dst = part + static_cast<size_t>(sg) * (4 * nQ) + 4 * q4;
      dst[0] = a0; dst[1] = a1; dst[2] = a2; dst[3] = a3;
    }
    __syncthreads();
    if (tid < B) {
      double zv = 0.0;
      for (int k2 = 0; k2 < nSeg; ++k2) zv += part[static_cast<size_t>(k2) * (4 * nQ) + tid];
      acc = zv;
    }
  }
  if (wide) part[tid] = acc;
  __syncthreads();
  double rz = 0.0, rr = 0.0;
  if (wide) {
    if (seg == 0 && i < B) {
      const int b0 = chunk * 128 + row;
      const double zv = part[b0] + part[b0 + 64];
      z[base + i] = zv;
      rz = rf[i] * zv;
      rr = rf[i] * rf[i];
    }
  } else if (tid < B) {
    z[base + tid] = acc;
    rz = rf[tid] * acc;
    rr = rf[tid] * rf[tid];
  }
  rz = waveSum(rz);
  rr = waveSum(rr);
  if ((tid & 63) == 0) { red[tid >> 6] = rz; red[16 + (tid >> 6)] = rr; }
  __syncthreads();
  if (tid == 0) {
    double a = 0.0, b = 0.0;
    for (int w = 0; w < nWaves; ++w) { a += red[w]; b += red[16 + w]; }
    storeMaybePublished(fdotRZ + f, a, closes);
    storeMaybePublished(fdotRR + f, b, closes);
  }
  if (fusedY) {
    // y_f <- y_f - alpha (W Z^T q)_f (ypart is complete: two barriers since it was written); |y_f|^2 is this
    // frame's share of the coarse part of r^T z = |W Z^T r|^2
    if (tid < kCB) {
      double sy = 0.0;
      for (int w = 0; w < nWaves; ++w) sy += ypart[w * kCB + tid];
      const double yn = cs.y[f * kCB + tid] - alpha * sy;
      cs.y[f * kCB + tid] = yn;
      ypart[16 * kCB + tid] = yn * yn;
    }
    __syncthreads();
    if (tid == 0) {
      double t = 0.0;
#pragma unroll
      for (int k = 0; k < kCB; ++k) t += ypart[16 * kCB + k];
      publishPartial(cs.fdotY + f, t);
    }
  }
  if (fusedDense && ds.rowSplit < kCB) {
    // ---- this frame's rows [rowSplit, 8) of the dense coarse level (DenseStep::rowSplit), in an LDS region of their own
    double* qcs = sm + ds.ldsPsum;
    double* psum = qcs + nC;
    if constexpr (FUSED) {
      for (int i = tid; i < static_cast<int>(nC); i += nThreads) qcs[i] = readPartial(ds.qc + i);  // (published by the finish halves)
    } else {
      for (int i = tid; i < static_cast<int>(nC); i += nThreads) qcs[i] = ds.qc[i];
    }
    const bool on0 = *ds.fail == 0;
    __syncthreads();
    double2 w[kDenseLoads];
    denseRows(f, ds.rowSplit, kCB - ds.rowSplit, qcs, psum, on0, w, false, ds.dotPart2 + f);
  }
  }  // frame workgroups
  if (!closes) return;
  // last workgroup: rz_new = sum, beta = rz_new / rz_old (device-side scalars, no host round trip)
  if (lastBlockArrivesLite(counter, gridDim.x, reinterpret_cast<int*>(red + 40))) {
    double a = 0.0, b = 0.0, cY = 0.0;
    for (int k = f0 + tid; k < f0 + nF; k += nThreads) {
      a += readPartial(fdotRZ + k);
      b += readPartial(fdotRR + k);
      if (fusedY) cY += readPartial(cs.fdotY + k);
      if (fusedDense && ds.rowSplit > 0) cY += readPartial(ds.dotPart + k);
      if (fusedDense && ds.rowSplit < kCB) cY += readPartial(ds.dotPart2 + k);
    }
    double cT = 0.0;  // third level's part of r^T z (kept apart: a broken-down sparse factor switches ITS level off below, not this one)
    if (tlOn)
      for (int k = tid; k < tsp->S * tsp->parts; k += nThreads) cT += readPartial(tsp->dotPart + k);
    if (tpOn)
      for (int k = tid; k < tpp->S * tpp->parts; k += nThreads) cT += readPartial(tpp->dotPart + k);
    a = waveSum(a);
    b = waveSum(b);
    cY = waveSum(cY);
    cT = waveSum(cT);
    __syncthreads();
    if ((tid & 63) == 0) { red[tid >> 6] = a; red[16 + (tid >> 6)] = b; ypart[tid >> 6] = cY; ypart[16 + (tid >> 6)] = cT; }
    __syncthreads();
    if (tid == 0) {
      double rzs = 0.0, rrs = 0.0, ys = 0.0, tls = 0.0;
      for (int w = 0; w < nWaves; ++w) { rzs += red[w]; rrs += red[16 + w]; ys += ypart[w]; tls += ypart[16 + w]; }
      // (owner-sharded iteration: every rank walks ALL rows of the third level -- they are few -- so its part of r^T z counts once,
      // on the first rank)
      rzs += (partOut == nullptr || f0 == 0) ? tls : 0.0;
      if (partOut != nullptr) {  // this rank's shares, summed over the ranks by k_pcg_scalars_dist
        partOut[0] = rzs + ((fusedY && *cs.fail != 0) ? 0.0 : ys);
        partOut[1] = rrs;
      } else if (fusedY) {  // two-level r^T z; a broken-down coarse factorisation switches the level off (consumers use c = 0)
        pcgFinishScalars(scal, 0, rzs + (*cs.fail == 0 ? ys : 0.0), rrs, tol2, hostMirror);
      } else if (fusedDense) {  // (a failed inverse left c = 0 and zero shares)
        pcgFinishScalars(scal, 0, rzs + ys, rrs, tol2, hostMirror);
      } else if (rc != nullptr || (init && (tsp != nullptr || tpp != nullptr))) {  // first residual: the coarse levels' kernels (k_coarse_apply_w /
                                                               // k_coarse_dense_apply / k_tl_rows_init) add their parts of r^T z and finish the scalars
        scal[S_RZPART] = rzs;
        scal[S_RR] = rrs;
      } else {
        pcgFinishScalars(scal, init, rzs, rrs, tol2, hostMirror);
      }
    }
  }
}

inline __global__ __launch_bounds__(1024) void k_cg_update(Layout L, int init, const double* __restrict__ g,
                                                    const float* __restrict__ minv, const double* __restrict__ p,
                                                    const double* __restrict__ q, double* __restrict__ scal,
                                                    unsigned int* __restrict__ counter, double* __restrict__ dx,
                                                    double* __restrict__ r, double* __restrict__ z,
                                                    double* __restrict__ fdotRZ, double* __restrict__ fdotRR,
                                                    double tol2, double* __restrict__ rc,
                                                    const unsigned char* __restrict__ modeActive,
                                                    double* __restrict__ hostMirror, CoarseStep cs, DenseStep ds,
                                                    const double* __restrict__ pqReduced, int f0, int nF,
                                                    double* __restrict__ partOut, const TlStep* __restrict__ tsp,
                                                    const TlStep* __restrict__ tpp) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  NoMid mid;
  cgUpdateBody<false>(L, init, g, minv, p, q, scal, counter, dx, r, z, fdotRZ, fdotRR, tol2, rc, modeActive, hostMirror, cs, ds,
                      pqReduced, sm, mid, f0, nF, partOut, tsp, tpp);
}

// Owner-sharded PCG iteration (multi-GPU): every rank updated x, r, z of ITS frames and left {r^T z, r^T r} of those frames in
// parts[2 rank]; after the all-gather of the shares one workgroup finishes the iteration's scalars (beta, convergence flag,
// iteration count, host mirror) on every rank -- identically: the ranks sum the same numbers in the same order.
inline __global__ void k_pcg_scalars_dist(const double* __restrict__ parts, int world, double* __restrict__ scal, double tol2,
                                          double* __restrict__ hostMirror) {
  if (threadIdx.x != 0 || scal[S_DONE] != 0.0) return;  // (iterations enqueued past convergence are no-ops)
  double rz = 0.0, rr = 0.0;
  for (int r = 0; r < world; ++r) {
    rz += parts[2 * r];
    rr += parts[2 * r + 1];
  }
  pcgFinishScalars(scal, 0, rz, rr, tol2, hostMirror);
}

// ---- one kernel for the tail of a PCG iteration ------------------------------------------------------
// k_matvec_finish and k_cg_update were two launches, two prologues and two last-workgroup hand-offs per iteration for
// F (+ F / 2 dense-level) workgroups that are all co-resident, each a chain of dependent round trips.  k_pcg_tail runs both
// halves in ONE launch: every workgroup first requests what its update half needs and nothing of this launch produces (its
// share of the f32 block M_f^-1 resp. of the dense coarse inverse, r, dx), the frame workgroups then run the finish half
// (partial rows -> q_f, p.q share, Z^T q published), ONE grid barrier, every workgroup sums the F shares of p.q itself
// (alpha), and the update half follows with its operands already in registers.  The last workgroup to leave publishes beta /
// the convergence flag exactly as k_cg_update does.  Single GPU, B <= 256, dense coarse level or none (the sparse level's
// column products cross workgroups through plain stores; a sharded run has a collective between the halves).
//
// Grid barrier (tailArrive / tailWait): self-resetting (the last arriver zeroes the count and bumps the generation), one use per launch.  Payload crossing it is published with agent-scope stores and read with
// agent-scope loads (publishPartial / readPartial, cdna_hip_programming.md G16 R1), every wave drains its stores first.
// The spin is bounded: a launch whose workgroups are not all resident abandons (the host checks the occupancy and serialises
// gated kernels of different handles, so this is a safety net) and the host's progress check reports the stalled PCG.
// The barrier carries the one reduction the halves need: the FIRST WAVE of the last workgroup to arrive sums the nParts published
// partials (p.q shares of the frames) and releases the others with records that hold the sum.
// Split in two: tailArrive right after the finish half (only the payload that crosses the barrier is drained in front of it: the
// direction and the product, which nobody in this launch reads from memory, are stored behind it; the first wave waits for its
// ticket there, and the last arriver's release does not wait on its own update half's operand requests), tailWait after the update
// half's operand requests.  Waiting costs MEMORY TRAFFIC: every poll is an
// L2-bypassing load, and hundreds of workgroups polling one address saturate the memory channel that holds it -- the finish
// halves still running slowed down 2x (measured with stamps, tools/tail_profile.py: 12.3 -> 7.6 us median when the poll
// interval went from 4 to 32 sleep units).  The release word is therefore replicated over kTailBarCopies pages (different
// channels), each workgroup polls the copy blockIdx % kTailBarCopies at a long interval.
// bar: [0] arrivals, [1] abandon flag, generation copies at bar[kTailBarStride * (1 + k)].
// scratch: 24 doubles of LDS ([16] role, [17] generation, [18] the sum; [0..15] unused since the first wave sums alone).
constexpr int kTailBarCopies = 16;
constexpr int kTailBarStride = 1024;  // unsigned ints: 4 KB
// (thread 0 reads its generation copy with tailGeneration at the START of the kernel: that round trip does not sit between the
// finish half and the arrival)
__device__ __forceinline__ unsigned int tailGeneration(const unsigned int* bar) {
  if (threadIdx.x != 0) return 0u;
  return *reinterpret_cast<const volatile unsigned int*>(bar + kTailBarStride * (1 + (blockIdx.x & (kTailBarCopies - 1))));
}
// tailArrive: the FIRST WAVE alone takes the ticket and waits for it; the workgroup that drew the last one releases the others
// right there -- its first wave sums the nParts published partials (lane l: partials l, l + 64, ... in that order, then waveSum: a
// fixed order), re-arms the count and writes the release records -- without a workgroup barrier, and without waiting on the update
// half's operand requests: those are issued meanwhile by the other waves, which in every workgroup return from here at once (the
// first wave of the releasing workgroup issues its own behind the release).  Role (1: wait,
// 2: released the others), generation and the sum are left in the scratch words for tailWait.
__device__ __forceinline__ void tailArrive(unsigned int* bar, unsigned int nGroups, unsigned int gen, const double* __restrict__ parts,
                                           int nParts, double* __restrict__ scratch) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // every wave: its published payload has landed
  __syncthreads();
  if (threadIdx.x >= 64) return;
  unsigned int ticket = 0u;
  if (threadIdx.x == 0) ticket = __hip_atomic_fetch_add(bar, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  ticket = __builtin_amdgcn_readfirstlane(ticket);
  gen = __builtin_amdgcn_readfirstlane(gen);  // (thread 0 read it at the start of the kernel)
  const bool last = ticket == nGroups - 1;
  if (last) {
    double a = 0.0;
    for (int k0 = threadIdx.x; k0 < nParts + static_cast<int>(threadIdx.x); k0 += 8 * 64) {  // (eight loads in flight per lane: 512 partials a trip)
      double w[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) w[u] = k0 + u * 64 < nParts ? readPartial(parts + k0 + u * 64) : 0.0;
#pragma unroll
      for (int u = 0; u < 8; ++u) a += w[u];
    }
    const double v = waveSum(a);
    if (threadIdx.x == 0) __hip_atomic_store(bar, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (threadIdx.x < kTailBarCopies) {
      cvd_u32x4 rec;
      rec.x = gen + 1u;
      rec.y = static_cast<unsigned int>(__double2loint(v));
      rec.z = static_cast<unsigned int>(__double2hiint(v));
      rec.w = gen + 1u;
      *reinterpret_cast<volatile cvd_u32x4*>(bar + kTailBarStride * (1 + threadIdx.x)) = rec;
    }
    if (threadIdx.x == 0) scratch[18] = v;
  }
  if (threadIdx.x == 0) {
    *reinterpret_cast<int*>(scratch + 16) = last ? 2 : 1;
    *reinterpret_cast<unsigned int*>(scratch + 17) = gen;
  }
}
// The release word of a copy is a 16-byte RECORD {generation, sum (2 words), generation}, written with ONE 16-byte store and read
// with one 16-byte load: the sum travels with the flag, so the last arriver neither publishes it separately nor drains that store
// before releasing (2.5 us of the 7 between the last arrival and the release).  A reader accepts a record whose two generation
// words agree (a 16-byte access of one lane is one transaction; the second word guards against a torn one anyway).
__device__ __forceinline__ bool tailWait(unsigned int* bar, double* __restrict__ scratch, double& sum) {
  int* role = reinterpret_cast<int*>(scratch + 16);
  __syncthreads();  // (tailArrive's first wave left role, generation and -- the releasing workgroup -- the sum)
  const unsigned int gen = *reinterpret_cast<unsigned int*>(scratch + 17);
  if (*role == 2) {
    sum = scratch[18];
    return true;
  }
  if (threadIdx.x == 0) {
    const volatile cvd_u32x4* mine = reinterpret_cast<const volatile cvd_u32x4*>(bar + kTailBarStride * (1 + (blockIdx.x & (kTailBarCopies - 1))));
    int ok = 1;
    unsigned int spins = 0;
    cvd_u32x4 rec;
    for (;;) {
      rec = *mine;
      if (rec.x == gen + 1u && rec.w == gen + 1u) break;
      __builtin_amdgcn_s_sleep(16);
      ++spins;
      if ((spins & 63u) == 0 && __hip_atomic_load(bar + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u) { ok = 0; break; }
      if (spins > (1u << 18)) {  // ~1 s
        __hip_atomic_store(bar + 1, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        //  ... and poison the arrival count: no later arriver of this solve can draw the LAST ticket any more, so an
        // abandoned barrier is never released behind the workgroups that left it (x / r stay consistent; the host's progress
        // check reports the stall and falls back to the two-launch tail)
        __hip_atomic_fetch_add(bar, 0x40000000u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        ok = 0;
        break;
      }
    }
    scratch[18] = ok ? __hiloint2double(static_cast<int>(rec.z), static_cast<int>(rec.y)) : 0.0;
    *role = ok;
  }
  __syncthreads();
  sum = scratch[18];
  return *role != 0;
}

// what the update half needs beside the finish half's arguments
struct TailUpdate {
  const float* minv;
  double* dx;
  double* r;
  double* z;
  double* fdotRZ;
  double* fdotRR;
  double tol2;
  const unsigned char* modeActive;
  double* hostMirror;
  unsigned int* counter;   // last-workgroup ticket of the update half
  unsigned int* gridBar;   // kTailBarStride * (1 + kTailBarCopies) words, zeroed by the host before a PCG solve
  double* pqSlot;          // where the barrier's last arriver publishes sum p.q (a line of its own)
  int ldsFinish;           // offset (doubles) of the finish half's LDS region
  int ldsScratch;          // offset of 24 doubles for the barrier flag and the p.q sum (beyond both kinds of workgroups' regions)
  DenseStep ds;
  const TlStep* ts;        // third level (device copy of its descriptor), nullptr: off
  const TlStep* tp;        // temporal pose level (coarse_level 3), nullptr: off
  int diagInProduct;       // explicit cross blocks: H_ff p_f is one of the frame's partial rows (k_cross_matvec), not the finish half's work
  int stageRows;           // 1: the temporal levels' workgroups copy their rows of the inverse to LDS in front of the grid barrier
                           // (tlStagedLds doubles each; 0: the launch would not fit or not be co-resident with them -- rows from memory)
  // shares mode (cgUpdateBody: closes = false): the share array (SH_RZ behind the PCG scalars; fdotRZ / fdotRR / ds.dotPart /
  // ds.dotPart2 point into it, `counter` is not used), nullptr: the launch closes r^T z itself.  The temporal levels' workgroups --
  // blockIdx levelWg0 onwards, the depth-grid level's parts, then the temporal pose level's -- store at levelShare0 onwards.
  double* shares;
  int levelShare0, levelWg0;
};

template <int KD>
inline __global__ __launch_bounds__(1024) __attribute__((amdgpu_waves_per_eu(6))) void k_pcg_tail(Layout L, const double* __restrict__ x,
                                                    const double* __restrict__ mask,
                                                    const double* __restrict__ lam, const float* __restrict__ median,
                                                    const unsigned char* __restrict__ inRange,
                                                    const unsigned char* __restrict__ rangeFlags,
                                                    const int* __restrict__ fiOff, const int* __restrict__ fiList,
                                                    const double* __restrict__ qPart, const double* __restrict__ pOld,
                                                    double* __restrict__ pNew, double* __restrict__ scal, int useBeta,
                                                    double* __restrict__ q, double* __restrict__ fdot, int nRows, RegCache rc,
                                                    CoarseView V, double* __restrict__ qc, const double* __restrict__ Hdiag,
                                                    TailUpdate U) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  const int f = blockIdx.x;
  const CoarseColumns ccOff{nullptr, nullptr, nullptr, nullptr, nullptr};
  const CoarseStep csOff{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  TAIL_STAMP(0);
  const unsigned int barGen = tailGeneration(U.gridBar);
  // (r^T z of the previous iteration, for alpha: S_RZ is rewritten only by the last workgroup to take the update half's ticket, i.e.
  // after every workgroup has passed the grid barrier -- read here, not in a round trip of its own behind the release)
  const double rzOld = scal[S_RZ];
  auto first = [&](double& pv, double& qv) -> bool {
    if (f < L.F) {
      TailCarry carry{0.0, 0.0};
      if (!matvecFinishBody<KD, true>(L, x, mask, lam, median, inRange, rangeFlags, fiOff, fiList, qPart, U.z, pOld, pNew, scal,
                                      nullptr, useBeta, q, fdot, 0, nRows, rc, V, qc, ccOff, Hdiag, nullptr, 0, U.diagInProduct ? 0 : L.F,
                                      sm + U.ldsFinish, carry, U.ts, sm + L.B))  // (restriction products: the update half's partial-sum region)
        return false;
      pv = carry.pv;
      qv = carry.qv;
    } else if (scal[S_DONE] != 0.0) {
      return false;  // (dense-level workgroup of a launch enqueued past convergence)
    }
    TAIL_STAMP(1);
    tailArrive(U.gridBar, gridDim.x, barGen, fdot, L.F, sm + U.ldsScratch);
    TAIL_STAMP(10);
    // (nobody in this launch reads the direction and the product from memory: stored behind the arrival, not drained in front of it)
    if (f < L.F && static_cast<int>(threadIdx.x) < L.B) {
      pNew[static_cast<size_t>(f) * L.B + threadIdx.x] = pv;
      q[static_cast<size_t>(f) * L.B + threadIdx.x] = qv;
    }
    return true;
  };
  auto second = [&](double& alpha) -> bool {
    double pq;
    TAIL_STAMP(2);
    if (!tailWait(U.gridBar, sm + U.ldsScratch, pq)) {
      // (shares mode: the product that would close this iteration must not -- the mirror stalls and the host falls back, as it
      // does when the parent's closing never gets its last ticket)
      if (U.shares != nullptr && threadIdx.x == 0) publishPartial(scal + SH_ABANDON, 1.0);
      return false;
    }
    TAIL_STAMP(3);
    alpha = rzOld / pq;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
      scal[S_PQ] = pq;
      scal[S_ALPHA] = alpha;
    }
    return true;
  };
  struct Mid {
    decltype(first)& f1;
    decltype(second)& f2;
    double* scratch;
    __device__ bool first(double& pv, double& qv) { return f1(pv, qv); }
    __device__ bool second(double& alpha) { return f2(alpha); }
    // (the barrier's generation at the start of this launch: tailWait left it in the scratch words for every thread)
    __device__ unsigned int generation() { return *reinterpret_cast<unsigned int*>(scratch + 17); }
    bool stage;
    __device__ bool stageRows() { return stage; }
    double* shares;
    double* abandonWord;
    int levelShare0, levelWg0;
    __device__ bool closes() { return shares == nullptr; }
    __device__ double* levelShare(double* fromDescriptor) {
      return shares != nullptr ? shares + levelShare0 + (static_cast<int>(blockIdx.x) - levelWg0) : fromDescriptor;
    }
    __device__ void gaveUp() {  // (a level's node sums timed out: as an abandoned grid barrier)
      if (shares != nullptr && threadIdx.x == 0) publishPartial(abandonWord, 1.0);
    }
  } mid{first, second, sm + U.ldsScratch, U.stageRows != 0, U.shares, scal + SH_ABANDON, U.levelShare0, U.levelWg0};
  cgUpdateBody<true>(L, 0, nullptr, U.minv, nullptr, nullptr, scal, U.counter, U.dx, U.r, U.z, U.fdotRZ, U.fdotRR, U.tol2, nullptr,
                     U.modeActive, U.hostMirror, csOff, U.ds, nullptr, sm, mid, 0, L.F, nullptr, U.ts, U.tp);
  TAIL_STAMP(4);
}

// Behind the last enqueued tail of a shares-mode solve (one wave): nothing follows that would sum its shares.  Sums them in the
// product's order (pcgSharesSum), r^T r too, and finishes the scalars as the product of iteration `enqueued` would have -- unless
// the PCG is done (the product that found out has written everything; iterations behind it were no-ops), a grid barrier was
// abandoned (nobody closes: the host falls back) or the iteration is closed already (S_ITERS): idempotent in all three.
inline __global__ __launch_bounds__(64) void k_pcg_close(double* __restrict__ scal, int enqueued, double* __restrict__ hostMirror) {
  const int lane = threadIdx.x;
  double wz[8], wr[8];
#pragma unroll
  for (int u = 0; u < 8; ++u) {
    wz[u] = scal[SH_RZ + lane + u * 64];
    wr[u] = scal[SH_RR + lane + u * 64];
  }
  const double done0 = scal[S_DONE], abandon = scal[SH_ABANDON], old = scal[S_RZ], target = scal[S_TARGET];
  const int applied = static_cast<int>(scal[S_ITERS]);
  const double rz = pcgSharesSum(wz), rr = pcgSharesSum(wr);
  if (lane != 0 || abandon != 0.0) return;
  if (done0 == 0.0 && applied == enqueued - 1) {
    const double done = !(rz == rz) ? 2.0 : (rz <= target ? 1.0 : 0.0);
    pcgCloseFromShares(scal, enqueued, rz, old, (old != 0.0) ? rz / old : 0.0, done, hostMirror);
    scal[S_RR] = rr;
  } else if (applied >= 1) {
    scal[S_RR] = rr;  // (r^T r of the last iteration that was applied: the products do not sum it)
  }
}

// xcand = x + dx with the lower bound 0 on theta_k[0] when requested (ParameterBlock::Plus projection).
inline __global__ void k_apply_step(Layout L, int boundDepth0, const double* __restrict__ x, const double* __restrict__ dx,
                             double* __restrict__ xc) {
  const size_t n = static_cast<size_t>(L.F) * L.B;
  const size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double v = x[i] + dx[i];
  if (boundDepth0) {
    const int c = static_cast<int>(i % L.B);
    if (c >= 7 && c < 7 + L.nD && ((c - 7) % L.N) == 0) v = fmax(v, 0.0);
  }
  xc[i] = v;
}

// ---- first residual of the temporal levels (launchTlRowsInit, cvd_solve.hip).  It lives beside k_cg_update because the two are the
// callers of tlLevelRows<false, NoMid>: compiled apart, the update kernel's code changes (interprocedural constants) ----
// t = A_T^-1 P^T r, r_T = P^T r, tl, and the level's part of r^T z added to S_RZPART (k_cg_update(init) left the block-Jacobi part
// there; the pose-graph level's kernel closes the scalars afterwards)
inline __global__ __launch_bounds__(1024) void k_tl_rows_init(const TlStep* __restrict__ tsp, int F, double* __restrict__ scal,
                                                       unsigned int* __restrict__ counter, int closeScalars, double tol2,
                                                       double* __restrict__ hostMirror) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  __shared__ int flag;
  NoMid mid;
  double alpha = 0.0;
  (void)tlLevelRows<false>(tsp, blockIdx.x, F, alpha, 1, 0.0, scal, sm, mid);
  if (!lastBlockArrivesLite(counter, gridDim.x, &flag)) return;
  if (threadIdx.x == 0) {
    double d = 0.0;
    for (int s = 0; s < tsp->S * tsp->parts; ++s) d += readPartial(tsp->dotPart + s);
    if (closeScalars) pcgFinishScalars(scal, 1, scal[S_RZPART] + d, scal[S_RR], tol2, hostMirror);
    else scal[S_RZPART] += d;
  }
}

}  // namespace cvd
