// cvd_table.h -- per-frame constants and the compiled constraint table: the kernels that run once per problem or per
// evaluation point, before anything is assembled (kernel map: cvd_kernels.h).
#pragma once

#include "cvd_kernels.h"

namespace cvd {

// ---------------------------------------------------------------------------------------------------
inline __global__ void k_frame_consts(Layout L, const double* __restrict__ x, FrameConst* __restrict__ fc) {
  const int f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= L.F) return;
  FrameConst c;
  frameConstFromParams(x + static_cast<size_t>(f) * L.B, L.intrOpt, L.vFocal, x, c);
  fc[f] = c;
}

// Observation ctor, reference lib/PoseOptimizer.cpp:104-116 (float arithmetic, no FMA contraction).
inline __global__ void k_build_table(int W, int H, float invAspect, long long C, const float4* __restrict__ loc,
                              const unsigned char* __restrict__ isStatic, const int* __restrict__ cpair,
                              const int* __restrict__ pairA, const int* __restrict__ pairB,
                              const unsigned char* __restrict__ inRange, const float* __restrict__ depth,
                              float4* __restrict__ ndc, float2* __restrict__ dsrc,
                              unsigned long long* __restrict__ nValid, int ignoreStatic) {
  // ignoreStatic: normalizeDepth's pair loop takes every constraint, dynamic ones included (reference
  // lib/PoseOptimizer.cpp:1036-1052 never looks at isStatic)
  const long long c = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x;
  bool ok = false;
  if (c < C) {
    const float4 l = loc[c];
    const int p = cpair[c];
    const int fa = pairA[p], fb = pairB[p];
    float4 n;
    n.x = __fadd_rn(-1.f, __fmul_rn(2.f, l.x));
    n.y = __fsub_rn(1.f, __fdiv_rn(__fmul_rn(2.f, l.y), invAspect));
    n.z = __fadd_rn(-1.f, __fmul_rn(2.f, l.z));
    n.w = __fsub_rn(1.f, __fdiv_rn(__fmul_rn(2.f, l.w), invAspect));
    int ax = static_cast<int>(__fmul_rn(l.x, static_cast<float>(W)));
    int ay = static_cast<int>(__fmul_rn(__fdiv_rn(l.y, invAspect), static_cast<float>(H)));
    int bx = static_cast<int>(__fmul_rn(l.z, static_cast<float>(W)));
    int by = static_cast<int>(__fmul_rn(__fdiv_rn(l.w, invAspect), static_cast<float>(H)));
    ax = min(max(ax, 0), W - 1); ay = min(max(ay, 0), H - 1);
    bx = min(max(bx, 0), W - 1); by = min(max(by, 0), H - 1);
    const size_t fs = static_cast<size_t>(W) * H;
    float da = depth[fa * fs + static_cast<size_t>(ay) * W + ax];
    float db = depth[fb * fs + static_cast<size_t>(by) * W + bx];
    ok = (ignoreStatic || isStatic[c]) && inRange[fa] && inRange[fb] && isfinite(da) && da > 0.f && isfinite(db) && db > 0.f;
    if (!ok) { da = 0.f; db = 0.f; }
    ndc[c] = n;
    dsrc[c] = make_float2(da, db);
  }
  const unsigned long long b = __ballot(ok);
  if ((threadIdx.x & 63) == 0 && b) atomicAdd(nValid, static_cast<unsigned long long>(__popcll(b)));
}

// Table order (cvd_solver_options::constraint_order).  The constraint lists arrive in raster order: the 64 lanes of a
// wave are neighbours along an image row, 2 - 4 of them inside the same cell of the depth grid, and their LDS f64 atomics
// on that cell's vertices (and the lanes of the next sample row: the same cells again) serialise -- SQ_LDS_BANK_CONFLICT is
// 88 % of the LDS-active cycles of the hot product.  Every directed pair's slice of the table is therefore re-ordered as a
// SWEEP OVER THE CELLS: first one constraint of every non-empty cell in cell order, then the second of every cell that has
// one, ...  Consecutive lanes then hit consecutive cells, i.e. distinct vertices on consecutive LDS banks (measured on the
// benchmark: product 52.6 -> 49.5 us, assembly 0.38 -> 0.34 ms; 1000 frames / 16 x 12 grid: 242 -> 212 us, 1.71 -> 1.20 ms;
// a random order: 56 us; two constraints of a cell side by side: no gain).  One wave per directed pair, windows of
// kOrderCap constraints, everything in a fixed order (the sums downstream stay reproducible).
constexpr int kOrderCap = 4096;       // constraints per window
constexpr int kOrderMaxCells = 4096;  // gx * gy
inline __global__ __launch_bounds__(64) void k_order_table(const long long* __restrict__ pairOff, int gx, int gy, double maxcx,
                                                           double maxcy, const float4* __restrict__ ndcIn,
                                                           const float2* __restrict__ dsrcIn, float4* __restrict__ ndcOut,
                                                           float2* __restrict__ dsrcOut) {
  extern __shared__ __attribute__((aligned(16))) int smo[];
  const int nCells = gx * gy;
  int* start = smo;  // nCells + 1: counts, then exclusive prefix sums
  unsigned short* cellOf = reinterpret_cast<unsigned short*>(smo + nCells + 1);
  unsigned short* rankOf = cellOf + kOrderCap;
  unsigned short* sorted = rankOf + kOrderCap;
  const int lane = threadIdx.x;
  const unsigned long long below = (1ull << lane) - 1ull;
  const long long pb = pairOff[blockIdx.x], pe = pairOff[blockIdx.x + 1];
  for (long long w0 = pb; w0 < pe; w0 += kOrderCap) {
    const int n = static_cast<int>(pe - w0 < kOrderCap ? pe - w0 : kOrderCap);
    for (int c = lane; c <= nCells; c += 64) start[c] = 0;
    __syncthreads();
    // A: cell of every constraint and its rank among the constraints of that cell (input order)
    for (int i0 = 0; i0 < n; i0 += 64) {
      const int i = i0 + lane;
      const bool valid = i < n;
      int cell = -1;
      if (valid) {
        const float4 nd = ndcIn[w0 + i];
        int ix, iy;
        double rx, ry;
        gridCell(nd.x, gx, maxcx, ix, rx);
        gridCell(nd.y, gy, maxcy, iy, ry);
        cell = ix + iy * gx;
      }
      unsigned long long todo = __ballot(valid);
      int rank = 0;
      while (todo) {
        const int leader = __ffsll(static_cast<long long>(todo)) - 1;
        const int c0 = __shfl(cell, leader, 64);
        const bool mine = valid && cell == c0;
        const unsigned long long m = __ballot(mine);
        if (mine) rank = start[c0] + __popcll(m & below);
        if (lane == leader) start[c0] += __popcll(m);   // (LDS operations of one wave execute in order)
        todo &= ~m;
      }
      if (valid) {
        cellOf[i] = static_cast<unsigned short>(cell);
        rankOf[i] = static_cast<unsigned short>(rank);
      }
    }
    __syncthreads();
    // exclusive prefix sums of the counts
    int carry = 0;
    for (int c0 = 0; c0 <= nCells; c0 += 64) {
      const int c = c0 + lane;
      const int v = c < nCells ? start[c] : 0;
      int incl = v;
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const int t = __shfl_up(incl, d, 64);
        if (lane >= d) incl += t;
      }
      if (c <= nCells) start[c] = carry + incl - v;
      carry += __shfl(incl, 63, 64);
    }
    __syncthreads();
    // B: constraints grouped by cell
    for (int i = lane; i < n; i += 64) sorted[start[cellOf[i]] + rankOf[i]] = static_cast<unsigned short>(i);
    __syncthreads();
    // C: sweep r = 0, 1, ...: the r-th constraint of every cell that has one, in cell order
    int base = 0;
    for (int r = 0; base < n; ++r) {
      for (int c0 = 0; c0 < nCells; c0 += 64) {
        const int c = c0 + lane;
        const bool has = c < nCells && start[c + 1] - start[c] > r;
        const unsigned long long m = __ballot(has);
        if (has) {
          const long long src = w0 + sorted[start[c] + r];
          const long long dst = w0 + base + __popcll(m & below);
          ndcOut[dst] = ndcIn[src];
          dsrcOut[dst] = dsrcIn[src];
        }
        base += __popcll(m);
      }
    }
    __syncthreads();
  }
}

// Valid constraints of the dense mode (what k_build_table counts for the list mode).
inline __global__ void k_dense_count(Table T, int P, const unsigned char* __restrict__ inRange, unsigned long long* __restrict__ nValid) {
  const long long npx = static_cast<long long>(T.W) * T.H;
  const long long c = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x;
  bool ok = false;
  if (c < npx * P) {
    const int p = static_cast<int>(c / npx);
    const int fa = T.pairA[p], fb = T.pairB[p];
    float4 n;
    float2 d;
    ok = inRange[fa] && inRange[fb] && fa != fb && loadConstraint<true>(T, c, static_cast<long long>(p) * npx, fa, fb, n, d);
  }
  const unsigned long long b = __ballot(ok);
  if ((threadIdx.x & 63) == 0 && b) atomicAdd(nValid, static_cast<unsigned long long>(__popcll(b)));
}

// AdaptiveDeformationCost constructor (reference lib/PoseOptimizer.cpp:560-618): every mask pixel is splatted bilinearly
// onto the four surrounding grid vertices, into the static (mask > 127) or the dynamic sums; vertex weight = dynamic /
// (dynamic + static).  One workgroup per frame, LDS accumulators (the sums are order-dependent only in the last bits).
inline __global__ __launch_bounds__(256) void k_adaptive_weights(const unsigned char* __restrict__ masks, int dw, int dh, int gw,
                                                          int gh, double* __restrict__ weights) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  const int G = gw * gh;
  double* dyn = sm;
  double* sta = sm + G;
  const int f = blockIdx.x;
  for (int i = threadIdx.x; i < 2 * G; i += blockDim.x) sm[i] = 0.0;
  __syncthreads();
  const unsigned char* m = masks + static_cast<size_t>(f) * dw * dh;
  for (int p = threadIdx.x; p < dw * dh; p += blockDim.x) {
    const int y = p / dw, x = p - y * dw;
    const double fy = static_cast<double>(y) * (gh - 1) / dh;
    const int iy = static_cast<int>(fy);
    const double ry = fy - iy;
    const double fx = static_cast<double>(x) * (gw - 1) / dw;
    const int ix = static_cast<int>(fx);
    const double rx = fx - ix;
    double* w = m[p] > 127 ? sta : dyn;
    atomicAdd(&w[iy * gw + ix], (1.0 - rx) * (1.0 - ry));
    atomicAdd(&w[iy * gw + ix + 1], rx * (1.0 - ry));
    atomicAdd(&w[(iy + 1) * gw + ix], (1.0 - rx) * ry);
    atomicAdd(&w[(iy + 1) * gw + ix + 1], rx * ry);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < G; i += blockDim.x) weights[static_cast<size_t>(f) * G + i] = dyn[i] / (dyn[i] + sta[i]);
}

}  // namespace cvd
