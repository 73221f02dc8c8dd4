// Epipolar RANSAC on the pair constraints: FlowConstraintsCollection::setStaticFlagFromRansac (the reference's caller,
// pose_optimization.py:170-174, names the method; its C++ never implemented it).  The method is defined in
// tests/epipolar_reference.py and DESIGN.md section 3.7; per directed pair p with n constraints:
//   pixels x_a = loc.xy * w, x_b = loc.zw * w (f64), Hartley normalisation per side; hypothesis k draws 8 distinct indices
//   splitmix64(seed << 44 | p << 24 | k << 8 | c) mod n, solves the 8 x 9 system x_b^T F x_a = 0 by full-pivoting elimination,
//   enforces rank 2 and denormalises; its count = constraints with max(d_a, d_b) <= threshold; the winner (largest count,
//   lowest k) is refitted once over its inliers (9 x 9 normal matrix, Jacobi) and the refit is adopted when it scores no
//   fewer inliers.  The adopted F's inliers are the pair's static flags.
//
// f64 throughout, no float atomics, every reduction in a fixed order: the result is bitwise the same run to run.
//   k_epi_normalise    one 256-thread workgroup per pair: the two centroids and mean distances (fixed-order LDS trees).
//   k_epi_hypotheses   one thread per (pair, k), 64-thread workgroups: sampler, the 8 x 9 elimination held in VGPRs (every
//                      index static: pivots are chosen and rows / columns swapped with selects), closed-form rank 2, F out.
//   k_epi_score        one 256-thread workgroup per (pair, block of 256 hypotheses): the pair's points are staged in LDS as
//                      f64 pixels in chunks of kEpiChunk, every lane reads the same point (a broadcast) and tests it against
//                      its own F held in VGPRs; an integer count per hypothesis.
//   k_epi_select       one 256-thread workgroup per pair: winner (LDS tree on (count, -k)), the winner's inliers summed into
//                      the 9 x 9 normal matrix (45 sums per thread in point order, butterfly per wave, waves in order), cyclic
//                      Jacobi by wave 0 (lane i holds row i), rank 2, rescoring, flags.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace cvd {

constexpr int kEpiThreads = 256;       // normalise / score / select workgroups
constexpr int kEpiHypThreads = 64;     // hypothesis workgroups (one wave)
constexpr int kEpiChunk = 1024;        // points per LDS chunk of the scoring kernel (32 KB of double4)
constexpr int kEpiMaxDraws = 256;      // draw counter c < 2^8
constexpr int kEpiMaxIterations = 65536;
constexpr int kEpiMaxPairs = 1 << 20;
constexpr int kEpiJacobiSweeps = 50;
constexpr double kEpiPivotRtol = 1e-12;

struct EpiNorm {  // Hartley normalisation of one pair: x' = s x - s c per side; valid = 0 leaves the pair all static
  double sa, ta0, ta1, sb, tb0, tb1;   // t = -s c
  int valid, pad;
};

struct EpiArgs {
  int numPairs;               // pairs of this launch
  int pairBase;               // global index of the launch's pair 0 (the sampler key)
  int K;                      // hypotheses per pair
  unsigned long long seed;
  double w;                   // pixel scale (width of the raster the constraints were sampled on)
  double thresh2;             // threshold^2 in px^2
  const long long* off;       // [numPairs + 1] global constraint offsets of the launch's pairs
  const float4* loc;          // [C] (loc0.xy, loc1.xy)
  EpiNorm* norm;              // [numPairs]
  double* F;                  // [numPairs][K][9] F_pix of every hypothesis (0 when invalid)
  int* count;                 // [numPairs][K] inliers (-1: invalid hypothesis)
  unsigned char* flags;       // [C] static flags out
  double* Fbest;              // [numPairs][9] adopted F_pix (0 for an all-static pair)
  int* best;                  // [numPairs][2] (winning k, inliers of the adopted F); (-1, -1) for an all-static pair
};

__device__ __forceinline__ unsigned long long epiSplitmix64(unsigned long long x) {
  unsigned long long z = x + 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// 1 when max(d_a, d_b) <= threshold: r^2 <= t^2 |l|^2 on both lines, a zero line (or a NaN) fails.  Explicit fma, no
// contraction: the scoring and the select kernels must reach the same decision for the same F and point.
__device__ __forceinline__ int epiInlier(const double F[9], const double4 x, double t2) {
#pragma clang fp contract(off)
  const double lb0 = fma(F[0], x.x, fma(F[1], x.y, F[2]));
  const double lb1 = fma(F[3], x.x, fma(F[4], x.y, F[5]));
  const double lb2 = fma(F[6], x.x, fma(F[7], x.y, F[8]));
  const double r = fma(x.z, lb0, fma(x.w, lb1, lb2));
  const double la0 = fma(F[0], x.z, fma(F[3], x.w, F[6]));
  const double la1 = fma(F[1], x.z, fma(F[4], x.w, F[7]));
  const double nb = fma(lb0, lb0, lb1 * lb1), na = fma(la0, la0, la1 * la1);
  const double r2 = r * r;
  return (nb > 0.0) & (na > 0.0) & (r2 <= t2 * nb) & (r2 <= t2 * na);
}

__device__ __forceinline__ double4 epiPixels(const float4 L, double w) {
  return make_double4(static_cast<double>(L.x) * w, static_cast<double>(L.y) * w, static_cast<double>(L.z) * w,
                      static_cast<double>(L.w) * w);
}

// F <- F (I - v v^T), v = unit eigenvector of the smallest eigenvalue of G = F^T F: trigonometric eigenvalue, then the
// longest cross product of two rows of G - lambda I (v = e_z when G is a multiple of I or the rows are dependent).
__device__ __forceinline__ void epiRank2(double f[9]) {
  double G[3][3];
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int d = 0; d < 3; ++d) G[c][d] = f[c] * f[d] + f[3 + c] * f[3 + d] + f[6 + c] * f[6 + d];
  const double q = (G[0][0] + G[1][1] + G[2][2]) / 3.0;
  const double p1 = G[0][1] * G[0][1] + G[0][2] * G[0][2] + G[1][2] * G[1][2];
  const double d0 = G[0][0] - q, d1 = G[1][1] - q, d2 = G[2][2] - q;
  const double p2 = d0 * d0 + d1 * d1 + d2 * d2 + 2.0 * p1;
  double v0 = 0.0, v1 = 0.0, v2 = 1.0;
  if (p2 > 0.0) {
    const double p = sqrt(p2 / 6.0), ip = 1.0 / p;
    const double b00 = d0 * ip, b11 = d1 * ip, b22 = d2 * ip, b01 = G[0][1] * ip, b02 = G[0][2] * ip, b12 = G[1][2] * ip;
    const double det = b00 * (b11 * b22 - b12 * b12) - b01 * (b01 * b22 - b12 * b02) + b02 * (b01 * b12 - b11 * b02);
    const double r = fmin(1.0, fmax(-1.0, 0.5 * det));
    const double lam = q + 2.0 * p * cos(acos(r) / 3.0 + 2.0943951023931954923);  // + 2 pi / 3: the smallest root
    const double m[3][3] = {{G[0][0] - lam, G[0][1], G[0][2]}, {G[1][0], G[1][1] - lam, G[1][2]},
                            {G[2][0], G[2][1], G[2][2] - lam}};
    double bx = 0.0, by = 0.0, bz = 0.0, bn = 0.0;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = a + 1; b < 3; ++b) {
        const double cx = m[a][1] * m[b][2] - m[a][2] * m[b][1];
        const double cy = m[a][2] * m[b][0] - m[a][0] * m[b][2];
        const double cz = m[a][0] * m[b][1] - m[a][1] * m[b][0];
        const double cn = cx * cx + cy * cy + cz * cz;
        if (cn > bn) { bx = cx; by = cy; bz = cz; bn = cn; }
      }
    if (bn > 0.0) {
      const double is = 1.0 / sqrt(bn);
      v0 = bx * is; v1 = by * is; v2 = bz * is;
    }
  }
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const double fv = f[3 * i] * v0 + f[3 * i + 1] * v1 + f[3 * i + 2] * v2;
    f[3 * i] -= fv * v0;
    f[3 * i + 1] -= fv * v1;
    f[3 * i + 2] -= fv * v2;
  }
}

// F_pix = T_b^T F T_a with T = [[s, 0, t0], [0, s, t1], [0, 0, 1]]
__device__ __forceinline__ void epiDenormalise(double f[9], const EpiNorm& N) {
  double g[9];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    g[3 * i] = f[3 * i] * N.sa;
    g[3 * i + 1] = f[3 * i + 1] * N.sa;
    g[3 * i + 2] = f[3 * i] * N.ta0 + f[3 * i + 1] * N.ta1 + f[3 * i + 2];
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    f[c] = N.sb * g[c];
    f[3 + c] = N.sb * g[3 + c];
    f[6 + c] = N.tb0 * g[c] + N.tb1 * g[3 + c] + g[6 + c];
  }
}

// the design row of x_b^T F x_a = 0 (F row-major) in normalised coordinates
__device__ __forceinline__ void epiRow(double a[9], const double4 x, const EpiNorm& N) {
  const double xa = fma(N.sa, x.x, N.ta0), ya = fma(N.sa, x.y, N.ta1);
  const double xb = fma(N.sb, x.z, N.tb0), yb = fma(N.sb, x.w, N.tb1);
  a[0] = xb * xa; a[1] = xb * ya; a[2] = xb;
  a[3] = yb * xa; a[4] = yb * ya; a[5] = yb;
  a[6] = xa; a[7] = ya; a[8] = 1.0;
}

// fixed-order sum over a 256-thread workgroup (sh: 256 doubles); every thread gets the result
__device__ __forceinline__ double epiBlockSum(double v, double* sh) {
  const int t = threadIdx.x;
  sh[t] = v;
  __syncthreads();
#pragma unroll
  for (int s = kEpiThreads / 2; s > 0; s >>= 1) {
    if (t < s) sh[t] += sh[t + s];
    __syncthreads();
  }
  const double r = sh[0];
  __syncthreads();
  return r;
}

// Step R of the 8 x 9 elimination with full pivoting: the first largest |entry| of the remaining block (rows R.., columns R..,
// row-major order) becomes the pivot; rows and columns are swapped with selects so that every array index is a
// compile-time constant (R is a template argument: the steps are unrolled by construction) and the matrix stays in VGPRs.
template <int R>
__device__ __forceinline__ void epiEliminate(double (&a)[8][9], int (&perm)[9], double& amax, bool& ok) {
  if constexpr (R < 8) {
    double bv = -1.0;
    int pr = R, pc = R;
#pragma unroll
    for (int i = R; i < 8; ++i)
#pragma unroll
      for (int j = R; j < 9; ++j) {
        const double v = fabs(a[i][j]);
        if (v > bv) { bv = v; pr = i; pc = j; }
      }
    if (R == 0) amax = bv;
    ok = ok && bv > 0.0 && !(bv < kEpiPivotRtol * amax);
#pragma unroll
    for (int i = R + 1; i < 8; ++i) {
      const bool sw = pr == i;
#pragma unroll
      for (int j = R; j < 9; ++j) {
        const double t = a[i][j];
        a[i][j] = sw ? a[R][j] : t;
        a[R][j] = sw ? t : a[R][j];
      }
    }
#pragma unroll
    for (int j = R + 1; j < 9; ++j) {
      const bool sw = pc == j;
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const double t = a[i][j];
        a[i][j] = sw ? a[i][R] : t;
        a[i][R] = sw ? t : a[i][R];
      }
      const int tp = perm[j];
      perm[j] = sw ? perm[R] : tp;
      perm[R] = sw ? tp : perm[R];
    }
    const double inv = 1.0 / a[R][R];
#pragma unroll
    for (int i = R + 1; i < 8; ++i) {
      const double fac = a[i][R] * inv;
#pragma unroll
      for (int j = R + 1; j < 9; ++j) a[i][j] = fma(-fac, a[R][j], a[i][j]);
      a[i][R] = 0.0;
    }
    epiEliminate<R + 1>(a, perm, amax, ok);
  }
}

// x[R] from the triangular rows R.. (x[8] = 1, the free column)
template <int R>
__device__ __forceinline__ void epiBackSubstitute(const double (&a)[8][9], double (&x)[9]) {
  if constexpr (R >= 0) {
    double acc = a[R][8];
#pragma unroll
    for (int j = R + 1; j < 8; ++j) acc = fma(a[R][j], x[j], acc);
    x[R] = -acc / a[R][R];
    epiBackSubstitute<R - 1>(a, x);
  }
}

inline __global__ __launch_bounds__(kEpiThreads) void k_epi_normalise(EpiArgs A) {
  __shared__ double sh[kEpiThreads];
  const int p = blockIdx.x;
  const long long o0 = A.off[p], n = A.off[p + 1] - o0;
  double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
  for (long long i = threadIdx.x; i < n; i += kEpiThreads) {
    const double4 x = epiPixels(A.loc[o0 + i], A.w);
    s0 += x.x; s1 += x.y; s2 += x.z; s3 += x.w;
  }
  const double dn = static_cast<double>(n > 0 ? n : 1);
  const double cxa = epiBlockSum(s0, sh) / dn, cya = epiBlockSum(s1, sh) / dn;
  const double cxb = epiBlockSum(s2, sh) / dn, cyb = epiBlockSum(s3, sh) / dn;
  double ma = 0.0, mb = 0.0;
  for (long long i = threadIdx.x; i < n; i += kEpiThreads) {
    const double4 x = epiPixels(A.loc[o0 + i], A.w);
    const double ax = x.x - cxa, ay = x.y - cya, bx = x.z - cxb, by = x.w - cyb;
    ma += sqrt(ax * ax + ay * ay);
    mb += sqrt(bx * bx + by * by);
  }
  const double mda = epiBlockSum(ma, sh) / dn, mdb = epiBlockSum(mb, sh) / dn;
  if (threadIdx.x == 0) {
    EpiNorm N;
    N.valid = n >= 8 && mda > 0.0 && mdb > 0.0;
    N.pad = 0;
    N.sa = N.valid ? 1.4142135623730950488 / mda : 0.0;
    N.sb = N.valid ? 1.4142135623730950488 / mdb : 0.0;
    N.ta0 = -N.sa * cxa; N.ta1 = -N.sa * cya;
    N.tb0 = -N.sb * cxb; N.tb1 = -N.sb * cyb;
    A.norm[p] = N;
  }
}

inline __global__ __launch_bounds__(kEpiHypThreads) void k_epi_hypotheses(EpiArgs A) {
  const int p = blockIdx.x;
  const int k = blockIdx.y * kEpiHypThreads + threadIdx.x;
  if (k >= A.K) return;
  const size_t hk = static_cast<size_t>(p) * A.K + k;
  const EpiNorm N = A.norm[p];
  double f[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  bool ok = N.valid != 0;
  if (ok) {
    const long long o0 = A.off[p];
    const unsigned long long n = static_cast<unsigned long long>(A.off[p + 1] - o0);  // >= 8 (valid)
    const unsigned long long key0 = (A.seed << 44) | (static_cast<unsigned long long>(A.pairBase + p) << 24) |
                                    (static_cast<unsigned long long>(k) << 8);
    unsigned long long s[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) s[j] = 0;
    int found = 0;
    for (int c = 0; c < kEpiMaxDraws && found < 8; ++c) {
      const unsigned long long i = epiSplitmix64(key0 | static_cast<unsigned long long>(c)) % n;
      bool dup = false;
#pragma unroll
      for (int j = 0; j < 8; ++j) dup |= (j < found) & (s[j] == i);
      if (!dup) {
#pragma unroll
        for (int j = 0; j < 8; ++j) s[j] = (j == found) ? i : s[j];
        ++found;
      }
    }
    ok = found == 8;
    double a[8][9];
#pragma unroll
    for (int j = 0; j < 8; ++j) epiRow(a[j], epiPixels(A.loc[o0 + static_cast<long long>(s[j])], A.w), N);
    int perm[9];
#pragma unroll
    for (int j = 0; j < 9; ++j) perm[j] = j;
    double amax = 0.0;
    epiEliminate<0>(a, perm, amax, ok);
    double x[9];
    x[8] = 1.0;
    epiBackSubstitute<7>(a, x);
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      double v = 0.0;
#pragma unroll
      for (int j = 0; j < 9; ++j) v = perm[j] == t ? x[j] : v;
      f[t] = v;
    }
    epiRank2(f);
    epiDenormalise(f, N);
#pragma unroll
    for (int j = 0; j < 9; ++j) ok = ok && isfinite(f[j]);
  }
  double* Fo = A.F + hk * 9;
#pragma unroll
  for (int j = 0; j < 9; ++j) Fo[j] = ok ? f[j] : 0.0;
  A.count[hk] = ok ? 0 : -1;
}

inline __global__ __launch_bounds__(kEpiThreads) void k_epi_score(EpiArgs A) {
  __shared__ double4 pts[kEpiChunk];
  const int p = blockIdx.x;
  if (!A.norm[p].valid) return;  // (workgroup-uniform) every count of the pair is already -1
  const int k = blockIdx.y * kEpiThreads + threadIdx.x;
  const size_t hk = static_cast<size_t>(p) * A.K + k;
  const bool act = k < A.K && A.count[hk] >= 0;
  double F[9];
#pragma unroll
  for (int j = 0; j < 9; ++j) F[j] = act ? A.F[hk * 9 + j] : 0.0;
  const long long o0 = A.off[p], n = A.off[p + 1] - o0;
  int cnt = 0;
  for (long long c0 = 0; c0 < n; c0 += kEpiChunk) {
    const int m = static_cast<int>(n - c0 < kEpiChunk ? n - c0 : kEpiChunk);
    __syncthreads();
    for (int i = threadIdx.x; i < m; i += kEpiThreads) pts[i] = epiPixels(A.loc[o0 + c0 + i], A.w);
    __syncthreads();
    if (act) {
#pragma unroll 4
      for (int i = 0; i < m; ++i) cnt += epiInlier(F, pts[i], A.thresh2);
    }
  }
  if (act) A.count[hk] = cnt;
}

inline __global__ __launch_bounds__(kEpiThreads) void k_epi_select(EpiArgs A) {
  __shared__ int shc[kEpiThreads], shk[kEpiThreads];
  __shared__ double part[kEpiThreads / 64][45];
  __shared__ double Fsh[9];
  const int p = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const long long o0 = A.off[p], n = A.off[p + 1] - o0;
  const EpiNorm N = A.norm[p];
  // winner: largest count, lowest k
  int bc = -2, bk = 0x7fffffff;
  for (int k = t; k < A.K; k += kEpiThreads) {
    const int c = A.count[static_cast<size_t>(p) * A.K + k];
    if (c > bc) { bc = c; bk = k; }
  }
  shc[t] = bc; shk[t] = bk;
  __syncthreads();
  for (int s = kEpiThreads / 2; s > 0; s >>= 1) {
    if (t < s) {
      const int c2 = shc[t + s], k2 = shk[t + s];
      if (c2 > shc[t] || (c2 == shc[t] && k2 < shk[t])) { shc[t] = c2; shk[t] = k2; }
    }
    __syncthreads();
  }
  bc = shc[0]; bk = shk[0];
  if (!N.valid || bc < 0) {  // (workgroup-uniform)
    for (long long i = t; i < n; i += kEpiThreads) A.flags[o0 + i] = 1;
    if (t < 9) A.Fbest[static_cast<size_t>(p) * 9 + t] = 0.0;
    if (t == 0) { A.best[2 * p] = -1; A.best[2 * p + 1] = -1; }
    return;
  }
  double F[9];
#pragma unroll
  for (int j = 0; j < 9; ++j) F[j] = A.F[(static_cast<size_t>(p) * A.K + bk) * 9 + j];
  int adoptedCount = bc;
  if (bc >= 8) {
    // the 9 x 9 normal matrix of the winner's inliers: 45 sums per thread in point order, butterfly per wave, waves in order
    double m[45];
#pragma unroll
    for (int e = 0; e < 45; ++e) m[e] = 0.0;
    for (long long i = t; i < n; i += kEpiThreads) {
      const double4 x = epiPixels(A.loc[o0 + i], A.w);
      if (!epiInlier(F, x, A.thresh2)) continue;
      double a[9];
      epiRow(a, x, N);
      int e = 0;
#pragma unroll
      for (int r = 0; r < 9; ++r)
#pragma unroll
        for (int c = r; c < 9; ++c, ++e) m[e] = fma(a[r], a[c], m[e]);
    }
#pragma unroll
    for (int e = 0; e < 45; ++e) {
      double v = m[e];
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
      if (lane == 0) part[wave][e] = v;
    }
    __syncthreads();
    if (wave == 0) {
      // cyclic Jacobi on M: lane i < 9 holds row i of M and of the eigenvector matrix V (other lanes hold zeros)
      double row[9], vr[9];
#pragma unroll
      for (int c = 0; c < 9; ++c) {
        const int r = lane < 9 ? lane : 0, lo = r < c ? r : c, hi = r < c ? c : r;
        const int e = lo * 9 - lo * (lo - 1) / 2 + (hi - lo);
        double v = 0.0;
#pragma unroll
        for (int w = 0; w < kEpiThreads / 64; ++w) v += part[w][e];
        row[c] = lane < 9 ? v : 0.0;
        vr[c] = lane == c ? 1.0 : 0.0;
      }
      for (int sweep = 0; sweep < kEpiJacobiSweeps; ++sweep) {
        double off = 0.0, tot = 0.0;
#pragma unroll
        for (int c = 0; c < 9; ++c) {
          const double q2 = row[c] * row[c];
          tot += q2;
          off += c == lane ? 0.0 : q2;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { off += __shfl_xor(off, o, 64); tot += __shfl_xor(tot, o, 64); }
        if (!(off > 1e-30 * tot)) break;
#pragma unroll
        for (int pp = 0; pp < 8; ++pp)
#pragma unroll
          for (int qq = pp + 1; qq < 9; ++qq) {
            const double apq = __shfl(row[qq], pp, 64);
            if (apq == 0.0) continue;  // (wave-uniform)
            const double app = __shfl(row[pp], pp, 64), aqq = __shfl(row[qq], qq, 64);
            const double th = (aqq - app) / (2.0 * apq);
            const double tt = (th >= 0.0 ? 1.0 : -1.0) / (fabs(th) + sqrt(fma(th, th, 1.0)));
            const double cs = 1.0 / sqrt(fma(tt, tt, 1.0)), sn = tt * cs;
            // columns pp, qq of every row (A J), then rows pp, qq (J^T A J), then V J
            const double rp = row[pp], rq = row[qq];
            row[pp] = cs * rp - sn * rq;
            row[qq] = sn * rp + cs * rq;
#pragma unroll
            for (int c = 0; c < 9; ++c) {
              const double xp = __shfl(row[c], pp, 64), xq = __shfl(row[c], qq, 64);
              row[c] = lane == pp ? cs * xp - sn * xq : (lane == qq ? sn * xp + cs * xq : row[c]);
            }
            const double vp = vr[pp], vq = vr[qq];
            vr[pp] = cs * vp - sn * vq;
            vr[qq] = sn * vp + cs * vq;
          }
      }
      // smallest diagonal entry (first on ties), its column of V
      double dmin = __shfl(row[0], 0, 64);
      int jm = 0;
#pragma unroll
      for (int c = 1; c < 9; ++c) {
        const double d = __shfl(row[c], c, 64);
        if (d < dmin) { dmin = d; jm = c; }
      }
      double mine = 0.0;
#pragma unroll
      for (int c = 0; c < 9; ++c) mine = c == jm ? vr[c] : mine;
      double fr[9];
#pragma unroll
      for (int c = 0; c < 9; ++c) fr[c] = __shfl(mine, c, 64);
      epiRank2(fr);
      epiDenormalise(fr, N);
      if (lane < 9) {
        double v = 0.0;
#pragma unroll
        for (int c = 0; c < 9; ++c) v = c == lane ? fr[c] : v;
        Fsh[lane] = v;
      }
    }
    __syncthreads();
    double Fr[9];
    bool fin = true;
#pragma unroll
    for (int j = 0; j < 9; ++j) { Fr[j] = Fsh[j]; fin = fin && isfinite(Fr[j]); }
    int cr = 0;
    if (fin)
      for (long long i = t; i < n; i += kEpiThreads) cr += epiInlier(Fr, epiPixels(A.loc[o0 + i], A.w), A.thresh2);
    shc[t] = cr;
    __syncthreads();
    for (int s = kEpiThreads / 2; s > 0; s >>= 1) {
      if (t < s) shc[t] += shc[t + s];
      __syncthreads();
    }
    cr = shc[0];
    if (fin && cr >= bc) {
      adoptedCount = cr;
#pragma unroll
      for (int j = 0; j < 9; ++j) F[j] = Fr[j];
    }
  }
  for (long long i = t; i < n; i += kEpiThreads)
    A.flags[o0 + i] = static_cast<unsigned char>(epiInlier(F, epiPixels(A.loc[o0 + i], A.w), A.thresh2));
  if (t < 9) {
    double v = 0.0;
#pragma unroll
    for (int c = 0; c < 9; ++c) v = c == t ? F[c] : v;
    A.Fbest[static_cast<size_t>(p) * 9 + t] = v;
  }
  if (t == 0) { A.best[2 * p] = bk; A.best[2 * p + 1] = adoptedCount; }
}

}  // namespace cvd
