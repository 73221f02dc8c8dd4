// Backward operators of the MiDaS v2.1 decoder's layers, f32: the gradients of the stride-1 convolutions of
// cvd_midas.h with respect to their input and their weights, and the backward of the bilinear x 2 upsampling.  This header does not
// include cvd_midas.h and shares no type with it; the front end, which includes both, runs the input gradient on the forward's own
// k_midas_conv (below).
//
//   k_midas_wflip<KS>             W [N][Cin][KS][KS] -> W' [Cin][N][KS][KS], W'[c][n][i][j] = W[n][c][KS-1-i][KS-1-j]: the filter whose
//                                 FORWARD convolution of gy is the input gradient, gx[b][c][h][w] = sum_{n,i,j} gy[b][n][h-i+p][w-j+p]
//                                 W[n][c][i][j].  One thread per element, a pure permutation.
//   k_midas_dgrad_fold            the input gradient's epilogue: element e of [B][Cin][H][W] = the S partial sums of the convolution
//                                 above in f64 in the order s = 0 .. S - 1, rounded ONCE to f32 (S = 1: the sum itself); with an
//                                 addend t = t + add[e]; with a mask t = mask[e] > 0 ? t : 0 (torch's ReLU: gradient 0 at 0).
//   k_midas_wgrad<KS>             gW[n][c][i][j] = sum_{b,h,w} gy[b][n][h][w] X[b][c][h+i-p][w+j-p], X = max(x, 0) under reluIn.
//   k_midas_wgrad_fold            sums the partial sums of a split weight gradient.
//   k_midas_bias_grad             gbias[n] = sum_{b,h,w} gy[b][n][h][w].
//   k_midas_upsample2x_grad<ALIGN> backward of k_midas_upsample2x in gather form.
//   k_midas_head_grad             the pointwise part of the output head's backward: from gy, the head's output y and the 32-channel
//                                 pre-activation t it writes the gradient g32 of t and per-workgroup sums for output_conv.4.
//   k_midas_head_grad_sum         the second stage of those sums.
//
// The weight gradient is a GEMM on the exact f32 MFMA (v_mfma_f32_32x32x2_f32: bit for bit a k-ordered fmaf chain) whose reduction
// runs over the pixels: rows = the N output channels, columns q = (c KS + i) KS + j = the Q = Cin KS KS elements of a weight row (so
// the result is the weight tensor, row-major), k = the flat pixel p of [B][H][W].  Both operands are contiguous along p in NCHW.  A
// workgroup (4 waves) owns a 64 row x 64 column tile, wave w the 32 x 32 sub-tile (columns 32 (w & 1), rows 32 (w >> 1)); a wave
// whose rows all lie past N or whose columns all lie past Q stages and waits at the barriers but issues no MFMA.  A chunk is 32
// pixels: thread (pixel pl = tid & 31, group g = tid >> 5) loads the rows g, g + 8, .. of gy and the columns g, g + 8, .. of the
// shifted input at its pixel, so a load instruction's lanes walk consecutive pixels.  Whether tap (i, j) of a pixel lies in the
// image is decided per PIXEL from its own (row, column), as in the forward; every load is unconditional and in range (a tap outside
// the image reads the pixel's own centre, a row past N the tile's first row, a column past Q column 0, a pixel past M pixel 0 of
// image 0) and is zeroed on its way to the LDS.
//
// Summation.  One fmaf chain per kWgFold = 8 chunks (256 pixels), each folded into a second register set as it completes, chains
// summed in pixel order, a last shorter chain added last.  The pixels are dealt to S slices of whole chains, slice s = blockIdx.z;
// S = midasWgradSplit(M, N, Q) is a pure function of the three GEMM sizes.  With S = 1 the kernel writes gW itself; with S > 1 it
// writes its sum to partial s of a scratch tensor [S][N][Q] with plain stores and k_midas_wgrad_fold sums the S partial sums of an
// element in f64 in the order s = 0 .. S - 1 and rounds once.  No atomics: one lane writes each element once.
//
// The bias gradient is its own reduction: one workgroup per channel, thread t sums the pixels t, t + 256, .. in f64 in that order,
// the 256 sums are added by a fixed tree in the LDS and rounded once.
#pragma once
#include <hip/hip_runtime.h>

namespace cvd {

constexpr int kMgThreads = 256;
constexpr int kWgTile = 64;            // rows (output channels) and columns (elements of a weight row) of a workgroup's tile
constexpr int kWgPixels = 32;          // pixels of a staged chunk
constexpr int kWgFold = 8;             // chunks per fmaf chain
constexpr int kWgChain = kWgPixels * kWgFold;      // 256 terms
constexpr int kWgMaxSplit = 128;
constexpr int kWgTargetGroups = 1024;  // workgroups a launch is brought up to by the split: four for each of the 256 CUs

// The split count of a weight gradient over M = B H W pixels with N rows and Q = Cin KS KS columns: as many slices of the pixels as
// bring the launch to kWgTargetGroups workgroups, each slice whole chains, at most kWgMaxSplit.  M, N and Q alone decide it.
inline int midasWgradSplit(long long M, long long N, long long Q) {
  const long long tiles = ((N + kWgTile - 1) / kWgTile) * ((Q + kWgTile - 1) / kWgTile);
  const long long chains = (M + kWgChain - 1) / kWgChain;
  long long want = kWgTargetGroups / tiles;
  if (want > kWgMaxSplit) want = kWgMaxSplit;
  if (want > chains) want = chains;
  if (want < 1) want = 1;
  const long long per = (chains + want - 1) / want;               // chains per slice
  return static_cast<int>((chains + per - 1) / per);
}

struct MidasFlipArgs {
  const float* w;             // [N][Cin][KS][KS]
  float* out;                 // [Cin][N][KS][KS]
  int N, Cin;
  long long total;            // N Cin KS KS
};

template <int KS>
inline __global__ __launch_bounds__(kMgThreads) void k_midas_wflip(MidasFlipArgs A) {
  constexpr int T = KS * KS;
  const long long e = static_cast<long long>(blockIdx.x) * kMgThreads + threadIdx.x;
  if (e >= A.total) return;
  const int t = static_cast<int>(e % T);
  const long long cn = e / T;
  const int n = static_cast<int>(cn % A.N), c = static_cast<int>(cn / A.N);
  A.out[e] = A.w[(static_cast<size_t>(n) * A.Cin + c) * T + (T - 1 - t)];
}

struct MidasDgradFoldArgs {
  const float* partial;       // [S][total]
  const float* add;           // or null: [total]
  const float* mask;          // or null: [total]
  float* out;                 // [total]
  int S;
  long long total;            // B Cin H W
};

inline __global__ __launch_bounds__(kMgThreads) void k_midas_dgrad_fold(MidasDgradFoldArgs A) {
  const long long i = static_cast<long long>(blockIdx.x) * kMgThreads + threadIdx.x;
  if (i >= A.total) return;
  double sum = 0.0;
  for (int s = 0; s < A.S; ++s) sum += static_cast<double>(A.partial[static_cast<size_t>(s) * static_cast<size_t>(A.total) + i]);
  float t = static_cast<float>(sum);
  if (A.add != nullptr) t = t + A.add[i];
  if (A.mask != nullptr) t = A.mask[i] > 0.f ? t : 0.f;
  A.out[i] = t;
}

struct MidasWgradArgs {
  const float* gy;            // [B][N][H][W]
  const float* x;             // [B][Cin][H][W]
  float* out;                 // S == 1: gW [N][Q]; S > 1: the partial sums [S][N][Q]
  int reluIn;
  int N, Cin, Q;              // Q = Cin KS KS
  int H, W, HW;
  int chunksPerSlice;         // a multiple of kWgFold
  long long M;                // B H W
};

using midas_grad_f32x16 = __attribute__((ext_vector_type(16))) float;

template <int KS>
inline __global__ __launch_bounds__(kMgThreads) void k_midas_wgrad(MidasWgradArgs A) {
  static_assert(KS == 1 || KS == 3, "filter sizes of the decoder");
  constexpr int T = KS * KS, R = KS / 2, PK = kWgPixels;
  constexpr int GS = PK + 1;                 // odd strides: the 32 lanes of an operand read, resp. of a staging write, fall on
  constexpr int XS = kWgTile + 1;            // distinct banks
  constexpr int PG = kMgThreads / PK;        // 8 thread groups share the chunk's pixels and stride over rows and columns
  constexpr int J = kWgTile / PG;            // rows and columns a thread stages: 8
  __shared__ float sG[kWgTile * GS];         // [row][pixel]
  __shared__ float sX[PK * XS];              // [pixel][column]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int pl = tid % PK, grp = tid / PK;
  const int q0 = static_cast<int>(blockIdx.x) * kWgTile, n0 = static_cast<int>(blockIdx.y) * kWgTile;
  const int slice = static_cast<int>(blockIdx.z);

  // the thread's columns (c, tap) and rows: fixed for the launch (channels, not offsets, are kept: 32 bits each)
  int colC[J];                               // the column's input channel
  int colOff[J];                             // the tap's offset from the centre (applied where the tap lies in the image)
  unsigned colTap = 0, colOk = 0, rowOk = 0; // 4 bits of tap index per column; bit j = column / row g + 8 j exists
#pragma unroll
  for (int j = 0; j < J; ++j) {
    const int q = q0 + grp + PG * j;
    const bool ok = q < A.Q;
    const int qq = ok ? q : 0;
    const int c = qq / T, t = qq - c * T;
    colC[j] = c;
    colOff[j] = (t / KS - R) * A.W + (t % KS - R);
    colTap |= static_cast<unsigned>(t) << (4 * j);
    if (ok) colOk |= 1u << j;
    if (n0 + grp + PG * j < A.N) rowOk |= 1u << j;
  }

  const long long numChunks = (A.M + PK - 1) / PK;
  const long long chunk0 = static_cast<long long>(slice) * A.chunksPerSlice;      // (< numChunks: the host's S leaves no empty slice)
  const long long chunk1 = chunk0 + A.chunksPerSlice < numChunks ? chunk0 + A.chunksPerSlice : numChunks;

  const int qsub = wave & 1, nsub = wave >> 1;
  const int half = lane >> 5, l31 = lane & 31;
  const bool mfmaLive = n0 + nsub * 32 < A.N && q0 + qsub * 32 < A.Q;              // wave-uniform
  const float* opG = sG + (nsub * 32 + l31) * GS + half;          // A operand: lane holds gy[row l31][pixel k = half]
  const float* opX = sX + half * XS + qsub * 32 + l31;            // B operand: lane holds X[pixel k = half][column l31]
  midas_grad_f32x16 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  midas_grad_f32x16 total = acc;

  // A chunk travels global -> registers -> LDS: the loads of chunk c + 1 are issued before the MFMA of chunk c.
  float gv[J], xv[J];
  unsigned xIn = 0;                          // bit j = column j's tap lies in the image at this chunk's pixel
  bool live = false;
  const auto load = [&](long long chunk) {
    const long long p = chunk * PK + pl;
    live = p < A.M;
    long long img = 0;
    int pix = 0;
    if (live) {
      img = p / A.HW;
      pix = static_cast<int>(p - img * A.HW);
    }
    const int cy = pix / A.W, cx = pix - cy * A.W;
    unsigned tapIn = 0;
#pragma unroll
    for (int t = 0; t < T; ++t) {
      const int y = cy + t / KS - R, x = cx + t % KS - R;
      if (live && y >= 0 && y < A.H && x >= 0 && x < A.W) tapIn |= 1u << t;
    }
    const float* __restrict__ gc = A.gy + static_cast<size_t>(img) * A.N * A.HW + static_cast<size_t>(pix);
    const float* __restrict__ xc = A.x + static_cast<size_t>(img) * A.Cin * A.HW + static_cast<size_t>(pix);
    xIn = 0;
#pragma unroll
    for (int j = 0; j < J; ++j) {
      gv[j] = gc[static_cast<size_t>(n0 + (((rowOk >> j) & 1u) ? grp + PG * j : 0)) * A.HW];
      const bool in = ((tapIn >> ((colTap >> (4 * j)) & 15u)) & 1u) && ((colOk >> j) & 1u);
      xv[j] = xc[static_cast<size_t>(colC[j]) * A.HW + (in ? colOff[j] : 0)];
      if (in) xIn |= 1u << j;
    }
  };
  if (chunk0 < chunk1) load(chunk0);
  for (long long chunk = chunk0; chunk < chunk1; ++chunk) {
#pragma unroll
    for (int j = 0; j < J; ++j) {
      sG[(grp + PG * j) * GS + pl] = (live && ((rowOk >> j) & 1u)) ? gv[j] : 0.f;
      float v = ((xIn >> j) & 1u) ? xv[j] : 0.f;
      if (A.reluIn) v = v < 0.f ? 0.f : v;
      sX[pl * XS + grp + PG * j] = v;
    }
    __syncthreads();
    if (chunk + 1 < chunk1) load(chunk + 1);
    if (mfmaLive) {
#pragma unroll 8
      for (int kk = 0; kk < PK; kk += 2) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(opG[kk], opX[kk * XS], acc, 0, 0, 0);
    }
    __syncthreads();
    if ((chunk - chunk0) % kWgFold == kWgFold - 1) {
      total += acc;
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    }
  }
  if ((chunk1 - chunk0) % kWgFold != 0) total += acc;          // the last, shorter chain

  // register r of lane (half, l31) is row (r & 3) + 8 (r >> 2) + 4 half of the sub-tile at column l31
  const int q = q0 + qsub * 32 + l31;
  if (!mfmaLive || q >= A.Q) return;
  float* __restrict__ dst = A.out + static_cast<size_t>(slice) * static_cast<size_t>(A.N) * A.Q;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int n = n0 + nsub * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
    if (n < A.N) dst[static_cast<size_t>(n) * A.Q + q] = total[r];
  }
}

struct MidasWgradFoldArgs {
  const float* partial;       // [S][total]
  float* out;                 // [total]
  int S;
  long long total;            // N Q
};

inline __global__ __launch_bounds__(kMgThreads) void k_midas_wgrad_fold(MidasWgradFoldArgs A) {
  const long long i = static_cast<long long>(blockIdx.x) * kMgThreads + threadIdx.x;
  if (i >= A.total) return;
  double sum = 0.0;
  for (int s = 0; s < A.S; ++s) sum += static_cast<double>(A.partial[static_cast<size_t>(s) * static_cast<size_t>(A.total) + i]);
  A.out[i] = static_cast<float>(sum);
}

struct MidasBiasGradArgs {
  const float* gy;            // [B][N][H][W]
  float* out;                 // [N]
  int B, N, HW;
};

// workgroup n: thread t sums gy[b][n][t], [t + 256], .. image by image in f64, then a fixed tree over the 256 sums
inline __global__ __launch_bounds__(kMgThreads) void k_midas_bias_grad(MidasBiasGradArgs A) {
  __shared__ double sSum[kMgThreads];
  const int n = static_cast<int>(blockIdx.x), tid = threadIdx.x;
  double sum = 0.0;
  for (int b = 0; b < A.B; ++b) {
    const float* __restrict__ src = A.gy + (static_cast<size_t>(b) * A.N + n) * A.HW;
    for (int i = tid; i < A.HW; i += kMgThreads) sum += static_cast<double>(src[i]);
  }
  sSum[tid] = sum;
  __syncthreads();
  for (int step = kMgThreads / 2; step > 0; step >>= 1) {
    if (tid < step) sSum[tid] += sSum[tid + step];
    __syncthreads();
  }
  if (tid == 0) A.out[n] = static_cast<float>(sSum[0]);
}

struct MidasUpsampleGradArgs {
  const float* gy;            // [planes][2 H][2 W]
  float* out;                 // [planes][H][W]
  int H, W;
  long long total;            // planes H W
};

// The forward's source coordinate of output index d along an axis of n input elements, formed in f32 exactly as k_midas_upsample2x
// (cvd_midas.h) forms it: i0 and i0 + ip are the two inputs output d reads, with the weights l0 and l1.
template <bool ALIGN>
__device__ __forceinline__ void midasUpsampleTaps(int d, int n, int& i0, int& ip, float& l0, float& l1) {
  const int no = 2 * n;
  float s;
  if (ALIGN) {
    const float r = no > 1 ? static_cast<float>(n - 1) / static_cast<float>(no - 1) : 0.f;
    s = r * static_cast<float>(d);
  } else {
    s = (static_cast<float>(d) + 0.5f) * 0.5f - 0.5f;
    s = s < 0.f ? 0.f : s;
  }
  i0 = static_cast<int>(s);
  i0 = i0 > n - 1 ? n - 1 : i0;
  ip = i0 < n - 1 ? 1 : 0;
  l1 = s - static_cast<float>(i0);
  l0 = 1.f - l1;
}

// One thread per INPUT element (iy, ix): the outputs that read it lie in the rows 2 iy - 3 .. 2 iy + 4 and the columns 2 ix - 3 ..
// 2 ix + 4 (both modes: the source coordinate advances by 1/2 resp. (n - 1) / (2 n - 1) in [1/3, 1/2) per output).  Each candidate
// is classified by the forward's own f32 arithmetic; wy[k] = the weight with which output row 2 iy - 3 + k reads input row iy (0: it
// does not; an output on the last input row reads it twice, l0 + l1).  g = sum_k wy[k] (sum_l wx[l] gy[row k][column l]) in the
// order k, l ascending, terms of weight 0 skipped.
template <bool ALIGN>
inline __global__ __launch_bounds__(kMgThreads) void k_midas_upsample2x_grad(MidasUpsampleGradArgs A) {
  const long long i = static_cast<long long>(blockIdx.x) * kMgThreads + threadIdx.x;
  if (i >= A.total) return;
  const int Ho = 2 * A.H, Wo = 2 * A.W;
  const long long row = i / A.W;
  const int ix = static_cast<int>(i - row * A.W);
  const long long plane = row / A.H;
  const int iy = static_cast<int>(row - plane * A.H);
  float wy[8], wx[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    wy[k] = 0.f;
    wx[k] = 0.f;
    const int oy = 2 * iy - 3 + k, ox = 2 * ix - 3 + k;
    int i0, ip;
    float l0, l1;
    if (oy >= 0 && oy < Ho) {
      midasUpsampleTaps<ALIGN>(oy, A.H, i0, ip, l0, l1);
      if (i0 == iy) wy[k] = l0;
      if (i0 + ip == iy) wy[k] = i0 == iy ? l0 + l1 : l1;
    }
    if (ox >= 0 && ox < Wo) {
      midasUpsampleTaps<ALIGN>(ox, A.W, i0, ip, l0, l1);
      if (i0 == ix) wx[k] = l0;
      if (i0 + ip == ix) wx[k] = i0 == ix ? l0 + l1 : l1;
    }
  }
  const float* __restrict__ src = A.gy + static_cast<size_t>(plane) * Ho * Wo;
  float g = 0.f;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    if (wy[k] == 0.f) continue;
    const float* __restrict__ line = src + static_cast<size_t>(2 * iy - 3 + k) * Wo;
    float s = 0.f;
#pragma unroll
    for (int l = 0; l < 8; ++l)
      if (wx[l] != 0.f) s = fmaf(wx[l], line[2 * ix - 3 + l], s);
    g = fmaf(wy[k], s, g);
  }
  A.out[i] = g;
}

// The decoder's training forward saves kMidasSaved tensors for the backward, in this order: 0 .. 3 the layerK_rn results; 4
// refinenet4.resConfUnit2's conv1 result; then for refinenet3, 2, 1 three each: resConfUnit1's conv1 result, the fusion sum
// (resConfUnit2's input), resConfUnit2's conv1 result; 14 output_conv.0's input; 15 output_conv.0's result.  The backward makes at
// most kMidasBackwardStages operator calls.
constexpr int kMidasSaved = 16;
constexpr int kMidasBackwardStages = 48;

constexpr int kHeadMid = 32;           // output_conv.2's channels, the head's only width
constexpr int kHeadSums = kHeadMid + 1;    // gW4[0 .. 31], gb4

struct MidasHeadGradArgs {
  const float* gy;            // [B][H][W]
  const float* y;             // [B][H][W], the head's output (read under nonNegative only)
  const float* t;             // [B][32][H][W] = output_conv.2(x) + bias, before its ReLU, the forward's own f32 values
  const float* w4;            // [32]
  float* g32;                 // [B][32][H][W]
  double* partial;            // [workgroups][33]
  int nonNegative;
  int HW;
  long long M;                // B H W
};

// The forward is y = relu?(b4 + sum_n w4[n] relu(t_n)).  One thread per pixel: g_s = gy [y > 0] under nonNegative (else gy);
// g32[n] = t_n > 0 ? g_s w4[n] : 0 (torch's ReLU: gradient 0 at 0); and the workgroup's share of gW4[n] = sum_p g_s relu(t_n) and
// gb4 = sum_p g_s: products and sums in f64, a fixed xor tree over the wave's lanes, the four waves' sums added in wave order.
inline __global__ __launch_bounds__(kMgThreads) void k_midas_head_grad(MidasHeadGradArgs A) {
  __shared__ double sPart[kMgThreads / 64][kHeadSums];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long p = static_cast<long long>(blockIdx.x) * kMgThreads + tid;
  const bool live = p < A.M;
  float gs = 0.f;
  size_t at = 0;
  if (live) {
    gs = A.gy[p];
    if (A.nonNegative && !(A.y[p] > 0.f)) gs = 0.f;
    const long long img = p / A.HW;
    at = static_cast<size_t>(img) * kHeadMid * A.HW + static_cast<size_t>(p - img * A.HW);
  }
  for (int n = 0; n <= kHeadMid; ++n) {
    double v = 0.0;
    if (n == kHeadMid) {
      v = static_cast<double>(gs);
    } else if (live) {
      const float tn = A.t[at + static_cast<size_t>(n) * A.HW];
      A.g32[at + static_cast<size_t>(n) * A.HW] = tn > 0.f ? gs * A.w4[n] : 0.f;
      v = tn > 0.f ? static_cast<double>(gs) * static_cast<double>(tn) : 0.0;
    }
#pragma unroll
    for (int step = 32; step > 0; step >>= 1) v += __shfl_xor(v, step);
    if (lane == 0) sPart[wave][n] = v;
  }
  __syncthreads();
  if (tid < kHeadSums) {
    double sum = 0.0;
    for (int w = 0; w < kMgThreads / 64; ++w) sum += sPart[w][tid];
    A.partial[static_cast<size_t>(blockIdx.x) * kHeadSums + tid] = sum;
  }
}

struct MidasHeadSumArgs {
  const double* partial;      // [groups][33]
  float* gW4;                 // [32]
  float* gb4;                 // [1]
  int groups;
};

// thread n: the workgroups' sums of entry n in workgroup order, rounded once
inline __global__ __launch_bounds__(64) void k_midas_head_grad_sum(MidasHeadSumArgs A) {
  const int n = threadIdx.x;
  if (n >= kHeadSums) return;
  double sum = 0.0;
  for (int g = 0; g < A.groups; ++g) sum += A.partial[static_cast<size_t>(g) * kHeadSums + n];
  if (n < kHeadMid) A.gW4[n] = static_cast<float>(sum);
  else A.gb4[0] = static_cast<float>(sum);
}

}  // namespace cvd
