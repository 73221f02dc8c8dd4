// Training of the MiDaS v2.1 backbone, f32: the batch norm of torchvision's ResNet in training mode and its
// backward, the backward of the grouped 3 x 3 convolution, of the strided 1 x 1 convolution, of the 7 x 7 stem (weights only) and of
// the max pool.  The stride-1 1 x 1 convolutions' gradients are the decoder's (cvd_midas_grad.h), called by the front end.  This
// header includes no other kernel header and shares no type with them.
//
//   k_rxg_norm_stats        per (channel, slice): the f64 sums of x and x^2 over the slice's elements of the channel
//   k_rxg_norm_finish       per channel: the slices' sums added in slice order; mean, invstd = 1 / sqrt(var + eps) rounded ONCE to f32;
//                           the running statistics r = (1 - m) r + m stat (unbiased variance M / (M - 1)); in eval mode mean and
//                           invstd come from the running statistics and nothing else is written
//   k_rxg_norm_apply        y = (c - mean) invstd gamma + beta; optionally ReLU; with a residual max(residual + y, 0)
//   k_rxg_norm_grad_sums    per (channel, slice): the f64 sums of g and g xhat, g = gy [y > 0] where the layer's output y is given,
//                           xhat = (c - mean) invstd formed in f64
//   k_rxg_norm_grad_finish  per channel: gbeta, ggamma = the slices' sums added in slice order, rounded once
//   k_rxg_norm_grad_apply   training: gc = gamma invstd (g - gbeta / M - xhat ggamma / M); eval: gc = g gamma invstd; optionally
//                           g_residual = g.  The mask lives here and in the sums: no masked copy of gy is written.
//   k_rxg_gconv_dgrad<CG, STRIDE>   input gradient of the grouped 3 x 3 convolution, gather form (below)
//   k_rxg_wgrad<KS, STRIDE> weight gradient of a (grouped) KS x KS convolution with padding KS / 2: the grouped 3 x 3 and the stem
//   k_rxg_wgrad_fold        the slices' f64 partial sums of a weight element added in slice order, rounded once
//   k_rxg_gather2           xs[plane][y][x] = x[plane][2 y][2 x]: the input a 1 x 1 convolution of stride 2 reads
//   k_rxg_scatter2          gx[plane][y][x] = (y, x both even ? g[plane][y / 2][x / 2] : 0) (+ add): its input gradient
//   k_rxg_maxpool_grad      backward of nn.MaxPool2d(3, 2, 1) in gather form
//
// Shared rules (§3.17-3.21): no atomics, one lane writes each output element once, so a call repeats bit for bit; every load is
// unconditional and in range (a position outside reads a position that exists and is replaced on its way to the arithmetic); offsets
// are 64-bit; whether a tap lies in the image is decided per pixel from its own (row, column).
//
// Reductions and their order.  A channel's M = B H W elements are numbered m = b HW + pixel.  They are dealt to S slices of
// `perSlice` consecutive elements (a multiple of kRgNormChunk); S = rxgNormSplit(N, M) depends on the two sizes alone.  Within a
// slice thread t of the workgroup adds the elements m0 + t, m0 + t + 256, .. in f64 in that order (the products x x and g xhat are
// formed in f64: exact resp. correctly rounded), the 256 sums are added by a fixed tree in the LDS, and the finish kernel adds the
// S slice sums in the order s = 0 .. S - 1.  The weight gradient deals the M = B Ho Wo output pixels to S slices of whole chains
// of kRgWgradChain pixels, S = rxgWgradSplit(M, elements); a thread owns ONE weight element and adds its slice's pixels in pixel
// order in f64 (products of two f32 are exact in f64); k_rxg_wgrad_fold adds the S partial sums in slice order and rounds once.
//
// The grouped input gradient mirrors k_rx_gconv (cvd_resnext.h): plain v_fma, a lane owns an INPUT pixel, a wave 8 input channels
// of one group; for each of the group's CG output channels it loads the 9 output pixels whose windows contain its pixel once and
// feeds them to its 8 channels, 72 fmaf, with the 8 x 9 weights at wave-uniform addresses (scalar operands): no LDS, no barrier.
// At stride 2 tap (i, j) contributes only where y + 1 - i and x + 1 - j are even; the others are fed as zeros.  An element's sum is
// one fmaf chain over (o, tap) per 32 output channels, chains added in order.
#pragma once
#include <hip/hip_runtime.h>

namespace cvd {

constexpr int kRgThreads = 256;
constexpr int kRgNormChunk = 1024;         // elements of a channel a slice holds at least
constexpr int kRgNormTargetGroups = 1024;  // workgroups the split brings a reduction up to: four for each of the 256 CUs
constexpr int kRgNormMaxSplit = 64;
constexpr int kRgWgradChain = 256;         // output pixels of a chain of the weight gradient
constexpr int kRgWgradMaxSplit = 128;
constexpr int kRgTile = 64;                // input pixels of a workgroup of the grouped input gradient
constexpr int kRgGroupChannels = 8;        // input channels of a wave of it
constexpr int kRgGroupTileN = 32;          // input channels of its workgroup

// The slices per channel of a batch norm reduction over M elements of each of N channels.
inline int rxgNormSplit(long long N, long long M) {
  const long long chunks = (M + kRgNormChunk - 1) / kRgNormChunk;
  long long want = kRgNormTargetGroups / N;
  if (want > kRgNormMaxSplit) want = kRgNormMaxSplit;
  if (want > chunks) want = chunks;
  if (want < 1) want = 1;
  const long long per = (chunks + want - 1) / want;               // chunks per slice
  return static_cast<int>((chunks + per - 1) / per);
}

// The slices of a weight gradient of `elements` weights over M output pixels.
inline int rxgWgradSplit(long long M, long long elements) {
  const long long groups = (elements + kRgThreads - 1) / kRgThreads;
  const long long chains = (M + kRgWgradChain - 1) / kRgWgradChain;
  long long want = kRgNormTargetGroups / groups;
  if (want > kRgWgradMaxSplit) want = kRgWgradMaxSplit;
  if (want > chains) want = chains;
  if (want < 1) want = 1;
  const long long per = (chains + want - 1) / want;               // chains per slice
  return static_cast<int>((chains + per - 1) / per);
}

// ---- batch norm -------------------------------------------------------------------------------------------------------------------
struct RxgNormArgs {
  const float* c;             // [B][N][H][W] the convolution's raw output
  const float* y;             // backward: the layer's output or null; forward: unused
  const float* gy;            // backward: [B][N][H][W]
  const float* gamma;         // [N]
  const float* beta;          // [N] (forward)
  const float* residual;      // forward: or null
  const float* mean;          // apply kernels: [N] the saved mean
  const float* invstd;        // apply kernels: [N]
  const float* gbeta;         // backward apply: [N]
  const float* ggamma;
  float* out;                 // forward: y; backward: gc
  float* outResidual;         // backward: or null
  double* partial;            // [N][S][2]
  int relu, training;
  int N, HW, S;
  long long perSlice;         // elements of a slice
  long long M;                // B HW
  long long total;            // M N
};

// the fixed tree over the workgroup's 256 sums; the result is valid in thread 0
__device__ __forceinline__ double rxgBlockSum(double v, double* s) {
  const int tid = threadIdx.x;
  s[tid] = v;
  __syncthreads();
  for (int step = kRgThreads / 2; step > 0; step >>= 1) {
    if (tid < step) s[tid] += s[tid + step];
    __syncthreads();
  }
  const double r = s[0];
  __syncthreads();
  return r;
}

// grid (S, N)
inline __global__ __launch_bounds__(kRgThreads) void k_rxg_norm_stats(RxgNormArgs A) {
  __shared__ double sSum[kRgThreads];
  const int n = static_cast<int>(blockIdx.y), slice = static_cast<int>(blockIdx.x), tid = threadIdx.x;
  const long long m0 = static_cast<long long>(slice) * A.perSlice;
  const long long m1 = m0 + A.perSlice < A.M ? m0 + A.perSlice : A.M;
  double sum = 0.0, sq = 0.0;
  for (long long m = m0 + tid; m < m1; m += kRgThreads) {
    const long long b = m / A.HW;
    const double v = static_cast<double>(A.c[(static_cast<size_t>(b) * A.N + n) * A.HW + static_cast<size_t>(m - b * A.HW)]);
    sum += v;
    sq += v * v;
  }
  sum = rxgBlockSum(sum, sSum);
  sq = rxgBlockSum(sq, sSum);
  if (tid == 0) {
    double* dst = A.partial + (static_cast<size_t>(n) * A.S + slice) * 2;
    dst[0] = sum;
    dst[1] = sq;
  }
}

struct RxgNormFinishArgs {
  const double* partial;      // [N][S][2] (training)
  float* runningMean;         // [N]: read in eval mode, updated in training mode
  float* runningVar;
  float* mean;                // [N] out
  float* invstd;              // [N] out
  double eps, momentum;
  int training, N, S;
  long long M;
};

inline __global__ __launch_bounds__(kRgThreads) void k_rxg_norm_finish(RxgNormFinishArgs A) {
  const int n = static_cast<int>(blockIdx.x) * kRgThreads + threadIdx.x;
  if (n >= A.N) return;
  if (!A.training) {
    A.mean[n] = A.runningMean[n];
    A.invstd[n] = static_cast<float>(1.0 / sqrt(static_cast<double>(A.runningVar[n]) + A.eps));
    return;
  }
  double sum = 0.0, sq = 0.0;
  for (int s = 0; s < A.S; ++s) {
    sum += A.partial[(static_cast<size_t>(n) * A.S + s) * 2];
    sq += A.partial[(static_cast<size_t>(n) * A.S + s) * 2 + 1];
  }
  const double count = static_cast<double>(A.M);
  const double mean = sum / count;
  double var = sq / count - mean * mean;
  var = var < 0.0 ? 0.0 : var;
  A.mean[n] = static_cast<float>(mean);
  A.invstd[n] = static_cast<float>(1.0 / sqrt(var + A.eps));
  const double unbiased = var * (count / (count - 1.0));
  A.runningMean[n] = static_cast<float>((1.0 - A.momentum) * static_cast<double>(A.runningMean[n]) + A.momentum * mean);
  A.runningVar[n] = static_cast<float>((1.0 - A.momentum) * static_cast<double>(A.runningVar[n]) + A.momentum * unbiased);
}

inline __global__ __launch_bounds__(kRgThreads) void k_rxg_norm_apply(RxgNormArgs A) {
  const long long e = static_cast<long long>(blockIdx.x) * kRgThreads + threadIdx.x;
  if (e >= A.total) return;
  const int n = static_cast<int>((e / A.HW) % A.N);
  float v = (A.c[e] - A.mean[n]) * A.invstd[n] * A.gamma[n] + A.beta[n];
  if (A.relu) v = v < 0.f ? 0.f : v;
  if (A.residual != nullptr) {
    v += A.residual[e];
    v = v < 0.f ? 0.f : v;
  }
  A.out[e] = v;
}

// grid (S, N)
inline __global__ __launch_bounds__(kRgThreads) void k_rxg_norm_grad_sums(RxgNormArgs A) {
  __shared__ double sSum[kRgThreads];
  const int n = static_cast<int>(blockIdx.y), slice = static_cast<int>(blockIdx.x), tid = threadIdx.x;
  const long long m0 = static_cast<long long>(slice) * A.perSlice;
  const long long m1 = m0 + A.perSlice < A.M ? m0 + A.perSlice : A.M;
  const double mean = static_cast<double>(A.mean[n]), invstd = static_cast<double>(A.invstd[n]);
  double sg = 0.0, sgx = 0.0;
  for (long long m = m0 + tid; m < m1; m += kRgThreads) {
    const long long b = m / A.HW;
    const size_t at = (static_cast<size_t>(b) * A.N + n) * A.HW + static_cast<size_t>(m - b * A.HW);
    float g = A.gy[at];
    if (A.y != nullptr) g = A.y[at] > 0.f ? g : 0.f;
    const double xhat = (static_cast<double>(A.c[at]) - mean) * invstd;
    sg += static_cast<double>(g);
    sgx += static_cast<double>(g) * xhat;
  }
  sg = rxgBlockSum(sg, sSum);
  sgx = rxgBlockSum(sgx, sSum);
  if (tid == 0) {
    double* dst = A.partial + (static_cast<size_t>(n) * A.S + slice) * 2;
    dst[0] = sg;
    dst[1] = sgx;
  }
}

struct RxgNormGradFinishArgs {
  const double* partial;      // [N][S][2]
  float* gbeta;               // [N]
  float* ggamma;
  int N, S;
};

inline __global__ __launch_bounds__(kRgThreads) void k_rxg_norm_grad_finish(RxgNormGradFinishArgs A) {
  const int n = static_cast<int>(blockIdx.x) * kRgThreads + threadIdx.x;
  if (n >= A.N) return;
  double sg = 0.0, sgx = 0.0;
  for (int s = 0; s < A.S; ++s) {
    sg += A.partial[(static_cast<size_t>(n) * A.S + s) * 2];
    sgx += A.partial[(static_cast<size_t>(n) * A.S + s) * 2 + 1];
  }
  A.gbeta[n] = static_cast<float>(sg);
  A.ggamma[n] = static_cast<float>(sgx);
}

inline __global__ __launch_bounds__(kRgThreads) void k_rxg_norm_grad_apply(RxgNormArgs A) {
  const long long e = static_cast<long long>(blockIdx.x) * kRgThreads + threadIdx.x;
  if (e >= A.total) return;
  const int n = static_cast<int>((e / A.HW) % A.N);
  float g = A.gy[e];
  if (A.y != nullptr) g = A.y[e] > 0.f ? g : 0.f;
  const float k = A.gamma[n] * A.invstd[n];
  float r;
  if (A.training) {
    const double count = static_cast<double>(A.M);
    const float mb = static_cast<float>(static_cast<double>(A.gbeta[n]) / count);
    const float mg = static_cast<float>(static_cast<double>(A.ggamma[n]) / count);
    const float xhat = (A.c[e] - A.mean[n]) * A.invstd[n];
    r = k * (g - mb - xhat * mg);
  } else {
    r = g * k;
  }
  A.out[e] = r;
  if (A.outResidual != nullptr) A.outResidual[e] = g;
}

// ---- grouped 3 x 3: input gradient --------------------------------------------------------------------------------------------------
struct RxgConvArgs {
  const float* gy;            // [B][N][Ho][Wo]
  const float* x;             // weight gradient: [B][Cin][H][W]
  const float* w;             // input gradient: [N][CG][3][3]
  float* out;                 // input gradient: gx [B][Cin][H][W]
  double* partial;            // weight gradient: [S][elements]
  int Cin, N;                 // grouped: Cin = N = groups CG
  int CG, NG;                 // input and output channels of a group
  int H, W, HW, Ho, Wo, HWo;
  long long chainsPerSlice;   // weight gradient
  long long M;                // input gradient: B H W; weight gradient: B Ho Wo
  long long elements;         // weight gradient: N CG KS KS
};

template <int CG, int STRIDE>
inline __global__ __launch_bounds__(kRgThreads) void k_rxg_gconv_dgrad(RxgConvArgs A) {
  static_assert(CG == 8 || CG == 16 || CG == 32 || CG == 64, "channels per group of the four stages of 32x8d");
  static_assert(STRIDE == 1 || STRIDE == 2, "strides of the backbone");
  constexpr int CI = kRgGroupChannels, T = 9;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6));
  const int c0 = static_cast<int>(blockIdx.y) * kRgGroupTileN + wave * CI;      // wave-uniform
  if (c0 >= A.Cin) return;                                                      // (no barrier below)
  const int g = c0 / CG, cl0 = c0 - g * CG;

  const long long p = static_cast<long long>(blockIdx.x) * kRgTile + lane;
  const bool live = p < A.M;
  long long img = 0;
  int pix = 0;
  if (live) {
    img = p / A.HW;
    pix = static_cast<int>(p - img * A.HW);
  }
  const int iy = pix / A.W, ix = pix - iy * A.W;
  // tap (i, j): the output pixel (oy, ox) with STRIDE oy + i - 1 = iy, STRIDE ox + j - 1 = ix, where there is one
  unsigned tapIn = 0;
  int tapOff[T];
#pragma unroll
  for (int t = 0; t < T; ++t) {
    const int ny = iy + 1 - t / 3, nx = ix + 1 - t % 3;
    const int oy = ny / STRIDE, ox = nx / STRIDE;
    const bool in = live && ny >= 0 && nx >= 0 && ny % STRIDE == 0 && nx % STRIDE == 0 && oy < A.Ho && ox < A.Wo;
    if (in) tapIn |= 1u << t;
    tapOff[t] = in ? oy * A.Wo + ox : 0;
  }
  const float* __restrict__ base = A.gy + (static_cast<size_t>(img) * A.N + static_cast<size_t>(g) * CG) * A.HWo;
  const float* __restrict__ w = A.w + (static_cast<size_t>(g) * CG * CG + cl0) * T;     // W[g CG + o][cl0 + k][t] = w[(o CG + k) 9 + t]

  float acc[CI], total[CI];
#pragma unroll
  for (int k = 0; k < CI; ++k) acc[k] = total[k] = 0.f;
  for (int o = 0; o < CG; ++o) {
    const float* __restrict__ src = base + static_cast<size_t>(o) * A.HWo;
    float gv[T];
#pragma unroll
    for (int t = 0; t < T; ++t) {
      const float v = src[tapOff[t]];
      gv[t] = ((tapIn >> t) & 1u) ? v : 0.f;
    }
    const float* __restrict__ wo = w + static_cast<size_t>(o) * (CG * T);
#pragma unroll
    for (int k = 0; k < CI; ++k)
#pragma unroll
      for (int t = 0; t < T; ++t) acc[k] = fmaf(wo[k * T + t], gv[t], acc[k]);
    if (CG > 32 && (o & 31) == 31) {
#pragma unroll
      for (int k = 0; k < CI; ++k) {
        total[k] += acc[k];
        acc[k] = 0.f;
      }
    }
  }
  if (CG <= 32) {
#pragma unroll
    for (int k = 0; k < CI; ++k) total[k] = acc[k];
  }
  if (!live) return;
  const size_t at0 = (static_cast<size_t>(img) * A.Cin + c0) * A.HW + static_cast<size_t>(pix);
#pragma unroll
  for (int k = 0; k < CI; ++k) A.out[at0 + static_cast<size_t>(k) * A.HW] = total[k];
}

// ---- weight gradient of a (grouped) KS x KS convolution, padding KS / 2 ------------------------------------------------------------
// grid (ceil(elements / 256), S).  Thread = weight element e = (o CG + c) KS KS + tap of [N][CG][KS][KS]; output channel o reads the
// input channels of its group o / NG.  The pixel loop is uniform over the workgroup.
template <int KS, int STRIDE>
inline __global__ __launch_bounds__(kRgThreads) void k_rxg_wgrad(RxgConvArgs A) {
  static_assert(KS == 3 || KS == 7, "the grouped 3 x 3 and the stem");
  static_assert(STRIDE == 1 || STRIDE == 2, "strides of the backbone");
  constexpr int T = KS * KS, R = KS / 2;
  const long long e = static_cast<long long>(blockIdx.x) * kRgThreads + threadIdx.x;
  if (e >= A.elements) return;                                                  // (no barrier below)
  const int slice = static_cast<int>(blockIdx.y);
  const int t = static_cast<int>(e % T);
  const long long oc = e / T;
  const int c = static_cast<int>(oc % A.CG), o = static_cast<int>(oc / A.CG);
  const int ci = (o / A.NG) * A.CG + c;
  const int di = t / KS - R, dj = t % KS - R;
  const long long p0 = static_cast<long long>(slice) * A.chainsPerSlice * kRgWgradChain;
  const long long p1 = p0 + A.chainsPerSlice * kRgWgradChain < A.M ? p0 + A.chainsPerSlice * kRgWgradChain : A.M;
  long long img = p0 / A.HWo;
  int pix = static_cast<int>(p0 - img * A.HWo);
  int oy = pix / A.Wo, ox = pix - oy * A.Wo;
  double sum = 0.0;
  for (long long p = p0; p < p1; ++p) {
    const int cy = oy * STRIDE, cx = ox * STRIDE;        // the window's centre: always inside the image
    const int y = cy + di, x = cx + dj;
    const bool in = y >= 0 && y < A.H && x >= 0 && x < A.W;
    const float gv = A.gy[(static_cast<size_t>(img) * A.N + o) * A.HWo + static_cast<size_t>(oy) * A.Wo + ox];
    const float xv = A.x[(static_cast<size_t>(img) * A.Cin + ci) * A.HW + static_cast<size_t>(in ? y : cy) * A.W + (in ? x : cx)];
    sum += static_cast<double>(gv) * static_cast<double>(in ? xv : 0.f);
    if (++ox == A.Wo) {
      ox = 0;
      if (++oy == A.Ho) {
        oy = 0;
        ++img;
      }
    }
  }
  A.partial[static_cast<size_t>(slice) * static_cast<size_t>(A.elements) + static_cast<size_t>(e)] = sum;
}

struct RxgFoldArgs {
  const double* partial;      // [S][total]
  float* out;                 // [total]
  int S;
  long long total;
};

inline __global__ __launch_bounds__(kRgThreads) void k_rxg_wgrad_fold(RxgFoldArgs A) {
  const long long i = static_cast<long long>(blockIdx.x) * kRgThreads + threadIdx.x;
  if (i >= A.total) return;
  double sum = 0.0;
  for (int s = 0; s < A.S; ++s) sum += A.partial[static_cast<size_t>(s) * static_cast<size_t>(A.total) + i];
  A.out[i] = static_cast<float>(sum);
}

// ---- 1 x 1 at stride 2 ---------------------------------------------------------------------------------------------------------------
struct RxgStrideArgs {
  const float* in;            // gather: x [planes][H][W]; scatter: g [planes][Ho][Wo]
  const float* add;           // scatter: or null, [planes][H][W]
  float* out;                 // gather: [planes][Ho][Wo]; scatter: [planes][H][W]
  int H, W, Ho, Wo;
  long long total;            // the output's elements
};

inline __global__ __launch_bounds__(kRgThreads) void k_rxg_gather2(RxgStrideArgs A) {
  const long long i = static_cast<long long>(blockIdx.x) * kRgThreads + threadIdx.x;
  if (i >= A.total) return;
  const long long row = i / A.Wo;
  const int ox = static_cast<int>(i - row * A.Wo);
  const long long plane = row / A.Ho;
  const int oy = static_cast<int>(row - plane * A.Ho);
  A.out[i] = A.in[static_cast<size_t>(plane) * A.H * A.W + static_cast<size_t>(2 * oy) * A.W + 2 * ox];
}

inline __global__ __launch_bounds__(kRgThreads) void k_rxg_scatter2(RxgStrideArgs A) {
  const long long i = static_cast<long long>(blockIdx.x) * kRgThreads + threadIdx.x;
  if (i >= A.total) return;
  const long long row = i / A.W;
  const int x = static_cast<int>(i - row * A.W);
  const long long plane = row / A.H;
  const int y = static_cast<int>(row - plane * A.H);
  const float v = A.in[static_cast<size_t>(plane) * A.Ho * A.Wo + static_cast<size_t>(y >> 1) * A.Wo + (x >> 1)];
  float r = ((y | x) & 1) ? 0.f : v;
  if (A.add != nullptr) r = r + A.add[i];
  A.out[i] = r;
}

// ---- max pool 3 x 3, stride 2, padding 1: backward ---------------------------------------------------------------------------------
struct RxgPoolArgs {
  const float* x;             // [planes][H][W]
  const float* gy;            // [planes][Ho][Wo]
  float* out;                 // [planes][H][W]
  int H, W, Ho, Wo;
  long long total;            // planes H W
};

// One thread per INPUT element (y, x).  The windows that contain it are oy in {y / 2} (y even) or {(y - 1) / 2, (y + 1) / 2} (y odd),
// likewise ox: at most 2 x 2, visited in ascending (oy, ox).  Each window's argmax is recomputed as torch forms it: a row-major scan
// of the window's positions inside the image, starting at the first of them, replaced on val > max || isnan(val), so the first
// maximum wins; gy of the window is added where the argmax is (y, x).
inline __global__ __launch_bounds__(kRgThreads) void k_rxg_maxpool_grad(RxgPoolArgs A) {
  const long long i = static_cast<long long>(blockIdx.x) * kRgThreads + threadIdx.x;
  if (i >= A.total) return;
  const long long row = i / A.W;
  const int x = static_cast<int>(i - row * A.W);
  const long long plane = row / A.H;
  const int y = static_cast<int>(row - plane * A.H);
  const float* __restrict__ src = A.x + static_cast<size_t>(plane) * A.H * A.W;
  const float* __restrict__ gsrc = A.gy + static_cast<size_t>(plane) * A.Ho * A.Wo;
  const int oy0 = y >> 1, ox0 = x >> 1;                  // the first window of each axis ((y - 1) / 2 for odd y, y / 2 for even)
  const int ny = (y & 1) + 1, nx = (x & 1) + 1;
  float g = 0.f;
#pragma unroll
  for (int a = 0; a < 2; ++a) {
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const int oy = oy0 + a, ox = ox0 + b;
      const bool window = a < ny && b < nx && oy < A.Ho && ox < A.Wo;
      const int wy = window ? oy : oy0, wx = window ? ox : ox0;      // (oy0 < Ho and ox0 < Wo always)
      const int cy = 2 * wy, cx = 2 * wx;
      float m = -__builtin_inff();
      int arg = -1;
#pragma unroll
      for (int t = 0; t < 9; ++t) {
        const int py = cy + t / 3 - 1, px = cx + t % 3 - 1;
        const bool in = py >= 0 && py < A.H && px >= 0 && px < A.W;
        const float v = src[static_cast<size_t>(in ? py : cy) * A.W + (in ? px : cx)];
        if (in && (arg < 0 || v > m || v != v)) {
          m = v;
          arg = py * A.W + px;
        }
      }
      const float gv = gsrc[static_cast<size_t>(wy) * A.Wo + wx];
      if (window && arg == y * A.W + x) g += gv;
    }
  }
  A.out[i] = g;
}

}  // namespace cvd
