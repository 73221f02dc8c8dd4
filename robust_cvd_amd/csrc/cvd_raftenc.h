// RAFT's feature and context encoders, f32, forward only: the sixteen convolutions of the reference's BasicEncoder
// (raft/core/extractor.py:124-197 with the ResidualBlock of :8-60) as ONE kernel template, and nn.InstanceNorm2d as fnet uses it.
//
//   k_enc_conv<KS, STRIDE, VEC>   KS = filter size (1, 3, 7), STRIDE = 1 or 2, padding KS / 2 (torch's), so an axis of H gives
//                                 (H + 2 (KS / 2) - KS) / STRIDE + 1 = (H - 1) / STRIDE + 1 outputs.  VEC = the weight chunks are
//                                 read as float4 (rows of Cin KS KS floats that start on 16 bytes), else as single floats (conv1:
//                                 rows of 147 floats).
//
// The kernel is k_raft_conv's scheme (cvd_raftconv.h, §3.17) with a stride, one input tensor and a longer epilogue: an implicit GEMM
// on the exact f32 MFMA (v_mfma_f32_32x32x2_f32: bit for bit a k-ordered fmaf chain), M = B Ho Wo OUTPUT pixels (flat), K = Cin KS KS
// in torch's weight order k = (c KS + i) KS + j, N = output channels.  A workgroup (4 waves) owns a 64 pixel x 64 channel tile, wave
// w the 32 x 32 sub-tile (pixels 32 (w & 1), channels 32 (w >> 1)); a wave whose 32 channels all lie past N stages and waits at the
// barriers but issues no MFMA (N = 96: the second channel tile is half dead).  Padding: whether tap (i, j) of an output pixel lies in
// the image is decided per PIXEL from its own (row, column), a 64-bit mask of KS x KS bits, so a tile that straddles rows or images
// reads no neighbour's pixel as halo; every load is unconditional and in range (a tap outside reads the pixel's own centre
// (STRIDE y, STRIDE x), which always exists; a channel past Cin the chunk's first channel; a weight past its row's end or past the
// tensor's last row element 0 of the tile's first row; a lane past M pixel 0 of image 0) and is zeroed on its way to the LDS.
// Accumulation order: one fmaf chain per kFold chunks in k order, each folded into a second register set as it completes, chains
// summed in k order, a last shorter chain added last.  For the encoder's K: 147 = one chain of 147 terms (two chunks of 98, the
// second half zeros); 576 = 288 + 288; 864 = 3 x 288; 1152 = 4 x 288; 64, 96, 128 (1 x 1) = one chain each.
// Epilogue, in this order: y = sum + bias[c]; with norm vectors y = (y - mean[c]) / sqrt(var[c] + eps) * gamma[c] + beta[c] (the eval
// batch norm, read from the four vectors where they lie: no fold launch, no host read); optionally ReLU; with a residual
// y = relu(residual + y).  No atomics, no split of K: one lane writes each output element once.  Offsets are 64-bit.
//
//   k_instnorm_stats   one workgroup per (image, channel) plane: the mean, then the biased variance as the mean of squared deviations
//                      from it, both in f64, each a fixed-order sum (a thread's strided elements in order, then a fixed LDS tree).
//                      Writes (mean, 1 / sqrt(var + eps)) as two doubles per plane.
//   k_instnorm_apply   y = (x - mean) * rstd formed in f64 and rounded once, optional ReLU, optional relu(residual + y); every element
//                      is read and written by one thread, so out may be x.
#pragma once
#include <hip/hip_runtime.h>

namespace cvd {

constexpr int kEncThreads = 256;
constexpr int kEncTile = 64;             // output pixels and output channels of a workgroup's tile

template <int KS>
struct EncShape {
  static_assert(KS == 1 || KS == 3 || KS == 7, "filter sizes of the encoder");
  static constexpr int kTaps = KS * KS;
  static constexpr int kChunkChannels = KS == 1 ? 32 : KS == 3 ? 8 : 2;
  static constexpr int kChunkK = kChunkChannels * kTaps;          // 32, 72, 98: even (an MFMA takes two k)
  static constexpr int kFold = KS == 1 ? 8 : KS == 3 ? 4 : 3;     // chunks per fmaf chain: 256, 288, 294 terms at most
  static constexpr int kWStride = kChunkK + 1;                    // odd: the 32 weight rows of an operand read fall on distinct banks
  static_assert(kChunkK % 2 == 0, "chunks tile the MFMA's k");
};

struct EncConvArgs {
  const float* x;             // [B][Cin][H][W]
  const float* w;             // [N][Cin][KS][KS]
  const float* bias;          // [N]
  const float* mean;          // or null: the eval batch norm's running_mean, running_var, weight, bias, [N] each
  const float* var;
  const float* gamma;
  const float* beta;
  const float* residual;      // or null: [B][N][Ho][Wo]
  float* out;                 // [B][N][Ho][Wo]
  float eps;
  int relu;
  int Cin, N;
  int H, W, HW;               // the input's
  int Ho, Wo, HWo;            // the output's
  long long M;                // B Ho Wo
};

using enc_f32x16 = __attribute__((ext_vector_type(16))) float;

template <int KS, int STRIDE, bool VEC>
inline __global__ __launch_bounds__(kEncThreads) void k_enc_conv(EncConvArgs A) {
  using S = EncShape<KS>;
  static_assert(STRIDE == 1 || STRIDE == 2, "strides of the encoder");
  constexpr int T = S::kTaps, CK = S::kChunkK, WS = S::kWStride, R = KS / 2;
  static_assert(!VEC || CK % 4 == 0, "float4 weight loads need a chunk of whole float4");
  __shared__ float sPix[CK * kEncTile];       // [c T + t][pixel]
  __shared__ float sW[kEncTile * WS];         // [channel][c T + t]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long m0 = static_cast<long long>(blockIdx.x) * kEncTile;

  // staging: lane = output pixel of the tile, the waves stride over the chunk's (channel, tap) items
  const long long p = m0 + lane;
  const bool live = p < A.M;
  long long img = 0;
  int pix = 0;
  if (live) {
    img = p / A.HWo;
    pix = static_cast<int>(p - img * A.HWo);
  }
  const int oy = pix / A.Wo, ox = pix - oy * A.Wo;
  const int cy = oy * STRIDE, cx = ox * STRIDE;          // the tap window's centre in the input: always inside the image
  unsigned long long tapIn = 0;
#pragma unroll
  for (int t = 0; t < T; ++t) {
    const int y = cy + t / KS - R, x = cx + t % KS - R;
    if (live && y >= 0 && y < A.H && x >= 0 && x < A.W) tapIn |= 1ull << t;
  }
  const float* __restrict__ centre = A.x + static_cast<size_t>(img) * A.Cin * A.HW + static_cast<size_t>(cy) * A.W + cx;

  const int n0 = static_cast<int>(blockIdx.y) * kEncTile;
  const int Ktot = A.Cin * T;
  const float* __restrict__ wTile = A.w + static_cast<size_t>(n0) * Ktot;
  const int rowsLive = A.N - n0;                         // rows of the tile that exist in the tensor (>= 1)
  const int numChunks = (A.Cin + S::kChunkChannels - 1) / S::kChunkChannels;

  const int msub = wave & 1, nsub = wave >> 1;
  const int half = lane >> 5, l31 = lane & 31;
  const bool mfmaLive = n0 + nsub * 32 < A.N;            // wave-uniform
  const float* opW = sW + (nsub * 32 + l31) * WS + half;             // A operand: lane holds W[row l31][k = half]
  const float* opP = sPix + half * kEncTile + msub * 32 + l31;       // B operand: lane holds P[k = half][column l31]
  enc_f32x16 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  enc_f32x16 total = acc;

  // A chunk travels global -> registers -> LDS: the loads of chunk c + 1 are issued before the MFMA of chunk c and land behind them.
  constexpr int kItems = (CK + 3) / 4;               // (channel, tap) items per wave: item i is e = wave + 4 i, c = e / T, t = e % T
  constexpr int kWPerRow = VEC ? CK / 4 : CK, kWTotal = kEncTile * kWPerRow, kWLoads = (kWTotal + kEncThreads - 1) / kEncThreads;
  // 1 x 1 and 3 x 3: a wave takes the channels wave, wave + 4, .. of the chunk with all their taps; 7 x 7 (two channels a chunk):
  // the 98 items are dealt round the waves.
  constexpr bool kByChannel = KS != 7;
  constexpr int kPerWave = kByChannel ? S::kChunkChannels / 4 : 1;
  int tapOff[kByChannel ? T : 1];
  if (kByChannel) {
#pragma unroll
    for (int t = 0; t < T; ++t) tapOff[t] = ((tapIn >> t) & 1ull) ? (t / KS - R) * A.W + (t % KS - R) : 0;
  }
  float pv[kByChannel ? kPerWave * T : kItems];
  unsigned pvOk = 0;                                 // by channel: bit j = channel wave + 4 j exists; else bit i = item i is live
  float4 wv4[VEC ? kWLoads : 1];
  float wv1[VEC ? 1 : kWLoads];
  const auto load = [&](int chunk) {
    const int cbase = chunk * S::kChunkChannels;
    const float* __restrict__ src = centre + static_cast<size_t>(cbase) * A.HW;
    pvOk = 0;
    if constexpr (kByChannel) {
#pragma unroll
      for (int j = 0; j < kPerWave; ++j) {
        const int c = wave + 4 * j;
        const bool chOk = cbase + c < A.Cin;
        const float* __restrict__ sc = src + static_cast<size_t>(chOk ? c : 0) * A.HW;
#pragma unroll
        for (int t = 0; t < T; ++t) pv[j * T + t] = sc[tapOff[t]];
        if (chOk) pvOk |= 1u << j;
      }
    } else {
#pragma unroll
      for (int i = 0; i < kItems; ++i) {
        const int e = wave + 4 * i;
        if (CK % 4 == 0 || e < CK) {
          const int c = e / T, t = e - c * T;
          const bool chOk = cbase + c < A.Cin;
          const bool in = (tapIn >> t) & 1ull;
          const int off = in ? (t / KS - R) * A.W + (t % KS - R) : 0;
          pv[i] = src[static_cast<long long>(chOk ? c : 0) * A.HW + off];
          if (in && chOk) pvOk |= 1u << i;
        }
      }
    }
#pragma unroll
    for (int i = 0; i < kWLoads; ++i) {
      const int e = tid + i * kEncThreads;
      if (kWTotal % kEncThreads == 0 || e < kWTotal) {
        const int n = e / kWPerRow, q = e - n * kWPerRow;
        const int k = chunk * CK + (VEC ? 4 * q : q);
        const bool ok = n < rowsLive && k < Ktot;
        const float* __restrict__ at = wTile + (ok ? static_cast<size_t>(n) * Ktot + k : size_t{0});
        if (VEC) {
          wv4[i] = *reinterpret_cast<const float4*>(at);
          if (!ok) wv4[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        } else {
          wv1[i] = *at;
          if (!ok) wv1[i] = 0.f;
        }
      }
    }
  };
  load(0);
  for (int chunk = 0; chunk < numChunks; ++chunk) {
    if constexpr (kByChannel) {
#pragma unroll
      for (int j = 0; j < kPerWave; ++j)
#pragma unroll
        for (int t = 0; t < T; ++t)
          sPix[(T * (wave + 4 * j) + t) * kEncTile + lane] = (((pvOk >> j) & 1u) && ((tapIn >> t) & 1ull)) ? pv[j * T + t] : 0.f;
    } else {
#pragma unroll
      for (int i = 0; i < kItems; ++i) {
        const int e = wave + 4 * i;
        if (CK % 4 == 0 || e < CK) sPix[e * kEncTile + lane] = ((pvOk >> i) & 1u) ? pv[i] : 0.f;
      }
    }
#pragma unroll
    for (int i = 0; i < kWLoads; ++i) {
      const int e = tid + i * kEncThreads;
      if (kWTotal % kEncThreads == 0 || e < kWTotal) {
        const int n = e / kWPerRow, q = e - n * kWPerRow;
        if (VEC) {
          float* d = sW + n * WS + 4 * q;
          d[0] = wv4[i].x; d[1] = wv4[i].y; d[2] = wv4[i].z; d[3] = wv4[i].w;
        } else {
          sW[n * WS + q] = wv1[i];
        }
      }
    }
    __syncthreads();
    if (chunk + 1 < numChunks) load(chunk + 1);
    if (mfmaLive) {
#pragma unroll 8
      for (int kk = 0; kk < CK; kk += 2)
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(opW[kk], opP[kk * kEncTile], acc, 0, 0, 0);
    }
    __syncthreads();
    if (chunk % S::kFold == S::kFold - 1) {
      total += acc;
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    }
  }
  if (numChunks % S::kFold != 0) total += acc;       // the last, shorter chain

  // epilogue: register r of lane (half, l31) is channel (r & 3) + 8 (r >> 2) + 4 half of the sub-tile at pixel l31
  const long long pe = m0 + msub * 32 + l31;
  if (pe >= A.M || !mfmaLive) return;
  const long long imgE = pe / A.HWo;
  const size_t at0 = static_cast<size_t>(imgE) * A.N * A.HWo + static_cast<size_t>(pe - imgE * A.HWo);
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int n = n0 + nsub * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
    if (n < A.N) {
      float v = total[r] + A.bias[n];
      if (A.mean != nullptr) v = (v - A.mean[n]) / sqrtf(A.var[n] + A.eps) * A.gamma[n] + A.beta[n];
      if (A.relu) v = v < 0.f ? 0.f : v;
      const size_t at = at0 + static_cast<size_t>(n) * A.HWo;
      if (A.residual != nullptr) {
        v += A.residual[at];
        v = v < 0.f ? 0.f : v;
      }
      A.out[at] = v;
    }
  }
}

// ---- instance norm ----------------------------------------------------------------------------------------------------------------
constexpr int kNormThreads = 256;

// a fixed tree over the workgroup's 256 partial sums; every thread returns the total
__device__ __forceinline__ double encBlockSum(double v, double* sRed) {
  const int tid = threadIdx.x;
  __syncthreads();                                    // (the previous use of sRed has been read)
  sRed[tid] = v;
  __syncthreads();
#pragma unroll
  for (int s = kNormThreads / 2; s > 0; s >>= 1) {
    if (tid < s) sRed[tid] += sRed[tid + s];
    __syncthreads();
  }
  return sRed[0];
}

struct InstNormArgs {
  const float* x;             // [planes][HW]
  const float* residual;      // or null, like x
  float* out;                 // like x; may be x
  double* stats;              // [planes][2]: mean, 1 / sqrt(var + eps)
  double eps;
  int relu;
  int HW;
  long long total;            // planes HW
};

inline __global__ __launch_bounds__(kNormThreads) void k_instnorm_stats(InstNormArgs A) {
  __shared__ double sRed[kNormThreads];
  const float* __restrict__ x = A.x + static_cast<size_t>(blockIdx.x) * A.HW;
  double s = 0.0;
  for (int i = threadIdx.x; i < A.HW; i += kNormThreads) s += static_cast<double>(x[i]);
  const double mean = encBlockSum(s, sRed) / A.HW;
  double q = 0.0;
  for (int i = threadIdx.x; i < A.HW; i += kNormThreads) {
    const double d = static_cast<double>(x[i]) - mean;
    q += d * d;
  }
  const double var = encBlockSum(q, sRed) / A.HW;
  if (threadIdx.x == 0) {
    A.stats[2 * static_cast<size_t>(blockIdx.x)] = mean;
    A.stats[2 * static_cast<size_t>(blockIdx.x) + 1] = 1.0 / sqrt(var + A.eps);
  }
}

inline __global__ __launch_bounds__(kNormThreads) void k_instnorm_apply(InstNormArgs A) {
  const long long i = static_cast<long long>(blockIdx.x) * kNormThreads + threadIdx.x;
  if (i >= A.total) return;
  const long long plane = i / A.HW;
  const double mean = A.stats[2 * plane], rstd = A.stats[2 * plane + 1];
  float v = static_cast<float>((static_cast<double>(A.x[i]) - mean) * rstd);
  if (A.relu) v = v < 0.f ? 0.f : v;
  if (A.residual != nullptr) {
    v += A.residual[i];
    v = v < 0.f ? 0.f : v;
  }
  A.out[i] = v;
}

}  // namespace cvd
