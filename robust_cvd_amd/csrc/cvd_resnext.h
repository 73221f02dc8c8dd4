// The backbone of MiDaS v2.1, f32, forward only: torchvision's ResNet(Bottleneck, blocks, groups, width_per_group)
// in eval mode -- ResNeXt-101 32x8d for the real network -- as three kernel families.
//
//   k_rx_gconv<CG, STRIDE>        the grouped 3 x 3 convolution (Bottleneck.conv2): CG = channels per group (8, 16, 32, 64), any number
//                                 of groups, STRIDE = 1 or 2, padding 1, no bias, with the eval batch norm and an optional ReLU behind it.
//   k_rx_conv<KS, STRIDE, VEC>    the dense convolutions: KS = 7 (the stem, stride 2) or 1 (conv1, conv3, downsample.0; stride 1 or 2),
//                                 padding KS / 2, no bias, the eval batch norm, an optional ReLU, an optional residual, a split of K.
//   k_rx_fold                     sums the partial sums of a split convolution and applies its epilogue.
//   k_rx_maxpool                  nn.MaxPool2d(3, 2, 1): padding counts as minus infinity.
//
// An axis of H gives (H - 1) / STRIDE + 1 outputs for all of them.  Shared rules (those of §3.17-3.19): no atomics, one lane writes
// each output element once, so a call repeats bit for bit; whether a tap of an output pixel lies in the image is decided per PIXEL
// from its own (row, column), so a tile that straddles rows or images reads no neighbour as halo; every load is unconditional and in
// range (a tap outside reads the window's centre (STRIDE y, STRIDE x), which always exists; a lane past M pixel 0 of image 0) and is
// replaced on its way to the arithmetic; offsets are 64-bit.
//
// The grouped convolution is plain v_fma, not MFMA.  A workgroup (4 waves) owns 64 output pixels (flat over B Ho Wo) x 32 output
// channels; wave w owns the 8 channels n0 = 32 blockIdx.y + 8 w .. n0 + 7, which lie in ONE group g = n0 / CG (CG is a multiple
// of 8), lane = pixel.  A lane holds 8 accumulators; for each input channel c of the group it loads its 9 taps once and feeds them
// to all 8 channels, 72 fmaf.  The 8 x 9 weights of that step sit at wave-uniform addresses (the wave index is read through
// readfirstlane), so they travel through the scalar cache and enter the fmaf as scalar operands: no LDS, no barrier, and a wave whose
// channels lie past the tensor leaves at once.  Accumulation order of an output element: one fmaf chain over k = c 9 + t in torch's
// weight order per 32 input channels (288 terms), each chain added to a second register as it completes, so CG = 64 is two chains
// summed in k order.
//
// The dense convolution is k_enc_conv's scheme (§3.18) with k_midas_conv's split (§3.19): an implicit GEMM on the exact f32 MFMA
// (v_mfma_f32_32x32x2_f32: bit for bit a k-ordered fmaf chain), M = B Ho Wo output pixels (flat), K = Cin KS KS in torch's weight
// order, N = output channels; a workgroup owns a 64 x 64 tile, wave w the 32 x 32 sub-tile (pixels 32 (w & 1), channels 32 (w >> 1)).
// The chunks of K (32 channels for 1 x 1, 2 channels x 49 taps for 7 x 7) are dealt to S slices of chunksPerSlice chunks, a multiple
// of kFold (8 resp. 3), slice s = blockIdx.z; one fmaf chain per kFold chunks, chains summed in k order, a last shorter chain last.
// The host picks S from K and the OUTPUT pixels of one image alone (rxSplit below).  With S = 1 the kernel applies the epilogue
// itself; with S > 1 it writes its raw sum to partial s of a scratch tensor [S][B][N][Ho][Wo] and k_rx_fold sums the S partial sums
// of an element in f64 in the order s = 0 .. S - 1, rounds ONCE to f32 and applies the epilogue.
// Epilogue of both convolutions, in this order: with norm vectors y = (sum - mean[c]) / sqrt(var[c] + eps) * gamma[c] + beta[c] (the
// eval batch norm as k_enc_conv writes it, read from the four vectors where they lie); optionally ReLU; with a residual
// y = max(residual + y, 0).
#pragma once
#include <hip/hip_runtime.h>

namespace cvd {

constexpr int kRxThreads = 256;
constexpr int kRxTile = 64;              // output pixels of a workgroup's tile; output channels of the dense tile
constexpr int kRxGroupChannels = 8;      // output channels of a wave of the grouped convolution
constexpr int kRxGroupTileN = 32;        // output channels of its workgroup
constexpr int kRxMaxSplit = 32;

template <int KS>
struct RxShape {
  static_assert(KS == 1 || KS == 7, "filter sizes of the backbone's dense convolutions");
  static constexpr int kTaps = KS * KS;
  static constexpr int kChunkChannels = KS == 1 ? 32 : 2;
  static constexpr int kChunkK = kChunkChannels * kTaps;          // 32, 98: even (an MFMA takes two k)
  static constexpr int kFold = KS == 1 ? 8 : 3;                   // chunks per fmaf chain: 256, 294 terms at most
  static constexpr int kWStride = kChunkK + 1;                    // odd: the 32 weight rows of an operand read fall on distinct banks
};

// The split count of a dense convolution with K = Cin KS KS whose OUTPUT has HWo pixels per image: as many slices as bring the pixel
// tiles of one image to 64 workgroups per channel tile, each slice whole chains (kFold chunks), at most kRxMaxSplit.  K and HWo alone
// decide it: not the batch, the channel count N or the device.
inline int rxSplit(long long K, long long HWo, int ks) {
  const int chunkK = ks == 1 ? RxShape<1>::kChunkK : RxShape<7>::kChunkK;
  const int fold = ks == 1 ? RxShape<1>::kFold : RxShape<7>::kFold;
  const long long chunks = (K + chunkK - 1) / chunkK, chains = (chunks + fold - 1) / fold;
  const long long tiles = (HWo + kRxTile - 1) / kRxTile;
  long long want = 64 / tiles;
  if (want > kRxMaxSplit) want = kRxMaxSplit;
  if (want > chains) want = chains;
  if (want < 1) want = 1;
  const long long per = (chains + want - 1) / want;               // chains per slice
  return static_cast<int>((chains + per - 1) / per);
}

struct RxConvArgs {
  const float* x;             // [B][Cin][H][W]
  const float* w;             // dense: [N][Cin][KS][KS]; grouped: [N][CG][3][3]
  const float* mean;          // or null: the eval batch norm's running_mean, running_var, weight, bias, [N] each
  const float* var;
  const float* gamma;
  const float* beta;
  const float* residual;      // or null: [B][N][Ho][Wo] (dense only)
  float* out;                 // [B][N][Ho][Wo]
  float* partial;             // dense, S > 1: [S][B][N][Ho][Wo]
  float eps;
  int relu;
  int Cin, N;                 // grouped: Cin = N = groups CG
  int H, W, HW;               // the input's
  int Ho, Wo, HWo;            // the output's
  int S, chunksPerSlice;      // dense
  long long M;                // B Ho Wo
};

using rx_f32x16 = __attribute__((ext_vector_type(16))) float;

__device__ __forceinline__ float rxEpilogue(const RxConvArgs& A, float sum, int n, size_t at) {
  float v = sum;
  if (A.mean != nullptr) v = (v - A.mean[n]) / sqrtf(A.var[n] + A.eps) * A.gamma[n] + A.beta[n];
  if (A.relu) v = v < 0.f ? 0.f : v;
  if (A.residual != nullptr) {
    v += A.residual[at];
    v = v < 0.f ? 0.f : v;
  }
  return v;
}

// ---- grouped 3 x 3 ----------------------------------------------------------------------------------------------------------------
template <int CG, int STRIDE>
inline __global__ __launch_bounds__(kRxThreads) void k_rx_gconv(RxConvArgs A) {
  static_assert(CG == 8 || CG == 16 || CG == 32 || CG == 64, "channels per group of the four stages of 32x8d");
  static_assert(STRIDE == 1 || STRIDE == 2, "strides of the backbone");
  constexpr int CO = kRxGroupChannels, T = 9;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6));
  const int n0 = static_cast<int>(blockIdx.y) * kRxGroupTileN + wave * CO;      // wave-uniform
  if (n0 >= A.N) return;                                                        // (no barrier below)
  const int g = n0 / CG;

  const long long p = static_cast<long long>(blockIdx.x) * kRxTile + lane;
  const bool live = p < A.M;
  long long img = 0;
  int pix = 0;
  if (live) {
    img = p / A.HWo;
    pix = static_cast<int>(p - img * A.HWo);
  }
  const int oy = pix / A.Wo, ox = pix - oy * A.Wo;
  const int cy = oy * STRIDE, cx = ox * STRIDE;          // the tap window's centre in the input: always inside the image
  unsigned tapIn = 0;
  int tapOff[T];
#pragma unroll
  for (int t = 0; t < T; ++t) {
    const int y = cy + t / 3 - 1, x = cx + t % 3 - 1;
    const bool in = live && y >= 0 && y < A.H && x >= 0 && x < A.W;
    if (in) tapIn |= 1u << t;
    tapOff[t] = in ? (t / 3 - 1) * A.W + (t % 3 - 1) : 0;
  }
  const float* __restrict__ centre =
      A.x + (static_cast<size_t>(img) * A.N + static_cast<size_t>(g) * CG) * A.HW + static_cast<size_t>(cy) * A.W + cx;
  const float* __restrict__ w = A.w + static_cast<size_t>(n0) * (CG * T);       // rows n0 .. n0 + 7 of [N][CG][9]

  float acc[CO], total[CO];
#pragma unroll
  for (int o = 0; o < CO; ++o) acc[o] = total[o] = 0.f;
  float xv[T], xn[T];
#pragma unroll
  for (int t = 0; t < T; ++t) xn[t] = centre[tapOff[t]];
  for (int c = 0; c < CG; ++c) {
#pragma unroll
    for (int t = 0; t < T; ++t) xv[t] = ((tapIn >> t) & 1u) ? xn[t] : 0.f;
    const float* __restrict__ next = centre + static_cast<size_t>(c + 1 < CG ? c + 1 : c) * A.HW;     // (the last step reloads its own)
#pragma unroll
    for (int t = 0; t < T; ++t) xn[t] = next[tapOff[t]];
    const float* __restrict__ wc = w + c * T;
#pragma unroll
    for (int o = 0; o < CO; ++o)
#pragma unroll
      for (int t = 0; t < T; ++t) acc[o] = fmaf(wc[o * (CG * T) + t], xv[t], acc[o]);
    if (CG > 32 && (c & 31) == 31) {
#pragma unroll
      for (int o = 0; o < CO; ++o) {
        total[o] += acc[o];
        acc[o] = 0.f;
      }
    }
  }
  if (CG <= 32) {
#pragma unroll
    for (int o = 0; o < CO; ++o) total[o] = acc[o];
  }
  if (!live) return;
  const size_t at0 = (static_cast<size_t>(img) * A.N + n0) * A.HWo + static_cast<size_t>(pix);
#pragma unroll
  for (int o = 0; o < CO; ++o) {
    const size_t at = at0 + static_cast<size_t>(o) * A.HWo;
    A.out[at] = rxEpilogue(A, total[o], n0 + o, at);
  }
}

// ---- dense 1 x 1 and 7 x 7 --------------------------------------------------------------------------------------------------------
template <int KS, int STRIDE, bool VEC>
inline __global__ __launch_bounds__(kRxThreads) void k_rx_conv(RxConvArgs A) {
  using S = RxShape<KS>;
  static_assert(STRIDE == 1 || STRIDE == 2, "strides of the backbone");
  constexpr int T = S::kTaps, CK = S::kChunkK, WS = S::kWStride, R = KS / 2;
  static_assert(!VEC || CK % 4 == 0 || KS == 7, "float4 weight loads need a chunk of whole float4");
  __shared__ float sPix[CK * kRxTile];        // [c T + t][pixel]
  __shared__ float sW[kRxTile * WS];          // [channel][c T + t]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long m0 = static_cast<long long>(blockIdx.x) * kRxTile;

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
  const int cy = oy * STRIDE, cx = ox * STRIDE;
  unsigned long long tapIn = 0;
#pragma unroll
  for (int t = 0; t < T; ++t) {
    const int y = cy + t / KS - R, x = cx + t % KS - R;
    if (live && y >= 0 && y < A.H && x >= 0 && x < A.W) tapIn |= 1ull << t;
  }
  const float* __restrict__ centre = A.x + static_cast<size_t>(img) * A.Cin * A.HW + static_cast<size_t>(cy) * A.W + cx;

  const int n0 = static_cast<int>(blockIdx.y) * kRxTile;
  const int Ktot = A.Cin * T;
  const float* __restrict__ wTile = A.w + static_cast<size_t>(n0) * Ktot;
  const int rowsLive = A.N - n0;                         // rows of the tile that exist in the tensor (>= 1)
  const int numChunks = (A.Cin + S::kChunkChannels - 1) / S::kChunkChannels;
  const int slice = static_cast<int>(blockIdx.z);
  const int chunk0 = slice * A.chunksPerSlice;           // (< numChunks: the host's S leaves no empty slice)
  const int chunk1 = chunk0 + A.chunksPerSlice < numChunks ? chunk0 + A.chunksPerSlice : numChunks;

  const int msub = wave & 1, nsub = wave >> 1;
  const int half = lane >> 5, l31 = lane & 31;
  const bool mfmaLive = n0 + nsub * 32 < A.N;            // wave-uniform
  const float* opW = sW + (nsub * 32 + l31) * WS + half;             // A operand: lane holds W[row l31][k = half]
  const float* opP = sPix + half * kRxTile + msub * 32 + l31;        // B operand: lane holds P[k = half][column l31]
  rx_f32x16 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  rx_f32x16 total = acc;

  // A chunk travels global -> registers -> LDS: the loads of chunk c + 1 are issued before the MFMA of chunk c and land behind them.
  // Item i of a wave is e = wave + 4 i of the chunk's CK (channel, tap) pairs, c = e / T, t = e % T.
  constexpr bool kVec = VEC && CK % 4 == 0;          // (7 x 7: chunks of 98 floats are read one by one)
  constexpr int kItems = (CK + 3) / 4;
  constexpr int kWPerRow = kVec ? CK / 4 : CK, kWTotal = kRxTile * kWPerRow, kWLoads = (kWTotal + kRxThreads - 1) / kRxThreads;
  float pv[kItems];
  unsigned pvOk = 0;                                 // bit i = item i is live
  float4 wv4[kVec ? kWLoads : 1];
  float wv1[kVec ? 1 : kWLoads];
  const auto load = [&](int chunk) {
    const int cbase = chunk * S::kChunkChannels;
    const float* __restrict__ src = centre + static_cast<size_t>(cbase) * A.HW;
    pvOk = 0;
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
#pragma unroll
    for (int i = 0; i < kWLoads; ++i) {
      const int e = tid + i * kRxThreads;
      if (kWTotal % kRxThreads == 0 || e < kWTotal) {
        const int n = e / kWPerRow, q = e - n * kWPerRow;
        const int k = chunk * CK + (kVec ? 4 * q : q);
        const bool ok = n < rowsLive && k < Ktot;
        const float* __restrict__ at = wTile + (ok ? static_cast<size_t>(n) * Ktot + k : size_t{0});
        if constexpr (kVec) {
          wv4[i] = *reinterpret_cast<const float4*>(at);
          if (!ok) wv4[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        } else {
          wv1[i] = *at;
          if (!ok) wv1[i] = 0.f;
        }
      }
    }
  };
  load(chunk0);
  for (int chunk = chunk0; chunk < chunk1; ++chunk) {
#pragma unroll
    for (int i = 0; i < kItems; ++i) {
      const int e = wave + 4 * i;
      if (CK % 4 == 0 || e < CK) sPix[e * kRxTile + lane] = ((pvOk >> i) & 1u) ? pv[i] : 0.f;
    }
#pragma unroll
    for (int i = 0; i < kWLoads; ++i) {
      const int e = tid + i * kRxThreads;
      if (kWTotal % kRxThreads == 0 || e < kWTotal) {
        const int n = e / kWPerRow, q = e - n * kWPerRow;
        if constexpr (kVec) {
          float* d = sW + n * WS + 4 * q;
          d[0] = wv4[i].x; d[1] = wv4[i].y; d[2] = wv4[i].z; d[3] = wv4[i].w;
        } else {
          sW[n * WS + q] = wv1[i];
        }
      }
    }
    __syncthreads();
    if (chunk + 1 < chunk1) load(chunk + 1);
    if (mfmaLive) {
#pragma unroll 8
      for (int kk = 0; kk < CK; kk += 2)
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(opW[kk], opP[kk * kRxTile], acc, 0, 0, 0);
    }
    __syncthreads();
    if ((chunk - chunk0) % S::kFold == S::kFold - 1) {
      total += acc;
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    }
  }
  if ((chunk1 - chunk0) % S::kFold != 0) total += acc;       // the last, shorter chain

  // epilogue: register r of lane (half, l31) is channel (r & 3) + 8 (r >> 2) + 4 half of the sub-tile at pixel l31
  const long long pe = m0 + msub * 32 + l31;
  if (pe >= A.M || !mfmaLive) return;
  const long long imgE = pe / A.HWo;
  const size_t at0 = static_cast<size_t>(imgE) * A.N * A.HWo + static_cast<size_t>(pe - imgE * A.HWo);
  float* __restrict__ dst = A.S > 1 ? A.partial + static_cast<size_t>(slice) * static_cast<size_t>(A.M) * A.N : A.out;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int n = n0 + nsub * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
    if (n < A.N) {
      const size_t at = at0 + static_cast<size_t>(n) * A.HWo;
      dst[at] = A.S > 1 ? total[r] : rxEpilogue(A, total[r], n, at);
    }
  }
}

// element i of [B][N][Ho][Wo]: the S partial sums in f64 in the order s = 0 .. S - 1, rounded once, then the convolution's epilogue
inline __global__ __launch_bounds__(kRxThreads) void k_rx_fold(RxConvArgs A) {
  const long long total = A.M * A.N;
  const long long i = static_cast<long long>(blockIdx.x) * kRxThreads + threadIdx.x;
  if (i >= total) return;
  double sum = 0.0;
  for (int s = 0; s < A.S; ++s) sum += static_cast<double>(A.partial[static_cast<size_t>(s) * static_cast<size_t>(total) + i]);
  const int n = static_cast<int>((i / A.HWo) % A.N);
  A.out[i] = rxEpilogue(A, static_cast<float>(sum), n, static_cast<size_t>(i));
}

// ---- max pool 3 x 3, stride 2, padding 1 ------------------------------------------------------------------------------------------
struct RxPoolArgs {
  const float* x;             // [planes][H][W]
  float* out;                 // [planes][Ho][Wo]
  int H, W, Ho, Wo;
  long long total;            // planes Ho Wo
};

// One thread per output element.  A tap outside the image reads the window's centre and counts as minus infinity; a NaN in the
// window is the result, as torch's.
inline __global__ __launch_bounds__(kRxThreads) void k_rx_maxpool(RxPoolArgs A) {
  const long long i = static_cast<long long>(blockIdx.x) * kRxThreads + threadIdx.x;
  if (i >= A.total) return;
  const long long row = i / A.Wo;
  const int ox = static_cast<int>(i - row * A.Wo);
  const long long plane = row / A.Ho;
  const int oy = static_cast<int>(row - plane * A.Ho);
  const int cy = 2 * oy, cx = 2 * ox;
  const float* __restrict__ centre = A.x + static_cast<size_t>(plane) * A.H * A.W + static_cast<size_t>(cy) * A.W + cx;
  float m = -__builtin_inff();
#pragma unroll
  for (int t = 0; t < 9; ++t) {
    const int dy = t / 3 - 1, dx = t % 3 - 1;
    const bool in = cy + dy >= 0 && cy + dy < A.H && cx + dx >= 0 && cx + dx < A.W;
    const float v = centre[in ? dy * A.W + dx : 0];
    if (in && (v > m || v != v)) m = v;
  }
  A.out[i] = m;
}

}  // namespace cvd
