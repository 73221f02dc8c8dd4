// The decoder of MiDaS v2.1, f32, forward only: the reference's monodepth/midas_v2/midas_net.py:57-74 behind the
// backbone -- the four layerK_rn convolutions, the four FeatureFusionBlocks of blocks.py:77-159 and the output head -- as one
// convolution template, a fold of its split partial sums, and the bilinear x 2 upsampling.
//
//   k_midas_conv<KS, VEC, HEAD>   KS = filter size (1, 3), stride 1, padding KS / 2.  VEC = the weight chunks are read as float4 (rows
//                                 of Cin KS KS floats that start on 16 bytes), else as single floats.  HEAD = the output head (below).
//   k_midas_fold                  sums the partial sums of a split convolution and applies its epilogue.
//   k_midas_upsample2x<ALIGN>     bilinear x 2 as torch.nn.functional.interpolate, align_corners = ALIGN.
//
// The convolution is k_enc_conv's scheme (cvd_raftenc.h, §3.18; k_raft_conv's, §3.17): an implicit GEMM on the exact f32 MFMA
// (v_mfma_f32_32x32x2_f32: bit for bit a k-ordered fmaf chain), M = B H W pixels (flat), K = Cin KS KS in torch's weight order
// k = (c KS + i) KS + j, N = output channels.  A workgroup (4 waves) owns a 64 pixel x 64 channel tile, wave w the 32 x 32 sub-tile
// (pixels 32 (w & 1), channels 32 (w >> 1)); a wave whose 32 channels all lie past N stages and waits at the barriers but issues no
// MFMA.  Padding: whether tap (i, j) of a pixel lies in the image is decided per PIXEL from its own (row, column), a mask of KS x KS
// bits, so a tile that straddles rows or images reads no neighbour's pixel as halo; every load is unconditional and in range (a tap
// outside reads the pixel's own centre; a channel past Cin the chunk's first channel; a weight past its row's end or past the
// tensor's last row element 0 of the tile's first row; a lane past M pixel 0 of image 0) and is zeroed on its way to the LDS.
// reluIn: the input is rectified on its way to the LDS (the ReLU in front of a ResidualConvUnit's convolutions); the tensor in memory
// is not modified.
//
// Split of K.  The chunks of K (8 channels x 9 taps = 72 for 3 x 3, 32 channels for 1 x 1) are dealt to S slices of chunksPerSlice
// chunks each, chunksPerSlice a multiple of kFold (4 resp. 8), slice s = blockIdx.z.  The host picks S from K and the pixels of ONE
// image alone (midasSplit below: not from the batch, the channel count N or the device), so a batch keeps the bits of its images one
// by one.  Accumulation order of slice s: one fmaf chain per kFold chunks in k order, each folded into a second register set as it
// completes, chains summed in k order, a last shorter chain added last.  With S = 1 the kernel applies the epilogue itself; with
// S > 1 it writes its raw sum to partial s of a scratch tensor [S][B][N][H][W] with plain stores and k_midas_fold sums the S partial
// sums of an element in f64 in the order s = 0 .. S - 1, rounds ONCE to f32 and applies the epilogue.  No atomics: one lane writes
// each element once.
// Epilogue, in this order: t = sum + bias[c] (no bias: t = sum); with relu t = max(t, 0); with an addend a, t = t + (reluA ?
// max(a, 0) : a); with a second addend b, y = b + t.  a is a ResidualConvUnit's rectified input (blocks.py:66-75: its nn.ReLU is in
// place, so `out + x` adds relu(x)), b the other path of FeatureFusionBlock's `output += resConfUnit1(xs[1])`.  Offsets are 64-bit.
//
// HEAD: output_conv.2, its ReLU, output_conv.4 and the last ReLU in one launch.  KS = 3, N = 32; the tile is 128 pixels x 32
// channels, wave w the pixels 32 w, so every wave has MFMA work.  Register r of lane (half, l31) holds channel n = (r & 3) +
// 8 (r >> 2) + 4 half of pixel l31: s = 0; for r = 0 .. 15 in order s = fmaf(max(sum + bias[n], 0), w4[n], s); then y = s(half 0) +
// s(half 1) + b4, rectified under nonNegative, written by the half-0 lane as ONE channel.  The 32-channel tensor is never written.
#pragma once
#include <hip/hip_runtime.h>

namespace cvd {

constexpr int kMidasThreads = 256;
constexpr int kMidasTile = 64;           // output pixels and output channels of a workgroup's tile (the head: 128 x 32)
constexpr int kMidasHeadPixels = 128;
constexpr int kMidasHeadMid = 32;        // output_conv.2's channels, the head's only width
constexpr int kMidasMaxSplit = 32;

template <int KS>
struct MidasShape {
  static_assert(KS == 1 || KS == 3, "filter sizes of the decoder");
  static constexpr int kTaps = KS * KS;
  static constexpr int kChunkChannels = KS == 1 ? 32 : 8;
  static constexpr int kChunkK = kChunkChannels * kTaps;          // 32, 72: even (an MFMA takes two k)
  static constexpr int kFold = KS == 1 ? 8 : 4;                   // chunks per fmaf chain: 256, 288 terms
  static constexpr int kWStride = kChunkK + 1;                    // odd: the 32 weight rows of an operand read fall on distinct banks
};

// The split count of a convolution with K = Cin KS KS over images of HW pixels: as many slices as bring the pixel tiles of one image
// to 64 workgroups per channel tile, each slice whole chains (kFold chunks), at most kMidasMaxSplit.  K and HW alone decide it.
inline int midasSplit(long long K, long long HW, int ks) {
  const int chunkK = ks == 1 ? MidasShape<1>::kChunkK : MidasShape<3>::kChunkK;
  const int fold = ks == 1 ? MidasShape<1>::kFold : MidasShape<3>::kFold;
  const long long chunks = (K + chunkK - 1) / chunkK, chains = (chunks + fold - 1) / fold;
  const long long tiles = (HW + kMidasTile - 1) / kMidasTile;
  long long want = 64 / tiles;
  if (want > kMidasMaxSplit) want = kMidasMaxSplit;
  if (want > chains) want = chains;
  if (want < 1) want = 1;
  const long long per = (chains + want - 1) / want;               // chains per slice
  return static_cast<int>((chains + per - 1) / per);
}

struct MidasConvArgs {
  const float* x;             // [B][Cin][H][W]
  const float* w;             // [N][Cin][KS][KS]
  const float* bias;          // [N] or null
  const float* a;             // or null: [B][N][H][W]
  const float* b;             // or null: [B][N][H][W]
  const float* w4;            // head: output_conv.4's 32 weights and its bias
  const float* b4;
  float* out;                 // [B][N][H][W]; the head: [B][H][W]
  float* partial;             // S > 1: [S][B][N][H][W]
  int reluIn, relu, reluA, nonNegative;
  int Cin, N;
  int H, W, HW;
  int S, chunksPerSlice;
  long long M;                // B H W
};

using midas_f32x16 = __attribute__((ext_vector_type(16))) float;

__device__ __forceinline__ float midasEpilogue(const MidasConvArgs& A, float sum, int n, size_t at) {
  float t = A.bias != nullptr ? sum + A.bias[n] : sum;
  if (A.relu) t = t < 0.f ? 0.f : t;
  if (A.a != nullptr) {
    float av = A.a[at];
    if (A.reluA) av = av < 0.f ? 0.f : av;
    t = t + av;
  }
  if (A.b != nullptr) t = A.b[at] + t;
  return t;
}

template <int KS, bool VEC, bool HEAD>
inline __global__ __launch_bounds__(kMidasThreads) void k_midas_conv(MidasConvArgs A) {
  using S = MidasShape<KS>;
  static_assert(!HEAD || KS == 3, "the head is a 3 x 3 convolution");
  constexpr int T = S::kTaps, CK = S::kChunkK, WS = S::kWStride, R = KS / 2;
  constexpr int TP = HEAD ? kMidasHeadPixels : kMidasTile;      // pixels of the tile
  constexpr int TN = HEAD ? kMidasHeadMid : kMidasTile;         // channels of the tile
  constexpr int PG = kMidasThreads / TP;                        // thread groups that share the tile's pixels and stride over channels
  constexpr int MW = TP / 32;                                   // waves along the pixels
  static_assert(!VEC || CK % 4 == 0, "float4 weight loads need a chunk of whole float4");
  static_assert(S::kChunkChannels % PG == 0, "a chunk's channels are dealt evenly to the groups");
  __shared__ float sPix[CK * TP];             // [c T + t][pixel]
  __shared__ float sW[TN * WS];               // [channel][c T + t]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long m0 = static_cast<long long>(blockIdx.x) * TP;

  // staging: thread = (pixel pl of the tile, group grp); the groups stride over the chunk's channels
  const int pl = tid % TP, grp = tid / TP;
  const long long p = m0 + pl;
  const bool live = p < A.M;
  long long img = 0;
  int pix = 0;
  if (live) {
    img = p / A.HW;
    pix = static_cast<int>(p - img * A.HW);
  }
  const int cy = pix / A.W, cx = pix - cy * A.W;
  unsigned tapIn = 0;
  int tapOff[T];
#pragma unroll
  for (int t = 0; t < T; ++t) {
    const int y = cy + t / KS - R, x = cx + t % KS - R;
    const bool in = live && y >= 0 && y < A.H && x >= 0 && x < A.W;
    if (in) tapIn |= 1u << t;
    tapOff[t] = in ? (t / KS - R) * A.W + (t % KS - R) : 0;
  }
  const float* __restrict__ centre = A.x + static_cast<size_t>(img) * A.Cin * A.HW + static_cast<size_t>(pix);

  const int n0 = static_cast<int>(blockIdx.y) * TN;
  const int Ktot = A.Cin * T;
  const float* __restrict__ wTile = A.w + static_cast<size_t>(n0) * Ktot;
  const int rowsLive = A.N - n0;                         // rows of the tile that exist in the tensor (>= 1)
  const int numChunks = (A.Cin + S::kChunkChannels - 1) / S::kChunkChannels;
  const int slice = static_cast<int>(blockIdx.z);
  const int chunk0 = slice * A.chunksPerSlice;           // (< numChunks: the host's S leaves no empty slice)
  const int chunk1 = chunk0 + A.chunksPerSlice < numChunks ? chunk0 + A.chunksPerSlice : numChunks;

  const int msub = wave % MW, nsub = wave / MW;
  const int half = lane >> 5, l31 = lane & 31;
  const bool mfmaLive = n0 + nsub * 32 < A.N;            // wave-uniform
  const float* opW = sW + (nsub * 32 + l31) * WS + half;          // A operand: lane holds W[row l31][k = half]
  const float* opP = sPix + half * TP + msub * 32 + l31;          // B operand: lane holds P[k = half][column l31]
  midas_f32x16 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  midas_f32x16 total = acc;

  // A chunk travels global -> registers -> LDS: the loads of chunk c + 1 are issued before the MFMA of chunk c and land behind them.
  constexpr int kPerGrp = S::kChunkChannels / PG;    // a group takes the channels grp, grp + PG, .. of the chunk with all their taps
  constexpr int kWPerRow = VEC ? CK / 4 : CK, kWTotal = TN * kWPerRow, kWLoads = (kWTotal + kMidasThreads - 1) / kMidasThreads;
  float pv[kPerGrp * T];
  unsigned pvOk = 0;                                 // bit j = channel grp + PG j of the chunk exists
  float4 wv4[VEC ? kWLoads : 1];
  float wv1[VEC ? 1 : kWLoads];
  const auto load = [&](int chunk) {
    const int cbase = chunk * S::kChunkChannels;
    const float* __restrict__ src = centre + static_cast<size_t>(cbase) * A.HW;
    pvOk = 0;
#pragma unroll
    for (int j = 0; j < kPerGrp; ++j) {
      const int c = grp + PG * j;
      const bool chOk = cbase + c < A.Cin;
      const float* __restrict__ sc = src + static_cast<size_t>(chOk ? c : 0) * A.HW;
#pragma unroll
      for (int t = 0; t < T; ++t) pv[j * T + t] = sc[tapOff[t]];
      if (chOk) pvOk |= 1u << j;
    }
#pragma unroll
    for (int i = 0; i < kWLoads; ++i) {
      const int e = tid + i * kMidasThreads;
      if (kWTotal % kMidasThreads == 0 || e < kWTotal) {
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
  load(chunk0);
  for (int chunk = chunk0; chunk < chunk1; ++chunk) {
#pragma unroll
    for (int j = 0; j < kPerGrp; ++j)
#pragma unroll
      for (int t = 0; t < T; ++t) {
        float v = (((pvOk >> j) & 1u) && ((tapIn >> t) & 1u)) ? pv[j * T + t] : 0.f;
        if (A.reluIn) v = v < 0.f ? 0.f : v;
        sPix[(T * (grp + PG * j) + t) * TP + pl] = v;
      }
#pragma unroll
    for (int i = 0; i < kWLoads; ++i) {
      const int e = tid + i * kMidasThreads;
      if (kWTotal % kMidasThreads == 0 || e < kWTotal) {
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
    if (chunk + 1 < chunk1) load(chunk + 1);
    if (mfmaLive) {
#pragma unroll 8
      for (int kk = 0; kk < CK; kk += 2)
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(opW[kk], opP[kk * TP], acc, 0, 0, 0);
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
  if constexpr (HEAD) {
    float s = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int n = (r & 3) + 8 * (r >> 2) + 4 * half;
      float v = total[r] + A.bias[n];
      v = v < 0.f ? 0.f : v;
      s = fmaf(v, A.w4[n], s);
    }
    const float other = __shfl_xor(s, 32);             // (every lane of the wave is here)
    float y = (half == 0 ? s + other : other + s) + A.b4[0];
    if (A.nonNegative) y = y < 0.f ? 0.f : y;
    if (half == 0 && pe < A.M) A.out[pe] = y;
  } else {
    if (pe >= A.M || !mfmaLive) return;
    const long long imgE = pe / A.HW;
    const size_t at0 = static_cast<size_t>(imgE) * A.N * A.HW + static_cast<size_t>(pe - imgE * A.HW);
    float* __restrict__ dst = A.S > 1 ? A.partial + static_cast<size_t>(slice) * static_cast<size_t>(A.M) * A.N : A.out;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int n = n0 + nsub * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
      if (n < A.N) {
        const size_t at = at0 + static_cast<size_t>(n) * A.HW;
        dst[at] = A.S > 1 ? total[r] : midasEpilogue(A, total[r], n, at);
      }
    }
  }
}

// element i of [B][N][H][W]: the S partial sums in f64 in the order s = 0 .. S - 1, rounded once, then the convolution's epilogue
inline __global__ __launch_bounds__(kMidasThreads) void k_midas_fold(MidasConvArgs A) {
  const long long total = A.M * A.N;
  const long long i = static_cast<long long>(blockIdx.x) * kMidasThreads + threadIdx.x;
  if (i >= total) return;
  double sum = 0.0;
  for (int s = 0; s < A.S; ++s) sum += static_cast<double>(A.partial[static_cast<size_t>(s) * static_cast<size_t>(total) + i]);
  const int n = static_cast<int>((i / A.HW) % A.N);
  A.out[i] = midasEpilogue(A, static_cast<float>(sum), n, static_cast<size_t>(i));
}

struct MidasUpsampleArgs {
  const float* x;             // [planes][H][W]
  float* out;                 // [planes][2 H][2 W]
  int H, W;
  long long total;            // planes 4 H W
};

// One thread per output element.  The source coordinate as torch forms it in f32: align_corners: d (in - 1) / (out - 1), the ratio 0
// where out == 1; else max(0, (d + 0.5) 0.5 - 0.5); i0 = its integer part, i1 = i0 + 1 where that exists, l1 = the fraction,
// l0 = 1 - l1; y = h0 (w0 x00 + w1 x01) + h1 (w0 x10 + w1 x11).
template <bool ALIGN>
inline __global__ __launch_bounds__(kMidasThreads) void k_midas_upsample2x(MidasUpsampleArgs A) {
  const long long i = static_cast<long long>(blockIdx.x) * kMidasThreads + threadIdx.x;
  if (i >= A.total) return;
  const int Ho = 2 * A.H, Wo = 2 * A.W;
  const long long row = i / Wo;
  const int ox = static_cast<int>(i - row * Wo);
  const long long plane = row / Ho;
  const int oy = static_cast<int>(row - plane * Ho);
  float sy, sx;
  if (ALIGN) {
    const float ry = Ho > 1 ? static_cast<float>(A.H - 1) / static_cast<float>(Ho - 1) : 0.f;
    const float rx = Wo > 1 ? static_cast<float>(A.W - 1) / static_cast<float>(Wo - 1) : 0.f;
    sy = ry * static_cast<float>(oy);
    sx = rx * static_cast<float>(ox);
  } else {
    sy = (static_cast<float>(oy) + 0.5f) * 0.5f - 0.5f;
    sx = (static_cast<float>(ox) + 0.5f) * 0.5f - 0.5f;
    sy = sy < 0.f ? 0.f : sy;
    sx = sx < 0.f ? 0.f : sx;
  }
  int y0 = static_cast<int>(sy), x0 = static_cast<int>(sx);
  y0 = y0 > A.H - 1 ? A.H - 1 : y0;
  x0 = x0 > A.W - 1 ? A.W - 1 : x0;
  const int yp = y0 < A.H - 1 ? 1 : 0, xp = x0 < A.W - 1 ? 1 : 0;
  const float h1 = sy - static_cast<float>(y0), h0 = 1.f - h1;
  const float w1 = sx - static_cast<float>(x0), w0 = 1.f - w1;
  const float* __restrict__ src = A.x + static_cast<size_t>(plane) * A.H * A.W + static_cast<size_t>(y0) * A.W + x0;
  const float x00 = src[0], x01 = src[xp], x10 = src[static_cast<size_t>(yp) * A.W], x11 = src[static_cast<size_t>(yp) * A.W + xp];
  A.out[i] = h0 * (w0 * x00 + w1 * x01) + h1 * (w0 * x10 + w1 * x11);
}

}  // namespace cvd
