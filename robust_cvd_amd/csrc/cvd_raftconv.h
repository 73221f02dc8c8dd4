// The stock convolutions of RAFT's update block, f32, forward only: the motion encoder, the flow head and the
// mask head of the reference's BasicUpdateBlock (raft/core/update.py:8-16, 96-114, 133-156) as ONE kernel template, a stride-1,
// "same"-padded, square-filter (1, 3 or 7) convolution as an implicit GEMM on the exact f32 MFMA (v_mfma_f32_32x32x2_f32: bit for
// bit a k-ordered fmaf chain), in the manner of k_gru_gemm (cvd_raftgru.h).
//
//   k_raft_conv<KS, VEC>   KS = filter size; VEC = the weight chunks are read as float4 (the row pitch Cin KS KS and the tensor's
//                          address are multiples of 16 bytes), else as single floats (convf1: rows of 98 floats = 392 bytes).
//
// M = B H W pixels (flat, NCHW), K = Cin x KS x KS in torch's own weight order k = (c KS + i) KS + j, so weight[o] is one
// contiguous row and is read where it lies; N = output channels.  The input is a table of one to three (tensor, first channel,
// tensor's channel count, channels used) segments: no cat is formed.  With several segments each holds a multiple of 32 channels,
// so a chunk (32, 8 or 2 channels: a divisor of 32) lies in one segment; a lone segment may hold any count, the last chunk's
// missing channels are zero-filled in the LDS (pixels and weights), nothing is read past a weight row.  A workgroup (4 waves) owns a
// 64 pixel x 64 channel tile, wave w the 32 x 32 sub-tile (pixels 32 (w & 1), channels 32 (w >> 1)); a wave whose 32 channels all
// lie past N stages and waits at the barriers but issues no MFMA (flow_head.conv2, N = 2).  Up to two weight tensors are stacked
// along N (an N tile lies wholly in one of them: flow_head.conv1 and mask.0 read `net` once).  Padding: whether tap (i, j) of a
// pixel lies in the image is decided per PIXEL from its own (row, column), a 64-bit mask of KS x KS bits, so a tile that straddles
// rows or images of a batch reads no neighbour's pixel as halo; every load is unconditional (a tap outside reads the lane's own
// pixel) and is zeroed on its way to the LDS.  The output is a channel window (first channel, N channels) of a tensor of outC
// channels; channels past N are not written.  Optionally the launch copies a small tensor (flow) into a second window of the same
// output (motion_features = [conv(cor_flo), flow]): the workgroups of the first N tile do it.
// Epilogue: scale * act(sum + bias), act in {none, ReLU}; the scale multiplies last (0.25 * mask(net): a power of two, the same
// bits as a separate multiply).
// Accumulation order: one fmaf chain per kFold chunks in k order (1 x 1: 8 x 32 = 256 terms; 3 x 3: 4 x 72 = 288 terms; 7 x 7:
// 3 x 98 = 294 terms), each folded into a second register set as it completes, chains summed in k order, a last shorter chain
// added last; then the bias.  No atomics, no split of K across workgroups: every output element is written once, by one lane, in a
// fixed order, so results repeat bit for bit and do not depend on how the input is segmented.  Offsets are 64-bit.
#pragma once
#include <hip/hip_runtime.h>

namespace cvd {

constexpr int kConvThreads = 256;
constexpr int kConvTile = 64;            // pixels and output channels of a workgroup's tile
constexpr int kConvMaxSegments = 3;
constexpr int kConvSegmentMultiple = 32; // channel granularity of a segment when there are several

template <int KS>
struct ConvShape {
  static_assert(KS == 1 || KS == 3 || KS == 7, "filter sizes of the update block");
  static constexpr int kTaps = KS * KS;
  static constexpr int kChunkChannels = KS == 1 ? 32 : KS == 3 ? 8 : 2;
  static constexpr int kChunkK = kChunkChannels * kTaps;          // 32, 72, 98: even (an MFMA takes two k)
  static constexpr int kFold = KS == 1 ? 8 : KS == 3 ? 4 : 3;     // chunks per fmaf chain: 256, 288, 294 terms
  static constexpr int kWStride = kChunkK + 1;                    // odd: the 32 weight rows of an operand read fall on distinct banks
  static_assert(kChunkK % 2 == 0 && kConvSegmentMultiple % kChunkChannels == 0, "chunks tile the MFMA's k and the segments");
};

struct ConvSegment {
  const float* p;   // [B][C][H][W]
  int c0, C, n;     // the segment is channels c0 .. c0 + n - 1 of the tensor's C
};

struct ConvArgs {
  ConvSegment seg[kConvMaxSegments];
  int numSeg, Cin;            // Cin = sum of seg[].n
  const float* w[2];          // one weight tensor, or two stacked along N; each [nPer][Cin][KS][KS]
  const float* bias[2];
  int nPer, N;                // output channels per weight tensor, in all (N = nPer or 2 nPer; two only with nPer % 64 == 0)
  float* out;                 // [B][outC][H][W]; channels outC0 .. outC0 + N - 1 are written
  int outC, outC0;
  const float* copySrc;       // or null: [B][copyC][H][W], copied to channels copyC0 .. of out
  int copyC, copyC0;
  float scale;
  int relu;
  long long M;                // B H W
  int HW, H, W;
};

using conv_f32x16 = __attribute__((ext_vector_type(16))) float;

template <int KS, bool VEC>
inline __global__ __launch_bounds__(kConvThreads) void k_raft_conv(ConvArgs A) {
  using S = ConvShape<KS>;
  constexpr int T = S::kTaps, CK = S::kChunkK, WS = S::kWStride, R = KS / 2;
  static_assert(!VEC || CK % 4 == 0, "float4 weight loads need a chunk of whole float4");
  __shared__ float sPix[CK * kConvTile];      // [c T + t][pixel]
  __shared__ float sW[kConvTile * WS];        // [channel][c T + t]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long m0 = static_cast<long long>(blockIdx.x) * kConvTile;

  // staging: lane = pixel of the tile, the waves stride over the chunk's (channel, tap) items
  const long long p = m0 + lane;
  const bool live = p < A.M;
  long long img = 0;
  int pix = 0;
  if (live) {
    img = p / A.HW;
    pix = static_cast<int>(p - img * A.HW);
  }
  const int py = pix / A.W, px = pix - py * A.W;
  unsigned long long tapIn = 0;
#pragma unroll
  for (int t = 0; t < T; ++t) {
    const int y = py + t / KS - R, x = px + t % KS - R;
    if (live && y >= 0 && y < A.H && x >= 0 && x < A.W) tapIn |= 1ull << t;
  }

  const int n0 = static_cast<int>(blockIdx.y) * kConvTile;
  const int gate = n0 >= A.nPer ? 1 : 0;
  const int nLocal0 = n0 - gate * A.nPer;            // the tile's first row in its weight tensor
  const int Ktot = A.Cin * T;
  const float* __restrict__ wTile = (gate ? A.w[1] : A.w[0]) + static_cast<size_t>(nLocal0) * Ktot;
  const int rowsLive = A.nPer - nLocal0;             // rows of the tile that exist in the tensor (>= 1)
  const int numChunks = (A.Cin + S::kChunkChannels - 1) / S::kChunkChannels;

  const int msub = wave & 1, nsub = wave >> 1;
  const int half = lane >> 5, l31 = lane & 31;
  const bool mfmaLive = n0 + nsub * 32 < A.N;        // wave-uniform
  const float* opW = sW + (nsub * 32 + l31) * WS + half;             // A operand: lane holds W[row l31][k = half]
  const float* opP = sPix + half * kConvTile + msub * 32 + l31;      // B operand: lane holds P[k = half][column l31]
  conv_f32x16 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  conv_f32x16 total = acc;

  // A chunk travels global -> registers -> LDS: the loads of chunk c + 1 are issued before the MFMA of chunk c and land behind
  // them.  Every load is unconditional and in range: a tap outside the image reads the lane's own pixel, a channel past Cin the
  // chunk's first channel, a weight past the row's end or the tensor's last row element 0 of the tile's first row (a lane past M
  // reads pixel 0 of image 0); pvOk / the weights' own test zero them on their way to the LDS.
  constexpr int kItems = (CK + 3) / 4;               // (channel, tap) items per wave: item i is e = wave + 4 i, c = e / T, t = e % T
  constexpr int kWPerRow = VEC ? CK / 4 : CK, kWTotal = kConvTile * kWPerRow, kWLoads = (kWTotal + kConvThreads - 1) / kConvThreads;
  // 1 x 1 and 3 x 3: a wave takes the channels wave, wave + 4, .. of the chunk with all their taps (tap offsets are compile-time
  // registers, as in k_gru_gemm); 7 x 7 (two channels a chunk): the 98 items are dealt round the waves.
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
    // the chunk's segment (it lies in one) and its first channel there
    int rel = cbase, sIdx = 0;
    if (A.numSeg > 1 && rel >= A.seg[0].n) {
      rel -= A.seg[0].n;
      sIdx = 1;
      if (A.numSeg > 2 && rel >= A.seg[1].n) {
        rel -= A.seg[1].n;
        sIdx = 2;
      }
    }
    const float* __restrict__ src = A.seg[sIdx].p + (static_cast<size_t>(img) * A.seg[sIdx].C + A.seg[sIdx].c0 + rel) * A.HW + pix;
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
      const int e = tid + i * kConvThreads;
      if (kWTotal % kConvThreads == 0 || e < kWTotal) {
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
          sPix[(T * (wave + 4 * j) + t) * kConvTile + lane] = (((pvOk >> j) & 1u) && ((tapIn >> t) & 1ull)) ? pv[j * T + t] : 0.f;
    } else {
#pragma unroll
      for (int i = 0; i < kItems; ++i) {
        const int e = wave + 4 * i;
        if (CK % 4 == 0 || e < CK) sPix[e * kConvTile + lane] = ((pvOk >> i) & 1u) ? pv[i] : 0.f;
      }
    }
#pragma unroll
    for (int i = 0; i < kWLoads; ++i) {
      const int e = tid + i * kConvThreads;
      if (kWTotal % kConvThreads == 0 || e < kWTotal) {
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
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(opW[kk], opP[kk * kConvTile], acc, 0, 0, 0);
    }
    __syncthreads();
    if (chunk % S::kFold == S::kFold - 1) {
      total += acc;
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    }
  }
  if (numChunks % S::kFold != 0) total += acc;       // the last, shorter chain

  // the copied window (flow into motion_features): the first N tile's workgroups, a pixel per lane of wave 0
  if (A.copySrc != nullptr && blockIdx.y == 0 && wave == 0 && live) {
    for (int c = 0; c < A.copyC; ++c)
      A.out[(static_cast<size_t>(img) * A.outC + A.copyC0 + c) * A.HW + pix] =
          A.copySrc[(static_cast<size_t>(img) * A.copyC + c) * A.HW + pix];
  }

  // epilogue: register r of lane (half, l31) is channel (r & 3) + 8 (r >> 2) + 4 half of the sub-tile at pixel l31
  const long long pe = m0 + msub * 32 + l31;
  if (pe >= A.M || !mfmaLive) return;
  const long long imgE = pe / A.HW;
  const size_t at0 = (static_cast<size_t>(imgE) * A.outC + A.outC0) * A.HW + static_cast<size_t>(pe - imgE * A.HW);
  const float* __restrict__ bias = gate ? A.bias[1] : A.bias[0];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int nl = nsub * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;   // channel of the tile
    if (n0 + nl < A.N) {
      float v = total[r] + bias[nLocal0 + nl];
      if (A.relu) v = v < 0.f ? 0.f : v;
      A.out[at0 + static_cast<size_t>(n0 + nl) * A.HW] = A.scale * v;
    }
  }
}

}  // namespace cvd
