// The recurrent core of RAFT's update block, f32, forward only: SepConvGRU(hidden 128, input 256) of the
// reference (raft/core/update.py:37-75) as an implicit GEMM on the exact f32 MFMA (v_mfma_f32_32x32x2_f32: bit for bit a k-ordered
// fmaf chain).  Per half (1 x 5 along a row, then 5 x 1 along a column):
//
//   z = sigmoid(conv_z([h, x]))   r = sigmoid(conv_r([h, x]))   q = tanh(conv_q([r h, x]))   h' = (1 - z) h + z q
//
//   k_gru_gemm<false>   launch one of a half: N = 256 output channels (z and r stacked; an N tile lies in one of the two weight
//                       tensors), epilogue stores sigmoid(z) and sigmoid(r) h.
//   k_gru_gemm<true>    launch two: N = 128, the first 128 input channels are r h, epilogue tanh and the gate, writes the new h.
//
// M = B H W pixels (flat, NCHW: a channel's pixels are contiguous), K = 384 channels x 5 taps in torch's own weight order
// k = 5 c + t, so weight[o] is a row of 1920 contiguous floats and is read where it lies.  No cat: the 384 input channels are
// twelve 32-channel blocks, each a (tensor, first channel, tensor's channel count) entry of a table the host fills from h (or r h)
// and the one to three tensors of x.  A workgroup (4 waves) owns a 64 pixel x 64 channel tile; wave w the 32 x 32 sub-tile (pixels
// 32 (w & 1), channels 32 (w >> 1)).  K runs in 24 chunks of 16 channels x 5 taps: the chunk's shifted pixels (im2col: element
// (5 c + t, pixel) = the pixel t - 2 further along the half's axis, zero outside the row resp. image -- decided per PIXEL, so a tile
// that straddles rows or images of a batch reads no neighbour's pixels as halo) and the chunk's 64 x 80 weights are staged in LDS
// (40.25 KiB), then 40 MFMA per wave; the next chunk's global loads are in flight meanwhile (registers).  The weights are the
// MFMA's A operand and the pixels its B operand, so an accumulator
// register holds 32 consecutive pixels of one output channel across a half wave: the epilogue's loads and stores are 128-byte rows.
// Accumulation order: one fmaf chain per 4 chunks (320 terms), folded into a second register set: six chains, summed in order
// (DESIGN.md §3.16 has the error figures behind that choice).  No atomics, no split of K across workgroups: every output element is
// written once, by one lane, in a fixed operation order, so results repeat bit for bit and do not depend on how x is segmented.
// Activations are expf / tanhf and an IEEE division: 1 / (1 + expf(-v)) is exactly 0 at v = -100 (expf overflows to +inf) and exactly
// 1 at v = 100.  Offsets are 64-bit.
#pragma once
#include <hip/hip_runtime.h>

namespace cvd {

constexpr int kGruHidden = 128;
constexpr int kGruInput = 256;
constexpr int kGruTaps = 5;
constexpr int kGruK = (kGruHidden + kGruInput) * kGruTaps;   // 1920: a weight row
constexpr int kGruThreads = 256;
constexpr int kGruTile = 64;                                 // pixels and output channels of a workgroup's tile
constexpr int kGruBlockChannels = 32;                        // granularity of the channel-segment table
constexpr int kGruBlocks = (kGruHidden + kGruInput) / kGruBlockChannels;   // 12
constexpr int kGruMaxSegments = 3;                           // tensors of x
constexpr int kGruChunkChannels = 16;
constexpr int kGruChunkK = kGruChunkChannels * kGruTaps;     // 80
constexpr int kGruChunks = (kGruHidden + kGruInput) / kGruChunkChannels;   // 24
constexpr int kGruFoldChunks = 4;                            // chunks per fmaf chain (320 terms)
constexpr int kGruWStride = kGruChunkK + 1;                  // odd: the 32 weight rows of an operand read fall on distinct banks

static_assert(kGruChunks % kGruFoldChunks == 0 && kGruBlockChannels % kGruChunkChannels == 0, "chunks tile the blocks and the chains");

struct GruBlock {
  const float* p;   // [B][C][H][W]
  int c0, C;        // this block is channels c0 .. c0 + 31 of the tensor's C
};

struct GruArgs {
  GruBlock blk[kGruBlocks];   // blocks 0..3: h (launch one) or r h (launch two); 4..11: x
  const float* w[2];          // launch one: convz, convr; launch two: convq, -- ; each [128][384][5]
  const float* bias[2];
  const float* h;             // [B][128][H][W] the half's incoming state
  const float* z;             // launch two: sigmoid(z) of launch one
  float* zOut;                // launch one
  float* rhOut;
  float* out;                 // launch two: the half's new state
  long long M;                // B H W
  int HW, W;
  int len, stride, vertical;  // the half's axis: its length, the pixel step along it, 0 = along a row
};

using gru_f32x16 = __attribute__((ext_vector_type(16))) float;

template <bool Q>
inline __global__ __launch_bounds__(kGruThreads) void k_gru_gemm(GruArgs A) {
  __shared__ float sPix[kGruChunkK * kGruTile];      // [5 c + t][pixel]
  __shared__ float sW[kGruTile * kGruWStride];       // [channel][5 c + t]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long m0 = static_cast<long long>(blockIdx.x) * kGruTile;

  // staging: lane = pixel of the tile, wave strides over the chunk's channels
  const long long p = m0 + lane;
  const bool live = p < A.M;
  long long img = 0;
  int pix = 0;
  if (live) {
    img = p / A.HW;
    pix = static_cast<int>(p - img * A.HW);
  }
  const int pos = A.vertical ? pix / A.W : pix % A.W;
  unsigned tapIn = 0;
#pragma unroll
  for (int t = 0; t < kGruTaps; ++t)
    if (live && pos + t - 2 >= 0 && pos + t - 2 < A.len) tapIn |= 1u << t;

  const int gate = Q ? 0 : static_cast<int>(blockIdx.y >> 1);
  const int n0 = Q ? static_cast<int>(blockIdx.y) * kGruTile : static_cast<int>(blockIdx.y & 1) * kGruTile;
  const float* __restrict__ wTile = A.w[gate] + static_cast<size_t>(n0) * kGruK;

  const int msub = wave & 1, nsub = wave >> 1;
  const int half = lane >> 5, l31 = lane & 31;
  const float* opW = sW + (nsub * 32 + l31) * kGruWStride + half;    // A operand: lane holds W[row l31][k = half]
  const float* opP = sPix + half * kGruTile + msub * 32 + l31;       // B operand: lane holds P[k = half][column l31]
  gru_f32x16 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  gru_f32x16 total = acc;

  // A chunk travels global -> registers -> LDS: the loads of chunk c + 1 are issued before the MFMA of chunk c and land behind
  // them.  Every load is unconditional: a tap outside the row / image reads the lane's own pixel instead (always in range; a lane
  // past M reads pixel 0 of image 0) and is zeroed on its way to the LDS.
  constexpr int kPerWave = kGruChunkChannels / 4, kW4 = kGruChunkK / 4, kWLoads = kGruTile * kW4 / kGruThreads;
  static_assert(kGruTile * kW4 % kGruThreads == 0, "the weight chunk divides among the threads");
  long long tapOff[kGruTaps];
#pragma unroll
  for (int t = 0; t < kGruTaps; ++t) tapOff[t] = ((tapIn >> t) & 1u) ? static_cast<long long>(t - 2) * A.stride : 0ll;
  float pv[kPerWave][kGruTaps];
  float4 wv[kWLoads];
  const auto load = [&](int chunk) {
    const int b = chunk / (kGruBlockChannels / kGruChunkChannels);
    const int c0 = A.blk[b].c0 + (chunk % (kGruBlockChannels / kGruChunkChannels)) * kGruChunkChannels;
    const float* __restrict__ src = A.blk[b].p + (static_cast<size_t>(img) * A.blk[b].C + c0) * A.HW + pix;
#pragma unroll
    for (int j = 0; j < kPerWave; ++j) {
      const float* __restrict__ s = src + static_cast<size_t>(wave + 4 * j) * A.HW;
#pragma unroll
      for (int t = 0; t < kGruTaps; ++t) pv[j][t] = s[tapOff[t]];
    }
    // the chunk's weights: 64 rows of 80 contiguous floats (16-byte aligned: the host checks the tensors)
#pragma unroll
    for (int i = 0; i < kWLoads; ++i) {
      const int e = tid + i * kGruThreads, n = e / kW4, q4 = e - n * kW4;
      wv[i] = *reinterpret_cast<const float4*>(wTile + static_cast<size_t>(n) * kGruK + chunk * kGruChunkK + q4 * 4);
    }
  };
  load(0);
  for (int chunk = 0; chunk < kGruChunks; ++chunk) {
#pragma unroll
    for (int j = 0; j < kPerWave; ++j)
#pragma unroll
      for (int t = 0; t < kGruTaps; ++t)
        sPix[(kGruTaps * (wave + 4 * j) + t) * kGruTile + lane] = ((tapIn >> t) & 1u) ? pv[j][t] : 0.f;
#pragma unroll
    for (int i = 0; i < kWLoads; ++i) {
      const int e = tid + i * kGruThreads, n = e / kW4, q4 = e - n * kW4;
      float* d = sW + n * kGruWStride + q4 * 4;
      d[0] = wv[i].x; d[1] = wv[i].y; d[2] = wv[i].z; d[3] = wv[i].w;
    }
    __syncthreads();
    if (chunk + 1 < kGruChunks) load(chunk + 1);
#pragma unroll 8
    for (int kk = 0; kk < kGruChunkK; kk += 2)
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(opW[kk], opP[kk * kGruTile], acc, 0, 0, 0);
    __syncthreads();
    if (chunk % kGruFoldChunks == kGruFoldChunks - 1) {
      total += acc;
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    }
  }

  // epilogue: register r of lane (half, l31) is channel (r & 3) + 8 (r >> 2) + 4 half of the sub-tile at pixel l31
  const long long pe = m0 + msub * 32 + l31;
  if (pe >= A.M) return;
  const long long imgE = pe / A.HW;
  const size_t at0 = static_cast<size_t>(imgE) * kGruHidden * A.HW + static_cast<size_t>(pe - imgE * A.HW);
  const float* __restrict__ bias = A.bias[gate];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int n = n0 + nsub * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
    const size_t at = at0 + static_cast<size_t>(n) * A.HW;
    const float v = total[r] + bias[n];
    if (Q) {
      const float q = tanhf(v), z = A.z[at], hv = A.h[at];
      A.out[at] = (1.f - z) * hv + z * q;
    } else {
      const float g = __fdiv_rn(1.f, 1.f + expf(-v));
      if (gate == 0) A.zOut[at] = g;
      else A.rhOut[at] = g * A.h[at];
    }
  }
}

}  // namespace cvd
