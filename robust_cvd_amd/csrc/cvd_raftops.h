// RAFT's two non-convolution operators, f32, forward only: the all-pairs correlation pyramid with its
// windowed lookup (reference raft/core/corr.py:8-46, raft/core/utils/utils.py:56-70) and the convex 8x upsampling of the flow
// (raft/core/raft.py:49-60).  No atomics anywhere: every output element is written once, by one thread, in a fixed operation
// order, so results repeat bit for bit.  f32 in the reference's operation order where that order is observable (no FMA
// contraction); the one non-reproducible operation is expf of the upsampling's softmax.
//
//   k_corr_pyramid      ONE pass over the volume: two adjacent lanes own an 8 x 8 block of one query's level-0 map, each an
//                       8-row x 4-column strip (one float4 per row: the wave's loads and stores are contiguous 16-byte pieces).
//                       A lane divides its strip by sqrt(dim) (IEEE division: level 0 matches torch / numpy bit for bit) and
//                       forms its 8 + 2 means of levels 1 and 2 in registers; the left lane takes the right lane's two level-2
//                       values across lanes for the block's level-3 mean.  Read once, write 1 + 1/4 + 1/16 + 1/64 of the volume.
//                       A level is floor(h / 2) x floor(w / 2) of the one above (avg_pool2d(2, stride 2)): an odd last row /
//                       column is dropped, level by level; every kept mean has its four inputs inside the level above.
//                       (One lane per 8 x 8 block, 32-byte pieces at a 32-byte lane stride, took 0.215 ms where this takes
//                       0.174 ms on the 340 MB volume of a 1024 x 576 input, same bits: DESIGN.md §3.15.)
//   k_corr_lookup<R>    one workgroup per (64 consecutive queries, level).  The (2R+1)^2 taps of a query share ONE fractional
//                       offset and a (2R+2)^2 footprint anchored at floor(c) - R: phase 1 gathers the footprints (row segments
//                       of 2R+2 contiguous floats, zero outside the map = grid_sample's zero padding) into LDS with an odd
//                       stride per query, phase 2 has lane = query, the four weights in registers and the four waves striding
//                       over the channels: every global store of a channel is 64 consecutive floats.
//   k_convex_upsample   one thread per (n, y, i, x): 9 x 8 logits (each read coalesced along x), max and sum per j in
//                       registers, the nine neighbours of 8 flow loaded once, 2 x 8 contiguous floats written.
#pragma once
#include <hip/hip_runtime.h>

namespace cvd {

constexpr int kRaftMaxLevels = 4;
constexpr int kRaftMaxRadius = 4;
constexpr int kRaftThreads = 256;
constexpr int kRaftTileQueries = 64;   // queries per lookup workgroup: phase 2 has lane = query

struct CorrPyramidArgs {
  const float* raw;          // [Q][h][w] fmap1^T fmap2; may be level[0] itself (a thread reads its strip before it writes it)
  float* level[kRaftMaxLevels];   // level l: [Q][h >> l][w >> l]; entries >= levels are not touched
  long long Q;
  int h, w, levels;
  int nbx, nby;              // 8 x 8 blocks per row / column of a level-0 map (ceil)
  float scale;               // sqrtf((float)dim)
};

// mean of a 2 x 2 cell in avg_pool2d's order: the window's sum row by row, then the division by 4 (exact as a product)
__device__ __forceinline__ float raftMean4(float a, float b, float c, float d) {
#pragma clang fp contract(off)
  return (((a + b) + c) + d) * 0.25f;
}

// threads of a launch: two per 8 x 8 block
__host__ __device__ inline long long corrPyramidThreads(const CorrPyramidArgs& A) { return A.Q * (2ll * A.nbx) * A.nby; }

inline __global__ __launch_bounds__(kRaftThreads) void k_corr_pyramid(CorrPyramidArgs A) {
#pragma clang fp contract(off)
  const int ns = 2 * A.nbx;                                  // strips per row of blocks: lanes 2 k, 2 k + 1 share an 8 x 8 block
  const long long perQuery = static_cast<long long>(ns) * A.nby;
  const long long t = static_cast<long long>(blockIdx.x) * kRaftThreads + threadIdx.x;
  if (t >= corrPyramidThreads(A)) return;                    // (an even count: the two lanes of a block leave together)
  const long long q = t / perQuery;
  const int rem = static_cast<int>(t - q * perQuery);
  const int by = rem / ns, s = rem - by * ns;
  const int y0 = by * 8, x0 = s * 4;
  const int h = A.h, w = A.w;
  const size_t base0 = static_cast<size_t>(q) * h * w;
  const float* src = A.raw + base0;
  float* dst0 = A.level[0] + base0;

  float v0[8][4];
  const bool wide = (w & 3) == 0 && x0 + 4 <= w;
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    const bool rowIn = y0 + r < h;
    const float* row = src + static_cast<size_t>(rowIn ? y0 + r : 0) * w + x0;
    if (wide) {
      float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
      if (rowIn) a = *reinterpret_cast<const float4*>(row);
      v0[r][0] = a.x; v0[r][1] = a.y; v0[r][2] = a.z; v0[r][3] = a.w;
    } else {
#pragma unroll
      for (int c = 0; c < 4; ++c) v0[r][c] = (rowIn && x0 + c < w) ? row[c] : 0.f;
    }
  }
#pragma unroll
  for (int r = 0; r < 8; ++r) {
#pragma unroll
    for (int c = 0; c < 4; ++c) v0[r][c] = __fdiv_rn(v0[r][c], A.scale);
    if (y0 + r < h) {
      float* row = dst0 + static_cast<size_t>(y0 + r) * w + x0;
      if (wide) *reinterpret_cast<float4*>(row) = make_float4(v0[r][0], v0[r][1], v0[r][2], v0[r][3]);
      else {
#pragma unroll
        for (int c = 0; c < 4; ++c)
          if (x0 + c < w) row[c] = v0[r][c];
      }
    }
  }
  if (A.levels < 2) return;

  const int h1 = h >> 1, w1 = w >> 1;
  float v1[4][2];
  {
    float* dst = A.level[1] + static_cast<size_t>(q) * h1 * w1;
    const int y1 = y0 >> 1, x1 = x0 >> 1;
    const bool pair = (w1 & 1) == 0 && x1 + 2 <= w1;   // 8-byte aligned and whole
#pragma unroll
    for (int r = 0; r < 4; ++r) {
#pragma unroll
      for (int c = 0; c < 2; ++c) v1[r][c] = raftMean4(v0[2 * r][2 * c], v0[2 * r][2 * c + 1], v0[2 * r + 1][2 * c], v0[2 * r + 1][2 * c + 1]);
      if (y1 + r < h1) {
        float* row = dst + static_cast<size_t>(y1 + r) * w1 + x1;
        if (pair) *reinterpret_cast<float2*>(row) = make_float2(v1[r][0], v1[r][1]);
        else {
          if (x1 < w1) row[0] = v1[r][0];
          if (x1 + 1 < w1) row[1] = v1[r][1];
        }
      }
    }
  }
  if (A.levels < 3) return;

  const int h2 = h1 >> 1, w2 = w1 >> 1;
  float v2[2];
  {
    float* dst = A.level[2] + static_cast<size_t>(q) * h2 * w2;
    const int y2 = y0 >> 2, x2 = s;
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      v2[r] = raftMean4(v1[2 * r][0], v1[2 * r][1], v1[2 * r + 1][0], v1[2 * r + 1][1]);
      if (y2 + r < h2 && x2 < w2) dst[static_cast<size_t>(y2 + r) * w2 + x2] = v2[r];
    }
  }
  if (A.levels < 4) return;

  // level 3: the left strip (even lane) takes the right strip's two values
  const float right0 = __shfl_xor(v2[0], 1), right1 = __shfl_xor(v2[1], 1);
  const int h3 = h2 >> 1, w3 = w2 >> 1;
  const int y3 = by, x3 = s >> 1;
  if ((s & 1) == 0 && y3 < h3 && x3 < w3)
    A.level[3][static_cast<size_t>(q) * h3 * w3 + static_cast<size_t>(y3) * w3 + x3] = raftMean4(v2[0], right0, v2[1], right1);
}

struct CorrLookupArgs {
  const float* level[kRaftMaxLevels];   // level l: [Q][h2 >> l][w2 >> l]
  const float* coords;       // [B][2][h1][w1]: channel 0 = x, 1 = y, level-0 pixels of frame 2
  float* out;                // [B][levels (2R+1)^2][h1][w1]
  long long Q;               // B h1 w1
  int hw1;                   // h1 w1
  int h2, w2, levels;
};

// One axis of a query's sampling position c: the integer anchor floor(c) (clamped, as a float, before the conversion, to where
// the whole window lies outside a map of `size` texels: any finite c, and NaN, gives an in-range int; beyond the clamp every
// footprint texel is padding) and the two weights of grid_sample's bilinear form, (floor + 1) - c and c - floor.
template <int R>
__device__ __forceinline__ int raftAnchor(float c, int size, float& wLo, float& wHi) {
#pragma clang fp contract(off)
  const float f = floorf(c);
  wLo = (f + 1.f) - c;
  wHi = c - f;
  return static_cast<int>(fminf(fmaxf(f, static_cast<float>(-R - 2)), static_cast<float>(size + R)));
}

template <int R>
inline __global__ __launch_bounds__(kRaftThreads) void k_corr_lookup(CorrLookupArgs A) {
#pragma clang fp contract(off)
  constexpr int N = 2 * R + 1, FP = 2 * R + 2, CELLS = FP * FP;
  constexpr int STRIDE = CELLS | 1;   // odd: the lanes of phase 2 (stride = one query) fall on distinct banks
  __shared__ float foot[kRaftTileQueries * STRIDE];
  __shared__ int anchor[kRaftTileQueries][2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lvl = blockIdx.y;
  const int h = A.h2 >> lvl, w = A.w2 >> lvl;
  const long long q0 = static_cast<long long>(blockIdx.x) * kRaftTileQueries;
  const float* __restrict__ vol = A.level[lvl];

  // every wave: the position and weights of query `lane` (phase 2 keeps them); wave 0 publishes the anchors for phase 1
  const long long q = q0 + lane;
  const bool live = q < A.Q;
  long long img = 0;
  int pos = 0;
  float cx = 0.f, cy = 0.f;
  if (live) {
    img = q / A.hw1;
    pos = static_cast<int>(q - img * A.hw1);
    const float* cb = A.coords + static_cast<size_t>(img) * 2 * A.hw1 + pos;
    const float inv = 1.f / static_cast<float>(1 << lvl);   // (a power of two: the product is the reference's division)
    cx = cb[0] * inv;
    cy = cb[A.hw1] * inv;
  }
  float wx0, wx1, wy0, wy1;
  const int ax = raftAnchor<R>(cx, w, wx0, wx1), ay = raftAnchor<R>(cy, h, wy0, wy1);
  if (wave == 0) { anchor[lane][0] = ax - R; anchor[lane][1] = ay - R; }
  __syncthreads();

  // phase 1: footprints, cell-major inside a query: a row segment of FP floats is contiguous in the map
  for (int i = tid; i < kRaftTileQueries * CELLS; i += kRaftThreads) {
    const int ql = i / CELLS, cell = i - ql * CELLS;
    const int fy = cell / FP, fx = cell - fy * FP;
    const int x = anchor[ql][0] + fx, y = anchor[ql][1] + fy;
    float v = 0.f;
    if (q0 + ql < A.Q && x >= 0 && x < w && y >= 0 && y < h)
      v = vol[(static_cast<size_t>(q0 + ql) * h + y) * w + x];
    foot[ql * STRIDE + cell] = v;
  }
  __syncthreads();

  // phase 2: channel a N + b samples (x + a - R, y + b - R): the FIRST window index moves x (the reference's meshgrid order)
  if (!live) return;
  const float wnw = wx0 * wy0, wne = wx1 * wy0, wsw = wx0 * wy1, wse = wx1 * wy1;
  const float* __restrict__ f = foot + lane * STRIDE;
  float* __restrict__ o = A.out + (static_cast<size_t>(img) * A.levels * (N * N) + static_cast<size_t>(lvl) * (N * N)) * A.hw1 + pos;
  for (int ch = wave; ch < N * N; ch += kRaftThreads / 64) {
    const int a = ch / N, b = ch - a * N;
    const float* c = f + b * FP + a;
    o[static_cast<size_t>(ch) * A.hw1] = ((c[0] * wnw + c[1] * wne) + c[FP] * wsw) + c[FP + 1] * wse;
  }
}

struct ConvexUpsampleArgs {
  const float* flow;   // [N][2][H][W]
  const float* mask;   // [N][576][H][W]: channel 64 k + 8 i + j = logit of neighbour k for the sub-pixel (i, j)
  float* out;          // [N][2][8 H][8 W]
  long long total;     // N H 8 W threads
  int H, W;
};

inline __global__ __launch_bounds__(kRaftThreads) void k_convex_upsample(ConvexUpsampleArgs A) {
#pragma clang fp contract(off)
  const long long t = static_cast<long long>(blockIdx.x) * kRaftThreads + threadIdx.x;
  if (t >= A.total) return;
  const int W = A.W, H = A.H;
  const int x = static_cast<int>(t % W);
  long long r = t / W;
  const int i = static_cast<int>(r & 7);
  r >>= 3;
  const int y = static_cast<int>(r % H);
  const long long n = r / H;
  const size_t hw = static_cast<size_t>(H) * W;

  // the nine neighbours of 8 flow, zero outside the image (unfold with padding 1)
  float fl[2][9];
  const float* __restrict__ fb = A.flow + static_cast<size_t>(n) * 2 * hw;
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    const int yy = y + k / 3 - 1, xx = x + k % 3 - 1;
    const bool in = yy >= 0 && yy < H && xx >= 0 && xx < W;
    const size_t at = static_cast<size_t>(in ? yy : y) * W + (in ? xx : x);
    const float u = fb[at], v = fb[hw + at];
    fl[0][k] = in ? 8.f * u : 0.f;
    fl[1][k] = in ? 8.f * v : 0.f;
  }

  const float* __restrict__ mb = A.mask + (static_cast<size_t>(n) * 576 + 8 * i) * hw + static_cast<size_t>(y) * W + x;
  float res[2][8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    float lg[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) lg[k] = mb[static_cast<size_t>(64 * k + j) * hw];
    float mx = lg[0];
#pragma unroll
    for (int k = 1; k < 9; ++k) mx = fmaxf(mx, lg[k]);
    float sum = 0.f;
#pragma unroll
    for (int k = 0; k < 9; ++k) { lg[k] = expf(lg[k] - mx); sum += lg[k]; }   // (logits of +-100: the largest term is exp(0))
    float u = 0.f, v = 0.f;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      const float p = __fdiv_rn(lg[k], sum);
      u += p * fl[0][k];
      v += p * fl[1][k];
    }
    res[0][j] = u;
    res[1][j] = v;
  }
  // 8 W floats per output row: 32-byte aligned at 8 x
  float* ob = A.out + (static_cast<size_t>(n) * 2 * 8 * H + (8 * static_cast<size_t>(y) + i)) * (8 * static_cast<size_t>(W)) + 8 * static_cast<size_t>(x);
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    float4* dst = reinterpret_cast<float4*>(ob + static_cast<size_t>(c) * 64 * hw);
    dst[0] = make_float4(res[c][0], res[c][1], res[c][2], res[c][3]);
    dst[1] = make_float4(res[c][4], res[c][5], res[c][6], res[c][7]);
  }
}

}  // namespace cvd
