// Fine-tuning batches from a device-resident store: what the reference's loaders/video_dataset.py::VideoDataset
// re-reads from disk, flips, transposes, stacks, collates and copies to the device for every sample of every epoch --
//   __getitem__ + get_neighbor_meta   reference loaders/video_dataset.py:223-256, 309-398   one sample's tensors
//   torch's default collate + to_device                                                       the batch on the GPU
//   update_poses                      reference loaders/video_dataset.py:153-217             per-frame scale maps and warps
// Here the colour, flow and mask images, the cameras and the per-frame tables stay in HBM in their FILE layout (interleaved HWC
// colour and flow, 8-bit masks) and ONE launch of k_dataset_batch writes every tensor of a batch in the layout the losses read
// (planar CHW, f32 masks).  Pure data movement: every output element is a copy of a store element or the constant 0 / 1, so the
// batch equals the reference's bit for bit.  The per-frame tables are filled by k_dataset_scale_map / k_dataset_warp_map with the
// gathers of cvd_dense.h (one launch per table instead of one host spline evaluation per pixel and frame).
#pragma once

#include <type_traits>

#include "cvd_dense.h"

namespace cvd {

constexpr int kBatchThreads = 256;
constexpr int kBatchMaxFrames = 6;   // frames of a sample: the pair, then the clamped neighbours (a-1, a+1, b-1, b+1)

// One sample of the table built by cvd_dataset_create: frames, store slots of the flows that go with them (slot[0..1]: a -> b,
// b -> a; slot[2..5]: a -> a-1, a -> a+1, b -> b-1, b -> b+1, -1 = the reference's dummy) and whether a / b is an interior frame.
struct DatasetSample {
  int frame[kBatchMaxFrames];
  int slot[kBatchMaxFrames];
  int valid[2];
};

// The store (device addresses; by value: uniform -> SGPRs).
struct DatasetStore {
  const float* color;           // [F][npx][3], the channel order of the batch
  const float* flow;            // [Q][npx][2]
  const unsigned char* mask;    // [Q][npx], nonzero = 1
  const float* depthOrig;       // [F][npx] or null
  const float* ext;             // [F][12]
  const float* intr;            // [F][4]
  const float* scales;          // [F][npx] (scaleMode 2), [F] (1) or null (0)
  const float* warp;            // [F][2][npx] or null
  const DatasetSample* samples; // [S]
  int S, npx, N, scaleMode;
};

// Where a batch goes (device addresses).  Optional outputs are null.
struct DatasetBatch {
  float* images;          // (B, N, 3, npx)
  float* ext;             // (B, N, 12)
  float* intr;            // (B, N, 4)
  long long* gcIndices;   // (B, 2)
  float* gcFlow[2];       // (B, 2, npx)
  float* gcMask[2];       // (B, npx)
  long long* tsIndices;   // (B, 4)
  float* tsFlow[4];
  float* tsMask[4];
  float* tsValid;         // (B, 2)
  float* scales;          // (B, N, npx) or (B, N)
  float* warp;            // (B, N, 2, npx)
  float* depthOrig;       // (B, 2, npx)
  // first segment (blockIdx.y) of each kind, in this order; a kind that is not written is empty.  segSmall = their total: the
  // workgroup row of the small outputs.
  int segGcFlow, segGcMask, segTsFlow, segTsMask, segScale, segWarp, segDepth, segSmall;
};

// the sample of batch entry b: an index outside [0, S) is clamped into it (counted by the small-output workgroup of entry 0)
__device__ __forceinline__ const DatasetSample& batchSample(const DatasetStore& st, const long long* __restrict__ indices, int b) {
  long long i = indices[b];
  i = i < 0 ? 0 : (i >= st.S ? st.S - 1 : i);
  return st.samples[i];
}

// VEC: 4 consecutive pixels per lane, 16-byte loads and stores (npx % 4 == 0: every plane starts 16-byte aligned); else one pixel.
template <bool VEC>
struct BatchLane {
  static constexpr int kPixels = VEC ? 4 : 1;
  using V = typename std::conditional<VEC, float4, float>::type;
  static __device__ __forceinline__ V splat(float v) {
    if constexpr (VEC) return make_float4(v, v, v, v);
    else return v;
  }
  static __device__ __forceinline__ V load(const float* p) { return *reinterpret_cast<const V*>(p); }
  static __device__ __forceinline__ void store(float* p, V v) { *reinterpret_cast<V*>(p) = v; }
};

// grid (ceil(npx / pixels per lane / kBatchThreads), segSmall + 1, B)
template <bool VEC>
inline __global__ __launch_bounds__(kBatchThreads) void k_dataset_batch(DatasetStore st, DatasetBatch o, const long long* __restrict__ indices,
                                                                        int B, unsigned int* __restrict__ bad) {
  using Lane = BatchLane<VEC>;
  const int b = blockIdx.z, seg = blockIdx.y, N = st.N;
  const size_t npx = static_cast<size_t>(st.npx);
  const DatasetSample& sm = batchSample(st, indices, b);

  if (seg == o.segSmall) {
    // cameras, indices, valid flags, scalar scales: a few hundred bytes, the first lanes of one workgroup per batch entry
    if (blockIdx.x != 0) return;
    const int t = threadIdx.x;
    for (int i = t; i < N * 12; i += kBatchThreads) {
      const int n = i / 12;
      const bool real = n < 2 || sm.valid[(n - 2) >> 1];
      o.ext[(static_cast<size_t>(b) * N + n) * 12 + (i - n * 12)] = real ? st.ext[static_cast<size_t>(sm.frame[n]) * 12 + (i - n * 12)] : 1.f;
    }
    for (int i = t; i < N * 4; i += kBatchThreads) {
      const int n = i >> 2;
      const bool real = n < 2 || sm.valid[(n - 2) >> 1];
      o.intr[(static_cast<size_t>(b) * N + n) * 4 + (i & 3)] = real ? st.intr[static_cast<size_t>(sm.frame[n]) * 4 + (i & 3)] : 1.f;
    }
    if (t < 2) o.gcIndices[static_cast<size_t>(b) * 2 + t] = sm.frame[t];
    if (N > 2) {
      if (t < 4) o.tsIndices[static_cast<size_t>(b) * 4 + t] = sm.frame[2 + t];
      if (t < 2) o.tsValid[static_cast<size_t>(b) * 2 + t] = sm.valid[t] ? 1.f : 0.f;
    }
    if (o.scales && st.scaleMode == 1 && t < N) o.scales[static_cast<size_t>(b) * N + t] = st.scales[sm.frame[t]];
    if (b == 0 && t == 0) {
      // out-of-range indices of this launch (launches on the store are ordered on one stream: a plain read-modify-write)
      unsigned int n = 0;
      for (int k = 0; k < B; ++k) n += (indices[k] < 0 || indices[k] >= st.S) ? 1u : 0u;
      if (n) *bad += n;
    }
    return;
  }

  const size_t q = static_cast<size_t>(blockIdx.x) * kBatchThreads + threadIdx.x;
  const size_t px = q * Lane::kPixels;   // first pixel of the lane
  if (px >= npx) return;

  if (seg < o.segGcFlow) {
    // colour of frame n: interleaved (r g b) x pixels -> three planes
    const int n = seg;
    float* dst = o.images + (static_cast<size_t>(b) * N + n) * 3 * npx + px;
    const bool real = n < 2 || sm.valid[(n - 2) >> 1];
    if (!real) {
      for (int c = 0; c < 3; ++c) Lane::store(dst + c * npx, Lane::splat(0.f));
      return;
    }
    const float* src = st.color + (static_cast<size_t>(sm.frame[n]) * npx + px) * 3;
    if constexpr (VEC) {
      const float4 v0 = Lane::load(src), v1 = Lane::load(src + 4), v2 = Lane::load(src + 8);
      Lane::store(dst, make_float4(v0.x, v0.w, v1.z, v2.y));
      Lane::store(dst + npx, make_float4(v0.y, v1.x, v1.w, v2.z));
      Lane::store(dst + 2 * npx, make_float4(v0.z, v1.y, v2.x, v2.w));
    } else {
      for (int c = 0; c < 3; ++c) dst[c * npx] = src[c];
    }
  } else if (seg < o.segTsFlow) {
    // flow (interleaved (x y) x pixels -> two planes) or mask (u8, nonzero -> 1.0) of the pair's direction d
    const bool isMask = seg >= o.segGcMask;
    const int d = seg - (isMask ? o.segGcMask : o.segGcFlow);
    const size_t slot = static_cast<size_t>(sm.slot[d]);
    if (!isMask) {
      const float* src = st.flow + (slot * npx + px) * 2;
      float* dst = o.gcFlow[d] + static_cast<size_t>(b) * 2 * npx + px;
      if constexpr (VEC) {
        const float4 v0 = Lane::load(src), v1 = Lane::load(src + 4);
        Lane::store(dst, make_float4(v0.x, v0.z, v1.x, v1.z));
        Lane::store(dst + npx, make_float4(v0.y, v0.w, v1.y, v1.w));
      } else {
        dst[0] = src[0];
        dst[npx] = src[1];
      }
    } else {
      const unsigned char* src = st.mask + slot * npx + px;
      float* dst = o.gcMask[d] + static_cast<size_t>(b) * npx + px;
      if constexpr (VEC) {
        const uchar4 m = *reinterpret_cast<const uchar4*>(src);
        Lane::store(dst, make_float4(m.x ? 1.f : 0.f, m.y ? 1.f : 0.f, m.z ? 1.f : 0.f, m.w ? 1.f : 0.f));
      } else {
        dst[0] = src[0] ? 1.f : 0.f;
      }
    }
  } else if (seg < o.segScale) {
    // the same of neighbour direction d (a -> a-1, a -> a+1, b -> b-1, b -> b+1); ones for a boundary frame
    const bool isMask = seg >= o.segTsMask;
    const int d = seg - (isMask ? o.segTsMask : o.segTsFlow);
    const int slot = sm.slot[2 + d];
    if (!isMask) {
      float* dst = o.tsFlow[d] + static_cast<size_t>(b) * 2 * npx + px;
      if (slot < 0) {
        Lane::store(dst, Lane::splat(1.f));
        Lane::store(dst + npx, Lane::splat(1.f));
        return;
      }
      const float* src = st.flow + (static_cast<size_t>(slot) * npx + px) * 2;
      if constexpr (VEC) {
        const float4 v0 = Lane::load(src), v1 = Lane::load(src + 4);
        Lane::store(dst, make_float4(v0.x, v0.z, v1.x, v1.z));
        Lane::store(dst + npx, make_float4(v0.y, v0.w, v1.y, v1.w));
      } else {
        dst[0] = src[0];
        dst[npx] = src[1];
      }
    } else {
      float* dst = o.tsMask[d] + static_cast<size_t>(b) * npx + px;
      if (slot < 0) {
        Lane::store(dst, Lane::splat(1.f));
        return;
      }
      const unsigned char* src = st.mask + static_cast<size_t>(slot) * npx + px;
      if constexpr (VEC) {
        const uchar4 m = *reinterpret_cast<const uchar4*>(src);
        Lane::store(dst, make_float4(m.x ? 1.f : 0.f, m.y ? 1.f : 0.f, m.z ? 1.f : 0.f, m.w ? 1.f : 0.f));
      } else {
        dst[0] = src[0] ? 1.f : 0.f;
      }
    }
  } else if (seg < o.segWarp) {
    // scale map of frame n (the clamped neighbours are real frames, also where their images are dummies)
    const int n = seg - o.segScale;
    Lane::store(o.scales + (static_cast<size_t>(b) * N + n) * npx + px, Lane::load(st.scales + static_cast<size_t>(sm.frame[n]) * npx + px));
  } else if (seg < o.segDepth) {
    // warp of frame n: two planes
    const int n = seg - o.segWarp;
    const float* src = st.warp + static_cast<size_t>(sm.frame[n]) * 2 * npx + px;
    float* dst = o.warp + (static_cast<size_t>(b) * N + n) * 2 * npx + px;
    const typename Lane::V v0 = Lane::load(src), v1 = Lane::load(src + npx);
    Lane::store(dst, v0);
    Lane::store(dst + npx, v1);
  } else {
    // initial depth (1 / disparity) of the pair's frame n
    const int n = seg - o.segDepth;
    Lane::store(o.depthOrig + (static_cast<size_t>(b) * 2 + n) * npx + px, Lane::load(st.depthOrig + static_cast<size_t>(sm.frame[n]) * npx + px));
  }
}

// The store's per-frame tables from the transforms' parameters (reference loaders/video_dataset.py:199-217 calls
// GridDepthXform::paramMap and SpatialXform::warp per frame on the host).  One thread per pixel, all frames in one launch, the
// f64 tap sums of cvd_dense.h stored as f32 (what torch.Tensor(...) makes of the reference's maps).  params: [F][per] doubles.
// out[f][y][x] = sum_k w_k theta_f[k]  (2-D grid, value transform Scale)
template <int KD>
inline __global__ __launch_bounds__(256) void k_dataset_scale_map(Layout L, int W, int H, const double* __restrict__ params,
                                                                  float* __restrict__ out) {
  const int pidx = blockIdx.x * blockDim.x + threadIdx.x;
  if (pidx >= W * H) return;
  const int py = pidx / W, px = pidx - py * W;
  const int f = blockIdx.z;
  float lx, ly;
  pixelLoc(px, py, W, H, lx, ly);
  const double* th = params + static_cast<size_t>(f) * L.nD;
  double a = 0.0;
  if constexpr (KD >= 16) {
    // cubic grid: depthGather's taps in their order (row by row), from the separable form so that no tap list is indexed
    CubicSep c;
    bicubicSeparable(lx, ly, L.gx, L.gy, L.maxcx, L.maxcy, c);
#pragma unroll
    for (int y = 0; y < 4; ++y)
#pragma unroll
      for (int x = 0; x < 4; ++x)
        if (y < c.ys && x < c.xs) a += th[c.base + x + y * L.gx] * (c.fx[x] * c.fy[y]);
  } else {
    Taps<KD> t;
    depthGather<KD>(L, lx, ly, 0.f, t);
#pragma unroll
    for (int k = 0; k < KD; ++k)   // (constant trip count: the taps stay in registers)
      if (k < t.n) a += th[t.idx[k]] * t.w[k];
  }
  out[static_cast<size_t>(f) * W * H + pidx] = static_cast<float>(a);
}

// out[f][c][y][x] = sum_k u_k phi_f[k][c]  (planar: the (2, H, W) the reference transposes its (H, W, 2) warp into)
template <int KS>
inline __global__ __launch_bounds__(256) void k_dataset_warp_map(Layout L, int W, int H, const double* __restrict__ params,
                                                                 float* __restrict__ out) {
  const int pidx = blockIdx.x * blockDim.x + threadIdx.x;
  if (pidx >= W * H) return;
  const int py = pidx / W, px = pidx - py * W;
  const int f = blockIdx.z;
  float lx, ly;
  pixelLoc(px, py, W, H, lx, ly);
  double wx = 0.0, wy = 0.0;
  if constexpr (KS >= 16) {
    // bicubic grid: spatialGather's taps in their order, from the separable form (as k_dataset_scale_map)
    const double* ph = params + static_cast<size_t>(f) * L.nS;
    CubicSep c;
    bicubicSeparable(lx, ly, L.sgx, L.sgy, L.smaxcx, L.smaxcy, c);
#pragma unroll
    for (int y = 0; y < 4; ++y)
#pragma unroll
      for (int x = 0; x < 4; ++x)
        if (y < c.ys && x < c.xs) {
          const int i = c.base + x + y * L.sgx;
          const double u = c.fx[x] * c.fy[y];
          wx += ph[i * 2] * u;
          wy += ph[i * 2 + 1] * u;
        }
  } else if constexpr (KS > 0) {
    Taps<KS> t;
    spatialGather<KS>(L, lx, ly, t);
    const double* ph = params + static_cast<size_t>(f) * L.nS;
#pragma unroll
    for (int k = 0; k < KS; ++k) {   // (constant trip count: the taps stay in registers)
      if (k < t.n) {
        wx += ph[t.idx[k] * 2] * t.w[k];
        wy += ph[t.idx[k] * 2 + 1] * t.w[k];
      }
    }
  }
  float* o = out + static_cast<size_t>(f) * 2 * W * H + pidx;
  o[0] = static_cast<float>(wx);
  o[static_cast<size_t>(W) * H] = static_cast<float>(wy);
}

// [F] scalars: 1.0 (Identity) or theta_f[0] (Global)
inline __global__ void k_dataset_scale_scalars(int F, int nD, const double* __restrict__ params, float* __restrict__ out) {
  const int f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f < F) out[f] = nD > 0 ? static_cast<float>(params[static_cast<size_t>(f) * nD]) : 1.f;
}

}  // namespace cvd
