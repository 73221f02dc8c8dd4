// Feature tracks (DepthVideoProcessor::computeTracks, reference lib/Processor.cpp:646-886).
//
// Per frame f of the walk: the tracks observed in f-1 are continued along the flow f-1 -> f in ascending id, each accepted
// target stamping a prune disk (which later tracks of the same frame may not land in) and a spawn disk; then new tracks are
// spawned at the frame's candidate pixels in descending corner response, each outside every spawn disk stamped so far.
// The state of frame f (its observation list) feeds frame f + 1, so the walk is sequential in f.
//
// Here: k_track_candidates (thread / pixel, a batch of frames) writes one 64-bit key per pixel = (order-preserving bits
// of the corner response, ~pixel index), the rocPRIM segmented radix sort orders each frame's keys descending (ties by
// ascending pixel index, as the sampler; the reference's std::sort leaves them open), and k_track_walk walks the frames
// in ONE persistent workgroup with the prune and spawn bitmasks in LDS.  Each step of a phase tests 1024 items against
// the masks as they stood at the step's start (every wave), compacts the survivors in order, and wave 0 resolves them
// 64 at a time: a lane is rejected if its target's bit is set now or if an accepted lower lane's disk covers it (integer
// test), and the accepted lanes' disks are stamped row by row.  f32 arithmetic in the reference's order (__f*_rn: no
// contraction); every decision is an integer test on those values, so the result is bit-exact.
//
// Storage: observations in walk order (frame by frame, ascending id inside a frame: continued tracks keep their order,
// spawned ones get the next ids), the start frame of every track.  k_track_lengths / k_track_scatter turn that into
// the table (lengths, kept flags, per-track locations) after the walk.
#pragma once

#include "cvd_sampling.h"

namespace cvd {

constexpr int kTrackThreads = 1024;
constexpr int kTrackWaves = kTrackThreads / 64;

struct TrackArgs {
  int F, W, H;
  float invAspect;
  int first, last;                          // frameRange.firstFrame() / lastFrame()
  int spawnR, pruneR;
  float minDyn;
  const unsigned char* active;              // [F] frame in range and its colour image present
  const unsigned char* pairPresent;         // [F-1] bit 0: flow f -> f+1 present, bit 1: its mask present
  const float* corner;                      // [F][H][W]
  const float* dyn;                         // [F][dh][dw] distance to the nearest dynamic pixel, or nullptr (FLT_MAX)
  int dw, dh;
  const float2* flow;                       // [F-1][H][W]
  const unsigned char* mask;                // [F-1][H][W]
};

struct TrackBufs {
  int* frameStart;                          // [F] first observation of the frame
  int* frameCount;                          // [F]
  int* obsTrack;                            // [obsCap] track id of each observation
  float2* obsLoc;                           // [obsCap]
  int* trackStart;                          // [trackCap] first frame of each track
  int obsCap, trackCap;
};

struct TrackState {                         // carried from one launch of the walk to the next
  int obsUsed, numTracks, stopFrame, pad;
};

// corner response -> ascending unsigned order; -0 ranks with +0 (the reference compares with `>`)
__device__ __forceinline__ unsigned int trackKeyBits(float v) {
  unsigned int u = __float_as_uint(v);
  if (u == 0x80000000u) u = 0u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// (x, y) -> index of the dynamic-distance map; the reference's Mat access is unchecked, the clamp only guards memory
__device__ __forceinline__ size_t trackDynIndex(const TrackArgs& A, int f, float fx, float fy) {
  const float sx = __fdiv_rn(static_cast<float>(A.dw), static_cast<float>(A.W));
  const float sy = __fdiv_rn(static_cast<float>(A.dh), static_cast<float>(A.H));
  const int ix = min(max(static_cast<int>(__fmul_rn(fx, sx)), 0), A.dw - 1);
  const int iy = min(max(static_cast<int>(__fmul_rn(fy, sy)), 0), A.dh - 1);
  return static_cast<size_t>(f) * A.dw * A.dh + static_cast<size_t>(iy) * A.dw + ix;
}

// Spawn candidates of frames f0 .. f0 + gridDim.y - 1, reference :830-858: frames that spawn (active, f < last), pixels
// with (no mask of (f-1, f) or mask set) and dynamic distance > minDyn.  Invalid pixels get key 0 and sink to the end.
inline __global__ __launch_bounds__(256) void k_track_candidates(TrackArgs A, int f0, unsigned long long* __restrict__ keys,
                                                                 unsigned int* __restrict__ nValid) {
  const int pix = blockIdx.x * blockDim.x + threadIdx.x;
  const int fb = blockIdx.y, f = f0 + fb;
  const int npx = A.W * A.H;
  bool ok = false;
  if (pix < npx) {
    const int y = pix / A.W, x = pix - y * A.W;
    ok = A.active[f] && f < A.last;
    if (ok && f > 0 && (A.pairPresent[f - 1] & 2))
      ok = A.mask[static_cast<size_t>(f - 1) * npx + pix] != 0;
    if (ok && A.dyn != nullptr)
      ok = A.dyn[trackDynIndex(A, f, static_cast<float>(x), static_cast<float>(y))] > A.minDyn;
    const unsigned int hi = ok ? trackKeyBits(A.corner[static_cast<size_t>(f) * npx + pix]) : 0u;
    keys[static_cast<size_t>(fb) * npx + pix] =
        (static_cast<unsigned long long>(hi) << 32) | static_cast<unsigned int>(~static_cast<unsigned int>(pix));
  }
  const unsigned long long b = __ballot(ok);
  if ((threadIdx.x & 63) == 0 && b) atomicAdd(&nValid[fb], static_cast<unsigned int>(__popcll(b)));
}

__device__ __forceinline__ bool trackBit(const unsigned int* m, int q) { return (m[q >> 5] >> (q & 31)) & 1u; }

// Stamp the disk dx^2 + dy^2 <= r^2 around (cx, cy), clipped to the image (reference splatKernel): one row per lane.
__device__ __forceinline__ void trackStampDisk(unsigned int* m, int W, int H, int cx, int cy, int r, int lane) {
  for (int r0 = -r; r0 <= r; r0 += 64) {
    const int dy = r0 + lane, yy = cy + dy;
    if (dy > r || yy < 0 || yy >= H) continue;
    const int rem = r * r - dy * dy;
    int hw = static_cast<int>(sqrtf(static_cast<float>(rem)));
    while (hw > 0 && hw * hw > rem) --hw;
    while ((hw + 1) * (hw + 1) <= rem) ++hw;
    const int x0 = max(cx - hw, 0), x1 = min(cx + hw, W - 1);
    if (x0 > x1) continue;
    const int q0 = yy * W + x0, q1 = yy * W + x1;
    for (int w = q0 >> 5; w <= (q1 >> 5); ++w) {
      const unsigned int lo = (w == (q0 >> 5)) ? (q0 & 31) : 0u, hi = (w == (q1 >> 5)) ? (q1 & 31) : 31u;
      atomicOr(&m[w], (0xFFFFFFFFu >> (31u - hi)) & (0xFFFFFFFFu << lo));
    }
  }
}

struct TrackShared {
  int sx[kTrackThreads], sy[kTrackThreads], sid[kTrackThreads];
  float2 sloc[kTrackThreads];
  int waveCount[kTrackWaves];
  int obsUsed, numTracks, prevStart, prevCount, stop, total;
};

// One walk over frames [f0, f1).  keys / nValid: the sorted candidates of this batch (frame f at (f - f0) * W * H).
// Stops before a frame whose worst case (continued + spawned observations, spawned tracks) does not fit the buffers and
// reports it in state->stopFrame (f1 when done); the host grows the buffers and launches again from there.
inline __global__ __launch_bounds__(kTrackThreads) void k_track_walk(TrackArgs A, int f0, int f1,
                                                                     const unsigned long long* __restrict__ keys,
                                                                     const unsigned int* __restrict__ nValid, TrackBufs B,
                                                                     TrackState* __restrict__ state) {
  extern __shared__ unsigned int masks[];   // prune bits, then spawn bits: 2 x ceil(W H / 32) words
  __shared__ TrackShared S;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int npx = A.W * A.H, words = (npx + 31) / 32;
  unsigned int* prune = masks;
  unsigned int* spawn = masks + words;
  if (tid == 0) {
    S.obsUsed = state->obsUsed;
    S.numTracks = state->numTracks;
    S.prevStart = f0 > 0 ? B.frameStart[f0 - 1] : 0;
    S.prevCount = f0 > 0 ? B.frameCount[f0 - 1] : 0;
    S.stop = f1;
  }
  __syncthreads();
  for (int f = f0; f < f1; ++f) {
    const unsigned int nCand = nValid[f - f0];
    if (tid == 0) {
      const long long needObs = static_cast<long long>(S.obsUsed) + S.prevCount + nCand;
      const long long needTracks = static_cast<long long>(S.numTracks) + nCand;
      if (needObs > B.obsCap || needTracks > B.trackCap) S.stop = f;
    }
    __syncthreads();
    if (S.stop != f1) break;
    const int frameObs0 = S.obsUsed;
    if (A.active[f]) {
      for (int i = tid; i < 2 * words; i += kTrackThreads) masks[i] = 0u;
      __syncthreads();
      // this frame reads the observations wave 0 wrote for f - 1: past the barrier, drop stale L1 lines
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      for (int phase = 0; phase < 2; ++phase) {
        const bool cont = phase == 0;
        if (cont && !(f > A.first && (A.pairPresent[f - 1] & 3) == 3)) continue;
        if (!cont && !(f < A.last)) continue;
        const int n = cont ? S.prevCount : static_cast<int>(nCand);
        const int r = cont ? A.pruneR : A.spawnR;
        const unsigned int* test = cont ? prune : spawn;
        const size_t pl = static_cast<size_t>(f - 1) * npx;  // (cont only)
        for (int base = 0; base < n; base += kTrackThreads) {
          // ---- every wave: the order-independent tests and the mask as it stood at the step's start
          const int k = base + tid;
          bool c = false;
          int x = 0, y = 0, id = 0;
          float2 loc = make_float2(0.f, 0.f);
          if (k < n && cont) {  // reference :796-818
            const int o = S.prevStart + k;
            id = B.obsTrack[o];
            const float2 l0 = B.obsLoc[o];
            const float fx0 = __fmul_rn(l0.x, static_cast<float>(A.W));
            const float fy0 = __fmul_rn(__fdiv_rn(l0.y, A.invAspect), static_cast<float>(A.H));
            const int ix0 = min(max(static_cast<int>(__fadd_rn(fx0, 0.5f)), 0), A.W - 1);
            const int iy0 = min(max(static_cast<int>(__fadd_rn(fy0, 0.5f)), 0), A.H - 1);
            const size_t q0 = pl + static_cast<size_t>(iy0) * A.W + ix0;
            if (A.mask[q0]) {
              const float2 ff = A.flow[q0];
              const float fx1 = __fadd_rn(fx0, ff.x), fy1 = __fadd_rn(fy0, ff.y);
              x = static_cast<int>(__fadd_rn(fx1, 0.5f));
              y = static_cast<int>(__fadd_rn(fy1, 0.5f));
              c = fx1 == fx1 && fy1 == fy1 && x >= 0 && x < A.W && y >= 0 && y < A.H;
              if (c && A.dyn != nullptr) c = A.dyn[trackDynIndex(A, f, fx1, fy1)] >= A.minDyn;
              loc = make_float2(__fdiv_rn(fx1, static_cast<float>(A.W)),
                                __fmul_rn(__fdiv_rn(fy1, static_cast<float>(A.H)), A.invAspect));
            }
          } else if (k < n) {  // reference :860-871
            const unsigned int pix = ~static_cast<unsigned int>(keys[static_cast<size_t>(f - f0) * npx + k]);
            const int py = static_cast<int>(pix) / A.W, px = static_cast<int>(pix) - py * A.W;
            loc = make_float2(__fdiv_rn(static_cast<float>(px), static_cast<float>(A.W)),
                              __fmul_rn(__fdiv_rn(static_cast<float>(py), static_cast<float>(A.H)), A.invAspect));
            // the f32 round trip of the stored position (some rows come back as y - 1)
            x = min(max(static_cast<int>(__fmul_rn(loc.x, static_cast<float>(A.W))), 0), A.W - 1);
            y = min(max(static_cast<int>(__fmul_rn(__fdiv_rn(loc.y, A.invAspect), static_cast<float>(A.H))), 0), A.H - 1);
            c = true;
          }
          if (c) c = !trackBit(test, y * A.W + x);
          // ---- in-order compaction of the survivors
          const unsigned long long b = __ballot(c);
          if (lane == 0) S.waveCount[wave] = __popcll(b);
          __syncthreads();
          int before = 0;
          for (int w2 = 0; w2 < wave; ++w2) before += S.waveCount[w2];
          if (c) {
            const int p = before + __popcll(b & ((1ull << lane) - 1ull));
            S.sx[p] = x; S.sy[p] = y; S.sid[p] = id; S.sloc[p] = loc;
          }
          if (tid == 0) {
            int t = 0;
            for (int w2 = 0; w2 < kTrackWaves; ++w2) t += S.waveCount[w2];
            S.total = t;
          }
          __syncthreads();
          // ---- wave 0: greedy in order, 64 survivors at a time
          if (wave == 0) {
            const int total = S.total;
            int used = S.obsUsed, nt = S.numTracks;
            for (int c0 = 0; c0 < total; c0 += 64) {
              const int j = c0 + lane;
              bool v = j < total;
              int lx = 0, ly = 0, lid = 0;
              float2 ll = make_float2(0.f, 0.f);
              if (v) { lx = S.sx[j]; ly = S.sy[j]; lid = S.sid[j]; ll = S.sloc[j]; }
              if (v) v = !trackBit(test, ly * A.W + lx);  // stamps of earlier chunks of this step
              unsigned long long rem = __ballot(v), acc = 0;
              while (rem) {
                const int l = __ffsll(static_cast<long long>(rem)) - 1;
                acc |= 1ull << l;
                const int bx = __shfl(lx, l, 64), by = __shfl(ly, l, 64);
                const int dx = lx - bx, dy = ly - by;
                rem &= ~__ballot(lane > l && dx * dx + dy * dy <= r * r);
                rem &= ~(1ull << l);
              }
              const bool mine = (acc >> lane) & 1ull;
              const int rank = __popcll(acc & ((1ull << lane) - 1ull));
              if (mine) {
                const int o = used + rank;
                if (cont) {
                  B.obsTrack[o] = lid;
                } else {
                  B.obsTrack[o] = nt + rank;
                  B.trackStart[nt + rank] = f;
                }
                B.obsLoc[o] = ll;
              }
              used += __popcll(acc);
              if (!cont) nt += __popcll(acc);
              for (unsigned long long a = acc; a;) {
                const int l = __ffsll(static_cast<long long>(a)) - 1;
                a &= a - 1;
                const int cx = __shfl(lx, l, 64), cy = __shfl(ly, l, 64);
                if (cont) trackStampDisk(prune, A.W, A.H, cx, cy, A.pruneR, lane);
                trackStampDisk(spawn, A.W, A.H, cx, cy, A.spawnR, lane);
              }
              __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");  // the stamps land before the next chunk's test
            }
            if (lane == 0) { S.obsUsed = used; S.numTracks = nt; }
          }
          __syncthreads();
        }
      }
    }
    if (tid == 0) {
      B.frameStart[f] = frameObs0;
      B.frameCount[f] = S.obsUsed - frameObs0;
      S.prevStart = frameObs0;
      S.prevCount = S.obsUsed - frameObs0;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    __syncthreads();
  }
  if (tid == 0) {
    state->obsUsed = S.obsUsed;
    state->numTracks = S.numTracks;
    state->stopFrame = S.stop;
  }
}

// observations per track (the tracks are sequential: its length)
inline __global__ __launch_bounds__(256) void k_track_lengths(int numObs, const int* __restrict__ obsTrack,
                                                              int* __restrict__ length) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < numObs) atomicAdd(&length[obsTrack[i]], 1);
}

// minTrackLength pruning, reference :875-883: kept length (0 for a deleted track) and kept flag
inline __global__ __launch_bounds__(256) void k_track_keep(int numTracks, int minLength, const int* __restrict__ length,
                                                           int* __restrict__ keptLength, unsigned char* __restrict__ kept) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t < numTracks) {
    const bool k = length[t] >= minLength;
    kept[t] = k ? 1 : 0;
    keptLength[t] = k ? length[t] : 0;
  }
}

// observations of frame blockIdx.y -> per-track location lists (offset[t] = exclusive scan of the kept lengths)
inline __global__ __launch_bounds__(256) void k_track_scatter(const int* __restrict__ frameStart, const int* __restrict__ frameCount,
                                                              const int* __restrict__ obsTrack, const float2* __restrict__ obsLoc,
                                                              const int* __restrict__ trackStart,
                                                              const unsigned char* __restrict__ kept,
                                                              const int* __restrict__ offset, float2* __restrict__ out) {
  const int f = blockIdx.y;
  const int n = frameCount[f], s = frameStart[f];
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const int t = obsTrack[s + i];
    if (kept[t]) out[offset[t] + (f - trackStart[t])] = obsLoc[s + i];
  }
}

}  // namespace cvd
