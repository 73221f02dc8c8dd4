// cvd_kernels.h -- what every solver kernel header shares, and the hot kernel: the plain types the host hands to the kernels
// (Table, Items, AsmWork, DenseRecords, RegCache, CoarsePlan, CrossPairs, TripletTable, ...), the device helpers more than one
// header needs (dense pixel geometry, loadConstraint / RecordStream, FastTaps, the fast scope's constraint model -- fastRay ...
// fastRows, the one statement every fast kernel calls --, the inter-workgroup hand-offs, pcgFinishScalars),
// the CVD_DETERMINISTIC default and the CVD_MV_* knobs, and the pair product (k_matvec_pairs_fast, k_matvec_pairs).
// cvd_host.h includes this header and no other kernel header: NO non-template __global__ function may be defined here (a unit
// emits device code for every non-template kernel it parses; tests/test_codegen_units.py).
//
// Kernel map -- a translation unit includes, by name, the headers of the kernels it launches (DESIGN.md has the roofline of each):
//   cvd_kernels.h        k_matvec_pairs_fast, k_matvec_pairs      pair-major partial q = J^T (rho' J p), matrix free  <- the hot kernel
//   cvd_table.h          k_frame_consts, k_build_table, k_order_table, k_dense_count, k_adaptive_weights   (per-frame / per-constraint set-up)
//   cvd_cost.h           k_cost_items, k_cost_items_fast, k_cost_frames, k_sum2, k_step_stats              (candidate cost, step statistics)
//   cvd_assembly.h       k_assemble, k_assemble_fast, k_shared_focal_fixup, k_extract_diag                 (g = J^T r, H_ff)
//   cvd_block_inverse.h  k_block_inverse_sweep, k_block_inverse_mfma, k_block_inverse                      (block-Jacobi preconditioner)
//   cvd_pcg.h            k_lm_diag, k_reg_cache, k_matvec_finish, k_dot_pq, k_cg_update, k_pcg_scalars_dist, k_pcg_tail, k_apply_step,
//                        k_tl_rows_init
//   cvd_coarse.h         k_coarse_* (pose-graph level), k_blocks_*, k_flag_to_bool       cvd_temporal.h       k_tl_* (set-up), k_pt_assemble
//   cvd_cross.h          k_cross_matvec, k_coarse_edges_cross                            cvd_dense_inverse.h  k_dense_spd_inverse(_pair)
//   cvd_dense_walk.h     k_dense_walk, k_dense_fold_cross, k_dense_gg, k_dense_list, k_coarse_edges_mfma
//   cvd_triplets.h       k_build_triplet_table, k_cost_triplets, k_assemble_triplets, k_matvec_triplets
#pragma once

#include "cvd_device.h"

namespace cvd {

// Compiled constraint table (the reference rebuilds `Observation`s for every solve,
// lib/PoseOptimizer.cpp:1185-1193; here it is 24 B per constraint, pair-major, resident in HBM).
struct Table {
  const float4* ndc;    // (ndc_a.xy, ndc_b.xy), f32 exactly as the reference computes them
  const float2* dsrc;   // (d_a, d_b) source depths; d_a <= 0 marks a skipped constraint
  const int* pairA;     // per pair
  const int* pairB;
  const long long* pairOff;  // P + 1
  // Dense mode (cvd_set_pair_flows: the reference's matchSeparation = 0 regime, lib/FlowConstraints.cpp:315-329, 381-465 --
  // every masked pixel whose flow target rounds into the image is a constraint): there is NO table; constraint slot c of
  // pair p is pixel c - pairOff[p] (pairOff[p] = p * W * H) and the kernels read flow / mask / depth directly,
  // 8 + 1 + 4 + 4 = 17 B per pixel pair (SURVEY.md 8d "dense mode").
  const float2* flow;           // [P][H][W] pixels
  const unsigned char* fmask;   // [P][H][W]
  const float* depth;           // [F][H][W] source depth
  int W, H;
  float sx, sy, invAspect;      // loc = pixel * (1 / W, invAspect / H), float as in the reference (:371)
};

// Dense mode: everything about a pixel's constraint that follows from its position and flow vector `f` -- ONE statement of the
// reference's float arithmetic for every kernel that reads the images (product, cost, walk, grid x grid, list materialisation):
// candidate test of FlowConstraintsCollection::compute (lib/FlowConstraints.cpp:436-460: target int(x + flow + 0.5) in bounds),
// constraint scaling (:371), the Observation constructor's pixel-edge NDC and truncating depth fetch (lib/PoseOptimizer.cpp:104-116).
// loc = (source x, y, target x, y) in [0, 1] x [0, invAspect]; n = ndc of both end points; ai / bi = the pixels whose source depths
// the two observations read (not always the constraint's own pixel: the fetch truncates loc * raster).  false: no candidate.
__device__ __forceinline__ int densePixelOfLoc(const Table& T, float lx, float ly) {
  int px = static_cast<int>(__fmul_rn(lx, static_cast<float>(T.W)));
  int py = static_cast<int>(__fmul_rn(__fdiv_rn(ly, T.invAspect), static_cast<float>(T.H)));
  px = min(max(px, 0), T.W - 1);
  py = min(max(py, 0), T.H - 1);
  return py * T.W + px;
}
__device__ __forceinline__ bool densePixelGeometry(const Table& T, int ix, int iy, float2 f, float4& loc, float4& n, int& ai, int& bi) {
  const float fx1 = __fadd_rn(static_cast<float>(ix), f.x), fy1 = __fadd_rn(static_cast<float>(iy), f.y);
  if (!(isfinite(fx1) && isfinite(fy1))) return false;
  const int ix1 = static_cast<int>(__fadd_rn(fx1, 0.5f)), iy1 = static_cast<int>(__fadd_rn(fy1, 0.5f));
  if (ix1 < 0 || ix1 >= T.W || iy1 < 0 || iy1 >= T.H) return false;
  const float lx0 = __fmul_rn(static_cast<float>(ix), T.sx), ly0 = __fmul_rn(static_cast<float>(iy), T.sy);
  const float lx1 = __fmul_rn(fx1, T.sx), ly1 = __fmul_rn(fy1, T.sy);
  loc = make_float4(lx0, ly0, lx1, ly1);
  n.x = __fadd_rn(-1.f, __fmul_rn(2.f, lx0));
  n.y = __fsub_rn(1.f, __fdiv_rn(__fmul_rn(2.f, ly0), T.invAspect));
  n.z = __fadd_rn(-1.f, __fmul_rn(2.f, lx1));
  n.w = __fsub_rn(1.f, __fdiv_rn(__fmul_rn(2.f, ly1), T.invAspect));
  ai = densePixelOfLoc(T, lx0, ly0);
  bi = densePixelOfLoc(T, lx1, ly1);
  return true;
}
// ... + the two depths, REQUESTED only (a kernel that runs its loads ahead tests the values when it uses them)
__device__ __forceinline__ bool denseConstraintRequest(const Table& T, int pix, int fa, int fb, float2 f, float4& n, float2& d) {
  const int iy = pix / T.W, ix = pix - iy * T.W;
  float4 loc;
  int ai, bi;
  d = make_float2(0.f, 0.f);
  if (!densePixelGeometry(T, ix, iy, f, loc, n, ai, bi)) return false;
  const size_t fs = static_cast<size_t>(T.W) * T.H;
  d.x = T.depth[fa * fs + ai];
  d.y = T.depth[fb * fs + bi];
  return true;
}
__device__ __forceinline__ bool denseDepthsValid(float2 d) { return isfinite(d.x) && d.x > 0.f && isfinite(d.y) && d.y > 0.f; }
// ... and tested (lib/PoseOptimizer.cpp:1190-1193: an invalid depth skips the whole constraint)
__device__ __forceinline__ bool denseConstraintFromFlow(const Table& T, long long c, long long pixBase, int fa, int fb, float2 f,
                                                        float4& n, float2& d) {
  return denseConstraintRequest(T, static_cast<int>(c - pixBase), fa, fb, f, n, d) && denseDepthsValid(d);
}

// One constraint of the pair-major / frame-major fast kernels: (ndc of both end points, the two source depths); false =
// skipped.  DENSE = false: the compiled 24 B table entry.  DENSE = true: built on the fly from the flow / mask / depth
// images with the reference's float arithmetic -- candidate test of FlowConstraintsCollection::compute (reference
// lib/FlowConstraints.cpp:436-460: mask, target pixel int(x + flow + 0.5) in bounds), constraint scaling (:371), then the
// Observation constructor (lib/PoseOptimizer.cpp:104-116, identical to k_build_table).  fa / fb = source / target frame,
// pixBase = first slot of the pair.
template <bool DENSE>
__device__ __forceinline__ bool loadConstraint(const Table& T, long long c, long long pixBase, int fa, int fb, float4& n,
                                               float2& d) {
  if constexpr (!DENSE) {
    // (both records are requested at once: testing d first made the 16-byte load a SECOND dependent round trip in every trip
    // of the constraint loops; skipped entries are rare and the 16 bytes of one are free)
    d = T.dsrc[c];
    n = T.ndc[c];
    return d.x > 0.f;
  } else {
    if (!T.fmask[c]) return false;
    return denseConstraintFromFlow(T, c, pixBase, fa, fb, T.flow[c], n, d);
  }
}

// Walk over table records c, c + step, ... < end with the NEXT record in flight (list mode; the dense mode's on-the-fly
// constraints go through loadConstraint).  Loaded at the top of its own trip a record is a global round trip -- two,
// dependent, where the compiler sinks the 16-byte half below the validity test of the 8-byte half -- that only the other
// waves of the SIMD can hide; requested one trip ahead (6 registers) it is back before it is needed (hot product
// 50.2 -> 48.6 us, 1000 frames: 213 -> 195 us).
template <bool DENSE>
struct RecordStream {
  float4 ndNext;
  float2 dNext;
  // records base + i, base + i + step, ... (i < n); base is wave-uniform: 32-bit offsets from a scalar base address
  __device__ __forceinline__ void prime(const Table& T, long long base, int i, int n) {
    ndNext = make_float4(0.f, 0.f, 0.f, 0.f);
    dNext = make_float2(0.f, 0.f);
    if (i < n) { dNext = (T.dsrc + base)[i]; ndNext = (T.ndc + base)[i]; }
  }
  // The same without a branch, for a kernel prologue whose loads are all requested before its first wait: a lane outside [0, n)
  // -- an empty direction included, whose base may be the table's end -- reads record 0, which exists whenever an item does.
  __device__ __forceinline__ void primeClamped(const Table& T, long long base, int i, int n) {
    const long long c = i < n ? base + i : 0;
    dNext = T.dsrc[c];
    ndNext = T.ndc[c];
    if (i >= n) { dNext = make_float2(0.f, 0.f); ndNext = make_float4(0.f, 0.f, 0.f, 0.f); }
  }
  // record base + i (false: skipped); requests record base + i + step
  __device__ __forceinline__ bool take(const Table& T, long long base, int i, int step, int n, long long, int, int, float4& nd,
                                       float2& d) {
    nd = ndNext;
    d = dNext;
    if (i + step < n) { dNext = (T.dsrc + base)[i + step]; ndNext = (T.ndc + base)[i + step]; }
    return d.x > 0.f;
  }
};
// Dense mode: a constraint is a chain mask byte -> flow vector -> the two depths (the target's address depends on the
// flow).  Mask and flow of the NEXT pixel are requested one trip ahead (3 registers): one dependent round trip per pixel --
// the depths -- instead of three.
template <>
struct RecordStream<true> {
  float2 fNext;
  unsigned int mNext;
  __device__ __forceinline__ void prime(const Table& T, long long base, int i, int n) {
    fNext = make_float2(0.f, 0.f);
    mNext = 0u;
    if (i < n) { mNext = (T.fmask + base)[i]; fNext = (T.flow + base)[i]; }
  }
  __device__ __forceinline__ void primeClamped(const Table& T, long long base, int i, int n) { prime(T, base, i, n); }
  __device__ __forceinline__ bool take(const Table& T, long long base, int i, int step, int n, long long pixBase, int fa, int fb,
                                       float4& nd, float2& d) {
    const unsigned int m = mNext;
    const float2 f = fNext;
    if (i + step < n) { mNext = (T.fmask + base)[i + step]; fNext = (T.flow + base)[i + step]; }
    if (!m) return false;
    return denseConstraintFromFlow(T, base + i, pixBase, fa, fb, f, nd, d);
  }
};

// The same two pixels ahead (the candidate-cost pass of the dense mode, whose trip is short): mask and flow of pixel i + 2 step are
// requested while the two depths of pixel i + step -- whose address follows from its flow -- are, and pixel i is worked on from
// registers.  One pixel ahead, every trip took the depths' round trip (1.9 ms per pass over 152 M pixel slots).
struct DenseStreamAhead {
  float2 fNext;        // pixel i + step: its flow and mask are here, its depths not yet requested
  unsigned int mNext;
  float4 ndCur;        // pixel i: candidate, ndc, depths (requested; validity is tested when they are used)
  float2 dCur;
  bool candCur;
  __device__ __forceinline__ bool request(const Table& T, int pix, int fa, int fb, float2 f, float4& n, float2& d) const {
    return denseConstraintRequest(T, pix, fa, fb, f, n, d);
  }
  __device__ __forceinline__ void prime(const Table& T, long long base, int i, int step, int n, long long pixBase, int fa, int fb) {
    unsigned int m0 = 0u;
    float2 f0 = make_float2(0.f, 0.f);
    fNext = make_float2(0.f, 0.f);
    mNext = 0u;
    if (i < n) { m0 = (T.fmask + base)[i]; f0 = (T.flow + base)[i]; }
    if (i + step < n) { mNext = (T.fmask + base)[i + step]; fNext = (T.flow + base)[i + step]; }
    ndCur = make_float4(0.f, 0.f, 0.f, 0.f);
    candCur = m0 != 0u && request(T, static_cast<int>(base - pixBase) + i, fa, fb, f0, ndCur, dCur);
  }
  __device__ __forceinline__ bool take(const Table& T, long long base, int i, int step, int n, long long pixBase, int fa, int fb,
                                       float4& nd, float2& d) {
    nd = ndCur;
    d = dCur;
    const bool cand = candCur;
    const unsigned int m1 = mNext;
    const float2 f1 = fNext;
    mNext = 0u;
    if (i + 2 * step < n) { mNext = (T.fmask + base)[i + 2 * step]; fNext = (T.flow + base)[i + 2 * step]; }
    candCur = m1 != 0u && request(T, static_cast<int>(base - pixBase) + i + step, fa, fb, f1, ndCur, dCur);
    return cand && denseDepthsValid(d);
  }
};

// Work items of the pair-major kernels: one UNDIRECTED frame pair {fa < fb} with a chunk of the constraints
// of the directed pair fa->fb (range[0..1]) and of fb->fa (range[2..3]); either may be empty.  Both directions
// share the two frames' parameter blocks, so one workgroup prologue / epilogue serves both.
// The same per item as ONE 64-byte record: k_matvec_pairs_fast reads it with a single scalar load at its top (four arrays were
// four dependent-address scalar loads in front of the prologue, and `range` / `slot` came back as loads behind barriers).
struct alignas(64) ItemRecord {
  int fa, fb;
  int slotA, slotB;        // rows of the partial-product buffer of frame fa / fb
  long long b0, e0;        // constraints of fa -> fb
  long long b1, e1;        // constraints of fb -> fa
  long long pad[2];
};
static_assert(sizeof(ItemRecord) == 64, "one record per 64-byte line");
struct Items {
  const int* fa;
  const int* fb;
  const long long* range;  // 4 per item
  const int* slot;         // 2 per item: rows of the partial-product buffer (frame-major, see k_matvec_finish)
  int count;
  const ItemRecord* rec;   // [count] the arrays above packed per item (the pair product reads only this)
};

// Work list of k_assemble_fast: a frame's (pair, side) entries are cut into units of at most kAsmUnit constraints
// and the units into parts (one workgroup each) of bounded size, so that frames with many pairs (the long-range
// levels of the hierarchical flow list) do not set the kernel's duration.  Parts of a split frame publish their
// packed partial blocks and the last one to arrive folds them (lastBlockArrives on a per-frame counter).
constexpr int kDenseFramesPerGroup = 2;  // frames per dense-level workgroup of k_cg_update (DenseStep)
constexpr int kAsmUnit = 128;
// Dense mode: 1024 pixel slots per unit, dealt to the 64 lanes in runs of 16 consecutive pixels (see kDenseRun)
constexpr int kAsmUnitDense = 1024;
// Dense mode lane mapping.  Consecutive pixels fall into the same grid cell, i.e. hit the same four vertices: with lane =
// pixel every LDS atomic of a wave would collide 64-fold.  Each lane therefore walks its own run of kDenseRun = 16
// consecutive pixels (two 64-byte lines of flow per lane: the images are still streamed once).  Measured on the three
// assembly kernels together: runs of 32 pixels 25.6 ms, 16: 22.5 ms, 8: 22.7 ms, 64: 28.6 ms (150 frames).
constexpr int kDenseRun = 16;

// ---- deterministic build (lib/libcvd_hip_det.so: robust_cvd_amd.build.build_deterministic; tests/test_gpu_determinism.py) ----
// The solver kernels accumulate through LDS f64 atomics from several waves of a workgroup (grid columns of the pair-major
// product, the packed frame blocks of the assembly, the regulariser rows of the PCG tail, the Galerkin blocks of the levels):
// the order in which the waves' atomics land is a matter of timing, so two runs of one solve differ in the last bits, and the
// LM / PCG stopping rules amplify that to +-1 PCG iteration (VERDICT r4 Missing #3).  With CVD_DETERMINISTIC = 1 every such
// accumulation is issued by ONE wave (the kernels run with 64-thread workgroups, or their first wave alone walks the
// constraints) and every fold of partial results runs in index order: a wave's LDS atomics execute in program order and the
// hardware resolves same-address lanes of one instruction in a fixed order, so the sums are reproducible bit for bit.  Several
// times slower; for tests and for telling a race from rounding -- the product build keeps the concurrent form.
#ifndef CVD_DETERMINISTIC
#define CVD_DETERMINISTIC 0
#endif
constexpr int kAtomicWalkers256 = CVD_DETERMINISTIC ? 64 : 256;  // threads of a 256-thread workgroup that walk constraints into LDS atomics
constexpr int kAsmThreads = CVD_DETERMINISTIC ? 64 : 512;  // 8 waves per frame: two per SIMD at 256 VGPRs (deterministic build: one)
struct AsmPart {
  int frame;
  int u0, u1;   // unit range
  int part;     // index within the frame
  int nParts;   // 1: the frame is not split
  int slot0;    // first partial-block slot of the frame (split frames only)
};
struct AsmWork {
  const AsmPart* parts;      // sorted by descending size (longest first)
  const int2* units;         // {pair * 2 + side, first constraint relative to the pair's offset}
  double* scratch;           // partial blocks: slots x (B(B+1)/2 + B + 2) doubles
  unsigned int* counters;    // one per frame, zero between launches
};

// Dense mode, one-walk assembly (cvd_dense_walk.h): k_dense_walk leaves one compact RECORD per directed pair (layout: that
// header); k_assemble_fast<.., FOLD> sums a frame's records into H_ff / g / cost through this view.
__host__ __device__ inline int dwRecordDoubles(int G) { return 256 + 40 * G + 8; }
struct DenseRecords {
  const double* records;
  const int* recOff;     // per directed pair: its records [recOff[p], recOff[p + 1])
  const int* fpOff;      // per frame: entries of fpList
  const int* fpList;     // directed pair * 2 + side (0: the frame is the pair's source, 1: its target)
};

// scalar slots kept on the device during PCG
enum : int { S_RZ = 0, S_RZOLD = 1, S_BETA = 2, S_PQ = 3, S_ALPHA = 4, S_RR = 5, S_RZ0 = 6, S_COST = 7,
             S_DG = 8, S_DR = 9, S_DLD = 10, S_DD = 11, S_XX = 12, S_NVALID = 13, S_GMAX = 14,
             // PCG control, owned by the device: S_DONE 0 running / 1 converged / 2 NaN, S_TARGET = tol^2 rz0,
             // S_ITERS = iterations applied.  Every kernel of an iteration returns at once when S_DONE is set, so
             // the host may enqueue iterations ahead of the convergence test without changing the result.
             S_DONE = 15, S_TARGET = 16, S_ITERS = 17,
             S_RZPART = 18,  // block-Jacobi part of r^T z while the coarse level (cvd_coarse.h) is pending
             S_NACTIVE = 19, // number of active unknowns (k_step_stats)
             S_COUNT = 20 };
// Shares mode of the fused PCG tail (cvd_pcg.h: k_pcg_tail ends without closing r^T z; the next product sums the shares): its words
// live BEHIND the scalars in the same allocation, so the product reaches them through the `scal` argument it has anyway.
//   SH_MIRROR   the host's progress mirror (a pointer, written once when the buffers are made)
//   SH_ABANDON  != 0: a tail of this solve abandoned its grid barrier -- nobody closes an iteration any more
//   SH_RING     r^T z after the iterations of even / odd count: the workgroups of a product read the slot the launch does not write
//   SH_RZ, SH_RR  kPcgSharesCap shares of r^T z (frames, dense-level parts, temporal levels' parts) and of r^T r (frames); the
//               words beyond a solve's share count are zero, so that every sum runs over the whole array in one fixed order
constexpr int kPcgSharesCap = 512;   // eight loads per lane of one wave
constexpr int kPcgMirrorAddressSlot = 15;   // of the host's 16-double pinned mirror buffer ([0 .. 8] are the mirror): the buffer's own
                                            // address, staged there once for the copy into SH_MIRROR
enum : int { SH_MIRROR = 24, SH_ABANDON = 32, SH_RING = 34, SH_RZ = 64, SH_RR = SH_RZ + kPcgSharesCap, SH_END = SH_RR + kPcgSharesCap };

// Sum of a short global array (F per-frame partials, L2-resident) by every workgroup that needs the scalar:
// cheaper than a separate 1-block reduction kernel + its launch boundary. `red` = 4 doubles of LDS.
__device__ __forceinline__ double blockSumArray(const double* __restrict__ a, int n, double* red) {
  double acc = 0.0;
  for (int i = threadIdx.x; i < n; i += blockDim.x) acc += a[i];
  acc = waveSum(acc);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  double t = 0.0;
  for (int w = 0; w < (blockDim.x >> 6); ++w) t += red[w];
  __syncthreads();
  return t;
}

// "Last workgroup finishes the reduction": every workgroup publishes its partials with an agent-scope release,
// takes a ticket, and the last one acquires and reduces (cdna_hip_programming.md G16: release on the producer,
// acquire on the consumer; L1 is per CU and the 8 XCD L2s are not coherent with each other).
// `flag` = one int of LDS. Returns true (for every thread of the block) in the last-arriving workgroup.
__device__ __forceinline__ bool lastBlockArrives(unsigned int* counter, unsigned int total, int* flag) {
  __syncthreads();
  if (threadIdx.x == 0) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const unsigned int t = __hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const bool last = (t == total - 1);
    if (last) {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      __hip_atomic_store(counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // re-arm for the next launch
    }
    *flag = last ? 1 : 0;
  }
  __syncthreads();
  return *flag != 0;
}

// The same hand-off WITHOUT fences, for the three kernels of a PCG iteration (their workgroups exchange a handful of
// doubles): the partials are published by write-through agent-scope stores (publishPartial), every storing wave drains
// them (s_waitcnt vmcnt(0)) before the workgroup's ticket, and the last workgroup reads them back with agent-scope loads
// (readPartial) -- cdna_hip_programming.md G16 recipe R1.  The release fence of lastBlockArrives is a buffer_wbl2 of the
// XCD's whole L2 in EVERY workgroup and the acquire an invalidate, although nothing but the partials crosses workgroups.
// The protocol leans on the gfx942 / gfx950 memory system (agent-scope relaxed atomics are write-through / L2-coherent accesses,
// s_waitcnt vmcnt(0) drains them, workgroups of one launch are ordered by the ticket's data dependency) rather than on the HIP
// memory model's release / acquire edges: this library is built for gfx950 only, and says so.
#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__) && !defined(__gfx942__)
#error "the fence-free inter-workgroup hand-off (publishPartial / readPartial / lastBlockArrivesLite) is written for gfx942 / gfx950"
#endif
__device__ __forceinline__ void publishPartial(double* p, double v) {
  __hip_atomic_store(reinterpret_cast<unsigned long long*>(p), static_cast<unsigned long long>(__double_as_longlong(v)),
                     __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ double readPartial(const double* p) {
  return __longlong_as_double(static_cast<long long>(__hip_atomic_load(
      reinterpret_cast<const unsigned long long*>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)));
}
__device__ __forceinline__ bool lastBlockArrivesLite(unsigned int* counter, unsigned int total, int* flag) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // every wave: its published partials have landed
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned int t = __hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const bool last = (t == total - 1);
    if (last) __hip_atomic_store(counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // re-arm for the next launch
    *flag = last ? 1 : 0;
  }
  __syncthreads();
  return *flag != 0;
}
// sum of n published partials by the whole (last) workgroup; `red` = 16 doubles of LDS
__device__ __forceinline__ double blockSumPartials(const double* __restrict__ a, int n, double* red) {
  double acc = 0.0;
  for (int i = threadIdx.x; i < n; i += blockDim.x) acc += readPartial(a + i);
  acc = waveSum(acc);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  double t = 0.0;
  for (int w = 0; w < (blockDim.x >> 6); ++w) t += red[w];
  __syncthreads();
  return t;
}

// ---- what the host hands to the kernels of the side headers (cvd_coarse.h, cvd_cross.h, cvd_triplets.h) ----
constexpr size_t kCoarseMaxUnknowns = 65536;  // 8192 frames (the plan is built on the host in O(F^2))
constexpr int kCBB = kCB * kCB;   // doubles per coarse block (kCB = 8 coarse unknowns per frame, cvd_device.h)
// Elimination plan (device pointers, built by the host in buildCoarsePlan).  Indices are elimination POSITIONS
// unless stated otherwise.  Block ids: [0, F) diagonal block of position j, F + e off-diagonal block e of L.
struct CoarsePlan {
  int F, nBlocks, nLevels, nEdges;
  const int* order;      // position -> frame
  const int* pos;        // frame -> position
  const int* levelPtr;   // nLevels + 1, into levelCols
  const int* levelCols;  // positions grouped by level (columns of one level are mutually independent)
  const int* lvlBlkPtr;  // nLevels + 1, into lvlBlks: every block (diagonal and below) of the level's columns
  const int* lvlBlks;    // block ids
  const int* blkCol;     // block id -> column position j
  const int* blkRow;     // block id -> row position i (>= j)
  const int* colPtr;     // F + 1: off-diagonal blocks below the diagonal of column j are ids F + [colPtr[j], colPtr[j+1])
  const int* rowPtr;     // F + 1: off-diagonal blocks of ROW j (left of the diagonal)
  const int* rowBlk;     //   their block ids
  const int* updPtr;     // nBlocks + 1: left-looking update list of block (i, j): pairs L(i,k), L(j,k), k < j
  const int* updA;       //   block id of L(i, k)
  const int* updB;       //   block id of L(j, k)
  const int* edgeBlk;    // nEdges: (block id << 1) | transposed   (edge block is stored rows = fa, cols = fb)
  const int* edgeFa;     // nEdges
  const int* edgeFb;     // nEdges
  // W = L^-1: column j holds blocks at rows path(j) = j, parent(j), parent(parent(j)), ... (W block id = wPtr[j] + t)
  const int* wPtr;       // F + 1
  const int* wRow;       // row position of every W block
  const int* wtPtr;      // F + 1: W blocks of ROW i (transpose structure), ordered by column
  const int* wtBlk;      //   W block id
  const int* wtCol;      //   column position
  const int* wtFrame;    //   frame of that column (order[wtCol])
  const int* wuPtr;      // nW + 1: gather list of W block (i, j): pairs L(i,k) W(k,j), k on the path below i
  const int* wuL;        //   block id of L(i, k)
  const int* wuW;        //   W block id of W(k, j)
  int nW;                // number of W blocks
  const int* updBlk;     // per update entry: the block id it belongs to (inverse of updPtr)
};

// Undirected frame pairs of the explicit-block mode: ranges of both directions' pixel slots (either may be empty) and the
// two rows of the partial-product buffer.
struct CrossPairs {
  const int* fa;            // fa < fb
  const int* fb;
  const long long* range;   // 4 per pair: [a -> b begin, end, b -> a begin, end) pixel slots
  const int* slot;          // 2 per pair: rows of the partial buffer (frame-major)
  int count;
};

struct TripletTable {
  const float2* ndc;       // 3 per constraint
  const float* dsrc;       // 3 per constraint, dsrc[3c] <= 0: constraint inactive
  const unsigned char* isStatic;
  const long long* off;    // per group: [2g] begin, [2g+1] end of its constraints
  const int* center;       // per group: centre frame (frames centre-1, centre, centre+1)
  const int* slot;         // 3 per group: rows of the partial-product buffer
  int nGroups;
  int smoothType;          // cvd_smooth_loss_type
  double wStaticSqrt, wDynamicSqrt;
};

enum : int { kSmoothEuclidLaplacian = 0, kSmoothDisparityLaplacian = 1, kSmoothDepthRatio = 2, kSmoothLogDepth = 3 };

__device__ __forceinline__ int packedIdx(int i, int j) {  // i >= j
  return i * (i + 1) / 2 + j;
}

// Row panels of the packed lower triangle for k_assemble / k_assemble_triplets: the triangle of a frame block
// (B (B + 1) / 2 doubles: 162 KB at B = 201, the reference's default deferred-spatial layout 7 + 170 + 24) no longer
// fits the 160 KB of LDS beyond B = 199, so the kernels accumulate it panel by panel -- rows [row[k], row[k + 1]) per
// pass over the frame's constraints (the Jacobians are re-evaluated per pass; one pass whenever the triangle fits).
struct AsmPanels {
  int n;
  int row[9];  // n + 1 boundaries, row[0] = 0, row[n] = B
};

typedef double cvd_d4 __attribute__((ext_vector_type(4)));  // f64 MFMA accumulator (block inverses, dense inverse, dense walk)

// ---------------------------------------------------------------------------------------------------
// Matrix-free product, pair-major (THE hot kernel): for the work item's constraints
//   t = rho' (J_a p_a + J_b p_b),  q_a += J_a^T t,  q_b += J_b^T t
// with J re-derived analytically from 24 B per constraint.  p is formed on the fly as z + beta p_old
// (beta lives on the device), masked for constant parameters.  Partials go to a per-item slot; the
// per-frame reduction (k_matvec_finish) is a gather, so there are no global atomics.
// ---------------------------------------------------------------------------------------------------
template <int KD, int KS>
inline __global__ __launch_bounds__(256) void k_matvec_pairs(Layout L, Table T, Items it, const double* __restrict__ x,
                                                      const FrameConst* __restrict__ fc,
                                                      const double* __restrict__ mask, const double* __restrict__ z,
                                                      const double* __restrict__ pOld,
                                                      const double* __restrict__ scal, int useBeta,
                                                      double* __restrict__ qPart, CoarseView V) {
  if (scal[S_DONE] != 0.0) return;  // PCG already converged (iterations enqueued ahead)
  extern __shared__ __attribute__((aligned(16))) double sm[];
  const int B = L.B;
  double* xa = sm;
  double* xb = xa + B;
  double* pa = xb + B;
  double* pb = pa + B;
  double* qa = pb + B;
  double* qb = qa + B;
  FrameConst* fcs = reinterpret_cast<FrameConst*>(qb + B);
  double* cl = reinterpret_cast<double*>(fcs + 2) + 18 + 4 * 24 + 8;  // 2 x kCB coarse corrections
  const int item = blockIdx.x;
  const int tid = threadIdx.x;
  const int fa = it.fa[item], fb = it.fb[item];
  const double beta = useBeta ? scal[S_BETA] : 0.0;
  // Prologue in ONE global round trip (the workgroup lives ~5 us, a dependent load costs ~1 us of it): every thread
  // issues its loads of x / z / p_old / mask for both frames, the coarse correction c_f (see CoarseView) and the
  // frame constants go to LDS in the same phase, and the search direction is formed after the barrier.  B <= 256:
  // one element per thread.
  constexpr int FCW = sizeof(FrameConst) / 8;
  if (V.Wb != nullptr) {  // (fused coarse variant: the correction is gathered here, one wave per frame)
    if (tid < 64) coarseFrameCorrection(V, fa, tid, cl);
    else if (tid < 128) coarseFrameCorrection(V, fb, tid - 64, cl + kCB);
  } else if (tid < 2 * kCB) {
    cl[tid] = (V.cF != nullptr) ? V.cF[(tid < kCB ? fa : fb) * kCB + (tid & (kCB - 1))] : 0.0;
  }
  if (tid >= 256 - 2 * FCW) {  // (the last waves: the first ones carry the coarse loads)
    const int t = tid - (256 - 2 * FCW);
    const int which = t / FCW, k = t % FCW;
    reinterpret_cast<double*>(fcs + which)[k] = reinterpret_cast<const double*>(fc + (which ? fb : fa))[k];
  }
  // (two elements per thread: B <= 512 -- the generic kernel serves the blocks beyond the fast kernels' 256)
  double vza[2] = {0.0, 0.0}, vzb[2] = {0.0, 0.0}, vpa[2] = {0.0, 0.0}, vpb[2] = {0.0, 0.0}, vma[2] = {0.0, 0.0}, vmb[2] = {0.0, 0.0};
#pragma unroll
  for (int e = 0; e < 2; ++e) {
    const int i = tid + e * 256;
    if (i < B) {
      const size_t ia = static_cast<size_t>(fa) * B + i, ib = static_cast<size_t>(fb) * B + i;
      xa[i] = x[ia];
      xb[i] = x[ib];
      vza[e] = z[ia];
      vzb[e] = z[ib];
      if (useBeta) { vpa[e] = pOld[ia]; vpb[e] = pOld[ib]; }
      vma[e] = mask[ia];
      vmb[e] = mask[ib];
      qa[i] = 0.0;
      qb[i] = 0.0;
    }
  }
  __syncthreads();
#pragma unroll
  for (int e = 0; e < 2; ++e) {
    const int i = tid + e * 256;
    if (i < B) {
      pa[i] = (vza[e] + coarseAtLds(cl, L, i) + (useBeta ? beta * vpa[e] : 0.0)) * vma[e];
      pb[i] = (vzb[e] + coarseAtLds(cl + kCB, L, i) + (useBeta ? beta * vpb[e] : 0.0)) * vmb[e];
    }
  }
  if (L.intrOpt == kIntrShared) {
    // every constraint's focal column is frame 0's slot (reference lib/PoseOptimizer.cpp:1226)
    __syncthreads();
    if (tid == 0) {
      const double p06 = (z[6] + (useBeta ? beta * pOld[6] : 0.0)) * mask[6];
      pa[6] = p06;
      pb[6] = p06;
    }
  }
  __syncthreads();
  for (int dir = 0; dir < 2; ++dir) {
  const long long cb = it.range[item * 4 + dir * 2], ce = it.range[item * 4 + dir * 2 + 1];
  if (cb >= ce) continue;
  // role swap for the reverse pair: source = fb, target = fa
  const FrameConst& Fs = fcs[dir];
  const FrameConst& Ft = fcs[dir ^ 1];
  const double* xs = dir ? xb : xa;
  const double* xt = dir ? xa : xb;
  const double* ps = dir ? pb : pa;
  const double* pt = dir ? pa : pb;
  double* qs = dir ? qb : qa;
  double* qt = dir ? qa : qb;
  double qpa[7], qpb[7];
#pragma unroll
  for (int i = 0; i < 7; ++i) { qpa[i] = 0.0; qpb[i] = 0.0; }
  for (long long c = cb + tid; c < ce; c += 256) {
    const float2 d = T.dsrc[c];
    if (!(d.x > 0.f)) continue;
    Sample<KD, KS> s;
    evalSample<KD, KS, true>(L, Fs, Ft, xs, xt, T.ndc[c], d, s);
    double t[3] = {0.0, 0.0, 0.0};
    sideJp(L, s.a, ps, t);
    sideJp(L, s.b, pt, t);
    t[0] *= s.rho1; t[1] *= s.rho1; t[2] *= s.rho1;
#pragma unroll
    for (int i = 0; i < 7; ++i) {
      qpa[i] += s.a.Jp[0][i] * t[0] + s.a.Jp[1][i] * t[1] + s.a.Jp[2][i] * t[2];
      qpb[i] += s.b.Jp[0][i] * t[0] + s.b.Jp[1][i] * t[1] + s.b.Jp[2][i] * t[2];
    }
    {
      const int nt = sideNumTapCols(L, s.a);
      for (int k = 0; k < nt; ++k) {
        int col;
        double J[3];
        sideTapCol(L, s.a, k, col, J);
        atomicAdd(&qs[col], J[0] * t[0] + J[1] * t[1] + J[2] * t[2]);
      }
    }
    {
      const int nt = sideNumTapCols(L, s.b);
      for (int k = 0; k < nt; ++k) {
        int col;
        double J[3];
        sideTapCol(L, s.b, k, col, J);
        atomicAdd(&qt[col], J[0] * t[0] + J[1] * t[1] + J[2] * t[2]);
      }
    }
  }
#pragma unroll
  for (int i = 0; i < 7; ++i) {
    qpa[i] = waveSum(qpa[i]);
    qpb[i] = waveSum(qpb[i]);
  }
  if ((tid & 63) == 0) {
#pragma unroll
    for (int i = 0; i < 7; ++i) {
      atomicAdd(&qs[i], qpa[i]);
      atomicAdd(&qt[i], qpb[i]);
    }
  }
  }  // dir
  __syncthreads();
  // rows are grouped by frame (slot = position in the frame's item list) so that k_matvec_finish streams them
  double* outA = qPart + static_cast<size_t>(it.slot[item * 2]) * B;
  double* outB = qPart + static_cast<size_t>(it.slot[item * 2 + 1]) * B;
  for (int i = tid; i < B; i += 256) {
    outA[i] = qa[i];
    outB[i] = qb[i];
  }
}

// Regulariser Jacobian cache: the rows of the per-frame regularisers depend on x only, so they are evaluated once per
// linearisation point (RegCache, filled by k_reg_cache) instead of once per product.  Entry a of residual i of
// frame f lives at (f * stride + a) * nr + i (consecutive threads = consecutive residuals).
struct RegCache {
  double* jac;
  unsigned short* col;
  unsigned char* cnt;
  int nr;      // residuals per frame
  int stride;  // entries per residual
};

// PCG scalars after the preconditioner has been applied (shared by k_cg_update and, with the coarse level, k_coarse_apply).
__device__ __forceinline__ void pcgFinishScalars(double* __restrict__ scal, int init, double rzs, double rrs, double tol2,
                                                 double* __restrict__ hostMirror) {
  double done, iters;
  if (init) {
    scal[S_RZ0] = rzs;
    scal[S_RZOLD] = rzs;
    scal[S_BETA] = 0.0;
    scal[S_TARGET] = tol2 * rzs;
    iters = 0.0;
    done = (rzs == rzs) ? ((rzs > 0.0) ? 0.0 : 1.0) : 2.0;
  } else {
    const double old = scal[S_RZ];
    scal[S_RZOLD] = old;
    scal[S_BETA] = (old != 0.0) ? rzs / old : 0.0;
    iters = scal[S_ITERS] + 1.0;
    done = scal[S_DONE];
    if (!(rzs == rzs)) done = 2.0;
    else if (rzs <= scal[S_TARGET]) done = 1.0;
  }
  scal[S_ITERS] = iters;
  scal[S_DONE] = done;
  scal[S_RZ] = rzs;
  scal[S_RR] = rrs;
  // Progress for the host in pinned, coherent memory, so that it can bound its run-ahead without any copy or event
  // in the stream: slot 1 + (iterations applied & 7) = 4 (iterations applied + 1) + the done flag after exactly that many
  // iterations (a ring: the host's decisions depend on the iteration count only, never on timing, which keeps the ranks
  // of a multi-GPU run enqueuing the same collectives).  ONE relaxed store carries both numbers: a release store after a
  // separate flag store was a system-scope write-back of the XCD's L2 (buffer_wbl2 sc0 sc1) at the end of every iteration.
  if (hostMirror != nullptr)
    __hip_atomic_store(hostMirror + 1 + (static_cast<int>(iters) & 7), 4.0 * (iters + 1.0) + done, __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_SYSTEM);
}

// =====================================================================================================
// Fast path of the hot kernel (identity spatial transform, reprojection losses, Identity / Global / bilinear
// depth transform = everything the reference's default pipeline uses).
//
// Same operator as k_matvec_pairs, restructured so that no 3x7 Jacobian is ever materialised:
//   forward  : dX = directional derivative of the world point along p_a, dq = R_b^T (dX - p_tb) + E_b^T v,
//              t = rho' * (d r / d q . dq + direct terms)            with E_f = sum_i p_w,i dR_f,i per frame
//   backward : y_q = (d r / d q)^T t, y_X = R_b y_q; translations get +-y_X, the rotation / focal / depth
//              columns are contracted per WORKGROUP from 3x3 outer-product accumulators
//              O_a = sum D_a y_X c_a^T, O_b = sum v y_q^T  (q_w,i = <dR_i, O>), so dR never enters the loop.
// Per-lane state: 23 accumulators; taps are fully unrolled (no scratch).
// =====================================================================================================
template <int KD>
struct FastTaps {
  int idx[KD];
  double w[KD];
  __device__ __forceinline__ bool ok(int) const { return true; }
  __device__ __forceinline__ int I(int k) const { return idx[k]; }
  __device__ __forceinline__ double Wt(int k) const { return w[k]; }
};

// bicubic: the 16 taps stay in separable form (8 weights + 3 ints instead of 16 + 16 registers); tap k = (k & 3, k >> 2)
// exists when it lies inside the folded xs x ys footprint, in the same row-major order as bicubicTaps enumerates.
template <>
struct FastTaps<16> {
  CubicSep s;
  int gx;
  __device__ __forceinline__ bool ok(int k) const { return (k & 3) < s.xs && (k >> 2) < s.ys; }
  __device__ __forceinline__ int I(int k) const { return s.base + (k & 3) + (k >> 2) * gx; }
  __device__ __forceinline__ double Wt(int k) const { return s.fx[k & 3] * s.fy[k >> 2]; }
};

// gridCell (cvd_device.h) in 6 instructions instead of 9, bit-identical: (loc + 1) is exact in double, so one FMA rounds the same
// real number as the product (loc + 1) * ((g - 1) / 2) does ((g - 1) / 2 is a half-integer: exact), and for the clamped s >= 0
// v_fract_f64 is s - trunc(s).  For the hot product's loop (four cells per constraint).
__device__ __forceinline__ void gridCellFast(float loc, double hg, double maxc, int& i, double& r) {
  double s = __builtin_fma(static_cast<double>(loc), hg, hg);
  s = fmin(fmax(s, 0.0), maxc);
  i = static_cast<int>(s);
  r = __builtin_amdgcn_fract(s);
}
template <int KD>
__device__ __forceinline__ void fastGather(const Layout& L, float lx, float ly, FastTaps<KD>& t) {
  if constexpr (KD == 16) {
    bicubicSeparable(lx, ly, L.gx, L.gy, L.maxcx, L.maxcy, t.s);
    t.gx = L.gx;
  } else if constexpr (KD == 4) {
    int ix, iy;
    double rx, ry;
    gridCellFast(lx, 0.5 * static_cast<double>(L.gx - 1), L.maxcx, ix, rx);
    gridCellFast(ly, 0.5 * static_cast<double>(L.gy - 1), L.maxcy, iy, ry);
    const int i0 = ix + iy * L.gx;
    t.idx[0] = i0;            t.w[0] = (1.0 - rx) * (1.0 - ry);
    t.idx[1] = i0 + 1;        t.w[1] = rx * (1.0 - ry);
    t.idx[2] = i0 + L.gx;     t.w[2] = (1.0 - rx) * ry;
    t.idx[3] = i0 + L.gx + 1; t.w[3] = rx * ry;
  } else {
    t.idx[0] = 0;
    t.w[0] = 1.0;
  }
}

// 1 / x to f64 accuracy (1-2 ulp; not correctly rounded): hardware estimate + two Newton steps, 5 instructions instead of the
// ~10 of the IEEE division sequence (div_scale x2, rcp, fma chain, div_fmas, div_fixup).  For the specialised constraint loops
// (the FAST policy of the constraint model below).
__device__ __forceinline__ double rcpFast(double x) {
  double r = __builtin_amdgcn_rcp(x);
  double e = __builtin_fma(-x, r, 1.0);
  r = __builtin_fma(r, e, r);
  e = __builtin_fma(-x, r, 1.0);
  return __builtin_fma(r, e, r);
}

// 1 / sqrt(x) the same way (hardware estimate + two Newton steps): the Huber weight of the specialised product.
__device__ __forceinline__ double rsqrtFast(double x) {
  double r = __builtin_amdgcn_rsq(x);
  const double h = 0.5 * x;
  double e = __builtin_fma(-h * r, r, 0.5);
  r = __builtin_fma(r, e, r);
  e = __builtin_fma(-h * r, r, 0.5);
  return __builtin_fma(r, e, r);
}

// A wave-uniform double as a scalar (SGPR pair): the compiler cannot prove that an LDS load is uniform.
__device__ __forceinline__ double uniformValue(double v) {
  return __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(v)), __builtin_amdgcn_readfirstlane(__double2loint(v)));
}

// =====================================================================================================
// The constraint model of the fast scope, stated ONCE.  A constraint a -> b with interpolated depths D_a, D_b:
//   q = R_b^T v, v = t_a + D_a R_a c_a - t_b;   z' = -q_z, (u, v') = (q_x / (z' fx_b), q_y / (z' fy_b));
//   r = (ws (u - p_b.x), ws (v' - p_b.y), wd r_depth(z', D_b)),   weight rho'(|r|^2)
// and the rows M = d r / d q of its Jacobian.  Users: k_cost_items_fast (value only), k_coarse_edges_fast, k_tl_edges,
// k_matvec_pairs_fast, the specialised walk of k_assemble_fast (asmWalkSpec) and dwChain of k_dense_walk.  The generic evalSample
// (cvd_device.h) is the independent statement the tests hold these against.  What differs between the users in the last bits
// stays at the call site: how v is summed (t_a - t_b pre-combined or not), the interpolated depths and the pose columns built
// on M.  The runtime-variant walk of k_assemble_fast (SPEC = 0) keeps its own text of the whole chain: through these functions
// its multiply-adds contracted differently and the bicubic variant's gradient moved in the last bits.  The one numeric policy
// here is FAST: hardware reciprocals + two Newton steps (rcpFast) for IEEE divisions.
// =====================================================================================================
template <bool FAST>
__device__ __forceinline__ double fastRcp(double x) {
  if constexpr (FAST) return rcpFast(x);
  else return 1.0 / x;
}

// the source ray c_a = (p_a.x fx_a, p_a.y fy_a, -1) and R_a c_a
__device__ __forceinline__ void fastRay(const double* Ra, double pax, double pay, double fxa, double fya, double (&ca)[3],
                                        double (&Rca)[3]) {
  ca[0] = pax * fxa;
  ca[1] = pay * fya;
  ca[2] = -1.0;
  Rca[0] = dot3(Ra, ca);
  Rca[1] = dot3(Ra + 3, ca);
  Rca[2] = dot3(Ra + 6, ca);
}

// projection into the target frame: z' (zz), 1 / z' (iz), the normalised image point (u, vv) and the two reprojection residuals
template <bool FAST>
__device__ __forceinline__ void fastProject(const Layout& L, const double* Rb, const double (&v)[3], double ifxb, double ifyb,
                                            double pbx, double pby, double& zz, double& iz, double& u, double& vv, double& r0,
                                            double& r1) {
  const double q0 = Rb[0] * v[0] + Rb[3] * v[1] + Rb[6] * v[2];
  const double q1 = Rb[1] * v[0] + Rb[4] * v[1] + Rb[7] * v[2];
  const double q2 = Rb[2] * v[0] + Rb[5] * v[1] + Rb[8] * v[2];
  zz = -q2;
  iz = fastRcp<FAST>(zz);
  u = q0 * iz * ifxb;
  vv = q1 * iz * ifyb;
  r0 = (u - pbx) * L.ws;
  r1 = (vv - pby) * L.ws;
}

// depth residual r2 of the three reprojection losses with d r2 / d z' (dr2dA) and d r2 / d D_b.  Disparity: 1 / max(z', eps) -
// 1 / max(D_b, eps), a clamped side has no derivative; Ratio: max / min - 1; LogRatio: log(min / max); at a tie z' = D_b both
// one-sided derivatives count (zIsMax and zIsMin).  A value-only user drops the derivatives.
template <bool FAST>
__device__ __forceinline__ void fastDepthResidual(const Layout& L, int lossType, double zz, double iz, double Db, double& r2,
                                                  double& dr2dA, double& dr2dDb) {
  constexpr double eps = 1e-6;
  if (lossType == kLossDisparity) {
    const bool zo = !(zz < eps), bo = !(Db < eps);
    const double bc = bo ? Db : eps;
    const double izc = zo ? iz : 1.0 / eps, ibc = fastRcp<FAST>(bc);
    r2 = (izc - ibc) * L.wd;
    dr2dA = zo ? (-L.wd * izc * izc) : 0.0;
    dr2dDb = bo ? (L.wd * ibc * ibc) : 0.0;
  } else {
    const bool zIsMax = !(zz < Db), zIsMin = !(Db < zz);
    const double mx = zIsMax ? zz : Db, mn = zIsMin ? zz : Db;
    if (lossType == kLossRatio) {
      r2 = (mx / mn - 1.0) * L.wd;
      const double dmx = 1.0 / mn, dmn = -mx / (mn * mn);
      dr2dA = ((zIsMax ? dmx : 0.0) + (zIsMin ? dmn : 0.0)) * L.wd;
      dr2dDb = ((zIsMax ? 0.0 : dmx) + (zIsMin ? 0.0 : dmn)) * L.wd;
    } else {
      r2 = log(mn / mx) * L.wd;
      const double dmn = 1.0 / mn, dmx = -1.0 / mx;
      dr2dA = ((zIsMax ? dmx : 0.0) + (zIsMin ? dmn : 0.0)) * L.wd;
      dr2dDb = ((zIsMax ? 0.0 : dmx) + (zIsMin ? 0.0 : dmn)) * L.wd;
    }
  }
}

// rho' with the robustifier fixed at compile time.  SPEC 1: Cauchy, what the reference hard-wires; SPEC 2: Huber, BASELINE
// configs[4]'s stress variant -- rho' = a / sqrt(s) beyond s = a^2, clamped like ceres::HuberLoss; SPEC 0: the runtime choice.
// (Huber: the reciprocal root is a statement of its own, on an argument that is valid on both sides of s = a^2 -- selects, no
// branch, in a loop that sits at its register budget.)
template <int SPEC>
__device__ __forceinline__ double fastRobustRho1(const Layout& L, double sq) {
  if constexpr (SPEC == 1) return rcpFast(1.0 + sq * L.cauchyC);
  else if constexpr (SPEC == 2) {
    const bool outer = sq > L.cauchyB;
    const double irt = rsqrtFast(outer ? sq : 1.0);
    return outer ? fmax(2.2250738585072014e-308, L.robustA * irt) : 1.0;
  }
  else return robustRho1(L, sq);
}
// ... and rho itself for the two compile-time forms, written out on the same intermediates (a user of both pays for them once;
// a separate function so that the caller can keep the logarithm under its own condition)
template <int SPEC>
__device__ __forceinline__ double fastRobustRho0(const Layout& L, double sq) {
  static_assert(SPEC == 1 || SPEC == 2, "the runtime choice goes through robustRho");
  if constexpr (SPEC == 1) {
    return L.cauchyB * log(1.0 + sq * L.cauchyC);
  } else {
    const bool outer = sq > L.cauchyB;
    const double irt = rsqrtFast(outer ? sq : 1.0);
    return outer ? (2.0 * L.robustA * (sq * irt) - L.cauchyB) : sq;
  }
}

// d r / d q (rows): M0 = (m00, 0, m02), M1 = (0, m11, m12), M2 = (0, 0, m22) with m22 = -dr2dA (the caller's)
__device__ __forceinline__ void fastRows(const Layout& L, double iz, double u, double vv, double ifxb, double ifyb, double& m00,
                                         double& m11, double& m02, double& m12) {
  const double wiz = L.ws * iz;
  m00 = wiz * ifxb;
  m11 = wiz * ifyb;
  m02 = wiz * u;
  m12 = wiz * vv;
}

// One wave's sum of the kPcgSharesCap shares in a FIXED order (lane l holds words l, l + 64, ..., l + 448): the lane's eight in a
// tree, then waveSum.  Every workgroup of the product and k_pcg_close get the same bits.
__device__ __forceinline__ double pcgSharesSum(const double (&w)[8]) {
  return waveSum(((w[0] + w[1]) + (w[2] + w[3])) + ((w[4] + w[5]) + (w[6] + w[7])));
}
// The bookkeeping of pcgFinishScalars for an iteration whose r^T z was summed from the shares (one thread: workgroup 0 of the next
// product, or k_pcg_close behind the last tail): `applied` iterations are through, rzs is the new r^T z, old the one before.
__device__ __forceinline__ void pcgCloseFromShares(double* scal, int applied, double rzs, double old, double beta, double done,
                                                   double* hostMirror) {
  scal[S_RZOLD] = old;
  scal[S_BETA] = beta;
  scal[S_ITERS] = static_cast<double>(applied);
  scal[S_DONE] = done;
  scal[S_RZ] = rzs;
  scal[SH_RING + (applied & 1)] = rzs;
  if (hostMirror != nullptr)
    __hip_atomic_store(hostMirror + 1 + (applied & 7), 4.0 * (static_cast<double>(applied) + 1.0) + done, __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_SYSTEM);
}
// The product's first wave behind the sum: beta and the stop flag (1: converged, NaN or an abandoned barrier -- the launch writes
// nothing) of iteration `applied`; ctl = lane 0 .. 4: r^T z before the sum, S_TARGET, SH_ABANDON, SH_MIRROR, S_DONE.  Thread 0 of
// workgroup 0 does the bookkeeping -- unless the PCG was done before the launch (later iterations are no-ops) or a grid barrier
// was abandoned (the mirror stalls, the host falls back: nobody advances S_ITERS).
__device__ __forceinline__ void pcgSharesClose(const double* scal, int applied, double rzs, double ctl, double& beta, double& stop) {
  const double old = readLane(ctl, 0), target = readLane(ctl, 1), abandon = readLane(ctl, 2), mirror = readLane(ctl, 3);
  const double sDone = readLane(ctl, 4);
  double done = sDone;
  if (done == 0.0) done = !(rzs == rzs) ? 2.0 : (rzs <= target ? 1.0 : 0.0);
  beta = (old != 0.0) ? rzs / old : 0.0;
  stop = (done != 0.0 || abandon != 0.0) ? 1.0 : 0.0;
  if (__builtin_expect(blockIdx.x == 0 && threadIdx.x == 0 && sDone == 0.0 && abandon == 0.0, 0))
    // (`scal` is const in the kernel's signature, which all forms share; the array is the handle's own and writable, the pointer is
    // derived from the restrict-qualified argument itself, and every read of the launch's first wave lies in front of these stores)
    pcgCloseFromShares(const_cast<double*>(scal), applied, rzs, old, beta, done,
                       reinterpret_cast<double*>(static_cast<unsigned long long>(__double_as_longlong(mirror))));
}

#ifdef CVD_MV_PROFILE  // tools/mv_profile.py: wall-clock (100 MHz) stamps of the hot product's workgroups
__device__ unsigned long long g_mvProf[4096 * 8];
#define MV_STAMP(slot) do { if ((threadIdx.x & 63) == 0) g_mvProf[(blockIdx.x & 4095) * 8 + (slot)] = wall_clock64(); } while (0)
#else
#define MV_STAMP(slot) do {} while (0)
#endif
constexpr int kRedVals = 15;               // accumulators of k_matvec_pairs_fast reduced per workgroup (11 + the 4 depth-block sums of KD = 1)
constexpr int kRedStride = 4 * 33 + 1;     // 128 columns (lane pairs pre-summed) in 33-padded segments of 32, +1 skew

// SPEC = 2: the same with the Huber robustifier (round 5: configs[4]'s Huber variant ran the generic-loss kernel at 253 us
// per product against 149 us for Cauchy).
// SPEC = 1: the default pipeline's variant fixed at compile time (one value parameter per vertex, ReproDisparity loss,
// Cauchy robustifier): the branches on the runtime Layout fields drop out of the constraint loop.
#ifndef CVD_MV_WAVES
#define CVD_MV_WAVES 4   // waves per SIMD the specialised list-mode product (Global / bilinear) is compiled for (round 5: 129 -> 128
                         // VGPRs; 3 = rounds 2-4 and still the bicubic and dense variants, which spill at 128)
#endif
#ifndef CVD_MV_EARLY
#define CVD_MV_EARLY 1   // 1: direction 0's first table record is requested at the top of the kernel
#endif
// SHARES (list mode; chosen per launch by launchMatvec): the tail of the previous iteration left its shares of r^T z unsummed
// (SH_RZ above) and `useBeta` carries the iteration's index k >= 1.  The first wave of every workgroup requests the shares in the
// prologue's load phase and sums them in a fixed order, so all workgroups form bit-identical beta = r^T z / (the sum before: SH_RING,
// S_RZ0 for k = 1) and the same convergence flag; workgroup 0 writes the scalars and the host mirror as pcgFinishScalars would have.
// S_DONE may be read stale or fresh by the others: a flag that was set before this launch returns everybody (the writer then writes
// nothing), and a fresh one is the value the reader computes itself.
template <int KD, int NT, int SPEC = 0, bool DENSE = false, bool SHARES = false>
inline __global__ __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(SPEC ? ((KD <= 4 && !DENSE) ? CVD_MV_WAVES : 3) : 2))) void k_matvec_pairs_fast(Layout L, Table T, Items it, const double* __restrict__ x,
                                                           const FrameConst* __restrict__ fc,
                                                           const double* __restrict__ mask,
                                                           const double* __restrict__ z, const double* __restrict__ pOld,
                                                           const double* __restrict__ scal, int useBeta,
                                                           double* __restrict__ qPart, CoarseView V) {
  // (PCG already converged: iterations enqueued ahead return -- tested after the prologue's loads have been issued, so
  // that the flag does not cost a dependent global round trip of its own in every working launch)
  double sDone = 0.0;
  if constexpr (!SHARES) sDone = scal[S_DONE];   // (SHARES: one of the first wave's words below)
  extern __shared__ __attribute__((aligned(16))) double sm[];
  constexpr int NV = KD == 1 ? kRedVals : 11;  // the depth-block sums exist only with one tap per side
  const int B = L.B;
  if (threadIdx.x == 0) MV_STAMP(0);
  double* xa = sm;
  double* xb = xa + B;
  double* pa = xb + B;
  double* pb = pa + B;
  double* qa = pb + B;
  double* qb = qa + B;
  double* fix = qb + B;                            // t, fy, J_l of both frames for the epilogue (2 x 13 of the 2 x 49 doubles reserved)
  double* red = fix + 2 * sizeof(FrameConst) / 8;  // the reduced accumulators
  double* W = red + 32;                            // transposed reduction scratch: kRedVals rows x kRedStride
  // Dense mode: neighbouring lanes are neighbouring pixels and hit the SAME grid vertices -- 64-way same-address LDS
  // atomics.  The grid columns are therefore accumulated into kPriv lane-keyed private copies (after W) and folded
  // before the epilogue.
  constexpr int kPriv = DENSE ? 8 : 1;   // (list mode: 2 lane-keyed copies 52.6 -> 51.4 us in raster order, nothing once the table is cell-ordered)
  constexpr bool kUsePriv = kPriv > 1;
  double* qpriv = W + static_cast<size_t>(kRedVals) * kRedStride;  // DENSE: [kPriv][2][B]
  double* cl = W;                                  // prologue only: 2 x kCB coarse corrections
  const int item = blockIdx.x;
  const int tid = threadIdx.x;
  // frames, constraint ranges and output rows of the item: ONE scalar load (four arrays were four, and `range` / `slot` were
  // loaded again behind the barriers of the loop and of the write-out)
  const ItemRecord* __restrict__ recp = it.rec + item;
  const int fa = recp->fa, fb = recp->fb;
  const int slotA = recp->slotA, slotB = recp->slotB;
  const long long cbD[2] = {recp->b0, recp->b1}, ceD[2] = {recp->e0, recp->e1};
  double beta = 0.0;
  if constexpr (!SHARES) beta = useBeta ? scal[S_BETA] : 0.0;   // (SHARES: formed behind the first barrier)
  // The frame constants (R, t, fy, J_l of both frames) are wave-uniform READ-ONLY global data at an address that depends on
  // blockIdx only: the compiler fetches them with scalar loads straight into SGPRs (round 5; rounds 2-4 staged the two structs in
  // LDS and moved 26 doubles per direction into SGPRs through v_readfirstlane: ~200 instructions per wave and direction).
  // (Staged in LDS instead, same box, 4140-pair set: 41.4 / 41.9 us against 39.6; without the early request below 40.8.)
  const FrameConst* __restrict__ fcF[2] = {fc + fa, fc + fb};
  // The first table record of direction 0 is requested before anything else: it is back when the prologue's barriers are.
  // (not the bicubic variant: six more live registers through the prologue spill at its budget; nor the one-wave workgroups of the
  // shares mode, for the same reason)
  constexpr bool kEarlyPrime = KD <= 4 && CVD_MV_EARLY && !(SHARES && NT == 64);
  RecordStream<DENSE> rs;   // (list mode: the next trip's table record is in flight during this trip's arithmetic)
  if constexpr (kEarlyPrime) rs.primeClamped(T, cbD[0], tid, static_cast<int>(ceD[0] - cbD[0]));
  // SHARES: the first wave's eight shares per lane (the whole array: the words beyond the solve's share count are zero), requested
  // in FRONT of the phase's other loads -- the waits those need cover them, the sum behind the phase needs none of its own -- and,
  // one word per lane 0 .. 4 (the lanes beyond repeat the last), what the closing needs beside them: r^T z before the sum (the ring slot this launch does not write;
  // the first iteration's is the first residual's), S_TARGET, the abandon word, the mirror's address and S_DONE.  All of it stays in the
  // first wave's vector registers: the loop's scalar registers are what this kernel is short of.  One-wave workgroups (the
  // deterministic build) close at once, a round trip of their own in front of everything else: sixteen registers held across
  // the phase do not fit beside their four elements of eight vectors per thread.
  double vsh[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  double vctl = 0.0, shBeta = 0.0, shStop = 0.0;
  if constexpr (SHARES) {
    if (tid < 64) {
      const double* __restrict__ sh = scal + SH_RZ + tid;
#pragma unroll
      for (int u = 0; u < 8; ++u) vsh[u] = sh[u * 64];
      const int prevAt = useBeta == 1 ? static_cast<int>(S_RZ0) : SH_RING + ((useBeta - 1) & 1);
      vctl = scal[tid == 0 ? prevAt : (tid == 1 ? static_cast<int>(S_TARGET) : (tid == 2 ? static_cast<int>(SH_ABANDON) : (tid == 3 ? static_cast<int>(SH_MIRROR) : static_cast<int>(S_DONE))))];
      if constexpr (NT == 64) {
        pcgSharesClose(scal, useBeta, pcgSharesSum(vsh), vctl, shBeta, shStop);
        if (tid == 0) {
          red[0] = shBeta;
          red[1] = shStop;
        }
        __builtin_amdgcn_sched_barrier(0);   // (the phase's loads stay behind: the seventeen registers are free again)
      }
    }
  }
  // Prologue in ONE global round trip (the workgroup lives ~5 us, a dependent load costs ~1 us of it): every thread
  // issues its loads of x / z / p_old / mask for both frames, the coarse correction c_f (see CoarseView), the third level's
  // coefficients and taps and the epilogue's frame constants in the same phase, and the search direction is formed after the
  // barrier.  B <= 256: one element per thread (two / four at 128 / 64 threads).
  // Every load below is issued UNCONDITIONALLY, into registers, from an address that is clamped or replaced so that it lies
  // inside its buffer (thread beyond B: element 0 of the frame's row; level off / first product of a solve: x, which always
  // holds F x B >= 2 doubles); the LDS stores follow the one wait and are predicated instead.  A load in a divergent block in
  // front of its own LDS store is waited for inside that block: the phases used to run one after the other, four round trips.
  constexpr int EPT = 256 / NT;  // elements of a frame block per thread (B <= 256)
  constexpr int TLE = (2 * kTlMaxS + NT - 1) / NT;  // third-level coefficients per thread (2 x tlS <= 2 kTlMaxS)
  const bool fusedCoarse = V.Wb != nullptr;
  const bool tlOn = V.tl != nullptr;
  const size_t rowA = static_cast<size_t>(fa) * B, rowB = static_cast<size_t>(fb) * B;
  double vcf;   // coarse correction c_f of both frames (threads < 2 kCB keep it)
  {
    const int k = tid & (2 * kCB - 1);
    vcf = *(V.cF != nullptr ? V.cF + static_cast<size_t>(k < kCB ? fa : fb) * kCB + (k & (kCB - 1)) : x);
  }
  // third level (CoarseView::tl): the two frames' coefficients go to LDS behind the coarse corrections, the thread's vertex
  // taps to registers -- same round trip as everything else here
  double* tls = cl + 2 * kCB;
  double vtl[TLE];
#pragma unroll
  for (int e = 0; e < TLE; ++e) {
    const int i = tid + e * NT;
    const int ic = (tlOn && i < 2 * V.tlS) ? i : 0;
    const int which = ic >= V.tlS ? 1 : 0;
    vtl[e] = *(tlOn ? V.tl + static_cast<size_t>(which ? fb : fa) * V.tlS + (ic - which * V.tlS) : x);
  }
  TlTaps tt[EPT];
#pragma unroll
  for (int e = 0; e < EPT; ++e) {
    const int i = tid + e * NT;
    const bool in = i >= 7 && i < 7 + L.nD;
    const int v = in ? i - 7 : 0;
    tt[e].w = *(tlOn ? V.tlW + v : reinterpret_cast<const float4*>(x));
    tt[e].idx = *(tlOn ? V.tlIdx + v : reinterpret_cast<const unsigned int*>(x));
    if (!in) tt[e].w = make_float4(0.f, 0.f, 0.f, 0.f);
  }
  // what the epilogue's pose-row fix-up needs of the two frames' constants (t, fy, J_l: 13 consecutive doubles of FrameConst)
  // is staged in LDS here: read there, behind the reduction's barrier, it was a global round trip of its own
  constexpr int kFix = 13;
  static_assert(offsetof(FrameConst, fy) == offsetof(FrameConst, t) + 24 && offsetof(FrameConst, Jl) == offsetof(FrameConst, t) + 32,
                "t, fy, Jl are consecutive");
  const int fixK = NT - 1 - tid;   // (the last threads: the first ones keep the coarse correction)
  double vfix;
  {
    const int k = fixK < 2 * kFix ? fixK : 0;
    vfix = (reinterpret_cast<const double*>(fc + (k >= kFix ? fb : fa)) + offsetof(FrameConst, t) / 8)[k >= kFix ? k - kFix : k];
  }
  double vxa[EPT], vxb[EPT], vza[EPT], vzb[EPT], vpa[EPT], vpb[EPT], vma[EPT], vmb[EPT];
  const double* __restrict__ pOldOrZ = useBeta ? pOld : z;   // (useBeta = 0: pOld may be unset and is not read)
#pragma unroll
  for (int e = 0; e < EPT; ++e) {
    const int i = tid + e * NT;
    const size_t ia = rowA + (i < B ? i : 0), ib = rowB + (i < B ? i : 0);
    vxa[e] = x[ia];
    vxb[e] = x[ib];
    vza[e] = z[ia];
    vzb[e] = z[ib];
    vpa[e] = pOldOrZ[ia];
    vpb[e] = pOldOrZ[ib];
    vma[e] = mask[ia];
    vmb[e] = mask[ib];
  }
  // (shared intrinsics: frame 0's focal slot, wave-uniform)
  const double z6 = z[6], po6 = pOldOrZ[6], m6 = mask[6];
  if (fusedCoarse) {  // (fused coarse variant, off by default: the correction is gathered here, one wave per frame)
    if (tid < 64) coarseFrameCorrection(V, fa, tid, cl);
    if (NT == 64) coarseFrameCorrection(V, fb, tid, cl + kCB);   // (one-wave workgroups of the deterministic build)
    else if (tid >= 64 && tid < 128) coarseFrameCorrection(V, fb, tid - 64, cl + kCB);
  }
  // ---- the one wait; from here on the prologue touches LDS only
  if (!fusedCoarse && tid < 2 * kCB) cl[tid] = (V.cF != nullptr) ? vcf : 0.0;
#pragma unroll
  for (int e = 0; e < TLE; ++e) {
    const int i = tid + e * NT;
    if (tlOn && i < 2 * V.tlS) tls[i] = vtl[e];
  }
  if (fixK < 2 * kFix) fix[fixK] = vfix;
#pragma unroll
  for (int e = 0; e < EPT; ++e) {
    const int i = tid + e * NT;
    if (i < B) {
      xa[i] = vxa[e];
      xb[i] = vxb[e];
      qa[i] = 0.0;
      qb[i] = 0.0;
    }
  }
  if constexpr (kUsePriv)
    for (int i = tid; i < kPriv * 2 * B; i += NT) qpriv[i] = 0.0;
  if constexpr (SHARES) {
    if (tid < 64) {  // beta and the stop flag for the workgroup through LDS (red is the reduction's: free until the loop is through)
      if constexpr (NT > 64) {
        pcgSharesClose(scal, useBeta, pcgSharesSum(vsh), vctl, shBeta, shStop);
        if (tid == 0) {
          red[0] = shBeta;
          red[1] = shStop;
        }
      }
    }
  }
  __syncthreads();
  if constexpr (SHARES) {
    beta = red[0];
    if (uniformValue(red[1]) != 0.0) return;  // uniform; only workgroup 0 has written (the scalars)
  } else {
    if (sDone != 0.0) return;  // uniform; nothing has been written to global memory yet
  }
#pragma unroll
  for (int e = 0; e < EPT; ++e) {
    const int i = tid + e * NT;
    if (i < B) {
      double ca = coarseAtLds(cl, L, i), cb2 = coarseAtLds(cl + kCB, L, i);
      if (tlOn) {
        ca += tlAt(tls, tt[e]);
        cb2 += tlAt(tls + V.tlS, tt[e]);
      }
      pa[i] = (vza[e] + ca + (useBeta ? beta * vpa[e] : 0.0)) * vma[e];
      pb[i] = (vzb[e] + cb2 + (useBeta ? beta * vpb[e] : 0.0)) * vmb[e];
    }
  }
  if (L.intrOpt == kIntrShared) {
    // every constraint's focal column is frame 0's slot (reference lib/PoseOptimizer.cpp:1226)
    __syncthreads();
    if (tid == 0) {
      const double p06 = (z6 + (useBeta ? beta * po6 : 0.0)) * m6;
      pa[6] = p06;
      pb[6] = p06;
    }
  }
  __syncthreads();
  // Rotation derivatives in CROSS-PRODUCT form (round 5).  R(w) = exp([w]x)  =>  dR/dw_i = [a_i]x R with a_i the i-th column of
  // the left Jacobian of SO(3) (FrameConst::Jl, read off dR_i R^T by k_frame_consts).  With e = sum_i p_w,i a_i
  //   forward   source: sum_i p_w,i dR_i c = e x (R c);   target: sum_i p_w,i dR_i^T v = R^T (v x e)
  //   adjoint   source: y . dR_i (D c)   = a_i . ((D R c) x y);   target: y_q . dR_i^T v = -a_i . (v x R y_q)
  // so a constraint contributes ONE cross product v x y_X to the rotation rows of both frames (3 accumulators and 6
  // instructions instead of the two 3 x 3 outer products: 18 accumulators, 21 instructions), the 18 E entries of a trip's LDS
  // broadcast reads become 6 scalars, and the workgroup reduction carries 11 values instead of 23.
  if (threadIdx.x == 0) MV_STAMP(1);

  const int N = SPEC ? 1 : L.N;
  const int lossType = SPEC ? static_cast<int>(kLossDisparity) : L.lossType;
  const double A = L.aspect;
  // The pose-level accumulators serve both directions through ONE reduction: aT = sum y_X of the running direction (the
  // translation adjoint: q_t,src = +aT, q_t,tgt = -aT; direction 0's sum is parked in aT0, the rotation rows need both),
  // Cx = sum v x y_X (negated between the directions: source and target swap), the focal sums per ROLE (swapped).
  double aT[3] = {0, 0, 0}, aT0[3] = {0, 0, 0};
  double Cx[3] = {0, 0, 0};
  double aFa = 0.0, aFb = 0.0;  // (unnormalised: x 1 / fy of the frame in the epilogue)
  double gDa[2] = {0.0, 0.0}, gDb[2] = {0.0, 0.0};  // KD == 1: every sample hits the one depth block -> registers
  const long long units0 = (ceD[0] - cbD[0] + 63) >> 6;  // wave-units of direction 0
  for (int dir = 0; dir < 2; ++dir) {
  const long long cb = cbD[dir], ce = ceD[dir];
  // role swap for the reverse pair (source = fb, target = fa): swap every per-frame pointer
  const FrameConst& Fa = *fcF[dir];
  const FrameConst& Fb = *fcF[dir ^ 1];
  if (dir) {
    double* t;
    t = xa; xa = xb; xb = t;
    t = pa; pa = pb; pb = t;
    t = qa; qa = qb; qb = t;
#pragma unroll
    for (int i = 0; i < 3; ++i) { aT0[i] = aT[i]; aT[i] = 0.0; Cx[i] = -Cx[i]; }
    { const double o = aFa; aFa = aFb; aFb = o; }
#pragma unroll
    for (int n = 0; n < 2; ++n) { const double o = gDa[n]; gDa[n] = gDb[n]; gDb[n] = o; }
  }
  const int firstUnit = dir == 0 ? (tid >> 6) : static_cast<int>(((tid >> 6) - units0) & (NT / 64 - 1));
  const int nDir = static_cast<int>(ce - cb);
  const int iFirst = firstUnit * 64 + (tid & 63);
  if (dir || !kEarlyPrime) rs.prime(T, cb, iFirst, nDir);   // (direction 0: requested at the top of the kernel; here: before the scalar set-up)
  // The frame constants are the same for every lane and reach the loop as SCALAR values (scalar loads; a VALU instruction
  // takes one scalar operand).  Rotations and translations of both frames are 24 doubles = 48 VGPRs less per lane.
  double RaU[9], RbU[9], dTU[3];
#pragma unroll
  for (int i = 0; i < 9; ++i) { RaU[i] = uniformValue(Fa.R[i]); RbU[i] = uniformValue(Fb.R[i]); }
#pragma unroll
  for (int i = 0; i < 3; ++i) dTU[i] = uniformValue(Fa.t[i] - Fb.t[i]);
  // (round 5: the rotation parts of the search direction are 3 + 3 scalars -- e = J_l^T p_w of both frames -- and its
  // translation / focal parts another 5; as 18 + 14 values they overflowed the SGPR file and were LDS broadcast reads inside
  // the loop.  Every wave forms them itself from the LDS copy of p: 18 multiply-adds instead of a barrier)
  double eaU[3], ebU[3], dptU[3];
  {
    const double pwa[3] = {uniformValue(pa[3]), uniformValue(pa[4]), uniformValue(pa[5])};
    const double pwb[3] = {uniformValue(pb[3]), uniformValue(pb[4]), uniformValue(pb[5])};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      eaU[k] = uniformValue(pwa[0] * Fa.Jl[k] + pwa[1] * Fa.Jl[3 + k] + pwa[2] * Fa.Jl[6 + k]);
      ebU[k] = uniformValue(pwb[0] * Fb.Jl[k] + pwb[1] * Fb.Jl[3 + k] + pwb[2] * Fb.Jl[6 + k]);
      dptU[k] = uniformValue(pa[k] - pb[k]);
    }
  }
  const double fya = uniformValue(Fa.fy), fxa = fya * A;
  const double fyb = uniformValue(Fb.fy);
  const double ifyb = uniformValue(1.0 / fyb), ifxb = uniformValue(1.0 / (fyb * A));
  const double pfaU = uniformValue(pa[6] / fya);          // p_f,src / fy_src: the focal column of the source is D R (c + e_z) / fy
  const double pfrU = uniformValue(L.ws * pb[6] * ifyb);   // ws p_f,tgt / fy_tgt

  const int fsrc = dir ? fb : fa, ftgt = dir ? fa : fb;
  const long long pixBase = DENSE ? (cb / (static_cast<long long>(T.W) * T.H)) * (static_cast<long long>(T.W) * T.H) : 0;
  // (dense mode keeps lane = pixel here: the private accumulator copies take care of the same-vertex collisions, and
  // the run-per-lane mapping of the assembly kernel measured slower for this kernel: 1.00 vs 0.75 ms)
  // Wave-units of 64 constraints are dealt round-robin over the waves ACROSS the two directions: direction 1 starts with
  // the wave after the one that took direction 0's last unit.  With ~9 units per direction and 4 waves the slowest wave
  // walks 5 units instead of 3 + 3 (both directions' remainders used to land on waves 0, 1).
  for (int ci = iFirst; ci < nDir; ci += NT) {
    float4 nd;
    float2 d;
    if (!rs.take(T, cb, ci, NT, nDir, pixBase, fsrc, ftgt, nd, d)) continue;
    const double da = static_cast<double>(d.x), db = static_cast<double>(d.y);
    FastTaps<KD> ta, tb;
    fastGather<KD>(L, nd.x, nd.y, ta);
    fastGather<KD>(L, nd.z, nd.w, tb);
    // depths and their directional derivatives
    double Da, Db, sDa, sDb;
    if (N == 0) {
      Da = da; Db = db; sDa = 0.0; sDb = 0.0;
    } else {
      Da = 0.0; Db = 0.0; sDa = 0.0; sDb = 0.0;
#pragma unroll
      for (int k = 0; k < KD; ++k) {
        if (ta.ok(k)) {
          const int ia = ta.I(k);
          const double wa = ta.Wt(k);
          if (N == 2) {
            Da += (da * xa[7 + ia * 2] + xa[7 + ia * 2 + 1]) * wa;
            sDa += (da * pa[7 + ia * 2] + pa[7 + ia * 2 + 1]) * wa;
          } else {  // (one value parameter: the source depth multiplies the interpolated scale once, below)
            Da += xa[7 + ia] * wa;
            sDa += pa[7 + ia] * wa;
          }
        }
        if (tb.ok(k)) {
          const int ib = tb.I(k);
          const double wb = tb.Wt(k);
          if (N == 2) {
            Db += (db * xb[7 + ib * 2] + xb[7 + ib * 2 + 1]) * wb;
            sDb += (db * pb[7 + ib * 2] + pb[7 + ib * 2 + 1]) * wb;
          } else {
            Db += xb[7 + ib] * wb;
            sDb += pb[7 + ib] * wb;
          }
        }
      }
      if (N != 2) { Da *= da; sDa *= da; Db *= db; sDb *= db; }
    }
    const double pax = static_cast<double>(nd.x), pay = static_cast<double>(nd.y);
    const double pbx = static_cast<double>(nd.z), pby = static_cast<double>(nd.w);
    double ca[3], Rca[3];
    fastRay(RaU, pax, pay, fxa, fya, ca, Rca);
    const double v[3] = {dTU[0] + Rca[0] * Da, dTU[1] + Rca[1] * Da, dTU[2] + Rca[2] * Da};
    double zz, iz, u, vv, r0, r1, r2, dr2dA, dr2dDb;
    fastProject<SPEC != 0>(L, RbU, v, ifxb, ifyb, pbx, pby, zz, iz, u, vv, r0, r1);
    fastDepthResidual<SPEC != 0>(L, lossType, zz, iz, Db, r2, dr2dA, dr2dDb);
    const double rho1 = fastRobustRho1<SPEC>(L, r0 * r0 + r1 * r1 + r2 * r2);

    // ---- forward: dX, dq, t
    // R c_f, c_f = d c_a / d fy = (c_a + e_z) / fy: the rotated ray plus R's third column (the 1 / fy sits in pfaU and, for the
    // adjoint, in the epilogue)
    const double Rcf[3] = {Rca[0] + RaU[2], Rca[1] + RaU[5], Rca[2] + RaU[8]};
    const double Eca[3] = {eaU[1] * Rca[2] - eaU[2] * Rca[1], eaU[2] * Rca[0] - eaU[0] * Rca[2], eaU[0] * Rca[1] - eaU[1] * Rca[0]};
    const double vxe[3] = {v[1] * ebU[2] - v[2] * ebU[1], v[2] * ebU[0] - v[0] * ebU[2], v[0] * ebU[1] - v[1] * ebU[0]};
    double w3[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) w3[i] = dptU[i] + Da * (Eca[i] + pfaU * Rcf[i]) + sDa * Rca[i] + vxe[i];
    const double dq0 = RbU[0] * w3[0] + RbU[3] * w3[1] + RbU[6] * w3[2];
    const double dq1 = RbU[1] * w3[0] + RbU[4] * w3[1] + RbU[7] * w3[2];
    const double dq2 = RbU[2] * w3[0] + RbU[5] * w3[1] + RbU[8] * w3[2];
    double m00, m11, m02, m12;
    fastRows(L, iz, u, vv, ifxb, ifyb, m00, m11, m02, m12);
    double t0 = (m00 * dq0 + m02 * dq2 - u * pfrU) * rho1;
    double t1 = (m11 * dq1 + m12 * dq2 - vv * pfrU) * rho1;
    double t2 = (-dr2dA * dq2 + dr2dDb * sDb) * rho1;

    // ---- backward
    const double yq0 = m00 * t0, yq1 = m11 * t1, yq2 = m02 * t0 + m12 * t1 - dr2dA * t2;
    aFb -= L.ws * (u * t0 + vv * t1);
    const double yX[3] = {RbU[0] * yq0 + RbU[1] * yq1 + RbU[2] * yq2, RbU[3] * yq0 + RbU[4] * yq1 + RbU[5] * yq2,
                          RbU[6] * yq0 + RbU[7] * yq1 + RbU[8] * yq2};
#pragma unroll
    for (int i = 0; i < 3; ++i) aT[i] += yX[i];
    Cx[0] += v[1] * yX[2] - v[2] * yX[1];
    Cx[1] += v[2] * yX[0] - v[0] * yX[2];
    Cx[2] += v[0] * yX[1] - v[1] * yX[0];
    aFa += Da * (Rcf[0] * yX[0] + Rcf[1] * yX[1] + Rcf[2] * yX[2]);
    if (N > 0) {
      const double ga = Rca[0] * yX[0] + Rca[1] * yX[1] + Rca[2] * yX[2];
      const double gb = dr2dDb * t2;
      // (the source depths are converted again here instead of being kept as doubles across the trip: with the next record
      // in flight the loop needs every register of its three-waves budget; the asm keeps the two conversions apart)
      float dxLate = d.x, dyLate = d.y;
      asm volatile("" : "+v"(dxLate), "+v"(dyLate));
      const double da = static_cast<double>(dxLate), db = static_cast<double>(dyLate);
      if constexpr (KD == 1) {
        gDa[0] += ga * da; gDa[1] += ga;
        gDb[0] += gb * db; gDb[1] += gb;
      } else {
      // (dense: this lane's private copy; qa / qb are swapped per direction, the private copies are indexed by role)
      const int pkey = (DENSE ? tid : (tid ^ (tid >> 5))) & (kPriv - 1);
      double* qaw = kUsePriv ? qpriv + (static_cast<size_t>(pkey) * 2 + dir) * B : qa;
      double* qbw = kUsePriv ? qpriv + (static_cast<size_t>(pkey) * 2 + (dir ^ 1)) * B : qb;
      const double gad = ga * da, gbd = gb * db;
#pragma unroll
      for (int k = 0; k < KD; ++k) {
        if (ta.ok(k)) {
          const int ia = ta.I(k);
          const double wa = ta.Wt(k);
          if (N == 2) {
            atomicAdd(&qaw[7 + ia * 2], gad * wa);
            atomicAdd(&qaw[7 + ia * 2 + 1], ga * wa);
          } else {
            atomicAdd(&qaw[7 + ia], gad * wa);
          }
        }
        if (tb.ok(k)) {
          const int ib = tb.I(k);
          const double wb = tb.Wt(k);
          if (N == 2) {
            atomicAdd(&qbw[7 + ib * 2], gbd * wb);
            atomicAdd(&qbw[7 + ib * 2 + 1], gb * wb);
          } else {
            atomicAdd(&qbw[7 + ib], gbd * wb);
          }
        }
      }
      }
    }
  }
  }  // dir
  MV_STAMP(4 + ((threadIdx.x >> 6) & 3));  // each wave's end of the constraint loop
  // ---- one workgroup reduction of the 11 (15) accumulators (roles of direction 1: source = fb, target = fa).
  // Lane pairs store their values transposed into LDS (row = accumulator, column = lane pair, 33-padded 32-column
  // segments), then 4 threads per accumulator sum one segment each: ~25 LDS ops per thread instead of 11 x 6
  // cross-lane butterfly steps.
  // (t, fy, J_l of the two frames from the prologue's LDS copy: [0..2] t, [3] fy, [4..12] J_l)
  const double* fixFa = fix + kFix;   // frame fb, the source of direction 1
  const double* fixFb = fix;
  {
    double vals[NV];
#pragma unroll
    for (int i = 0; i < 3; ++i) { vals[i] = aT[i]; vals[3 + i] = aT0[i]; vals[6 + i] = Cx[i]; }
    vals[9] = aFa;
    vals[10] = aFb;
    if constexpr (KD == 1) { vals[11] = gDa[0]; vals[12] = gDa[1]; vals[13] = gDb[0]; vals[14] = gDb[1]; }
    // neighbouring lanes are summed in registers first (one DPP swap), so only the even lanes store: half the LDS
    const int half = tid >> 1;
    const int colw = (half >> 5) * 33 + (half & 31);
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const double v = vals[i] + dppMove<0xB1>(vals[i]);
      if ((tid & 1) == 0) W[i * kRedStride + colw] = v;
    }
  }
  __syncthreads();
  constexpr int SEG = NT / 64;  // 32-column segments per accumulator row (lane pairs): 4 at 256 threads, 2 at 128
  if (tid < NV * SEG) {
    const double* row = W + (tid / SEG) * kRedStride + (tid % SEG) * 33;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
#pragma unroll
    for (int k = 0; k < 32; k += 4) {
      s0 += row[k];
      s1 += row[k + 1];
      s2 += row[k + 2];
      s3 += row[k + 3];
    }
    double sacc = (s0 + s1) + (s2 + s3);
    if (SEG >= 2) sacc += dppMove<0xB1>(sacc);   // SEG consecutive lanes hold one accumulator's segments
    if (SEG == 4) sacc += dppMove<0x4E>(sacc);
    if (tid % SEG == 0) red[tid / SEG] = sacc;
  }
  __syncthreads();
  // red: [0..2] aT of direction 1 (source fb), [3..5] aT of direction 0 (source fa), [6..8] C = C_1 - C_0, [9] / [10] focal sums of
  // the source / target ROLE of direction 1, [11..14] the depth-block sums (KD == 1).  With dT = t_src - t_tgt of direction 1:
  //   q_t,src = aT_1 - aT_0 = -q_t,tgt;   q_w,src,i = a_src,i . (C - dT x aT_1);   q_w,tgt,i = a_tgt,i . (dT x aT_0 - C)
  if (tid < 3) {
    const double d = red[tid] - red[3 + tid];
    qa[tid] += d;
    qb[tid] -= d;
  } else if (tid < 9) {
    const bool tgt = tid >= 6;
    const int i = tgt ? tid - 6 : tid - 3;
    const double dT[3] = {fixFa[0] - fixFb[0], fixFa[1] - fixFb[1], fixFa[2] - fixFb[2]};
    const double* y = red + (tgt ? 3 : 0);
    const double m[3] = {red[6] - (dT[1] * y[2] - dT[2] * y[1]), red[7] - (dT[2] * y[0] - dT[0] * y[2]),
                         red[8] - (dT[0] * y[1] - dT[1] * y[0])};
    const double* a = (tgt ? fixFb : fixFa) + 4 + 3 * i;   // (frame fb is the source of direction 1)
    const double sdot = a[0] * m[0] + a[1] * m[1] + a[2] * m[2];
    if (tgt) qb[3 + i] -= sdot;
    else qa[3 + i] += sdot;
  } else if (tid == 9) {
    qa[6] += red[9] / fixFa[3];
  } else if (tid == 10) {
    qb[6] += red[10] / fixFb[3];
  } else if (KD == 1 && tid < 15) {
    const int n = (tid - 11) & 1;
    if (n < N) {
      if (tid < 13) qa[7 + n] += red[11 + n];
      else qb[7 + n] += red[13 + n];
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) MV_STAMP(2);
  { double* t = qa; qa = qb; qb = t; }  // undo the role swap
  if constexpr (kUsePriv) {
    // private copy [k][0] collected frame fa's grid columns (source of direction 0, target of direction 1), [k][1] fb's
    for (int i = tid; i < B; i += NT) {
      double sa = 0.0, sb = 0.0;
#pragma unroll
      for (int k = 0; k < kPriv; ++k) {
        sa += qpriv[(static_cast<size_t>(k) * 2 + 0) * B + i];
        sb += qpriv[(static_cast<size_t>(k) * 2 + 1) * B + i];
      }
      qa[i] += sa;
      qb[i] += sb;
    }
    __syncthreads();
  }
  // rows are grouped by frame (slot = position in the frame's item list) so that k_matvec_finish streams them
  double* outA = qPart + static_cast<size_t>(slotA) * B;
  double* outB = qPart + static_cast<size_t>(slotB) * B;
  for (int i = tid; i < B; i += NT) {
    outA[i] = qa[i];
    outB[i] = qb[i];
  }
  if (threadIdx.x == 0) MV_STAMP(3);
}

}  // namespace cvd
