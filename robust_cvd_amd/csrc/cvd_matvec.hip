// cvd_matvec.hip -- the PCG product q = (J^T J + diag(lam)) p: pair-major partial products, per-frame finish, exchange.
#include "cvd_host.h"
#include "cvd_pcg.h"
#include "cvd_cross.h"
#include "cvd_triplets.h"

namespace cvd {

bool coarseFusedConsumers() {
  return false;  // (c_f formed inside the consumers: measured slower than the k_coarse_apply_wt launch; kept as a code path of CoarseView)
}
// Pair-sharded mode: the product's exchange carries [q | Z^T q | p.q] in one all-reduce unless the SPARSE coarse level is on
// (its column products need the reduced Z^T q: k_dot_pq).  Layout: [q (F B) | Z^T q (8 F, dense coarse level only) | p.q].
bool fusedExchange(cvd_handle* h, bool withCoarse) { return !withCoarse || h->coarse.denseMode; }
// (sharded: the q part is padded to world x chunk frames, so that its reduce-scatter / all-gather chunks are equal)
size_t exchangeOffsetQc(const Ctx& c) { return c.h->dist() ? static_cast<size_t>(c.h->framesPadded()) * c.L.B : c.n; }
size_t exchangeOffsetPq(const Ctx& c, bool withDenseCoarse) {
  return exchangeOffsetQc(c) + (withDenseCoarse ? static_cast<size_t>(c.L.F) * kCB : 0);
}
// Owner-sharded PCG iteration: with the fused exchange the product's q is REDUCE-SCATTERED to
// the frames' owners ([Z^T q | p.q] all-reduced beside it, one RCCL group), every rank updates x, r, z (and its rows of the dense
// coarse level) for ITS frames only, and z / c / the r^T z shares are all-gathered (one group): two collectives per iteration,
// the per-frame update work divided by the number of ranks.
size_t exchangeTemporalCount(cvd_handle* h, bool withCoarse) {
  const TlStep ts = temporalStep(h);
  return (ts.Ainv != nullptr && h->dist() && fusedExchange(h, withCoarse)) ? static_cast<size_t>(h->F) * ts.S : 0;
}
bool ownerShardedUpdate(cvd_handle* h, bool withCoarse) {
  return h->dist() && fusedExchange(h, withCoarse) && h->opt.dist_owner_update != 0;
}
CoarseView coarseView(cvd_handle* h, bool on, bool walk) {
  auto& C = h->coarse;
  CoarseView v = on ? CoarseView{C.pos.p, C.wPtr.p, C.wRow.p, walk ? C.Wb.p : nullptr, C.y.p, C.modeActive.p, C.fail.p, C.c.p}
                    : CoarseView{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  if (h->temporal.on && h->temporal.built) {  // third level: its per-frame coefficients and the vertex table of the prolongation
    v.tl = h->temporal.tl.p;
    v.tlW = h->temporal.vW.p;
    v.tlIdx = h->temporal.vIdx.p;
    v.tlS = h->temporal.S;
  }
  return v;
}

// Fills the regulariser Jacobian cache for the products at linearisation point x (before runPcg / the J^T J hook).
void prepareMatvec(Ctx& c, const double* x) {
  cvd_handle* h = c.h;
  const Layout& L = c.L;
  // the per-frame constants must be those of x: a rejected LM step leaves the candidate's behind (evalCost)
  launchFrameConsts(c, x);
  int nr = 0;
  if (L.scaleRegSqrt > 0.0) nr += L.sregX * L.sregY;
  if (L.focalRegSqrt > 0.0) nr += 1;
  if (L.depthDeformW > 0.0 && L.depthType == CVD_DEPTH_GRID) nr += gridNumEdges(L.gx, L.gy, L.gz) * L.N;
  if (L.spatialDeformW > 0.0) nr += L.nS;
  const int stride = std::max(2, c.KD * std::max(1, L.N));
  const size_t entries = static_cast<size_t>(L.F) * stride * std::max(nr, 1);
  h->dRegJac.ensure(entries);
  h->dRegCol.ensure(entries);
  h->dRegCnt.ensure(static_cast<size_t>(L.F) * std::max(nr, 1));
  h->regCache = RegCache{h->dRegJac.p, h->dRegCol.p, h->dRegCnt.p, nr, stride};
  HIP_CHECK(hipMemsetAsync(h->dScal.p + S_DONE, 0, sizeof(double), h->stream));
  if (nr == 0) return;
  CVD_DISPATCH_KD(c.KD, {
    hipLaunchKernelGGL((k_reg_cache<KD>), dim3(L.F), dim3(256), static_cast<size_t>(L.B) * 8, h->stream, L, x, h->dMedian.p, h->dRegOwner.p,
                       h->regCache);
  });
  HIP_CHECK(hipGetLastError());
}

// The product the PCG loop launches for this problem: the list-mode fast kernel in its Cauchy compile-time variant (SPEC 1),
// four depth taps per side (the bilinear grids), no triplet kernel behind it -- the only product that sums the fused tail's r^T z
// shares (k_matvec_triplets, k_cross_matvec, the dense-mode and the generic kernels read beta from the scalars; the Global level's
// KD = 1 instantiation pays for the shares prologue with scalar-register restores in its loop's set-up and the bicubic one has no
// registers to spare, so neither is built).  Mirrors launchMatvec.
static bool productSumsShares(const Ctx& c) {
  const cvd_handle* h = c.h;
  if (c.cross || !c.L.includeStatic || c.nItems <= 0 || h->dense) return false;
  if (h->forceGeneric || c.KS != 0 || !fastLoss(c.L)) return false;
  if (!(c.L.N == 1 && c.L.lossType == CVD_STATIC_REPRO_DISPARITY)) return false;   // (SPEC 0: runtime loss branches)
  // (SPEC 2, the Huber variant: its shares forms miss the budget -- <4,256,2> spills a vector register (8 B of scratch), <4,128,2>
  // restores more scalar registers in its loop segment than its twin -- and are not built)
  if (c.L.robustKind != 0) return false;
  if (c.KD != 4) return false;
  return !(c.trip && c.TT.nGroups > 0);
}

void launchMatvec(Ctx& c, const double* x, const double* z, const double* pOld, double* pNew, int useBeta,
                         const double* lam, double* q, bool withCoarse, bool tailFused, int sharesIteration) {
  cvd_handle* h = c.h;
  if (sharesIteration > 0 && !productSumsShares(c)) throw std::runtime_error("launchMatvec: this product cannot sum the tail's shares");
  hipStream_t s = h->stream;
  const CoarseView cF = coarseView(h, withCoarse, coarseFusedConsumers());  // z + Z c: the coarse part of the preconditioned residual
  const size_t B = c.L.B;
  // (cvd_product_launch_debug: called with the template arguments of the instantiation that is launched)
  auto recordLaunch = [h](int threads, int spec, int kd, int kind, int items) {
    const int launched[6] = {threads, spec, kd, kind, items, h->numCU};
    std::copy(launched, launched + 6, h->lastProduct);
  };
  if (c.cross) {
    // explicit cross blocks (dense mode): one workgroup per undirected pair streams its B x B block
    hipEvent_t evStart, evStop;
    (void)h->tReserve(KC_MATVEC_PAIRS, evStart, evStop);
    const size_t ldsX = (3 * B + (kCrossThreads / 64) * B + 2 * kCB + 2 * kTlMaxS) * 8;
    // (+ one workgroup per frame for its own block H_ff: see k_cross_matvec)
    const unsigned nP = static_cast<unsigned>(h->xFa.size()) + (h->xDiagRows ? static_cast<unsigned>(c.L.F) : 0u);
    const int* diagSlot = h->xDiagRows ? h->dXDiagSlot.p : nullptr;
    recordLaunch(kCrossThreads, 0, c.KD, 3, static_cast<int>(nP));
    if (evStart)
      hipExtLaunchKernelGGL(k_cross_matvec, dim3(nP), dim3(kCrossThreads), ldsX, s, evStart, evStop, 0, c.L, crossPairs(h),
                            h->dXBlocks.p, h->dH.p, diagSlot, h->dMask.p, z, pOld, h->dScal.p, useBeta, h->dQPart.p, cF);
    else
      hipLaunchKernelGGL(k_cross_matvec, dim3(nP), dim3(kCrossThreads), ldsX, s, c.L, crossPairs(h), h->dXBlocks.p, h->dH.p, diagSlot,
                         h->dMask.p, z, pOld, h->dScal.p, useBeta, h->dQPart.p, cF);
    HIP_CHECK(hipGetLastError());
  } else if (c.L.includeStatic && c.nItems > 0) {
    const size_t lds = 6 * B * 8 + 2 * sizeof(FrameConst) + (18 + 4 * 24 + 8 + 2 * kCB) * 8;
    const size_t ldsFast = 6 * B * 8 + 2 * sizeof(FrameConst) + (32 + static_cast<size_t>(kRedVals) * kRedStride) * 8;  // (the two FrameConst: 2 x 13 doubles of them hold t, fy, J_l for the epilogue)
    hipEvent_t evStart, evStop;
    (void)h->tReserve(KC_MATVEC_PAIRS, evStart, evStop);
    const bool fast = !h->forceGeneric && c.KS == 0 && fastLoss(c.L);
    // (plain launches unless the launch is timed: hipExtLaunchKernelGGL is not used inside a graph capture)
    const FrameConst* fcp = h->dFc.p;
    const double* maskp = h->dMask.p;
    const double* scalp = h->dScal.p;
    if (fast) {
      // Workgroup size: 256 threads when the items fit into one round of 256-thread workgroups (nItems <= slots256, below) or
      // need more than one round even at 128 threads (nItems > slots128); 128 threads in between, where the launch then has no
      // ragged second round.  On 256 CUs the 128-thread windows are (1024, 2048] items for SPEC 1 / 2 with KD <= 4, (768, 1536]
      // for SPEC 1 / 2 with KD = 16 and (512, 1024] for SPEC 0: the benchmarked lists (2070 and 883 items, SPEC 1, KD <= 4) lie
      // outside theirs and run 256 threads.
      // SPEC = 1 / 2: the default pipeline's variant (one value parameter, ReproDisparity; Cauchy / Huber) fixed at compile time
      const int spec = (c.L.N == 1 && c.L.lossType == CVD_STATIC_REPRO_DISPARITY) ? (c.L.robustKind == 0 ? 1 : 2) : 0;
      // Slots of 256-thread workgroups on the device: waves per SIMD the variant is compiled for (cvd_kernels.h) x CUs; 128-thread
      // workgroups: twice as many, as far as the LDS of a CU holds them.  One round of 256 when the items fit; one round of 128
      // when only that fits; else 256 (rounds 2-4 assumed two waves per SIMD for every variant).
      const int wavesPerSimd = spec ? ((c.KD <= 4) ? CVD_MV_WAVES : 3) : 2;
      const long long slots256 = static_cast<long long>(wavesPerSimd) * h->numCU;
      const long long slots128 = std::min<long long>(2 * slots256, static_cast<long long>(kMaxLds / std::max<size_t>(ldsFast, 1)) * h->numCU);
#ifndef CVD_MV_NT_RULE
#define CVD_MV_NT_RULE 1   // 0: the rule of rounds 2-4 (2 x CUs slots assumed)
#endif
      const int nt = CVD_MV_NT_RULE ? ((c.nItems <= slots256 || c.nItems > slots128) ? 256 : 128)
                                    : (c.nItems > 2 * h->numCU && c.nItems <= 4 * h->numCU ? 128 : 256);
#define CVD_LAUNCH_PAIRS_FAST_S(NTV, SPECV)                                                                              \
      CVD_DISPATCH_KD(c.KD, {                                                                                            \
        recordLaunch(NTV, SPECV, KD, 1, c.nItems);                                                                       \
        if constexpr (SPECV == 1 && KD == 4) {                                                                           \
          if (sharesIteration > 0) { /* (the shares instantiation: `useBeta` carries the iteration's index) */          \
            allowLds((k_matvec_pairs_fast<KD, NTV, SPECV, false, true>), ldsFast);                                       \
            if (evStart)                                                                                                 \
              hipExtLaunchKernelGGL((k_matvec_pairs_fast<KD, NTV, SPECV, false, true>), dim3(c.nItems), dim3(NTV), ldsFast, s, \
                                    evStart, evStop, 0, c.L, c.T, c.it, x, fcp, maskp, z, pOld, scalp, sharesIteration,  \
                                    h->dQPart.p, cF);                                                                    \
            else                                                                                                         \
              hipLaunchKernelGGL((k_matvec_pairs_fast<KD, NTV, SPECV, false, true>), dim3(c.nItems), dim3(NTV), ldsFast, s, c.L, \
                                 c.T, c.it, x, fcp, maskp, z, pOld, scalp, sharesIteration, h->dQPart.p, cF);             \
            break;                                                                                                       \
          }                                                                                                              \
        }                                                                                                                \
        allowLds((k_matvec_pairs_fast<KD, NTV, SPECV>), ldsFast);                                                        \
        if (evStart)                                                                                                     \
          hipExtLaunchKernelGGL((k_matvec_pairs_fast<KD, NTV, SPECV>), dim3(c.nItems), dim3(NTV), ldsFast, s, evStart, evStop, 0, \
                                c.L, c.T, c.it, x, fcp, maskp, z, pOld, scalp, useBeta, h->dQPart.p, cF);                \
        else                                                                                                             \
          hipLaunchKernelGGL((k_matvec_pairs_fast<KD, NTV, SPECV>), dim3(c.nItems), dim3(NTV), ldsFast, s, c.L, c.T, c.it, x, \
                             fcp, maskp, z, pOld, scalp, useBeta, h->dQPart.p, cF);                                      \
      })
#define CVD_LAUNCH_PAIRS_FAST(NTV) do { if (spec == 1) CVD_LAUNCH_PAIRS_FAST_S(NTV, 1); else if (spec == 2) CVD_LAUNCH_PAIRS_FAST_S(NTV, 2); else CVD_LAUNCH_PAIRS_FAST_S(NTV, 0); } while (0)
      if (h->dense) {
        // dense mode: flow / mask / depth read directly (17 B per pixel pair), grid columns in 8 lane-keyed private copies
        const size_t ldsDense = ldsFast + 8 * 2 * B * 8;
#define CVD_LAUNCH_PAIRS_DENSE(SPECV)                                                                                     \
        CVD_DISPATCH_KD(c.KD, {                                                                                          \
          if constexpr (KD <= 4) { /* (dense mode: Global and bilinear grids) */                                         \
            recordLaunch(256, SPECV, KD, 2, c.nItems);                                                                   \
            allowLds((k_matvec_pairs_fast<KD, 256, SPECV, true>), ldsDense);                                             \
            if (evStart)                                                                                                 \
              hipExtLaunchKernelGGL((k_matvec_pairs_fast<KD, 256, SPECV, true>), dim3(c.nItems), dim3(256), ldsDense, s, evStart, \
                                    evStop, 0, c.L, c.T, c.it, x, fcp, maskp, z, pOld, scalp, useBeta, h->dQPart.p, cF); \
            else                                                                                                         \
              hipLaunchKernelGGL((k_matvec_pairs_fast<KD, 256, SPECV, true>), dim3(c.nItems), dim3(256), ldsDense, s, c.L, c.T, \
                                 c.it, x, fcp, maskp, z, pOld, scalp, useBeta, h->dQPart.p, cF);                         \
          }                                                                                                              \
        })
        if (spec == 1) CVD_LAUNCH_PAIRS_DENSE(1);
        else if (spec == 2) CVD_LAUNCH_PAIRS_DENSE(2);
        else CVD_LAUNCH_PAIRS_DENSE(0);  // (the other reprojection losses: runtime branches)
#undef CVD_LAUNCH_PAIRS_DENSE
      }
#if CVD_DETERMINISTIC
      else { (void)nt; CVD_LAUNCH_PAIRS_FAST(64); }  // (one wave per work item: its LDS atomics land in program order)
#else
      else if (nt == 128) CVD_LAUNCH_PAIRS_FAST(128);
      else CVD_LAUNCH_PAIRS_FAST(256);
#endif
#undef CVD_LAUNCH_PAIRS_FAST_S
#undef CVD_LAUNCH_PAIRS_FAST
    } else {
      recordLaunch(256, 0, c.KD, 0, c.nItems);
      CVD_DISPATCH(c.KD, c.KS, {
        allowLds(k_matvec_pairs<KD, KS>, lds);
        if (evStart)
          hipExtLaunchKernelGGL((k_matvec_pairs<KD, KS>), dim3(c.nItems), dim3(256), lds, s, evStart, evStop, 0, c.L, c.T,
                                c.it, x, fcp, maskp, z, pOld, scalp, useBeta, h->dQPart.p, cF);
        else
          hipLaunchKernelGGL((k_matvec_pairs<KD, KS>), dim3(c.nItems), dim3(256), lds, s, c.L, c.T, c.it, x, fcp, maskp, z,
                             pOld, scalp, useBeta, h->dQPart.p, cF);
      });
    }
    HIP_CHECK(hipGetLastError());
  }
  if (c.trip && c.TT.nGroups > 0) {
    const size_t ldsT = (9 * B + 3 * kCB) * 8;
    CVD_DISPATCH(c.KD, c.KS, {
      allowLds(k_matvec_triplets<KD, KS>, ldsT);
      hipLaunchKernelGGL((k_matvec_triplets<KD, KS>), dim3(c.TT.nGroups), dim3(256), ldsT, s, c.L, c.TT, x, h->dFc.p,
                         h->dMask.p, z, pOld, h->dScal.p, useBeta, h->dQPart.p, cF);
    });
    HIP_CHECK(hipGetLastError());
  }
  if (!tailFused) {
    if (B > 512) throw std::runtime_error("frame block larger than 512 unknowns is not supported by k_matvec_finish");
    const TlStep ts = temporalStep(h);
    // xf, pf, qf + red[6] + flag + coarse correction (+ third level: its coefficients and the restriction's products)
    const size_t lds = 3 * B * 8 + (8 + kCB) * 8 + (ts.Ainv != nullptr ? (kTlMaxS + static_cast<size_t>(ts.S) * ts.width) * 8 : 0);
    // column half of the fused coarse update y <- y - alpha W (Z^T q) (the row half is in k_cg_update)
    const bool fusedCoarse = withCoarse && !h->coarse.denseMode;
    const bool denseFused = withCoarse && h->coarse.denseMode;  // (needs Z^T q: DenseStep)
    // pair-sharded mode, FUSED exchange (dense coarse level or none): this rank's q, Z^T q and p.q lie contiguously behind
    // q and travel in one all-reduce; k_cg_update forms alpha from the reduced p.q.  With the sparse coarse level the
    // column products need the REDUCED Z^T q: q alone is exchanged and k_dot_pq finishes the product.
    const bool fusedX = h->dist() && fusedExchange(h, withCoarse);
    double* qcX = q + exchangeOffsetQc(c);
    double* pqX = q + exchangeOffsetPq(c, denseFused);
    const CoarseColumns cc{h->coarse.pos.p, h->coarse.wPtr.p, h->coarse.wSlot.p, fusedCoarse ? h->coarse.Wb.p : nullptr,
                           h->coarse.wq.p};
    const int slot = h->tBegin(KC_MATVEC_FINISH);
    CVD_DISPATCH_KD(c.KD, {
      hipLaunchKernelGGL((k_matvec_finish<KD>), dim3(c.L.F), dim3(256), lds, s, c.L, x, h->dMask.p, lam,
                         h->dMedian.p, h->dRegOwner.p, h->dInRange.p, c.cross ? h->dXFiOff.p : h->dFiOff.p, h->dFiList.p,
                         h->dQPart.p, z, pOld, pNew, h->dScal.p, h->dCounters.p, useBeta, q, h->dFdot.p,
                         h->dist() ? (h->rank == 0 ? 1 : 2) : 0, c.cross ? static_cast<int>(h->xFa.size()) * 2 : h->qRows,
                         h->regCache, cF,
                         fusedX ? (denseFused ? qcX : nullptr) : (((fusedCoarse || denseFused) && !h->dist()) ? h->coarse.qc.p : nullptr), cc,
                         c.cross ? h->dH.p : nullptr, fusedX ? pqX : nullptr, h->dist() ? h->ownFirst() : 0,
                         h->dist() ? h->ownCount() : ((c.cross && h->xDiagRows) ? 0 : c.L.F), ts.Ainv != nullptr ? temporalStepDev(h) : static_cast<const TlStep*>(nullptr));
    });
    HIP_CHECK(hipGetLastError());
    if (fusedX && ownerShardedUpdate(h, withCoarse)) {
      // q to the frames' owners (in place: the reduced chunk lands where the frames' q lives), [Z^T q | p.q] to everybody
      const int ct = h->tBegin(KC_COMM_PRODUCT);
      const size_t chunk = static_cast<size_t>(h->ownChunk()) * B;
      commGroupStart(h);
      commReduceScatter(h, q, q + static_cast<size_t>(h->rank) * chunk, chunk, CT_F64, s);
      commAllReduce(h, qcX, exchangeOffsetPq(c, denseFused) - exchangeOffsetQc(c) + 1 + exchangeTemporalCount(h, withCoarse), CT_F64, s);
      commGroupEnd(h);
      h->tEnd(ct);
    } else if (fusedX) {
      const int ct = h->tBegin(KC_COMM_PRODUCT);
      commAllReduce(h, q, exchangeOffsetPq(c, denseFused) + 1 + exchangeTemporalCount(h, withCoarse), CT_F64, s);
      h->tEnd(ct);
    } else if (h->dist()) {
      // per-product exchange: q (F x B doubles) summed over the pair shards, then p.q / alpha on the reduced vector
      const int ct = h->tBegin(KC_COMM_PRODUCT);
      commAllReduce(h, q, c.n, CT_F64, s);
      h->tEnd(ct);
      hipLaunchKernelGGL(k_dot_pq, dim3(c.L.F), dim3(256), 0, s, c.L, pNew, q, h->dScal.p, h->dCounters.p, h->dFdot.p,
                         withCoarse ? h->coarse.qc.p : nullptr, h->coarse.modeActive.p, cc,
                         ts.Ainv != nullptr ? temporalStepDev(h) : static_cast<const TlStep*>(nullptr));
      HIP_CHECK(hipGetLastError());
    }
    h->tEnd(slot);
  }
}

// ---- k_pcg_tail: finish + update of a PCG iteration in one launch (cvd_pcg.h) --------------------------------------------
// Scope and launch geometry: one GPU, frame block <= 256, dense coarse level or none, and every workgroup of the launch
// resident at once (the kernel has a grid barrier): checked against the kernel's occupancy on this device.
bool pcgTailScope(Ctx& c, bool coarse, int nThreads, size_t& lds, int& ldsFinish, int& ldsScratch) {
  cvd_handle* h = c.h;
  const int F = c.L.F, B = c.L.B;
  h->tailStageRows = false;  // (true only where this call chooses the staged launch)
  if (!h->opt.pcg_fused_tail || h->tailDisabled || h->dist() || B > 256 || h->forceGeneric) return false;
  if (coarse && !h->coarse.denseMode) return false;
  const int split = denseRowSplit(h);
  const TlStep ts = temporalStep(h);
  // (third level: S more workgroups; the restriction's products of a frame use the update half's partial-sum region)
  if (ts.Ainv != nullptr && (ts.S * ts.width > cgUpdatePartDoubles(B, nThreads) || tlRowsLds(ts.NT) > B + cgUpdatePartDoubles(B, nThreads)))
    return false;
  const bool poseT = coarse && h->coarse.temporalPose;  // (coarse_level 3: kCB workgroups walk the node-reduced inverse, no dense-level ones)
  if (poseT && tlRowsLds(h->coarse.ptN) > B + cgUpdatePartDoubles(B, nThreads)) return false;
  const int grid = F + (coarse && !poseT && split > 0 ? (F + kDenseFramesPerGroup - 1) / kDenseFramesPerGroup : 0) +
                   (ts.Ainv != nullptr ? ts.S * ts.parts : 0) + (poseT ? kCB * tlParts(h->coarse.ptNn) : 0);
  const int update = B + cgUpdatePartDoubles(B, nThreads) + 48 + 17 * kCB;  // k_cg_update's region (cvd_solve.hip: ldsU)
  const int finish = 3 * B + 8 + kCB + (nThreads / 256 - 1) * 256 + kTlMaxS;  // k_matvec_finish's + the partial sums of its row walk + the third level's coefficients
  const int denseEnd = (coarse && !poseT) ? F * kCB + nThreads + 16 : 0;    // the dense-level workgroups' (Z^T q + partial sums)
  ldsFinish = update;
  // (frame workgroups that walk rows of the dense level themselves: Z^T q + partial sums behind their two regions)
  const int unstaged = std::max(update + finish + (coarse && split < kCB ? denseEnd : 0), denseEnd);
  // (the temporal levels' workgroups stage their rows of the inverse in LDS in front of the grid barrier where that fits and keeps
  // the launch co-resident: TailUpdate::stageRows; otherwise they read the rows from memory behind it, as the two-launch path does)
  int stagedEnd = 0;
  if (ts.Ainv != nullptr) stagedEnd = std::max(stagedEnd, tlStagedLds(ts.NT));
  if (poseT) stagedEnd = std::max(stagedEnd, tlStagedLds(h->coarse.ptN));
  // occupancy of this (kernel, block size, LDS size) on this device: asked once
  static std::map<std::tuple<int, int, int, size_t>, int> perCuCache;
  static std::mutex cacheMutex;
  auto resident = [&](size_t bytes) {
    if (bytes > kMaxLds) return false;
    int perCu = 0;
    std::lock_guard<std::mutex> lock(cacheMutex);
    const auto key = std::make_tuple(h->device, c.KD, nThreads, bytes);
    auto it = perCuCache.find(key);
    if (it == perCuCache.end()) {
      CVD_DISPATCH_KD(c.KD, {
        allowLds((k_pcg_tail<KD>), bytes);
        HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&perCu, reinterpret_cast<const void*>(&k_pcg_tail<KD>), nThreads, bytes));
      });
      perCuCache[key] = perCu;
    } else {
      perCu = it->second;
    }
    return static_cast<long long>(perCu) * h->numCU >= grid;
  };
  if (stagedEnd > 0 && h->dbg.tail_no_row_staging == 0) {
    ldsScratch = std::max(unstaged, stagedEnd);
    lds = static_cast<size_t>(ldsScratch + 24) * sizeof(double);
    if (resident(lds)) {
      h->tailStageRows = true;
      return true;
    }
  }
  ldsScratch = unstaged;
  lds = static_cast<size_t>(ldsScratch + 24) * sizeof(double);
  return resident(lds);
}

// Shares mode of the fused tail (cvd_pcg.h): the tail ends when its slowest workgroup has stored its share of r^T z, and the next
// product sums the shares in its prologue.  In scope when the solve runs the fused tail (the caller has asked pcgTailScope), the
// product is the one that can sum (productSumsShares), the host checks the mirror only for iterations a later product closes (not in
// lockstep, not with the per-iteration trace), the test option does not force the closing tail, and the shares fit the cap.
// Share layout: the frames' r^T z, the dense level's parts (its workgroups' rows, then the frame workgroups' rows), the depth-grid
// level's parts, the temporal pose level's parts.
bool pcgSharesScope(Ctx& c, bool coarse, PcgShares& sh) {
  cvd_handle* h = c.h;
  if (h->dbg.tail_closes_scalars != 0 || h->dbg.pcg_lockstep != 0 || h->opt.verbose >= 2 || !productSumsShares(c)) return false;
  const int F = c.L.F;
  const int split = denseRowSplit(h);
  const TlStep ts = temporalStep(h);
  const bool poseT = coarse && h->coarse.temporalPose;
  const bool dense = coarse && !poseT;
  const int nDenseWg = (dense && split > 0) ? (F + kDenseFramesPerGroup - 1) / kDenseFramesPerGroup : 0;
  sh.levelShare0 = F + ((dense && split > 0) ? F : 0) + ((dense && split < kCB) ? F : 0);
  sh.levelWg0 = F + nDenseWg;
  sh.count = sh.levelShare0 + (ts.Ainv != nullptr ? ts.S * ts.parts : 0) + (poseT ? kCB * tlParts(h->coarse.ptNn) : 0);
  return sh.count <= kPcgSharesCap;
}

void launchPcgClose(Ctx& c, int enqueued) {
  cvd_handle* h = c.h;
  hipLaunchKernelGGL(k_pcg_close, dim3(1), dim3(64), 0, h->stream, h->dScal.p, enqueued, h->hPcg);
  HIP_CHECK(hipGetLastError());
}

void launchPcgTail(Ctx& c, const double* x, const double* pOld, double* pNew, int useBeta, const double* lam, double* q,
                   bool withCoarse, int nThreads, size_t lds, int ldsFinish, int ldsScratch, double tol2, const PcgShares* shares) {
  cvd_handle* h = c.h;
  hipStream_t s = h->stream;
  const int F = c.L.F;
  const CoarseView cF = coarseView(h, withCoarse, false);
  const int split = denseRowSplit(h);
  const int finishDoubles = 3 * static_cast<int>(c.L.B) + 8 + kCB + (nThreads / 256 - 1) * 256 + kTlMaxS;  // (pcgTailScope)
  const TlStep ts = temporalStep(h);
  const bool poseT = withCoarse && h->coarse.temporalPose;
  // (shares mode: every share of r^T z goes into the one array behind the PCG scalars, in pcgSharesScope's layout)
  double* sharesRz = shares != nullptr ? h->dScal.p + SH_RZ : nullptr;
  double* densePart = shares != nullptr ? sharesRz + F : h->coarse.dotPart.p;
  double* densePart2 = shares != nullptr ? sharesRz + F + (split > 0 ? F : 0) : h->coarse.dotPart.p + F;
  const DenseStep ds = (withCoarse && !poseT) ? DenseStep{h->coarse.denseInv.p, h->coarse.qc.p, h->coarse.rc.p, h->coarse.c.p, densePart,
                                               h->coarse.modeActive.p, h->coarse.fail.p, split, ldsFinish + finishDoubles,
                                               densePart2}
                                  : DenseStep{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, kCB, 0, nullptr};
  double* fd = h->dFdot.p;
  const TailUpdate U{h->dMinv.p, h->dDx.p, h->dR.p, h->dZ.p, shares != nullptr ? sharesRz : fd + F,
                     shares != nullptr ? h->dScal.p + SH_RR : fd + 2 * F, tol2, h->coarse.modeActive.p, h->hPcg,
                     shares != nullptr ? static_cast<unsigned int*>(nullptr) : h->dCounters.p + 1, h->dTailBar.p,
                     h->dFdot.p + 4 * static_cast<size_t>(F) + 32, ldsFinish, ldsScratch, ds,
                     ts.Ainv != nullptr ? temporalStepDev(h) : static_cast<const TlStep*>(nullptr),
                     poseT ? poseTemporalStepDev(h) : static_cast<const TlStep*>(nullptr),
                     (c.cross && h->xDiagRows) ? 1 : 0, h->tailStageRows ? 1 : 0, sharesRz,
                     shares != nullptr ? shares->levelShare0 : 0, shares != nullptr ? shares->levelWg0 : 0};
  const int grid = F + (withCoarse && !poseT && split > 0 ? (F + kDenseFramesPerGroup - 1) / kDenseFramesPerGroup : 0) +
                   (ts.Ainv != nullptr ? ts.S * ts.parts : 0) + (poseT ? kCB * tlParts(h->coarse.ptNn) : 0);
  const int slot = h->tBegin(KC_CG_UPDATE);  // (timed under the update class: the finish class stays empty on this path)
  {
    // several handles of this process on one device: their grid-barrier kernels must not overlap (PersistentGate).  A handle
    // that is alone launches under the slot's mutex only (no events in the stream): cvd_create counts a second handle under the
    // same mutex and drains the device, so no ungated launch can still be in flight once another handle exists.
    std::unique_ptr<PersistentGate> gate;
    std::unique_lock<std::mutex> alone(PersistentGate::slot(h->device).m);
    if (liveHandles(h->device) > 1) {
      alone.unlock();
      gate.reset(new PersistentGate(h->device, s));
    }
    CVD_DISPATCH_KD(c.KD, {
      hipLaunchKernelGGL((k_pcg_tail<KD>), dim3(grid), dim3(nThreads), lds, s, c.L, x, h->dMask.p, lam, h->dMedian.p, h->dRegOwner.p,
                         h->dInRange.p, c.cross ? h->dXFiOff.p : h->dFiOff.p, h->dFiList.p, h->dQPart.p, pOld, pNew, h->dScal.p,
                         useBeta, q, fd, c.cross ? static_cast<int>(h->xFa.size()) * 2 : h->qRows, h->regCache, cF,
                         withCoarse ? h->coarse.qc.p : static_cast<double*>(nullptr),
                         c.cross ? static_cast<const double*>(h->dH.p) : static_cast<const double*>(nullptr), U);
    });
    HIP_CHECK(hipGetLastError());
  }
  h->tEnd(slot);
}

// One kernel of this translation unit's code object is looked up at handle creation: the HIP runtime loads a unit's device
// code at its first use, ~20 ms per unit that would otherwise land in the first solve of a process (cvd_create: loadDeviceCode).
void touchModule_matvec() {
  hipFuncAttributes a;
  (void)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(k_dot_pq));
}

}  // namespace cvd

#ifdef CVD_TAIL_PROFILE
extern "C" int32_t cvd_debug_tail_profile(unsigned long long* out) {
  (void)hipDeviceSynchronize();
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(cvd::g_tailProf), sizeof(unsigned long long) * 1024 * 16) == hipSuccess ? 0 : 1;
}
#endif
#ifdef CVD_MV_PROFILE
extern "C" int32_t cvd_debug_mv_profile(unsigned long long* out) {  // (same translation unit as the launches: the symbol is per unit)
  (void)hipDeviceSynchronize();
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(cvd::g_mvProf), sizeof(unsigned long long) * 4096 * 8) == hipSuccess ? 0 : 1;
}
#endif
