// cvd_solve.hip -- the PCG loop, the Levenberg-Marquardt driver (Ceres defaults) and the evaluation hook.
#include <optional>

#include "cvd_host.h"
#include "cvd_lm.h"
#include "cvd_pcg.h"
#include "cvd_coarse.h"

namespace cvd {

void launchTlRowsInit(cvd_handle* h, const TlStep* tsp, int NT, int groups, int F, unsigned int* counter, int closeScalars, double tol2,
                      hipStream_t s) {
  const size_t lds = static_cast<size_t>(tlRowsLds(NT)) * 8;
  allowLds(k_tl_rows_init, lds);
  hipLaunchKernelGGL(k_tl_rows_init, dim3(groups), dim3(768), lds, s, tsp, F, h->dScal.p, counter, closeScalars, tol2, h->hPcg);
  HIP_CHECK(hipGetLastError());
}

// PCG on (H + diag(lam)) dx = -g with the block-Jacobi preconditioner; returns iterations used.
// Three launches per iteration (pairs product, per-frame finish, per-frame update).  alpha / beta live on
// the device: the last workgroup of k_matvec_finish / k_cg_update reduces the per-frame partial dot products
// (agent-scope release/acquire ticket), so there is neither a scalar kernel nor a host round trip in the loop.
namespace {
struct TailStalled {};  // k_pcg_tail's grid barrier was abandoned (its workgroups were not co-resident: the device is shared)
}
static int runPcgAttempt(Ctx& c, const double* x, const std::function<void()>& tail);
int runPcg(Ctx& c, const double* x, const std::function<void()>& tail) {
  const size_t firstTimerSlot = c.h->evUsed;
  try {
    return runPcgAttempt(c, x, tail);
  } catch (const TailStalled&) {
    //  not an error: the fused tail is an optimisation.  The handle falls back to the two-launch path for good and
    // the solve is repeated from its start (the PCG's inputs -- g, lam, the block inverses, the levels -- are untouched; its
    // state vectors and last-workgroup tickets are re-initialised).
    //  EVERY ticket and counter a half-finished fused iteration may have left behind is reset -- the update / finish
    // tickets, the levels' (temporal node sums), the barrier words (the attempt re-zeroes them too) -- and the timer slots of the
    // abandoned attempt are dropped, so the kernel-time averages hold the repeated solve only.
    cvd_handle* h = c.h;
    HIP_CHECK(hipStreamSynchronize(h->stream));
    HIP_CHECK(hipMemsetAsync(h->dCounters.p, 0, 8 * sizeof(unsigned int), h->stream));
    // (the shares mode's words behind the scalars: the abandon flag, the ring, the shares -- the mirror's address in front stays)
    HIP_CHECK(hipMemsetAsync(h->dScal.p + SH_ABANDON, 0, (SH_END - SH_ABANDON) * sizeof(double), h->stream));
    h->sharesF = h->sharesN = -1;
    if (h->temporal.counter.p) HIP_CHECK(hipMemsetAsync(h->temporal.counter.p, 0, 4 * sizeof(unsigned int), h->stream));
    if (h->dTailBar.p)
      HIP_CHECK(hipMemsetAsync(h->dTailBar.p, 0, static_cast<size_t>(kTailBarStride) * (1 + kTailBarCopies) * sizeof(unsigned int), h->stream));
    h->curPcgIter = -1;
    h->tDropFrom(firstTimerSlot, 0);
    h->tailDisabled = true;
    fprintf(stderr, "[cvd] warning: k_pcg_tail's grid barrier was abandoned (device shared with other work?); this handle uses the "
                    "two-launch PCG tail from here on\n");
    return runPcgAttempt(c, x, tail);
  }
}
static int runPcgAttempt(Ctx& c, const double* x, const std::function<void()>& tail) {
  cvd_handle* h = c.h;
  hipStream_t s = h->stream;
  const int F = c.L.F;
  const size_t B = c.L.B;
  if (B > 512) throw std::runtime_error("frame block larger than 512 unknowns is not supported by k_cg_update");
  prepareMatvec(c, x);
  const int nChunks = static_cast<int>((B + 63) / 64);
  const int nThreads = (B > 256 ? 128 : 256) * nChunks;  // (k_cg_update: four segments per row up to B = 256, two beyond)
  double* fd = h->dFdot.p;
  size_t ldsU = (B + cgUpdatePartDoubles(static_cast<int>(B), nThreads) + 48 + 17 * kCB) * 8;
  const double tol2 = c.h->opt.pcg_relative_tolerance * c.h->opt.pcg_relative_tolerance;
  for (int i = 0; i < 9; ++i) h->hPcg[i] = 0.0;  // device progress mirror (pcgFinishScalars): nothing applied yet
  const bool coarse = h->coarseOn;
  double* rc = coarse ? h->coarse.rc.p : nullptr;
  // Coarse level per iteration: y = W Z^T r is kept up to date inside k_cg_update (CoarseStep: y <- y - alpha W Z^T q,
  // |y|^2 closes r^T z), so only c = W^T y remains as a launch; the first residual goes through k_coarse_apply_w.
  const bool denseCoarse = coarse && h->coarse.denseMode;
  const bool unfusedY = denseCoarse;  // (the dense level has no W to recur on: Z^T r is restricted every iteration)
  auto coarseC = [&](int init) {
    if (c.L.positionRegSqrt > 0.0 || c.trip || !coarseFusedConsumers())
      hipLaunchKernelGGL(k_coarse_apply_wt, dim3(F), dim3(256), 0, s, coarseView(h, true, true), F, h->coarse.c.p,
                         h->dScal.p, init);
  };
  // coarse_level 3: the temporal pose level -- dense-mode plumbing (exchange layout, in-line build), but its rows are walked by
  // kCB extra workgroups of the update launch (tlLevelRows) and no workgroup streams an 8F x 8F inverse
  const bool poseT = denseCoarse && h->coarse.temporalPose;
  auto coarseApply = [&](int init) {
    if (poseT) {
      launchPoseTemporalInit(c, tol2);  // (first residual only: the iterations carry the level inside k_cg_update / k_pcg_tail)
      return;
    }
    if (denseCoarse) {
      hipLaunchKernelGGL(k_coarse_dense_apply, dim3(F), dim3(256), 0, s, F, h->coarse.denseInv.p, h->coarse.rc.p, h->coarse.c.p,
                         h->coarse.modeActive.p, h->coarse.dotPart.p, h->dScal.p, h->dCounters.p + 3, h->coarse.fail.p, init,
                         tol2, h->hPcg);
      return;
    }
    hipLaunchKernelGGL(k_coarse_apply_w, dim3(F), dim3(1024), 0, s, h->coarse.plan, h->coarse.Wb.p, h->coarse.rc.p,
                       h->coarse.y.p, h->coarse.dotPart.p, h->dScal.p, h->dCounters.p + 3, h->coarse.fail.p, init, tol2,
                       h->hPcg);
    coarseC(init);
  };
  const CoarseStep csOff{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  const CoarseStep csOn = (coarse && !unfusedY)
                              ? CoarseStep{h->coarse.wtPtr.p, h->coarse.wtBlk.p, h->coarse.wtFrame.p, h->coarse.Wb.p,
                                           h->coarse.qc.p, h->coarse.y.p, h->coarse.fdotY.p, h->coarse.fail.p, h->coarse.wq.p}
                              : csOff;
  const DenseStep dsOff{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, kCB, 0, nullptr};
  // dense level: c <- c - alpha A_c^-1 Z^T q inside k_cg_update (F extra workgroups) instead of a launch of its own
  const bool denseFused = denseCoarse;
  // pair-sharded mode with the fused exchange (cvd_matvec.hip): Z^T q and p.q arrive all-reduced behind q
  const bool fusedX = h->dist() && fusedExchange(h, coarse);
  const double* pqReduced = fusedX ? h->dQ.p + exchangeOffsetPq(c, denseFused) : nullptr;
  const bool denseRows = denseFused && !poseT;
  const DenseStep dsOn = denseRows ? DenseStep{h->coarse.denseInv.p, fusedX ? h->dQ.p + exchangeOffsetQc(c) : h->coarse.qc.p, h->coarse.rc.p, h->coarse.c.p,
                                                h->coarse.dotPart.p, h->coarse.modeActive.p, h->coarse.fail.p,
                                                // (two launches: the split costs 2 % -- the frame workgroups are this kernel's long
                                                // pole already; it pays in k_pcg_tail, whose DenseStep launchPcgTail builds)
                                                kCB, static_cast<int>(ldsU / 8), h->coarse.dotPart.p + F}
                                    : dsOff;
  if (denseRows) {
    // (dense-level workgroups: Z^T q + partial sums; frame workgroups walking rows of their own: the same again behind their region)
    const size_t dense = static_cast<size_t>(F) * kCB + nThreads + 16;
    ldsU = std::max((dsOn.rowSplit < kCB ? ldsU / 8 + dense : ldsU / 8), dense) * 8;
  }
  // third level (cvd_temporal.h): S more workgroups of the update launch (q_T and the coefficients of one coarse hat in LDS)
  const TlStep tsOn = temporalStep(h);
  const int nTlWg = tsOn.Ainv != nullptr ? tsOn.S * tsOn.parts : 0;
  if (nTlWg) ldsU = std::max(ldsU, static_cast<size_t>(tlRowsLds(tsOn.NT)) * 8);
  const int nPtWg = poseT ? kCB * tlParts(h->coarse.ptNn) : 0;
  if (poseT) ldsU = std::max(ldsU, static_cast<size_t>(tlRowsLds(h->coarse.ptN)) * 8);
  const TlStep* tpDev = poseT ? poseTemporalStepDev(h) : nullptr;
  allowLds(k_cg_update, ldsU);
  hipLaunchKernelGGL(k_cg_update, dim3(F), dim3(nThreads), ldsU, s, c.L, 1, h->dG.p, h->dMinv.p, h->dP0.p, h->dQ.p,
                     h->dScal.p, h->dCounters.p + 1, h->dDx.p, h->dR.p, h->dZ.p, fd + F, fd + 2 * F, tol2, rc,
                     h->coarse.modeActive.p, h->hPcg, csOff, dsOff, static_cast<const double*>(nullptr), 0, F,
                     static_cast<double*>(nullptr), nTlWg ? temporalStepDev(h) : static_cast<const TlStep*>(nullptr),
                     static_cast<const TlStep*>(nullptr));
  // (adds the level's part of r^T z before the pose-graph level's kernel closes the scalars -- or closes them itself)
  if (nTlWg) launchTemporalInit(c, !coarse, tol2);
  if (coarse) coarseApply(1);
  HIP_CHECK(hipGetLastError());
  double* pOld = h->dP0.p;
  double* pNew = h->dP1.p;
  // finish + update as ONE launch per iteration where the fused kernel's scope allows (k_pcg_tail, cvd_matvec.hip)
  size_t ldsTail = 0;
  int ldsFinish = 0, ldsScratch = 0;
  const bool fusedTail = pcgTailScope(c, coarse, nThreads, ldsTail, ldsFinish, ldsScratch);
  h->lastFusedTail = fusedTail;
  h->lastKD = c.KD;
  h->lastCross = c.cross;
  if (fusedTail) {  // (its grid barrier's words)
    h->dTailBar.ensure(static_cast<size_t>(kTailBarStride) * (1 + kTailBarCopies));
    HIP_CHECK(hipMemsetAsync(h->dTailBar.p, 0, static_cast<size_t>(kTailBarStride) * (1 + kTailBarCopies) * sizeof(unsigned int), s));
    // (the temporal level's node-sum records carry the barrier's generation, which restarts with its words)
    if (tsOn.rec != nullptr) HIP_CHECK(hipMemsetAsync(tsOn.rec, 0, 2 * static_cast<size_t>(tsOn.NT) * sizeof(double), s));
  }
  // ... and whether that tail leaves the sum of its r^T z shares to the next product (pcgSharesScope)
  PcgShares sharesLayout;
  const bool shares = fusedTail && pcgSharesScope(c, coarse, sharesLayout);
  h->lastShares = shares;
  h->lastShareCount = shares ? sharesLayout.count : 0;
  if (shares && (h->sharesF != F || h->sharesN != sharesLayout.count)) {
    // the sums run over the whole arrays: the words beyond this solve's shares must be zero (a solve with the same layout
    // overwrites every word the last one wrote)
    HIP_CHECK(hipMemsetAsync(h->dScal.p + SH_RZ, 0, 2 * static_cast<size_t>(kPcgSharesCap) * sizeof(double), s));
    h->sharesF = F;
    h->sharesN = sharesLayout.count;
  }
  const bool ownerMode = ownerShardedUpdate(h, coarse);
  const int maxIt = std::max(1, c.h->opt.pcg_max_iterations);
  // Convergence is decided on the device (S_DONE, set by the last workgroup of k_cg_update); how far the host runs ahead of it
  // is described at the loop below.
  // (profiling aid: cvd_solver_options::pcg_lockstep checks after every iteration and never runs ahead, so that per-launch
  // counter averages contain no early-exit launches)
  const bool lockstep = h->dbg.pcg_lockstep != 0;
  const size_t firstTimerSlot = h->evUsed;
  int enq = 0;
  auto enqueueIteration = [&](int it, int useBeta) {
    h->curPcgIter = it;
    if (fusedTail) {
      // (shares mode: the product of iteration `it` >= 1 closes iteration it - 1; the first one has nothing to close)
      launchMatvec(c, x, h->dZ.p, pOld, pNew, useBeta, h->dLam.p, h->dQ.p, coarse, true, shares ? it : 0);
      launchPcgTail(c, x, pOld, pNew, useBeta, h->dLam.p, h->dQ.p, coarse, nThreads, ldsTail, ldsFinish, ldsScratch, tol2,
                    shares ? &sharesLayout : nullptr);
      std::swap(pOld, pNew);
      return;
    }
    launchMatvec(c, x, h->dZ.p, pOld, pNew, useBeta, h->dLam.p, h->dQ.p, coarse);
    if (ownerMode) {
      // ---- owner-sharded iteration: the exchange above left the reduced q of THIS rank's frames (and [Z^T q | p.q] everywhere);
      // update the own frames, gather z / c / the r^T z shares, finish the scalars
      const int f0 = h->ownFirst(), nOwn = h->ownCount();
      const int slotO = h->tBegin(KC_CG_UPDATE);
      if (nOwn > 0 || nTlWg || nPtWg)  // (a rank without frames still walks the temporal levels' rows: every rank keeps its own copy of t / tl)
        hipLaunchKernelGGL(k_cg_update, dim3((denseRows && dsOn.rowSplit > 0 ? nOwn + (nOwn + kDenseFramesPerGroup - 1) / kDenseFramesPerGroup : nOwn) + nTlWg + nPtWg),
                           dim3(nThreads), ldsU, s, c.L, 0, h->dG.p, h->dMinv.p, pNew, h->dQ.p, h->dScal.p, h->dCounters.p + 1,
                           h->dDx.p, h->dR.p, h->dZ.p, fd + F, fd + 2 * F, tol2, static_cast<double*>(nullptr),
                           h->coarse.modeActive.p, h->hPcg, csOff, dsOn, pqReduced, f0, nOwn, h->dOwnerScal.p + 2 * h->rank,
                           nTlWg ? temporalStepDev(h) : static_cast<const TlStep*>(nullptr), tpDev);
      else
        HIP_CHECK(hipMemsetAsync(h->dOwnerScal.p + 2 * h->rank, 0, 2 * sizeof(double), s));
      HIP_CHECK(hipGetLastError());
      h->tEnd(slotO);
      const int ct = h->tBegin(KC_COMM_PRODUCT);
      const size_t chunkF = static_cast<size_t>(h->ownChunk());
      commGroupStart(h);
      commAllGather(h, h->dZ.p + h->rank * chunkF * B, h->dZ.p, chunkF * B, CT_F64, s);
      if (denseRows) commAllGather(h, h->coarse.c.p + h->rank * chunkF * kCB, h->coarse.c.p, chunkF * kCB, CT_F64, s);
      commAllGather(h, h->dOwnerScal.p + 2 * h->rank, h->dOwnerScal.p, 2, CT_F64, s);
      commGroupEnd(h);
      h->tEnd(ct);
      hipLaunchKernelGGL(k_pcg_scalars_dist, dim3(1), dim3(64), 0, s, h->dOwnerScal.p, h->world, h->dScal.p, tol2, h->hPcg);
      HIP_CHECK(hipGetLastError());
      std::swap(pOld, pNew);
      return;
    }
    const int slot = h->tBegin(KC_CG_UPDATE);
    hipLaunchKernelGGL(k_cg_update, dim3((denseRows && dsOn.rowSplit > 0 ? F + (F + kDenseFramesPerGroup - 1) / kDenseFramesPerGroup : F) + nTlWg + nPtWg), dim3(nThreads), ldsU, s, c.L, 0, h->dG.p, h->dMinv.p, pNew,
                       h->dQ.p, h->dScal.p, h->dCounters.p + 1, h->dDx.p, h->dR.p, h->dZ.p, fd + F, fd + 2 * F, tol2,
                       (coarse && unfusedY && !denseFused) ? rc : nullptr, h->coarse.modeActive.p, h->hPcg, csOn, dsOn, pqReduced,
                       0, F, static_cast<double*>(nullptr), nTlWg ? temporalStepDev(h) : static_cast<const TlStep*>(nullptr), tpDev);
    if (coarse && !denseFused) { if (unfusedY) coarseApply(0); else coarseC(0); }
    HIP_CHECK(hipGetLastError());
    h->tEnd(slot);
    std::swap(pOld, pNew);
  };
  // (Replaying the batch as a hipGraph was tried: the ~6 us between the five dependent launches of an iteration are
  // device-side dependency resolution, not host launch latency -- no gain, removed.)
  // Convergence is decided on the device (S_DONE); the last workgroup of every iteration also mirrors its progress
  // into pinned host memory (pcgFinishScalars).  Iteration k is enqueued once the done flag after exactly
  // k - kRunAhead + 1 iterations is known to be clear: nothing but the PCG kernels is in the stream, the device is
  // never starved (kRunAhead iterations are queued ahead) and kRunAhead - 1 early-exit iterations are wasted per
  // solve.  The rule is a function of iteration counts only, hence identical on all ranks of a sharded run.
  const int kRunAhead = lockstep ? 1 : 2;  // (3-4 iterations ahead: no change, the host is not late)
  volatile double* prog = h->hPcg;
  while (enq < maxIt) {
    if (enq >= kRunAhead - 1) {
      const int need = enq - kRunAhead + 1;
      // slot 1 + (need & 7) = 4 (need + 1) + done flag once exactly `need` iterations have been applied
      double v;
      for (unsigned long long spins = 0; static_cast<long long>((v = prog[1 + (need & 7)]) * 0.25) != need + 1; ++spins) {
        if ((spins & 0xFFFFF) == 0xFFFFF) {
          // never spin forever on a mirror that cannot advance: a faulted stream reports here, and an idle stream
          // whose iterations did not publish progress is a logic error
          const hipError_t e = hipStreamQuery(s);
          if (e != hipErrorNotReady) {
            HIP_CHECK(e);
            if (static_cast<long long>(prog[1 + (need & 7)] * 0.25) != need + 1) {
              if (fusedTail) throw TailStalled{};
              throw std::runtime_error("PCG progress mirror stalled");
            }
          }
        }
      }
      if (v - 4.0 * (need + 1) != 0.0) break;
    }
    enqueueIteration(enq, enq > 0 ? 1 : 0);
    ++enq;
    // (test hook, cvd_debug_options::stall_fused_tail_once: the host behaves as if the fused tail's barrier had been abandoned in the middle of the
    // first solve it is used in -- exercises the recovery path above without needing a second tenant on the device)
    if (fusedTail && h->dbg.stall_fused_tail_once != 0 && enq == 3) throw TailStalled{};
    if (h->opt.verbose >= 2) {  // development trace: per-iteration scalars (synchronises every iteration)
      readScalars(c);
      std::printf("    pcg %3d  rz %.6e  rzpart %.6e  alpha %.6e  beta %.6e  pq %.6e  done %g\n", enq - 1, h->hScal[S_RZ],
                  h->hScal[S_RZPART], h->hScal[S_ALPHA], h->hScal[S_BETA], h->hScal[S_PQ], h->hScal[S_DONE]);
    }
  }
  h->curPcgIter = -1;
  // shares mode: no product follows the last enqueued tail -- one workgroup sums its shares and finishes the scalars (a no-op when
  // the PCG is done, a barrier was abandoned or the iteration is closed)
  if (shares && enq > 0) launchPcgClose(c, enq);
  if (ownerMode) {
    // the step and the residual of the frames live on their owners: everybody needs both (step statistics, candidate point)
    const int ct = h->tBegin(KC_COMM_PRODUCT);
    const size_t chunk = static_cast<size_t>(h->ownChunk()) * B;
    commGroupStart(h);
    commAllGather(h, h->dDx.p + h->rank * chunk, h->dDx.p, chunk, CT_F64, s);
    commAllGather(h, h->dR.p + h->rank * chunk, h->dR.p, chunk, CT_F64, s);
    commGroupEnd(h);
    h->tEnd(ct);
  }
  if (tail) tail();  // follow-up work that does not need the host's decision rides on the same read-back
  readScalars(c);    // drains the stream; S_DONE / S_ITERS are final
  if (h->hScal[S_DONE] == 2.0) throw std::runtime_error("PCG produced NaN");
  const int iters = static_cast<int>(h->hScal[S_ITERS]);
  // The run-ahead check above never looks at the last kRunAhead - 1 enqueued iterations: an abandon there shows as iterations that
  // were enqueued before convergence and never applied.
  if (fusedTail && h->hScal[S_DONE] == 0.0 && iters != enq) throw TailStalled{};
  h->tDropFrom(firstTimerSlot, iters);
  return iters;
}

// Scene-flow smoothness triplets of this problem (reference lib/PoseOptimizer.cpp:899): on when a weight is > 0.
bool wantsTriplets(const cvd_opt_params& p, ProblemKind kind) {
  return kind == PK_POSE_STEP && (p.smooth_static_weight > 0.0 || p.smooth_dynamic_weight > 0.0);
}
void bindTriplets(Ctx& c, const cvd_opt_params& p, ProblemKind kind) {
  cvd_handle* h = c.h;
  c.trip = wantsTriplets(p, kind) && c.L.includeStatic;
  if (!c.trip) return;
  c.TT = TripletTable{h->dTNdc.p, h->dTDsrc.p, h->dTStatic.p, h->dTOff.p, h->dTCenter.p, h->dTSlot.p,
                      static_cast<int>(h->tripActive.size()),
                      static_cast<int>(p.smooth_loss_type),  // (CVD_SMOOTH_* == kSmooth*)
                      std::sqrt(std::max(0.0, p.smooth_static_weight)), std::sqrt(std::max(0.0, p.smooth_dynamic_weight))};
}

namespace {

// verbose >= 3 (development): where a solve's fixed cost goes.  tools/setup_phases.py reads the labels.
struct SetupPhases {
  bool on;
  double t = nowSeconds();
  void operator()(const char* what) {
    if (!on) return;
    const double now = nowSeconds();
    fprintf(stderr, "[setup] %-14s %8.1f us\n", what, (now - t) * 1e6);
    t = now;
  }
};

// What solve() and evaluate() do differently while they bind a problem.
struct BindMode {
  bool checkBlock;    // checkFrameBlock before any state is touched
  bool staticGuards;  // the dense-list scope and the dense-scope check only for a problem with static constraints (else: always)
  bool levels;        // the preconditioner's levels per the options, with their tables (else: coarseOn off, their state untouched)
};
struct BoundProblem {
  Ctx c;
  // dense mode outside the fast kernels' scope: the problem runs on the device-materialised list (flipped back when it goes out of scope)
  std::optional<DenseListScope> denseList;
};

// Layout through the state upload.  compileTable, DenseListScope and ensureBuffers mutate the handle: the order is behaviour.
void bindProblem(BoundProblem& b, cvd_handle* h, const cvd_opt_params& p, double depthDeformReg, ProblemKind kind,
                 const std::vector<int>& range, const BindMode& mode, SetupPhases& phase) {
  Ctx& c = b.c;
  c.h = h;
  c.L = makeLayout(h, p, depthDeformReg, kind);
  if (mode.checkBlock) checkFrameBlock(static_cast<size_t>(c.L.B), "solve");
  tapCounts(c.L, c.KD, c.KS);
  phase("layout");
  const bool guarded = !mode.staticGuards || c.L.includeStatic;
  b.denseList.emplace(h, h->dense && guarded && !denseFastScope(h, c.L, c.KS, wantsTriplets(p, kind)));
  compileTable(h, range, wantsTriplets(p, kind), kind == PK_NORMALIZE && c.L.includeStatic);
  orderTable(h, c.L, c.KD);
  phase("table");
  refreshMedians(h);
  phase("medians");
  c.T = makeTable(h);
  c.nItems = static_cast<int>(h->itemFa.size());
  c.it = Items{h->dItemFa.p, h->dItemFb.p, h->dItemRange.p, h->dItemSlot.p, c.nItems, h->dItemRec.p};
  c.n = static_cast<size_t>(c.L.F) * c.L.B;
  c.boundDepth0 = (kind == PK_NORMALIZE && c.L.N > 0) ? 1 : 0;
  bindTriplets(c, p, kind);
  if (guarded) checkDenseScope(h, c.L, c.KS, c.trip);
  c.cross = crossScope(h, c);
  h->coarseOn = mode.levels && h->opt.coarse_level != 0 && h->coarse.valid && c.L.includeStatic && h->coarse.nEdges > 0 &&
                !h->forceGeneric && kind == PK_POSE_STEP;  // (normalizeDepth's problems have no pose unknowns: the block-Jacobi level alone)
  ensureBuffers(c);
  phase("buffers");
  if (mode.levels) {
    h->coarse.ptInvPending = false;   // (a request left behind by a solve that threw)
    h->temporal.on = temporalScope(c);
    if (h->temporal.on) h->temporal.on = temporalPrepare(c);
    phase("level 3 tables");
    if (h->coarseOn && h->coarse.temporalPose) poseTemporalPrepare(c);
    phase("level 2 tables");
  }
  buildMask(h, c.L, p, kind, range);
  phase("mask");
  uploadState(h, c.L, h->dX);
  phase("upload");
}

// Residual blocks besides the static constraints': the triplets' and the regularisers', as Ceres would count them.
long long countResidualBlocks(const Ctx& c, const std::vector<int>& range) {
  const cvd_handle* h = c.h;
  const long long nr = static_cast<long long>(range.size());
  long long blocks = c.trip ? h->numValidTrip : 0;
  if (c.L.scaleRegSqrt > 0.0) blocks += nr * c.L.sregX * c.L.sregY;
  if (c.L.focalRegSqrt > 0.0) blocks += nr;
  if (c.L.depthDeformW > 0.0 && c.L.depthType == CVD_DEPTH_GRID) blocks += nr;
  if (c.L.spatialDeformW > 0.0 && c.L.nS > 0) blocks += nr;
  if (c.L.positionRegSqrt > 0.0)
    for (int k = c.L.firstFrame; k < c.L.lastFrame - 1; ++k)
      blocks += (h->tableRange[k] && h->tableRange[k + 1] && h->tableRange[k + 2]) ? 1 : 0;
  return blocks;
}

// A coarse rebuild still running on the side stream when the solve ends (or throws) must finish before anything on the
// main stream -- the next solve's in-line setup, a table upload -- touches the coarse buffers again.
struct PendingGuard {
  cvd_handle* h;
  const LevelSchedule& schedule;  // (pending: a rebuild is running on the side stream)
  bool inverseAside = false;      // the block inverses were forked to their own stream and the solve left before the join
  ~PendingGuard() {
    if (schedule.pending) (void)hipStreamWaitEvent(h->stream, h->evCoarseDone, 0);
    if (inverseAside) (void)hipStreamWaitEvent(h->stream, h->evInvDone, 0);
    if (h->temporal.sidePending) {  // (the third level's assembly was forked and the solve left before its join)
      (void)hipStreamWaitEvent(h->stream, h->temporal.evDone, 0);
      h->temporal.sidePending = false;
    }
  }
};

// the depth-grid level by itself, both halves, at the current (H, lam, x)
void rebuildTemporalLevel(Ctx& c) {
  cvd_handle* h = c.h;
  const int slot = h->tBegin(KC_INVERSE);
  launchTemporalSetup(c, h->dX.p, 0);
  launchTemporalSetup(c, h->dX.p, 1);
  h->tEnd(slot);
}

// Carries out one LM iteration's schedule decision: the block-Jacobi level, which follows lam every LM iteration (lagging it as
// well is ~4% faster on the benchmark but makes the converged parameters visibly sensitive to rounding noise along the weak gauge
// directions), and whatever rebuild of the other levels the decision asks for.
void buildLevels(Ctx& c, const LevelSchedule::Decision& d, PendingGuard& guard) {
  cvd_handle* h = c.h;
  hipStream_t s = h->stream;
  if (d.inverseAside) {
    // The levels are built in line: the frames' block inverses -- one workgroup per frame, a latency-bound sweep of 0.12 - 0.17 ms
    // that leaves most of every CU idle, and that only the PCG reads -- run on a stream of their own BESIDE the build instead of
    // in front of it.
    HIP_CHECK(hipEventRecord(h->evInvIn, s));
    HIP_CHECK(hipStreamWaitEvent(h->stream3, h->evInvIn, 0));
    launchBlockInverse(c, h->stream3);
    HIP_CHECK(hipEventRecord(h->evInvDone, h->stream3));
    guard.inverseAside = true;
  } else {
    const int slot = h->tBegin(KC_INVERSE);
    launchBlockInverse(c);
    h->tEnd(slot);
  }
  if (d.coarse == LevelSchedule::SIDE_STREAM) {
    // The rebuild runs concurrently with this iteration's PCG (which keeps the old factor) and is installed for the next iteration:
    // its ~0.8 ms leave the critical path.  Its inputs (H, lam, x, mask, the table) are not written before the install; the frame
    // constants, which the main stream rewrites for the candidate point, are private to the side stream.
    h->dFc2.ensure(c.L.F);
    //  the third level is "rebuilt together with the pose-graph level": also when that rebuild runs on the side
    // stream -- at this linearisation point, for THIS iteration's PCG (it is small: two launches and a 0.1 ms inverse).
    //  its assembly goes to the side stream BEFORE the pose-graph level's rebuild: queued behind it, the main
    // stream's wait for the third level would have been a wait for the whole rebuild the side stream exists to hide.
    // Its inverse (a persistent kernel: gated per device) is enqueued before the rebuild's factorisation as well, so that the
    // gate's event chain makes the SIDE stream wait for the small inverse and not the solver's stream for the rebuild; the two
    // levels' inverses have scratch (panel, barrier words) of their own.
    if (h->temporal.on) rebuildTemporalLevel(c);
    HIP_CHECK(hipEventRecord(h->evCoarseIn, s));
    HIP_CHECK(hipStreamWaitEvent(h->stream2, h->evCoarseIn, 0));
    launchCoarseSetup(c, h->dX.p, 1);
    HIP_CHECK(hipEventRecord(h->evCoarseDone, h->stream2));
  } else if (d.coarse == LevelSchedule::IN_LINE) {
    const int slot = h->tBegin(KC_INVERSE);  // preconditioner construction, same class as the block inverse
    const bool measure = h->coarse.denseMode && !h->dist() && h->opt.coarse_rebuild_excess_dense < 0;
    if (measure) {
      if (!h->evRebuild[0]) for (auto& e : h->evRebuild) HIP_CHECK(hipEventCreate(&e));
      HIP_CHECK(hipEventRecord(h->evRebuild[0], s));
    }
    // (third level: same linearisation point and damping; its assembly runs beside the pose-graph level's build)
    if (h->temporal.on) launchTemporalSetup(c, h->dX.p, 0);
    launchCoarseSetup(c, h->dX.p);
    if (d.inverseAside) {  // (joined before the temporal levels' persistent inverse pair: that kernel keeps the device to itself)
      HIP_CHECK(hipStreamWaitEvent(s, h->evInvDone, 0));
      guard.inverseAside = false;
    }
    if (h->temporal.on) launchTemporalSetup(c, h->dX.p, 1);
    if (measure) {
      HIP_CHECK(hipEventRecord(h->evRebuild[1], s));
      h->rebuildTimed = true;
    }
    h->tEnd(slot);
  }
  if (d.temporalOnly) rebuildTemporalLevel(c);
}

// a factor the side stream finished during this iteration's PCG is swapped in for the next one
void installPendingCoarse(cvd_handle* h, LevelSchedule& schedule) {
  if (!schedule.pending) return;
  HIP_CHECK(hipStreamWaitEvent(h->stream, h->evCoarseDone, 0));  // (device-side wait: the host does not block)
  std::swap(h->coarse.Wb.p, h->coarse.Wb2.p);
  std::swap(h->coarse.Wb.n, h->coarse.Wb2.n);
  std::swap(h->coarse.fail.p, h->coarse.fail2.p);
  std::swap(h->coarse.fail.n, h->coarse.fail2.n);
  schedule.installed();
}

// what denseRebuildThreshold's -1 setting prices a rebuild with: the handle's running averages of an in-line rebuild and a PCG iteration
void notePcgTime(cvd_handle* h, double seconds, int cgIters) {
  if (cgIters <= 0 || h->dist()) return;
  double ms = seconds * 1e3;
  if (h->rebuildTimed) {  // (the rebuild ran in line right before this PCG: its time is not the iterations')
    float rb = 0.f;
    if (hipEventElapsedTime(&rb, h->evRebuild[0], h->evRebuild[1]) == hipSuccess && rb > 0.f) {
      h->coarseRebuildMs = h->coarseRebuildMs > 0.0 ? 0.5 * (h->coarseRebuildMs + rb) : rb;
      ms = std::max(0.0, ms - rb);
    }
    h->rebuildTimed = false;
  }
  const double per = ms / cgIters;
  h->pcgIterMs = h->pcgIterMs > 0.0 ? 0.75 * h->pcgIterMs + 0.25 * per : per;
}

// one iteration record at the current point's cost and radius, with its line of the verbose table
void pushRecord(cvd_handle* h, cvd_iteration_record& rec, double cost, double radius, double gmax, bool tableLine = true) {
  rec.cost = cost;
  rec.trust_region_radius = radius;
  h->records.push_back(rec);
  if (tableLine && h->opt.verbose)
    printf("%4d % .6e    % .2e   % .2e   % .2e  % .2e % .2e   %5d\n", rec.iteration, cost, rec.cost_change, gmax, rec.step_norm,
           rec.relative_decrease, radius, rec.linear_iterations);
}

}  // namespace

void solve(cvd_handle* h, const cvd_opt_params& p, double depthDeformReg, ProblemKind kind) {
  const double t0 = nowSeconds();
  if (h->F <= 0) throw std::runtime_error("no video set");
  if (!h->poseParamsValid) posesToParams(h);
  const std::vector<int> range = rangeOf(p, h->F);
  LevelSchedule schedule;
  PendingGuard guard{h, schedule};
  SetupPhases phase{h->opt.verbose >= 3};
  BoundProblem bound;
  bindProblem(bound, h, p, depthDeformReg, kind, range, BindMode{/*checkBlock*/ true, /*staticGuards*/ true, /*levels*/ true}, phase);
  Ctx& c = bound.c;
  hipStream_t s = h->stream;
  HIP_CHECK(hipMemsetAsync(h->dDx.p, 0, c.n * sizeof(double), s));
  HIP_CHECK(hipMemsetAsync(h->dR.p, 0, c.n * sizeof(double), s));
  HIP_CHECK(hipMemsetAsync(h->dFail.p, 0, sizeof(int), s));

  cvd_solve_summary sum{};
  sum.num_residual_blocks = static_cast<int>((c.L.includeStatic ? h->numValid : 0) + countResidualBlocks(c, range));
  double tEval = 0.0, tLin = 0.0;
  double te = nowSeconds();
  // first evaluation: cost, |g|_max, |x| and the number of active unknowns arrive with ONE read-back (until round 5: the cost, then the
  // statistics, then a downloaded copy of diag(H) counted on the host -- three round trips of 25 - 55 us at the start of every solve)
  double xCost = evalFull(c, h->dX.p, true, false);
  tEval += nowSeconds() - te;
  sum.initial_cost = xCost;
  phase("first eval");
  double gmax = h->hScal[S_GMAX];
  double xNorm = std::sqrt(h->hScal[S_XX]);
  sum.num_parameters = static_cast<int>(h->hScal[S_NACTIVE] + 0.5);
  phase("stats");

  TrustRegion tr;
  // (sparse factor, rebuilt on the side stream: the option; dense level, built in line: denseRebuildThreshold)
  const int rebuildExcess = h->coarse.denseMode ? denseRebuildThreshold(h->opt.coarse_rebuild_excess_dense, h->dist(), h->coarseRebuildMs, h->pcgIterMs)
                                                : h->opt.coarse_rebuild_excess;
  const LevelSchedule::Config levels{h->opt.coarse_level, h->opt.temporal_level, std::max(0, rebuildExcess), h->coarseOn, h->temporal.on,
                                     h->coarse.denseMode, h->dist(), h->stream3 != nullptr, c.L.B <= 256};
  // After an accepted step the host does not wait for the new point's |g|_max / |x| (one idle round trip of ~60 us per LM
  // iteration, round 5): the step statistics of the NEXT PCG solve recompute both for the same point (k_step_stats) and arrive
  // with its read-back.  gradPending: the gradient-tolerance test of the last accepted step and its record's gradient norm are
  // still open.  (verbose runs keep the immediate read: the table prints the norm with its iteration)
  bool gradPending = false;
  const bool deferStats = h->opt.verbose == 0;
  auto gradientConverged = [&]() { return gmax <= Ceres::gradient_tolerance && !h->dbg.force_iterations; };
  int iteration = 0, termination = 1;
  bool scaleDone = false;
  cvd_iteration_record r0{};
  r0.gradient_max_norm = gmax;
  r0.step_is_successful = 1;
  if (h->opt.verbose) printf("iter      cost      cost_change  |gradient|   |step|    tr_ratio  tr_radius  ls_iter\n");
  pushRecord(h, r0, xCost, tr.radius, gmax);

  if (sum.num_parameters == 0 || gradientConverged()) {
    termination = 0;
  } else {
    while (true) {
      if (iteration >= p.max_iterations) { termination = 1; break; }
      if (tr.belowMinRadius()) { termination = 0; break; }
      ++iteration;
      cvd_iteration_record rec{};
      rec.iteration = iteration;

      double tl = nowSeconds();
      hipLaunchKernelGGL(k_lm_diag, dim3((c.n + 255) / 256), dim3(256), 0, s, c.L, h->dHd.p, h->dScale.p,
                         scaleDone ? 0 : 1, tr.radius, h->dLam.p);
      scaleDone = true;
      buildLevels(c, schedule.decide(levels), guard);
      // one read-back for the PCG result, the step statistics and the cost of the candidate point (the
      // candidate is formed speculatively; it is simply not used when the model decrease is invalid)
      const double tPcgStart = nowSeconds();
      const int cgIters = runPcg(c, h->dX.p, [&]() {
        enqueueStats(c);
        hipLaunchKernelGGL(k_apply_step, dim3((c.n + 255) / 256), dim3(256), 0, s, c.L, c.boundDepth0, h->dX.p,
                           h->dDx.p, h->dXc.p);
        HIP_CHECK(hipGetLastError());
        enqueueCost(c, h->dXc.p);
      });
      notePcgTime(h, nowSeconds() - tPcgStart, cgIters);
      schedule.afterPcg(cgIters);
      installPendingCoarse(h, schedule);
      tLin += nowSeconds() - tl;
      if (gradPending) {
        gradPending = false;
        gmax = h->hScal[S_GMAX];
        xNorm = std::sqrt(h->hScal[S_XX]);
        h->records.back().gradient_max_norm = gmax;
        if (gradientConverged()) {
          // the previous iteration ended the solve (Ceres tests the gradient right after a successful step): this iteration's
          // linear solve was speculative and is dropped -- x, the cost and the records are those of the previous iteration
          --iteration;
          termination = 0;
          break;
        }
      }
      rec.linear_iterations = cgIters;
      sum.total_linear_iterations += cgIters;
      const double dg = h->hScal[S_DG], dr = h->hScal[S_DR], dld = h->hScal[S_DLD], dd = h->hScal[S_DD];
      const double modelCostChange = -0.5 * dg + 0.5 * dr + 0.5 * dld;
      if (!(std::isfinite(modelCostChange) && modelCostChange > 0.0 && std::isfinite(dd))) {
        if (!tr.invalidStep()) { termination = 2; break; }
        pushRecord(h, rec, xCost, tr.radius, gmax, false);
        continue;
      }
      tr.validStep();
      double candCost = h->hScal[S_COST];
      if (!std::isfinite(candCost)) candCost = std::numeric_limits<double>::max();
      rec.step_norm = std::sqrt(dd);
      rec.cost_change = xCost - candCost;
      rec.relative_decrease = (xCost - candCost) / modelCostChange;
      if (!h->dbg.force_iterations &&
          (TrustRegion::parameterToleranceReached(rec.step_norm, xNorm) || TrustRegion::functionToleranceReached(xCost, candCost))) {
        pushRecord(h, rec, xCost, tr.radius, gmax);
        termination = 0;
        break;
      }
      if (rec.relative_decrease > Ceres::min_relative_decrease) {
        std::swap(h->dX.p, h->dXc.p);
        std::swap(h->dX.n, h->dXc.n);
        schedule.accepted(std::abs(xCost - candCost) / std::max(std::abs(xCost), 1e-300));
        xCost = candCost;
        te = nowSeconds();
        // (the last iteration allowed reads at once: nothing follows that would bring the statistics)
        gradPending = deferStats && iteration < p.max_iterations;
        (void)evalFull(c, h->dX.p, true, gradPending);
        tEval += nowSeconds() - te;
        if (!gradPending) {  // (else gmax / xNorm keep the previous point's values until the next solve's read-back)
          gmax = h->hScal[S_GMAX];
          xNorm = std::sqrt(h->hScal[S_XX]);
        }
        ++sum.num_successful_steps;
        rec.step_is_successful = 1;
        tr.accept(rec.relative_decrease);
        rec.gradient_max_norm = gmax;
        pushRecord(h, rec, xCost, tr.radius, gmax);
        if (!gradPending && gradientConverged()) { termination = 0; break; }
      } else {
        tr.reject();
        pushRecord(h, rec, xCost, tr.radius, gmax);
      }
    }
  }
  if (gradPending) {  // (the loop left before another solve brought the last accepted point's statistics)
    HIP_CHECK(hipMemsetAsync(h->dLam.p, 0, c.n * sizeof(double), s));
    enqueueStats(c);
    readScalars(c);
    h->records.back().gradient_max_norm = h->hScal[S_GMAX];
  }
  phase("LM loop");
  // a barrier timeout of the dense coarse inverse (bit 30) only costs PCG iterations -- but it should never pass unnoticed: its
  // status word travels with the state (one host wait for both; a round trip of its own cost ~25 us per solve)
  int* failWord = reinterpret_cast<int*>(h->hScal + S_COUNT);
  *failWord = 0;
  if (h->coarseOn && h->coarse.denseMode && h->coarse.fail.p != nullptr && !h->dist())
    HIP_CHECK(hipMemcpyAsync(failWord, h->coarse.fail.p, sizeof(int), hipMemcpyDeviceToHost, s));
  downloadState(h, c.L, h->dX);
  if (*failWord & 0x40000000)
    fprintf(stderr, "[cvd] warning: the dense coarse inverse timed out at its grid barrier (device shared with other work?); "
                    "the coarse level was off for the last LM iteration(s)\n");
  phase("download");
  h->tCollect();
  sum.num_iterations = iteration;
  sum.termination = termination;
  sum.final_cost = xCost;
  sum.total_seconds = nowSeconds() - t0;
  sum.evaluate_seconds = tEval;
  sum.linear_solve_seconds = tLin;
  h->summary = sum;
}
void evaluate(cvd_handle* h, const cvd_opt_params& p, double depthDeformReg, const double* pose7,
                     double* cost, int32_t* nres, double* gradient, double* hdiag, double* hfull) {
  if (pose7) {
    h->poseParams.resize(h->F);
    for (int f = 0; f < h->F; ++f)
      for (int i = 0; i < 7; ++i) h->poseParams[f][i] = pose7[f * 7 + i];
    h->poseParamsValid = true;
  } else {
    posesToParams(h);
  }
  const std::vector<int> range = rangeOf(p, h->F);
  SetupPhases quiet{false};
  BoundProblem bound;
  bindProblem(bound, h, p, depthDeformReg, PK_POSE_STEP, range, BindMode{/*checkBlock*/ false, /*staticGuards*/ false, /*levels*/ false}, quiet);
  Ctx& c = bound.c;
  hipStream_t s = h->stream;
  double cst;
  if (!gradient && !hdiag && !hfull) {
    cst = evalCost(c, h->dX.p);
  } else {
    cst = evalFull(c, h->dX.p);
  }
  if (cost) *cost = cst;
  if (nres) *nres = static_cast<int32_t>(h->numValid + countResidualBlocks(c, range));
  if (gradient) h->dG.download(gradient, c.n, s);
  if (hdiag) {
    if (h->dist()) {  // (parity hook: collect the owners' reduced blocks)
      const size_t chunk = static_cast<size_t>(h->ownChunk()) * c.L.B * c.L.B;
      commAllGather(h, h->dH.p + static_cast<size_t>(h->rank) * chunk, h->dH.p, chunk, CT_F64, s);
    }
    h->dH.download(hdiag, c.n * c.L.B, s);
  }
  HIP_CHECK(hipStreamSynchronize(s));
  if (hfull) {
    // column j of J^T J = matvec with the unit vector e_j (lam = 0)
    std::vector<double> e(c.n, 0.0), col(c.n);
    HIP_CHECK(hipMemsetAsync(h->dLam.p, 0, c.n * sizeof(double), s));
    prepareMatvec(c, h->dX.p);
    for (size_t j = 0; j < c.n; ++j) {
      e[j] = 1.0;
      h->dZ.upload(e.data(), c.n, s);
      launchMatvec(c, h->dX.p, h->dZ.p, h->dP0.p, h->dP1.p, 0, h->dLam.p, h->dQ.p);
      h->dQ.download(col.data(), c.n, s);
      HIP_CHECK(hipStreamSynchronize(s));
      for (size_t i = 0; i < c.n; ++i) hfull[i * c.n + j] = col[i];
      e[j] = 0.0;
    }
  }
}

// One kernel of this translation unit's code object is looked up at handle creation: the HIP runtime loads a unit's device
// code at its first use, ~20 ms per unit that would otherwise land in the first solve of a process (cvd_create: loadDeviceCode).
void touchModule_solve() {
  hipFuncAttributes a;
  (void)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(k_cg_update));
}

}  // namespace cvd
