// cvd_frontend.hip -- the steps either side of the solve: constraint sampling, epipolar RANSAC flags, image operators, dense
// consumers, flow-guided and bilateral filters, feature tracks, flow consistency masks, the fine-tuning consistency,
// scene-flow and spatial losses, the parameter regulariser and the optimizer step, the fine-tuning batches, RAFT's correlation pyramid / lookup and convex
// upsampling (cvd_raftops.h: k_corr_pyramid, k_corr_lookup, k_convex_upsample), the SepConvGRU of RAFT's update block
// (cvd_raftgru.h: k_gru_gemm), its other convolutions (cvd_raftconv.h: k_raft_conv), RAFT's encoders (cvd_raftenc.h: k_enc_conv,
// k_instnorm_stats, k_instnorm_apply) and the decoder of MiDaS v2.1 (cvd_midas.h: k_midas_conv, k_midas_fold, k_midas_upsample2x), the backward of its layers
// (cvd_midas_grad.h: k_midas_wflip, k_midas_dgrad_fold, k_midas_wgrad, k_midas_wgrad_fold, k_midas_bias_grad, k_midas_upsample2x_grad,
// k_midas_head_grad, k_midas_head_grad_sum) and its
// ResNeXt backbone (cvd_resnext.h: k_rx_gconv, k_rx_conv, k_rx_fold, k_rx_maxpool) with its training form and backward
// (cvd_resnext_grad.h: k_rxg_norm_stats, k_rxg_norm_finish, k_rxg_norm_apply, k_rxg_norm_grad_sums, k_rxg_norm_grad_finish,
// k_rxg_norm_grad_apply, k_rxg_gconv_dgrad, k_rxg_wgrad, k_rxg_wgrad_fold, k_rxg_gather2, k_rxg_scatter2, k_rxg_maxpool_grad).  The only unit that includes their kernel headers and the only one that knows their device state (Frontend; the handle owns it
// through a pointer to the incomplete type).
#include "cvd_host.h"
#include "cvd_dense.h"
#include "cvd_sampling.h"
#include "cvd_imageops.h"
#include "cvd_filter.h"
#include "cvd_bilateral.h"
#include "cvd_epipolar.h"
#include "cvd_tracks.h"
#include "cvd_flowmask.h"
#include "cvd_loss_common.h"
#include "cvd_consistency.h"
#include "cvd_sceneflow.h"
#include "cvd_spatial.h"
#include "cvd_paramstep.h"
#include "cvd_batch.h"
#include "cvd_raftops.h"
#include "cvd_raftgru.h"
#include "cvd_raftconv.h"
#include "cvd_raftenc.h"
#include "cvd_midas.h"
#include "cvd_midas_grad.h"
#include "cvd_resnext.h"
#include "cvd_resnext_grad.h"
#include <rocprim/device/device_scan.hpp>
#include <rocprim/device/device_segmented_radix_sort.hpp>

namespace cvd {

constexpr int kLossMaxArrays = 17;  // real input arrays of a fine-tuning loss at most (the scene-flow loss)

// A multi-tensor table of cvd_paramstep.h on the device, kept between calls.  The static part (counts, chunk list) is rebuilt only
// when the list of element counts changes.  The dynamic part (the K pointer arrays and the records: gradients are reallocated
// between steps, the step scalars change every step) is written into one of kParamSlots slots of pinned staging and copied with
// one asynchronous copy per call; a slot is rewritten only after the event recorded behind its last copy has completed.
constexpr int kParamSlots = 4;
struct ParamTableState {
  std::vector<long long> counts;       // the tensor list the static part was built for
  bool built = false;
  int numChunks = 0;
  std::vector<int> chunkTensor;        // (outlive their uploads: a rebuild waits for the stream)
  std::vector<long long> chunkStart;
  DevBuf<long long> dCounts, dChunkStart;
  DevBuf<int> dChunkTensor;
  DevBuf<unsigned char> dDynamic;      // [K][T] addresses, then [T] ParamRecord
  unsigned char* staging = nullptr;    // pinned, kParamSlots slots of slotBytes
  size_t slotBytes = 0;
  hipEvent_t copied[kParamSlots] = {};
  bool pending[kParamSlots] = {};
  int next = 0;
  ParamTableState() = default;
  ParamTableState(const ParamTableState&) = delete;
  ParamTableState& operator=(const ParamTableState&) = delete;
  ~ParamTableState() {
    for (auto& e : copied)
      if (e) (void)hipEventDestroy(e);
    if (staging) (void)hipHostFree(staging);
  }
};

// The device-resident fine-tuning dataset of cvd_batch.h (cvd_dataset_create .. cvd_dataset_clear): images in their file layout,
// cameras, per-frame tables, the sample table and the word that counts out-of-range indices of the device entry point.
struct DatasetState {
  bool created = false;
  int F = 0, H = 0, W = 0, Q = 0, S = 0, N = 2;
  bool hasDepthOrig = false;
  int scaleMode = 0;      // 0: no scales, 1: [F] scalars, 2: [F][H][W] maps
  bool haveWarp = false;
  DevBuf<float> color, flow, depthOrig, ext, intr, scales, warp;
  DevBuf<unsigned char> mask;
  DevBuf<DatasetSample> samples;
  DevBuf<unsigned int> bad;
  DevBuf<double> params;              // staging of cvd_dataset_set_xforms
  DevBuf<unsigned char> stage;        // staging of the host-array batch: indices, then every output
  size_t npx() const { return static_cast<size_t>(H) * W; }
  void clear() {
    for (DevBuf<float>* b : {&color, &flow, &depthOrig, &ext, &intr, &scales, &warp}) b->release();
    mask.release(); samples.release(); bad.release(); params.release(); stage.release();
    created = false;
    F = H = W = Q = S = 0; N = 2;
    hasDepthOrig = haveWarp = false;
    scaleMode = 0;
  }
};

// Device state of the operators below.  Nothing is allocated before an operator runs; the staging buffers then keep their
// high-water size for the life of the handle.
struct Frontend {
  DevBuf<double> dDense;     // output of the dense consumer kernels (cvd_dense.h)
  DevBuf<float> dImgIn, dImgGray, dImgCov, dImgOut;  // cvd_imageops.h staging
  DevBuf<unsigned char> dImgMask;
  DevBuf<unsigned int> dImgTmp;
  DevBuf<float> dFltDepth, dFltOut, dFltFlowF, dFltFlowB;  // cvd_filter.h staging
  DevBuf<unsigned char> dFltMaskF, dFltMaskB;
  DevBuf<FilterCam> dFltCams;
  DevBuf<float> dBilDepth, dBilColor, dBilOut;  // cvd_bilateral.h staging
  // cvd_flowmask.h staging: colour table, pair frames, both flows, both masks, kept counts, error maps
  DevBuf<float> dFmColor;
  DevBuf<int2> dFmPairs;
  DevBuf<float2> dFmFlowAB, dFmFlowBA, dFmErr;
  DevBuf<unsigned char> dFmMaskAB, dFmMaskBA;
  DevBuf<int> dFmKept;
  // cvd_epipolar.h: constraints, offsets, per-pair normalisation, per-hypothesis F / counts (one batch of pairs), results
  DevBuf<float4> dEpiLoc;
  DevBuf<long long> dEpiOff;
  DevBuf<EpiNorm> dEpiNorm;
  DevBuf<double> dEpiF, dEpiFbest;
  DevBuf<int> dEpiCount, dEpiBest;
  DevBuf<unsigned char> dEpiFlags;
  // constraint sampling (cvd_sampling.h): result of the last cvd_sample_pair_constraints / cvd_sample_triplet_constraints
  DevBuf<float2> dSampledLoc, dSampledTrip;  // 2 resp. 3 float2 per constraint
  std::vector<long long> sampledOff, sampledTripOff;
  // feature tracks (cvd_tracks.h): the table of the last cvd_compute_tracks
  DevBuf<int> dTrkStart, dTrkLen, dTrkKeptLen, dTrkOff;
  DevBuf<unsigned char> dTrkKept;
  DevBuf<float2> dTrkLoc;
  long long trkTracks = 0, trkKeptObs = 0;
  // cvd_consistency.h / cvd_sceneflow.h: per-workgroup partial sums, per-(pair, direction or class) sums and backward factors;
  // cvd_spatial.h: per-workgroup partial sums, per-sample contrast sums.  Per operator: the device entry points use them on the
  // caller's stream.
  DevBuf<double> dConsSlab, dConsSums, dConsCoef;
  DevBuf<double> dSfSlab, dSfSums, dSfCoef;
  DevBuf<double> dSpSlab, dSpPart;
  // cvd_paramstep.h: the tables of the regulariser [0] and of the step [1] per precision, the regulariser's per-workgroup sums
  ParamTableState paramTable[2][2];
  DevBuf<double> dParamSlab;
  DatasetState dataset;      // cvd_batch.h
  // staging of the three losses' host-array entry points, which run to completion on the handle's stream one at a time and so
  // share it (runLossOnHostArrays): real inputs in the loss's own order, pair and neighbour frames, scalar results, gradient, maps
  DevBuf<unsigned char> dLossIn[kLossMaxArrays], dLossGrad, dLossMaps;
  DevBuf<int32_t> dLossFrames[2];
  DevBuf<double> dLossOut;
  // cvd_raftgru.h: sigmoid(z), r h and the state between the halves, 128 B H W floats each.  The device entry point uses them on
  // the caller's stream (the loss operators' rule: calls on one device are ordered on one stream).
  DevBuf<float> dGru;
  // cvd_raftconv.h: the update block's intermediates (cor1, cor_flo, flo1, motion_features; the stacked heads' hidden tensor lies
  // over the first two, which are dead by then), 768 B H W floats, under the same rule.
  DevBuf<float> dBlock;
  // cvd_raftenc.h: the encoder's intermediates (three rotating tensors and the downsample branch's) and the instance norm's
  // (mean, rstd) per plane, under the same rule.
  DevBuf<float> dEnc;
  DevBuf<double> dEncStats;
  // cvd_midas.h: the decoder's intermediates and the partial sums of a split convolution, under the same rule.
  DevBuf<float> dMidas, dMidasSplit;
  // cvd_midas_grad.h: the flipped, transposed filter of an input gradient and the partial sums of a split weight gradient, under
  // the same rule (an input gradient's partial sums lie in dMidasSplit: it runs the forward's convolution).
  DevBuf<float> dMidasGradW, dMidasGradSplit;
  // the head's backward: its recomputed pre-activation t, the gradient of t, its recomputed output; the per-workgroup sums
  DevBuf<float> dMidasHeadGrad;
  // the one-call decoder backward: the recomputed head input, its gradient, output_conv.0's output gradient, the path gradient and
  // five rotating tensors of the largest level
  DevBuf<float> dMidasBackward;
  DevBuf<double> dMidasHeadPart;
  // cvd_resnext.h: the backbone's intermediates and the partial sums of a split convolution, under the same rule.
  DevBuf<float> dRx, dRxSplit;
  // cvd_resnext_grad.h: the strided 1 x 1 convolution's gathered input resp. unscattered gradient, and the f64 partial sums of the
  // batch norm's reductions and of a weight gradient, under the same rule.
  DevBuf<float> dRxGrad;
  DevBuf<double> dRxGradSums;
  // the one-call block backward: the gradients between its operators
  DevBuf<float> dRxBlock;
};

std::shared_ptr<Frontend> makeFrontend() { return std::make_shared<Frontend>(); }

// HIP-event times of an operator's kernel phases.  mark() records the next event on the stream: the one before the first phase,
// then one after each phase.  collect(), once the marked events have completed, adds every closed phase's milliseconds to its
// entry of kernelMs and starts over at phase 0.  With a null kernelMs no event is created or recorded.  The entries are zeroed
// at construction, the events destroyed with the timer (also when a HIP call in between throws).
class KernelTimer {
 public:
  KernelTimer(hipStream_t stream, double* kernelMs, int phases) : s(stream), ms(kernelMs) {
    if (!ms) return;
    std::fill(ms, ms + phases, 0.0);
    ev.assign(phases + 1, nullptr);
    try {
      for (auto& e : ev) HIP_CHECK(hipEventCreate(&e));
    } catch (...) {
      destroy();
      throw;
    }
  }
  KernelTimer(const KernelTimer&) = delete;
  KernelTimer& operator=(const KernelTimer&) = delete;
  ~KernelTimer() { destroy(); }
  void mark() {
    if (ms) HIP_CHECK(hipEventRecord(ev[next++], s));
  }
  void seek(int phase) { first = next = phase; }  // the next mark() opens this phase (phases timed out of order: computeTracks)
  void wait() {                                   // host wait for the last marked event
    if (ms) HIP_CHECK(hipEventSynchronize(ev[next - 1]));
  }
  void collect() {
    for (int k = first; ms && k + 1 < next; ++k) {
      float t = 0.f;
      HIP_CHECK(hipEventElapsedTime(&t, ev[k], ev[k + 1]));
      ms[k] += t;
    }
    first = next = 0;
  }

 private:
  void destroy() {
    for (auto& e : ev)
      if (e) (void)hipEventDestroy(e);
  }
  hipStream_t s;
  double* ms;
  std::vector<hipEvent_t> ev;
  int first = 0, next = 0;
};

// Batched segmented key sort (rocprim, descending, bits 0..64): at most maxSegments segments of segLen keys each, back to back in
// `keys`; run() sorts the first `segments` of them into keysOut.  Owns the segment table and rocprim's temporary storage.
class SegmentedKeySort {
 public:
  SegmentedKeySort(int maxSegments, size_t segLen, unsigned long long* keys, unsigned long long* keysOut, hipStream_t stream)
      : len(segLen), in(keys), out(keysOut), s(stream), seg(maxSegments + 1) {
    for (int i = 0; i <= maxSegments; ++i) seg[i] = static_cast<unsigned int>(static_cast<size_t>(i) * segLen);
    dSeg.upload(seg.data(), seg.size(), s);
    sort(nullptr, tmpBytes, maxSegments);
    dTmp.ensure(tmpBytes);
  }
  void run(int segments) {
    size_t tb = tmpBytes;
    sort(dTmp.p, tb, segments);
  }

 private:
  void sort(void* tmp, size_t& bytes, int segments) {
    HIP_CHECK(rocprim::segmented_radix_sort_keys_desc(tmp, bytes, in, out, static_cast<unsigned int>(static_cast<size_t>(segments) * len),
                                                      static_cast<unsigned int>(segments), dSeg.p, dSeg.p + 1, 0, 64, s));
  }
  size_t len, tmpBytes = 0;
  unsigned long long *in, *out;
  hipStream_t s;
  std::vector<unsigned int> seg;  // (outlives the asynchronous upload)
  DevBuf<unsigned int> dSeg;
  DevBuf<unsigned char> dTmp;
};

// checks the flow-guided and the bilateral filter share (rasterOk / inputsOk: the operator's own conditions)
static void checkFilterBatch(int n, int first, int count, bool rasterOk, int frameRadius, int spatialRadius, bool inputsOk) {
  if (n < 1 || first < 0 || count < 0 || first + count > n) throw std::runtime_error("invalid frame batch");
  if (!rasterOk) throw std::runtime_error("invalid raster");
  if (frameRadius < 0 || spatialRadius < 0) throw std::runtime_error("negative filter radius");
  if (!inputsOk) throw std::runtime_error("null filter input");
}

// ---- constraint sampling (cvd_sampling.h) -----------------------------------------------------------
// triplet == false: keyFrames = 2 x n frames (a, b) of the directed pairs, flow / mask = a -> b.
// triplet == true : keyFrames = n centre frames c, flow / mask = c -> c-1, flow2 / mask2 = c -> c+1.
void sampleConstraints(cvd_handle* h, bool triplet, int num, const int32_t* keyFrames, const float* corner,
                              const float* flow, const uint8_t* mask, const float* flow2, const uint8_t* mask2,
                              const float* dyn, int dw, int dh, int matchSeparation, float minDynamicDistance,
                              int64_t* offsets) {
  if (h->F <= 0) throw std::runtime_error("no video set");
  if (matchSeparation < 0) throw std::runtime_error("matchSeparation must be >= 0");
  const int W = h->W, H = h->H;
  const size_t npx = static_cast<size_t>(W) * H;
  const int width = triplet ? 3 : 2;  // float2 per constraint
  if ((npx + 31) / 32 * 4 > kMaxLds) throw std::runtime_error("image too large for the LDS-resident sampling mask");
  for (int i = 0; i < (triplet ? 1 : 2) * num; ++i) {
    const int f = keyFrames[i];
    if (f < 0 || f >= h->F || (triplet && (f < 1 || f + 1 >= h->F))) throw std::runtime_error("sampling frame out of range");
  }
  hipStream_t s = h->stream;
  DevBuf<float> dCorner, dDyn;
  DevBuf<float2> dFlow, dFlow2, dSlab;
  DevBuf<unsigned char> dMaskS, dMaskS2;
  DevBuf<int> dKeysF;
  DevBuf<unsigned long long> dKeys, dKeysOut;
  DevBuf<unsigned int> dNValid, dCount;
  DevBuf<long long> dOff;
  dCorner.upload(corner, static_cast<size_t>(h->F) * npx, s);
  if (dyn) dDyn.upload(dyn, static_cast<size_t>(h->F) * dw * dh, s);
  dKeysF.upload(keyFrames, static_cast<size_t>(num) * (triplet ? 1 : 2), s);
  dFlow.upload(reinterpret_cast<const float2*>(flow), static_cast<size_t>(num) * npx, s);
  dMaskS.upload(mask, static_cast<size_t>(num) * npx, s);
  if (triplet) {
    dFlow2.upload(reinterpret_cast<const float2*>(flow2), static_cast<size_t>(num) * npx, s);
    dMaskS2.upload(mask2, static_cast<size_t>(num) * npx, s);
  }
  SamplingArgs A{W, H, h->invAspect, matchSeparation, minDynamicDistance, dCorner.p, dyn ? dDyn.p : nullptr,
                 dyn ? dw : W, dyn ? dh : H};
  // batches: keys (2 x 8 B) and the output slab (8 B x width) per pixel, ~1 GiB at a time
  const int PB = static_cast<int>(std::max<size_t>(1, std::min<size_t>(num, (size_t(1) << 30) / (npx * (16 + 8 * width)))));
  if (static_cast<size_t>(PB) * npx > 0xFFFFFFFFull) throw std::runtime_error("sampling batch too large");
  dKeys.ensure(static_cast<size_t>(PB) * npx);
  dKeysOut.ensure(static_cast<size_t>(PB) * npx);
  dSlab.ensure(static_cast<size_t>(PB) * npx * width);
  dNValid.ensure(PB);
  dCount.ensure(PB);
  SegmentedKeySort sorter(PB, npx, dKeys.p, dKeysOut.p, s);
  Frontend& fe = *h->frontend;
  DevBuf<float2>& result = triplet ? fe.dSampledTrip : fe.dSampledLoc;
  std::vector<long long> off(num + 1, 0);
  std::vector<unsigned int> cnt(PB);
  result.ensure(1);
  for (int p0 = 0; p0 < num; p0 += PB) {
    const int nb = std::min(PB, num - p0);
    HIP_CHECK(hipMemsetAsync(dNValid.p, 0, sizeof(unsigned int) * nb, s));
    const dim3 gridC(static_cast<unsigned>((npx + 255) / 256), nb);
    if (triplet)
      hipLaunchKernelGGL(k_fc_triplet_candidates, gridC, dim3(256), 0, s, A, p0, dKeysF.p, dFlow.p, dMaskS.p, dFlow2.p,
                         dMaskS2.p, dKeys.p, dNValid.p);
    else
      hipLaunchKernelGGL(k_fc_candidates, gridC, dim3(256), 0, s, A, p0, dKeysF.p, dFlow.p, dMaskS.p, dKeys.p, dNValid.p);
    HIP_CHECK(hipGetLastError());
    sorter.run(nb);
    const size_t ldsBytes = (npx + 31) / 32 * 4;
    if (triplet) {
      allowLds(k_fc_greedy<true>, ldsBytes);
      hipLaunchKernelGGL(k_fc_greedy<true>, dim3(nb), dim3(64), ldsBytes, s, A, p0, dKeysOut.p, dNValid.p, dFlow.p,
                         dFlow2.p, dSlab.p, dCount.p);
    } else {
      allowLds(k_fc_greedy<false>, ldsBytes);
      hipLaunchKernelGGL(k_fc_greedy<false>, dim3(nb), dim3(64), ldsBytes, s, A, p0, dKeysOut.p, dNValid.p, dFlow.p,
                         static_cast<const float2*>(nullptr), dSlab.p, dCount.p);
    }
    HIP_CHECK(hipGetLastError());
    dCount.download(cnt.data(), nb, s);
    HIP_CHECK(hipStreamSynchronize(s));
    for (int i = 0; i < nb; ++i) off[p0 + i + 1] = off[p0 + i] + cnt[i];
    // grow the result buffer and compact this batch into it
    const size_t total = static_cast<size_t>(off[p0 + nb]) * width;
    if (total > result.n) result.grow(std::max<size_t>(total, result.n * 2), static_cast<size_t>(off[p0]) * width, s);
    dOff.upload(off.data(), off.size(), s);
    hipLaunchKernelGGL(k_fc_compact, dim3(16, nb), dim3(256), 0, s, static_cast<int>(npx), width, p0, dOff.p, dSlab.p,
                       result.p);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipStreamSynchronize(s));
  }
  (triplet ? fe.sampledTripOff : fe.sampledOff) = off;
  for (int i = 0; i <= num; ++i) offsets[i] = off[i];
}

// the constraints of the last sampleConstraints of that kind: 2 (pairs) resp. 3 (triplets) float2 each
void getSampledConstraints(cvd_handle* h, bool triplet, float* out) {
  const Frontend& fe = *h->frontend;
  const std::vector<long long>& off = triplet ? fe.sampledTripOff : fe.sampledOff;
  const size_t n = off.empty() ? 0 : static_cast<size_t>(off.back());
  if (n) {
    HIP_CHECK(hipMemcpyAsync(out, (triplet ? fe.dSampledTrip : fe.dSampledLoc).p, n * (triplet ? 3 : 2) * sizeof(float2),
                             hipMemcpyDeviceToHost, h->stream));
    HIP_CHECK(hipStreamSynchronize(h->stream));
  }
}

// ---- dense consumers of the result (cvd_dense.h) ----------------------------------------------
// kind 0: DepthXform::apply -> f32 [n][H][W]; 1: GridDepthXform::paramMap -> f64 [n][H][W][N];
// 2: SpatialXform::warp -> f32 [n][h][w][2] for the raster (w, h).  Host buffer out; the device buffer is kept for
// the next call.  Returns the kernel time in ms through *kernelMs when asked (HIP events on the solver stream).
void denseMaps(cvd_handle* h, int kind, int first, int count, int w, int hh, void* out, double* kernelMs) {
  if (h->F <= 0) throw std::runtime_error("no video set");
  if (first < 0 || count < 0 || first + count > h->F) throw std::runtime_error("frame range out of bounds");
  if (!h->poseParamsValid) posesToParams(h);
  cvd_opt_params p;
  cvd_opt_params_default(&p);
  Layout L = makeLayout(h, p, 0.0, PK_POSE_STEP);
  int KD, KS;
  tapCounts(L, KD, KS);
  if (kind == 1 && L.depthType != CVD_DEPTH_GRID)
    throw std::runtime_error("Parameter map not implemented for this transform type.");  // reference :422-425
  if (kind != 2) { w = h->W; hh = h->H; }
  if (w < 2 || hh < 2) throw std::runtime_error("raster too small");
  uploadState(h, L, h->dX);
  hipStream_t s = h->stream;
  Frontend& fe = *h->frontend;
  const size_t pixels = static_cast<size_t>(count) * hh * w;
  const size_t bytes = pixels * (kind == 0 ? sizeof(float) : kind == 1 ? sizeof(double) * std::max(L.N, 1) : sizeof(float2));
  fe.dDense.ensure((bytes + 7) / 8);
  if (count == 0) return;
  KernelTimer timer(s, kernelMs, 1);
  timer.mark();
  const dim3 grid((w * hh + 255) / 256, 1, count), block(256);
  if (kind == 0) {
    CVD_DISPATCH_KD(KD, {
      hipLaunchKernelGGL((k_apply_depth<KD>), grid, block, 0, s, L, w, hh, first, h->dDepth.p, h->dX.p,
                         reinterpret_cast<float*>(fe.dDense.p));
    });
  } else if (kind == 1) {
    CVD_DISPATCH_KD(KD, {
      hipLaunchKernelGGL((k_param_map<KD>), grid, block, 0, s, L, w, hh, first, h->dDepth.p, h->dX.p, fe.dDense.p);
    });
  } else {
    if (KS == 0) hipLaunchKernelGGL((k_warp_map<0>), grid, block, 0, s, L, w, hh, first, h->dX.p, reinterpret_cast<float2*>(fe.dDense.p));
    else if (KS == 4) hipLaunchKernelGGL((k_warp_map<4>), grid, block, 0, s, L, w, hh, first, h->dX.p, reinterpret_cast<float2*>(fe.dDense.p));
    else hipLaunchKernelGGL((k_warp_map<16>), grid, block, 0, s, L, w, hh, first, h->dX.p, reinterpret_cast<float2*>(fe.dDense.p));
  }
  HIP_CHECK(hipGetLastError());
  timer.mark();
  if (out) HIP_CHECK(hipMemcpyAsync(out, fe.dDense.p, bytes, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
  timer.collect();
}

// cornerMinEigenVal of n BGR float images (kind 0) / chamfer distance transform of n 8-bit masks (kind 1)
void imageOps(cvd_handle* h, int kind, int n, int w, int hh, const void* in, float* out, double* kernelMs) {
  if (n < 0 || w < 1 || hh < 1) throw std::runtime_error("invalid image batch");
  if (n == 0) return;
  if (!in) throw std::runtime_error("null image input");
  hipStream_t s = h->stream;
  const size_t px = static_cast<size_t>(w) * hh, pixels = px * n;
  if (pixels > (1ull << 31)) throw std::runtime_error("image batch too large for one call");
  Frontend& fe = *h->frontend;
  fe.dImgOut.ensure(pixels);
  KernelTimer timer(s, kernelMs, 1);
  if (kind == 0) {
    fe.dImgIn.ensure(pixels * 3);
    fe.dImgGray.ensure(pixels);
    fe.dImgCov.ensure(pixels * 3);
    HIP_CHECK(hipMemcpyAsync(fe.dImgIn.p, in, pixels * 3 * sizeof(float), hipMemcpyHostToDevice, s));
    timer.mark();
    hipLaunchKernelGGL(k_bgr_to_gray, dim3(static_cast<unsigned>((pixels + 255) / 256)), dim3(256), 0, s, fe.dImgIn.p, pixels,
                       fe.dImgGray.p);
    const dim3 grid(static_cast<unsigned>((px + 255) / 256), 1, n);
    hipLaunchKernelGGL(k_sobel_cov, grid, dim3(256), 0, s, fe.dImgGray.p, w, hh, fe.dImgCov.p);
    hipLaunchKernelGGL(k_box_min_eigenval, grid, dim3(256), 0, s, fe.dImgCov.p, w, hh, fe.dImgOut.p);
  } else {
    const size_t tmpPer = static_cast<size_t>(w + 4) * (hh + 4);
    fe.dImgMask.ensure(pixels);
    fe.dImgTmp.ensure(tmpPer * n);
    HIP_CHECK(hipMemcpyAsync(fe.dImgMask.p, in, pixels, hipMemcpyHostToDevice, s));
    timer.mark();
    const size_t lds = kChamferThreads * sizeof(long long) + static_cast<size_t>(w) * sizeof(unsigned int);
    if (lds > 64 * 1024) throw std::runtime_error("mask too wide for the distance transform kernel");
    hipLaunchKernelGGL(k_chamfer_5x5, dim3(n), dim3(kChamferThreads), lds, s, fe.dImgMask.p, w, hh, fe.dImgTmp.p,
                       fe.dImgOut.p);
  }
  HIP_CHECK(hipGetLastError());
  timer.mark();
  if (out) HIP_CHECK(hipMemcpyAsync(out, fe.dImgOut.p, pixels * sizeof(float), hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
  timer.collect();
}

// Quaternion (x, y, z, w) times vector, the way Eigen evaluates it in float (uv = 2 q.vec x v; v + w uv + q.vec x uv)
static void quatRotate(const float* q, const float* v, float* out) {
  float uv[3] = {q[1] * v[2] - q[2] * v[1], q[2] * v[0] - q[0] * v[2], q[0] * v[1] - q[1] * v[0]};
  for (int i = 0; i < 3; ++i) uv[i] += uv[i];
  const float c[3] = {q[1] * uv[2] - q[2] * uv[1], q[2] * uv[0] - q[0] * uv[2], q[0] * uv[1] - q[1] * uv[0]};
  for (int i = 0; i < 3; ++i) out[i] = v[i] + q[3] * uv[i] + c[i];
}

void flowGuidedFilter(cvd_handle* h, int n, int first, int count, int w, int hh, int dw, int dh, float invAspect,
                             const float* depth, const float* cameras, const float* flowF, const uint8_t* maskF,
                             const float* flowB, const uint8_t* maskB, int frameRadius, int spatialRadius, int median,
                             float* out, double* kernelMs) {
  checkFilterBatch(n, first, count, w >= 1 && hh >= 1 && dw >= 1 && dh >= 1 && invAspect > 0.f, frameRadius, spatialRadius,
                   depth && cameras && !(n > 1 && frameRadius > 0 && (!flowF || !maskF || !flowB || !maskB)));
  if (count == 0) return;
  const long long side = 2ll * spatialRadius + 1, maxSamples = side * side * (2ll * frameRadius + 1);
  if (median && maxSamples > 256)
    throw std::runtime_error("flow guided median filter: (2 spatialRadius + 1)^2 (2 frameRadius + 1) > 256 samples per pixel");
  hipStream_t s = h->stream;
  Frontend& fe = *h->frontend;
  const size_t px = static_cast<size_t>(w) * hh, dpx = static_cast<size_t>(dw) * dh;
  std::vector<FilterCam> cams(n);
  for (int k = 0; k < n; ++k) {
    const float* c = cameras + static_cast<size_t>(k) * 9;
    const float ex[3] = {1.f, 0.f, 0.f}, ey[3] = {0.f, 1.f, 0.f}, ez[3] = {0.f, 0.f, -1.f};
    for (int i = 0; i < 3; ++i) cams[k].pos[i] = c[i];
    quatRotate(c + 3, ex, cams[k].right);
    quatRotate(c + 3, ey, cams[k].up);
    quatRotate(c + 3, ez, cams[k].front);
    cams[k].tanH = std::tan(c[7] / 2.f);
    cams[k].tanV = std::tan(c[8] / 2.f);
  }
  fe.dFltCams.upload(cams.data(), n, s);
  fe.dFltDepth.upload(depth, dpx * n, s);
  const size_t links = n > 1 && frameRadius > 0 ? static_cast<size_t>(n - 1) : 0;
  fe.dFltFlowF.upload(flowF, links * px * 2, s);
  fe.dFltFlowB.upload(flowB, links * px * 2, s);
  fe.dFltMaskF.upload(maskF, links * px, s);
  fe.dFltMaskB.upload(maskB, links * px, s);
  fe.dFltOut.ensure(px * count);
  FilterArgs A;
  A.n = n; A.first = first; A.count = count; A.w = w; A.h = hh; A.dw = dw; A.dh = dh; A.invAspect = invAspect;
  A.frameRadius = links ? frameRadius : 0; A.spatialRadius = spatialRadius; A.median = median;
  A.depth = fe.dFltDepth.p; A.cams = fe.dFltCams.p;
  A.flowFwd = reinterpret_cast<const float2*>(fe.dFltFlowF.p); A.maskFwd = fe.dFltMaskF.p;
  A.flowBwd = reinterpret_cast<const float2*>(fe.dFltFlowB.p); A.maskBwd = fe.dFltMaskB.p;
  A.out = fe.dFltOut.p;
  KernelTimer timer(s, kernelMs, 1);
  timer.mark();
  const dim3 grid(static_cast<unsigned>((px + 255) / 256), 1, count), block(256);
  if (!median) hipLaunchKernelGGL((k_flow_guided_filter<0>), grid, block, 0, s, A);
  else if (maxSamples <= 16) hipLaunchKernelGGL((k_flow_guided_filter<16>), grid, block, 0, s, A);
  else if (maxSamples <= 64) hipLaunchKernelGGL((k_flow_guided_filter<64>), grid, block, 0, s, A);
  else hipLaunchKernelGGL((k_flow_guided_filter<256>), grid, block, 0, s, A);
  HIP_CHECK(hipGetLastError());
  timer.mark();
  if (out) HIP_CHECK(hipMemcpyAsync(out, fe.dFltOut.p, px * count * sizeof(float), hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
  timer.collect();
}

// DepthVideoProcessor::bilateralFilter (reference lib/Processor.cpp:183-313) on a batch of consecutive frames, cvd_bilateral.h
void bilateralFilter(cvd_handle* h, int n, int first, int count, int w, int hh, const float* depth, const float* color,
                     int frameRadius, int spatialRadius, float depthSigma, float colorSigma, int median, float* out,
                     double* kernelMs) {
  const bool useColor = colorSigma > 0.f;
  checkFilterBatch(n, first, count, w >= 1 && hh >= 1, frameRadius, spatialRadius, depth && !(useColor && !color));
  const size_t px = static_cast<size_t>(w) * hh;
  if (px * n > (1ull << 31)) throw std::runtime_error("bilateral filter batch too large for one call");
  // [kf - R, kf + R] clipped to [0, n) is the same window with R = min(R, n - 1): the sample counts below are exact
  const int R = std::min(frameRadius, n - 1);
  const long long side = 2ll * spatialRadius + 1, samples = side * side * (2ll * R + 1);
  if (median && samples > kBilateralMaxSamples)
    throw std::runtime_error(fmt("bilateral median filter: %lld samples per pixel ((2 spatialRadius + 1)^2 (2 frameRadius + 1)) "
                                 "exceed the supported %d", samples, kBilateralMaxSamples));
  if (count == 0) return;
  hipStream_t s = h->stream;
  Frontend& fe = *h->frontend;
  fe.dBilDepth.upload(depth, px * n, s);
  if (useColor) fe.dBilColor.upload(color, px * n * 3, s);
  fe.dBilOut.ensure(px * count);
  BilateralArgs A;
  A.n = n; A.w = w; A.h = hh; A.frameRadius = R; A.spatialRadius = spatialRadius;
  A.useDepth = depthSigma > 0.f; A.useColor = useColor;
  A.depthSigma2 = depthSigma * depthSigma; A.colorSigma2 = colorSigma * colorSigma;
  A.depth = fe.dBilDepth.p; A.color = useColor ? fe.dBilColor.p : nullptr;
  const long long tileTexels = (kBilateralTileW + 2ll * spatialRadius) * (kBilateralTileH + 2ll * spatialRadius);
  const size_t stageBytes = static_cast<size_t>(tileTexels) * (useColor ? 16 : 4);
  const bool stage = spatialRadius > 0 && stageBytes <= kBilateralMaxLds;
  int P2 = 128;
  while (P2 < samples) P2 *= 2;
  KernelTimer timer(s, kernelMs, 1);
  timer.mark();
  const dim3 tiles((w + kBilateralTileW - 1) / kBilateralTileW, (hh + kBilateralTileH - 1) / kBilateralTileH), block(256);
  for (int c0 = 0; c0 < count; c0 += 65535) {  // (grid z limit)
    const int nz = std::min(count - c0, 65535);
    A.first = first + c0;
    A.out = fe.dBilOut.p + px * c0;
    const dim3 grid(tiles.x, tiles.y, nz);
    if (!median) {
      if (stage && useColor) {
        allowLds(k_bilateral_mean<true, true>, stageBytes);
        hipLaunchKernelGGL((k_bilateral_mean<true, true>), grid, block, stageBytes, s, A);
      } else if (stage) {
        allowLds(k_bilateral_mean<false, true>, stageBytes);
        hipLaunchKernelGGL((k_bilateral_mean<false, true>), grid, block, stageBytes, s, A);
      }
      else if (useColor) hipLaunchKernelGGL((k_bilateral_mean<true, false>), grid, block, 0, s, A);
      else hipLaunchKernelGGL((k_bilateral_mean<false, false>), grid, block, 0, s, A);
    } else if (samples <= 16) {
      if (useColor) hipLaunchKernelGGL((k_bilateral_median_small<16, true>), grid, block, 0, s, A);
      else hipLaunchKernelGGL((k_bilateral_median_small<16, false>), grid, block, 0, s, A);
    } else if (samples <= 64) {
      if (useColor) hipLaunchKernelGGL((k_bilateral_median_small<64, true>), grid, block, 0, s, A);
      else hipLaunchKernelGGL((k_bilateral_median_small<64, false>), grid, block, 0, s, A);
    } else {
      const dim3 gridW(static_cast<unsigned>((px + 3) / 4), 1, nz);
      const size_t lds = static_cast<size_t>(P2) * 2 * sizeof(float) * 4;  // <= 64 KB: P2 <= kBilateralMaxSamples
      if (useColor) {
        allowLds(k_bilateral_median_wave<true>, lds);
        hipLaunchKernelGGL((k_bilateral_median_wave<true>), gridW, block, lds, s, A, P2);
      } else {
        allowLds(k_bilateral_median_wave<false>, lds);
        hipLaunchKernelGGL((k_bilateral_median_wave<false>), gridW, block, lds, s, A, P2);
      }
    }
    HIP_CHECK(hipGetLastError());
  }
  timer.mark();
  if (out) HIP_CHECK(hipMemcpyAsync(out, fe.dBilOut.p, px * count * sizeof(float), hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
  timer.collect();
}

// FlowConstraintsCollection::setStaticFlagFromRansac (no reference implementation; tests/epipolar_reference.py defines it):
// cvd_epipolar.h's four kernels per batch of pairs.  The batch bounds the per-hypothesis buffers ([pairs][K][9] f64 + counts)
// to ~512 MiB; the sampler key carries the global pair index, so batching does not change the result.  kernelMs (may be
// NULL): {normalise, hypotheses, score, select} HIP-event times summed over the batches.  counts / hypotheses (test hook,
// may be NULL): every hypothesis's inlier count [P][K] and F_pix [P][K][9].
void epipolarStaticFlags(cvd_handle* h, int numPairs, const int64_t* offsets, const float* loc, double pixelScale,
                         double thresholdPx, int iterations, uint64_t seed, uint8_t* isStatic, double* fundamental,
                         int32_t* best, double* kernelMs, int32_t* counts, double* hypotheses) {
  if (!(std::isfinite(thresholdPx) && thresholdPx > 0.0))
    throw std::runtime_error(fmt("epipolar RANSAC: threshold_px must be finite and > 0 (got %g)", thresholdPx));
  if (iterations < 1 || iterations > kEpiMaxIterations)
    throw std::runtime_error(fmt("epipolar RANSAC: iterations must lie in [1, %d] (got %d)", kEpiMaxIterations, iterations));
  if (numPairs < 0 || numPairs >= kEpiMaxPairs)
    throw std::runtime_error(fmt("epipolar RANSAC: num_pairs must lie in [0, 2^20) (got %d)", numPairs));
  if (!(std::isfinite(pixelScale) && pixelScale > 0.0))
    throw std::runtime_error(fmt("epipolar RANSAC: pixel_scale must be finite and > 0 (got %g)", pixelScale));
  if (numPairs > 0 && !offsets) throw std::runtime_error("epipolar RANSAC: null offsets");
  if (kernelMs) std::fill(kernelMs, kernelMs + 4, 0.0);
  if (numPairs == 0) return;
  if (offsets[0] != 0) throw std::runtime_error("epipolar RANSAC: offsets[0] must be 0");
  for (int p = 0; p < numPairs; ++p)
    if (offsets[p + 1] < offsets[p]) throw std::runtime_error(fmt("epipolar RANSAC: offsets decrease at pair %d", p));
  const long long C = offsets[numPairs];
  if (C > 0 && (!loc || !isStatic)) throw std::runtime_error("epipolar RANSAC: null constraint locations or flags");
  for (long long i = 0; i < 4 * C; ++i)
    if (!std::isfinite(loc[i]))
      throw std::runtime_error(fmt("epipolar RANSAC: non-finite constraint location (loc of constraint %lld)", i / 4));
  const int K = iterations;
  const size_t perPair = static_cast<size_t>(K) * (9 * sizeof(double) + sizeof(int));
  const int batch = static_cast<int>(std::max<size_t>(1, std::min<size_t>(numPairs, (512ull << 20) / perPair)));
  hipStream_t s = h->stream;
  Frontend& fe = *h->frontend;
  fe.dEpiLoc.upload(reinterpret_cast<const float4*>(loc), static_cast<size_t>(C), s);
  fe.dEpiOff.upload(reinterpret_cast<const long long*>(offsets), static_cast<size_t>(numPairs) + 1, s);
  fe.dEpiNorm.ensure(batch);
  fe.dEpiF.ensure(static_cast<size_t>(batch) * K * 9);
  fe.dEpiCount.ensure(static_cast<size_t>(batch) * K);
  fe.dEpiFlags.ensure(static_cast<size_t>(C));
  fe.dEpiFbest.ensure(static_cast<size_t>(numPairs) * 9);
  fe.dEpiBest.ensure(static_cast<size_t>(numPairs) * 2);
  KernelTimer timer(s, kernelMs, 4);
  EpiArgs A;
  A.K = K;
  A.seed = seed;
  A.w = pixelScale;
  A.thresh2 = thresholdPx * thresholdPx;
  A.loc = fe.dEpiLoc.p;
  A.norm = fe.dEpiNorm.p;
  A.F = fe.dEpiF.p;
  A.count = fe.dEpiCount.p;
  A.flags = fe.dEpiFlags.p;
  for (int p0 = 0; p0 < numPairs; p0 += batch) {
    const int np = std::min(batch, numPairs - p0);
    A.numPairs = np;
    A.pairBase = p0;
    A.off = fe.dEpiOff.p + p0;
    A.Fbest = fe.dEpiFbest.p + static_cast<size_t>(p0) * 9;
    A.best = fe.dEpiBest.p + static_cast<size_t>(p0) * 2;
    timer.mark();
    hipLaunchKernelGGL(k_epi_normalise, dim3(np), dim3(kEpiThreads), 0, s, A);
    HIP_CHECK(hipGetLastError());
    timer.mark();
    hipLaunchKernelGGL(k_epi_hypotheses, dim3(np, (K + kEpiHypThreads - 1) / kEpiHypThreads), dim3(kEpiHypThreads), 0, s, A);
    HIP_CHECK(hipGetLastError());
    timer.mark();
    hipLaunchKernelGGL(k_epi_score, dim3(np, (K + kEpiThreads - 1) / kEpiThreads), dim3(kEpiThreads), 0, s, A);
    HIP_CHECK(hipGetLastError());
    timer.mark();
    hipLaunchKernelGGL(k_epi_select, dim3(np), dim3(kEpiThreads), 0, s, A);
    HIP_CHECK(hipGetLastError());
    timer.mark();
    if (counts) fe.dEpiCount.download(counts + static_cast<size_t>(p0) * K, static_cast<size_t>(np) * K, s);
    if (hypotheses) fe.dEpiF.download(hypotheses + static_cast<size_t>(p0) * K * 9, static_cast<size_t>(np) * K * 9, s);
    if (kernelMs || counts || hypotheses) HIP_CHECK(hipStreamSynchronize(s));  // (the next batch reuses the buffers)
    timer.collect();
  }
  fe.dEpiFlags.download(isStatic, static_cast<size_t>(C), s);
  if (fundamental) fe.dEpiFbest.download(fundamental, static_cast<size_t>(numPairs) * 9, s);
  if (best) fe.dEpiBest.download(best, static_cast<size_t>(numPairs) * 2, s);
  HIP_CHECK(hipStreamSynchronize(s));
}

// DepthVideoProcessor::computeTracks (reference lib/Processor.cpp:646-886), cvd_tracks.h.  Batches of frames bound the
// candidate keys (2 x 8 B per pixel) to ~1 GiB; each batch is candidates -> segmented sort -> walk.  The walk stops before a
// frame whose worst case does not fit the observation / track buffers; they are doubled and the walk resumes there.
// kernelMs (may be NULL): {candidates, sort, walk, table} HIP-event times summed over the batches.
void computeTracks(cvd_handle* h, int F, int H, int W, float invAspect, const uint8_t* active, int first, int last,
                   const float* corner, const float* dyn, int dh, int dw, const float* flow, const uint8_t* mask,
                   const uint8_t* pairPresent, int spawnDistance, int pruneDistance, float minDynamicDistance,
                   int minTrackLength, int64_t* counts, double* kernelMs) {
  if (F < 1) throw std::runtime_error(fmt("compute tracks: num_frames must be >= 1 (got %d)", F));
  if (W < 1 || H < 1) throw std::runtime_error(fmt("compute tracks: invalid image size %d x %d", W, H));
  if (!(std::isfinite(invAspect) && invAspect > 0.f))
    throw std::runtime_error(fmt("compute tracks: inv_aspect must be finite and > 0 (got %g)", static_cast<double>(invAspect)));
  if (first < 0 || last >= F || first > last)
    throw std::runtime_error(fmt("compute tracks: frame range [%d, %d] outside [0, %d)", first, last, F));
  constexpr int kMaxRadius = 1 << 14;
  if (spawnDistance < 0 || spawnDistance > kMaxRadius)
    throw std::runtime_error(fmt("compute tracks: trackSpawnDistance must lie in [0, %d] (got %d)", kMaxRadius, spawnDistance));
  if (pruneDistance < 0 || pruneDistance > kMaxRadius)
    throw std::runtime_error(fmt("compute tracks: trackPruneDistance must lie in [0, %d] (got %d)", kMaxRadius, pruneDistance));
  if (!std::isfinite(minDynamicDistance))
    throw std::runtime_error("compute tracks: minDynamicDistance must be finite");
  if (!active || !corner || !counts) throw std::runtime_error("compute tracks: null frame flags, corner input or counts");
  if (dyn && (dw < 1 || dh < 1)) throw std::runtime_error(fmt("compute tracks: invalid dynamic distance size %d x %d", dw, dh));
  bool anyFlow = false, anyMask = false;
  for (int p = 0; p + 1 < F && pairPresent; ++p) {
    anyFlow |= (pairPresent[p] & 1) != 0;
    anyMask |= (pairPresent[p] & 2) != 0;
  }
  if (F > 1 && !pairPresent) throw std::runtime_error("compute tracks: null pair flags");
  if ((anyFlow && !flow) || (anyMask && !mask)) throw std::runtime_error("compute tracks: a present pair has a null flow or mask");
  const size_t npx = static_cast<size_t>(W) * H;
  if (npx * F >= (size_t(1) << 31)) throw std::runtime_error(fmt("compute tracks: %d frames of %d x %d exceed 2^31 pixels per call", F, W, H));
  const size_t maskBytes = 2 * ((npx + 31) / 32) * sizeof(unsigned int);
  if (maskBytes + sizeof(TrackShared) > kMaxLds)
    throw std::runtime_error(fmt("compute tracks: image too large: the prune and spawn bitmasks of a %d x %d image need %zu B of "
                                 "LDS (> %zu)", W, H, maskBytes, kMaxLds - sizeof(TrackShared)));
  hipStream_t s = h->stream;
  DevBuf<unsigned char> dActive, dPair, dMask;
  DevBuf<float> dCorner, dDyn;
  DevBuf<float2> dFlow;
  DevBuf<unsigned long long> dKeys, dKeysOut;
  DevBuf<unsigned int> dNValid;
  DevBuf<int> dFrameStart, dFrameCount, dObsTrack;
  DevBuf<float2> dObsLoc;
  DevBuf<TrackState> dState;
  std::vector<unsigned char> pairs(std::max(F - 1, 1), 0);
  if (pairPresent) std::copy(pairPresent, pairPresent + (F - 1), pairs.begin());
  dActive.upload(active, F, s);
  dPair.upload(pairs.data(), pairs.size(), s);
  dCorner.upload(corner, static_cast<size_t>(F) * npx, s);
  if (dyn) dDyn.upload(dyn, static_cast<size_t>(F) * dw * dh, s);
  if (anyFlow) dFlow.upload(reinterpret_cast<const float2*>(flow), static_cast<size_t>(F - 1) * npx, s);
  if (anyMask) dMask.upload(mask, static_cast<size_t>(F - 1) * npx, s);
  dFlow.ensure(1);
  dMask.ensure(1);
  TrackArgs A{F, W, H, invAspect, first, last, spawnDistance, pruneDistance, minDynamicDistance, dActive.p, dPair.p,
              dCorner.p, dyn ? dDyn.p : nullptr, dyn ? dw : W, dyn ? dh : H, dFlow.p, dMask.p};
  const int PB = static_cast<int>(std::max<size_t>(1, std::min<size_t>(F, (size_t(1) << 30) / (npx * 16))));
  dKeys.ensure(static_cast<size_t>(PB) * npx);
  dKeysOut.ensure(static_cast<size_t>(PB) * npx);
  dNValid.ensure(PB);
  SegmentedKeySort sorter(PB, npx, dKeys.p, dKeysOut.p, s);
  Frontend& fe = *h->frontend;
  // observation / track buffers: the walk's worst case per frame is (continued + spawned) <= W H each; typical videos keep
  // a few hundred tracks per frame, so these start small and grow on demand
  dFrameStart.ensure(F);
  dFrameCount.ensure(F);
  int obsCap = static_cast<int>(std::min<size_t>(npx * 4, (size_t(1) << 31) - 1));
  int trackCap = static_cast<int>(std::min<size_t>(npx * 2, (size_t(1) << 31) - 1));
  dObsTrack.ensure(obsCap);
  dObsLoc.ensure(obsCap);
  fe.dTrkStart.ensure(trackCap);
  TrackState st{0, 0, 0, 0};
  dState.upload(&st, 1, s);
  const size_t walkLds = maskBytes;
  allowLds(k_track_walk, walkLds + sizeof(TrackShared));
  // (always timed: the host waits for the sort through the timer's event; kernelMs is written on success only)
  double ms[4];
  KernelTimer timer(s, ms, 4);
  try {
    for (int f0 = 0; f0 < F; f0 += PB) {
      const int nb = std::min(PB, F - f0);
      timer.mark();
      HIP_CHECK(hipMemsetAsync(dNValid.p, 0, sizeof(unsigned int) * nb, s));
      hipLaunchKernelGGL(k_track_candidates, dim3(static_cast<unsigned>((npx + 255) / 256), nb), dim3(256), 0, s, A, f0,
                         dKeys.p, dNValid.p);
      HIP_CHECK(hipGetLastError());
      timer.mark();
      sorter.run(nb);
      timer.mark();
      timer.wait();
      timer.collect();
      for (int fw = f0; fw < f0 + nb;) {
        TrackBufs B{dFrameStart.p, dFrameCount.p, dObsTrack.p, dObsLoc.p, fe.dTrkStart.p, obsCap, trackCap};
        timer.seek(2);
        timer.mark();
        hipLaunchKernelGGL(k_track_walk, dim3(1), dim3(kTrackThreads), walkLds, s, A, fw, f0 + nb,
                           dKeysOut.p + static_cast<size_t>(fw - f0) * npx, dNValid.p + (fw - f0), B, dState.p);
        HIP_CHECK(hipGetLastError());
        timer.mark();
        dState.download(&st, 1, s);
        HIP_CHECK(hipStreamSynchronize(s));
        timer.collect();
        if (st.stopFrame < fw) throw std::runtime_error("compute tracks: the walk made no progress");
        fw = st.stopFrame;
        if (fw < f0 + nb) {  // grow the buffers (keeping their contents) and resume at that frame
          const size_t maxCap = (size_t(1) << 31) - 1;
          const size_t no = std::min(maxCap, std::max<size_t>(2 * static_cast<size_t>(obsCap), st.obsUsed + 2 * npx));
          const size_t nt = std::min(maxCap, std::max<size_t>(2 * static_cast<size_t>(trackCap), st.numTracks + npx));
          if (no == static_cast<size_t>(obsCap) && nt == static_cast<size_t>(trackCap))
            throw std::runtime_error("compute tracks: observation buffer limit reached");
          dObsTrack.grow(no, st.obsUsed, s);
          dObsLoc.grow(no, st.obsUsed, s);
          fe.dTrkStart.grow(nt, st.numTracks, s);
          obsCap = static_cast<int>(no);
          trackCap = static_cast<int>(nt);
        }
      }
    }
    // the table: lengths, minTrackLength pruning, per-track location lists
    const int T = st.numTracks, O = st.obsUsed;
    fe.dTrkLen.ensure(T);
    fe.dTrkKeptLen.ensure(static_cast<size_t>(T) + 1);
    fe.dTrkOff.ensure(static_cast<size_t>(T) + 1);
    fe.dTrkKept.ensure(T);
    timer.seek(3);
    timer.mark();
    long long keptObs = 0;
    if (T > 0) {
      HIP_CHECK(hipMemsetAsync(fe.dTrkLen.p, 0, sizeof(int) * T, s));
      HIP_CHECK(hipMemsetAsync(fe.dTrkKeptLen.p + T, 0, sizeof(int), s));  // (the scan's last item: offset[T] = the total)
      hipLaunchKernelGGL(k_track_lengths, dim3((O + 255) / 256), dim3(256), 0, s, O, dObsTrack.p, fe.dTrkLen.p);
      hipLaunchKernelGGL(k_track_keep, dim3((T + 255) / 256), dim3(256), 0, s, T, minTrackLength, fe.dTrkLen.p,
                         fe.dTrkKeptLen.p, fe.dTrkKept.p);
      HIP_CHECK(hipGetLastError());
      size_t scanBytes = 0;
      HIP_CHECK(rocprim::exclusive_scan(nullptr, scanBytes, fe.dTrkKeptLen.p, fe.dTrkOff.p, 0, static_cast<size_t>(T) + 1,
                                        rocprim::plus<int>(), s));
      DevBuf<unsigned char> scanTmp;
      scanTmp.ensure(scanBytes);
      HIP_CHECK(rocprim::exclusive_scan(scanTmp.p, scanBytes, fe.dTrkKeptLen.p, fe.dTrkOff.p, 0, static_cast<size_t>(T) + 1,
                                        rocprim::plus<int>(), s));
      int total = 0;
      HIP_CHECK(hipMemcpyAsync(&total, fe.dTrkOff.p + T, sizeof(int), hipMemcpyDeviceToHost, s));
      HIP_CHECK(hipStreamSynchronize(s));
      keptObs = total;
      fe.dTrkLoc.ensure(static_cast<size_t>(std::max(total, 1)));
      hipLaunchKernelGGL(k_track_scatter, dim3(16, F), dim3(256), 0, s, dFrameStart.p, dFrameCount.p, dObsTrack.p, dObsLoc.p,
                         fe.dTrkStart.p, fe.dTrkKept.p, fe.dTrkOff.p, fe.dTrkLoc.p);
      HIP_CHECK(hipGetLastError());
    }
    timer.mark();
    HIP_CHECK(hipStreamSynchronize(s));
    timer.collect();
    fe.trkTracks = T;
    fe.trkKeptObs = keptObs;
    long long kept = 0;
    if (T > 0) {
      std::vector<unsigned char> k(T);
      fe.dTrkKept.download(k.data(), T, s);
      HIP_CHECK(hipStreamSynchronize(s));
      for (unsigned char v : k) kept += v;
    }
    counts[0] = T;
    counts[1] = kept;
    counts[2] = keptObs;
  } catch (...) {
    fe.trkTracks = fe.trkKeptObs = 0;
    throw;
  }
  if (kernelMs) std::copy(ms, ms + 4, kernelMs);
}

void getTracks(cvd_handle* h, int32_t* startFrame, int32_t* length, uint8_t* kept, float* loc) {
  hipStream_t s = h->stream;
  const Frontend& fe = *h->frontend;
  const size_t T = static_cast<size_t>(fe.trkTracks);
  if (T > 0) {
    if (startFrame) fe.dTrkStart.download(startFrame, T, s);
    if (length) fe.dTrkLen.download(length, T, s);
    if (kept) fe.dTrkKept.download(kept, T, s);
  }
  if (loc && fe.trkKeptObs > 0) fe.dTrkLoc.download(reinterpret_cast<float2*>(loc), static_cast<size_t>(fe.trkKeptObs), s);
  HIP_CHECK(hipStreamSynchronize(s));
}

// Flow.compute_flow_masks on a batch of pairs (reference flow.py:180-209, utils/consistency.py:8-67), cvd_flowmask.h: one launch
// for both directions of every pair.  pixelsPerThread: 0 = the product choice, 1 / 4 = that map (test and measurement hook).
template <int C>
static void launchFlowMasks(const FlowMaskArgs& A, int numPairs, int pix, hipStream_t s) {
  const size_t npx = static_cast<size_t>(A.w) * A.h;
  const size_t perBlock = static_cast<size_t>(kFlowMaskThreads) * pix;
  const dim3 grid(static_cast<unsigned>((npx + perBlock - 1) / perBlock), numPairs, 2), block(kFlowMaskThreads);
  if (pix == 4) hipLaunchKernelGGL((k_flow_masks<C, 4>), grid, block, 0, s, A);
  else hipLaunchKernelGGL((k_flow_masks<C, 1>), grid, block, 0, s, A);
}

void flowConsistencyMasks(cvd_handle* h, int numFrames, int hh, int w, int channels, const float* color, int numPairs,
                          const int32_t* pairFrames, const float* flowAB, const float* flowBA, float flowThresh,
                          float colorThresh, uint8_t* maskAB, uint8_t* maskBA, int32_t* kept, float* errors, double* kernelMs,
                          int pixelsPerThread) {
  if (numFrames < 1) throw std::runtime_error(fmt("flow masks: num_frames must be >= 1 (got %d)", numFrames));
  if (hh < 1 || w < 1) throw std::runtime_error(fmt("flow masks: invalid image size: height %d, width %d", hh, w));
  if (channels < 1 || channels > 4) throw std::runtime_error(fmt("flow masks: channels must lie in [1, 4] (got %d)", channels));
  if (numPairs < 0 || numPairs > 65535)
    throw std::runtime_error(fmt("flow masks: num_pairs must lie in [0, 65535] (got %d)", numPairs));
  if (!(std::isfinite(flowThresh) && flowThresh >= 0.f))
    throw std::runtime_error(fmt("flow masks: flow_thresh must be finite and >= 0 (got %g)", static_cast<double>(flowThresh)));
  if (!(std::isfinite(colorThresh) && colorThresh >= 0.f))
    throw std::runtime_error(fmt("flow masks: color_thresh must be finite and >= 0 (got %g)", static_cast<double>(colorThresh)));
  if (pixelsPerThread != 0 && pixelsPerThread != 1 && pixelsPerThread != 4)
    throw std::runtime_error(fmt("flow masks: pixels_per_thread must be 0, 1 or 4 (got %d)", pixelsPerThread));
  if (pixelsPerThread == 4 && w % 4 != 0)
    throw std::runtime_error(fmt("flow masks: four pixels per thread need a width that is a multiple of 4 (got %d)", w));
  const size_t npx = static_cast<size_t>(w) * hh;
  if (npx > (size_t(1) << 28)) throw std::runtime_error(fmt("flow masks: image size %d x %d exceeds 2^28 pixels", w, hh));
  if (kernelMs) *kernelMs = 0.0;
  if (numPairs == 0) return;
  if (!color) throw std::runtime_error("flow masks: null color");
  if (!pairFrames) throw std::runtime_error("flow masks: null pair_frames");
  if (!flowAB) throw std::runtime_error("flow masks: null flow_ab");
  if (!flowBA) throw std::runtime_error("flow masks: null flow_ba");
  if (!maskAB) throw std::runtime_error("flow masks: null mask_ab");
  if (!maskBA) throw std::runtime_error("flow masks: null mask_ba");
  for (int p = 0; p < numPairs; ++p) {
    const int a = pairFrames[2 * p], b = pairFrames[2 * p + 1];
    if (a < 0 || a >= numFrames || b < 0 || b >= numFrames)
      throw std::runtime_error(fmt("flow masks: pair_frames[%d] = (%d, %d) outside [0, %d)", p, a, b, numFrames));
    if (a == b) throw std::runtime_error(fmt("flow masks: pair_frames[%d] = (%d, %d) names one frame twice", p, a, b));
  }
  hipStream_t s = h->stream;
  const size_t P = static_cast<size_t>(numPairs);
  Frontend& fe = *h->frontend;
  fe.dFmColor.upload(color, static_cast<size_t>(numFrames) * npx * channels, s);
  fe.dFmPairs.upload(reinterpret_cast<const int2*>(pairFrames), P, s);
  fe.dFmFlowAB.upload(reinterpret_cast<const float2*>(flowAB), P * npx, s);
  fe.dFmFlowBA.upload(reinterpret_cast<const float2*>(flowBA), P * npx, s);
  fe.dFmMaskAB.ensure(P * npx);
  fe.dFmMaskBA.ensure(P * npx);
  fe.dFmKept.ensure(P * 2);
  if (errors) fe.dFmErr.ensure(P * 2 * npx);
  HIP_CHECK(hipMemsetAsync(fe.dFmKept.p, 0, sizeof(int) * P * 2, s));
  FlowMaskArgs A;
  A.w = w;
  A.h = hh;
  // thresholds of utils/consistency.py:53-63, computed in double and rounded once (numpy compares the f32 errors in f32)
  A.flowT = static_cast<float>(static_cast<double>(flowThresh) * static_cast<double>(flowThresh));
  A.colorT = static_cast<float>(channels * (static_cast<double>(colorThresh) * static_cast<double>(colorThresh)));
  A.color = fe.dFmColor.p;
  A.pairs = fe.dFmPairs.p;
  A.flowAB = fe.dFmFlowAB.p;
  A.flowBA = fe.dFmFlowBA.p;
  A.maskAB = fe.dFmMaskAB.p;
  A.maskBA = fe.dFmMaskBA.p;
  A.kept = fe.dFmKept.p;
  A.errors = errors ? fe.dFmErr.p : nullptr;
  const int pix = pixelsPerThread ? pixelsPerThread : (w % 4 == 0 ? 4 : 1);
  KernelTimer timer(s, kernelMs, 1);
  timer.mark();
  switch (channels) {
    case 1: launchFlowMasks<1>(A, numPairs, pix, s); break;
    case 2: launchFlowMasks<2>(A, numPairs, pix, s); break;
    case 3: launchFlowMasks<3>(A, numPairs, pix, s); break;
    default: launchFlowMasks<4>(A, numPairs, pix, s); break;
  }
  HIP_CHECK(hipGetLastError());
  timer.mark();
  fe.dFmMaskAB.download(maskAB, P * npx, s);
  fe.dFmMaskBA.download(maskBA, P * npx, s);
  if (kept) fe.dFmKept.download(kept, P * 2, s);
  if (errors) fe.dFmErr.download(reinterpret_cast<float2*>(errors), P * 2 * npx, s);
  HIP_CHECK(hipStreamSynchronize(s));
  timer.collect();
}

// ---- what the fine-tuning losses share on the host (cvd_loss_common.h on the device) -----------------------------------------
namespace {
template <typename Desc> constexpr bool kPairLoss = !std::is_same<Desc, cvd_spatial_desc>::value;

// Checks of the desc fields the three losses share; `op` is the operator's message prefix.  lambdas: every weight, finite and
// >= 0.  A loss of flow pairs (kPairLoss) also has num_pairs and the robust distances `distances` with their scale and alpha.
template <typename Desc>
void checkLossDesc(const char* op, const Desc* d, int minFrames, std::initializer_list<std::pair<const char*, double Desc::*>> lambdas,
                   std::initializer_list<std::pair<const char*, int32_t Desc::*>> distances) {
  if (!d) throw std::runtime_error(fmt("%s: null desc", op));
  if (d->struct_size != CVD_STRUCT_STAMP(Desc))
    throw std::runtime_error(fmt("%s: desc.struct_size %llu is not this library's %llu (built against another revision of cvd_hip.h)",
                                 op, static_cast<unsigned long long>(d->struct_size),
                                 static_cast<unsigned long long>(CVD_STRUCT_STAMP(Desc))));
  if (d->precision != CVD_PRECISION_F32 && d->precision != CVD_PRECISION_F64)
    throw std::runtime_error(fmt("%s: precision must be 0 (f32) or 1 (f64) (got %d)", op, d->precision));
  if (d->width < 2 || d->height < 2)
    throw std::runtime_error(fmt("%s: width and height must be >= 2 (got %d x %d)", op, d->width, d->height));
  if (static_cast<size_t>(d->width) * d->height > (size_t(1) << 28))
    throw std::runtime_error(fmt("%s: image size %d x %d exceeds 2^28 pixels", op, d->width, d->height));
  if (d->num_frames < minFrames) throw std::runtime_error(fmt("%s: num_frames must be >= %d (got %d)", op, minFrames, d->num_frames));
  if constexpr (kPairLoss<Desc>) {
    if (d->num_pairs < 1 || d->num_pairs > 65535)
      throw std::runtime_error(fmt("%s: num_pairs must lie in [1, 65535] (got %d)", op, d->num_pairs));
  }
  for (const auto& l : lambdas)
    if (!(std::isfinite(d->*l.second) && d->*l.second >= 0.0))
      throw std::runtime_error(fmt("%s: %s must be finite and >= 0 (got %g)", op, l.first, d->*l.second));
  if constexpr (kPairLoss<Desc>) {
    for (const auto& t : distances)
      if (d->*t.second < CVD_DISTANCE_L1 || d->*t.second > CVD_DISTANCE_GENERAL)
        throw std::runtime_error(fmt("%s: %s must lie in [0, 4] (got %d)", op, t.first, d->*t.second));
    if (!(std::isfinite(d->distance_scale) && d->distance_scale > 0.0))
      throw std::runtime_error(fmt("%s: distance_scale must be finite and > 0 (got %g)", op, d->distance_scale));
    if (!std::isfinite(d->distance_alpha)) throw std::runtime_error(fmt("%s: distance_alpha must be finite (got %g)", op, d->distance_alpha));
  }
}

// host-side check of a pair table [P][2] against F frames
void checkPairFrames(const char* op, const int32_t* pairFrames, int P, int F) {
  for (int p = 0; p < P; ++p) {
    const int a = pairFrames[2 * p], b = pairFrames[2 * p + 1];
    if (a < 0 || a >= F || b < 0 || b >= F)
      throw std::runtime_error(fmt("%s: pair_frames[%d] = (%d, %d) outside [0, %d)", op, p, a, b, F));
    if (a == b) throw std::runtime_error(fmt("%s: pair_frames[%d] = (%d, %d) names one frame twice", op, p, a, b));
  }
}

// Pixels per thread of a loss walk: four when the rows are whole 4-pixel groups and every per-pixel table is aligned for the
// vector accesses (a null table is not read and counts as aligned), else one.
template <size_t N>
int lossPixelsPerThread(int width, size_t elemSize, const void* const (&tables)[N]) {
  bool four = width % 4 == 0;
  for (const void* p : tables) four = four && reinterpret_cast<uintptr_t>(p) % (4 * elemSize) == 0;
  return four ? 4 : 1;
}

// workgroups of kConsThreads threads that cover an image of npx pixels
int lossWorkgroups(size_t npx, int pix) {
  return static_cast<int>((npx + static_cast<size_t>(kConsThreads) * pix - 1) / (static_cast<size_t>(kConsThreads) * pix));
}

// f(T{}) with T the precision's type
template <typename Fn>
void withPrecision(int precision, Fn&& f) {
  if (precision == CVD_PRECISION_F64) f(double{});
  else f(float{});
}

// Arrays of a loss's host-array entry point.  in: the real inputs in the loss's own order with their sizes in bytes (null: not
// read); frames: the int32 frame tables with their element counts (null: none); out: the double results with their counts.
struct LossHostArrays {
  int numIn;
  const void* in[kLossMaxArrays];
  size_t inBytes[kLossMaxArrays];
  const int32_t* frames[2];
  size_t frameCount[2];
  double* out[3];
  size_t outCount[3];
  void* grad;
  size_t gradBytes;
  void* maps;
  size_t mapBytes;
};
// their staged copies on the device, null where the host array is null
struct LossDeviceArrays {
  const void* in[kLossMaxArrays];
  const int32_t* frames[2];
  double* out[3];
  void* grad;
  void* maps;
};

// The host-array entry point of a loss: uploads the inputs into the handle's staging buffers, runs launch(device arrays, stream,
// timer) on the handle's stream, copies the results back, waits, and collects the timer's `phases` phases into kernelMs (may be
// null).
template <typename Launch>
void runLossOnHostArrays(cvd_handle* h, const LossHostArrays& a, double* kernelMs, int phases, Launch&& launch) {
  hipStream_t s = h->stream;
  Frontend& fe = *h->frontend;
  LossDeviceArrays dv{};
  for (int k = 0; k < a.numIn; ++k) {
    if (!a.in[k]) continue;
    fe.dLossIn[k].upload(static_cast<const unsigned char*>(a.in[k]), a.inBytes[k], s);
    dv.in[k] = fe.dLossIn[k].p;
  }
  for (int k = 0; k < 2; ++k) {
    if (!a.frames[k]) continue;
    fe.dLossFrames[k].upload(a.frames[k], a.frameCount[k], s);
    dv.frames[k] = fe.dLossFrames[k].p;
  }
  fe.dLossOut.ensure(a.outCount[0] + a.outCount[1] + a.outCount[2]);
  dv.out[0] = fe.dLossOut.p;
  dv.out[1] = dv.out[0] + a.outCount[0];
  dv.out[2] = dv.out[1] + a.outCount[1];
  if (a.grad) fe.dLossGrad.ensure(a.gradBytes);
  if (a.maps) fe.dLossMaps.ensure(a.mapBytes);
  dv.grad = a.grad ? fe.dLossGrad.p : nullptr;
  dv.maps = a.maps ? fe.dLossMaps.p : nullptr;
  KernelTimer timer(s, kernelMs, phases);
  launch(dv, s, timer);
  for (int k = 0; k < 3; ++k)
    if (a.outCount[k]) HIP_CHECK(hipMemcpyAsync(a.out[k], dv.out[k], sizeof(double) * a.outCount[k], hipMemcpyDeviceToHost, s));
  if (a.grad) fe.dLossGrad.download(static_cast<unsigned char*>(a.grad), a.gradBytes, s);
  if (a.maps) fe.dLossMaps.download(static_cast<unsigned char*>(a.maps), a.mapBytes, s);
  HIP_CHECK(hipStreamSynchronize(s));
  timer.collect();
}
}  // namespace

// ---- consistency loss of flow pairs and its depth gradient (reference loss/consistency_loss.py, cvd_consistency.h) ----------
namespace {
constexpr int kConsArrays = 8;  // depth, extrinsics, intrinsics, warp, flow a->b, flow b->a, weight a->b, weight b->a
struct ConsistencyArrays {
  const void *depth, *ext, *intr, *warp, *flowAB, *flowBA, *weightAB, *weightBA;
  const int32_t* pairs;
};

void checkConsistency(const cvd_consistency_desc* d, const ConsistencyArrays& in, const double* total, const double* terms) {
  using D = cvd_consistency_desc;
  checkLossDesc("consistency loss", d, 2, {{"lambda_reprojection", &D::lambda_reprojection}, {"lambda_disparity", &D::lambda_disparity},
                                           {"lambda_depth_ratio", &D::lambda_depth_ratio}}, {{"distance_type", &D::distance_type}});
  const void* arr[] = {in.depth, in.ext, in.intr, in.pairs, in.flowAB, in.flowBA, in.weightAB, in.weightBA, total, terms};
  const char* arrName[] = {"depth", "extrinsics", "intrinsics", "pair_frames", "flow_ab", "flow_ba", "weight_ab", "weight_ba",
                           "total", "terms"};
  for (int k = 0; k < 10; ++k)
    if (!arr[k]) throw std::runtime_error(fmt("consistency loss: null %s", arrName[k]));
  if (d->have_warp && !in.warp) throw std::runtime_error("consistency loss: null warp (desc.have_warp is set)");
}

// One distance of the fine-tuning losses for the kernels.  l2 / smooth_l1 / cauchy are the general loss at alpha = 2 / 1 / 0
// (reference loss/distance.py); the branch is chosen from alpha in the kernel's precision, as the reference's torch.where does.
template <typename T>
ConsDistance<T> robustDistance(int type, double scale, double alpha) {
  ConsDistance<T> r;
  r.scale = static_cast<T>(scale);
  r.alpha = static_cast<T>(type == CVD_DISTANCE_L2 ? 2.0 : type == CVD_DISTANCE_SMOOTH_L1 ? 1.0 : type == CVD_DISTANCE_CAUCHY ? 0.0 : alpha);
  r.kind = type == CVD_DISTANCE_L1 ? CONS_RHO_L1 : r.alpha == T(2) ? CONS_RHO_TWO : r.alpha == T(0) ? CONS_RHO_ZERO : CONS_RHO_GENERAL;
  const T eps = static_cast<T>(std::numeric_limits<float>::epsilon());
  r.beta = std::max(eps, std::abs(r.alpha - T(2)));
  r.alphaSafe = (r.alpha >= T(0) ? T(1) : T(-1)) * std::max(eps, std::abs(r.alpha));
  return r;
}

template <typename T>
void launchConsistency(cvd_handle* h, const cvd_consistency_desc& d, const ConsistencyArrays& in, double* total, double* terms,
                       void* grad, hipStream_t s, KernelTimer& timer) {
  const int P = d.num_pairs, F = d.num_frames;
  const size_t npx = static_cast<size_t>(d.width) * d.height;
  Frontend& fe = *h->frontend;
  timer.mark();
  if (d.lambda_reprojection == 0.0 && d.lambda_disparity == 0.0 && d.lambda_depth_ratio == 0.0) {  // no term exists
    HIP_CHECK(hipMemsetAsync(total, 0, sizeof(double), s));
    HIP_CHECK(hipMemsetAsync(terms, 0, sizeof(double) * 3 * P, s));
    timer.mark();
    if (grad) HIP_CHECK(hipMemsetAsync(grad, 0, sizeof(T) * F * npx, s));
    timer.mark();
    return;
  }
  const void* const vec[] = {in.depth, in.warp, in.flowAB, in.flowBA, in.weightAB, in.weightBA};
  const int pix = lossPixelsPerThread(d.width, sizeof(T), vec), nb = lossWorkgroups(npx, pix);
  fe.dConsSlab.ensure(static_cast<size_t>(P) * 2 * nb * 4);
  fe.dConsSums.ensure(static_cast<size_t>(P) * 8);
  fe.dConsCoef.ensure(static_cast<size_t>(P) * 6);
  ConsArgs<T> A{};
  A.F = F; A.P = P; A.W = d.width; A.H = d.height;
  A.useRep = d.lambda_reprojection > 0.0; A.useDsp = d.lambda_disparity > 0.0; A.useRat = d.lambda_depth_ratio > 0.0;
  A.nb = nb;
  A.lamRat = static_cast<T>(d.lambda_depth_ratio);
  A.rho = robustDistance<T>(d.distance_type, d.distance_scale, d.distance_alpha);
  A.depth = static_cast<const T*>(in.depth);
  A.ext = static_cast<const T*>(in.ext);
  A.intr = static_cast<const T*>(in.intr);
  A.warp = d.have_warp ? static_cast<const T*>(in.warp) : nullptr;
  A.pairs = reinterpret_cast<const int2*>(in.pairs);
  A.flow[0] = static_cast<const T*>(in.flowAB);
  A.flow[1] = static_cast<const T*>(in.flowBA);
  A.weight[0] = static_cast<const T*>(in.weightAB);
  A.weight[1] = static_cast<const T*>(in.weightBA);
  A.slab = fe.dConsSlab.p;
  A.coef = fe.dConsCoef.p;
  A.grad = static_cast<T*>(grad);
  ConsFinishArgs FA{F, P, nb, d.lambda_reprojection, d.lambda_disparity, d.lambda_depth_ratio, A.pairs, fe.dConsSlab.p,
                    fe.dConsSums.p, fe.dConsCoef.p, terms, total};
  const dim3 grid(nb, P, 2), block(kConsThreads);
  if (pix == 4) hipLaunchKernelGGL((k_cons_forward<T, 4>), grid, block, 0, s, A);
  else hipLaunchKernelGGL((k_cons_forward<T, 1>), grid, block, 0, s, A);
  hipLaunchKernelGGL(k_cons_finish_pairs, dim3(P), dim3(64), 0, s, FA);
  hipLaunchKernelGGL((k_cons_finish_total<T>), dim3(1), block, 0, s, FA, A.intr);
  HIP_CHECK(hipGetLastError());
  timer.mark();
  if (grad) {
    HIP_CHECK(hipMemsetAsync(grad, 0, sizeof(T) * F * npx, s));
#if CVD_DETERMINISTIC
    hipLaunchKernelGGL((k_cons_backward_det<T>), dim3(F), dim3(kConsDetThreads), 0, s, A);
#else
    if (pix == 4) hipLaunchKernelGGL((k_cons_backward<T, 4>), grid, block, 0, s, A);
    else hipLaunchKernelGGL((k_cons_backward<T, 1>), grid, block, 0, s, A);
#endif
    HIP_CHECK(hipGetLastError());
  }
  timer.mark();
}
}  // namespace

// Device arrays in, device results out, on the caller's stream: no copy and no host wait.  The pair table lives on the device and
// cannot be checked here; the kernels never dereference a pair that names a frame out of range (or one frame twice) and return NaN.
void consistencyLossDevice(cvd_handle* h, const cvd_consistency_desc* d, const void* depth, const void* ext, const void* intr,
                           const void* warp, const int32_t* pairFrames, const void* flowAB, const void* flowBA,
                           const void* weightAB, const void* weightBA, double* total, double* terms, void* grad, hipStream_t s) {
  const ConsistencyArrays in{depth, ext, intr, warp, flowAB, flowBA, weightAB, weightBA, pairFrames};
  checkConsistency(d, in, total, terms);
  KernelTimer timer(s, nullptr, 2);
  withPrecision(d->precision, [&](auto t) { launchConsistency<decltype(t)>(h, *d, in, total, terms, grad, s, timer); });
}

// Host arrays in, host results out.  kernelMs (may be NULL): {forward + finish, backward} HIP-event times.
void consistencyLoss(cvd_handle* h, const cvd_consistency_desc* d, const void* depth, const void* ext, const void* intr,
                     const void* warp, const int32_t* pairFrames, const void* flowAB, const void* flowBA, const void* weightAB,
                     const void* weightBA, double* total, double* terms, void* grad, double* kernelMs) {
  checkConsistency(d, ConsistencyArrays{depth, ext, intr, warp, flowAB, flowBA, weightAB, weightBA, pairFrames}, total, terms);
  const size_t P = d->num_pairs, F = d->num_frames;
  checkPairFrames("consistency loss", pairFrames, d->num_pairs, d->num_frames);
  const size_t es = d->precision == CVD_PRECISION_F64 ? 8 : 4, npx = static_cast<size_t>(d->width) * d->height;
  const LossHostArrays host{kConsArrays,
                            {depth, ext, intr, d->have_warp ? warp : nullptr, flowAB, flowBA, weightAB, weightBA},
                            {F * npx * es, F * 12 * es, F * 4 * es, F * 2 * npx * es, P * 2 * npx * es, P * 2 * npx * es, P * npx * es, P * npx * es},
                            {pairFrames, nullptr}, {2 * P, 0}, {total, terms, nullptr}, {1, 3 * P, 0}, grad, F * npx * es, nullptr, 0};
  runLossOnHostArrays(h, host, kernelMs, 2, [&](const LossDeviceArrays& dv, hipStream_t s, KernelTimer& timer) {
    const ConsistencyArrays in{dv.in[0], dv.in[1], dv.in[2], dv.in[3], dv.in[4], dv.in[5], dv.in[6], dv.in[7], dv.frames[0]};
    withPrecision(d->precision, [&](auto t) { launchConsistency<decltype(t)>(h, *d, in, dv.out[0], dv.out[1], dv.grad, s, timer); });
  });
}

// ---- scene-flow loss of flow pairs and its depth gradient (reference loss/scene_flow_loss.py, cvd_sceneflow.h) --------------
namespace {
constexpr int kSfArrays = kLossMaxArrays;
// real[]: depth, extrinsics, intrinsics, warp, flows[2], masks[2], neighbor_flows[4], neighbor_masks[4], valid
struct SceneFlowArrays {
  const void* real[kSfArrays];
  const int32_t *pairs, *nbrs;
};
const char* const kSfNames[kSfArrays] = {"depth", "extrinsics", "intrinsics", "warp", "flows[0]", "flows[1]", "masks[0]", "masks[1]",
                                         "neighbor_flows[0]", "neighbor_flows[1]", "neighbor_flows[2]", "neighbor_flows[3]",
                                         "neighbor_masks[0]", "neighbor_masks[1]", "neighbor_masks[2]", "neighbor_masks[3]", "valid"};

bool sfHasStatic(const cvd_scene_flow_desc& d) { return d.lambda_static > 0.0; }
bool sfHasSmooth(const cvd_scene_flow_desc& d) {
  return d.lambda_smooth_reprojection > 0.0 || d.lambda_smooth_disparity > 0.0 || d.lambda_smooth_depth_ratio > 0.0;
}

// checks the desc and gathers the arrays; an array group the enabled terms do not read may be NULL (and is then never read)
SceneFlowArrays checkSceneFlow(const cvd_scene_flow_desc* d, const void* depth, const void* ext, const void* intr, const void* warp,
                               const int32_t* pairs, const void* const* flows, const void* const* masks, const int32_t* nbrs,
                               const void* const* nflows, const void* const* nmasks, const void* valid, const double* total,
                               const double* terms) {
  using D = cvd_scene_flow_desc;
  checkLossDesc("scene flow loss", d, 2,
                {{"lambda_static", &D::lambda_static}, {"lambda_smooth_reprojection", &D::lambda_smooth_reprojection},
                 {"lambda_smooth_disparity", &D::lambda_smooth_disparity}, {"lambda_smooth_depth_ratio", &D::lambda_smooth_depth_ratio}},
                {{"distance_type_static", &D::distance_type_static}, {"distance_type_smooth", &D::distance_type_smooth}});
  const bool st = sfHasStatic(*d), sm = sfHasSmooth(*d);
  if (st && !flows) throw std::runtime_error("scene flow loss: null flows (lambda_static > 0)");
  if (st && !masks) throw std::runtime_error("scene flow loss: null masks (lambda_static > 0)");
  if (sm && !nbrs) throw std::runtime_error("scene flow loss: null neighbor_frames (a smooth lambda > 0)");
  if (sm && !nflows) throw std::runtime_error("scene flow loss: null neighbor_flows (a smooth lambda > 0)");
  if (sm && !nmasks) throw std::runtime_error("scene flow loss: null neighbor_masks (a smooth lambda > 0)");
  SceneFlowArrays in{};
  in.real[0] = depth; in.real[1] = ext; in.real[2] = intr;
  in.real[3] = d->have_warp ? warp : nullptr;
  for (int k = 0; k < 2 && st; ++k) {
    in.real[4 + k] = flows[k];
    in.real[6 + k] = masks[k];
  }
  for (int k = 0; k < 4 && sm; ++k) {
    in.real[8 + k] = nflows[k];
    in.real[12 + k] = nmasks[k];
  }
  in.real[16] = sm ? valid : nullptr;
  in.pairs = pairs;
  in.nbrs = sm ? nbrs : nullptr;
  for (int k = 0; k < kSfArrays; ++k) {
    const bool needed = k < 3 || (k == 3 && d->have_warp) || (k >= 4 && k < 8 && st) || (k >= 8 && sm);
    if (needed && !in.real[k])
      throw std::runtime_error(fmt("scene flow loss: null %s%s", kSfNames[k], k == 3 ? " (desc.have_warp is set)" : ""));
  }
  if (!pairs) throw std::runtime_error("scene flow loss: null pair_frames");
  if (!total) throw std::runtime_error("scene flow loss: null total");
  if (!terms) throw std::runtime_error("scene flow loss: null terms");
  return in;
}

template <typename T>
void launchSceneFlow(cvd_handle* h, const cvd_scene_flow_desc& d, const SceneFlowArrays& in, double* total, double* terms, void* grad,
                     void* maps, hipStream_t s, KernelTimer& timer) {
  const int P = d.num_pairs, F = d.num_frames;
  const size_t npx = static_cast<size_t>(d.width) * d.height;
  Frontend& fe = *h->frontend;
  timer.mark();
  if (!sfHasStatic(d) && !sfHasSmooth(d)) {  // no term exists
    HIP_CHECK(hipMemsetAsync(total, 0, sizeof(double), s));
    HIP_CHECK(hipMemsetAsync(terms, 0, sizeof(double) * 4 * P, s));
    if (maps) HIP_CHECK(hipMemsetAsync(maps, 0, sizeof(T) * 6 * P * 3 * npx, s));
    timer.mark();
    if (grad) HIP_CHECK(hipMemsetAsync(grad, 0, sizeof(T) * F * npx, s));
    timer.mark();
    return;
  }
  const void* vec[14] = {in.real[0]};   // every per-pixel table: depth, then warp .. neighbor_masks[3]
  std::copy(in.real + 3, in.real + 16, vec + 1);
  const int pix = lossPixelsPerThread(d.width, sizeof(T), vec), nb = lossWorkgroups(npx, pix);
  fe.dSfSlab.ensure(static_cast<size_t>(P) * 4 * nb * 4);
  fe.dSfSums.ensure(static_cast<size_t>(P) * 16);
  fe.dSfCoef.ensure(static_cast<size_t>(P) * 12);
  SfArgs<T> A{};
  A.F = F; A.P = P; A.W = d.width; A.H = d.height;
  A.useStatic = sfHasStatic(d);
  A.useRep = d.lambda_smooth_reprojection > 0.0; A.useDsp = d.lambda_smooth_disparity > 0.0; A.useRat = d.lambda_smooth_depth_ratio > 0.0;
  A.nb = nb;
  A.lamRat = static_cast<T>(d.lambda_smooth_depth_ratio);
  A.rhoS = robustDistance<T>(d.distance_type_static, d.distance_scale, d.distance_alpha);
  A.rhoM = robustDistance<T>(d.distance_type_smooth, d.distance_scale, d.distance_alpha);
  A.depth = static_cast<const T*>(in.real[0]);
  A.ext = static_cast<const T*>(in.real[1]);
  A.intr = static_cast<const T*>(in.real[2]);
  A.warp = static_cast<const T*>(in.real[3]);
  A.pairs = reinterpret_cast<const int2*>(in.pairs);
  A.nbrs = in.nbrs;
  for (int k = 0; k < 2; ++k) {
    A.flow[k] = static_cast<const T*>(in.real[4 + k]);
    A.mask[k] = static_cast<const T*>(in.real[6 + k]);
  }
  for (int k = 0; k < 4; ++k) {
    A.nflow[k] = static_cast<const T*>(in.real[8 + k]);
    A.nmask[k] = static_cast<const T*>(in.real[12 + k]);
  }
  A.valid = static_cast<const T*>(in.real[16]);
  A.slab = fe.dSfSlab.p;
  A.coef = fe.dSfCoef.p;
  A.grad = static_cast<T*>(grad);
  A.maps = static_cast<T*>(maps);
  SfFinishArgs FA{F, P, nb, d.lambda_static, d.lambda_smooth_reprojection, d.lambda_smooth_disparity, d.lambda_smooth_depth_ratio,
                  A.pairs, A.nbrs, fe.dSfSlab.p, fe.dSfSums.p, fe.dSfCoef.p, terms, total};
  const dim3 grid(nb, P, 4), block(kConsThreads);
  if (pix == 4) hipLaunchKernelGGL((k_sf_forward<T, 4>), grid, block, 0, s, A);
  else hipLaunchKernelGGL((k_sf_forward<T, 1>), grid, block, 0, s, A);
  hipLaunchKernelGGL(k_sf_finish_pairs, dim3(P), dim3(64), 0, s, FA);
  hipLaunchKernelGGL((k_sf_finish_total<T>), dim3(1), block, 0, s, FA, A.intr);
  HIP_CHECK(hipGetLastError());
  timer.mark();
  if (grad) {
    HIP_CHECK(hipMemsetAsync(grad, 0, sizeof(T) * F * npx, s));
#if CVD_DETERMINISTIC
    hipLaunchKernelGGL((k_sf_backward_det<T>), dim3(F), dim3(kConsDetThreads), 0, s, A);
#else
    if (pix == 4) hipLaunchKernelGGL((k_sf_backward<T, 4>), grid, block, 0, s, A);
    else hipLaunchKernelGGL((k_sf_backward<T, 1>), grid, block, 0, s, A);
#endif
    HIP_CHECK(hipGetLastError());
  }
  timer.mark();
}
}  // namespace

// Device arrays in, device results out, on the caller's stream: no copy and no host wait.  flows / masks / nflows / nmasks are
// HOST arrays of 2 / 2 / 4 / 4 device pointers.  The frame tables live on the device and cannot be checked here; the kernels never
// dereference a pair or neighbour that names a frame out of range (or a pair of one frame twice) and return NaN.
void sceneFlowLossDevice(cvd_handle* h, const cvd_scene_flow_desc* d, const void* depth, const void* ext, const void* intr,
                         const void* warp, const int32_t* pairFrames, const void* const* flows, const void* const* masks,
                         const int32_t* neighborFrames, const void* const* nflows, const void* const* nmasks, const void* valid,
                         double* total, double* terms, void* grad, void* maps, hipStream_t s) {
  const SceneFlowArrays in = checkSceneFlow(d, depth, ext, intr, warp, pairFrames, flows, masks, neighborFrames, nflows, nmasks,
                                            valid, total, terms);
  KernelTimer timer(s, nullptr, 2);
  withPrecision(d->precision, [&](auto t) { launchSceneFlow<decltype(t)>(h, *d, in, total, terms, grad, maps, s, timer); });
}

// Host arrays in, host results out.  kernelMs (may be NULL): {forward + finish, backward} HIP-event times.
void sceneFlowLoss(cvd_handle* h, const cvd_scene_flow_desc* d, const void* depth, const void* ext, const void* intr,
                   const void* warp, const int32_t* pairFrames, const void* const* flows, const void* const* masks,
                   const int32_t* neighborFrames, const void* const* nflows, const void* const* nmasks, const void* valid,
                   double* total, double* terms, void* grad, void* maps, double* kernelMs) {
  const SceneFlowArrays host = checkSceneFlow(d, depth, ext, intr, warp, pairFrames, flows, masks, neighborFrames, nflows, nmasks,
                                              valid, total, terms);
  const size_t P = d->num_pairs, F = d->num_frames;
  checkPairFrames("scene flow loss", pairFrames, d->num_pairs, d->num_frames);
  for (size_t k = 0; k < 4 * P && host.nbrs; ++k)
    if (host.nbrs[k] < 0 || host.nbrs[k] >= d->num_frames)
      throw std::runtime_error(fmt("scene flow loss: neighbor_frames[%d][%d] = %d outside [0, %d)", static_cast<int>(k / 4),
                                   static_cast<int>(k % 4), host.nbrs[k], d->num_frames));
  const size_t es = d->precision == CVD_PRECISION_F64 ? 8 : 4, npx = static_cast<size_t>(d->width) * d->height;
  LossHostArrays a{kSfArrays, {}, {}, {pairFrames, host.nbrs}, {2 * P, 4 * P}, {total, terms, nullptr}, {1, 4 * P, 0},
                   grad, F * npx * es, maps, 6 * P * 3 * npx * es};
  for (int k = 0; k < kSfArrays; ++k) {
    a.in[k] = host.real[k];
    a.inBytes[k] = es * (k == 0 ? F * npx : k == 1 ? F * 12 : k == 2 ? F * 4 : k == 3 ? F * 2 * npx
                         : k == 16 ? P * 2 : (k < 6 || (k >= 8 && k < 12)) ? P * 2 * npx : P * npx);
  }
  runLossOnHostArrays(h, a, kernelMs, 2, [&](const LossDeviceArrays& dv, hipStream_t s, KernelTimer& timer) {
    SceneFlowArrays in{};
    std::copy(dv.in, dv.in + kSfArrays, in.real);
    in.pairs = dv.frames[0];
    in.nbrs = dv.frames[1];
    withPrecision(d->precision, [&](auto t) {
      launchSceneFlow<decltype(t)>(h, *d, in, dv.out[0], dv.out[1], dv.grad, dv.maps, s, timer);
    });
  });
}

// ---- spatial smoothness and contrast losses and their depth gradient (reference loss/disparity_smooth_loss.py,
// loss/contrast_loss.py; cvd_spatial.h) ----------------------------------------------------------------------------------------
namespace {
bool spHasSmooth(const cvd_spatial_desc& d) { return d.lambda_disparity_smooth > 0.0; }
bool spHasContrast(const cvd_spatial_desc& d) { return d.lambda_contrast_loss > 0.0; }

// checks the desc and the pointers; a table the enabled terms do not read may be NULL (and is then never read)
void checkSpatial(const cvd_spatial_desc* d, const void* depth, const void* depthOrig, const void* image, const double* total,
                  const double* smooth, const double* contrast) {
  using D = cvd_spatial_desc;
  checkLossDesc("spatial losses", d, 1, {{"lambda_disparity_smooth", &D::lambda_disparity_smooth},
                                         {"lambda_contrast_loss", &D::lambda_contrast_loss}}, {});
  if (d->frames_per_sample < 1)
    throw std::runtime_error(fmt("spatial losses: frames_per_sample must be >= 1 (got %d)", d->frames_per_sample));
  if (d->num_frames % d->frames_per_sample != 0)
    throw std::runtime_error(fmt("spatial losses: num_frames %d is not a multiple of frames_per_sample %d", d->num_frames,
                                 d->frames_per_sample));
  if (spHasSmooth(*d) && !(std::isfinite(d->sigma_color_grad) && d->sigma_color_grad > 0.0))
    throw std::runtime_error(fmt("spatial losses: sigma_color_grad must be finite and > 0 (got %g)", d->sigma_color_grad));
  if (spHasContrast(*d) && !std::isfinite(d->contrast_thresh))
    throw std::runtime_error(fmt("spatial losses: contrast_thresh must be finite (got %g)", d->contrast_thresh));
  if (!depth) throw std::runtime_error("spatial losses: null depth");
  if (spHasContrast(*d) && !depthOrig) throw std::runtime_error("spatial losses: null depth_orig (lambda_contrast_loss > 0)");
  if (spHasSmooth(*d) && !image) throw std::runtime_error("spatial losses: null image (lambda_disparity_smooth > 0)");
  if (!total) throw std::runtime_error("spatial losses: null total");
  if (!smooth) throw std::runtime_error("spatial losses: null smooth");
  if (!contrast) throw std::runtime_error("spatial losses: null contrast");
  // one workgroup per 256 pixels of a frame at least: the grid's x extent
  const size_t npx = static_cast<size_t>(d->width) * d->height;
  if (((npx + kConsThreads - 1) / kConsThreads) * static_cast<size_t>(d->num_frames) >= (size_t(1) << 31))
    throw std::runtime_error(fmt("spatial losses: %d frames of %d x %d exceed the grid", d->num_frames, d->width, d->height));
}

template <typename T, int PIX>
void launchSpatialPass(const SpArgs<T>& A, bool grad, hipStream_t s) {
  const dim3 grid(static_cast<unsigned>(static_cast<size_t>(A.nb) * A.F)), block(kConsThreads);
  if (grad) hipLaunchKernelGGL((k_sp_pass<T, PIX, true>), grid, block, 0, s, A);
  else hipLaunchKernelGGL((k_sp_pass<T, PIX, false>), grid, block, 0, s, A);
}

// device pointers in, device results out, on s; the timer's one phase is the pass and its finish
template <typename T>
void launchSpatial(cvd_handle* h, const cvd_spatial_desc& d, const void* depth, const void* depthOrig, const void* image,
                   double* total, double* smooth, double* contrast, void* grad, hipStream_t s, KernelTimer& timer) {
  const int F = d.num_frames, N = d.frames_per_sample, B = F / N, W = d.width, H = d.height;
  const size_t npx = static_cast<size_t>(W) * H;
  const bool sm = spHasSmooth(d), ct = spHasContrast(d);
  Frontend& fe = *h->frontend;
  timer.mark();
  if (!sm && !ct) {  // no term exists
    HIP_CHECK(hipMemsetAsync(total, 0, sizeof(double), s));
    HIP_CHECK(hipMemsetAsync(smooth, 0, sizeof(double) * B, s));
    HIP_CHECK(hipMemsetAsync(contrast, 0, sizeof(double), s));
    if (grad) HIP_CHECK(hipMemsetAsync(grad, 0, sizeof(T) * F * npx, s));
    timer.mark();
    return;
  }
  const void* const vec[] = {depth, ct ? depthOrig : nullptr, sm ? image : nullptr, grad};   // every table read or written
  const int pix = lossPixelsPerThread(W, sizeof(T), vec), nb = lossWorkgroups(npx, pix);
  fe.dSpSlab.ensure(static_cast<size_t>(F) * nb * 3);
  fe.dSpPart.ensure(static_cast<size_t>(B));
  SpArgs<T> A{};
  A.F = F; A.W = W; A.H = H; A.nb = nb;
  A.useSmooth = sm; A.useContrast = ct;
  A.sigma = static_cast<T>(d.sigma_color_grad);
  A.tau = static_cast<T>(d.contrast_thresh);
  // smooth = mean_b S_b: an x-edge of any frame weighs lambda_s / (B N H (W-1)), a y-edge lambda_s / (B N (H-1) W); an edge's
  // contrast value lambda_c / F
  const double nx = static_cast<double>(N) * H * (W - 1), ny = static_cast<double>(N) * (H - 1) * W;
  A.kx = static_cast<T>(sm ? d.lambda_disparity_smooth / (nx * B) : 0.0);
  A.ky = static_cast<T>(sm ? d.lambda_disparity_smooth / (ny * B) : 0.0);
  A.kc = static_cast<T>(ct ? d.lambda_contrast_loss / F : 0.0);
  A.depth = static_cast<const T*>(depth);
  A.depthOrig = ct ? static_cast<const T*>(depthOrig) : nullptr;
  A.image = sm ? static_cast<const T*>(image) : nullptr;
  A.slab = fe.dSpSlab.p;
  A.grad = static_cast<T*>(grad);
  if (pix == 4) launchSpatialPass<T, 4>(A, grad != nullptr, s);
  else launchSpatialPass<T, 1>(A, grad != nullptr, s);
  SpFinishArgs FA{F, N, nb, sm, ct, d.lambda_disparity_smooth, nx, ny, d.lambda_contrast_loss, fe.dSpSlab.p, fe.dSpPart.p,
                  total, smooth, contrast};
  hipLaunchKernelGGL(k_sp_finish, dim3(1), dim3(kSpFinishThreads), 0, s, FA);
  HIP_CHECK(hipGetLastError());
  timer.mark();
}
}  // namespace

// Device arrays in, device results out, on the caller's stream: no copy and no host wait.
void spatialLossesDevice(cvd_handle* h, const cvd_spatial_desc* d, const void* depth, const void* depthOrig, const void* image,
                         double* total, double* smooth, double* contrast, void* grad, hipStream_t s) {
  checkSpatial(d, depth, depthOrig, image, total, smooth, contrast);
  KernelTimer timer(s, nullptr, 1);
  withPrecision(d->precision, [&](auto t) {
    launchSpatial<decltype(t)>(h, *d, depth, depthOrig, image, total, smooth, contrast, grad, s, timer);
  });
}

// Host arrays in, host results out.  kernelMs (may be NULL): {pass + finish} HIP-event time.
void spatialLosses(cvd_handle* h, const cvd_spatial_desc* d, const void* depth, const void* depthOrig, const void* image,
                   double* total, double* smooth, double* contrast, void* grad, double* kernelMs) {
  checkSpatial(d, depth, depthOrig, image, total, smooth, contrast);
  const size_t es = d->precision == CVD_PRECISION_F64 ? 8 : 4, npx = static_cast<size_t>(d->width) * d->height;
  const size_t F = d->num_frames, B = F / d->frames_per_sample;
  const LossHostArrays host{3, {depth, spHasContrast(*d) ? depthOrig : nullptr, spHasSmooth(*d) ? image : nullptr},
                            {F * npx * es, F * npx * es, F * 3 * npx * es}, {nullptr, nullptr}, {0, 0},
                            {total, contrast, smooth}, {1, 1, B}, grad, F * npx * es, nullptr, 0};
  runLossOnHostArrays(h, host, kernelMs, 1, [&](const LossDeviceArrays& dv, hipStream_t s, KernelTimer& timer) {
    withPrecision(d->precision, [&](auto t) {
      launchSpatial<decltype(t)>(h, *d, dv.in[0], dv.in[1], dv.in[2], dv.out[0], dv.out[2], dv.out[1], dv.grad, s, timer);
    });
  });
}

// ---- parameter regulariser and optimizer step over a multi-tensor table (reference loss/parameter_loss.py,
// optimizer/radam.py, torch.optim.Adam; cvd_paramstep.h) ----------------------------------------------------------------------
namespace {
// checks the desc; returns the element size
size_t checkParamDesc(const char* op, const cvd_param_desc* d) {
  if (!d) throw std::runtime_error(fmt("%s: null desc", op));
  if (d->struct_size != CVD_STRUCT_STAMP(cvd_param_desc))
    throw std::runtime_error(fmt("%s: desc.struct_size %llu is not this library's %llu (built against another revision of cvd_hip.h)",
                                 op, static_cast<unsigned long long>(d->struct_size),
                                 static_cast<unsigned long long>(CVD_STRUCT_STAMP(cvd_param_desc))));
  if (d->precision != CVD_PRECISION_F32 && d->precision != CVD_PRECISION_F64)
    throw std::runtime_error(fmt("%s: precision must be 0 (f32) or 1 (f64) (got %d)", op, d->precision));
  if (d->num_tensors < 0) throw std::runtime_error(fmt("%s: num_tensors must be >= 0 (got %d)", op, d->num_tensors));
  return d->precision == CVD_PRECISION_F64 ? 8 : 4;
}

void checkParamCounts(const char* op, int T, const int64_t* counts) {
  if (T && !counts) throw std::runtime_error(fmt("%s: null counts", op));
  long long chunks = 0;
  for (int t = 0; t < T; ++t) {
    if (counts[t] < 0) throw std::runtime_error(fmt("%s: counts[%d] = %lld is negative", op, t, static_cast<long long>(counts[t])));
    chunks += counts[t] / kParamChunk + (counts[t] % kParamChunk != 0);   // (no rounding up by addition: a count near 2^63 would wrap)
    if (chunks >= (1ll << 31)) break;
  }
  if (chunks >= (1ll << 31)) throw std::runtime_error(fmt("%s: %lld chunks exceed the chunk list", op, chunks));
}

// one array of T device addresses: none may be null or off the element size unless its tensor is empty
void checkParamAddresses(const char* op, const char* name, int T, const void* const* a, const int64_t* counts, size_t es) {
  if (T && !a) throw std::runtime_error(fmt("%s: null %s", op, name));
  for (int t = 0; t < T; ++t) {
    if (counts[t] == 0) continue;
    if (!a[t]) throw std::runtime_error(fmt("%s: %s[%d] is a null pointer", op, name, t));
    if (reinterpret_cast<uintptr_t>(a[t]) % es)
      throw std::runtime_error(fmt("%s: %s[%d] = %p is misaligned for %zu-byte elements", op, name, t, a[t], es));
  }
}

void checkParamLambda(const char* op, double lambda) {
  if (!std::isfinite(lambda)) throw std::runtime_error(fmt("%s: lambda must be finite (got %g)", op, lambda));
}

void checkParamRecords(const char* op, int T, const cvd_param_record* r) {
  if (T && !r) throw std::runtime_error(fmt("%s: null records", op));
  for (int t = 0; t < T; ++t) {
    const std::pair<const char*, double> scalars[] = {{"beta1", r[t].beta1}, {"beta2", r[t].beta2}, {"eps", r[t].eps},
                                                      {"grad_decay", r[t].grad_decay}, {"param_decay", r[t].param_decay},
                                                      {"step", r[t].step}, {"denom_scale", r[t].denom_scale}};
    for (const auto& v : scalars)
      if (!std::isfinite(v.second)) throw std::runtime_error(fmt("%s: records[%d].%s must be finite (got %g)", op, t, v.first, v.second));
    for (int k = 0; k < 2; ++k)
      if (!(scalars[k].second >= 0.0 && scalars[k].second < 1.0))
        throw std::runtime_error(fmt("%s: records[%d].%s must lie in [0, 1) (got %g)", op, t, scalars[k].first, scalars[k].second));
    if (!(r[t].denom_scale > 0.0))
      throw std::runtime_error(fmt("%s: records[%d].denom_scale must be > 0 (got %g)", op, t, r[t].denom_scale));
    if (r[t].rule < CVD_PARAM_RULE_ADAM || r[t].rule > CVD_PARAM_RULE_MOMENTS)
      throw std::runtime_error(fmt("%s: records[%d].rule %d is not a CVD_PARAM_RULE_*", op, t, r[t].rule));
  }
}

// The table of T tensors with K pointer arrays (arrays[k] NULL: zeros) on the device, ready for a launch on s.
ParamTable paramTable(ParamTableState& st, int T, int K, const void* const* const* arrays, const int64_t* counts,
                      const cvd_param_record* records, hipStream_t s) {
  ParamTable tab{};
  tab.numTensors = T;
  if (T == 0) return tab;
  const bool same = st.built && st.counts.size() == static_cast<size_t>(T) && std::equal(st.counts.begin(), st.counts.end(), counts);
  const size_t slotBytes = static_cast<size_t>(T) * (kParamStepArrays * sizeof(unsigned long long) + sizeof(ParamRecord));
  if (!same) {
    // the uploads below read host vectors this rewrites, and the staging may move: nothing of the last table may be in flight
    HIP_CHECK(hipStreamSynchronize(s));
    for (int k = 0; k < kParamSlots; ++k) {
      if (st.pending[k]) HIP_CHECK(hipEventSynchronize(st.copied[k]));
      st.pending[k] = false;
      if (!st.copied[k]) HIP_CHECK(hipEventCreateWithFlags(&st.copied[k], hipEventDisableTiming));
    }
    st.built = false;
    st.counts.assign(counts, counts + T);
    st.chunkTensor.clear();
    st.chunkStart.clear();
    for (int t = 0; t < T; ++t)
      for (long long at = 0; at < counts[t]; at += kParamChunk) {
        st.chunkTensor.push_back(t);
        st.chunkStart.push_back(at);
      }
    st.numChunks = static_cast<int>(st.chunkTensor.size());
    st.dCounts.upload(st.counts.data(), st.counts.size(), s);
    st.dChunkTensor.upload(st.chunkTensor.data(), st.chunkTensor.size(), s);
    st.dChunkStart.upload(st.chunkStart.data(), st.chunkStart.size(), s);
    st.dDynamic.ensure(slotBytes);
    if (slotBytes > st.slotBytes) {
      if (st.staging) HIP_CHECK(hipHostFree(st.staging));
      st.staging = nullptr;
      st.slotBytes = 0;
      HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&st.staging), slotBytes * kParamSlots, hipHostMallocDefault));
      st.slotBytes = slotBytes;
    }
    HIP_CHECK(hipStreamSynchronize(s));
    st.built = true;
  }
  const int slot = st.next;
  st.next = (slot + 1) % kParamSlots;
  if (st.pending[slot]) HIP_CHECK(hipEventSynchronize(st.copied[slot]));   // (kParamSlots calls ago: long complete)
  unsigned char* stage = st.staging + static_cast<size_t>(slot) * st.slotBytes;
  auto* addr = reinterpret_cast<unsigned long long*>(stage);
  for (int k = 0; k < kParamStepArrays; ++k)
    for (int t = 0; t < T; ++t)
      addr[static_cast<size_t>(k) * T + t] = k < K && arrays[k] ? reinterpret_cast<uintptr_t>(arrays[k][t]) : 0ull;
  auto* rec = reinterpret_cast<ParamRecord*>(stage + static_cast<size_t>(T) * kParamStepArrays * sizeof(unsigned long long));
  for (int t = 0; t < T; ++t) {
    ParamRecord r{};
    if (records) {
      const cvd_param_record& c = records[t];
      r = ParamRecord{c.beta1, 1.0 - c.beta1, c.beta2, 1.0 - c.beta2, c.eps, c.grad_decay, c.param_decay, c.step, c.denom_scale,
                      c.rule, 0};
    }
    rec[t] = r;
  }
  HIP_CHECK(hipMemcpyAsync(st.dDynamic.p, stage, slotBytes, hipMemcpyHostToDevice, s));
  HIP_CHECK(hipEventRecord(st.copied[slot], s));
  st.pending[slot] = true;
  tab.numChunks = st.numChunks;
  tab.ptrs = reinterpret_cast<const unsigned long long*>(st.dDynamic.p);
  tab.counts = st.dCounts.p;
  tab.chunkTensor = st.dChunkTensor.p;
  tab.chunkStart = st.dChunkStart.p;
  tab.records = reinterpret_cast<const ParamRecord*>(st.dDynamic.p + static_cast<size_t>(T) * kParamStepArrays * sizeof(unsigned long long));
  return tab;
}

dim3 paramGrid(const ParamTable& tab) { return dim3(static_cast<unsigned>(std::min(tab.numChunks, kParamMaxGrid))); }

// value (total != null) and gradient (grad != null) of the regulariser on device tensors, on s; the timer's phases: value, gradient
template <typename T>
void launchParameterL1(cvd_handle* h, int numTensors, const void* const* p, const void* const* p0, const int64_t* counts,
                       double lambda, double* total, void* const* grad, const void* gradOut, bool accumulate, hipStream_t s,
                       KernelTimer& timer) {
  Frontend& fe = *h->frontend;
  const void* const* arrays[kParamL1Arrays] = {p, p0, grad};
  const ParamTable tab = paramTable(fe.paramTable[0][sizeof(T) == 8], numTensors, kParamL1Arrays, arrays, counts, nullptr, s);
  timer.mark();
  if (total) {
    fe.dParamSlab.ensure(kParamMaxGrid);
    const dim3 grid = paramGrid(tab);
    if (tab.numChunks) hipLaunchKernelGGL((k_param_l1<T>), grid, dim3(kConsThreads), 0, s, tab, fe.dParamSlab.p);
    hipLaunchKernelGGL(k_param_l1_finish, dim3(1), dim3(kConsThreads), 0, s, fe.dParamSlab.p, static_cast<int>(tab.numChunks ? grid.x : 0),
                       lambda, total);
    HIP_CHECK(hipGetLastError());
  }
  timer.mark();
  if (grad) {
    if (tab.numChunks) {
      if (accumulate) hipLaunchKernelGGL((k_param_l1_grad<T, true>), paramGrid(tab), dim3(kConsThreads), 0, s, tab, lambda, static_cast<const T*>(gradOut));
      else hipLaunchKernelGGL((k_param_l1_grad<T, false>), paramGrid(tab), dim3(kConsThreads), 0, s, tab, lambda, static_cast<const T*>(gradOut));
      HIP_CHECK(hipGetLastError());
    }
    timer.mark();
  }
}

template <typename T>
void launchParamStep(cvd_handle* h, int numTensors, void* const* p, const void* const* g, void* const* m, void* const* v,
                     const int64_t* counts, const cvd_param_record* records, hipStream_t s, KernelTimer& timer) {
  Frontend& fe = *h->frontend;
  const void* const* arrays[kParamStepArrays] = {p, g, m, v};
  const ParamTable tab = paramTable(fe.paramTable[1][sizeof(T) == 8], numTensors, kParamStepArrays, arrays, counts, records, s);
  timer.mark();
  if (tab.numChunks) {
    hipLaunchKernelGGL((k_param_step<T>), paramGrid(tab), dim3(kConsThreads), 0, s, tab);
    HIP_CHECK(hipGetLastError());
  }
  timer.mark();
}

void checkParameterL1(const char* op, const cvd_param_desc* d, const int64_t* counts, double lambda) {
  checkParamDesc(op, d);
  checkParamCounts(op, d->num_tensors, counts);
  checkParamLambda(op, lambda);
}

// device addresses of the tensors inside a staged flat array
std::vector<const void*> paramAddresses(const unsigned char* base, int T, const int64_t* offsets, size_t es) {
  std::vector<const void*> a(T);
  for (int t = 0; t < T; ++t) a[t] = base + static_cast<size_t>(offsets[t]) * es;
  return a;
}

void checkParamFlat(const char* op, int T, const int64_t* offsets, const int64_t* counts, int64_t flatCount) {
  if (flatCount < 0) throw std::runtime_error(fmt("%s: flat_count %lld is negative", op, static_cast<long long>(flatCount)));
  if (T && !offsets) throw std::runtime_error(fmt("%s: null offsets", op));
  for (int t = 0; t < T; ++t)
    if (offsets[t] < 0 || offsets[t] > flatCount || counts[t] > flatCount - offsets[t])
      throw std::runtime_error(fmt("%s: tensor %d (%lld elements at %lld) leaves the flat arrays of %lld elements", op, t,
                                   static_cast<long long>(counts[t]), static_cast<long long>(offsets[t]),
                                   static_cast<long long>(flatCount)));
}
}  // namespace

void parameterL1Device(cvd_handle* h, const cvd_param_desc* d, const void* const* p, const void* const* p0, const int64_t* counts,
                       double lambda, double* total, void* const* grad, const void* gradOut, int accumulate, hipStream_t s) {
  const char* op = "parameter l1";
  checkParameterL1(op, d, counts, lambda);
  const size_t es = d->precision == CVD_PRECISION_F64 ? 8 : 4;
  checkParamAddresses(op, "p", d->num_tensors, p, counts, es);
  checkParamAddresses(op, "p0", d->num_tensors, p0, counts, es);
  if (!total && !grad) throw std::runtime_error(fmt("%s: neither total nor grad is asked for", op));
  if (grad) {
    checkParamAddresses(op, "grad", d->num_tensors, grad, counts, es);
    if (!gradOut) throw std::runtime_error(fmt("%s: null grad_out", op));
  }
  KernelTimer timer(s, nullptr, 2);
  withPrecision(d->precision, [&](auto t) {
    launchParameterL1<decltype(t)>(h, d->num_tensors, p, p0, counts, lambda, total, grad, gradOut, accumulate != 0, s, timer);
  });
}

// Host arrays in, host results out.  kernelMs (may be NULL): {value, gradient} HIP-event times.
void parameterL1(cvd_handle* h, const cvd_param_desc* d, const int64_t* offsets, const int64_t* counts, int64_t flatCount,
                 const void* p, const void* p0, double lambda, double* total, void* grad, double gradOut, int accumulate,
                 double* kernelMs) {
  const char* op = "parameter l1";
  checkParameterL1(op, d, counts, lambda);
  const int T = d->num_tensors;
  const size_t es = d->precision == CVD_PRECISION_F64 ? 8 : 4;
  checkParamFlat(op, T, offsets, counts, flatCount);
  if (flatCount && !p) throw std::runtime_error(fmt("%s: null p", op));
  if (flatCount && !p0) throw std::runtime_error(fmt("%s: null p0", op));
  if (!total) throw std::runtime_error(fmt("%s: null total", op));
  if (!std::isfinite(gradOut)) throw std::runtime_error(fmt("%s: grad_out must be finite (got %g)", op, gradOut));
  hipStream_t s = h->stream;
  Frontend& fe = *h->frontend;
  const size_t bytes = static_cast<size_t>(flatCount) * es;
  fe.dLossIn[0].upload(static_cast<const unsigned char*>(p), bytes, s);
  fe.dLossIn[1].upload(static_cast<const unsigned char*>(p0), bytes, s);
  if (grad) fe.dLossGrad.upload(static_cast<const unsigned char*>(grad), bytes, s);
  fe.dLossOut.ensure(2);   // the total, the scalar grad_out
  const float go32 = static_cast<float>(gradOut);
  HIP_CHECK(hipMemcpyAsync(fe.dLossOut.p + 1, es == 8 ? static_cast<const void*>(&gradOut) : static_cast<const void*>(&go32), es,
                           hipMemcpyHostToDevice, s));
  const auto ap = paramAddresses(fe.dLossIn[0].p, T, offsets, es), ap0 = paramAddresses(fe.dLossIn[1].p, T, offsets, es);
  const auto ag = grad ? paramAddresses(fe.dLossGrad.p, T, offsets, es) : std::vector<const void*>();
  KernelTimer timer(s, kernelMs, 2);
  withPrecision(d->precision, [&](auto t) {
    launchParameterL1<decltype(t)>(h, T, ap.data(), ap0.data(), counts, lambda, fe.dLossOut.p,
                                   grad ? const_cast<void* const*>(ag.data()) : nullptr, fe.dLossOut.p + 1, accumulate != 0, s, timer);
  });
  HIP_CHECK(hipMemcpyAsync(total, fe.dLossOut.p, sizeof(double), hipMemcpyDeviceToHost, s));
  if (grad) fe.dLossGrad.download(static_cast<unsigned char*>(grad), bytes, s);
  HIP_CHECK(hipStreamSynchronize(s));
  timer.collect();
}

void paramStepDevice(cvd_handle* h, const cvd_param_desc* d, void* const* p, const void* const* g, void* const* m, void* const* v,
                     const int64_t* counts, const cvd_param_record* records, hipStream_t s) {
  const char* op = "param step";
  const size_t es = checkParamDesc(op, d);
  const int T = d->num_tensors;
  checkParamCounts(op, T, counts);
  checkParamAddresses(op, "p", T, p, counts, es);
  checkParamAddresses(op, "g", T, g, counts, es);
  checkParamAddresses(op, "m", T, m, counts, es);
  checkParamAddresses(op, "v", T, v, counts, es);
  checkParamRecords(op, T, records);
  KernelTimer timer(s, nullptr, 1);
  withPrecision(d->precision, [&](auto t) { launchParamStep<decltype(t)>(h, T, p, g, m, v, counts, records, s, timer); });
}

// Host arrays in, p / m / v updated in place.  kernelMs (may be NULL): the launch's HIP-event time.
void paramStep(cvd_handle* h, const cvd_param_desc* d, const int64_t* offsets, const int64_t* counts, int64_t flatCount, void* p,
               const void* g, void* m, void* v, const cvd_param_record* records, double* kernelMs) {
  const char* op = "param step";
  const size_t es = checkParamDesc(op, d);
  const int T = d->num_tensors;
  checkParamCounts(op, T, counts);
  checkParamFlat(op, T, offsets, counts, flatCount);
  const std::pair<const char*, const void*> flat[] = {{"p", p}, {"g", g}, {"m", m}, {"v", v}};
  for (const auto& a : flat)
    if (flatCount && !a.second) throw std::runtime_error(fmt("%s: null %s", op, a.first));
  checkParamRecords(op, T, records);
  hipStream_t s = h->stream;
  Frontend& fe = *h->frontend;
  const size_t bytes = static_cast<size_t>(flatCount) * es;
  std::vector<const void*> dev[kParamStepArrays];
  for (int k = 0; k < kParamStepArrays; ++k) {
    fe.dLossIn[k].upload(static_cast<const unsigned char*>(flat[k].second), bytes, s);
    dev[k] = paramAddresses(fe.dLossIn[k].p, T, offsets, es);
  }
  KernelTimer timer(s, kernelMs, 1);
  withPrecision(d->precision, [&](auto t) {
    launchParamStep<decltype(t)>(h, T, const_cast<void* const*>(dev[0].data()), dev[1].data(), const_cast<void* const*>(dev[2].data()),
                                 const_cast<void* const*>(dev[3].data()), counts, records, s, timer);
  });
  fe.dLossIn[0].download(static_cast<unsigned char*>(p), bytes, s);
  fe.dLossIn[2].download(static_cast<unsigned char*>(m), bytes, s);
  fe.dLossIn[3].download(static_cast<unsigned char*>(v), bytes, s);
  HIP_CHECK(hipStreamSynchronize(s));
  timer.collect();
}

long long paramChunkElements() { return kParamChunk; }

// ---- fine-tuning batches from a device-resident store (reference loaders/video_dataset.py; cvd_batch.h) ---------------------------
namespace {
const char* kDsOp = "dataset";

DatasetState& datasetStore(cvd_handle* h, const char* what) {
  DatasetState& ds = h->frontend->dataset;
  if (!ds.created) throw std::runtime_error(fmt("%s %s: no store (cvd_dataset_create first)", kDsOp, what));
  return ds;
}

void checkDatasetRange(const char* what, int first, int count, int total, const char* unit) {
  if (first < 0 || count < 0 || first > total || count > total - first)
    throw std::runtime_error(fmt("%s %s: %s [%d, %d + %d) leave the store's %d", kDsOp, what, unit, first, first, count, total));
}

// the gather-relevant part of a Layout from the two transform descriptors (makeLayout's statement of it, without a video)
Layout datasetLayout(int F, const cvd_xform_desc& dd, const cvd_xform_desc& sd) {
  Layout L{};
  L.F = F;
  L.depthType = dd.depth_type;
  L.N = xformBlockSize(dd);
  L.cubic = dd.cubic_interpolation ? 1 : 0;
  L.gx = dd.depth_type == CVD_DEPTH_GRID ? dd.grid_size[0] : 1;
  L.gy = dd.depth_type == CVD_DEPTH_GRID ? dd.grid_size[1] : 1;
  L.maxcx = std::nextafter(static_cast<double>(L.gx - 1), 0.0);
  L.maxcy = std::nextafter(static_cast<double>(L.gy - 1), 0.0);
  L.gz = 1;
  L.maxcz = 0.0;
  L.dispMin = 0.0;
  L.dispInterval = 1.0;
  L.nD = xformNumBlocks(dd) * xformBlockSize(dd);
  L.spatialType = sd.spatial_type;
  L.sgx = sd.grid_size[0];
  L.sgy = sd.grid_size[1];
  L.smaxcx = std::nextafter(static_cast<double>(L.sgx - 1), 0.0);
  L.smaxcy = std::nextafter(static_cast<double>(L.sgy - 1), 0.0);
  L.nS = xformNumBlocks(sd) * xformBlockSize(sd);
  L.B = 7 + L.nD + L.nS;
  return L;
}

// the outputs of a batch in the order of cvd_dataset_batch_out's members: kBatchRequired that the shape of the store decides, then
// the optional scales, warp and depth_orig
constexpr int kBatchRequired = 18, kBatchOutputs = 21;
const char* const kBatchOutNames[kBatchOutputs] = {"images", "extrinsics", "intrinsics", "gc_indices", "gc_flows[0]", "gc_flows[1]",
                                                   "gc_masks[0]", "gc_masks[1]", "ts_indices", "ts_flows[0]", "ts_flows[1]", "ts_flows[2]",
                                                   "ts_flows[3]", "ts_masks[0]", "ts_masks[1]", "ts_masks[2]", "ts_masks[3]", "ts_valid",
                                                   "scales", "warp", "depth_orig"};
void batchOutMembers(const cvd_dataset_batch_out* o, void** list) {
  void* m[kBatchOutputs] = {o->images, o->extrinsics, o->intrinsics, o->gc_indices, o->gc_flows[0], o->gc_flows[1], o->gc_masks[0],
                            o->gc_masks[1], o->ts_indices, o->ts_flows[0], o->ts_flows[1], o->ts_flows[2], o->ts_flows[3],
                            o->ts_masks[0], o->ts_masks[1], o->ts_masks[2], o->ts_masks[3], o->ts_valid, o->scales, o->warp,
                            o->depth_orig};
  std::copy(m, m + kBatchOutputs, list);
}

// checks a batch request against the store (before any device work); fills the bytes of every output (0: not written)
void checkBatch(const DatasetState& ds, const char* what, int B, const int64_t* indices, const cvd_dataset_batch_out* o,
                size_t* bytes) {
  if (B < 1) throw std::runtime_error(fmt("%s %s: batch size must be >= 1 (got %d)", kDsOp, what, B));
  if (ds.S < 1) throw std::runtime_error(fmt("%s %s: the store has no samples", kDsOp, what));
  if (!indices) throw std::runtime_error(fmt("%s %s: null indices", kDsOp, what));
  if (!o) throw std::runtime_error(fmt("%s %s: null out", kDsOp, what));
  if (o->struct_size != CVD_STRUCT_STAMP(cvd_dataset_batch_out))
    throw std::runtime_error(fmt("%s %s: out.struct_size %llu is not this library's %llu (built against another revision of cvd_hip.h)",
                                 kDsOp, what, static_cast<unsigned long long>(o->struct_size),
                                 static_cast<unsigned long long>(CVD_STRUCT_STAMP(cvd_dataset_batch_out))));
  const size_t npx = ds.npx(), b = static_cast<size_t>(B), N = static_cast<size_t>(ds.N), f = sizeof(float);
  const bool ts = ds.N > 2;
  const size_t flowB = b * 2 * npx * f, maskB = b * npx * f;
  const size_t sizes[kBatchRequired] = {b * N * 3 * npx * f, b * N * 12 * f, b * N * 4 * f, b * 2 * sizeof(int64_t), flowB, flowB, maskB, maskB,
                            ts ? b * 4 * sizeof(int64_t) : 0, ts ? flowB : 0, ts ? flowB : 0, ts ? flowB : 0, ts ? flowB : 0,
                            ts ? maskB : 0, ts ? maskB : 0, ts ? maskB : 0, ts ? maskB : 0, ts ? b * 2 * f : 0};
  void* members[kBatchOutputs];
  batchOutMembers(o, members);
  for (int k = 0; k < kBatchRequired; ++k) {
    bytes[k] = sizes[k];
    if (sizes[k] && !members[k]) throw std::runtime_error(fmt("%s %s: null output %s", kDsOp, what, kBatchOutNames[k]));
  }
  if (o->scales && ds.scaleMode == 0) throw std::runtime_error(fmt("%s %s: scales asked for, but no scale table is set", kDsOp, what));
  if (o->warp && !ds.haveWarp) throw std::runtime_error(fmt("%s %s: warp asked for, but no warp table is set", kDsOp, what));
  if (o->depth_orig && !ds.hasDepthOrig)
    throw std::runtime_error(fmt("%s %s: depth_orig asked for, but the store was created without it", kDsOp, what));
  bytes[18] = o->scales ? b * N * (ds.scaleMode == 2 ? npx : 1) * f : 0;
  bytes[19] = o->warp ? b * N * 2 * npx * f : 0;
  bytes[20] = o->depth_orig ? b * 2 * npx * f : 0;
}

// one launch for the whole batch, on s; `o` holds DEVICE addresses
void launchDatasetBatch(DatasetState& ds, int B, const long long* indices, const cvd_dataset_batch_out& o, hipStream_t s) {
  DatasetStore st{ds.color.p, ds.flow.p, ds.mask.p, ds.hasDepthOrig ? ds.depthOrig.p : nullptr, ds.ext.p, ds.intr.p,
                  ds.scaleMode ? ds.scales.p : nullptr, ds.haveWarp ? ds.warp.p : nullptr, ds.samples.p, ds.S,
                  static_cast<int>(ds.npx()), ds.N, ds.scaleMode};
  DatasetBatch out{};
  auto fp = [](void* p) { return static_cast<float*>(p); };
  out.images = fp(o.images); out.ext = fp(o.extrinsics); out.intr = fp(o.intrinsics);
  out.gcIndices = static_cast<long long*>(o.gc_indices);
  out.tsIndices = static_cast<long long*>(o.ts_indices);
  for (int d = 0; d < 2; ++d) { out.gcFlow[d] = fp(o.gc_flows[d]); out.gcMask[d] = fp(o.gc_masks[d]); }
  for (int d = 0; d < 4; ++d) { out.tsFlow[d] = fp(o.ts_flows[d]); out.tsMask[d] = fp(o.ts_masks[d]); }
  out.tsValid = fp(o.ts_valid); out.scales = fp(o.scales); out.warp = fp(o.warp); out.depthOrig = fp(o.depth_orig);
  const int ts = ds.N > 2 ? 4 : 0;
  out.segGcFlow = ds.N;
  out.segGcMask = out.segGcFlow + 2;
  out.segTsFlow = out.segGcMask + 2;
  out.segTsMask = out.segTsFlow + ts;
  out.segScale = out.segTsMask + ts;
  out.segWarp = out.segScale + (o.scales && ds.scaleMode == 2 ? ds.N : 0);
  out.segDepth = out.segWarp + (o.warp ? ds.N : 0);
  out.segSmall = out.segDepth + (o.depth_orig ? 2 : 0);
  const bool vec = ds.npx() % 4 == 0;   // every plane then starts 16-byte aligned from an aligned base
  const size_t lanes = vec ? ds.npx() / 4 : ds.npx();
  const dim3 grid(static_cast<unsigned>((lanes + kBatchThreads - 1) / kBatchThreads), out.segSmall + 1, B);
  if (vec) hipLaunchKernelGGL((k_dataset_batch<true>), grid, dim3(kBatchThreads), 0, s, st, out, indices, B, ds.bad.p);
  else hipLaunchKernelGGL((k_dataset_batch<false>), grid, dim3(kBatchThreads), 0, s, st, out, indices, B, ds.bad.p);
  HIP_CHECK(hipGetLastError());
}
}  // namespace

// Builds the store and its sample table (reference loaders/video_dataset.py:223-256, 309-367: which flows a sample reads, the
// rule 0 < k < num_frames - 1 for real neighbours, the clamped neighbour indices).  pairFrames [Q][2]: the directed pairs whose
// flow and mask the store holds, slot = position; samples [S][2].
void datasetCreate(cvd_handle* h, const cvd_dataset_desc* d, const int32_t* pairFrames, const int32_t* samples) {
  const char* what = "create";
  if (!d) throw std::runtime_error(fmt("%s %s: null desc", kDsOp, what));
  if (d->struct_size != CVD_STRUCT_STAMP(cvd_dataset_desc))
    throw std::runtime_error(fmt("%s %s: desc.struct_size %llu is not this library's %llu (built against another revision of cvd_hip.h)",
                                 kDsOp, what, static_cast<unsigned long long>(d->struct_size),
                                 static_cast<unsigned long long>(CVD_STRUCT_STAMP(cvd_dataset_desc))));
  const int F = d->num_frames, Q = d->num_pairs, S = d->num_samples;
  if (F < 1 || d->height < 1 || d->width < 1)
    throw std::runtime_error(fmt("%s %s: invalid shape (%d frames of %d x %d)", kDsOp, what, F, d->height, d->width));
  if (static_cast<long long>(d->height) * d->width > (1ll << 30)) throw std::runtime_error(fmt("%s %s: frame too large", kDsOp, what));
  if (Q < 0 || S < 0) throw std::runtime_error(fmt("%s %s: negative count (%d pairs, %d samples)", kDsOp, what, Q, S));
  if ((Q && !pairFrames) || (S && !samples)) throw std::runtime_error(fmt("%s %s: null pair or sample list", kDsOp, what));
  if (d->temporal != 0 && d->temporal != 1) throw std::runtime_error(fmt("%s %s: temporal must be 0 or 1 (got %d)", kDsOp, what, d->temporal));
  const int ruleF = d->neighbor_rule_frames > 0 ? d->neighbor_rule_frames : F;
  if (ruleF > F)
    throw std::runtime_error(fmt("%s %s: neighbor_rule_frames %d exceeds the store's %d frames", kDsOp, what, ruleF, F));
  std::map<std::pair<int, int>, int> slotOf;
  for (int q = 0; q < Q; ++q) {
    const int a = pairFrames[2 * q], b = pairFrames[2 * q + 1];
    for (int f : {a, b})
      if (f < 0 || f >= F) throw std::runtime_error(fmt("%s %s: frame %d of pair %d is out of range [0, %d)", kDsOp, what, f, q, F));
    if (!slotOf.emplace(std::make_pair(a, b), q).second)
      throw std::runtime_error(fmt("%s %s: directed pair (%d, %d) is listed twice", kDsOp, what, a, b));
  }
  std::vector<DatasetSample> table(S);
  for (int i = 0; i < S; ++i) {
    const int ab[2] = {samples[2 * i], samples[2 * i + 1]};
    DatasetSample& sm = table[i];
    for (int k = 0; k < 2; ++k)
      if (ab[k] < 0 || ab[k] >= F)
        throw std::runtime_error(fmt("%s %s: frame %d of sample %d is out of range [0, %d)", kDsOp, what, ab[k], i, F));
    for (int k = 0; k < 2; ++k) {
      const auto it = slotOf.find({ab[k], ab[1 - k]});
      if (it == slotOf.end())
        throw std::runtime_error(fmt("%s %s: sample %d (%d, %d): direction (%d, %d) is not in the pair list", kDsOp, what, i, ab[0],
                                     ab[1], ab[k], ab[1 - k]));
      sm.frame[k] = ab[k];
      sm.slot[k] = it->second;
    }
    for (int k = 0; k < 2; ++k) {
      const bool interior = 0 < ab[k] && ab[k] < ruleF - 1;
      sm.valid[k] = interior ? 1 : 0;
      for (int j = 0; j < 2; ++j) {
        const int nb = ab[k] + (j ? 1 : -1);
        sm.frame[2 + 2 * k + j] = std::max(0, std::min(nb, ruleF - 1));
        sm.slot[2 + 2 * k + j] = -1;
        if (d->temporal && interior) {
          const auto it = slotOf.find({ab[k], nb});
          if (it == slotOf.end())
            throw std::runtime_error(fmt("%s %s: temporal sample %d: neighbour flow (%d, %d) of interior frame %d is not in the pair list",
                                         kDsOp, what, i, ab[k], nb, ab[k]));
          sm.slot[2 + 2 * k + j] = it->second;
        }
      }
    }
  }
  // (validated: device work from here)
  DatasetState& ds = h->frontend->dataset;
  hipStream_t s = h->stream;
  HIP_CHECK(hipDeviceSynchronize());   // a batch of the previous store may be in flight on a caller's stream
  ds.clear();
  ds.F = F; ds.H = d->height; ds.W = d->width; ds.Q = Q; ds.S = S; ds.N = d->temporal ? 6 : 2;
  ds.hasDepthOrig = d->has_depth_orig != 0;
  const size_t npx = ds.npx();
  auto zeroed = [&](auto& buf, size_t n) {
    buf.ensure(std::max<size_t>(n, 1));
    HIP_CHECK(hipMemsetAsync(buf.p, 0, std::max<size_t>(n, 1) * sizeof(*buf.p), s));
  };
  zeroed(ds.color, static_cast<size_t>(F) * npx * 3);
  zeroed(ds.flow, static_cast<size_t>(Q) * npx * 2);
  zeroed(ds.mask, static_cast<size_t>(Q) * npx);
  if (ds.hasDepthOrig) zeroed(ds.depthOrig, static_cast<size_t>(F) * npx);
  zeroed(ds.ext, static_cast<size_t>(F) * 12);
  zeroed(ds.intr, static_cast<size_t>(F) * 4);
  zeroed(ds.bad, 1);
  ds.samples.upload(table.data(), table.size(), s);
  HIP_CHECK(hipStreamSynchronize(s));
  ds.created = true;
}

void datasetClear(cvd_handle* h) {
  HIP_CHECK(hipDeviceSynchronize());
  h->frontend->dataset.clear();
}

// host f32 [count][H][W][3], in the channel order the batch returns (reference load_color, loaders/video_dataset.py:49-60)
void datasetSetColors(cvd_handle* h, int first, int count, const float* hwc3) {
  DatasetState& ds = datasetStore(h, "set_colors");
  checkDatasetRange("set_colors", first, count, ds.F, "frames");
  if (count == 0) return;
  if (!hwc3) throw std::runtime_error(fmt("%s set_colors: null input", kDsOp));
  HIP_CHECK(hipMemcpyAsync(ds.color.p + static_cast<size_t>(first) * ds.npx() * 3, hwc3, static_cast<size_t>(count) * ds.npx() * 3 * sizeof(float),
                           hipMemcpyHostToDevice, h->stream));
  HIP_CHECK(hipStreamSynchronize(h->stream));
}

// file layout: flow f32 [count][H][W][2], mask u8 [count][H][W] (reference load_flow / load_mask, loaders/video_dataset.py:63-78)
void datasetSetFlows(cvd_handle* h, int first, int count, const float* flow, const uint8_t* mask) {
  DatasetState& ds = datasetStore(h, "set_flows");
  checkDatasetRange("set_flows", first, count, ds.Q, "pairs");
  if (count == 0) return;
  if (!flow || !mask) throw std::runtime_error(fmt("%s set_flows: null input", kDsOp));
  const size_t npx = ds.npx();
  HIP_CHECK(hipMemcpyAsync(ds.flow.p + static_cast<size_t>(first) * npx * 2, flow, static_cast<size_t>(count) * npx * 2 * sizeof(float),
                           hipMemcpyHostToDevice, h->stream));
  HIP_CHECK(hipMemcpyAsync(ds.mask.p + static_cast<size_t>(first) * npx, mask, static_cast<size_t>(count) * npx, hipMemcpyHostToDevice, h->stream));
  HIP_CHECK(hipStreamSynchronize(h->stream));
}

// f32 [count][H][W], already 1 / disparity (reference depth_fine_tuning.py:457-471)
void datasetSetDepthOrig(cvd_handle* h, int first, int count, const float* depth) {
  DatasetState& ds = datasetStore(h, "set_depth_orig");
  if (!ds.hasDepthOrig) throw std::runtime_error(fmt("%s set_depth_orig: the store was created without depth_orig", kDsOp));
  checkDatasetRange("set_depth_orig", first, count, ds.F, "frames");
  if (count == 0) return;
  if (!depth) throw std::runtime_error(fmt("%s set_depth_orig: null input", kDsOp));
  HIP_CHECK(hipMemcpyAsync(ds.depthOrig.p + static_cast<size_t>(first) * ds.npx(), depth, static_cast<size_t>(count) * ds.npx() * sizeof(float),
                           hipMemcpyHostToDevice, h->stream));
  HIP_CHECK(hipStreamSynchronize(h->stream));
}

// f32 [F][3][4] and [F][4], as update_poses forms them (reference loaders/video_dataset.py:177-189)
void datasetSetCameras(cvd_handle* h, const float* ext, const float* intr) {
  DatasetState& ds = datasetStore(h, "set_cameras");
  if (!ext || !intr) throw std::runtime_error(fmt("%s set_cameras: null input", kDsOp));
  ds.ext.upload(ext, static_cast<size_t>(ds.F) * 12, h->stream);
  ds.intr.upload(intr, static_cast<size_t>(ds.F) * 4, h->stream);
  HIP_CHECK(hipStreamSynchronize(h->stream));
}

// The per-frame tables from the transforms' parameters, one launch per table (reference loaders/video_dataset.py:191-217).
void datasetSetXforms(cvd_handle* h, const cvd_xform_desc* dd, const double* dparams, const cvd_xform_desc* sd, const double* sparams) {
  DatasetState& ds = datasetStore(h, "set_xforms");
  if (!dd || !sd) throw std::runtime_error(fmt("%s set_xforms: null descriptor", kDsOp));
  if (dd->type != CVD_XFORM_DEPTH || sd->type != CVD_XFORM_SPATIAL)
    throw std::runtime_error(fmt("%s set_xforms: a depth and a spatial descriptor are expected, in this order", kDsOp));
  // what the reference refuses (:195-217), before any device work
  if (dd->depth_type != CVD_DEPTH_IDENTITY && dd->value_xform != CVD_VALUE_SCALE)
    throw std::runtime_error("We only support scale-based transforms at the moment.");
  if (dd->depth_type != CVD_DEPTH_IDENTITY && dd->depth_type != CVD_DEPTH_GLOBAL && dd->depth_type != CVD_DEPTH_GRID)
    throw std::runtime_error(fmt("Unsupported depth transform type '%d'.", dd->depth_type));
  if (sd->spatial_type < CVD_SPATIAL_IDENTITY || sd->spatial_type > CVD_SPATIAL_BICUBIC_GRID)
    throw std::runtime_error(fmt("Unsupported spatial transform type '%d'.", sd->spatial_type));
  if (dd->depth_type == CVD_DEPTH_GRID && dd->grid_size[2] > 1)
    throw std::runtime_error(fmt("%s set_xforms: a depth-wise grid (grid z = %d) needs the source depth for its map: evaluate it on the "
                                 "host and use cvd_dataset_set_maps", kDsOp, dd->grid_size[2]));
  if (ds.W < 2 || ds.H < 2) throw std::runtime_error(fmt("%s set_xforms: raster too small", kDsOp));
  const Layout L = datasetLayout(ds.F, *dd, *sd);   // (throws what the transforms' own constructors throw for a bad grid)
  if ((L.nD && !dparams) || (L.nS && !sparams)) throw std::runtime_error(fmt("%s set_xforms: null parameters", kDsOp));
  int KD, KS;
  tapCounts(L, KD, KS);
  hipStream_t s = h->stream;
  const size_t F = ds.F, npx = ds.npx();
  HIP_CHECK(hipDeviceSynchronize());   // the tables may be read by a batch in flight on a caller's stream
  ds.params.ensure(F * (L.nD + L.nS));
  if (L.nD) HIP_CHECK(hipMemcpyAsync(ds.params.p, dparams, F * L.nD * sizeof(double), hipMemcpyHostToDevice, s));
  if (L.nS) HIP_CHECK(hipMemcpyAsync(ds.params.p + F * L.nD, sparams, F * L.nS * sizeof(double), hipMemcpyHostToDevice, s));
  const dim3 grid(static_cast<unsigned>((npx + 255) / 256), 1, ds.F), block(256);
  if (L.depthType == CVD_DEPTH_GRID) {
    ds.scales.ensure(F * npx);
    if (KD == 16) hipLaunchKernelGGL((k_dataset_scale_map<16>), grid, block, 0, s, L, ds.W, ds.H, ds.params.p, ds.scales.p);
    else hipLaunchKernelGGL((k_dataset_scale_map<4>), grid, block, 0, s, L, ds.W, ds.H, ds.params.p, ds.scales.p);
    ds.scaleMode = 2;
  } else {
    ds.scales.ensure(F);
    hipLaunchKernelGGL(k_dataset_scale_scalars, dim3((ds.F + 255) / 256), block, 0, s, ds.F, L.nD, ds.params.p, ds.scales.p);
    ds.scaleMode = 1;
  }
  HIP_CHECK(hipGetLastError());
  ds.warp.ensure(F * 2 * npx);
  const double* sp = ds.params.p + F * L.nD;
  if (KS == 0) hipLaunchKernelGGL((k_dataset_warp_map<0>), grid, block, 0, s, L, ds.W, ds.H, sp, ds.warp.p);
  else if (KS == 4) hipLaunchKernelGGL((k_dataset_warp_map<4>), grid, block, 0, s, L, ds.W, ds.H, sp, ds.warp.p);
  else hipLaunchKernelGGL((k_dataset_warp_map<16>), grid, block, 0, s, L, ds.W, ds.H, sp, ds.warp.p);
  HIP_CHECK(hipGetLastError());
  ds.haveWarp = true;
  HIP_CHECK(hipStreamSynchronize(s));
}

// The same tables from host arrays: scales f32 [F][H][W] (scaleIsMap) or [F], or NULL (no scales); warp f32 [F][2][H][W] or NULL.
void datasetSetMaps(cvd_handle* h, const float* scales, int scaleIsMap, const float* warp) {
  DatasetState& ds = datasetStore(h, "set_maps");
  const size_t F = ds.F, npx = ds.npx();
  HIP_CHECK(hipDeviceSynchronize());
  ds.scaleMode = scales ? (scaleIsMap ? 2 : 1) : 0;
  if (scales) ds.scales.upload(scales, scaleIsMap ? F * npx : F, h->stream);
  ds.haveWarp = warp != nullptr;
  if (warp) ds.warp.upload(warp, F * 2 * npx, h->stream);
  HIP_CHECK(hipStreamSynchronize(h->stream));
}

// Device indices in, device outputs out, one launch on the caller's stream: no copy and no host wait.  An index outside [0, S)
// cannot be seen here: the kernel clamps and counts it (datasetBadIndices).
void datasetBatchDevice(cvd_handle* h, int B, const int64_t* indices, const cvd_dataset_batch_out* out, hipStream_t s) {
  DatasetState& ds = datasetStore(h, "batch");
  size_t bytes[kBatchOutputs];
  checkBatch(ds, "batch", B, indices, out, bytes);
  launchDatasetBatch(ds, B, reinterpret_cast<const long long*>(indices), *out, s);
}

// Host indices in, host outputs out.  kernelMs (may be NULL): the launch's HIP-event time.
void datasetBatch(cvd_handle* h, int B, const int64_t* indices, const cvd_dataset_batch_out* out, double* kernelMs) {
  DatasetState& ds = datasetStore(h, "batch");
  size_t sizes[kBatchOutputs];
  checkBatch(ds, "batch", B, indices, out, sizes);
  for (int b = 0; b < B; ++b)
    if (indices[b] < 0 || indices[b] >= ds.S)
      throw std::runtime_error(fmt("%s batch: indices[%d] = %lld is outside the store's %d samples", kDsOp, b,
                                   static_cast<long long>(indices[b]), ds.S));
  hipStream_t s = h->stream;
  void* hostMembers[kBatchOutputs];
  batchOutMembers(out, hostMembers);
  // staging: the indices, then every output at a 256-byte boundary
  auto pad = [](size_t n) { return (n + 255) / 256 * 256; };
  size_t total = pad(static_cast<size_t>(B) * sizeof(int64_t));
  size_t offset[kBatchOutputs];
  for (int k = 0; k < kBatchOutputs; ++k) { offset[k] = total; total += pad(sizes[k]); }
  ds.stage.ensure(total);
  HIP_CHECK(hipMemcpyAsync(ds.stage.p, indices, static_cast<size_t>(B) * sizeof(int64_t), hipMemcpyHostToDevice, s));
  auto dev = [&](int k) -> void* { return sizes[k] ? ds.stage.p + offset[k] : nullptr; };
  cvd_dataset_batch_out d{};
  d.struct_size = out->struct_size;
  d.images = dev(0); d.extrinsics = dev(1); d.intrinsics = dev(2); d.gc_indices = dev(3);
  d.gc_flows[0] = dev(4); d.gc_flows[1] = dev(5); d.gc_masks[0] = dev(6); d.gc_masks[1] = dev(7);
  d.ts_indices = dev(8);
  for (int k = 0; k < 4; ++k) { d.ts_flows[k] = dev(9 + k); d.ts_masks[k] = dev(13 + k); }
  d.ts_valid = dev(17); d.scales = dev(18); d.warp = dev(19); d.depth_orig = dev(20);
  KernelTimer timer(s, kernelMs, 1);
  timer.mark();
  launchDatasetBatch(ds, B, reinterpret_cast<const long long*>(ds.stage.p), d, s);
  timer.mark();
  for (int k = 0; k < kBatchOutputs; ++k)
    if (sizes[k]) HIP_CHECK(hipMemcpyAsync(hostMembers[k], ds.stage.p + offset[k], sizes[k], hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
  timer.collect();
}

// Out-of-range indices the device entry point has clamped since cvd_dataset_create.  Waits for the device.
long long datasetBadIndices(cvd_handle* h) {
  DatasetState& ds = datasetStore(h, "bad_indices");
  HIP_CHECK(hipDeviceSynchronize());
  unsigned int n = 0;
  HIP_CHECK(hipMemcpy(&n, ds.bad.p, sizeof(n), hipMemcpyDeviceToHost));
  return n;
}

// ---- RAFT's correlation pyramid, lookup and convex upsampling (reference raft/core/corr.py, raft/core/raft.py:49-60;
// cvd_raftops.h).  Device arrays on the caller's stream: one launch each, no copy, no host wait, no scratch. -----
namespace {
void checkRaftPyramidShape(const char* who, int h2, int w2, int levels) {
  if (levels < 1 || levels > kRaftMaxLevels)
    throw std::runtime_error(fmt("%s: num_levels must be 1..%d (got %d)", who, kRaftMaxLevels, levels));
  if (h2 < 1 || w2 < 1) throw std::runtime_error(fmt("%s: the correlation maps must be at least 1 x 1 (got %d x %d)", who, h2, w2));
  // (the reference divides by (size - 1) of every level it samples: a 1-wide level is NaN there)
  if ((h2 >> (levels - 1)) < 2 || (w2 >> (levels - 1)) < 2)
    throw std::runtime_error(fmt("%s: level %d of a %d x %d map is %d x %d, below 2 x 2", who, levels - 1, h2, w2,
                                 h2 >> (levels - 1), w2 >> (levels - 1)));
}
void checkAligned16(const char* who, const char* name, const void* p) {
  if (!p) throw std::runtime_error(fmt("%s: null %s", who, name));
  if (reinterpret_cast<uintptr_t>(p) & 15) throw std::runtime_error(fmt("%s: %s is not 16-byte aligned", who, name));
}
unsigned raftGrid(const char* who, long long threads) {
  const long long blocks = (threads + kRaftThreads - 1) / kRaftThreads;
  if (blocks > 0x7fffffffll) throw std::runtime_error(fmt("%s: %lld workgroups exceed the grid", who, blocks));
  return static_cast<unsigned>(blocks);
}
}  // namespace

void raftCorrPyramidDevice(cvd_handle*, long long Q, int h2, int w2, int dim, int levels, const float* raw, float* const* level,
                           hipStream_t s) {
  const char* who = "raft corr pyramid";
  if (Q < 1) throw std::runtime_error(fmt("%s: num_queries must be >= 1 (got %lld)", who, Q));
  if (dim < 1) throw std::runtime_error(fmt("%s: dim must be >= 1 (got %d)", who, dim));
  checkRaftPyramidShape(who, h2, w2, levels);
  checkAligned16(who, "raw", raw);
  if (!level) throw std::runtime_error(fmt("%s: null levels", who));
  CorrPyramidArgs A{};
  A.raw = raw;
  for (int l = 0; l < levels; ++l) {
    checkAligned16(who, "level", level[l]);
    A.level[l] = level[l];
  }
  A.Q = Q; A.h = h2; A.w = w2; A.levels = levels;
  A.nbx = (w2 + 7) / 8; A.nby = (h2 + 7) / 8;
  A.scale = sqrtf(static_cast<float>(dim));
  const unsigned grid = raftGrid(who, corrPyramidThreads(A));
  hipLaunchKernelGGL(k_corr_pyramid, dim3(grid), dim3(kRaftThreads), 0, s, A);
  HIP_CHECK(hipGetLastError());
}

namespace {
template <int R>
void launchCorrLookup(const CorrLookupArgs& A, unsigned tiles, hipStream_t s) {
  hipLaunchKernelGGL((k_corr_lookup<R>), dim3(tiles, A.levels), dim3(kRaftThreads), 0, s, A);
}
}  // namespace

void raftCorrLookupDevice(cvd_handle*, int B, int h1, int w1, int h2, int w2, int levels, int radius, const float* const* level,
                          const float* coords, float* out, hipStream_t s) {
  const char* who = "raft corr lookup";
  if (B < 1 || h1 < 1 || w1 < 1) throw std::runtime_error(fmt("%s: batch, h1 and w1 must be >= 1 (got %d, %d, %d)", who, B, h1, w1));
  if (radius < 1 || radius > kRaftMaxRadius)
    throw std::runtime_error(fmt("%s: radius must be 1..%d (got %d)", who, kRaftMaxRadius, radius));
  checkRaftPyramidShape(who, h2, w2, levels);
  if (static_cast<long long>(h1) * w1 > 0x7fffffffll) throw std::runtime_error(fmt("%s: %d x %d queries per image exceed 2^31", who, h1, w1));
  if (!level || !coords || !out) throw std::runtime_error(fmt("%s: null array", who));
  CorrLookupArgs A{};
  for (int l = 0; l < levels; ++l) {
    if (!level[l]) throw std::runtime_error(fmt("%s: null level %d", who, l));
    A.level[l] = level[l];
  }
  A.coords = coords; A.out = out;
  A.hw1 = h1 * w1;
  A.Q = static_cast<long long>(B) * A.hw1;
  A.h2 = h2; A.w2 = w2; A.levels = levels;
  const long long tiles = (A.Q + kRaftTileQueries - 1) / kRaftTileQueries;
  if (tiles > 0x7fffffffll) throw std::runtime_error(fmt("%s: %lld workgroups exceed the grid", who, tiles));
  switch (radius) {
    case 1: launchCorrLookup<1>(A, static_cast<unsigned>(tiles), s); break;
    case 2: launchCorrLookup<2>(A, static_cast<unsigned>(tiles), s); break;
    case 3: launchCorrLookup<3>(A, static_cast<unsigned>(tiles), s); break;
    default: launchCorrLookup<4>(A, static_cast<unsigned>(tiles), s); break;
  }
  HIP_CHECK(hipGetLastError());
}

void raftUpsampleFlowDevice(cvd_handle*, int N, int H, int W, const float* flow, const float* mask, float* out, hipStream_t s) {
  const char* who = "raft upsample flow";
  if (N < 1 || H < 1 || W < 1) throw std::runtime_error(fmt("%s: n, height and width must be >= 1 (got %d, %d, %d)", who, N, H, W));
  if (!flow || !mask) throw std::runtime_error(fmt("%s: null array", who));
  checkAligned16(who, "out", out);
  ConvexUpsampleArgs A{};
  A.flow = flow; A.mask = mask; A.out = out;
  A.H = H; A.W = W;
  A.total = static_cast<long long>(N) * H * 8 * W;
  const unsigned grid = raftGrid(who, A.total);
  hipLaunchKernelGGL(k_convex_upsample, dim3(grid), dim3(kRaftThreads), 0, s, A);
  HIP_CHECK(hipGetLastError());
}


// ---- SepConvGRU of RAFT's update block (reference raft/core/update.py:37-75; cvd_raftgru.h).  Device arrays on
// the caller's stream: four launches, no copy, no host wait once the handle's scratch has its size. ---------------------------------
void raftSepConvGruDevice(cvd_handle* h, int B, int H, int W, const float* hidden, int numSegments, const float* const* segments,
                          const int32_t* segmentChannels, const float* const* weights, const float* const* biases, float* out,
                          hipStream_t s, double* kernelMs) {
  const char* who = "raft sepconv gru";
  if (B < 1 || H < 1 || W < 1) throw std::runtime_error(fmt("%s: batch, height and width must be >= 1 (got %d, %d, %d)", who, B, H, W));
  const long long HW = static_cast<long long>(H) * W;
  if (HW > 0x7fffffffll) throw std::runtime_error(fmt("%s: %d x %d pixels per image exceed 2^31", who, H, W));
  const long long M = HW * B;
  const long long tiles = (M + kGruTile - 1) / kGruTile;
  if (tiles > 0x7fffffffll) throw std::runtime_error(fmt("%s: %lld workgroups exceed the grid", who, tiles));
  if (numSegments < 1 || numSegments > kGruMaxSegments)
    throw std::runtime_error(fmt("%s: num_segments must be 1..%d (got %d)", who, kGruMaxSegments, numSegments));
  if (!hidden || !segments || !segmentChannels || !weights || !biases || !out) throw std::runtime_error(fmt("%s: null array", who));
  int sum = 0;
  for (int i = 0; i < numSegments; ++i) {
    const int c = segmentChannels[i];
    if (c < kGruBlockChannels || c % kGruBlockChannels)
      throw std::runtime_error(fmt("%s: segment %d has %d channels, not a positive multiple of %d", who, i, c, kGruBlockChannels));
    if (!segments[i]) throw std::runtime_error(fmt("%s: null segment %d", who, i));
    sum += c;
  }
  if (sum != kGruInput) throw std::runtime_error(fmt("%s: the segments hold %d channels, input_dim is %d", who, sum, kGruInput));
  for (int i = 0; i < 6; ++i) {
    if (!biases[i]) throw std::runtime_error(fmt("%s: null bias %d", who, i));
    checkAligned16(who, "weight", weights[i]);
  }
  // the output is written while the neighbours of x are still being read by other workgroups
  const auto overlaps = [&](const float* a, long long channels) {
    const uintptr_t lo = reinterpret_cast<uintptr_t>(a), hi = lo + static_cast<uintptr_t>(channels) * M * sizeof(float);
    const uintptr_t olo = reinterpret_cast<uintptr_t>(out), ohi = olo + static_cast<uintptr_t>(kGruHidden) * M * sizeof(float);
    return lo < ohi && olo < hi;
  };
  if (overlaps(hidden, kGruHidden)) throw std::runtime_error(fmt("%s: out aliases h", who));
  for (int i = 0; i < numSegments; ++i)
    if (overlaps(segments[i], segmentChannels[i])) throw std::runtime_error(fmt("%s: out aliases segment %d of x", who, i));

  Frontend& fe = *h->frontend;
  const size_t plane = static_cast<size_t>(kGruHidden) * M;
  fe.dGru.ensure(3 * plane);
  float* z = fe.dGru.p;
  float* rh = z + plane;
  float* mid = rh + plane;

  GruArgs A{};
  int nb = kGruHidden / kGruBlockChannels;
  for (int i = 0; i < numSegments; ++i)
    for (int c = 0; c < segmentChannels[i]; c += kGruBlockChannels) A.blk[nb++] = GruBlock{segments[i], c, segmentChannels[i]};
  A.M = M; A.HW = static_cast<int>(HW); A.W = W;
  A.zOut = z; A.rhOut = rh; A.z = z;
  KernelTimer timer(s, kernelMs, 4);   // (measurement only: tools/raftgru_bench.py; nothing is recorded with a null kernelMs)
  timer.mark();
  for (int half = 0; half < 2; ++half) {
    const float* state = half == 0 ? hidden : mid;
    A.len = half == 0 ? W : H;
    A.stride = half == 0 ? 1 : W;
    A.vertical = half;
    A.h = state;
    for (int c = 0; c < kGruHidden / kGruBlockChannels; ++c) A.blk[c] = GruBlock{state, c * kGruBlockChannels, kGruHidden};
    A.w[0] = weights[3 * half]; A.w[1] = weights[3 * half + 1];
    A.bias[0] = biases[3 * half]; A.bias[1] = biases[3 * half + 1];
    A.out = nullptr;
    hipLaunchKernelGGL((k_gru_gemm<false>), dim3(static_cast<unsigned>(tiles), 2 * kGruHidden / kGruTile), dim3(kGruThreads), 0, s, A);
    HIP_CHECK(hipGetLastError());
    timer.mark();
    for (int c = 0; c < kGruHidden / kGruBlockChannels; ++c) A.blk[c] = GruBlock{rh, c * kGruBlockChannels, kGruHidden};
    A.w[0] = weights[3 * half + 2]; A.w[1] = nullptr;
    A.bias[0] = biases[3 * half + 2]; A.bias[1] = nullptr;
    A.out = half == 0 ? mid : out;
    hipLaunchKernelGGL((k_gru_gemm<true>), dim3(static_cast<unsigned>(tiles), kGruHidden / kGruTile), dim3(kGruThreads), 0, s, A);
    HIP_CHECK(hipGetLastError());
    timer.mark();
  }
  if (kernelMs) {
    timer.wait();
    timer.collect();
  }
}

// ---- The stock convolutions of RAFT's update block and the block itself (reference raft/core/update.py:8-16, 96-114, 133-156;
// cvd_raftconv.h).  Device arrays on the caller's stream: enqueued launches only. ------------------------------------
namespace {
template <int KS>
void launchRaftConvK(const ConvArgs& A, bool vec, dim3 grid, hipStream_t s) {
  if constexpr (KS != 7) {
    if (vec) {
      hipLaunchKernelGGL((k_raft_conv<KS, true>), grid, dim3(kConvThreads), 0, s, A);
      return;
    }
  }
  hipLaunchKernelGGL((k_raft_conv<KS, false>), grid, dim3(kConvThreads), 0, s, A);
}

// One launch.  The arguments have been checked by the callers (checkRaftConvShape and their own pointer checks).
void launchRaftConv(const ConvArgs& A, int ks, hipStream_t s) {
  const long long tiles = (A.M + kConvTile - 1) / kConvTile;
  const dim3 grid(static_cast<unsigned>(tiles), static_cast<unsigned>((A.N + kConvTile - 1) / kConvTile));
  // float4 weight loads only where every row of every tensor starts on 16 bytes
  bool vec = (static_cast<long long>(A.Cin) * ks * ks) % 4 == 0;
  for (int i = 0; i < (A.N > A.nPer ? 2 : 1); ++i) vec = vec && (reinterpret_cast<uintptr_t>(A.w[i]) & 15) == 0;
  switch (ks) {
    case 1: launchRaftConvK<1>(A, vec, grid, s); break;
    case 3: launchRaftConvK<3>(A, vec, grid, s); break;
    default: launchRaftConvK<7>(A, vec, grid, s); break;
  }
  HIP_CHECK(hipGetLastError());
}

// (M, HW) of a convolution over B x H x W pixels with the filter and the workgroup count in range
long long checkRaftConvShape(const char* who, int B, int H, int W, int ks) {
  if (B < 1 || H < 1 || W < 1) throw std::runtime_error(fmt("%s: batch, height and width must be >= 1 (got %d, %d, %d)", who, B, H, W));
  if (ks != 1 && ks != 3 && ks != 7) throw std::runtime_error(fmt("%s: kernel_size must be 1, 3 or 7 (got %d)", who, ks));
  const long long HW = static_cast<long long>(H) * W;
  if (HW > 0x7fffffffll) throw std::runtime_error(fmt("%s: %d x %d pixels per image exceed 2^31", who, H, W));
  const long long M = HW * B;
  if ((M + kConvTile - 1) / kConvTile > 0x7fffffffll) throw std::runtime_error(fmt("%s: %lld pixels exceed the grid", who, M));
  return M;
}

bool rangesOverlap(const void* a, long long aFloats, const void* b, long long bFloats) {
  const uintptr_t alo = reinterpret_cast<uintptr_t>(a), ahi = alo + static_cast<uintptr_t>(aFloats) * sizeof(float);
  const uintptr_t blo = reinterpret_cast<uintptr_t>(b), bhi = blo + static_cast<uintptr_t>(bFloats) * sizeof(float);
  return alo < bhi && blo < ahi;
}

ConvArgs raftConvArgs(int B, int H, int W) {
  ConvArgs A{};
  A.H = H; A.W = W; A.HW = H * W;
  A.M = static_cast<long long>(A.HW) * B;
  A.scale = 1.f;
  return A;
}
void raftConvInput(ConvArgs& A, const float* p, int c0, int C, int n) {
  A.seg[A.numSeg++] = ConvSegment{p, c0, C, n};
  A.Cin += n;
}
void raftConvWeights(ConvArgs& A, const float* w0, const float* b0, const float* w1, const float* b1, int nPer) {
  A.w[0] = w0; A.bias[0] = b0; A.w[1] = w1; A.bias[1] = b1;
  A.nPer = nPer;
  A.N = w1 ? 2 * nPer : nPer;
}
void raftConvOutput(ConvArgs& A, float* out, int outC, int outC0, int relu) {
  A.out = out; A.outC = outC; A.outC0 = outC0; A.relu = relu;
}
}  // namespace

void raftConv2dDevice(cvd_handle*, int B, int H, int W, int numSegments, const float* const* segments,
                      const int32_t* segmentChannels, int numWeights, const float* const* weights, const float* const* biases,
                      int inChannels, int outChannels, int kernelSize, int stride, int dilation, int groups, int relu, float scale,
                      float* out, int outTotalChannels, int outFirstChannel, hipStream_t s) {
  const char* who = "raft conv2d";
  const long long M = checkRaftConvShape(who, B, H, W, kernelSize);
  if (stride != 1) throw std::runtime_error(fmt("%s: stride must be 1 (got %d)", who, stride));
  if (dilation != 1) throw std::runtime_error(fmt("%s: dilation must be 1 (got %d)", who, dilation));
  if (groups != 1) throw std::runtime_error(fmt("%s: groups must be 1 (got %d)", who, groups));
  if (relu != 0 && relu != 1) throw std::runtime_error(fmt("%s: activation must be 0 (none) or 1 (ReLU) (got %d)", who, relu));
  if (numSegments < 1 || numSegments > kConvMaxSegments)
    throw std::runtime_error(fmt("%s: num_segments must be 1..%d (got %d)", who, kConvMaxSegments, numSegments));
  if (numWeights < 1 || numWeights > 2) throw std::runtime_error(fmt("%s: num_weights must be 1 or 2 (got %d)", who, numWeights));
  if (!segments || !segmentChannels || !weights || !biases || !out) throw std::runtime_error(fmt("%s: null array", who));
  long long sum = 0;
  for (int i = 0; i < numSegments; ++i) {
    const int c = segmentChannels[i];
    if (c < 1) throw std::runtime_error(fmt("%s: segment %d has %d channels", who, i, c));
    if (numSegments > 1 && c % kConvSegmentMultiple)
      throw std::runtime_error(fmt("%s: segment %d has %d channels, not a positive multiple of %d (several segments)", who, i, c,
                                   kConvSegmentMultiple));
    if (!segments[i]) throw std::runtime_error(fmt("%s: null segment %d", who, i));
    sum += c;
  }
  if (sum != inChannels)
    throw std::runtime_error(fmt("%s: the segments hold %lld channels, the weights' in_channels is %d", who, sum, inChannels));
  if (static_cast<long long>(inChannels) * kernelSize * kernelSize > 0x7fffffffll)
    throw std::runtime_error(fmt("%s: in_channels %d exceeds the kernel's range", who, inChannels));
  if (outChannels < 1) throw std::runtime_error(fmt("%s: out_channels must be >= 1 (got %d)", who, outChannels));
  if (numWeights == 2 && outChannels % kConvTile)
    throw std::runtime_error(fmt("%s: two stacked weight tensors need out_channels in multiples of %d (got %d)", who, kConvTile, outChannels));
  for (int i = 0; i < numWeights; ++i)
    if (!weights[i] || !biases[i]) throw std::runtime_error(fmt("%s: null weight or bias %d", who, i));
  const long long N = static_cast<long long>(outChannels) * numWeights;
  if (outFirstChannel < 0 || outTotalChannels < 1 || outFirstChannel + N > outTotalChannels)
    throw std::runtime_error(fmt("%s: the output window, channels %d .. %lld, exceeds the tensor's %d channels", who, outFirstChannel,
                                 outFirstChannel + N - 1, outTotalChannels));
  for (int i = 0; i < numSegments; ++i)
    if (rangesOverlap(out, outTotalChannels * M, segments[i], segmentChannels[i] * M))
      throw std::runtime_error(fmt("%s: out overlaps segment %d of the input", who, i));

  ConvArgs A = raftConvArgs(B, H, W);
  for (int i = 0; i < numSegments; ++i) raftConvInput(A, segments[i], 0, segmentChannels[i], segmentChannels[i]);
  raftConvWeights(A, weights[0], biases[0], numWeights == 2 ? weights[1] : nullptr, numWeights == 2 ? biases[1] : nullptr, outChannels);
  raftConvOutput(A, out, outTotalChannels, outFirstChannel, relu);
  A.scale = scale;
  launchRaftConv(A, kernelSize, s);
}

// BasicUpdateBlock.forward.  weights / biases: the 15 tensors in the order include/cvd_hip.h documents.
// kernelMs (measurement only, may be null): 12 entries, the launches in their order; with it the call waits on the host.
void raftUpdateBlockDevice(cvd_handle* h, int B, int H, int W, int corrChannels, int corPlanes, const float* net, const float* inp,
                           const float* corr, const float* flow, const float* const* weights, const float* const* biases,
                           float* netOut, float* deltaFlow, float* mask, hipStream_t s, double* kernelMs) {
  const char* who = "raft update block";
  const long long M = checkRaftConvShape(who, B, H, W, 3);
  if (corrChannels < 1) throw std::runtime_error(fmt("%s: corr_channels must be >= 1 (got %d)", who, corrChannels));
  if (corrChannels != corPlanes)
    throw std::runtime_error(fmt("%s: corr has %d channels, encoder.convc1 takes %d", who, corrChannels, corPlanes));
  if (!net || !inp || !corr || !flow || !weights || !biases || !netOut || !deltaFlow) throw std::runtime_error(fmt("%s: null array", who));
  for (int i = 0; i < 15; ++i)
    if (!weights[i] || !biases[i]) throw std::runtime_error(fmt("%s: null weight or bias %d", who, i));
  struct Span { const float* p; long long channels; const char* name; };
  const Span ins[] = {{net, 128, "net"}, {inp, 128, "inp"}, {corr, corrChannels, "corr"}, {flow, 2, "flow"}};
  const Span outs[] = {{netOut, 128, "net_out"}, {deltaFlow, 2, "delta_flow"}, {mask, 576, "mask"}};
  for (const Span& o : outs) {
    if (!o.p) continue;
    for (const Span& i : ins)
      if (rangesOverlap(o.p, o.channels * M, i.p, i.channels * M)) throw std::runtime_error(fmt("%s: %s overlaps %s", who, o.name, i.name));
    for (const Span& o2 : outs)
      if (o2.p && o2.p != o.p && rangesOverlap(o.p, o.channels * M, o2.p, o2.channels * M))
        throw std::runtime_error(fmt("%s: %s overlaps %s", who, o.name, o2.name));
  }
  for (int i = 5; i < 11; ++i) checkAligned16(who, "gru weight", weights[i]);   // (before any launch: the GRU's own check comes later)

  Frontend& fe = *h->frontend;
  const size_t m = static_cast<size_t>(M);
  fe.dBlock.ensure(768 * m);
  float* cor1 = fe.dBlock.p;               // 256 channels
  float* corFlo = cor1 + 256 * m;          // 256: convc2 -> 0..191, convf2 -> 192..255
  float* flo1 = corFlo + 256 * m;          // 128
  float* motion = flo1 + 128 * m;          // 128: conv -> 0..125, flow -> 126..127
  float* hidden = cor1;                    // 512 (256 without the mask): flow_head.conv1 | mask.0, once cor1 and cor_flo are dead
  fe.dGru.ensure(3 * 128 * m);             // (the GRU's scratch, so that its call below does not allocate between launches)

  KernelTimer enc(s, kernelMs, 5);
  enc.mark();
  {  // encoder.convc1: 1 x 1, corr -> 256, ReLU
    ConvArgs A = raftConvArgs(B, H, W);
    raftConvInput(A, corr, 0, corrChannels, corrChannels);
    raftConvWeights(A, weights[0], biases[0], nullptr, nullptr, 256);
    raftConvOutput(A, cor1, 256, 0, 1);
    launchRaftConv(A, 1, s);
    enc.mark();
  }
  {  // encoder.convc2: 3 x 3, 256 -> 192, ReLU, into cor_flo 0..191
    ConvArgs A = raftConvArgs(B, H, W);
    raftConvInput(A, cor1, 0, 256, 256);
    raftConvWeights(A, weights[1], biases[1], nullptr, nullptr, 192);
    raftConvOutput(A, corFlo, 256, 0, 1);
    launchRaftConv(A, 3, s);
    enc.mark();
  }
  {  // encoder.convf1: 7 x 7, 2 -> 128, ReLU
    ConvArgs A = raftConvArgs(B, H, W);
    raftConvInput(A, flow, 0, 2, 2);
    raftConvWeights(A, weights[2], biases[2], nullptr, nullptr, 128);
    raftConvOutput(A, flo1, 128, 0, 1);
    launchRaftConv(A, 7, s);
    enc.mark();
  }
  {  // encoder.convf2: 3 x 3, 128 -> 64, ReLU, into cor_flo 192..255
    ConvArgs A = raftConvArgs(B, H, W);
    raftConvInput(A, flo1, 0, 128, 128);
    raftConvWeights(A, weights[3], biases[3], nullptr, nullptr, 64);
    raftConvOutput(A, corFlo, 256, 192, 1);
    launchRaftConv(A, 3, s);
    enc.mark();
  }
  {  // encoder.conv: 3 x 3, 256 -> 126, ReLU, into motion_features 0..125; the same launch copies flow to 126..127
    ConvArgs A = raftConvArgs(B, H, W);
    raftConvInput(A, corFlo, 0, 256, 256);
    raftConvWeights(A, weights[4], biases[4], nullptr, nullptr, 126);
    raftConvOutput(A, motion, 128, 0, 1);
    A.copySrc = flow; A.copyC = 2; A.copyC0 = 126;
    launchRaftConv(A, 3, s);
    enc.mark();
  }
  if (kernelMs) {
    enc.wait();
    enc.collect();
  }
  {  // gru: the existing four launches, x = (inp, motion_features)
    const float* segs[2] = {inp, motion};
    const int32_t chans[2] = {128, 128};
    raftSepConvGruDevice(h, B, H, W, net, 2, segs, chans, weights + 5, biases + 5, netOut, s, kernelMs ? kernelMs + 5 : nullptr);
  }
  KernelTimer heads(s, kernelMs ? kernelMs + 9 : nullptr, 3);
  heads.mark();
  const int hiddenC = mask ? 512 : 256;
  {  // flow_head.conv1 and mask.0 stacked: 3 x 3, 128 -> 256 (+ 256), ReLU
    ConvArgs A = raftConvArgs(B, H, W);
    raftConvInput(A, netOut, 0, 128, 128);
    raftConvWeights(A, weights[11], biases[11], mask ? weights[13] : nullptr, mask ? biases[13] : nullptr, 256);
    raftConvOutput(A, hidden, hiddenC, 0, 1);
    launchRaftConv(A, 3, s);
    heads.mark();
  }
  {  // flow_head.conv2: 3 x 3, 256 -> 2
    ConvArgs A = raftConvArgs(B, H, W);
    raftConvInput(A, hidden, 0, hiddenC, 256);
    raftConvWeights(A, weights[12], biases[12], nullptr, nullptr, 2);
    raftConvOutput(A, deltaFlow, 2, 0, 0);
    launchRaftConv(A, 3, s);
    heads.mark();
  }
  if (mask) {  // mask.2: 1 x 1, 256 -> 576, x 0.25
    ConvArgs A = raftConvArgs(B, H, W);
    raftConvInput(A, hidden, 256, 512, 256);
    raftConvWeights(A, weights[14], biases[14], nullptr, nullptr, 576);
    raftConvOutput(A, mask, 576, 0, 0);
    A.scale = 0.25f;
    launchRaftConv(A, 1, s);
    heads.mark();
  }
  if (kernelMs) {
    heads.wait();
    heads.collect();
  }
}

// ---- RAFT's feature and context encoders (reference raft/core/extractor.py:8-60, 124-197; cvd_raftenc.h).  Device
// arrays on the caller's stream: enqueued launches only. ----------------------------------------------------------------------------
namespace {
template <int KS, int STRIDE>
void launchEncConvK(const EncConvArgs& A, bool vec, dim3 grid, hipStream_t s) {
  if constexpr (KS != 7) {
    if (vec) {
      hipLaunchKernelGGL((k_enc_conv<KS, STRIDE, true>), grid, dim3(kEncThreads), 0, s, A);
      return;
    }
  }
  hipLaunchKernelGGL((k_enc_conv<KS, STRIDE, false>), grid, dim3(kEncThreads), 0, s, A);
}

struct EncDims {
  int Ho, Wo;
  long long HW, HWo, M;
};

// the sizes of a convolution over B x H x W input pixels with the filter, the stride and the workgroup count in range
EncDims checkEncConvShape(const char* who, int B, int H, int W, int ks, int stride) {
  if (B < 1 || H < 1 || W < 1) throw std::runtime_error(fmt("%s: batch, height and width must be >= 1 (got %d, %d, %d)", who, B, H, W));
  if (ks != 1 && ks != 3 && ks != 7) throw std::runtime_error(fmt("%s: kernel_size must be 1, 3 or 7 (got %d)", who, ks));
  if (stride != 1 && stride != 2) throw std::runtime_error(fmt("%s: stride must be 1 or 2 (got %d)", who, stride));
  EncDims d{};
  d.HW = static_cast<long long>(H) * W;
  if (d.HW > 0x7fffffffll) throw std::runtime_error(fmt("%s: %d x %d pixels per image exceed 2^31", who, H, W));
  d.Ho = (H - 1) / stride + 1;
  d.Wo = (W - 1) / stride + 1;
  d.HWo = static_cast<long long>(d.Ho) * d.Wo;
  d.M = d.HWo * B;
  if ((d.M + kEncTile - 1) / kEncTile > 0x7fffffffll) throw std::runtime_error(fmt("%s: %lld pixels exceed the grid", who, d.M));
  return d;
}

// One launch.  The arguments have been checked by the callers.  norm: {weight, bias, running_mean, running_var} or null.
void launchEncConv(int B, int H, int W, int Cin, int N, int ks, int stride, const float* x, const float* w, const float* bias,
                   const float* const* norm, float eps, int relu, const float* residual, float* out, hipStream_t s) {
  EncConvArgs A{};
  A.x = x; A.w = w; A.bias = bias;
  if (norm) {
    A.gamma = norm[0]; A.beta = norm[1]; A.mean = norm[2]; A.var = norm[3];
  }
  A.residual = residual; A.out = out; A.eps = eps; A.relu = relu;
  A.Cin = Cin; A.N = N;
  A.H = H; A.W = W; A.HW = H * W;
  A.Ho = (H - 1) / stride + 1; A.Wo = (W - 1) / stride + 1; A.HWo = A.Ho * A.Wo;
  A.M = static_cast<long long>(A.HWo) * B;
  const dim3 grid(static_cast<unsigned>((A.M + kEncTile - 1) / kEncTile), static_cast<unsigned>((N + kEncTile - 1) / kEncTile));
  // float4 weight loads only where every row starts on 16 bytes
  const bool vec = (static_cast<long long>(Cin) * ks * ks) % 4 == 0 && (reinterpret_cast<uintptr_t>(w) & 15) == 0;
  switch (ks * 10 + stride) {
    case 11: launchEncConvK<1, 1>(A, vec, grid, s); break;
    case 12: launchEncConvK<1, 2>(A, vec, grid, s); break;
    case 31: launchEncConvK<3, 1>(A, vec, grid, s); break;
    case 32: launchEncConvK<3, 2>(A, vec, grid, s); break;
    case 71: launchEncConvK<7, 1>(A, vec, grid, s); break;
    default: launchEncConvK<7, 2>(A, vec, grid, s); break;
  }
  HIP_CHECK(hipGetLastError());
}

// The two launches of the instance norm over `planes` planes of HW elements; stats: 2 planes doubles.  Checked by the callers.
// mark (may be empty) is called after each launch.
template <class Mark>
void launchInstanceNorm(long long planes, int HW, const float* x, double eps, int relu, const float* residual, float* out, double* stats,
                        hipStream_t s, Mark&& mark) {
  InstNormArgs A{};
  A.x = x; A.residual = residual; A.out = out; A.stats = stats; A.eps = eps; A.relu = relu; A.HW = HW;
  A.total = planes * HW;
  hipLaunchKernelGGL(k_instnorm_stats, dim3(static_cast<unsigned>(planes)), dim3(kNormThreads), 0, s, A);
  HIP_CHECK(hipGetLastError());
  mark();
  hipLaunchKernelGGL(k_instnorm_apply, dim3(static_cast<unsigned>((A.total + kNormThreads - 1) / kNormThreads)), dim3(kNormThreads), 0, s, A);
  HIP_CHECK(hipGetLastError());
  mark();
}

void checkNormSize(const char* who, long long planes, long long HW) {
  if (HW < 2) throw std::runtime_error(fmt("%s: planes of %lld element: instance norm expects more than 1 spatial element", who, HW));
  if (planes > 0x7fffffffll || (planes * HW + kNormThreads - 1) / kNormThreads > 0x7fffffffll)
    throw std::runtime_error(fmt("%s: %lld planes of %lld elements exceed the grid", who, planes, HW));
}
}  // namespace

void raftEncoderConvDevice(cvd_handle*, int B, int H, int W, int inChannels, int outChannels, int kernelSize, int stride,
                           const float* x, const float* weight, const float* bias, const float* const* norm, float eps, int relu,
                           const float* residual, float* out, hipStream_t s) {
  const char* who = "raft encoder conv";
  const EncDims d = checkEncConvShape(who, B, H, W, kernelSize, stride);
  if (inChannels < 1) throw std::runtime_error(fmt("%s: in_channels must be >= 1 (got %d)", who, inChannels));
  if (outChannels < 1) throw std::runtime_error(fmt("%s: out_channels must be >= 1 (got %d)", who, outChannels));
  if (static_cast<long long>(inChannels) * kernelSize * kernelSize > 0x7fffffffll)
    throw std::runtime_error(fmt("%s: in_channels %d exceeds the kernel's range", who, inChannels));
  if (relu != 0 && relu != 1) throw std::runtime_error(fmt("%s: relu must be 0 or 1 (got %d)", who, relu));
  if (!x || !weight || !bias || !out) throw std::runtime_error(fmt("%s: null array", who));
  if (norm) {
    for (int i = 0; i < 4; ++i)
      if (!norm[i]) throw std::runtime_error(fmt("%s: null norm vector %d", who, i));
    if (!(eps > 0.f)) throw std::runtime_error(fmt("%s: eps must be > 0 (got %g)", who, static_cast<double>(eps)));
  }
  const long long outFloats = d.M * outChannels;
  if (rangesOverlap(out, outFloats, x, d.HW * B * inChannels)) throw std::runtime_error(fmt("%s: out overlaps x", who));
  if (residual && rangesOverlap(out, outFloats, residual, outFloats)) throw std::runtime_error(fmt("%s: out overlaps the residual", who));
  launchEncConv(B, H, W, inChannels, outChannels, kernelSize, stride, x, weight, bias, norm, eps, relu, residual, out, s);
}

void raftInstanceNormDevice(cvd_handle* h, int B, int channels, int H, int W, const float* x, float eps, int relu,
                            const float* residual, float* out, hipStream_t s) {
  const char* who = "raft instance norm";
  if (B < 1 || channels < 1 || H < 1 || W < 1)
    throw std::runtime_error(fmt("%s: batch, channels, height and width must be >= 1 (got %d, %d, %d, %d)", who, B, channels, H, W));
  const long long HW = static_cast<long long>(H) * W;
  if (HW > 0x7fffffffll) throw std::runtime_error(fmt("%s: %d x %d pixels per image exceed 2^31", who, H, W));
  const long long planes = static_cast<long long>(B) * channels;
  checkNormSize(who, planes, HW);
  if (relu != 0 && relu != 1) throw std::runtime_error(fmt("%s: relu must be 0 or 1 (got %d)", who, relu));
  if (!(eps > 0.f)) throw std::runtime_error(fmt("%s: eps must be > 0 (got %g)", who, static_cast<double>(eps)));
  if (!x || !out) throw std::runtime_error(fmt("%s: null array", who));
  const long long n = planes * HW;
  if (out != x && rangesOverlap(out, n, x, n)) throw std::runtime_error(fmt("%s: out overlaps x (only out == x, in place, is allowed)", who));
  if (residual && rangesOverlap(out, n, residual, n)) throw std::runtime_error(fmt("%s: out overlaps the residual", who));
  Frontend& fe = *h->frontend;
  fe.dEncStats.ensure(2 * static_cast<size_t>(planes));
  launchInstanceNorm(planes, static_cast<int>(HW), x, static_cast<double>(eps), relu, residual, out, fe.dEncStats.p, s, [] {});
}

// BasicEncoder.forward.  weights / biases / norms: the tables include/cvd_hip.h documents.
// kernelMs (measurement only, may be null): 48 entries; with it the call waits on the host.
void raftEncoderDevice(cvd_handle* h, int B, int H, int W, int outputDim, int normMode, float eps, const float* images,
                       const float* const* weights, const float* const* biases, const float* const* norms, float* out,
                       hipStream_t s, double* kernelMs) {
  const char* who = "raft encoder";
  checkEncConvShape(who, B, H, W, 7, 2);
  if (outputDim < 1) throw std::runtime_error(fmt("%s: output_dim must be >= 1 (got %d)", who, outputDim));
  if (normMode < 0 || normMode > 2) throw std::runtime_error(fmt("%s: norm_mode must be 0 (none), 1 (instance) or 2 (batch) (got %d)", who, normMode));
  if (normMode != 0 && !(eps > 0.f)) throw std::runtime_error(fmt("%s: eps must be > 0 (got %g)", who, static_cast<double>(eps)));
  if (!images || !weights || !biases || !out || (normMode == 2 && !norms)) throw std::runtime_error(fmt("%s: null array", who));
  for (int i = 0; i < 16; ++i)
    if (!weights[i] || !biases[i]) throw std::runtime_error(fmt("%s: null weight or bias %d", who, i));
  if (normMode == 2)
    for (int i = 0; i < 60; ++i)
      if (!norms[i]) throw std::runtime_error(fmt("%s: null norm vector %d", who, i));
  const int H1 = (H - 1) / 2 + 1, W1 = (W - 1) / 2 + 1, H2 = (H1 - 1) / 2 + 1, W2 = (W1 - 1) / 2 + 1, H3 = (H2 - 1) / 2 + 1,
            W3 = (W2 - 1) / 2 + 1;
  const size_t b = static_cast<size_t>(B);
  const size_t m1 = b * H1 * W1, m2 = b * H2 * W2, m3 = b * H3 * W3;
  if (normMode == 1) checkNormSize(who, static_cast<long long>(B) * 128, static_cast<long long>(H3) * W3);
  if (rangesOverlap(out, static_cast<long long>(m3) * outputDim, images, static_cast<long long>(b) * 3 * H * W))
    throw std::runtime_error(fmt("%s: out overlaps the images", who));

  // three rotating tensors (a block's input, its middle, its output) and the downsample branch's
  Frontend& fe = *h->frontend;
  const size_t big = std::max(64 * m1, std::max(96 * m2, 128 * m3)), small = std::max(96 * m2, 128 * m3);
  fe.dEnc.ensure(3 * big + small);
  fe.dEncStats.ensure(2 * b * 128);
  float* bufA = fe.dEnc.p;
  float* bufB = bufA + big;
  float* bufC = bufB + big;
  float* bufD = bufC + big;

  constexpr int kLaunchesMost = 46;
  double phaseMs[kLaunchesMost];
  int slot[kLaunchesMost];
  int launches = 0;
  KernelTimer timer(s, kernelMs ? phaseMs : nullptr, kLaunchesMost);
  timer.mark();
  // convolution `idx` with its norm, ReLU and residual; under instance norm the norm is the two launches behind it, in place
  const auto conv = [&](int idx, const float* x, int Cin, int Hin, int Win, int N, int ks, int stride, int relu, const float* residual,
                        float* y) {
    const bool normed = idx < 15;
    const int Ho = (Hin - 1) / stride + 1, Wo = (Win - 1) / stride + 1;
    if (normMode == 1 && normed) {
      launchEncConv(B, Hin, Win, Cin, N, ks, stride, x, weights[idx], biases[idx], nullptr, eps, 0, nullptr, y, s);
      slot[launches++] = 3 * idx;
      timer.mark();
      int part = 1;
      launchInstanceNorm(static_cast<long long>(B) * N, Ho * Wo, y, static_cast<double>(eps), relu, residual, y, fe.dEncStats.p, s, [&] {
        slot[launches++] = 3 * idx + part++;
        timer.mark();
      });
    } else {
      launchEncConv(B, Hin, Win, Cin, N, ks, stride, x, weights[idx], biases[idx], normMode == 2 && normed ? norms + 4 * idx : nullptr,
                    eps, relu, residual, y, s);
      slot[launches++] = 3 * idx;
      timer.mark();
    }
  };
  // a ResidualBlock: conv1 = idx, conv2 = idx + 1, downsample.0 = idx + 2 (stride 2 only)
  const auto block = [&](int idx, const float* x, int Cin, int Hin, int Win, int N, int stride, float* mid, float* y) {
    const int Ho = (Hin - 1) / stride + 1, Wo = (Win - 1) / stride + 1;
    conv(idx, x, Cin, Hin, Win, N, 3, stride, 1, nullptr, mid);
    const float* residual = x;
    if (stride != 1) {
      conv(idx + 2, x, Cin, Hin, Win, N, 1, stride, 0, nullptr, bufD);
      residual = bufD;
    }
    conv(idx + 1, mid, N, Ho, Wo, N, 3, 1, 1, residual, y);
  };
  conv(0, images, 3, H, W, 64, 7, 2, 1, nullptr, bufA);
  block(1, bufA, 64, H1, W1, 64, 1, bufB, bufC);
  block(3, bufC, 64, H1, W1, 64, 1, bufB, bufA);
  block(5, bufA, 64, H1, W1, 96, 2, bufB, bufC);
  block(8, bufC, 96, H2, W2, 96, 1, bufB, bufA);
  block(10, bufA, 96, H2, W2, 128, 2, bufB, bufC);
  block(13, bufC, 128, H3, W3, 128, 1, bufB, bufA);
  conv(15, bufA, 128, H3, W3, outputDim, 1, 1, 0, nullptr, out);
  if (kernelMs) {
    timer.wait();
    timer.collect();
    std::fill(kernelMs, kernelMs + 48, 0.0);
    for (int i = 0; i < launches; ++i) kernelMs[slot[i]] = phaseMs[i];
  }
}

// ---- The decoder of MiDaS v2.1 (reference monodepth/midas_v2/midas_net.py:57-74, blocks.py:41-159; cvd_midas.h).
// Device arrays on the caller's stream: enqueued launches only. ---------------------------------------------------------------------
namespace {
struct MidasDims {
  long long HW, M;
};

MidasDims checkMidasShape(const char* who, int B, int H, int W) {
  if (B < 1 || H < 1 || W < 1) throw std::runtime_error(fmt("%s: batch, height and width must be >= 1 (got %d, %d, %d)", who, B, H, W));
  MidasDims d{};
  d.HW = static_cast<long long>(H) * W;
  if (d.HW > 0x7fffffffll) throw std::runtime_error(fmt("%s: %d x %d pixels per image exceed 2^31", who, H, W));
  d.M = d.HW * B;
  if ((d.M + kMidasTile - 1) / kMidasTile > 0x7fffffffll) throw std::runtime_error(fmt("%s: %lld pixels exceed the grid", who, d.M));
  return d;
}

void checkMidasChannels(const char* who, int Cin, int N, int ks, long long M) {
  if (ks != 1 && ks != 3) throw std::runtime_error(fmt("%s: kernel_size must be 1 or 3 (got %d)", who, ks));
  if (Cin < 1) throw std::runtime_error(fmt("%s: in_channels must be >= 1 (got %d)", who, Cin));
  if (N < 1) throw std::runtime_error(fmt("%s: out_channels must be >= 1 (got %d)", who, N));
  if (static_cast<long long>(Cin) * ks * ks > 0x7fffffffll) throw std::runtime_error(fmt("%s: in_channels %d exceeds the kernel's range", who, Cin));
  if ((N + kMidasTile - 1) / kMidasTile > 65535) throw std::runtime_error(fmt("%s: out_channels %d exceeds the grid", who, N));
  if ((M * N + kMidasThreads - 1) / kMidasThreads > 0x7fffffffll)
    throw std::runtime_error(fmt("%s: %lld pixels of %d channels exceed the grid", who, M, N));
}

int midasChunks(int Cin, int ks) {
  const int cc = ks == 1 ? MidasShape<1>::kChunkChannels : MidasShape<3>::kChunkChannels;
  return (Cin + cc - 1) / cc;
}

// the split the convolution runs with: `forced` >= 1 as given (checked by the caller), 0 = the rule
int midasSplitFor(int Cin, int ks, long long HW, int forced) {
  return forced > 0 ? forced : midasSplit(static_cast<long long>(Cin) * ks * ks, HW, ks);
}

// floats of split scratch a convolution needs (0 without a split)
size_t midasSplitFloats(int S, long long M, int N) { return S > 1 ? static_cast<size_t>(S) * static_cast<size_t>(M) * N : 0; }

// One convolution: one launch, with S > 1 the fold behind it.  Checked by the callers; `partial` holds midasSplitFloats floats.
// mark (may be empty) is called after each launch; returns the launches (1 or 2).
template <class Mark>
int launchMidasConv(int B, int H, int W, int Cin, int N, int ks, const float* x, const float* w, const float* bias, int reluIn, int relu,
                    const float* a, int reluA, const float* b, int S, float* partial, float* out, hipStream_t s, Mark&& mark) {
  MidasConvArgs A{};
  A.x = x; A.w = w; A.bias = bias; A.a = a; A.b = b; A.out = out; A.partial = partial;
  A.reluIn = reluIn; A.relu = relu; A.reluA = reluA;
  A.Cin = Cin; A.N = N; A.H = H; A.W = W; A.HW = H * W;
  A.M = static_cast<long long>(A.HW) * B;
  const int fold = ks == 1 ? MidasShape<1>::kFold : MidasShape<3>::kFold;
  const int chunks = midasChunks(Cin, ks), chains = (chunks + fold - 1) / fold;
  const int per = (chains + S - 1) / S;                   // chains per slice
  A.S = (chains + per - 1) / per;                         // (the rule's S already has this form; a forced one may shrink)
  A.chunksPerSlice = per * fold;
  const dim3 grid(static_cast<unsigned>((A.M + kMidasTile - 1) / kMidasTile), static_cast<unsigned>((N + kMidasTile - 1) / kMidasTile),
                  static_cast<unsigned>(A.S));
  // float4 weight loads only where every row starts on 16 bytes
  const bool vec = (static_cast<long long>(Cin) * ks * ks) % 4 == 0 && (reinterpret_cast<uintptr_t>(w) & 15) == 0;
  if (ks == 1) {
    if (vec) hipLaunchKernelGGL((k_midas_conv<1, true, false>), grid, dim3(kMidasThreads), 0, s, A);
    else hipLaunchKernelGGL((k_midas_conv<1, false, false>), grid, dim3(kMidasThreads), 0, s, A);
  } else {
    if (vec) hipLaunchKernelGGL((k_midas_conv<3, true, false>), grid, dim3(kMidasThreads), 0, s, A);
    else hipLaunchKernelGGL((k_midas_conv<3, false, false>), grid, dim3(kMidasThreads), 0, s, A);
  }
  HIP_CHECK(hipGetLastError());
  mark();
  if (A.S == 1) return 1;
  hipLaunchKernelGGL(k_midas_fold, dim3(static_cast<unsigned>((A.M * N + kMidasThreads - 1) / kMidasThreads)), dim3(kMidasThreads), 0, s, A);
  HIP_CHECK(hipGetLastError());
  mark();
  return 2;
}

void launchMidasUpsample(long long planes, int H, int W, int align, const float* x, float* out, hipStream_t s) {
  MidasUpsampleArgs A{};
  A.x = x; A.out = out; A.H = H; A.W = W;
  A.total = planes * 4 * H * W;
  const dim3 grid(static_cast<unsigned>((A.total + kMidasThreads - 1) / kMidasThreads));
  if (align) hipLaunchKernelGGL((k_midas_upsample2x<true>), grid, dim3(kMidasThreads), 0, s, A);
  else hipLaunchKernelGGL((k_midas_upsample2x<false>), grid, dim3(kMidasThreads), 0, s, A);
  HIP_CHECK(hipGetLastError());
}

void checkMidasUpsampleSize(const char* who, long long planes, int H, int W) {
  const long long HW = static_cast<long long>(H) * W;
  if (HW > 0x7fffffffll / 4) throw std::runtime_error(fmt("%s: %d x %d output pixels per plane exceed 2^31", who, 2 * H, 2 * W));
  if (planes > 0x7fffffffll || (planes * 4 * HW + kMidasThreads - 1) / kMidasThreads > 0x7fffffffll)
    throw std::runtime_error(fmt("%s: %lld planes of %lld elements exceed the grid", who, planes, 4 * HW));
}

void launchMidasHead(int B, int H, int W, int Cin, const float* x, const float* w2, const float* b2, const float* w4, const float* b4,
                     int nonNegative, float* out, hipStream_t s) {
  MidasConvArgs A{};
  A.x = x; A.w = w2; A.bias = b2; A.w4 = w4; A.b4 = b4; A.out = out;
  A.nonNegative = nonNegative;
  A.Cin = Cin; A.N = kMidasHeadMid; A.H = H; A.W = W; A.HW = H * W;
  A.M = static_cast<long long>(A.HW) * B;
  A.S = 1;
  A.chunksPerSlice = midasChunks(Cin, 3);
  const dim3 grid(static_cast<unsigned>((A.M + kMidasHeadPixels - 1) / kMidasHeadPixels));
  const bool vec = (static_cast<long long>(Cin) * 9) % 4 == 0 && (reinterpret_cast<uintptr_t>(w2) & 15) == 0;
  if (vec) hipLaunchKernelGGL((k_midas_conv<3, true, true>), grid, dim3(kMidasThreads), 0, s, A);
  else hipLaunchKernelGGL((k_midas_conv<3, false, true>), grid, dim3(kMidasThreads), 0, s, A);
  HIP_CHECK(hipGetLastError());
}

void checkFlag(const char* who, const char* name, int v) {
  if (v != 0 && v != 1) throw std::runtime_error(fmt("%s: %s must be 0 or 1 (got %d)", who, name, v));
}
}  // namespace

void midasConvDevice(cvd_handle* h, int B, int H, int W, int inChannels, int outChannels, int kernelSize, const float* x,
                     const float* weight, const float* bias, int reluIn, int relu, const float* a, int reluA, const float* b, int split,
                     float* out, hipStream_t s) {
  const char* who = "midas conv";
  const MidasDims d = checkMidasShape(who, B, H, W);
  checkMidasChannels(who, inChannels, outChannels, kernelSize, d.M);
  checkFlag(who, "relu_in", reluIn);
  checkFlag(who, "relu", relu);
  checkFlag(who, "relu_a", reluA);
  const int chunks = midasChunks(inChannels, kernelSize);
  if (split < 0 || split > chunks)
    throw std::runtime_error(fmt("%s: split must be 0 (the rule) or 1 .. %d, the chunks of K (got %d)", who, chunks, split));
  if (!x || !weight || !out) throw std::runtime_error(fmt("%s: null array", who));
  const long long outFloats = d.M * outChannels;
  if (rangesOverlap(out, outFloats, x, d.M * inChannels)) throw std::runtime_error(fmt("%s: out overlaps x", who));
  if (a && rangesOverlap(out, outFloats, a, outFloats)) throw std::runtime_error(fmt("%s: out overlaps the addend a", who));
  if (b && rangesOverlap(out, outFloats, b, outFloats)) throw std::runtime_error(fmt("%s: out overlaps the addend b", who));
  const int S = midasSplitFor(inChannels, kernelSize, d.HW, split);
  Frontend& fe = *h->frontend;
  fe.dMidasSplit.ensure(midasSplitFloats(S, d.M, outChannels));
  launchMidasConv(B, H, W, inChannels, outChannels, kernelSize, x, weight, bias, reluIn, relu, a, reluA, b, S, fe.dMidasSplit.p, out, s,
                  [] {});
}

void midasUpsample2xDevice(cvd_handle*, int B, int channels, int H, int W, int alignCorners, const float* x, float* out, hipStream_t s) {
  const char* who = "midas upsample2x";
  if (B < 1 || channels < 1 || H < 1 || W < 1)
    throw std::runtime_error(fmt("%s: batch, channels, height and width must be >= 1 (got %d, %d, %d, %d)", who, B, channels, H, W));
  checkFlag(who, "align_corners", alignCorners);
  const long long planes = static_cast<long long>(B) * channels;
  checkMidasUpsampleSize(who, planes, H, W);
  if (!x || !out) throw std::runtime_error(fmt("%s: null array", who));
  const long long n = planes * H * W;
  if (rangesOverlap(out, 4 * n, x, n)) throw std::runtime_error(fmt("%s: out overlaps x", who));
  launchMidasUpsample(planes, H, W, alignCorners, x, out, s);
}

void midasHeadDevice(cvd_handle*, int B, int H, int W, int inChannels, int midChannels, const float* x, const float* weight2,
                     const float* bias2, const float* weight4, const float* bias4, int nonNegative, float* out, hipStream_t s) {
  const char* who = "midas head";
  const MidasDims d = checkMidasShape(who, B, H, W);
  if ((d.M + kMidasHeadPixels - 1) / kMidasHeadPixels > 0x7fffffffll) throw std::runtime_error(fmt("%s: %lld pixels exceed the grid", who, d.M));
  if (inChannels < 1) throw std::runtime_error(fmt("%s: in_channels must be >= 1 (got %d)", who, inChannels));
  if (static_cast<long long>(inChannels) * 9 > 0x7fffffffll) throw std::runtime_error(fmt("%s: in_channels %d exceeds the kernel's range", who, inChannels));
  if (midChannels != kMidasHeadMid) throw std::runtime_error(fmt("%s: mid_channels must be %d (got %d)", who, kMidasHeadMid, midChannels));
  checkFlag(who, "non_negative", nonNegative);
  if (!x || !weight2 || !bias2 || !weight4 || !bias4 || !out) throw std::runtime_error(fmt("%s: null array", who));
  if (rangesOverlap(out, d.M, x, d.M * inChannels)) throw std::runtime_error(fmt("%s: out overlaps x", who));
  launchMidasHead(B, H, W, inChannels, x, weight2, bias2, weight4, bias4, nonNegative, out, s);
}

// MidasNet.forward behind the backbone.  channels / heights / widths: of the four feature maps, layer 1 first.
// weights (21) / biases (17): the tables include/cvd_hip.h documents.  kernelMs (measurement only, may be null): 44 entries; with it the
// call waits on the host.
void midasDecoderDevice(cvd_handle* h, int B, int features, const int* channels, const int* heights, const int* widths,
                        const float* const* maps, const float* const* weights, const float* const* biases, int nonNegative, float* out,
                        hipStream_t s, double* kernelMs, float* const* saved) {
  const char* who = saved ? "midas decoder train" : "midas decoder";
  if (!channels || !heights || !widths || !maps || !weights || !biases || !out) throw std::runtime_error(fmt("%s: null array", who));
  if (features < 1) throw std::runtime_error(fmt("%s: features must be >= 1 (got %d)", who, features));
  checkFlag(who, "non_negative", nonNegative);
  long long M[4];
  for (int k = 0; k < 4; ++k) {
    const MidasDims d = checkMidasShape(who, B, heights[k], widths[k]);
    M[k] = d.M;
    if (channels[k] < 1) throw std::runtime_error(fmt("%s: channels of feature map %d must be >= 1 (got %d)", who, k + 1, channels[k]));
    checkMidasChannels(who, channels[k], features, 3, d.M);
    if (k > 0 && (heights[k - 1] != 2 * heights[k] || widths[k - 1] != 2 * widths[k]))
      throw std::runtime_error(fmt("%s: feature map %d is %d x %d, not twice map %d's %d x %d", who, k, heights[k - 1], widths[k - 1], k + 1,
                                   heights[k], widths[k]));
    if (!maps[k]) throw std::runtime_error(fmt("%s: null feature map %d", who, k + 1));
  }
  const int H1 = heights[0], W1 = widths[0];
  if (static_cast<long long>(H1) * W1 > 0x7fffffffll / 16)
    throw std::runtime_error(fmt("%s: %d x %d output pixels per image exceed 2^31", who, 4 * H1, 4 * W1));
  const long long Mout = 16 * M[0];
  checkMidasShape(who, B, 4 * H1, 4 * W1);
  checkMidasChannels(who, features, std::max(features, 128), 3, 4 * M[0]);
  checkMidasUpsampleSize(who, static_cast<long long>(B) * std::max(features, 128), 2 * H1, 2 * W1);
  for (int i = 0; i < 21; ++i)
    if (!weights[i]) throw std::runtime_error(fmt("%s: null weight %d", who, i));
  for (int i = 0; i < 17; ++i)
    if (!biases[i]) throw std::runtime_error(fmt("%s: null bias %d", who, i));
  for (int k = 0; k < 4; ++k)
    if (rangesOverlap(out, Mout, maps[k], M[k] * channels[k])) throw std::runtime_error(fmt("%s: out overlaps feature map %d", who, k + 1));

  // scratch: the four layerK_rn outputs, three rotating tensors of the largest level, the path (up to features channels at twice
  // level 1), output_conv.0's result and its upsampling; and the split convolutions' partial sums
  const size_t F = static_cast<size_t>(features);
  size_t n[4], off[4], total = 0, split = 0;
  for (int k = 0; k < 4; ++k) {
    n[k] = F * static_cast<size_t>(M[k]);
    off[k] = total;
    total += n[k];
    const long long HW = static_cast<long long>(heights[k]) * widths[k];
    split = std::max(split, midasSplitFloats(midasSplitFor(channels[k], 3, HW, 0), M[k], features));
    split = std::max(split, midasSplitFloats(midasSplitFor(features, 3, HW, 0), M[k], features));
  }
  split = std::max(split, midasSplitFloats(midasSplitFor(features, 3, 4ll * H1 * W1, 0), 4 * M[0], 128));
  const size_t oT = total, oP = oT + 3 * n[0], oH0 = oP + 4 * n[0], oH1 = oH0 + 128 * 4 * static_cast<size_t>(M[0]);
  total = oH1 + 128 * static_cast<size_t>(Mout);
  Frontend& fe = *h->frontend;
  fe.dMidas.ensure(total);
  fe.dMidasSplit.ensure(split);
  float* base = fe.dMidas.p;
  float* L[4] = {base + off[0], base + off[1], base + off[2], base + off[3]};
  float* T0 = base + oT;
  float* T1 = T0 + n[0];
  float* T2 = T1 + n[0];
  float* P = base + oP;
  float* H0 = base + oH0;
  float* Hup = base + oH1;
  // Training: the activations the backward reads go to the caller's table (kMidasSaved tensors, the order of midasSavedIndex) and not
  // to scratch; the launches and their arguments' values are the same, so the output is the same bits.
  float *tU1[4] = {T0, T0, T0, T0}, *sumO[4] = {T1, T1, T1, T1}, *tU2[4] = {T0, T0, T0, T0};
  float* P0 = P;
  if (saved) {
    for (int i = 0; i < kMidasSaved; ++i)
      if (!saved[i]) throw std::runtime_error(fmt("%s: null saved tensor %d", who, i));
    const size_t big = 128 * 4 * static_cast<size_t>(M[0]);
    for (int i = 0; i < kMidasSaved; ++i) {
      const int lvl = i < 4 ? i : i == 4 ? 3 : i < 14 ? 2 - (i - 5) / 3 : 0;
      const size_t count = i == 14 ? 4 * n[0] : i == 15 ? big : n[lvl];
      if (rangesOverlap(out, Mout, saved[i], static_cast<long long>(count))) throw std::runtime_error(fmt("%s: out overlaps saved tensor %d", who, i));
      for (int k = 0; k < 4; ++k)
        if (rangesOverlap(saved[i], static_cast<long long>(count), maps[k], M[k] * channels[k]))
          throw std::runtime_error(fmt("%s: saved tensor %d overlaps feature map %d", who, i, k + 1));
    }
    for (int k = 0; k < 4; ++k) L[k] = saved[k];
    tU2[3] = saved[4];
    for (int k = 2; k >= 0; --k) {
      const int at = 5 + 3 * (2 - k);
      tU1[k] = saved[at]; sumO[k] = saved[at + 1]; tU2[k] = saved[at + 2];
    }
    P0 = saved[14];
    H0 = saved[15];
  }

  constexpr int kSlots = 44;
  double phaseMs[kSlots];
  int slot[kSlots];
  int launches = 0;
  KernelTimer timer(s, kernelMs ? phaseMs : nullptr, kSlots);
  timer.mark();
  // convolution `idx` of the weight table (bias idx - 4, none for the first four): slot 2 idx, its fold 2 idx + 1
  const auto conv = [&](int idx, int k, const float* x, int Cin, int N, int reluIn, const float* a, const float* b, float* y) {
    int part = 0;
    const long long HW = static_cast<long long>(heights[k]) * widths[k];
    launchMidasConv(B, heights[k], widths[k], Cin, N, 3, x, weights[idx], idx < 4 ? nullptr : biases[idx - 4], reluIn, 0, a, 1, b,
                    midasSplitFor(Cin, 3, HW, 0), fe.dMidasSplit.p, y, s, [&] {
                      slot[launches++] = 2 * idx + part++;
                      timer.mark();
                    });
  };
  const auto upsample = [&](int which, long long planes, int H, int W, int align, const float* x, float* y) {
    launchMidasUpsample(planes, H, W, align, x, y, s);
    slot[launches++] = 38 + which;
    timer.mark();
  };
  for (int k = 0; k < 4; ++k) conv(k, k, maps[k], channels[k], features, 0, nullptr, nullptr, L[k]);
  // refinenet4 .. refinenet1: FeatureFusionBlock.forward with the in-place ReLU of its units (blocks.py:66-75, 94-111)
  for (int k = 3; k >= 0; --k) {
    const int w0 = k == 3 ? 4 : 6 + 4 * (2 - k);         // the block's first weight: rn4 has resConfUnit2 only
    const float* o = L[k];
    if (k < 3) {
      conv(w0, k, L[k], features, features, 1, nullptr, nullptr, tU1[k]);       // resConfUnit1.conv1(relu(x1))
      conv(w0 + 1, k, tU1[k], features, features, 1, L[k], P, sumO[k]);         // path + (conv2(relu(.)) + relu(x1))
      o = sumO[k];
    }
    const int u2 = k == 3 ? w0 : w0 + 2;
    conv(u2, k, o, features, features, 1, nullptr, nullptr, tU2[k]);            // resConfUnit2.conv1(relu(o))
    conv(u2 + 1, k, tU2[k], features, features, 1, o, nullptr, T2);             // conv2(relu(.)) + relu(o)
    upsample(3 - k, static_cast<long long>(B) * features, heights[k], widths[k], 1, T2, k == 0 ? P0 : P);
  }
  // output_conv: 0 (features -> 128 at twice level 1), Interpolate, then 2, ReLU, 4 and the last ReLU in the head's launch
  {
    int part = 0;
    launchMidasConv(B, 2 * H1, 2 * W1, features, 128, 3, P0, weights[18], biases[14], 0, 0, nullptr, 0, nullptr,
                    midasSplitFor(features, 3, 4ll * H1 * W1, 0), fe.dMidasSplit.p, H0, s, [&] {
                      slot[launches++] = 36 + part++;
                      timer.mark();
                    });
  }
  upsample(4, static_cast<long long>(B) * 128, 2 * H1, 2 * W1, 0, H0, Hup);
  launchMidasHead(B, 4 * H1, 4 * W1, 128, Hup, weights[19], biases[15], weights[20], biases[16], nonNegative, out, s);
  slot[launches++] = 43;
  timer.mark();
  if (kernelMs) {
    timer.wait();
    timer.collect();
    std::fill(kernelMs, kernelMs + kSlots, 0.0);
    for (int i = 0; i < launches; ++i) kernelMs[slot[i]] = phaseMs[i];
  }
}

// ---- Backward of the decoder's layers (cvd_midas_grad.h): the gradients of nn.Conv2d(stride 1, padding k / 2) as the
// reference's blocks.py:41-159 and midas_net.py:31-74 use it, and of the bilinear x 2 interpolate.  Device arrays on the caller's
// stream: enqueued launches only. ---------------------------------------------------------------------------------------------------
// gx = conv(gy, W') on the forward's k_midas_conv, W' the flipped, transposed filter: the forward's split rule (from K = N KS KS and
// the pixels of one image), chains and f64 fold hold as they stand.  With an addend, a mask or a split the convolution writes its
// raw sums as partial sums (its S > 1 path, also for one slice) and k_midas_dgrad_fold applies the epilogue.
void midasConvGradInputDevice(cvd_handle* h, int B, int H, int W, int inChannels, int outChannels, int kernelSize, const float* gy,
                              const float* weight, const float* add, const float* mask, int split, float* gx, hipStream_t s) {
  const char* who = "midas conv grad input";
  const MidasDims d = checkMidasShape(who, B, H, W);
  checkMidasChannels(who, inChannels, outChannels, kernelSize, d.M);
  checkMidasChannels(who, outChannels, inChannels, kernelSize, d.M);           // the convolution that runs: N -> Cin
  const int chunks = midasChunks(outChannels, kernelSize);
  if (split < 0 || split > chunks)
    throw std::runtime_error(fmt("%s: split must be 0 (the rule) or 1 .. %d, the chunks of K (got %d)", who, chunks, split));
  if (!gy || !weight || !gx) throw std::runtime_error(fmt("%s: null array", who));
  const long long outFloats = d.M * inChannels;
  const int T = kernelSize * kernelSize;
  if (rangesOverlap(gx, outFloats, gy, d.M * outChannels)) throw std::runtime_error(fmt("%s: gx overlaps gy", who));
  if (rangesOverlap(gx, outFloats, weight, static_cast<long long>(inChannels) * outChannels * T))
    throw std::runtime_error(fmt("%s: gx overlaps the weight", who));
  if (add && rangesOverlap(gx, outFloats, add, outFloats)) throw std::runtime_error(fmt("%s: gx overlaps the addend", who));
  if (mask && rangesOverlap(gx, outFloats, mask, outFloats)) throw std::runtime_error(fmt("%s: gx overlaps the mask", who));
  const int fold = kernelSize == 1 ? MidasShape<1>::kFold : MidasShape<3>::kFold;
  const int chains = (chunks + fold - 1) / fold;
  const int want = midasSplitFor(outChannels, kernelSize, d.HW, split);
  const int per = (chains + want - 1) / want;
  const int S = (chains + per - 1) / per;                  // (a forced split may shrink: slices are whole chains)
  const bool folded = S > 1 || add || mask;
  Frontend& fe = *h->frontend;
  const size_t wFloats = static_cast<size_t>(inChannels) * outChannels * T;
  fe.dMidasGradW.ensure(wFloats);
  if (folded) fe.dMidasSplit.ensure(static_cast<size_t>(S) * static_cast<size_t>(outFloats));

  MidasFlipArgs F{};
  F.w = weight; F.out = fe.dMidasGradW.p; F.N = outChannels; F.Cin = inChannels; F.total = static_cast<long long>(wFloats);
  const dim3 flipGrid(static_cast<unsigned>((F.total + kMgThreads - 1) / kMgThreads));
  if (kernelSize == 1) hipLaunchKernelGGL(k_midas_wflip<1>, flipGrid, dim3(kMgThreads), 0, s, F);
  else hipLaunchKernelGGL(k_midas_wflip<3>, flipGrid, dim3(kMgThreads), 0, s, F);
  HIP_CHECK(hipGetLastError());

  MidasConvArgs A{};
  A.x = gy; A.w = fe.dMidasGradW.p; A.out = gx; A.partial = fe.dMidasSplit.p;
  A.Cin = outChannels; A.N = inChannels; A.H = H; A.W = W; A.HW = H * W;
  A.M = d.M;
  A.S = folded ? std::max(S, 2) : 1;                       // > 1: raw sums to partial `blockIdx.z`, no epilogue
  A.chunksPerSlice = per * fold;
  const dim3 grid(static_cast<unsigned>((A.M + kMidasTile - 1) / kMidasTile), static_cast<unsigned>((inChannels + kMidasTile - 1) / kMidasTile),
                  static_cast<unsigned>(S));
  const bool vec = (static_cast<long long>(outChannels) * T) % 4 == 0 && (reinterpret_cast<uintptr_t>(A.w) & 15) == 0;
  if (kernelSize == 1) {
    if (vec) hipLaunchKernelGGL((k_midas_conv<1, true, false>), grid, dim3(kMidasThreads), 0, s, A);
    else hipLaunchKernelGGL((k_midas_conv<1, false, false>), grid, dim3(kMidasThreads), 0, s, A);
  } else {
    if (vec) hipLaunchKernelGGL((k_midas_conv<3, true, false>), grid, dim3(kMidasThreads), 0, s, A);
    else hipLaunchKernelGGL((k_midas_conv<3, false, false>), grid, dim3(kMidasThreads), 0, s, A);
  }
  HIP_CHECK(hipGetLastError());
  if (!folded) return;
  MidasDgradFoldArgs G{};
  G.partial = fe.dMidasSplit.p; G.add = add; G.mask = mask; G.out = gx; G.S = S; G.total = outFloats;
  hipLaunchKernelGGL(k_midas_dgrad_fold, dim3(static_cast<unsigned>((G.total + kMgThreads - 1) / kMgThreads)), dim3(kMgThreads), 0, s, G);
  HIP_CHECK(hipGetLastError());
}

void midasConvGradWeightDevice(cvd_handle* h, int B, int H, int W, int inChannels, int outChannels, int kernelSize, const float* gy,
                               const float* x, int reluIn, int split, float* gWeight, float* gBias, hipStream_t s) {
  const char* who = "midas conv grad weight";
  const MidasDims d = checkMidasShape(who, B, H, W);
  checkMidasChannels(who, inChannels, outChannels, kernelSize, d.M);
  checkFlag(who, "relu_in", reluIn);
  const long long Q = static_cast<long long>(inChannels) * kernelSize * kernelSize;
  if ((Q + kWgTile - 1) / kWgTile > 0x7fffffffll || (Q * outChannels + kMgThreads - 1) / kMgThreads > 0x7fffffffll)
    throw std::runtime_error(fmt("%s: %d x %lld weights exceed the grid", who, outChannels, Q));
  const long long chains = (d.M + kWgChain - 1) / kWgChain;
  if (split < 0 || split > kWgMaxSplit)
    throw std::runtime_error(fmt("%s: split must be 0 (the rule) or 1 .. %d (got %d)", who, kWgMaxSplit, split));
  if (!gy || !x || !gWeight) throw std::runtime_error(fmt("%s: null array", who));
  const long long wFloats = Q * outChannels;
  for (const auto& in : {std::make_pair(gy, d.M * outChannels), std::make_pair(x, d.M * inChannels)}) {
    if (rangesOverlap(gWeight, wFloats, in.first, in.second)) throw std::runtime_error(fmt("%s: the weight gradient overlaps an input", who));
    if (gBias && rangesOverlap(gBias, outChannels, in.first, in.second)) throw std::runtime_error(fmt("%s: the bias gradient overlaps an input", who));
  }
  if (gBias && rangesOverlap(gBias, outChannels, gWeight, wFloats)) throw std::runtime_error(fmt("%s: the two gradients overlap", who));
  const long long want = split > 0 ? std::min<long long>(split, chains) : midasWgradSplit(d.M, outChannels, Q);
  const long long per = (chains + want - 1) / want;
  const int S = static_cast<int>((chains + per - 1) / per);                    // (a forced split may shrink: slices are whole chains)
  Frontend& fe = *h->frontend;
  if (S > 1) fe.dMidasGradSplit.ensure(static_cast<size_t>(S) * static_cast<size_t>(wFloats));

  MidasWgradArgs A{};
  A.gy = gy; A.x = x; A.out = S > 1 ? fe.dMidasGradSplit.p : gWeight;
  A.reluIn = reluIn; A.N = outChannels; A.Cin = inChannels; A.Q = static_cast<int>(Q);
  A.H = H; A.W = W; A.HW = H * W; A.M = d.M;
  A.chunksPerSlice = static_cast<int>(per) * kWgFold;
  const dim3 grid(static_cast<unsigned>((Q + kWgTile - 1) / kWgTile), static_cast<unsigned>((outChannels + kWgTile - 1) / kWgTile),
                  static_cast<unsigned>(S));
  if (kernelSize == 1) hipLaunchKernelGGL(k_midas_wgrad<1>, grid, dim3(kMgThreads), 0, s, A);
  else hipLaunchKernelGGL(k_midas_wgrad<3>, grid, dim3(kMgThreads), 0, s, A);
  HIP_CHECK(hipGetLastError());
  if (S > 1) {
    MidasWgradFoldArgs G{};
    G.partial = fe.dMidasGradSplit.p; G.out = gWeight; G.S = S; G.total = wFloats;
    hipLaunchKernelGGL(k_midas_wgrad_fold, dim3(static_cast<unsigned>((G.total + kMgThreads - 1) / kMgThreads)), dim3(kMgThreads), 0, s, G);
    HIP_CHECK(hipGetLastError());
  }
  if (gBias) {
    MidasBiasGradArgs Bg{};
    Bg.gy = gy; Bg.out = gBias; Bg.B = B; Bg.N = outChannels; Bg.HW = H * W;
    hipLaunchKernelGGL(k_midas_bias_grad, dim3(static_cast<unsigned>(outChannels)), dim3(kMgThreads), 0, s, Bg);
    HIP_CHECK(hipGetLastError());
  }
}

// gy [B][channels][2 H][2 W] -> gx [B][channels][H][W]
void midasUpsample2xGradDevice(cvd_handle*, int B, int channels, int H, int W, int alignCorners, const float* gy, float* gx,
                               hipStream_t s) {
  const char* who = "midas upsample2x grad";
  if (B < 1 || channels < 1 || H < 1 || W < 1)
    throw std::runtime_error(fmt("%s: batch, channels, height and width must be >= 1 (got %d, %d, %d, %d)", who, B, channels, H, W));
  checkFlag(who, "align_corners", alignCorners);
  const long long planes = static_cast<long long>(B) * channels;
  checkMidasUpsampleSize(who, planes, H, W);
  if (!gy || !gx) throw std::runtime_error(fmt("%s: null array", who));
  const long long n = planes * H * W;
  if (rangesOverlap(gx, n, gy, 4 * n)) throw std::runtime_error(fmt("%s: gx overlaps gy", who));
  MidasUpsampleGradArgs A{};
  A.gy = gy; A.out = gx; A.H = H; A.W = W; A.total = n;
  const dim3 grid(static_cast<unsigned>((n + kMgThreads - 1) / kMgThreads));
  if (alignCorners) hipLaunchKernelGGL(k_midas_upsample2x_grad<true>, grid, dim3(kMgThreads), 0, s, A);
  else hipLaunchKernelGGL(k_midas_upsample2x_grad<false>, grid, dim3(kMgThreads), 0, s, A);
  HIP_CHECK(hipGetLastError());
}

// The output head's backward (midas_net.py:38-41: output_conv.2, ReLU, output_conv.4, ReLU under non_negative).  The forward never
// writes the 32-channel tensor, so it is RECOMPUTED here with the forward's arithmetic: k_midas_conv<3, VEC, false> with one slice
// runs, per output element, the head instantiation's own chain (the same chunks in the same order, folded every kFold chunks) and
// adds the bias in the same operation, so its t is the head's, bit for bit; the head's output for the last ReLU's mask is the head
// launch itself.  Then the pointwise kernel, the two-stage sums for output_conv.4, and the weight and input gradients of
// output_conv.2 through the entry points above on the gradient of t.
void midasHeadGradDevice(cvd_handle* h, int B, int H, int W, int inChannels, int midChannels, const float* gy, const float* x,
                         const float* weight2, const float* bias2, const float* weight4, const float* bias4, int nonNegative, float* gx,
                         float* gWeight2, float* gBias2, float* gWeight4, float* gBias4, hipStream_t s) {
  const char* who = "midas head grad";
  const MidasDims d = checkMidasShape(who, B, H, W);
  if ((d.M + kMidasHeadPixels - 1) / kMidasHeadPixels > 0x7fffffffll) throw std::runtime_error(fmt("%s: %lld pixels exceed the grid", who, d.M));
  if (midChannels != kMidasHeadMid) throw std::runtime_error(fmt("%s: mid_channels must be %d (got %d)", who, kMidasHeadMid, midChannels));
  checkMidasChannels(who, inChannels, kMidasHeadMid, 3, d.M);
  checkFlag(who, "non_negative", nonNegative);
  if (!gy || !x || !weight2 || !bias2 || !weight4 || !bias4 || !gx || !gWeight2 || !gBias2 || !gWeight4 || !gBias4)
    throw std::runtime_error(fmt("%s: null array", who));
  static_assert(kHeadMid == kMidasHeadMid, "one width");
  const long long Q = static_cast<long long>(inChannels) * 9;
  const std::pair<const float*, long long> ins[] = {{gy, d.M}, {x, d.M * inChannels}, {weight2, Q * kHeadMid}, {bias2, kHeadMid},
                                                     {weight4, kHeadMid}, {bias4, 1}};
  const std::pair<const float*, long long> outs[] = {{gx, d.M * inChannels}, {gWeight2, Q * kHeadMid}, {gBias2, kHeadMid},
                                                      {gWeight4, kHeadMid}, {gBias4, 1}};
  for (int o = 0; o < 5; ++o) {
    for (const auto& in : ins)
      if (rangesOverlap(outs[o].first, outs[o].second, in.first, in.second)) throw std::runtime_error(fmt("%s: output %d overlaps an input", who, o));
    for (int o2 = 0; o2 < o; ++o2)
      if (rangesOverlap(outs[o].first, outs[o].second, outs[o2].first, outs[o2].second))
        throw std::runtime_error(fmt("%s: outputs %d and %d overlap", who, o2, o));
  }
  // every scratch buffer at its size before the first launch (the two entry points below then find theirs large enough)
  Frontend& fe = *h->frontend;
  const size_t M32 = static_cast<size_t>(d.M) * kHeadMid;
  const long long groups = (d.M + kMgThreads - 1) / kMgThreads;
  fe.dMidasHeadGrad.ensure(2 * M32 + static_cast<size_t>(d.M));
  fe.dMidasHeadPart.ensure(static_cast<size_t>(groups) * kHeadSums);
  fe.dMidasGradW.ensure(static_cast<size_t>(Q) * kHeadMid);
  const int Sw = midasWgradSplit(d.M, kHeadMid, Q);
  if (Sw > 1) fe.dMidasGradSplit.ensure(static_cast<size_t>(Sw) * static_cast<size_t>(Q) * kHeadMid);
  {
    const int Sd = midasSplitFor(kHeadMid, 3, d.HW, 0);
    if (Sd > 1) fe.dMidasSplit.ensure(static_cast<size_t>(Sd) * static_cast<size_t>(d.M) * inChannels);
  }
  float* t = fe.dMidasHeadGrad.p;
  float* g32 = t + M32;
  float* y = g32 + M32;
  launchMidasConv(B, H, W, inChannels, kMidasHeadMid, 3, x, weight2, bias2, 0, 0, nullptr, 0, nullptr, 1, nullptr, t, s, [] {});
  if (nonNegative) launchMidasHead(B, H, W, inChannels, x, weight2, bias2, weight4, bias4, 1, y, s);
  MidasHeadGradArgs A{};
  A.gy = gy; A.y = y; A.t = t; A.w4 = weight4; A.g32 = g32; A.partial = fe.dMidasHeadPart.p;
  A.nonNegative = nonNegative; A.HW = H * W; A.M = d.M;
  hipLaunchKernelGGL(k_midas_head_grad, dim3(static_cast<unsigned>(groups)), dim3(kMgThreads), 0, s, A);
  HIP_CHECK(hipGetLastError());
  MidasHeadSumArgs G{};
  G.partial = fe.dMidasHeadPart.p; G.gW4 = gWeight4; G.gb4 = gBias4; G.groups = static_cast<int>(groups);
  hipLaunchKernelGGL(k_midas_head_grad_sum, dim3(1), dim3(64), 0, s, G);
  HIP_CHECK(hipGetLastError());
  midasConvGradWeightDevice(h, B, H, W, inChannels, kMidasHeadMid, 3, g32, x, 0, 0, gWeight2, gBias2, s);
  midasConvGradInputDevice(h, B, H, W, inChannels, kMidasHeadMid, 3, g32, weight2, nullptr, nullptr, 0, gx, s);
}

// The decoder's backward in ONE call (cvd_midas_decoder_backward_device): from gy [B][4 H_1][4 W_1], the saved table of
// cvd_midas_decoder_train_device and the parameters to the 21 weight and 17 bias gradients and (gMaps non-null) the four feature-map
// gradients.  It chains the four operators above in the reverse of the forward's order; its results are theirs bit for bit.  The
// 128-channel full-resolution tensor is not saved: it is recomputed from output_conv.0's saved result by the forward's own upsampling
// launch (44 MB per frame less in the table for one more 0.03 ms launch).  kernelMs (measurement only, may be null): one entry per
// stage in the order they run, kMidasBackwardStages of them; with it the call waits on the host.
void midasDecoderBackwardDevice(cvd_handle* h, int B, int features, const int* channels, const int* heights, const int* widths,
                                const float* gy, const float* const* maps, const float* const* saved, const float* const* weights,
                                const float* const* biases, int nonNegative, float* const* gWeights, float* const* gBiases,
                                float* const* gMaps, hipStream_t s, double* kernelMs) {
  const char* who = "midas decoder backward";
  if (!channels || !heights || !widths || !gy || !maps || !saved || !weights || !biases || !gWeights || !gBiases)
    throw std::runtime_error(fmt("%s: null array", who));
  if (features < 1) throw std::runtime_error(fmt("%s: features must be >= 1 (got %d)", who, features));
  checkFlag(who, "non_negative", nonNegative);
  long long M[4];
  for (int k = 0; k < 4; ++k) {
    const MidasDims d = checkMidasShape(who, B, heights[k], widths[k]);
    M[k] = d.M;
    if (channels[k] < 1) throw std::runtime_error(fmt("%s: channels of feature map %d must be >= 1 (got %d)", who, k + 1, channels[k]));
    checkMidasChannels(who, channels[k], features, 3, d.M);
    if (k > 0 && (heights[k - 1] != 2 * heights[k] || widths[k - 1] != 2 * widths[k]))
      throw std::runtime_error(fmt("%s: feature map %d is %d x %d, not twice map %d's %d x %d", who, k, heights[k - 1], widths[k - 1], k + 1,
                                   heights[k], widths[k]));
    if (!maps[k]) throw std::runtime_error(fmt("%s: null feature map %d", who, k + 1));
    if (gMaps && !gMaps[k]) throw std::runtime_error(fmt("%s: null feature-map gradient %d", who, k + 1));
  }
  const int H1 = heights[0], W1 = widths[0];
  if (static_cast<long long>(H1) * W1 > 0x7fffffffll / 16)
    throw std::runtime_error(fmt("%s: %d x %d output pixels per image exceed 2^31", who, 4 * H1, 4 * W1));
  checkMidasUpsampleSize(who, static_cast<long long>(B) * std::max(features, 128), 2 * H1, 2 * W1);
  for (int i = 0; i < 21; ++i)
    if (!weights[i] || !gWeights[i]) throw std::runtime_error(fmt("%s: null weight or weight gradient %d", who, i));
  for (int i = 0; i < 17; ++i)
    if (!biases[i] || !gBiases[i]) throw std::runtime_error(fmt("%s: null bias or bias gradient %d", who, i));
  for (int i = 0; i < kMidasSaved; ++i)
    if (!saved[i]) throw std::runtime_error(fmt("%s: null saved tensor %d", who, i));

  const size_t F = static_cast<size_t>(features), n0 = F * static_cast<size_t>(M[0]);
  const size_t big = 128 * 16 * static_cast<size_t>(M[0]), quarter = 128 * 4 * static_cast<size_t>(M[0]);
  Frontend& fe = *h->frontend;
  fe.dMidasBackward.ensure(2 * big + quarter + 4 * n0 + 5 * n0);
  float* Hup = fe.dMidasBackward.p;
  float* gHup = Hup + big;
  float* gH0 = gHup + big;
  float* gPath = gH0 + quarter;             // [B][F][2 H_1][2 W_1]
  float* X[5];
  for (int i = 0; i < 5; ++i) X[i] = gPath + 4 * n0 + static_cast<size_t>(i) * n0;

  int stage = 0;
  double phaseMs[kMidasBackwardStages];
  KernelTimer timer(s, kernelMs ? phaseMs : nullptr, kMidasBackwardStages);
  timer.mark();
  const auto done = [&] { ++stage; timer.mark(); };
  const auto wgrad = [&](int idx, int k, int Cin, int N, int Hk, int Wk, const float* g, const float* x, int reluIn) {
    midasConvGradWeightDevice(h, B, Hk, Wk, Cin, N, 3, g, x, reluIn, 0, gWeights[idx], idx < 4 ? nullptr : gBiases[idx - 4], s);
    (void)k;
    done();
  };
  const auto dgrad = [&](int idx, int Cin, int N, int Hk, int Wk, const float* g, const float* add, const float* mask, float* gx) {
    midasConvGradInputDevice(h, B, Hk, Wk, Cin, N, 3, g, weights[idx], add, mask, 0, gx, s);
    done();
  };
  // the head: its input recomputed, then its backward; output_conv.0 behind the half-pixel upsampling
  launchMidasUpsample(static_cast<long long>(B) * 128, 2 * H1, 2 * W1, 0, saved[15], Hup, s);
  done();
  midasHeadGradDevice(h, B, 4 * H1, 4 * W1, 128, kMidasHeadMid, gy, Hup, weights[19], biases[15], weights[20], biases[16], nonNegative, gHup,
                      gWeights[19], gBiases[15], gWeights[20], gBiases[16], s);
  done();
  midasUpsample2xGradDevice(h, B, 128, 2 * H1, 2 * W1, 0, gHup, gH0, s);
  done();
  wgrad(18, 0, features, 128, 2 * H1, 2 * W1, gH0, saved[14], 0);
  dgrad(18, features, 128, 2 * H1, 2 * W1, gH0, nullptr, nullptr, gPath);
  // refinenet1 .. refinenet4: the reverse of the forward's order
  const float* gP = gPath;
  for (int k = 0; k < 4; ++k) {
    const int Hk = heights[k], Wk = widths[k];
    const int w0 = k == 3 ? 4 : 6 + 4 * (2 - k);
    const int u2 = k == 3 ? w0 : w0 + 2;
    const int at = 5 + 3 * (2 - k);
    const float* o = k == 3 ? saved[3] : saved[at + 1];       // resConfUnit2's input
    const float* t2 = k == 3 ? saved[4] : saved[at + 2];
    float* g = X[0];
    float* g1 = X[1];
    float* go = X[2 + (k & 1)];                                // (the next level's path gradient: not this level's)
    float* grn = X[4];
    midasUpsample2xGradDevice(h, B, features, Hk, Wk, 1, gP, g, s);
    done();
    wgrad(u2 + 1, k, features, features, Hk, Wk, g, t2, 1);
    dgrad(u2 + 1, features, features, Hk, Wk, g, nullptr, t2, g1);
    wgrad(u2, k, features, features, Hk, Wk, g1, o, 1);
    dgrad(u2, features, features, Hk, Wk, g1, g, o, go);     // (conv1's input gradient + the skip) [o > 0]
    const float* gL = go;
    if (k < 3) {                                               // o = path + resConfUnit1(layerK_rn's result): go flows to both
      const float* t1 = saved[at];
      wgrad(w0 + 1, k, features, features, Hk, Wk, go, t1, 1);
      dgrad(w0 + 1, features, features, Hk, Wk, go, nullptr, t1, g1);
      wgrad(w0, k, features, features, Hk, Wk, g1, saved[k], 1);
      dgrad(w0, features, features, Hk, Wk, g1, go, saved[k], grn);
      gL = grn;
    }
    wgrad(k, k, channels[k], features, Hk, Wk, gL, maps[k], 0);
    if (gMaps) dgrad(k, channels[k], features, Hk, Wk, gL, nullptr, nullptr, gMaps[k]);
    gP = go;
  }
  if (kernelMs) {
    timer.wait();
    timer.collect();
    std::fill(kernelMs, kernelMs + kMidasBackwardStages, 0.0);
    std::copy(phaseMs, phaseMs + stage, kernelMs);
  }
}

// ---- The ResNeXt backbone of MiDaS v2.1 (torchvision's ResNet(Bottleneck, blocks, groups, width_per_group) in eval mode, which the
// reference's monodepth/midas_v2/blocks.py:6-31 builds; cvd_resnext.h).  Device arrays on the caller's stream:
// enqueued launches only. ---------------------------------------------------------------------------------------------------------------
namespace {
struct RxDims {
  long long HW, HWo, M;
  int Ho, Wo;
};

RxDims checkRxShape(const char* who, int B, int H, int W, int stride) {
  if (B < 1 || H < 1 || W < 1) throw std::runtime_error(fmt("%s: batch, height and width must be >= 1 (got %d, %d, %d)", who, B, H, W));
  if (stride != 1 && stride != 2) throw std::runtime_error(fmt("%s: stride must be 1 or 2 (got %d)", who, stride));
  RxDims d{};
  d.HW = static_cast<long long>(H) * W;
  if (d.HW > 0x7fffffffll) throw std::runtime_error(fmt("%s: %d x %d pixels per image exceed 2^31", who, H, W));
  d.Ho = (H - 1) / stride + 1;
  d.Wo = (W - 1) / stride + 1;
  d.HWo = static_cast<long long>(d.Ho) * d.Wo;
  d.M = d.HWo * B;
  if ((d.M + kRxTile - 1) / kRxTile > 0x7fffffffll) throw std::runtime_error(fmt("%s: %lld pixels exceed the grid", who, d.M));
  return d;
}

void checkRxNorm(const char* who, const float* const* norm, float eps) {
  if (!norm) return;
  for (int i = 0; i < 4; ++i)
    if (!norm[i]) throw std::runtime_error(fmt("%s: null norm vector %d", who, i));
  if (!(eps > 0.f)) throw std::runtime_error(fmt("%s: eps must be > 0 (got %g)", who, static_cast<double>(eps)));
}

bool rxGroupWidthBuilt(int cg) { return cg == 8 || cg == 16 || cg == 32 || cg == 64; }

// the dense convolution's channel counts and filter against the instantiations and the grid
void checkRxChannels(const char* who, int Cin, int N, int ks, int stride, long long M) {
  if (ks != 1 && ks != 7) throw std::runtime_error(fmt("%s: kernel_size must be 1 or 7 (got %d)", who, ks));
  if (ks == 7 && stride != 2) throw std::runtime_error(fmt("%s: kernel_size 7 is built for stride 2 only (got stride %d)", who, stride));
  if (Cin < 1) throw std::runtime_error(fmt("%s: in_channels must be >= 1 (got %d)", who, Cin));
  if (N < 1) throw std::runtime_error(fmt("%s: out_channels must be >= 1 (got %d)", who, N));
  if (static_cast<long long>(Cin) * ks * ks > 0x7fffffffll) throw std::runtime_error(fmt("%s: in_channels %d exceeds the kernel's range", who, Cin));
  if ((N + kRxTile - 1) / kRxTile > 65535) throw std::runtime_error(fmt("%s: out_channels %d exceeds the grid", who, N));
  if ((M * N + kRxThreads - 1) / kRxThreads > 0x7fffffffll)
    throw std::runtime_error(fmt("%s: %lld pixels of %d channels exceed the grid", who, M, N));
}

void checkRxGroups(const char* who, int G, int cg, long long M) {
  if (G < 1) throw std::runtime_error(fmt("%s: groups must be >= 1 (got %d)", who, G));
  if (!rxGroupWidthBuilt(cg)) throw std::runtime_error(fmt("%s: channels per group must be 8, 16, 32 or 64 (got %d)", who, cg));
  const long long N = static_cast<long long>(G) * cg;
  if ((N + kRxGroupTileN - 1) / kRxGroupTileN > 65535) throw std::runtime_error(fmt("%s: %d groups of %d channels exceed the grid", who, G, cg));
  if (M * N / kRxThreads > 0x7fffffffll) throw std::runtime_error(fmt("%s: %lld pixels of %lld channels exceed the kernel's range", who, M, N));
}

int rxChunks(int Cin, int ks) {
  const int cc = ks == 1 ? RxShape<1>::kChunkChannels : RxShape<7>::kChunkChannels;
  return (Cin + cc - 1) / cc;
}

// the split the convolution runs with: `forced` >= 1 as given (checked by the caller), 0 = the rule
int rxSplitFor(int Cin, int ks, long long HWo, int forced) {
  return forced > 0 ? forced : rxSplit(static_cast<long long>(Cin) * ks * ks, HWo, ks);
}

size_t rxSplitFloats(int S, long long M, int N) { return S > 1 ? static_cast<size_t>(S) * static_cast<size_t>(M) * N : 0; }

void rxNormArgs(RxConvArgs& A, const float* const* norm, float eps) {
  if (norm) {
    A.gamma = norm[0]; A.beta = norm[1]; A.mean = norm[2]; A.var = norm[3];
  }
  A.eps = eps;
}

template <int KS, int STRIDE>
void launchRxConvK(const RxConvArgs& A, bool vec, dim3 grid, hipStream_t s) {
  if (vec) hipLaunchKernelGGL((k_rx_conv<KS, STRIDE, true>), grid, dim3(kRxThreads), 0, s, A);
  else hipLaunchKernelGGL((k_rx_conv<KS, STRIDE, false>), grid, dim3(kRxThreads), 0, s, A);
}

// One dense convolution: one launch, with S > 1 the fold behind it.  Checked by the callers; `partial` holds rxSplitFloats floats.
// norm: {weight, bias, running_mean, running_var} or null.  mark (may be empty) is called after each launch.
template <class Mark>
void launchRxConv(int B, int H, int W, int Cin, int N, int ks, int stride, const float* x, const float* w, const float* const* norm,
                  float eps, int relu, const float* residual, int S, float* partial, float* out, hipStream_t s, Mark&& mark) {
  RxConvArgs A{};
  A.x = x; A.w = w; A.residual = residual; A.out = out; A.partial = partial; A.relu = relu;
  rxNormArgs(A, norm, eps);
  A.Cin = Cin; A.N = N;
  A.H = H; A.W = W; A.HW = H * W;
  A.Ho = (H - 1) / stride + 1; A.Wo = (W - 1) / stride + 1; A.HWo = A.Ho * A.Wo;
  A.M = static_cast<long long>(A.HWo) * B;
  const int fold = ks == 1 ? RxShape<1>::kFold : RxShape<7>::kFold;
  const int chunks = rxChunks(Cin, ks), chains = (chunks + fold - 1) / fold;
  const int per = (chains + S - 1) / S;                   // chains per slice
  A.S = (chains + per - 1) / per;                         // (the rule's S already has this form; a forced one may shrink)
  A.chunksPerSlice = per * fold;
  const dim3 grid(static_cast<unsigned>((A.M + kRxTile - 1) / kRxTile), static_cast<unsigned>((N + kRxTile - 1) / kRxTile),
                  static_cast<unsigned>(A.S));
  // float4 weight loads only where every row starts on 16 bytes
  const bool vec = (static_cast<long long>(Cin) * ks * ks) % 4 == 0 && (reinterpret_cast<uintptr_t>(w) & 15) == 0;
  if (ks == 7) hipLaunchKernelGGL((k_rx_conv<7, 2, false>), grid, dim3(kRxThreads), 0, s, A);
  else if (stride == 1) launchRxConvK<1, 1>(A, vec, grid, s);
  else launchRxConvK<1, 2>(A, vec, grid, s);
  HIP_CHECK(hipGetLastError());
  mark();
  if (A.S == 1) return;
  hipLaunchKernelGGL(k_rx_fold, dim3(static_cast<unsigned>((A.M * N + kRxThreads - 1) / kRxThreads)), dim3(kRxThreads), 0, s, A);
  HIP_CHECK(hipGetLastError());
  mark();
}

template <int CG>
void launchRxGroupConvK(const RxConvArgs& A, int stride, dim3 grid, hipStream_t s) {
  if (stride == 1) hipLaunchKernelGGL((k_rx_gconv<CG, 1>), grid, dim3(kRxThreads), 0, s, A);
  else hipLaunchKernelGGL((k_rx_gconv<CG, 2>), grid, dim3(kRxThreads), 0, s, A);
}

// One grouped 3 x 3 convolution over G groups of cg channels: one launch.  Checked by the callers.
void launchRxGroupConv(int B, int H, int W, int G, int cg, int stride, const float* x, const float* w, const float* const* norm,
                       float eps, int relu, float* out, hipStream_t s) {
  RxConvArgs A{};
  A.x = x; A.w = w; A.out = out; A.relu = relu;
  rxNormArgs(A, norm, eps);
  A.Cin = A.N = G * cg;
  A.H = H; A.W = W; A.HW = H * W;
  A.Ho = (H - 1) / stride + 1; A.Wo = (W - 1) / stride + 1; A.HWo = A.Ho * A.Wo;
  A.M = static_cast<long long>(A.HWo) * B;
  A.S = 1;
  const dim3 grid(static_cast<unsigned>((A.M + kRxTile - 1) / kRxTile), static_cast<unsigned>((A.N + kRxGroupTileN - 1) / kRxGroupTileN));
  switch (cg) {
    case 8: launchRxGroupConvK<8>(A, stride, grid, s); break;
    case 16: launchRxGroupConvK<16>(A, stride, grid, s); break;
    case 32: launchRxGroupConvK<32>(A, stride, grid, s); break;
    default: launchRxGroupConvK<64>(A, stride, grid, s); break;
  }
  HIP_CHECK(hipGetLastError());
}

void checkRxPoolSize(const char* who, long long planes, long long HWo) {
  if (planes > 0x7fffffffll || (planes * HWo + kRxThreads - 1) / kRxThreads > 0x7fffffffll)
    throw std::runtime_error(fmt("%s: %lld planes of %lld elements exceed the grid", who, planes, HWo));
}

void launchRxMaxPool(long long planes, int H, int W, const float* x, float* out, hipStream_t s) {
  RxPoolArgs A{};
  A.x = x; A.out = out; A.H = H; A.W = W;
  A.Ho = (H - 1) / 2 + 1; A.Wo = (W - 1) / 2 + 1;
  A.total = planes * A.Ho * A.Wo;
  hipLaunchKernelGGL(k_rx_maxpool, dim3(static_cast<unsigned>((A.total + kRxThreads - 1) / kRxThreads)), dim3(kRxThreads), 0, s, A);
  HIP_CHECK(hipGetLastError());
}
}  // namespace

void resnextGroupedConvDevice(cvd_handle*, int B, int H, int W, int groups, int channelsPerGroup, int stride, const float* x,
                              const float* weight, const float* const* norm, float eps, int relu, float* out, hipStream_t s) {
  const char* who = "resnext grouped conv";
  const RxDims d = checkRxShape(who, B, H, W, stride);
  checkRxGroups(who, groups, channelsPerGroup, d.M);
  checkFlag(who, "relu", relu);
  if (!x || !weight || !out) throw std::runtime_error(fmt("%s: null array", who));
  checkRxNorm(who, norm, eps);
  const long long N = static_cast<long long>(groups) * channelsPerGroup;
  if (rangesOverlap(out, d.M * N, x, d.HW * B * N)) throw std::runtime_error(fmt("%s: out overlaps x", who));
  launchRxGroupConv(B, H, W, groups, channelsPerGroup, stride, x, weight, norm, eps, relu, out, s);
}

void resnextConvDevice(cvd_handle* h, int B, int H, int W, int inChannels, int outChannels, int kernelSize, int stride, const float* x,
                       const float* weight, const float* const* norm, float eps, int relu, const float* residual, int split, float* out,
                       hipStream_t s) {
  const char* who = "resnext conv";
  const RxDims d = checkRxShape(who, B, H, W, stride);
  checkRxChannels(who, inChannels, outChannels, kernelSize, stride, d.M);
  checkFlag(who, "relu", relu);
  const int chunks = rxChunks(inChannels, kernelSize);
  if (split < 0 || split > chunks)
    throw std::runtime_error(fmt("%s: split must be 0 (the rule) or 1 .. %d, the chunks of K (got %d)", who, chunks, split));
  if (!x || !weight || !out) throw std::runtime_error(fmt("%s: null array", who));
  checkRxNorm(who, norm, eps);
  const long long outFloats = d.M * outChannels;
  if (rangesOverlap(out, outFloats, x, d.HW * B * inChannels)) throw std::runtime_error(fmt("%s: out overlaps x", who));
  if (residual && rangesOverlap(out, outFloats, residual, outFloats)) throw std::runtime_error(fmt("%s: out overlaps the residual", who));
  const int S = rxSplitFor(inChannels, kernelSize, d.HWo, split);
  Frontend& fe = *h->frontend;
  fe.dRxSplit.ensure(rxSplitFloats(S, d.M, outChannels));
  launchRxConv(B, H, W, inChannels, outChannels, kernelSize, stride, x, weight, norm, eps, relu, residual, S, fe.dRxSplit.p, out, s, [] {});
}

void resnextMaxPoolDevice(cvd_handle*, int B, int channels, int H, int W, const float* x, float* out, hipStream_t s) {
  const char* who = "resnext maxpool";
  if (channels < 1) throw std::runtime_error(fmt("%s: channels must be >= 1 (got %d)", who, channels));
  const RxDims d = checkRxShape(who, B, H, W, 2);
  const long long planes = static_cast<long long>(B) * channels;
  checkRxPoolSize(who, planes, d.HWo);
  if (!x || !out) throw std::runtime_error(fmt("%s: null array", who));
  if (rangesOverlap(out, planes * d.HWo, x, planes * d.HW)) throw std::runtime_error(fmt("%s: out overlaps x", who));
  launchRxMaxPool(planes, H, W, x, out, s);
}

// ResNet.forward up to layer4 as MidasNet.forward reads it (the four stages' outputs).  blocks: the four stages' block counts.
// weights: one per convolution in the state dict's order (the stem, then per block conv1, conv2, conv3 and, in a stage's first
// block, downsample.0); norms: 4 vectors per convolution in the same order.  outs: the four stages' outputs.
// kernelMs (measurement only, may be null): 2 convolutions + 1 entries; with it the call waits on the host.
void midasBackboneDevice(cvd_handle* h, int B, int H, int W, const int* blocks, int groups, int widthPerGroup, float eps,
                         const float* images, const float* const* weights, const float* const* norms, float* const* outs,
                         hipStream_t s, double* kernelMs) {
  const char* who = "midas backbone";
  if (!blocks || !images || !weights || !norms || !outs) throw std::runtime_error(fmt("%s: null array", who));
  if (B < 1 || H < 1 || W < 1) throw std::runtime_error(fmt("%s: batch, height and width must be >= 1 (got %d, %d, %d)", who, B, H, W));
  if (H % 32 != 0 || W % 32 != 0) throw std::runtime_error(fmt("%s: height and width must be multiples of 32 (got %d x %d)", who, H, W));
  if (groups < 1) throw std::runtime_error(fmt("%s: groups must be >= 1 (got %d)", who, groups));
  if (widthPerGroup < 1) throw std::runtime_error(fmt("%s: width_per_group must be >= 1 (got %d)", who, widthPerGroup));
  if (!(eps > 0.f)) throw std::runtime_error(fmt("%s: eps must be > 0 (got %g)", who, static_cast<double>(eps)));
  checkRxShape(who, B, H, W, 2);
  int cg[4], width[4], outC[4], hs[4], ws[4], numConvs = 1;
  long long outFloats[4];
  const size_t b = static_cast<size_t>(B);
  for (int k = 0; k < 4; ++k) {
    if (blocks[k] < 1) throw std::runtime_error(fmt("%s: blocks of layer%d must be >= 1 (got %d)", who, k + 1, blocks[k]));
    if (blocks[k] > 1000000) throw std::runtime_error(fmt("%s: blocks of layer%d exceed the call's range (got %d)", who, k + 1, blocks[k]));
    const long long planes = 64ll << k, per = planes * widthPerGroup / 64;
    if (per > 64 || !rxGroupWidthBuilt(static_cast<int>(per)))
      throw std::runtime_error(fmt("%s: layer%d has %lld channels per group; 8, 16, 32 and 64 are built (width_per_group %d)", who, k + 1,
                                   per, widthPerGroup));
    cg[k] = static_cast<int>(per);
    outC[k] = static_cast<int>(4 * planes);
    hs[k] = H >> (k + 2);
    ws[k] = W >> (k + 2);
    const long long M = static_cast<long long>(B) * hs[k] * ws[k];
    checkRxGroups(who, groups, cg[k], 4 * M);
    width[k] = groups * cg[k];
    checkRxChannels(who, width[k], outC[k], 1, 1, M);
    checkRxChannels(who, outC[k], width[k], 1, 1, 4 * M);
    outFloats[k] = M * outC[k];
    numConvs += 3 * blocks[k] + 1;
  }
  checkRxChannels(who, 3, 64, 7, 2, static_cast<long long>(B) * (H / 2) * (W / 2));
  checkRxPoolSize(who, static_cast<long long>(B) * 64, static_cast<long long>(H / 4) * (W / 4));
  for (int i = 0; i < numConvs; ++i) {
    if (!weights[i]) throw std::runtime_error(fmt("%s: null weight %d", who, i));
    for (int j = 0; j < 4; ++j)
      if (!norms[4 * i + j]) throw std::runtime_error(fmt("%s: null norm vector %d of convolution %d", who, j, i));
  }
  for (int k = 0; k < 4; ++k) {
    if (!outs[k]) throw std::runtime_error(fmt("%s: null output map %d", who, k + 1));
    if (rangesOverlap(outs[k], outFloats[k], images, static_cast<long long>(b) * 3 * H * W))
      throw std::runtime_error(fmt("%s: output map %d overlaps the images", who, k + 1));
    for (int j = 0; j < k; ++j)
      if (rangesOverlap(outs[k], outFloats[k], outs[j], outFloats[j]))
        throw std::runtime_error(fmt("%s: output map %d overlaps output map %d", who, k + 1, j + 1));
  }

  // scratch: the stem's output, the pooled map, a block's two middle tensors and its downsample branch at their largest, two
  // rotating block outputs; and the split convolutions' partial sums
  const size_t m2 = b * (H / 2) * (W / 2), m4 = b * (H / 4) * (W / 4);
  size_t t1 = 0, t2 = 0, big = 0, split = 0;
  {
    int Cin = 64, hin = H / 4, win = W / 4;
    for (int k = 0; k < 4; ++k) {
      const size_t mIn = b * hin * win, mOut = b * hs[k] * ws[k];
      const long long hwIn = static_cast<long long>(hin) * win, hwOut = static_cast<long long>(hs[k]) * ws[k];
      t1 = std::max(t1, std::max(mIn, mOut) * width[k]);
      t2 = std::max(t2, mOut * width[k]);
      big = std::max(big, mOut * outC[k]);
      split = std::max(split, rxSplitFloats(rxSplitFor(Cin, 1, hwIn, 0), static_cast<long long>(mIn), width[k]));        // first conv1
      split = std::max(split, rxSplitFloats(rxSplitFor(Cin, 1, hwOut, 0), static_cast<long long>(mOut), outC[k]));       // downsample.0
      split = std::max(split, rxSplitFloats(rxSplitFor(outC[k], 1, hwOut, 0), static_cast<long long>(mOut), width[k]));  // later conv1
      split = std::max(split, rxSplitFloats(rxSplitFor(width[k], 1, hwOut, 0), static_cast<long long>(mOut), outC[k]));  // conv3
      Cin = outC[k]; hin = hs[k]; win = ws[k];
    }
  }
  Frontend& fe = *h->frontend;
  fe.dRx.ensure(64 * m2 + 64 * m4 + t1 + t2 + 3 * big);
  fe.dRxSplit.ensure(split);
  float* stem = fe.dRx.p;
  float* pooled = stem + 64 * m2;
  float* T1 = pooled + 64 * m4;
  float* T2 = T1 + t1;
  float* DS = T2 + t2;
  float* R[2] = {DS + big, DS + 2 * big};

  const int slots = 2 * numConvs + 1;
  std::vector<double> phaseMs(kernelMs ? slots : 0);
  std::vector<int> slot;
  slot.reserve(slots);
  KernelTimer timer(s, kernelMs ? phaseMs.data() : nullptr, slots);
  timer.mark();
  const auto conv = [&](int idx, const float* x, int Cin, int hin, int win, int N, int ks, int stride, int relu, const float* residual,
                        float* y) {
    int part = 0;
    const long long hwo = static_cast<long long>((hin - 1) / stride + 1) * ((win - 1) / stride + 1);
    launchRxConv(B, hin, win, Cin, N, ks, stride, x, weights[idx], norms + 4 * idx, eps, relu, residual, rxSplitFor(Cin, ks, hwo, 0),
                 fe.dRxSplit.p, y, s, [&] {
                   slot.push_back(2 * idx + part++);
                   timer.mark();
                 });
  };
  conv(0, images, 3, H, W, 64, 7, 2, 1, nullptr, stem);
  launchRxMaxPool(static_cast<long long>(B) * 64, H / 2, W / 2, stem, pooled, s);
  slot.push_back(2 * numConvs);
  timer.mark();
  const float* cur = pooled;
  int Cin = 64, hin = H / 4, win = W / 4, idx = 1, turn = 0;
  for (int k = 0; k < 4; ++k) {
    for (int blk = 0; blk < blocks[k]; ++blk) {
      const int stride = blk == 0 && k > 0 ? 2 : 1;
      const bool down = blk == 0;                       // stride 2 or in != 4 planes: every stage's first block
      conv(idx, cur, Cin, hin, win, width[k], 1, 1, 1, nullptr, T1);
      launchRxGroupConv(B, hin, win, groups, cg[k], stride, T1, weights[idx + 1], norms + 4 * (idx + 1), eps, 1, T2, s);
      slot.push_back(2 * (idx + 1));
      timer.mark();
      const float* residual = cur;
      if (down) {
        conv(idx + 3, cur, Cin, hin, win, outC[k], 1, stride, 0, nullptr, DS);
        residual = DS;
      }
      float* y = blk == blocks[k] - 1 ? outs[k] : R[turn ^= 1];
      conv(idx + 2, T2, width[k], hs[k], ws[k], outC[k], 1, 1, 0, residual, y);
      cur = y;
      Cin = outC[k]; hin = hs[k]; win = ws[k];
      idx += down ? 4 : 3;
    }
  }
  if (kernelMs) {
    timer.wait();
    timer.collect();
    std::fill(kernelMs, kernelMs + slots, 0.0);
    for (size_t i = 0; i < slot.size(); ++i) kernelMs[slot[i]] = phaseMs[i];
  }
}

// ---- Training of the backbone (cvd_resnext_grad.h): nn.BatchNorm2d in training and in eval mode with its backward,
// and the backward of the backbone's convolutions and of its pool.  Device arrays on the caller's stream: enqueued launches only. -----
namespace {
struct RxgNormPlan {
  int S;
  long long perSlice;
};

RxgNormPlan rxgNormPlan(int N, long long M) {
  const long long chunks = (M + kRgNormChunk - 1) / kRgNormChunk;
  const int want = rxgNormSplit(N, M);
  const long long per = (chunks + want - 1) / want;
  return {static_cast<int>((chunks + per - 1) / per), per * kRgNormChunk};
}

// channelGrid: the caller puts the channels on grid.y (the two batch norm reductions)
long long checkRxgPlanes(const char* who, int B, int channels, int H, int W, bool channelGrid = false) {
  if (B < 1 || channels < 1 || H < 1 || W < 1)
    throw std::runtime_error(fmt("%s: batch, channels, height and width must be >= 1 (got %d, %d, %d, %d)", who, B, channels, H, W));
  const long long HW = static_cast<long long>(H) * W;
  if (HW > 0x7fffffffll) throw std::runtime_error(fmt("%s: %d x %d pixels per image exceed 2^31", who, H, W));
  if (channelGrid && channels > 65535) throw std::runtime_error(fmt("%s: %d channels exceed the grid", who, channels));
  const long long total = HW * B * channels;
  if ((total + kRgThreads - 1) / kRgThreads > 0x7fffffffll)
    throw std::runtime_error(fmt("%s: %lld elements exceed the grid", who, total));
  return total;
}

template <int KS, int STRIDE>
void launchRxgWgradK(const RxgConvArgs& A, dim3 grid, hipStream_t s) {
  hipLaunchKernelGGL((k_rxg_wgrad<KS, STRIDE>), grid, dim3(kRgThreads), 0, s, A);
}

// The weight gradient of a (grouped) ks x ks convolution on k_rxg_wgrad and its fold.  Checked by the callers.
void launchRxgWgrad(Frontend& fe, int B, int H, int W, int Cin, int N, int cg, int ng, int ks, int stride, const float* gy, const float* x,
                    int split, float* gWeight, hipStream_t s) {
  RxgConvArgs A{};
  A.gy = gy; A.x = x;
  A.Cin = Cin; A.N = N; A.CG = cg; A.NG = ng;
  A.H = H; A.W = W; A.HW = H * W;
  A.Ho = (H - 1) / stride + 1; A.Wo = (W - 1) / stride + 1; A.HWo = A.Ho * A.Wo;
  A.M = static_cast<long long>(A.HWo) * B;
  A.elements = static_cast<long long>(N) * cg * ks * ks;
  const long long chains = (A.M + kRgWgradChain - 1) / kRgWgradChain;
  const long long want = split > 0 ? std::min<long long>(split, chains) : rxgWgradSplit(A.M, A.elements);
  const long long per = (chains + want - 1) / want;
  const int S = static_cast<int>((chains + per - 1) / per);                      // (a forced split may shrink: slices are whole chains)
  A.chainsPerSlice = per;
  fe.dRxGradSums.ensure(static_cast<size_t>(S) * static_cast<size_t>(A.elements));
  A.partial = fe.dRxGradSums.p;
  const dim3 grid(static_cast<unsigned>((A.elements + kRgThreads - 1) / kRgThreads), static_cast<unsigned>(S));
  if (ks == 7) launchRxgWgradK<7, 2>(A, grid, s);
  else if (stride == 1) launchRxgWgradK<3, 1>(A, grid, s);
  else launchRxgWgradK<3, 2>(A, grid, s);
  HIP_CHECK(hipGetLastError());
  RxgFoldArgs F{};
  F.partial = fe.dRxGradSums.p; F.out = gWeight; F.S = S; F.total = A.elements;
  hipLaunchKernelGGL(k_rxg_wgrad_fold, dim3(static_cast<unsigned>((F.total + kRgThreads - 1) / kRgThreads)), dim3(kRgThreads), 0, s, F);
  HIP_CHECK(hipGetLastError());
}

template <int CG>
void launchRxgGroupDgradK(const RxgConvArgs& A, int stride, dim3 grid, hipStream_t s) {
  if (stride == 1) hipLaunchKernelGGL((k_rxg_gconv_dgrad<CG, 1>), grid, dim3(kRgThreads), 0, s, A);
  else hipLaunchKernelGGL((k_rxg_gconv_dgrad<CG, 2>), grid, dim3(kRgThreads), 0, s, A);
}
}  // namespace

// nn.BatchNorm2d on the raw convolution output c [B][N][H][W]: y = (c - mean) invstd gamma + beta, ReLU under relu, with a residual
// max(residual + y, 0).  training: the batch statistics (written to saveMean / saveInvstd, the running statistics updated with
// `momentum`); else the running statistics (saveMean / saveInvstd receive what the expression used, for the backward).
void resnextNormTrainDevice(cvd_handle* h, int B, int channels, int H, int W, const float* c, const float* gamma, const float* beta,
                            float* runningMean, float* runningVar, double eps, double momentum, int training, int relu,
                            const float* residual, float* saveMean, float* saveInvstd, float* y, hipStream_t s) {
  const char* who = "resnext norm train";
  const long long total = checkRxgPlanes(who, B, channels, H, W, true);
  checkFlag(who, "training", training);
  checkFlag(who, "relu", relu);
  if (!(eps > 0.0)) throw std::runtime_error(fmt("%s: eps must be > 0 (got %g)", who, eps));
  if (!(momentum >= 0.0 && momentum <= 1.0)) throw std::runtime_error(fmt("%s: momentum must lie in [0, 1] (got %g)", who, momentum));
  const long long M = total / channels;
  if (training && M < 2)
    throw std::runtime_error(fmt("%s: training mode needs more than 1 value per channel (got batch %d of %d x %d)", who, B, H, W));
  if (!c || !gamma || !beta || !runningMean || !runningVar || !saveMean || !saveInvstd || !y) throw std::runtime_error(fmt("%s: null array", who));
  if (rangesOverlap(y, total, c, total)) throw std::runtime_error(fmt("%s: y overlaps c", who));
  if (residual && rangesOverlap(y, total, residual, total)) throw std::runtime_error(fmt("%s: y overlaps the residual", who));
  const std::pair<const float*, const char*> vectors[] = {{gamma, "gamma"}, {beta, "beta"}, {runningMean, "running_mean"},
                                                          {runningVar, "running_var"}, {saveMean, "save_mean"}, {saveInvstd, "save_invstd"}};
  for (const auto& v : vectors)
    if (rangesOverlap(y, total, v.first, channels)) throw std::runtime_error(fmt("%s: y overlaps %s", who, v.second));
  for (int i = 2; i < 6; ++i) {
    if (rangesOverlap(vectors[i].first, channels, c, total)) throw std::runtime_error(fmt("%s: %s overlaps c", who, vectors[i].second));
    for (int j = 0; j < i; ++j)
      if (rangesOverlap(vectors[i].first, channels, vectors[j].first, channels))
        throw std::runtime_error(fmt("%s: %s overlaps %s", who, vectors[i].second, vectors[j].second));
  }
  Frontend& fe = *h->frontend;
  const RxgNormPlan plan = rxgNormPlan(channels, M);
  RxgNormArgs A{};
  A.c = c; A.gamma = gamma; A.beta = beta; A.residual = residual; A.mean = saveMean; A.invstd = saveInvstd; A.out = y;
  A.relu = relu; A.training = training;
  A.N = channels; A.HW = H * W; A.S = plan.S; A.perSlice = plan.perSlice; A.M = M; A.total = total;
  if (training) {
    fe.dRxGradSums.ensure(static_cast<size_t>(channels) * plan.S * 2);
    A.partial = fe.dRxGradSums.p;
    hipLaunchKernelGGL(k_rxg_norm_stats, dim3(static_cast<unsigned>(plan.S), static_cast<unsigned>(channels)), dim3(kRgThreads), 0, s, A);
    HIP_CHECK(hipGetLastError());
  }
  RxgNormFinishArgs F{};
  F.partial = fe.dRxGradSums.p; F.runningMean = runningMean; F.runningVar = runningVar; F.mean = saveMean; F.invstd = saveInvstd;
  F.eps = eps; F.momentum = momentum; F.training = training; F.N = channels; F.S = plan.S; F.M = M;
  hipLaunchKernelGGL(k_rxg_norm_finish, dim3(static_cast<unsigned>((channels + kRgThreads - 1) / kRgThreads)), dim3(kRgThreads), 0, s, F);
  HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(k_rxg_norm_apply, dim3(static_cast<unsigned>((total + kRgThreads - 1) / kRgThreads)), dim3(kRgThreads), 0, s, A);
  HIP_CHECK(hipGetLastError());
}

// Its backward: g = gy [y > 0] with the layer's output y (null: g = gy); gBeta = sum g, gGamma = sum g xhat; gc; gResidual = g.
void resnextNormGradDevice(cvd_handle* h, int B, int channels, int H, int W, const float* gy, const float* c, const float* y,
                           const float* mean, const float* invstd, const float* gamma, int training, float* gc, float* gGamma,
                           float* gBeta, float* gResidual, hipStream_t s) {
  const char* who = "resnext norm grad";
  const long long total = checkRxgPlanes(who, B, channels, H, W, true);
  checkFlag(who, "training", training);
  const long long M = total / channels;
  if (training && M < 2)
    throw std::runtime_error(fmt("%s: training mode needs more than 1 value per channel (got batch %d of %d x %d)", who, B, H, W));
  if (!gy || !c || !mean || !invstd || !gamma || !gc || !gGamma || !gBeta) throw std::runtime_error(fmt("%s: null array", who));
  const std::pair<const float*, long long> inputs[] = {{gy, total}, {c, total}, {y, y ? total : 0}, {mean, channels},
                                                       {invstd, channels}, {gamma, channels}};
  const std::pair<const float*, long long> outputs[] = {{gc, total}, {gGamma, channels}, {gBeta, channels},
                                                        {gResidual, gResidual ? total : 0}};
  for (int i = 0; i < 4; ++i) {
    if (!outputs[i].first) continue;
    for (const auto& in : inputs)
      if (in.first && rangesOverlap(outputs[i].first, outputs[i].second, in.first, in.second))
        throw std::runtime_error(fmt("%s: output %d overlaps an input", who, i));
    for (int j = 0; j < i; ++j)
      if (outputs[j].first && rangesOverlap(outputs[i].first, outputs[i].second, outputs[j].first, outputs[j].second))
        throw std::runtime_error(fmt("%s: output %d overlaps output %d", who, i, j));
  }
  Frontend& fe = *h->frontend;
  const RxgNormPlan plan = rxgNormPlan(channels, M);
  fe.dRxGradSums.ensure(static_cast<size_t>(channels) * plan.S * 2);
  RxgNormArgs A{};
  A.c = c; A.y = y; A.gy = gy; A.gamma = gamma; A.mean = mean; A.invstd = invstd; A.gbeta = gBeta; A.ggamma = gGamma;
  A.out = gc; A.outResidual = gResidual; A.partial = fe.dRxGradSums.p; A.training = training;
  A.N = channels; A.HW = H * W; A.S = plan.S; A.perSlice = plan.perSlice; A.M = M; A.total = total;
  hipLaunchKernelGGL(k_rxg_norm_grad_sums, dim3(static_cast<unsigned>(plan.S), static_cast<unsigned>(channels)), dim3(kRgThreads), 0, s, A);
  HIP_CHECK(hipGetLastError());
  RxgNormGradFinishArgs F{};
  F.partial = fe.dRxGradSums.p; F.gbeta = gBeta; F.ggamma = gGamma; F.N = channels; F.S = plan.S;
  hipLaunchKernelGGL(k_rxg_norm_grad_finish, dim3(static_cast<unsigned>((channels + kRgThreads - 1) / kRgThreads)), dim3(kRgThreads), 0, s, F);
  HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(k_rxg_norm_grad_apply, dim3(static_cast<unsigned>((total + kRgThreads - 1) / kRgThreads)), dim3(kRgThreads), 0, s, A);
  HIP_CHECK(hipGetLastError());
}

// gy [B][G cg][Ho][Wo], weight [G cg][cg][3][3] -> gx [B][G cg][H][W]
void resnextGroupedConvGradInputDevice(cvd_handle*, int B, int H, int W, int groups, int channelsPerGroup, int stride, const float* gy,
                                       const float* weight, float* gx, hipStream_t s) {
  const char* who = "resnext grouped conv grad input";
  const RxDims d = checkRxShape(who, B, H, W, stride);
  checkRxGroups(who, groups, channelsPerGroup, d.HW * B);
  if (!gy || !weight || !gx) throw std::runtime_error(fmt("%s: null array", who));
  const long long N = static_cast<long long>(groups) * channelsPerGroup;
  if (rangesOverlap(gx, d.HW * B * N, gy, d.M * N)) throw std::runtime_error(fmt("%s: gx overlaps gy", who));
  if (rangesOverlap(gx, d.HW * B * N, weight, N * channelsPerGroup * 9)) throw std::runtime_error(fmt("%s: gx overlaps the weight", who));
  RxgConvArgs A{};
  A.gy = gy; A.w = weight; A.out = gx;
  A.Cin = A.N = static_cast<int>(N); A.CG = A.NG = channelsPerGroup;
  A.H = H; A.W = W; A.HW = H * W; A.Ho = d.Ho; A.Wo = d.Wo; A.HWo = static_cast<int>(d.HWo);
  A.M = d.HW * B;
  const dim3 grid(static_cast<unsigned>((A.M + kRgTile - 1) / kRgTile), static_cast<unsigned>((N + kRgGroupTileN - 1) / kRgGroupTileN));
  switch (channelsPerGroup) {
    case 8: launchRxgGroupDgradK<8>(A, stride, grid, s); break;
    case 16: launchRxgGroupDgradK<16>(A, stride, grid, s); break;
    case 32: launchRxgGroupDgradK<32>(A, stride, grid, s); break;
    default: launchRxgGroupDgradK<64>(A, stride, grid, s); break;
  }
  HIP_CHECK(hipGetLastError());
}

// gy [B][G cg][Ho][Wo], x [B][G cg][H][W] -> gWeight [G cg][cg][3][3]
void resnextGroupedConvGradWeightDevice(cvd_handle* h, int B, int H, int W, int groups, int channelsPerGroup, int stride, const float* gy,
                                        const float* x, int split, float* gWeight, hipStream_t s) {
  const char* who = "resnext grouped conv grad weight";
  const RxDims d = checkRxShape(who, B, H, W, stride);
  checkRxGroups(who, groups, channelsPerGroup, d.HW * B);
  if (split < 0 || split > kRgWgradMaxSplit)
    throw std::runtime_error(fmt("%s: split must be 0 (the rule) or 1 .. %d (got %d)", who, kRgWgradMaxSplit, split));
  if (!gy || !x || !gWeight) throw std::runtime_error(fmt("%s: null array", who));
  const long long N = static_cast<long long>(groups) * channelsPerGroup, wFloats = N * channelsPerGroup * 9;
  if (rangesOverlap(gWeight, wFloats, gy, d.M * N) || rangesOverlap(gWeight, wFloats, x, d.HW * B * N))
    throw std::runtime_error(fmt("%s: the weight gradient overlaps an input", who));
  launchRxgWgrad(*h->frontend, B, H, W, static_cast<int>(N), static_cast<int>(N), channelsPerGroup, channelsPerGroup, 3, stride, gy, x,
                 split, gWeight, s);
}

// The dense convolutions' input gradient: 1 x 1 at stride 1 or 2 (the stem's images need none).  gy [B][N][Ho][Wo], weight
// [N][Cin][1][1], add (or null) [B][Cin][H][W] -> gx [B][Cin][H][W] = conv_transpose(gy) + add.  Stride 1 is the decoder's input
// gradient; stride 2 runs it at Ho x Wo into scratch and k_rxg_scatter2 places it at the even positions.
void resnextConvGradInputDevice(cvd_handle* h, int B, int H, int W, int inChannels, int outChannels, int kernelSize, int stride,
                                const float* gy, const float* weight, const float* add, float* gx, hipStream_t s) {
  const char* who = "resnext conv grad input";
  const RxDims d = checkRxShape(who, B, H, W, stride);
  if (kernelSize != 1) throw std::runtime_error(fmt("%s: kernel_size must be 1: the stem's input gradient is not built (got %d)", who, kernelSize));
  checkRxChannels(who, inChannels, outChannels, 1, stride, d.M);
  if (stride == 1) {
    midasConvGradInputDevice(h, B, H, W, inChannels, outChannels, 1, gy, weight, add, nullptr, 0, gx, s);
    return;
  }
  const long long total = checkRxgPlanes(who, B, inChannels, H, W);
  if (!gy || !weight || !gx) throw std::runtime_error(fmt("%s: null array", who));
  if (rangesOverlap(gx, total, gy, d.M * outChannels)) throw std::runtime_error(fmt("%s: gx overlaps gy", who));
  if (rangesOverlap(gx, total, weight, static_cast<long long>(inChannels) * outChannels)) throw std::runtime_error(fmt("%s: gx overlaps the weight", who));
  if (add && rangesOverlap(gx, total, add, total)) throw std::runtime_error(fmt("%s: gx overlaps the addend", who));
  Frontend& fe = *h->frontend;
  fe.dRxGrad.ensure(static_cast<size_t>(d.M) * inChannels);
  midasConvGradInputDevice(h, B, d.Ho, d.Wo, inChannels, outChannels, 1, gy, weight, nullptr, nullptr, 0, fe.dRxGrad.p, s);
  RxgStrideArgs A{};
  A.in = fe.dRxGrad.p; A.add = add; A.out = gx; A.H = H; A.W = W; A.Ho = d.Ho; A.Wo = d.Wo; A.total = total;
  hipLaunchKernelGGL(k_rxg_scatter2, dim3(static_cast<unsigned>((total + kRgThreads - 1) / kRgThreads)), dim3(kRgThreads), 0, s, A);
  HIP_CHECK(hipGetLastError());
}

// The dense convolutions' weight gradient: gy [B][N][Ho][Wo], x [B][Cin][H][W] -> gWeight [N][Cin][k][k].  1 x 1 at stride 1 is the
// decoder's weight gradient; at stride 2 the same on x gathered at the even positions; the 7 x 7 stem runs k_rxg_wgrad.
void resnextConvGradWeightDevice(cvd_handle* h, int B, int H, int W, int inChannels, int outChannels, int kernelSize, int stride,
                                 const float* gy, const float* x, int split, float* gWeight, hipStream_t s) {
  const char* who = "resnext conv grad weight";
  const RxDims d = checkRxShape(who, B, H, W, stride);
  checkRxChannels(who, inChannels, outChannels, kernelSize, stride, d.M);
  if (kernelSize == 7 && (split < 0 || split > kRgWgradMaxSplit))       // (the 1 x 1 paths' split is checked by the path they run)
    throw std::runtime_error(fmt("%s: split must be 0 (the rule) or 1 .. %d (got %d)", who, kRgWgradMaxSplit, split));
  if (kernelSize == 1 && stride == 1) {
    midasConvGradWeightDevice(h, B, H, W, inChannels, outChannels, 1, gy, x, 0, split, gWeight, nullptr, s);
    return;
  }
  if (!gy || !x || !gWeight) throw std::runtime_error(fmt("%s: null array", who));
  const long long wFloats = static_cast<long long>(inChannels) * outChannels * kernelSize * kernelSize;
  if (rangesOverlap(gWeight, wFloats, gy, d.M * outChannels) || rangesOverlap(gWeight, wFloats, x, d.HW * B * inChannels))
    throw std::runtime_error(fmt("%s: the weight gradient overlaps an input", who));
  Frontend& fe = *h->frontend;
  if (kernelSize == 7) {
    if ((wFloats + kRgThreads - 1) / kRgThreads > 0x7fffffffll) throw std::runtime_error(fmt("%s: %lld weights exceed the grid", who, wFloats));
    launchRxgWgrad(fe, B, H, W, inChannels, outChannels, inChannels, outChannels, 7, 2, gy, x, split, gWeight, s);
    return;
  }
  checkRxgPlanes(who, B, inChannels, d.Ho, d.Wo);
  fe.dRxGrad.ensure(static_cast<size_t>(d.M) * inChannels);
  RxgStrideArgs A{};
  A.in = x; A.out = fe.dRxGrad.p; A.H = H; A.W = W; A.Ho = d.Ho; A.Wo = d.Wo; A.total = d.M * inChannels;
  hipLaunchKernelGGL(k_rxg_gather2, dim3(static_cast<unsigned>((A.total + kRgThreads - 1) / kRgThreads)), dim3(kRgThreads), 0, s, A);
  HIP_CHECK(hipGetLastError());
  midasConvGradWeightDevice(h, B, d.Ho, d.Wo, inChannels, outChannels, 1, gy, fe.dRxGrad.p, 0, split, gWeight, nullptr, s);
}

// x [B][channels][H][W], gy [B][channels][Ho][Wo] -> gx [B][channels][H][W]
void resnextMaxPoolGradDevice(cvd_handle*, int B, int channels, int H, int W, const float* x, const float* gy, float* gx, hipStream_t s) {
  const char* who = "resnext maxpool grad";
  const long long total = checkRxgPlanes(who, B, channels, H, W);
  const RxDims d = checkRxShape(who, B, H, W, 2);
  if (!x || !gy || !gx) throw std::runtime_error(fmt("%s: null array", who));
  const long long planes = static_cast<long long>(B) * channels;
  if (rangesOverlap(gx, total, x, total)) throw std::runtime_error(fmt("%s: gx overlaps x", who));
  if (rangesOverlap(gx, total, gy, planes * d.HWo)) throw std::runtime_error(fmt("%s: gx overlaps gy", who));
  RxgPoolArgs A{};
  A.x = x; A.gy = gy; A.out = gx; A.H = H; A.W = W; A.Ho = d.Ho; A.Wo = d.Wo; A.total = total;
  hipLaunchKernelGGL(k_rxg_maxpool_grad, dim3(static_cast<unsigned>((total + kRgThreads - 1) / kRgThreads)), dim3(kRgThreads), 0, s, A);
  HIP_CHECK(hipGetLastError());
}

// ---- One Bottleneck per call.  weights: conv1, conv2, conv3 (and downsample.0); norms: 4 vectors per convolution {weight, bias,
// running_mean, running_var}; training: one flag per norm; saved: 4 tensors per convolution {c, mean, invstd, post-activation}, the
// post-activation of conv3 being the block's output (api.resnext_block_saved_shapes).  Both calls run the operator entry points
// above in order, so their results are the chained operators' bit for bit. ---------------------------------------------------------
namespace {
struct RxBlockDims {
  int n, cg, Ho, Wo;
  long long mIn, mOut;
};

RxBlockDims checkRxBlock(const char* who, int B, int H, int W, int inChannels, int width, int outChannels, int groups, int stride,
                         int downsample) {
  const RxDims d = checkRxShape(who, B, H, W, stride);
  checkFlag(who, "downsample", downsample);
  if (inChannels < 1 || width < 1 || outChannels < 1 || groups < 1)
    throw std::runtime_error(fmt("%s: in_channels, width, out_channels and groups must be >= 1 (got %d, %d, %d, %d)", who, inChannels,
                                 width, outChannels, groups));
  if (width % groups) throw std::runtime_error(fmt("%s: width %d is no whole groups of %d", who, width, groups));
  if (!downsample && (stride != 1 || inChannels != outChannels))
    throw std::runtime_error(fmt("%s: without a downsample branch stride must be 1 and in_channels == out_channels (got %d, %d, %d)", who,
                                 stride, inChannels, outChannels));
  checkRxGroups(who, groups, width / groups, d.HW * B);
  return {downsample ? 4 : 3, width / groups, d.Ho, d.Wo, d.HW * B, d.M};
}
}  // namespace

void resnextBlockTrainDevice(cvd_handle* h, int B, int H, int W, int inChannels, int width, int outChannels, int groups, int stride,
                             int downsample, const float* x, const float* const* weights, float* const* norms, double eps,
                             double momentum, const int* training, float* const* saved, hipStream_t s) {
  const char* who = "resnext block train";
  const RxBlockDims d = checkRxBlock(who, B, H, W, inChannels, width, outChannels, groups, stride, downsample);
  if (!x || !weights || !norms || !training || !saved) throw std::runtime_error(fmt("%s: null array", who));
  for (int i = 0; i < d.n; ++i) {
    if (!weights[i]) throw std::runtime_error(fmt("%s: null weight %d", who, i));
    for (int j = 0; j < 4; ++j) {
      if (!norms[4 * i + j]) throw std::runtime_error(fmt("%s: null norm vector %d of convolution %d", who, j, i));
      if (!saved[4 * i + j]) throw std::runtime_error(fmt("%s: null saved tensor %d of convolution %d", who, j, i));
    }
  }
  const long long counts[4] = {d.mIn * width, d.mOut * width, d.mOut * outChannels, d.mOut * outChannels};
  for (int i = 0; i < d.n; ++i)
    for (int j = 0; j < 4; j += 3) {
      if (rangesOverlap(saved[4 * i + j], counts[i], x, d.mIn * inChannels))
        throw std::runtime_error(fmt("%s: saved tensor %d of convolution %d overlaps x", who, j, i));
      for (int k = 0; k < 4 * i + j; ++k)
        if (k % 4 == 0 || k % 4 == 3)
          if (rangesOverlap(saved[4 * i + j], counts[i], saved[k], counts[k / 4]))
            throw std::runtime_error(fmt("%s: saved tensors %d and %d overlap", who, 4 * i + j, k));
    }
  const float fe = static_cast<float>(eps);
  const auto norm = [&](int i, int channels, int hh, int ww, int relu, const float* residual) {
    resnextNormTrainDevice(h, B, channels, hh, ww, saved[4 * i], norms[4 * i], norms[4 * i + 1], norms[4 * i + 2], norms[4 * i + 3], eps,
                           momentum, training[i], relu, residual, saved[4 * i + 1], saved[4 * i + 2], saved[4 * i + 3], s);
  };
  resnextConvDevice(h, B, H, W, inChannels, width, 1, 1, x, weights[0], nullptr, fe, 0, nullptr, 0, saved[0], s);
  norm(0, width, H, W, 1, nullptr);
  resnextGroupedConvDevice(h, B, H, W, groups, d.cg, stride, saved[3], weights[1], nullptr, fe, 0, saved[4], s);
  norm(1, width, d.Ho, d.Wo, 1, nullptr);
  const float* identity = x;
  if (downsample) {
    resnextConvDevice(h, B, H, W, inChannels, outChannels, 1, stride, x, weights[3], nullptr, fe, 0, nullptr, 0, saved[12], s);
    norm(3, outChannels, d.Ho, d.Wo, 0, nullptr);
    identity = saved[15];
  }
  resnextConvDevice(h, B, d.Ho, d.Wo, width, outChannels, 1, 1, saved[7], weights[2], nullptr, fe, 0, nullptr, 0, saved[8], s);
  norm(2, outChannels, d.Ho, d.Wo, 0, identity);
}

// gy [B][out][Ho][Wo] -> gx (or null) [B][in][H][W], gWeights[n], gGammas[n], gBetas[n]: bn3 (mask = the block's output, which yields
// the residual branch's gradient), conv3, bn2, conv2, bn1, conv1; conv1's input gradient takes that gradient, or the downsample
// branch's input gradient, as its addend.
void resnextBlockBackwardDevice(cvd_handle* h, int B, int H, int W, int inChannels, int width, int outChannels, int groups, int stride,
                                int downsample, const float* gy, const float* x, const float* const* weights, const float* const* gammas,
                                const float* const* saved, const int* training, float* gx, float* const* gWeights,
                                float* const* gGammas, float* const* gBetas, hipStream_t s) {
  const char* who = "resnext block backward";
  const RxBlockDims d = checkRxBlock(who, B, H, W, inChannels, width, outChannels, groups, stride, downsample);
  if (!gy || !x || !weights || !gammas || !saved || !training || !gWeights || !gGammas || !gBetas)
    throw std::runtime_error(fmt("%s: null array", who));
  for (int i = 0; i < d.n; ++i) {
    if (!weights[i] || !gammas[i] || !gWeights[i] || !gGammas[i] || !gBetas[i]) throw std::runtime_error(fmt("%s: null array of convolution %d", who, i));
    for (int j = 0; j < 4; ++j)
      if (!saved[4 * i + j]) throw std::runtime_error(fmt("%s: null saved tensor %d of convolution %d", who, j, i));
  }
  Frontend& fe = *h->frontend;
  const size_t big = static_cast<size_t>(d.mOut) * outChannels, mid = static_cast<size_t>(d.mOut) * width,
               wide = static_cast<size_t>(d.mIn) * width, in = static_cast<size_t>(d.mIn) * inChannels;
  fe.dRxBlock.ensure(3 * big + 2 * mid + 2 * wide + in);
  float* gc3 = fe.dRxBlock.p;
  float* gres = gc3 + big;
  float* gcd = gres + big;
  float* g2 = gcd + big;
  float* gc2 = g2 + mid;
  float* g1 = gc2 + mid;
  float* gc1 = g1 + wide;
  float* gxd = gc1 + wide;
  const auto norm = [&](int i, int channels, int hh, int ww, const float* g, bool mask, float* gc, float* gr) {
    resnextNormGradDevice(h, B, channels, hh, ww, g, saved[4 * i], mask ? saved[4 * i + 3] : nullptr, saved[4 * i + 1], saved[4 * i + 2],
                          gammas[i], training[i], gc, gGammas[i], gBetas[i], gr, s);
  };
  norm(2, outChannels, d.Ho, d.Wo, gy, true, gc3, gres);
  resnextConvGradWeightDevice(h, B, d.Ho, d.Wo, width, outChannels, 1, 1, gc3, saved[7], 0, gWeights[2], s);
  resnextConvGradInputDevice(h, B, d.Ho, d.Wo, width, outChannels, 1, 1, gc3, weights[2], nullptr, g2, s);
  norm(1, width, d.Ho, d.Wo, g2, true, gc2, nullptr);
  resnextGroupedConvGradWeightDevice(h, B, H, W, groups, d.cg, stride, gc2, saved[3], 0, gWeights[1], s);
  resnextGroupedConvGradInputDevice(h, B, H, W, groups, d.cg, stride, gc2, weights[1], g1, s);
  norm(0, width, H, W, g1, true, gc1, nullptr);
  resnextConvGradWeightDevice(h, B, H, W, inChannels, width, 1, 1, gc1, x, 0, gWeights[0], s);
  const float* add = gres;
  if (downsample) {
    norm(3, outChannels, d.Ho, d.Wo, gres, false, gcd, nullptr);
    resnextConvGradWeightDevice(h, B, H, W, inChannels, outChannels, 1, stride, gcd, x, 0, gWeights[3], s);
    if (gx) resnextConvGradInputDevice(h, B, H, W, inChannels, outChannels, 1, stride, gcd, weights[3], nullptr, gxd, s);
    add = gxd;
  }
  if (gx) resnextConvGradInputDevice(h, B, H, W, inChannels, width, 1, 1, gc1, weights[0], add, gx, s);
}

// One kernel of this translation unit's code object is looked up at handle creation: the HIP runtime loads a unit's device
// code at its first use, ~20 ms per unit that would otherwise land in the first solve of a process (cvd_create: loadDeviceCode).
void touchModule_frontend() {
  hipFuncAttributes a;
  (void)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(k_bgr_to_gray));
}

}  // namespace cvd
