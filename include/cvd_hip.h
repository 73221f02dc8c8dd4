/*
 * cvd_hip.h -- C ABI of the MI355X-native geometric-consistency optimizer (libcvd_hip.so).
 *
 * Drop-in boundary for ONE hot path of facebookresearch/robust_cvd: the pose / depth-deformation
 * optimizer behind DepthVideoProcessor::{normalizeDepth, optimizePoses} (reference lib/Processor.cpp:1015-1025)
 * i.e. DepthVideoPoseOptimizer (reference lib/PoseOptimizer.h:52-124, lib/PoseOptimizer.cpp), with the
 * transform model of lib/DepthMapTransform.{h,cpp} and the constraint container of lib/FlowConstraints.h.
 *
 * The reference exposes this path through a pybind11 class surface (lib/PythonBindings.cpp:170-555), not a
 * C ABI.  Each entry point below names the reference interface it replaces; INTEGRATION.md shows the
 * reference-side stub (C++ and ctypes) a maintainer would add.  Handle-based, plain pointers and sizes,
 * host buffers in / host buffers out; all device memory, streams and kernels are owned by the handle.
 * Every function returns 0 on success and -1 on error (message: cvd_last_error), never aborts.
 */
#ifndef CVD_HIP_H_
#define CVD_HIP_H_

#include "cvd_types.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct cvd_handle_t cvd_handle;

/* Inner linear solver / LM knobs that have no counterpart in the reference (Ceres' SPARSE_NORMAL_CHOLESKY
 * is replaced by a block-Jacobi preconditioned conjugate-gradient solve on the device). */
typedef struct cvd_solver_options {
  uint64_t struct_size;          /* CVD_STRUCT_STAMP(cvd_solver_options) of the header the CALLER was built with -- sizeof in the low
                                    32 bits, CVD_ABI_REVISION in the high 32 (round 6, ADVICE r5: removing one int32 left sizeof
                                    unchanged behind the padding, so the size alone could not tell the revisions apart) -- set by
                                    cvd_solver_options_default, checked by cvd_set_solver_options: a caller built against another
                                    revision of this header is refused instead of being read with shifted fields */
  double pcg_relative_tolerance; /* eta: the PCG stops when sqrt(r^T M^-1 r) <= eta * its initial value.  Default 1e-3:
                                    the reference's SPARSE_NORMAL_CHOLESKY takes EXACT LM steps, and the iterate at which
                                    function_tolerance (1e-6 relative cost change) stops them is only reproduced -- to the
                                    1e-3 pose tolerance of BASELINE.json -- when every step is this accurate.  On BASELINE
                                    configs[0..2] 5e-3 sufficed (round 2's default); on the BENCHMARKED 4140-pair problem it
                                    takes one LM iteration more than the exact-step solve and ends 2.0e-3 away, 2e-3 likewise,
                                    1e-3 ends within 8.5e-5 (config0/1/2: 3.7e-5 / 6.1e-6 / 6.1e-6): profiles/r03_parity_probe.log,
                                    DESIGN.md 4.  Ceres' own inexact-step default is 0.1. */
  int32_t pcg_max_iterations;    /* default 300 */
  int32_t verbose;               /* 1: print a Ceres-like per-iteration table to stdout; 2: + PCG scalars per iteration;
                                    3: + setup phases and the shape of the coarse elimination (development) */
  int32_t coarse_level;          /* 1 (default): block-Jacobi + a pose-graph coarse solve (8 unknowns per frame) -- the EXACT
                                    block-sparse factor while its elimination is cheap, else what coarse_over_budget names
                                    (default: the temporal pose level); rebuilt on demand; 2: the same rebuilt every LM
                                    iteration; 3: ALWAYS the TEMPORAL pose level -- the same 8 modes per frame x temporal hat
                                    functions with a node every coarse_temporal_step frames (312 unknowns instead of 2400 at 300
                                    frames), inverted densely, applied inside the PCG launches (cvd_temporal.h);
                                    0: block-Jacobi only */
  int32_t robust_loss;           /* robust loss on the static flow constraints, parameter = cvd_opt_params::robustness:
                                    0 (default) ceres::CauchyLoss, what the reference hard-wires
                                    (lib/PoseOptimizer.cpp:1220); 1 ceres::HuberLoss, the stress variant of BASELINE.json
                                    configs[4] (no counterpart in the reference) */
  /* ---- POLICY: which of the library's variants a solve uses.  The defaults are the product path (chosen on the benchmarked video,
   * held off it by tools/defaults_sweep.py: DESIGN.md 8); a caller has no reason to touch anything below this line.  Test and
   * measurement hooks are NOT here: include/cvd_hip_debug.h ---- */
  int32_t dense_matrix_free;      /* dense mode: 1 = matrix-free products everywhere (no explicit cross blocks) */
  int32_t block_inverse_variant;  /* 0: MFMA blocked sweep (default); 1: scalar register-resident sweep */
  int32_t coarse_dense_max_unknowns; /* the coarse level is inverted as ONE dense matrix up to this many unknowns
                                     (8 per frame) when its sparse elimination is too expensive; default 4096 */
  int32_t coarse_rebuild_excess;  /* coarse_level 1: the coarse level is rebuilt once the PCG iterations spent beyond the count seen
                                     right after the last rebuild add up to this many (about what a rebuild costs); default 16 */
  int64_t coarse_update_budget;   /* 8x8 block updates of the sparse elimination beyond which the coarse level goes dense
                                     (or, beyond coarse_dense_max_unknowns, is built on a sparsified graph); default 40000 */
  double coarse_dense_shift;      /* dense coarse level: A_c + shift * diag(A_c) is what gets inverted (default 1e-5).  The level
                                     applies an EXPLICIT inverse, whose rounding errors scale with cond(A_c) / lambda_min: beyond
                                     cond ~ 1e8 (the damped matrix late in an LM run: the gauge directions carry only the
                                     damping) the stored inverse stops being positive definite and PCG stalls.  The shift
                                     bounds the condition number of the Jacobi-scaled matrix; as a preconditioner the level
                                     loses nothing on directions that carry gradient */
  int32_t constraint_order;       /* 1 (default): every pair's slice of the constraint table is re-ordered as a sweep over the
                                     cells of the depth grid (consecutive lanes of a wave hit different grid vertices: the
                                     LDS atomics of the pair-major kernels stop serialising); 0: the caller's order */
  int32_t coarse_rebuild_excess_dense; /* the same threshold for the DENSE coarse level, whose rebuild is one in-line kernel chain
                                     (1.9 ms at 300 frames), not a side-stream job.  0 (default): 32, a constant -- identical inputs
                                     take identical rebuild decisions on every run and rank.  > 0: that many.  -1 (opt-in, one GPU):
                                     1.5 x the cost ratio MEASURED on this handle (duration of a rebuild / duration of a PCG
                                     iteration), in steps of 8; wall-clock dependent, so PCG counts may differ run to run */
  int32_t pcg_fused_tail;         /* 1 (default): the two per-frame kernels of a PCG iteration (finish of the product, update) run
                                     as ONE launch with a grid barrier between their halves (k_pcg_tail) where its scope allows --
                                     one GPU, frame block <= 256, dense coarse level or none, every workgroup resident; 0: always
                                     the two launches.  A handle whose fused tail ever abandons its barrier (device shared with
                                     other work) falls back to the two launches for good and repeats the solve (a warning on
                                     stderr) */
  int32_t coarse_dense_row_split; /* dense coarse level, per PCG iteration: of a frame's 8 rows of A_c^-1 the first this-many are applied by
                                     the dense-level workgroups (two frames each), the others by the frame's own workgroup after its
                                     update (default 5; 8 = rounds 2-3: dense-level workgroups only; 0 = frame workgroups only) */
  int32_t dist_owner_update;      /* pair-sharded multi-GPU solves, 1 (default): the per-frame update of a PCG iteration runs on the
                                     frames' OWNER ranks only -- q reduce-scattered to the owners, z / c / the r^T z shares all-gathered
                                     (two grouped collectives per iteration); 0: q all-reduced and the update replicated on every
                                     rank (one collective per iteration; rounds 2-3) */
  int32_t temporal_level;         /* third level of the preconditioner (cvd_temporal.h): temporal hat functions (one node every
                                     temporal_step frames) x bilinear hats of a coarse grid on the depth grid, its Galerkin matrix
                                     inverted densely, applied inside the PCG launches.  0: off; 1: rebuilt whenever the pose-graph
                                     level is (in line or on the side stream) -- without a pose-graph level (coarse_level 0) by the
                                     same excess-iterations rule; 2: rebuilt every LM iteration.  Scope (temporalScope,
                                     cvd_temporal.hip): list mode or dense mode with explicit cross blocks, one GPU or pair-sharded,
                                     any form of the pose-graph level or none; fast-path problems only -- bilinear one-parameter
                                     depth grid of at least 3 x 3 vertices, identity spatial transform, reprojection losses, Fixed /
                                     PerFrame intrinsics, no triplets, no position regulariser, more than 2 temporal_step frames;
                                     elsewhere the option is ignored */
  int32_t temporal_step;          /* frames between two temporal nodes (default 32) */
  int32_t temporal_grid_x;        /* coarse hats per axis; 0 (default): (grid + 1) / 2 */
  int32_t temporal_grid_y;
  int32_t coarse_temporal_step;   /* temporal pose level: frames between two temporal nodes (default 8) */
  int32_t coarse_over_budget;     /* coarse_level 1 / 2, what replaces the exact block-sparse factor when its elimination exceeds
                                     coarse_update_budget (flow lists with long-range pairs from nearly every frame).  0 (default):
                                     the TEMPORAL pose level (see coarse_level 3); 1: rounds 2-3 -- the exact level as ONE dense
                                     inverse up to coarse_dense_max_unknowns, on a sparsified graph beyond */
  int32_t coarse_temporal_min_frames; /* coarse_level 1 / 2 on ONE GPU with frame blocks <= 256: from this many frames on (default 128;
                                     0: never) the temporal pose level is used even where the exact factor is cheap -- it brings
                                     the PCG iteration inside k_pcg_tail's scope (one launch for finish + update), which the exact
                                     sparse level is not: 1766-pair list at 300 frames 296 -> 331 LM iterations/s at 37.6 -> 39.8
                                     PCG iterations.  Beyond ~400 frames the fused kernel's workgroups are no longer co-resident
                                     and the exact factor stays (configs[4]: 52.9 against 47 iterations/s) */
  double temporal_weight;         /* the temporal levels (depth-grid level, temporal pose level) enter the additive preconditioner
                                     as weight x P A^-1 P^T: their spaces overlap each other's and the per-frame blocks', and an
                                     additive combination of overlapping exact corrections overshoots (default 0.7: 5 - 8 % fewer
                                     PCG iterations than 1.0 on the benchmarked problem) */
} cvd_solver_options;

/* Revision of this header's binary interface: bumped whenever a struct layout or an entry point's meaning changes (round 4: 4 --
 * cvd_solver_options gained struct_size as its FIRST field; round 5: 5 -- pcg_check_every removed, cvd_path_info added; round 6: 6 --
 * the test / measurement hooks left cvd_solver_options for cvd_debug_options (cvd_hip_debug.h), struct_size carries the revision,
 * cvd_get_dense_times added).  cvd_abi_revision() returns the revision the LIBRARY was built with; bindings compare it with the
 * header they were written against before any struct crosses the boundary (robust_cvd_amd/api.py does at load). */
#define CVD_ABI_REVISION 6
#define CVD_STRUCT_STAMP(T) ((uint64_t)sizeof(T) | ((uint64_t)CVD_ABI_REVISION << 32))
int32_t cvd_abi_revision(void);

/* ---- lifetime ------------------------------------------------------------------------------------- */
/* One optimizer per DepthVideo + depth stream (reference: DepthVideoPoseOptimizer ctor,
 * lib/PoseOptimizer.cpp:748-783). `device` = HIP device ordinal. Fails (NULL) when no GPU is usable. */
cvd_handle* cvd_create(int32_t device);
void cvd_destroy(cvd_handle* h);
const char* cvd_last_error(cvd_handle* h);
/* sizeof() of the ABI structs as compiled, for binding self-checks: fills 6 ints
 * {xform_desc, opt_params, frame_pose, iteration_record, solve_summary, solver_options}. */
void cvd_abi_sizes(int32_t* out6);
void cvd_opt_params_default(cvd_opt_params* p);       /* reference lib/PoseOptimizer.h:55-103 defaults */
void cvd_solver_options_default(cvd_solver_options* o);
int32_t cvd_set_solver_options(cvd_handle* h, const cvd_solver_options* o);

/* ---- multi-GPU: one process per GPU, frame pairs sharded across ranks ---------------------
 * Every rank holds all frames (depth, parameters) but only ITS pairs (cvd_set_pair_constraints with the shard);
 * the regularisers of frame f belong to rank f % world; frames are OWNED in contiguous chunks of ceil(F / world).  Per
 * Jacobian evaluation the library all-reduces g and the per-frame costs, reduce-scatters H_ff to the frames' owners and
 * all-gathers diag(H) and the owners' f32 block inverses; per PCG iteration it reduce-scatters q to the owners (with
 * [Z^T q | p.q] all-reduced in the same group), updates the owners' frames and all-gathers z / c / the r^T z shares -- two
 * grouped collectives over RCCL on the solver's stream.  The reference has no counterpart (single process).  Rank 0 creates the id, the caller broadcasts the 128 bytes (any transport). */
void cvd_comm_unique_id(uint8_t* out128);
int32_t cvd_comm_init(cvd_handle* h, int32_t rank, int32_t world, const uint8_t* id128);
/* Pair-sharded mode only: the frame pairs of the WHOLE problem (2 * num_pairs frame indices, direction and order
 * irrelevant), identical on every rank.  The coarse level of the preconditioner is built on this graph; without it
 * a multi-rank solve falls back to the block-Jacobi level alone.  Call after cvd_set_video. */
int32_t cvd_set_pair_graph(cvd_handle* h, int32_t num_pairs, const int32_t* pair_frames);

/* ---- inputs (what the reference reads through DepthVideo / DepthStream / FlowConstraintsCollection) -- */
/* DepthVideo dims + aspect (reference lib/DepthVideo.h: numFrames(), aspect(), invAspect(); DepthStream w/h). */
int32_t cvd_set_video(cvd_handle* h, int32_t num_frames, int32_t width, int32_t height, float aspect,
                      float inv_aspect);
/* DepthFrame::sourceDepth() of one frame: width*height floats, row-major, depth (not disparity), invalid = 0
 * (reference lib/DepthStream.cpp:176-216). Copied to HBM; the per-frame median used by the scale
 * regulariser (lib/PoseOptimizer.cpp:1363-1375) is taken here. */
int32_t cvd_set_depth(cvd_handle* h, int32_t frame, const float* depth);
/* All frames at once, depth = [F][H][W] contiguous: one host->device copy instead of F (same semantics as F calls of
 * cvd_set_depth; the reference keeps one cv::Mat1f per DepthFrame, lib/DepthStream.h, so its binding copies frame by frame). */
int32_t cvd_set_depth_all(cvd_handle* h, const float* depth);
/* FlowConstraintsCollection pair constraints (reference lib/FlowConstraints.h:41-205): pair-major,
 * pair_frames[2*P], offsets[P+1], loc4[4*C] = (loc0.xy, loc1.xy) in [0,1]x[0,invAspect], is_static[C] or NULL. */
int32_t cvd_set_pair_constraints(cvd_handle* h, int32_t num_pairs, const int32_t* pair_frames,
                                 const int64_t* offsets, const float* loc4, const uint8_t* is_static);
/* Dense mode -- the reference's matchSeparation = 0 regime (lib/FlowConstraints.cpp:315-329: buildDiskMask(0) is a 1x1 disk,
 * so every masked pixel whose flow target rounds into the image becomes a constraint, :381-465).  Instead of a constraint
 * list the optimizer is handed the flow and mask images of every directed pair -- flow[P][H][W][2] f32 in pixels,
 * mask[P][H][W] u8 (non-zero = valid), at the size given to cvd_set_video -- and its kernels read flow / mask / depth
 * directly (17 B per pixel pair); nothing is sampled or tabulated.  Every constraint is static.  Replaces the constraint
 * list (cvd_set_pair_constraints switches back).  A solve outside the scope of the image-reading kernels (see
 * cvd_dense_mode_supported) writes the list the images stand for on the device (44 B per constraint) and runs on the list kernels. */
int32_t cvd_set_pair_flows(cvd_handle* h, int32_t num_pairs, const int32_t* pair_frames, const float* flow, const uint8_t* mask);
/* 1 when a problem with these parameters / transform descriptors lies within the scope of the dense mode (identity spatial
 * transform, a reprojection loss, Scale value transform, Global or bilinear grid, per-frame or fixed intrinsics, no
 * smoothness triplets, frame block <= 199 -- a frame's packed triangle in LDS --): its kernels read the images directly.  0: a dense-mode solve still runs, on the
 * constraint list materialised on the device (pixel order, 6.4 GB for 144 M constraints); a caller that holds the list
 * anyway may as well hand it over (cvd_set_pair_constraints).  problem: 0 = poseOptimization, 1 = normalizeDepth.
 * What lib_python's FlowConstraintsCollection asks before it keeps a matchSeparation = 0 collection as images. */
int32_t cvd_dense_mode_supported(const cvd_opt_params* params, const cvd_xform_desc* depth, const cvd_xform_desc* spatial,
                                 int32_t have_triplets, int32_t world_size, int32_t problem);
/* Triplet constraints (reference lib/FlowConstraints.h:109-111), keyed by centre frame; loc6[6*C]. */
int32_t cvd_set_triplet_constraints(cvd_handle* h, int32_t num_triplets, const int32_t* centers,
                                    const int64_t* offsets, const float* loc6, const uint8_t* is_static);
/* Dynamic masks of all frames, masks[F][height][width] u8 (the `dynamic_mask` colour stream; NULL forgets them):
 * used by AdaptiveDeformationCost when params.adaptive_deformation_cost > 0 (reference lib/PoseOptimizer.cpp:559-656,
 * 1449-1491; "Adaptive smoothness requires a dynamic mask stream." without them).  Call after cvd_set_video. */
int32_t cvd_set_dynamic_masks(cvd_handle* h, int32_t height, int32_t width, const uint8_t* masks);

/* ---- per-frame state (DepthFrame::{extrinsics,intrinsics,depthXform(),spatialXform()}) --------------- */
int32_t cvd_set_poses(cvd_handle* h, const cvd_frame_pose* poses /* [F] */);
int32_t cvd_get_poses(cvd_handle* h, cvd_frame_pose* poses /* [F] */);
/* DepthVideoProcessor::resetPoses (reference lib/Processor.cpp:987-1003) */
int32_t cvd_reset_poses(cvd_handle* h, double focal_long);
/* DepthStream::resetDepthXforms / resetSpatialXforms (reference lib/DepthStream.cpp:368-383) */
int32_t cvd_reset_depth_xforms(cvd_handle* h, const cvd_xform_desc* desc);
int32_t cvd_reset_spatial_xforms(cvd_handle* h, const cvd_xform_desc* desc);
/* DepthVideoProcessor::gridXformSplit (reference lib/Processor.cpp:888-985) */
int32_t cvd_grid_xform_split(cvd_handle* h, const cvd_xform_desc* desc);
int32_t cvd_get_xform_desc(cvd_handle* h, int32_t spatial, cvd_xform_desc* desc);
int32_t cvd_num_xform_params(cvd_handle* h, int32_t spatial);          /* Xform::numParams() */
int32_t cvd_get_xform_params(cvd_handle* h, int32_t spatial, double* out /* [F x numParams] */);
int32_t cvd_set_xform_params(cvd_handle* h, int32_t spatial, const double* in /* [F x numParams] */);
/* Internal 7-tuples (t, angle-axis, tan(vFov/2)) of reference lib/PoseOptimizer.h:149, [F x 7] doubles. */
int32_t cvd_get_pose_params(cvd_handle* h, double* pose7);
int32_t cvd_set_pose_params(cvd_handle* h, const double* pose7); /* continue a solve from saved tuples */
int32_t cvd_block_size(cvd_handle* h); /* unknowns per frame: 7 + depth params + spatial params */

/* ---- the path --------------------------------------------------------------------------------------- */
/* DepthVideoPoseOptimizer::normalizeDepth (reference lib/PoseOptimizer.cpp:992-1147) */
int32_t cvd_normalize_depth(cvd_handle* h, const cvd_opt_params* params);
/* DepthVideoPoseOptimizer::poseOptimization (reference lib/PoseOptimizer.cpp:788-888) */
int32_t cvd_pose_optimization(cvd_handle* h, const cvd_opt_params* params);
/* DepthVideoPoseOptimizer::poseOptimizationStep (reference lib/PoseOptimizer.cpp:890-990).
 * convert_poses != 0: rebuild the internal 7-tuples from the float poses first (what constructing a new
 * DepthVideoPoseOptimizer does); 0: continue from the double-precision tuples of the previous step. */
int32_t cvd_pose_optimization_step(cvd_handle* h, const cvd_opt_params* params, double depth_deform_reg,
                                   int32_t convert_poses);
/* Parity hook: cost, gradient (F x B) and per-frame J^T J blocks (F x B x B) of the poseOptimizationStep
 * problem at the current state (pose7 != NULL overrides the 7-tuples). Any output pointer may be NULL.
 * hfull ((F*B)^2, small problems only) is produced by F*B device mat-vec products with unit vectors. */
int32_t cvd_evaluate(cvd_handle* h, const cvd_opt_params* params, double depth_deform_reg,
                     const double* pose7, double* cost, int32_t* num_residual_blocks, double* gradient,
                     double* hdiag, double* hfull);
int32_t cvd_get_summary(cvd_handle* h, cvd_solve_summary* s);
int32_t cvd_num_records(cvd_handle* h);
int32_t cvd_get_records(cvd_handle* h, cvd_iteration_record* out);

/* ---- constraint sampling: FlowConstraintsCollection::compute(PairKey), reference
 * lib/FlowConstraints.cpp:296-465.  Images have the size given to cvd_set_video.  Inputs (host): corner[F][H][W] =
 * cornerMinEigenVal response of every frame's colour image (computed by the caller), flow[P][H][W][2] and mask[P][H][W]
 * of every directed pair (pair_frames[2P]), optionally dyn_dist[F][dyn_h][dyn_w] = distance transform of the dynamic
 * mask (NULL: no dynamic-mask stream).  offsets[P + 1] receives the constraint counts as a prefix sum; the constraints
 * (rank order per pair, loc0.xy loc1.xy scaled to [0,1]x[0,invAspect]) stay on the device until
 * cvd_get_sampled_constraints copies them out (loc4 holds offsets[P] x 4 floats).  Ties in the corner response resolve
 * by ascending pixel index (unspecified in the reference: std::sort). */
int32_t cvd_sample_pair_constraints(cvd_handle* h, int32_t num_pairs, const int32_t* pair_frames, const float* corner,
                                    const float* flow, const uint8_t* mask, const float* dyn_dist, int32_t dyn_w,
                                    int32_t dyn_h, int32_t match_separation, float min_dynamic_distance,
                                    int64_t* offsets);
int32_t cvd_get_sampled_constraints(cvd_handle* h, float* loc4);
/* FlowConstraintsCollection::compute(TripletKey), reference lib/FlowConstraints.cpp:467-550: centres[T] (frames c with
 * c-1 and c+1 inside the video), flow10 / mask10 = c -> c-1 and flow12 / mask12 = c -> c+1, each [T][H][W](x2).  Result:
 * offsets[T + 1] and, through cvd_get_sampled_triplet_constraints, loc6 = (loc(c-1), loc(c), loc(c+1)) per constraint.
 * The reference's two index slips are reproduced (corner response read at the column of the c-1 target; third
 * dynamic-distance test on frame c's map). */
int32_t cvd_sample_triplet_constraints(cvd_handle* h, int32_t num_triplets, const int32_t* centers, const float* corner,
                                       const float* flow10, const uint8_t* mask10, const float* flow12,
                                       const uint8_t* mask12, const float* dyn_dist, int32_t dyn_w, int32_t dyn_h,
                                       int32_t match_separation, float min_dynamic_distance, int64_t* offsets);
int32_t cvd_get_sampled_triplet_constraints(cvd_handle* h, float* loc6);

/* ---- image operators in front of the sampler: the two OpenCV calls of
 * FlowConstraintsCollection::compute.  Batches of num_images images of height x width, host buffers in and out
 * (out may be NULL: compute only), kernel_ms (may be NULL) = kernel time from HIP events. */
/* cvtColor(BGR2GRAY) + cornerMinEigenVal(gray, blockSize 3, Sobel aperture 3, BORDER_DEFAULT) of float BGR images
 * (reference lib/FlowConstraints.cpp:417-423): bgr [n][H][W][3] -> out [n][H][W], the `corner` input of the samplers. */
int32_t cvd_corner_min_eigenval(cvd_handle* h, int32_t num_images, int32_t height, int32_t width, const float* bgr,
                                float* out, double* kernel_ms);
/* FlowConstraintsCollection::dynamicDistance (reference lib/FlowConstraints.cpp:257-286): binarise the dynamic mask
 * (< 127 -> 0) and distanceTransform(DIST_L2, DIST_MASK_5) = 5x5 chamfer distance to the nearest zero pixel:
 * mask [n][H][W] u8 -> out [n][H][W] f32, the `dyn_dist` input of the samplers. */
int32_t cvd_dynamic_distance(cvd_handle* h, int32_t num_images, int32_t height, int32_t width, const uint8_t* mask,
                             float* out, double* kernel_ms);

/* ---- dense consumers of the result: what loaders/video_dataset.py reads after every optimisation --
 * All frames [first_frame, first_frame + num_frames) in one launch, current transform parameters of the handle, host
 * buffer out (may be NULL: compute only).  kernel_ms (may be NULL) receives the kernel time (HIP events).
 * Pixel-centre convention loc = (-1 + x 2/(w-1), 1 - y 2/(h-1)) of the reference. */
/* DepthXform::apply (reference lib/DepthMapTransform.cpp:394-415): out [n][H][W] f32 transformed depth. */
int32_t cvd_apply_depth_xforms(cvd_handle* h, int32_t first_frame, int32_t num_frames, float* out, double* kernel_ms);
/* GridDepthXform::paramMap (reference lib/DepthMapTransform.cpp:950-994): out [n][H][W][N] f64; Grid transforms only
 * ("Parameter map not implemented for this transform type." otherwise, :422-425). */
int32_t cvd_depth_param_maps(cvd_handle* h, int32_t first_frame, int32_t num_frames, double* out, double* kernel_ms);
/* SpatialXform::warp(h, w) (reference lib/DepthMapTransform.cpp:428-449): out [n][height][width][2] f32. */
int32_t cvd_spatial_warp_maps(cvd_handle* h, int32_t first_frame, int32_t num_frames, int32_t height, int32_t width,
                              float* out, double* kernel_ms);

/* DepthVideoProcessor::flowGuidedFilter (reference lib/Processor.cpp:315-590; Op::FlowGuidedFilter, the --post_filter of
 * the pipeline) with DepthVideo::project (reference lib/DepthVideo.cpp:637-681).  The batch holds num_frames CONSECUTIVE
 * frames: batch frame 0 must be video frame max(0, firstFrame - frame_radius) and the last batch frame the last frame
 * of the range (the reference's temporal window is [max(0, frame - radius), min(lastFrame, frame + radius)]); outputs
 * are produced for batch frames [first_output, first_output + num_outputs).
 *   depth    [n][depth_height][depth_width]  DepthFrame::depth() of the source stream (transformed depth)
 *   cameras  [n][9]  position xyz, orientation quaternion x y z w, hFov, vFov
 *   flow_fwd [n-1][height][width][2], mask_fwd [n-1][height][width]: flow / mask of (k -> k+1), pixels
 *   flow_bwd, mask_bwd: entry k = (k+1 -> k)
 *   out      [num_outputs][height][width] filtered depth (weighted mean, or weighted median if median != 0)
 * farConnections is not supported (the caller must reject it); the median holds at most 256 samples per pixel.
 * f32 in the reference's operation order; expf is the device function (float tolerance, not bit-exact). */
int32_t cvd_flow_guided_filter(cvd_handle* h, int32_t num_frames, int32_t first_output, int32_t num_outputs,
                               int32_t height, int32_t width, int32_t depth_height, int32_t depth_width, float inv_aspect,
                               const float* depth, const float* cameras, const float* flow_fwd, const uint8_t* mask_fwd,
                               const float* flow_bwd, const uint8_t* mask_bwd, int32_t frame_radius,
                               int32_t spatial_radius, int32_t median, float* out, double* kernel_ms);

/* DepthVideoProcessor::bilateralFilter (reference lib/Processor.cpp:183-313; Op::BilateralFilter, defaults
 * lib/Processor.h:64-70: frame_radius 2, spatial_radius 0, depth_sigma 0.3, color_sigma 0).  The batch holds num_frames
 * CONSECUTIVE frames; outputs are produced for batch frames [first_output, first_output + num_outputs), each from the window
 * [k - frame_radius, k + frame_radius] x [y - r, y + r] x [x - r, x + r] clipped to the batch and the image (the caller builds
 * the batch so that its ends are the video's ends or lie at least frame_radius away from every output).
 *   depth [n][height][width]     DepthFrame::depth() of depth stream 0 (transformed depth)
 *   color [n][height][width][3]  BGR f32 of the "down" colour stream; may be NULL when color_sigma <= 0
 *   out   [num_outputs][height][width] filtered depth (weighted mean, or weighted median if median != 0)
 * The median supports windows of up to 2048 samples per pixel ((2 spatial_radius + 1)^2 (2 min(frame_radius, n - 1) + 1));
 * larger windows are rejected before any work.  f32 in the reference's operation order; expf is the device function
 * (float tolerance on the mean, not bit-exact; the median returns one of the window's samples).  kernel_ms (may be NULL):
 * kernel time, HIP events. */
int32_t cvd_bilateral_filter(cvd_handle* h, int32_t num_frames, int32_t first_output, int32_t num_outputs, int32_t height,
                             int32_t width, const float* depth, const float* color, int32_t frame_radius,
                             int32_t spatial_radius, float depth_sigma, float color_sigma, int32_t median, float* out,
                             double* kernel_ms);

/* FlowConstraintsCollection::setStaticFlagFromRansac (the reference's pose_optimization.py:170-174 calls it for
 * --opt.dynamic_constraints Ransac; its C++ never implemented the method: the definition is tests/epipolar_reference.py,
 * DESIGN.md section 3.7).  Per directed pair p (constraints [offsets[p], offsets[p+1]), offsets[0] = 0) an epipolar RANSAC
 * in f64: pixels = loc * pixel_scale (the width of the raster the constraints were sampled on), Hartley normalisation,
 * `iterations` 8-point hypotheses drawn with splitmix64(seed << 44 | p << 24 | k << 8 | c), rank 2, inlier <=> both
 * point-to-epipolar-line distances <= threshold_px, winner = most inliers (lowest k on ties), one least-squares refit over
 * its inliers adopted when it keeps at least as many.  Bitwise deterministic.
 *   loc             [C][4]  (loc0.xy, loc1.xy), C = offsets[num_pairs]; every value must be finite
 *   is_static_out   [C]     1 = inlier of the pair's adopted F; a pair with fewer than 8 constraints, a zero spread or no valid
 *                           hypothesis is all 1
 *   fundamental_out [P][9]  adopted F (row-major, pixel coordinates, up to scale; 0 for an all-static pair); may be NULL
 *   best_out        [P][2]  (winning k, inliers of the adopted F); (-1, -1) for an all-static pair; may be NULL
 *   kernel_ms       [4]     {normalise, hypotheses, score, select} kernel time, HIP events; may be NULL
 * Rejected before any work, with an error naming the argument: threshold_px <= 0 or non-finite, iterations outside
 * [1, 65536], num_pairs >= 2^20, a non-finite loc, non-monotone offsets. */
int32_t cvd_epipolar_static_flags(cvd_handle* h, int32_t num_pairs, const int64_t* offsets, const float* loc, double pixel_scale,
                                  double threshold_px, int32_t iterations, uint64_t seed, uint8_t* is_static_out,
                                  double* fundamental_out, int32_t* best_out, double* kernel_ms);

/* ---- feature tracks: DepthVideoProcessor::computeTracks, reference lib/Processor.cpp:646-886 ----------
 * Independent of cvd_set_video.  Host inputs, images of height x width (the "down" colour stream's size):
 *   frame_active [F]          nonzero: the frame lies in frameRange and its colour image exists (others are skipped)
 *   first_frame, last_frame   frameRange.firstFrame() / lastFrame(): continue only when f > first, spawn only when f < last
 *   corner [F][H][W]          cornerMinEigenVal response of every active frame (cvd_corner_min_eigenval)
 *   dyn_dist [F][dyn_h][dyn_w] distance to the nearest dynamic pixel (cvd_dynamic_distance) or NULL (no dynamic_mask stream)
 *   flow [F-1][H][W][2], flow_mask [F-1][H][W], pair_present [F-1]: pair f -> f+1, bit 0 = its flow exists (right size),
 *                             bit 1 = its mask exists; flow / flow_mask may be NULL when no pair has the bit
 *   spawn_distance, prune_distance, min_dynamic_distance, min_track_length: DvpParams' track* fields and minDynamicDistance
 * counts[3] receives {tracks created (ids 0 .. n-1), tracks kept (length >= min_track_length), their observations}; the table
 * stays on the device until cvd_get_tracks.  kernel_ms[4] (may be NULL): {candidates, sort, walk, table} HIP-event times.
 * Spawn candidates are ranked by descending corner response, ties by ascending pixel index (unspecified in the reference).
 * Rejected before any work, with an error naming the value: a bad size or frame range, a negative or > 16384 distance, null
 * inputs, images whose two LDS bitmasks exceed the LDS budget ("image too large"). */
int32_t cvd_compute_tracks(cvd_handle* h, int32_t num_frames, int32_t height, int32_t width, float inv_aspect,
                           const uint8_t* frame_active, int32_t first_frame, int32_t last_frame, const float* corner,
                           const float* dyn_dist, int32_t dyn_h, int32_t dyn_w, const float* flow, const uint8_t* flow_mask,
                           const uint8_t* pair_present, int32_t spawn_distance, int32_t prune_distance,
                           float min_dynamic_distance, int32_t min_track_length, int64_t* counts, double* kernel_ms);
/* The table of the last cvd_compute_tracks: per track id start_frame[n], length[n] and kept[n] (0: deleted by the length
 * pruning, an id hole), and loc[counts[2]][2] = the kept tracks' observations (x / w, y / h * invAspect), track by track in
 * id order, frame by frame inside a track.  Any pointer may be NULL. */
int32_t cvd_get_tracks(cvd_handle* h, int32_t* start_frame, int32_t* length, uint8_t* kept, float* loc);

/* ---- flow consistency masks: Flow.compute_flow_masks, reference flow.py:180-209 + utils/consistency.py:8-67
 * Independent of cvd_set_video.  For every pair p = (a, b) of pair_frames both directed masks, in one launch:
 *   color [num_frames][H][W][channels]  the frames' "down" colour images (channels 1..4), passed once; pairs index into it
 *   pair_frames [P][2]                  (a, b), a != b
 *   flow_ab, flow_ba [P][H][W][2]       flow a -> b and b -> a, pixels
 *   mask_ab, mask_ba [P][H][W]          255 where the pixel passes, else 0
 * Direction a -> b at pixel (x, y): target t = (x, y) + flow_ab in f64; in bounds iff 0 <= t.x <= W - 1 and 0 <= t.y <= H - 1;
 * S = grid_sample (bilinear, align_corners = false, border padding, f32) of the other frame's image at g = f32(2 t / size - 1),
 * which lies HALF A PIXEL up and left of t (the reference's behaviour, kept); ef = |flow_ab + S(flow_ba)|^2,
 * ec = |color_a - S(color_b)|^2; mask = in bounds && ef < flow_thresh^2 && ec < channels * color_thresh^2 (thresholds formed
 * in double, rounded once to f32; a NaN fails).  Reference defaults: flow_thresh 1, color_thresh 1.
 *   kept   [P][2]          optional (may be NULL): pixels set in mask_ab, mask_ba
 *   errors [P][2][H][W][2] optional (may be NULL): (ef, ec) per direction, for value-level parity checks
 *   kernel_ms              optional (may be NULL): kernel time, HIP events
 * Every output repeats bit for bit.  Rejected before any work, with an error naming the argument and the value: sizes < 1,
 * channels outside [1, 4], num_pairs outside [0, 65535], more than 2^28 pixels per image, a negative or non-finite threshold,
 * a frame index out of range, a == b, null pointers.  num_pairs == 0 returns at once. */
int32_t cvd_flow_consistency_masks(cvd_handle* h, int32_t num_frames, int32_t height, int32_t width, int32_t channels,
                                   const float* color, int32_t num_pairs, const int32_t* pair_frames, const float* flow_ab,
                                   const float* flow_ba, float flow_thresh, float color_thresh, uint8_t* mask_ab,
                                   uint8_t* mask_ba, int32_t* kept, float* errors, double* kernel_ms);

/* ---- geometric consistency loss of flow pairs and its depth gradient: the static terms of the reference's fine-tuning loss,
 * ConsistencyLoss (loss/consistency_loss.py:92-182, 219-239; utils/geometry.py; utils/loss.py:62-80), DESIGN.md §3.10.
 * Independent of cvd_set_video.  One forward pass over all pairs and both directions, one backward pass; every real array has
 * the precision desc names (float or double):
 *   depth      [F][H][W]
 *   extrinsics [F][3][4]       [R | t], columns right / up / backward (the camera looks down -z)
 *   intrinsics [F][4]          (fx, fy, cx, cy), pixels
 *   warp       [F][2][H][W]    pixel offsets added to the pixel grid, planar (x then y); read only when desc.have_warp
 *   pair_frames [P][2]         (a, b), a != b
 *   flow_ab, flow_ba [P][2][H][W]  planar flow a -> b on a's raster, b -> a on b's raster, pixels
 *   weight_ab, weight_ba [P][H][W] weights of the samples (the reference's masks; multiplied, not tested)
 * Per pair and direction (ref r, target t): pix = (x, y) + warp_r; X_t = R_t^T (R_r ray(pix) D_r + t_r - t_t); the reprojection
 * error |project_t(X_t) - (pix + flow)|, the disparity error 1 / X_t.z - 1 / z_w and the depth-ratio error
 * lambda_depth_ratio log(min / max of |z_w|, |X_t.z|), z_w = -D_t sampled bilinearly at (pix + flow) size / (size - 1) - 0.5
 * (clamped to the image: grid_sample, align_corners = false, border).  Each goes through the distance rho and a weighted mean
 * sum w rho / max(sum w, 1e-6); per pair  reproj = lambda_reprojection mean_k(.),  disp = lambda_disparity mean_k(fbar_k .) with
 * fbar_k the mean focal length of the ref frames of all pairs,  depth ratio = mean_k(.);  a term exists only when its lambda
 * is > 0 (else 0);  total = mean over pairs of the sum of the terms.
 *   total [1], terms [P][3]    (reproj, disp, depth ratio), double in both precisions
 *   grad  [F][H][W]            optional (may be NULL): d total / d depth, in the arrays' precision
 *   kernel_ms [2]              optional (may be NULL): {forward, backward} kernel times, HIP events
 * The forward results repeat bit for bit; the gradient is accumulated with float atomics (in a fixed order in the deterministic
 * build).  Rejected before any device work: a desc of another header revision (struct_size), width or height < 2, num_pairs < 1,
 * a pair frame out of range or a pair naming one frame twice, a negative or non-finite lambda, distance_scale <= 0, a non-finite
 * distance_alpha, null arrays.  All lambdas 0: zeros. */
enum { CVD_PRECISION_F32 = 0, CVD_PRECISION_F64 = 1 };
enum { CVD_DISTANCE_L1 = 0, CVD_DISTANCE_L2 = 1, CVD_DISTANCE_SMOOTH_L1 = 2, CVD_DISTANCE_CAUCHY = 3, CVD_DISTANCE_GENERAL = 4 };
typedef struct cvd_consistency_desc {
  uint64_t struct_size;        /* CVD_STRUCT_STAMP(cvd_consistency_desc), set by the caller */
  int32_t precision;           /* CVD_PRECISION_* of every real array */
  int32_t num_frames, num_pairs, height, width;
  int32_t distance_type;       /* CVD_DISTANCE_*: l1 = |e / scale|; l2 / smooth_l1 / cauchy / general = the general robust loss
                                  (reference loss/general.py, exact branch) at alpha = 2 / 1 / 0 / distance_alpha */
  int32_t have_warp;
  int32_t reserved;            /* 0 */
  double lambda_reprojection, lambda_disparity, lambda_depth_ratio;   /* reference defaults 1, 0, 100 */
  double distance_scale, distance_alpha;
} cvd_consistency_desc;
int32_t cvd_consistency_loss(cvd_handle* h, const cvd_consistency_desc* desc, const void* depth, const void* extrinsics,
                             const void* intrinsics, const void* warp, const int32_t* pair_frames, const void* flow_ab,
                             const void* flow_ba, const void* weight_ab, const void* weight_ba, double* total, double* terms,
                             void* grad, double* kernel_ms);
/* The same on DEVICE arrays (inputs and results), enqueued on `stream` (a hipStream_t of the handle's device): no copy and no
 * host synchronisation; the results are valid once the stream reaches the end of the call.  One call at a time per handle (its
 * scratch buffers are shared).  pair_frames cannot be checked before the launch here: a pair that names a frame outside [0, F)
 * or one frame twice is never dereferenced, and its terms and the total come back NaN. */
int32_t cvd_consistency_loss_device(cvd_handle* h, const cvd_consistency_desc* desc, const void* depth, const void* extrinsics,
                                    const void* intrinsics, const void* warp, const int32_t* pair_frames, const void* flow_ab,
                                    const void* flow_ba, const void* weight_ab, const void* weight_ba, double* total,
                                    double* terms, void* grad, void* stream);

/* ---- scene-flow loss of flow pairs and its depth gradient: the reference's SceneFlowLoss (loss/scene_flow_loss.py:31-356;
 * utils/geometry.py; utils/loss.py:62-80), DESIGN.md §3.11.  The static term compares matched points in world space; the three
 * temporally smooth terms ask the forward and backward scene flow of an anchor frame to its temporal neighbours to cancel.
 * Independent of cvd_set_video; tables and precision as for cvd_consistency_loss, and in addition
 *   flows[2], masks[2]          per direction k (0: a -> b on a's raster, 1: b -> a on b's): [P][2][H][W] pixels, [P][H][W]
 *   neighbor_frames [P][4]      (a - 1, a + 1, b - 1, b + 1) as the loader clamps them: a boundary anchor names itself
 *   neighbor_flows[4], neighbor_masks[4]   anchor -> neighbour, in the order of neighbor_frames: [P][2][H][W], [P][H][W]
 *   valid [P][2]                0 / 1 per anchor: both neighbours of the anchor exist
 * flows / masks / neighbor_flows / neighbor_masks are (host) arrays of 2 / 2 / 4 / 4 array pointers.
 * With X_f(x, y) = ray_f((x, y) + warp_f) D_f the camera-space point map of frame f, Xw_f = R_f X_f + t_f and S_f(m) the
 * bilinear sample of the three-channel map X_f at pixel position m (m size / (size - 1) - 0.5, clamped: grid_sample, bilinear,
 * align_corners = false, border):
 *   static  (pair, direction k; ref r, target t)   Y = R_t S_t(pix_r + flow_k) + t_t,  d = |Xw_r - Y|,  w = mask_k / |D_r|
 *           static = lambda_static mean_k sum w rho_static(d) / max(sum w, 1e-6)     (w is a function of the depth, also in grad)
 *   smooth  (pair, anchor al; frame r, neighbours n-, n+)   Y+- = R_n S_n(pix_r + neighbor_flow) + t_n,
 *           X_s = R_r^T (Y+ + Y- - Xw_r - t_r),  w = valid neighbor_mask- neighbor_mask+,
 *           e_rep = |project_r(X_s) - pix_r|,  e_dsp = 1 / X_s.z - 1 / X_r.z,
 *           e_rat = lambda_smooth_depth_ratio log(min / max of |X_r.z|, |X_s.z|);  each through rho_smooth and the weighted mean;
 *           smooth_reproj = lambda mean_al(.),  smooth_disparity = lambda mean_al(fbar_al .) with fbar_al the mean focal length of
 *           anchor al's frames over all pairs,  smooth_depth_ratio = mean_al(.)
 * A term exists only when its lambda is > 0 (else 0); total = mean over pairs of the sum of the terms.
 *   total [1], terms [P][4]     (static, smooth_reproj, smooth_disparity, smooth_depth_ratio), double in both precisions
 *   grad  [F][H][W]             optional (may be NULL): d total / d depth, in the arrays' precision
 *   maps  [6][P][3][H][W]       optional (may be NULL): the reference's visualisation maps, in the arrays' precision:
 *                               w (Xw_r - Y) of direction 0 / 1, then per anchor w (Y+ - Xw_r), w (Y- - Xw_r); zeros for a part
 *                               whose lambdas are all 0.  Nothing is written (or computed) for them when NULL.
 *   kernel_ms [2]               optional (may be NULL): {forward, backward} kernel times, HIP events
 * flows / masks may be NULL when lambda_static is 0; neighbor_frames / neighbor_flows / neighbor_masks / valid may be NULL when
 * the three smooth lambdas are 0.  The forward results repeat bit for bit; the gradient is accumulated with float atomics (in a
 * fixed order in the deterministic build).  Rejected before any device work: a desc of another header revision (struct_size),
 * width or height < 2, num_frames < 2, num_pairs < 1, a pair or neighbour frame out of range or a pair naming one frame twice, a
 * negative or non-finite lambda, distance_scale <= 0, a non-finite distance_alpha, a null array an enabled term reads.  All
 * lambdas 0: zeros. */
typedef struct cvd_scene_flow_desc {
  uint64_t struct_size;        /* CVD_STRUCT_STAMP(cvd_scene_flow_desc), set by the caller */
  int32_t precision;           /* CVD_PRECISION_* of every real array */
  int32_t num_frames, num_pairs, height, width;
  int32_t distance_type_static, distance_type_smooth;   /* CVD_DISTANCE_*; both use distance_scale and distance_alpha */
  int32_t have_warp;
  double lambda_static, lambda_smooth_reprojection, lambda_smooth_disparity, lambda_smooth_depth_ratio;
  double distance_scale, distance_alpha;
} cvd_scene_flow_desc;
int32_t cvd_scene_flow_loss(cvd_handle* h, const cvd_scene_flow_desc* desc, const void* depth, const void* extrinsics,
                            const void* intrinsics, const void* warp, const int32_t* pair_frames, const void* const* flows,
                            const void* const* masks, const int32_t* neighbor_frames, const void* const* neighbor_flows,
                            const void* const* neighbor_masks, const void* valid, double* total, double* terms, void* grad,
                            void* maps, double* kernel_ms);
/* The same on DEVICE arrays (inputs and results; the four pointer arrays themselves stay host arrays), enqueued on `stream`: no
 * copy and no host synchronisation.  One call at a time per handle.  pair_frames and neighbor_frames cannot be checked before the
 * launch here: a pair or neighbour that names a frame outside [0, F), or a pair of one frame twice, is never dereferenced, and
 * its terms and the total come back NaN.  With lambda_smooth_disparity > 0 such a pair also leaves the mean focal length over
 * all pairs undefined: the smooth_disparity term of EVERY pair is then NaN, and so is the gradient it reaches. */
int32_t cvd_scene_flow_loss_device(cvd_handle* h, const cvd_scene_flow_desc* desc, const void* depth, const void* extrinsics,
                                   const void* intrinsics, const void* warp, const int32_t* pair_frames, const void* const* flows,
                                   const void* const* masks, const int32_t* neighbor_frames, const void* const* neighbor_flows,
                                   const void* const* neighbor_masks, const void* valid, double* total, double* terms,
                                   void* grad, void* maps, void* stream);

/* ---- spatial smoothness and contrast losses and their depth gradient: the reference's DisparitySmoothLoss
 * (loss/disparity_smooth_loss.py:15-56) and ContrastLoss (loss/contrast_loss.py:13-79), DESIGN.md §3.12.  Independent of
 * cvd_set_video.  One pass computes both terms and, on request, the complete gradient; every real array has the precision desc
 * names.  F = num_frames = B frames_per_sample; frame f belongs to sample f / frames_per_sample:
 *   depth      [F][H][W]       the predicted depths D
 *   depth_orig [F][H][W]       the original estimator's depths Do; read only when lambda_contrast_loss > 0 (else may be NULL)
 *   image      [F][3][H][W]    colours I; read only when lambda_disparity_smooth > 0 (else may be NULL)
 * With d = 1 / D and N = frames_per_sample:
 *   x-edge (x < W-1)  s_x = exp(-mean_c |I_c(x,y) - I_c(x+1,y)| / sigma_color_grad) |d(x,y) - d(x+1,y)|;  y-edge likewise
 *   smooth[b] = lambda_disparity_smooth [ sum_{f in b} sum s_x / (N H (W-1)) + sum_{f in b} sum s_y / (N (H-1) W) ]
 *   r(a, b) = max(a, b) / (min(a, b) + 1e-10)
 *   h-edge (x < W-1)  c_h = [ r(Do(x+1,y), Do(x,y)) > contrast_thresh ] (contrast_thresh - r(D(x+1,y), D(x,y)))^2;  v-edge likewise
 *   contrast = lambda_contrast_loss (sum c_h + sum c_v) / F
 *   total = mean_b smooth[b] + contrast            (a term exists only when its lambda is > 0, else 0)
 *   total [1], smooth [B], contrast [1]   double in both precisions
 *   grad  [F][H][W]            optional (may be NULL): d total / d depth, in the arrays' precision, written once per pixel
 *   kernel_ms [1]              optional (may be NULL): kernel time, HIP events
 * No atomics: values and gradient repeat bit for bit on every build.  Rejected before any device work: a desc of another header
 * revision (struct_size), width or height < 2 (the reference returns NaN there), num_frames < 1 or not a multiple of
 * frames_per_sample, a negative or non-finite lambda, sigma_color_grad <= 0 with the smoothness term on, a non-finite
 * contrast_thresh with the contrast term on, a null table an enabled term reads, null results.  Both lambdas 0: zeros. */
typedef struct cvd_spatial_desc {
  uint64_t struct_size;        /* CVD_STRUCT_STAMP(cvd_spatial_desc), set by the caller */
  int32_t precision;           /* CVD_PRECISION_* of every real array */
  int32_t num_frames, frames_per_sample, height, width;
  int32_t reserved;            /* 0 */
  double lambda_disparity_smooth, sigma_color_grad;   /* reference defaults 0, 1 */
  double lambda_contrast_loss, contrast_thresh;       /* reference defaults 1, 1.05 */
} cvd_spatial_desc;
int32_t cvd_spatial_losses(cvd_handle* h, const cvd_spatial_desc* desc, const void* depth, const void* depth_orig,
                           const void* image, double* total, double* smooth, double* contrast, void* grad, double* kernel_ms);
/* The same on DEVICE arrays (inputs and results), enqueued on `stream`: no copy and no host synchronisation.  One call at a time
 * per handle. */
int32_t cvd_spatial_losses_device(cvd_handle* h, const cvd_spatial_desc* desc, const void* depth, const void* depth_orig,
                                  const void* image, double* total, double* smooth, double* contrast, void* grad, void* stream);

/* ---- parameter regulariser and optimizer step over a list of tensors, DESIGN.md §3.13.  Independent of cvd_set_video.  Each
 * is ONE kernel launch for any number of tensors: the tensors are cut into chunks of cvd_param_chunk() elements, a chunk whose
 * addresses are all 16-byte aligned moves 16 bytes per lane, any other goes element by element with the same arithmetic (the
 * same bits).  desc names the precision of every tensor and their number T (>= 0); a tensor of zero elements is legal (its
 * address may then be NULL) and contributes nothing.  State and arithmetic are in the tensors' precision; the loss is summed in
 * double, without atomics: it repeats bit for bit.
 * Rejected before any device work: a desc of another header revision (struct_size), a precision other than CVD_PRECISION_*,
 * num_tensors < 0, a NULL address or one that is not a multiple of the element size (of a tensor with elements), a negative
 * count, a non-finite lambda, beta, eps or step scalar, a beta outside [0, 1), a denom_scale <= 0, an unknown rule; the host
 * variants also a tensor that leaves the flat arrays. */
typedef struct cvd_param_desc {
  uint64_t struct_size;        /* CVD_STRUCT_STAMP(cvd_param_desc), set by the caller */
  int32_t precision;           /* CVD_PRECISION_* of every tensor */
  int32_t num_tensors;
} cvd_param_desc;
/* cvd_param_record::rule.  Every rule moves the moments: m = beta1 m + (1 - beta1) g, v = beta2 v + (1 - beta2) g g.
 *   ADAM       torch.optim.Adam (amsgrad = False, maximize = False, no decoupled decay): g += grad_decay p first, then
 *              p -= step m / (sqrt(v) / denom_scale + eps)
 *   RADAM      reference optimizer/radam.py:85-90 (N_sma >= 5): p -= param_decay p; p -= step m / (sqrt(v) + eps)
 *   RADAM_SGD  optimizer/radam.py:91-95 (N_sma < 5, degenerated_to_sgd): p -= param_decay p; p -= step m
 *   MOMENTS    N_sma < 5 without degenerated_to_sgd: p stays */
enum { CVD_PARAM_RULE_ADAM = 0, CVD_PARAM_RULE_RADAM = 1, CVD_PARAM_RULE_RADAM_SGD = 2, CVD_PARAM_RULE_MOMENTS = 3 };
/* One tensor's scalars of one step, formed by the caller in double exactly as the Python of the rule forms them (the kernel casts
 * them to the tensors' precision) */
typedef struct cvd_param_record {
  double beta1, beta2, eps;
  double grad_decay;           /* ADAM: weight_decay; else 0 */
  double param_decay;          /* RADAM, RADAM_SGD: weight_decay lr; else 0 */
  double step;                 /* ADAM: lr / (1 - beta1^t); RADAM, RADAM_SGD: step_size lr (optimizer/radam.py:77-79) */
  double denom_scale;          /* ADAM: sqrt(1 - beta2^t); else 1 */
  int32_t rule;                /* CVD_PARAM_RULE_* */
  int32_t reserved;            /* 0 */
} cvd_param_record;
/* Elements per chunk of the tables (CVD_PARAM_CHUNK of the build). */
int64_t cvd_param_chunk(void);
/* The reference's ParameterLoss (loss/parameter_loss.py:9-27): total = lambda sum_i sum |p_i - p0_i|, and its subgradient
 * grad_i (+)= lambda sign(p_i - p0_i) grad_out with sign(0) = 0 (torch.abs's).  Host arrays: tensor i is counts[i] elements at
 * element offsets[i] of the flat arrays p, p0 (and grad) of flat_count elements.
 *   total [1]        double
 *   grad             optional (may be NULL): flat, the tensors' precision; accumulate = 0 overwrites the tensors' elements,
 *                    1 adds to what the array holds; elements between the tensors stay as they are
 *   kernel_ms [2]    optional (may be NULL): {value, gradient} kernel time, HIP events */
int32_t cvd_parameter_l1(cvd_handle* h, const cvd_param_desc* desc, const int64_t* offsets, const int64_t* counts,
                         int64_t flat_count, const void* p, const void* p0, double lambda, double* total, void* grad,
                         double grad_out, int32_t accumulate, double* kernel_ms);
/* The same on DEVICE tensors, enqueued on `stream`: p, p0 and grad are host arrays of T device addresses, total (device, double)
 * and grad_out (device, one scalar of the tensors' precision) device addresses.  total != NULL computes the value, grad != NULL
 * the gradient (one launch each; at least one of the two).  No allocation once the table has been seen and no host
 * synchronisation; the table's static part is rebuilt (one wait for the stream) when the list of counts changes.  One call at a
 * time per handle. */
int32_t cvd_parameter_l1_device(cvd_handle* h, const cvd_param_desc* desc, const void* const* p, const void* const* p0,
                                const int64_t* counts, double lambda, double* total, void* const* grad, const void* grad_out,
                                int32_t accumulate, void* stream);
/* One optimizer step of every tensor in one launch: torch.optim.Adam's or the reference's RAdam.step (optimizer/radam.py:31-97),
 * as records[i].rule says; p, m (exp_avg) and v (exp_avg_sq) are updated in place, g is read.  Host arrays laid out as above;
 * kernel_ms [1] optional. */
int32_t cvd_param_step(cvd_handle* h, const cvd_param_desc* desc, const int64_t* offsets, const int64_t* counts, int64_t flat_count,
                       void* p, const void* g, void* m, void* v, const cvd_param_record* records, double* kernel_ms);
/* The same on DEVICE tensors (host arrays of T device addresses), enqueued on `stream`; conditions as cvd_parameter_l1_device. */
int32_t cvd_param_step_device(cvd_handle* h, const cvd_param_desc* desc, void* const* p, const void* const* g, void* const* m,
                              void* const* v, const int64_t* counts, const cvd_param_record* records, void* stream);

/* ---- fine-tuning batches from a device-resident dataset, DESIGN.md §3.14.  Independent of cvd_set_video.  Replaces the
 * reference's loaders/video_dataset.py::VideoDataset behind a DataLoader and to_device: the colour, flow and mask images of a
 * video are uploaded ONCE, in their file layout, and every batch is then ONE kernel launch that writes all its tensors in the
 * layout the losses read.  Every output element is a copy of a store element or the constant 0 / 1.
 * The store belongs to the handle: calls on it are ordered on one stream (or synchronised across streams) by the caller; the
 * set_* calls and cvd_dataset_create / _clear wait for the device, the batch entry points do not allocate once their staging
 * has its size.  cvd_destroy frees the store. */
typedef struct cvd_dataset_desc {
  uint64_t struct_size;          /* CVD_STRUCT_STAMP(cvd_dataset_desc), set by the caller */
  int32_t num_frames;            /* F: frames of the store */
  int32_t height, width;
  int32_t num_pairs;             /* Q: directed pairs whose flow and mask the store holds */
  int32_t num_samples;           /* S */
  int32_t temporal;              /* 0: a sample is its pair (N = 2 frames); 1: and the four neighbours (N = 6) */
  int32_t has_depth_orig;        /* 1: the store also holds an initial depth per frame (cvd_dataset_set_depth_orig) */
  int32_t neighbor_rule_frames;  /* the reference's self.num_frames = len(frames) of its rule for real neighbours, 0 < k <
                                    num_frames - 1, and of the clamp of the neighbour indices; 0 = num_frames, never more */
} cvd_dataset_desc;
/* Allocates the store (zeroed) and builds the device-resident sample table (reference loaders/video_dataset.py:223-256, 309-328,
 * 358-367).  pair_frames [Q][2]: the directed pairs (source, target), slot = position; samples [S][2]: the frame pair (a, b) of
 * every sample.  A sample reads the flows of (a, b) and (b, a) and, with `temporal`, of (k, k-1) and (k, k+1) for k = a, b where k
 * is an interior frame (else the reference's dummies: images 0, cameras, flows and masks 1, valid 0).  Rejected before any device
 * work: a desc of another header revision, a shape or count below its minimum, a frame outside [0, F), a directed pair listed
 * twice, a sample one of whose directions is not in the pair list, a temporal sample whose interior frame lacks a neighbour flow.
 * Replaces the store of an earlier call. */
int32_t cvd_dataset_create(cvd_handle* h, const cvd_dataset_desc* desc, const int32_t* pair_frames, const int32_t* samples);
/* Frees the store. */
int32_t cvd_dataset_clear(cvd_handle* h);
/* Uploads, in chunks of the caller's choice (a caller streams from disk).  Colour of frames [first, first + count): host f32
 * [count][H][W][3] in the channel order the batch returns (the reference's load_color, loaders/video_dataset.py:49-60: raw files
 * flipped BGR -> RGB, other files / 255).  Flow and mask of pair slots [first, first + count) in their file layout: flow f32
 * [count][H][W][2] pixels, mask u8 [count][H][W], any nonzero value counts as 1 (load_flow / load_mask, :63-78).  Initial depth of
 * frames [first, first + count): f32 [count][H][W], already 1 / disparity (reference depth_fine_tuning.py:457-471). */
int32_t cvd_dataset_set_colors(cvd_handle* h, int32_t first, int32_t count, const float* hwc3);
int32_t cvd_dataset_set_flows(cvd_handle* h, int32_t first, int32_t count, const float* flow, const uint8_t* mask);
int32_t cvd_dataset_set_depth_orig(cvd_handle* h, int32_t first, int32_t count, const float* depth);
/* Cameras of all frames as update_poses forms them (reference loaders/video_dataset.py:177-189): extrinsics f32 [F][3][4] with
 * columns right, up, backward, position; intrinsics f32 [F][4] = (fx, fy, cx, cy) in pixels. */
int32_t cvd_dataset_set_cameras(cvd_handle* h, const float* extrinsics, const float* intrinsics);
/* The per-frame tables of update_poses (reference loaders/video_dataset.py:191-217) from the transforms' parameters, on the
 * device, one launch per table: scales = GridDepthXform::paramMap as f32 [F][H][W] for a 2-D grid, [F] scalars 1.0 for Identity
 * and params[0] for Global; warp = SpatialXform::warp(H, W) as f32 [F][2][H][W] (planar) for the five spatial families.
 * depth_params [F][nD], spatial_params [F][nS] doubles (NULL where the count is 0).  Refused as the reference refuses them: a value
 * transform other than Scale when the depth type is not Identity ("We only support scale-based transforms at the moment."), other
 * depth / spatial types ("Unsupported depth / spatial transform type").  A depth-wise grid (grid z > 1), whose map needs the source
 * depth, is refused too: evaluate it on the host and use cvd_dataset_set_maps. */
int32_t cvd_dataset_set_xforms(cvd_handle* h, const cvd_xform_desc* depth_desc, const double* depth_params,
                               const cvd_xform_desc* spatial_desc, const double* spatial_params);
/* The same tables from host arrays: scales f32 [F][H][W] (scale_is_map != 0) or [F], NULL = no scales; warp f32 [F][2][H][W],
 * NULL = no warp. */
int32_t cvd_dataset_set_maps(cvd_handle* h, const float* scales, int32_t scale_is_map, const float* warp);
/* Where a batch of B samples goes; f32 and contiguous unless noted, N = 6 with `temporal`, else 2.  The ts_* members are written
 * with `temporal` only (else ignored); scales, warp and depth_orig are optional (NULL: not written) and need their table. */
typedef struct cvd_dataset_batch_out {
  uint64_t struct_size;        /* CVD_STRUCT_STAMP(cvd_dataset_batch_out), set by the caller */
  void* images;                /* (B, N, 3, H, W): colour of the pair, then of the four neighbours (0 for a dummy) */
  void* extrinsics;            /* (B, N, 3, 4); dummies are 1 */
  void* intrinsics;            /* (B, N, 4); dummies are 1 */
  void* gc_indices;            /* (B, 2) int64: the pair */
  void* gc_flows[2];           /* (B, 2, H, W): a -> b, b -> a, planar */
  void* gc_masks[2];           /* (B, 1, H, W): 0 or 1 */
  void* ts_indices;            /* (B, 4) int64: (a-1, a+1, b-1, b+1) clamped */
  void* ts_flows[4];           /* (B, 2, H, W): a -> a-1, a -> a+1, b -> b-1, b -> b+1; dummies are 1 */
  void* ts_masks[4];           /* (B, 1, H, W); dummies are 1 */
  void* ts_valid;              /* (B, 2, 1): 1 where a / b is an interior frame */
  void* scales;                /* (B, N, H, W) or (B, N, 1, 1): of the pair and the clamped neighbours (real frames, dummies or not) */
  void* warp;                  /* (B, N, 2, H, W): frames as for scales */
  void* depth_orig;            /* (B, 2, H, W): of the pair */
} cvd_dataset_batch_out;
/* One batch: host indices (int64 [B], each in [0, S): checked before any device work) and host arrays.  kernel_ms [1] optional. */
int32_t cvd_dataset_batch(cvd_handle* h, int32_t batch_size, const int64_t* indices, const cvd_dataset_batch_out* out,
                          double* kernel_ms);
/* The same with DEVICE indices and DEVICE outputs, one launch enqueued on `stream`: no copy, no allocation and no host
 * synchronisation.  The indices cannot be checked here: the kernel clamps an index outside [0, S) into it -- it never reads
 * outside the store -- and counts it in a device word. */
int32_t cvd_dataset_batch_device(cvd_handle* h, int32_t batch_size, const int64_t* indices, const cvd_dataset_batch_out* out,
                                 void* stream);
/* Indices the device entry point has clamped since cvd_dataset_create.  Waits for the device: for tests and debugging. */
int32_t cvd_dataset_bad_indices(cvd_handle* h, int64_t* count);

/* ---- RAFT's correlation pyramid, windowed lookup and convex upsampling, DESIGN.md §3.15.  Independent of cvd_set_video.  The two
 * stages of the reference's flow network (raft/core/raft.py) that are neither a convolution nor a matmul; f32, forward only (RAFT
 * runs under no_grad).  DEVICE arrays, enqueued on `stream` (a hipStream_t of the handle's device): ONE kernel launch each, no
 * copy, no host synchronisation, no scratch of the handle -- calls need no ordering among themselves beyond the data's.  No
 * atomics: every result repeats bit for bit.  Each call rejects, before any device work and with an error that names the value:
 * sizes < 1, num_levels outside [1, 4], radius outside [1, 4], a coarsest level below 2 x 2 (the reference divides by size - 1:
 * NaN), null arrays, an array that must be 16-byte aligned and is not.
 *
 * Pyramid -- reference raft/core/corr.py:15-23 and :48-56, what CorrBlock.__init__ does after its matmul:
 *   raw        [Q][height][width]   fmap1^T fmap2, Q = B h1 w1 queries, (height, width) = (h2, w2) of frame 2; 16-byte aligned
 *   levels     host array of num_levels device arrays, 16-byte aligned; levels[l] is [Q][height >> l][width >> l]
 *   levels[0] = raw / sqrtf((float)dim), an IEEE f32 division (bit for bit torch's); levels[0] may BE raw (scaled in place).
 *   levels[l + 1] = mean of the 2 x 2 cells of levels[l] (avg_pool2d(2, stride = 2): an odd last row or column is dropped). */
int32_t cvd_raft_corr_pyramid_device(cvd_handle* h, int64_t num_queries, int32_t height, int32_t width, int32_t dim,
                                     int32_t num_levels, const float* raw, float* const* levels, void* stream);
/* Lookup -- reference raft/core/corr.py:25-46 (CorrBlock.__call__) with raft/core/utils/utils.py:56-70 (bilinear_sampler):
 *   coords     [batch][2][h1][w1]   channel 0 = x, 1 = y, in level-0 pixels of frame 2
 *   levels     as above, (h2, w2) the level-0 size
 *   out        [batch][num_levels n^2][h1][w1], n = 2 radius + 1
 * out channel l n^2 + a n + b = levels[l] of the query sampled at (x / 2^l + a - radius, y / 2^l + b - radius): the FIRST window
 * index moves x (the reference's meshgrid(dy, dx) order; the trained weights depend on it).  Bilinear, pixel centres at integers
 * (align_corners = True), corners by floor, corners outside the map count 0 (padding_mode = "zeros").  The n^2 taps of a query
 * share one pair of fractions (the reference rounds each tap through a normalise / unnormalise round trip: last-bit differences).
 * Any finite coordinate, however large, gives zeros; a non-finite one gives unspecified values; neither reads out of range. */
int32_t cvd_raft_corr_lookup_device(cvd_handle* h, int32_t batch, int32_t h1, int32_t w1, int32_t h2, int32_t w2,
                                    int32_t num_levels, int32_t radius, const float* const* levels, const float* coords,
                                    float* out, void* stream);
/* Convex upsampling -- reference raft/core/raft.py:49-60 (RAFT.upsample_flow):
 *   flow [n][2][height][width], mask [n][576][height][width], out [n][2][8 height][8 width] (16-byte aligned)
 *   out[n][c][8 y + i][8 x + j] = sum_k softmax_k(mask[n][64 k + 8 i + j][y][x]) 8 flow[n][c][y + k / 3 - 1][x + k % 3 - 1],
 * flow outside the image counting 0 (unfold with padding 1); the softmax subtracts the maximum (stable for logits of +-100). */
int32_t cvd_raft_upsample_flow_device(cvd_handle* h, int32_t n, int32_t height, int32_t width, const float* flow,
                                      const float* mask, float* out, void* stream);

/* ---- SepConvGRU of RAFT's update block, DESIGN.md §3.16 -- reference raft/core/update.py:37-75 (SepConvGRU.forward with
 * hidden_dim = 128, input_dim = 256, the only sizes BasicUpdateBlock builds).  Independent of cvd_set_video.  f32, forward only.
 * Per half (1 x 5 with padding (0, 2), then 5 x 1 with padding (2, 0)):
 *   z = sigmoid(conv_z([h, x])), r = sigmoid(conv_r([h, x])), q = tanh(conv_q([r h, x])), h = (1 - z) h + z q.
 * DEVICE arrays, enqueued on `stream`: four kernel launches, no copy, no host synchronisation, no atomics; results repeat bit for
 * bit and do not depend on how x is segmented.  Scratch (3 x 128 batch height width floats) belongs to the handle and keeps its
 * high-water size: calls on one device must be ordered on one stream (the rule of the *_loss_device entry points), and a call
 * that has to grow the scratch allocates (every call after the first of a shape does not).
 *   hidden            [batch][128][height][width]
 *   segments          host array of num_segments (1..3) device arrays; segments[i] is [batch][segment_channels[i]][height][width].
 *                     x is their concatenation along the channels, which is never formed.
 *   segment_channels  host array; positive multiples of 32 that sum to 256
 *   weights, biases   host arrays of six device arrays in the order convz1, convr1, convq1, convz2, convr2, convq2, in torch's
 *                     layout: weight [128][384][1][5] resp. [128][384][5][1] (the same memory order, k = 5 c + t), 16-byte
 *                     aligned; bias [128]
 *   out               [batch][128][height][width]; must not overlap hidden or a segment
 * Rejected before any device work, with an error that names the value: sizes < 1, a wrong segment table, null arrays, a weight that
 * is not 16-byte aligned, an output that overlaps an input. */
int32_t cvd_raft_sepconv_gru_device(cvd_handle* h, int32_t batch, int32_t height, int32_t width, const float* hidden,
                                    int32_t num_segments, const float* const* segments, const int32_t* segment_channels,
                                    const float* const* weights, const float* const* biases, float* out, void* stream);
/* The same call for measurement (tools/raftgru_bench.py): HIP events around the four launches on `stream`, then a host wait;
 * kernel_ms[4] = {z and r of the 1 x 5 half, q and gate of it, z and r of the 5 x 1 half, q and gate of it} in milliseconds. */
int32_t cvd_raft_sepconv_gru_timed(cvd_handle* h, int32_t batch, int32_t height, int32_t width, const float* hidden,
                                   int32_t num_segments, const float* const* segments, const int32_t* segment_channels,
                                   const float* const* weights, const float* const* biases, float* out, void* stream,
                                   double* kernel_ms);

/* ---- The stock convolutions of RAFT's update block and the block itself, DESIGN.md §3.17.  Independent of cvd_set_video.  f32,
 * forward only.  DEVICE arrays, enqueued on `stream`: kernel launches only, no copy, no host synchronisation, no atomics; every
 * output element is written once in a fixed operation order, so results repeat bit for bit and do not depend on how an input is
 * segmented.
 *
 * One convolution -- reference raft/core/update.py:11-12, 100-104, 142-144 (the nn.Conv2d of FlowHead, BasicMotionEncoder and
 * the mask head: square filter, stride 1, padding kernel_size / 2) with the ReLU behind it (:16, :107-113, :143) and the factor
 * of :155:
 *   out[b][out_first_channel + o][y][x] = scale * act(bias[o] + sum_{c,i,j} weight[o][c][i][j] in[b][c][y + i - r][x + j - r]),
 * r = kernel_size / 2, the input outside the image counting 0; ONE launch.
 *   segments          host array of num_segments (1..3) device arrays; segments[i] is [batch][segment_channels[i]][height][width].
 *                     The input is their concatenation along the channels, which is never formed.
 *   segment_channels  host array; one segment: any count >= 1; several: positive multiples of 32.  Their sum must be in_channels.
 *   weights, biases   host arrays of num_weights (1 or 2) device arrays in torch's layout, weight
 *                     [out_channels][in_channels][kernel_size][kernel_size], bias [out_channels].  Two tensors are stacked along
 *                     the output channels (o = 0 .. 2 out_channels - 1) and need out_channels in multiples of 64.  Any alignment:
 *                     weights are read as float4 where their rows start on 16 bytes, as floats elsewhere.
 *   kernel_size       1, 3 or 7;  stride, dilation, groups: must be 1
 *   activation        0 none, 1 ReLU;  scale multiplies after the activation (a power of two gives the bits of a separate multiply)
 *   out               [batch][out_total_channels][height][width]; only channels out_first_channel .. out_first_channel +
 *                     num_weights out_channels - 1 are written.  The tensor must not overlap a segment.
 * Rejected before any device work, with an error that names the value: sizes < 1, a filter size other than 1, 3, 7, a stride,
 * dilation or groups other than 1, null arrays, more than three segments, several segments not in multiples of 32 channels,
 * segments that do not sum to in_channels, an output window that exceeds its tensor, an output that overlaps an input. */
int32_t cvd_raft_conv2d_device(cvd_handle* h, int32_t batch, int32_t height, int32_t width, int32_t num_segments,
                               const float* const* segments, const int32_t* segment_channels, int32_t num_weights,
                               const float* const* weights, const float* const* biases, int32_t in_channels, int32_t out_channels,
                               int32_t kernel_size, int32_t stride, int32_t dilation, int32_t groups, int32_t activation, float scale,
                               float* out, int32_t out_total_channels, int32_t out_first_channel, void* stream);
/* The block -- reference raft/core/update.py:133-156 (BasicUpdateBlock.forward with hidden_dim = 128, input_dim = 128) and what it
 * calls (:96-114 BasicMotionEncoder.forward, :37-75 SepConvGRU.forward, :8-16 FlowHead.forward):
 *   cor = relu(convc1(corr)); cor = relu(convc2(cor)); flo = relu(convf1(flow)); flo = relu(convf2(flo));
 *   motion_features = [relu(conv([cor, flo])), flow];  net_out = gru(net, [inp, motion_features]);
 *   delta_flow = flow_head.conv2(relu(flow_head.conv1(net_out)));  mask = 0.25 * mask.2(relu(mask.0(net_out)))
 * No cat is formed.  8 launches of the convolution above (7 with a null mask: flow_head.conv1 and mask.0 are one launch, mask.2
 * falls away) and the 4 unchanged launches of cvd_raft_sepconv_gru_device.  Scratch (768 batch height width floats and the
 * GRU's) belongs to the handle and keeps its high-water size, under the GRU's rule: calls on one device must be ordered on one
 * stream; a call that has to grow the scratch allocates, every later call of that size only enqueues.
 *   net, inp          [batch][128][height][width];  corr [batch][corr_channels][height][width];  flow [batch][2][height][width]
 *   cor_planes        in_channels of encoder.convc1.weight (corr_levels (2 corr_radius + 1)^2 = 324 in RAFT); must equal corr_channels
 *   weights, biases   host arrays of 15 device arrays in the order encoder.convc1, encoder.convc2, encoder.convf1, encoder.convf2,
 *                     encoder.conv, gru.convz1, gru.convr1, gru.convq1, gru.convz2, gru.convr2, gru.convq2, flow_head.conv1,
 *                     flow_head.conv2, mask.0, mask.2, in torch's layout and the reference's shapes; the GRU's 16-byte aligned
 *   net_out [batch][128][height][width], delta_flow [batch][2][height][width], mask [batch][576][height][width] or NULL (not
 *   computed); none may overlap an input or another output.
 * Rejected before any device work: sizes < 1, corr_channels != cor_planes, null arrays, overlapping arrays, a GRU weight that is
 * not 16-byte aligned. */
int32_t cvd_raft_update_block_device(cvd_handle* h, int32_t batch, int32_t height, int32_t width, int32_t corr_channels,
                                     int32_t cor_planes, const float* net, const float* inp, const float* corr, const float* flow,
                                     const float* const* weights, const float* const* biases, float* net_out, float* delta_flow,
                                     float* mask, void* stream);
/* The same call for measurement (tools/raftblock_bench.py): HIP events around every launch on `stream` and host waits;
 * kernel_ms[12] = {convc1, convc2, convf1, convf2, conv (with the flow copy), the GRU's four as in cvd_raft_sepconv_gru_timed,
 * flow_head.conv1 | mask.0, flow_head.conv2, mask.2 (0 with a null mask)} in milliseconds. */
int32_t cvd_raft_update_block_timed(cvd_handle* h, int32_t batch, int32_t height, int32_t width, int32_t corr_channels,
                                    int32_t cor_planes, const float* net, const float* inp, const float* corr, const float* flow,
                                    const float* const* weights, const float* const* biases, float* net_out, float* delta_flow,
                                    float* mask, void* stream, double* kernel_ms);

/* ---- RAFT's feature and context encoders, DESIGN.md §3.18 -- reference raft/core/extractor.py:8-60 (ResidualBlock) and :124-197
 * (BasicEncoder); SmallEncoder and BottleneckBlock are out of scope.  Independent of cvd_set_video.  f32, forward only, eval mode.
 * DEVICE arrays, enqueued on `stream`: kernel launches only, no copy, no host synchronisation, no atomics; every output element is
 * written once in a fixed operation order, so results repeat bit for bit and an image's result does not depend on its batch.
 *
 * One convolution -- square filter of kernel_size 1, 3 or 7, stride 1 or 2, padding kernel_size / 2, ONE launch:
 *   x [batch][in_channels][height][width] -> out [batch][out_channels][ho][wo], ho = (height - 1) / stride + 1, wo alike
 *   y = bias[o] + sum_{c,i,j} weight[o][c][i][j] x[b][c][stride y + i - r][stride x + j - r], the input outside the image counting 0;
 *   norm != NULL: a host array of four device vectors [out_channels] in the state dict's order {weight, bias, running_mean,
 *                 running_var} of an nn.BatchNorm2d in eval mode: y = (y - running_mean) / sqrt(running_var + eps) * weight + bias
 *   relu != 0:    y = max(y, 0)
 *   residual != NULL ([batch][out_channels][ho][wo]): y = max(residual + y, 0)
 * weight is torch's [out_channels][in_channels][k][k], any alignment (float4 loads where its rows start on 16 bytes).  out must
 * not overlap x, the weights or the residual.
 * Rejected before any device work, with an error that names the value: null arrays, sizes < 1, a filter other than 1, 3, 7, a stride
 * other than 1, 2, relu other than 0, 1, eps <= 0 with a norm, height width above 2^31, an output that overlaps x or the residual. */
int32_t cvd_raft_encoder_conv_device(cvd_handle* h, int32_t batch, int32_t height, int32_t width, int32_t in_channels,
                                     int32_t out_channels, int32_t kernel_size, int32_t stride, const float* x, const float* weight,
                                     const float* bias, const float* const* norm, float eps, int32_t relu, const float* residual,
                                     float* out, void* stream);
/* nn.InstanceNorm2d(affine=False, track_running_stats=False) per (image, channel) plane of x [batch][channels][height][width]:
 *   y = (x - mean) / sqrt(var + eps), var the biased variance; relu and residual as above.  Two launches: the statistics (mean first,
 *   then squared deviations from it, f64 sums in a fixed order; two doubles per plane in scratch of the handle, under the rule of
 *   cvd_raft_sepconv_gru_device) and the elementwise pass.  out may BE x (in place); any other overlap of out with x or the residual,
 *   planes of one element (the reference: "Expected more than 1 spatial element"), eps <= 0, null arrays, sizes < 1 and
 *   height width above 2^31 are rejected before any device work. */
int32_t cvd_raft_instance_norm_device(cvd_handle* h, int32_t batch, int32_t channels, int32_t height, int32_t width, const float* x,
                                      float eps, int32_t relu, const float* residual, float* out, void* stream);
/* BasicEncoder.forward in eval mode (no dropout):
 *   images     [batch][3][height][width], already scaled to [-1, 1]
 *   norm_mode  0 none, 1 instance, 2 batch (eval: running statistics); eps is the norms' (1e-5 in torch)
 *   weights, biases   host arrays of 16 device arrays in the state dict's order: conv1, layer1.0.conv1, layer1.0.conv2,
 *              layer1.1.conv1, layer1.1.conv2, layer2.0.conv1, layer2.0.conv2, layer2.0.downsample.0, layer2.1.conv1, layer2.1.conv2,
 *              layer3.0.conv1, layer3.0.conv2, layer3.0.downsample.0, layer3.1.conv1, layer3.1.conv2, conv2 ([output_dim][128][1][1])
 *   norms      batch only (else ignored, may be NULL): host array of 15 x 4 device vectors, norm i belonging to convolution i (norm1,
 *              layer1.0.norm1, layer1.0.norm2, .., layer2.0.norm3 (= downsample.1), ..), each as {weight, bias, running_mean,
 *              running_var}
 *   out        [batch][output_dim][ceil(height / 8)][ceil(width / 8)]
 * 16 launches of the convolution above (none, batch); instance: 15 more of each of the two norm kernels.  Intermediates are scratch
 * of the handle (high-water size, grown before the first launch) under the GRU's rule: calls on one device are ordered on one stream.
 * The result equals, bit for bit, the stages chained through the two entry points above.
 * Rejected before any device work: null arrays, sizes < 1, an unknown norm_mode, eps <= 0 with a norm, height width above 2^31,
 * feature planes of one element under instance norm, an output that overlaps the images. */
int32_t cvd_raft_encoder_device(cvd_handle* h, int32_t batch, int32_t height, int32_t width, int32_t output_dim, int32_t norm_mode,
                                float eps, const float* images, const float* const* weights, const float* const* biases,
                                const float* const* norms, float* out, void* stream);
/* The same call for measurement (tools/raftenc_bench.py): HIP events around every launch on `stream` and a host wait;
 * kernel_ms[48]: entry 3 i is convolution i, 3 i + 1 and 3 i + 2 the statistics and the elementwise pass of the instance norm behind
 * it (0 where there is none), in milliseconds. */
int32_t cvd_raft_encoder_timed(cvd_handle* h, int32_t batch, int32_t height, int32_t width, int32_t output_dim, int32_t norm_mode,
                               float eps, const float* images, const float* const* weights, const float* const* biases,
                               const float* const* norms, float* out, void* stream, double* kernel_ms);

/* ---- The decoder of MiDaS v2.1, DESIGN.md §3.19 -- reference monodepth/midas_v2/midas_net.py:57-74 behind the backbone and
 * blocks.py:41-159 (Interpolate, ResidualConvUnit, FeatureFusionBlock).  The ResNeXt backbone, backward and DepthModel's file I/O are
 * out of scope.  Independent of cvd_set_video.  f32, forward only.  DEVICE arrays, enqueued on `stream`: kernel launches only, no
 * copy, no host synchronisation, no atomics; every output element is written once in a fixed operation order, so results repeat bit
 * for bit and an image's result does not depend on its batch.
 *
 * One convolution -- square filter of kernel_size 1 or 3, stride 1, padding kernel_size / 2:
 *   x [batch][in_channels][height][width] -> out [batch][out_channels][height][width]
 *   sum  = sum_{c,i,j} weight[o][c][i][j] x'[b][c][y + i - r][x + j - r], x' = max(x, 0) with relu_in, else x (x itself is not
 *          modified), the input outside the image counting 0
 *   t    = sum + bias[o] (bias may be NULL: t = sum);  relu != 0: t = max(t, 0)
 *   a != NULL ([batch][out_channels][height][width]): t = t + (relu_a ? max(a, 0) : a)
 *   b != NULL (like a): out = b + t, else out = t
 * (a ResidualConvUnit rectifies its input in place, so its `out + x` adds max(x, 0): a with relu_a; b is the other path of
 * FeatureFusionBlock's `output += resConfUnit1(xs[1])`.)
 * split: 0 = the rule, S = a function of in_channels kernel_size^2 and height width alone (cvd_midas.h: midasSplit); 1 .. the chunks
 * of K = forced (tests, measurement).  With S > 1 the S slices of K write partial sums to scratch of the handle [S][batch]
 * [out_channels][height][width] and a second launch sums them in f64 in the order s = 0 .. S - 1, rounds once and applies the
 * epilogue.  The scratch follows the rule of cvd_raft_sepconv_gru_device (high-water size, grown before the first launch; calls on
 * one device are ordered on one stream).  out must not overlap x, a or b.
 * Rejected before any device work, with an error that names the value: null arrays (bias, a, b may be NULL), sizes < 1, a filter
 * other than 1, 3, flags other than 0, 1, a split outside its range, height width above 2^31, an output that overlaps an input. */
int32_t cvd_midas_conv_device(cvd_handle* h, int32_t batch, int32_t height, int32_t width, int32_t in_channels, int32_t out_channels,
                              int32_t kernel_size, const float* x, const float* weight, const float* bias, int32_t relu_in, int32_t relu,
                              const float* a, int32_t relu_a, const float* b, int32_t split, float* out, void* stream);
/* Bilinear x 2 as torch.nn.functional.interpolate(scale_factor=2, mode="bilinear") with align_corners != 0 (FeatureFusionBlock) or
 * 0 (Interpolate): x [batch][channels][height][width] -> out [batch][channels][2 height][2 width], ONE launch, one thread per output
 * element; a 1 x 1 input gives four copies.  out must not overlap x. */
int32_t cvd_midas_upsample2x_device(cvd_handle* h, int32_t batch, int32_t channels, int32_t height, int32_t width, int32_t align_corners,
                                    const float* x, float* out, void* stream);
/* The output head behind Interpolate in ONE launch: output_conv.2 (in_channels -> mid_channels = 32, 3 x 3), ReLU, output_conv.4
 * (32 -> 1, 1 x 1), and ReLU where non_negative != 0:
 *   x [batch][in_channels][height][width], weight2 [32][in_channels][3][3], bias2 [32], weight4 [1][32][1][1], bias4 [1]
 *   -> out [batch][height][width].  The 32-channel tensor is never written.  mid_channels other than 32 is refused. */
int32_t cvd_midas_head_device(cvd_handle* h, int32_t batch, int32_t height, int32_t width, int32_t in_channels, int32_t mid_channels,
                              const float* x, const float* weight2, const float* bias2, const float* weight4, const float* bias4,
                              int32_t non_negative, float* out, void* stream);
/* MidasNet.forward behind the backbone:
 *   channels4, heights4, widths4   host arrays: the four feature maps' sizes, layer1 first; heights4[k] = 2 heights4[k + 1] exactly,
 *              widths alike (images whose sides are multiples of 32)
 *   maps       host array of the 4 device arrays [batch][channels4[k]][heights4[k]][widths4[k]]; they are read only
 *   weights    host array of 21 device arrays in the state dict's order without refinenet4.resConfUnit1 (which never runs):
 *              layer1_rn .. layer4_rn, refinenet4.resConfUnit2.{conv1, conv2}, refinenet3.resConfUnit1.{conv1, conv2},
 *              refinenet3.resConfUnit2.{conv1, conv2}, refinenet2 and refinenet1 alike, output_conv.0, output_conv.2, output_conv.4
 *   biases     host array of 17 device arrays: those of weights 4 .. 20 (the layerK_rn convolutions have none)
 *   out        [batch][4 heights4[0]][4 widths4[0]]
 * 19 launches of the convolution above (and the folds of those that split), 5 upsamplings and the head.  Intermediates are scratch of
 * the handle under the same rule.  The result equals, bit for bit, the stages chained through the three entry points above.
 * Rejected before any device work: null arrays, sizes < 1, feature maps that are not exact halvings, height width above 2^31, an
 * output that overlaps a feature map. */
int32_t cvd_midas_decoder_device(cvd_handle* h, int32_t batch, int32_t features, const int32_t* channels4, const int32_t* heights4,
                                 const int32_t* widths4, const float* const* maps, const float* const* weights,
                                 const float* const* biases, int32_t non_negative, float* out, void* stream);
/* The same call for measurement (tools/midas_bench.py): HIP events around every launch on `stream` and a host wait; kernel_ms[44]:
 * entry 2 i is convolution i of the weight table (i = 0 .. 18), 2 i + 1 its fold (0 without a split), 38 .. 42 the upsamplings in the
 * order they run, 43 the head, in milliseconds. */
int32_t cvd_midas_decoder_timed(cvd_handle* h, int32_t batch, int32_t features, const int32_t* channels4, const int32_t* heights4,
                                const int32_t* widths4, const float* const* maps, const float* const* weights,
                                const float* const* biases, int32_t non_negative, float* out, void* stream, double* kernel_ms);

/* ---- Backward of the decoder's layers, DESIGN.md §3.21 (csrc/cvd_midas_grad.h): what torch's autograd computes for the reference's
 * nn.Conv2d(stride 1, padding kernel_size / 2) -- monodepth/midas_v2/blocks.py:39-50 (layerK_rn), 100-107 (ResidualConvUnit),
 * midas_net.py:36-40 (output_conv) -- and for nn.functional.interpolate(scale_factor=2, mode="bilinear") -- blocks.py:54-84
 * (Interpolate), 155-157 (FeatureFusionBlock) -- and for the output head; then the whole decoder's training forward and backward as
 * one call each, which robust_cvd_amd/midas_train.py's MidasNet uses.  f32, DEVICE
 * arrays, enqueued on `stream`: kernel launches only, no copy, no host synchronisation, no atomics; every output element is written
 * once in a fixed operation order, so results repeat bit for bit.  Scratch of the handle under the rule of cvd_midas_conv_device.
 *
 * Input gradient of one convolution, gy [batch][out_channels][height][width], weight [out_channels][in_channels][k][k] ->
 * gx [batch][in_channels][height][width]:
 *   sum = sum_{n,i,j} gy[b][n][y - i + r][x - j + r] weight[n][c][i][j], gy outside the image counting 0
 *   t   = sum;  add != NULL (like gx): t = t + add;  mask != NULL (like gx): t = mask > 0 ? t : 0   (torch's ReLU: gradient 0 at 0)
 * (a ResidualConvUnit's input ReLU is the mask; its skip path the addend: (dgrad(g) + gy) [x > 0].)  It runs cvd_midas_conv_device's
 * kernel on the transposed, flipped filter (a small launch writes it to scratch): the same padding scheme and the same split rule
 * from K = out_channels k k and height width alone, so a batch's gradients are the bits of its images one by one; the partial sums
 * are summed in f64 in slice order and rounded once, then the epilogue.  split: 0 = the rule, 1 .. the chunks of K = forced.
 * Rejected before any device work: null arrays (add, mask may be NULL), sizes < 1, a filter other than 1, 3, a split outside its
 * range, height width above 2^31, gx overlapping gy, weight, add or mask. */
int32_t cvd_midas_conv_grad_input_device(cvd_handle* h, int32_t batch, int32_t height, int32_t width, int32_t in_channels,
                                         int32_t out_channels, int32_t kernel_size, const float* gy, const float* weight, const float* add,
                                         const float* mask, int32_t split, float* gx, void* stream);
/* Weight and bias gradient of one convolution, gy as above, x [batch][in_channels][height][width] the convolution's input ->
 * g_weight [out_channels][in_channels][k][k], g_bias [out_channels] (NULL: not computed):
 *   g_weight[n][c][i][j] = sum_{b,y,x} gy[b][n][y][x] x'[b][c][y + i - r][x + j - r], x' = max(x, 0) with relu_in, else x, 0 outside
 *   g_bias[n]            = sum_{b,y,x} gy[b][n][y][x]   (f64 sums in a fixed order, rounded once)
 * A GEMM over the batch height width pixels on the exact f32 MFMA: fmaf chains of 256 pixels in pixel order, each added to a second
 * register set as it completes.  split: 0 = the rule, S = a function of (batch height width, out_channels, in_channels k k) alone
 * (cvd_midas_grad.h: midasWgradSplit); 1 .. 128 = forced (it shrinks to whole chains, no slice empty).  With S > 1 the S slices of the
 * pixels write partial sums to scratch [S][out_channels][in_channels k k] and a second launch sums them in f64 in the order
 * s = 0 .. S - 1 and rounds once.
 * Rejected before any device work: null arrays (g_bias may be NULL), sizes < 1, a filter other than 1, 3, a flag other than 0, 1, a
 * split outside its range, height width above 2^31, a gradient that overlaps an input or the other gradient. */
int32_t cvd_midas_conv_grad_weight_device(cvd_handle* h, int32_t batch, int32_t height, int32_t width, int32_t in_channels,
                                          int32_t out_channels, int32_t kernel_size, const float* gy, const float* x, int32_t relu_in,
                                          int32_t split, float* g_weight, float* g_bias, void* stream);
/* Backward of cvd_midas_upsample2x_device: gy [batch][channels][2 height][2 width] -> gx [batch][channels][height][width], ONE launch
 * in gather form: one thread per element of gx sums the (at most 8 x 8 candidates, classified by the forward's own f32 source
 * coordinate) outputs that read it, with the forward's f32 weights, rows then columns ascending.  On a 1 x 1 input gx is the sum of
 * the four gy.  gx must not overlap gy. */
int32_t cvd_midas_upsample2x_grad_device(cvd_handle* h, int32_t batch, int32_t channels, int32_t height, int32_t width,
                                         int32_t align_corners, const float* gy, float* gx, void* stream);

/* Backward of cvd_midas_head_device (midas_net.py:38-41), y = relu?(b4 + sum_n w4[n] relu(t_n)), t = output_conv.2(x) + bias2:
 *   g_s = gy [y > 0] with non_negative, else gy;  g32[n] = g_s w4[n] [t_n > 0]
 *   g_weight4[n] = sum_p g_s relu(t_n), g_bias4 = sum_p g_s: f64 products and sums, per workgroup then over the workgroups in order
 *   g_weight2, g_bias2 = the weight gradient above on (g32, x);  gx = the input gradient above on (g32, weight2)
 * gy [batch][height][width], x and the parameters as cvd_midas_head_device -> gx like x, the four parameter gradients like their
 * parameters.  The forward never writes t: it is recomputed in scratch by cvd_midas_conv_device's kernel with one slice, whose chain
 * per element is the head launch's own, so the masks come from the forward's own f32 t; y is recomputed by the head launch.
 * Rejected before any device work: null arrays, sizes < 1, mid_channels other than 32, a flag other than 0, 1, an output that
 * overlaps an input or another output. */
int32_t cvd_midas_head_grad_device(cvd_handle* h, int32_t batch, int32_t height, int32_t width, int32_t in_channels, int32_t mid_channels,
                                   const float* gy, const float* x, const float* weight2, const float* bias2, const float* weight4,
                                   const float* bias4, int32_t non_negative, float* gx, float* g_weight2, float* g_bias2, float* g_weight4,
                                   float* g_bias4, void* stream);

/* cvd_midas_decoder_device for training (midas_net.py:57-74 under autograd): the same launches with the same arguments -- out equals
 * cvd_midas_decoder_device's bit for bit -- but the activations the backward reads are written to the caller's table instead of
 * scratch.  saved16: host array of 16 device arrays, shapes as api.midas_saved_shapes:
 *   0 .. 3   the layerK_rn results [batch][features][heights4[k]][widths4[k]]
 *   4        refinenet4.resConfUnit2.conv1's result (level 4)
 *   5 .. 13  for refinenet3, refinenet2, refinenet1 three each at their level: resConfUnit1.conv1's result, the fusion sum
 *            (resConfUnit2's input), resConfUnit2.conv1's result
 *   14       output_conv.0's input  [batch][features][2 heights4[0]][2 widths4[0]]
 *   15       output_conv.0's result [batch][128][2 heights4[0]][2 widths4[0]]
 * The 128-channel full-resolution tensor (the head's input) is NOT saved: the backward recomputes it from entry 15 with the forward's
 * own upsampling launch, the same bits, for a quarter of the memory.  Rejected like cvd_midas_decoder_device, and: a null saved
 * table or entry, a saved tensor that overlaps out or a feature map. */
int32_t cvd_midas_decoder_train_device(cvd_handle* h, int32_t batch, int32_t features, const int32_t* channels4, const int32_t* heights4,
                                       const int32_t* widths4, const float* const* maps, const float* const* weights,
                                       const float* const* biases, int32_t non_negative, float* const* saved16, float* out, void* stream);
/* The decoder's backward in ONE call: gy [batch][4 heights4[0]][4 widths4[0]], the feature maps, the saved table and the parameters ->
 * g_weights (21) and g_biases (17) in the order of the weight and bias tables, and g_maps (4, like maps; NULL skips the four
 * layerK_rn input gradients).  It chains the four entry points above in the reverse of the forward's order (the head on the
 * recomputed input, output_conv.0, then refinenet1 .. refinenet4 with their layerK_rn), so its results equal theirs bit for bit,
 * repeat bit for bit, and the map gradients of a batch are those of its images one by one.  Intermediates are scratch of the handle.
 * Rejected before any device work: null arrays or entries (g_maps may be NULL), sizes < 1, feature maps that are not exact halvings,
 * a flag other than 0, 1, and what the four entry points reject. */
int32_t cvd_midas_decoder_backward_device(cvd_handle* h, int32_t batch, int32_t features, const int32_t* channels4, const int32_t* heights4,
                                          const int32_t* widths4, const float* gy, const float* const* maps, const float* const* saved16,
                                          const float* const* weights, const float* const* biases, int32_t non_negative,
                                          float* const* g_weights, float* const* g_biases, float* const* g_maps, void* stream);
/* The same call for measurement (tools/midas_grad_bench.py): HIP events around every operator call it makes (each one to three
 * launches: transform or convolution, fold, bias) on `stream` and a host wait; kernel_ms[48]: the stages in the order they run
 * (api.midas_backward_stages names them), the rest 0, in milliseconds. */
int32_t cvd_midas_decoder_backward_timed(cvd_handle* h, int32_t batch, int32_t features, const int32_t* channels4, const int32_t* heights4,
                                         const int32_t* widths4, const float* gy, const float* const* maps, const float* const* saved16,
                                         const float* const* weights, const float* const* biases, int32_t non_negative,
                                         float* const* g_weights, float* const* g_biases, float* const* g_maps, void* stream,
                                         double* kernel_ms);

/* ---- the backbone of MiDaS v2.1 (csrc/cvd_resnext.h): torchvision's ResNet(Bottleneck, blocks, groups,
 * width_per_group) in eval mode -- the ResNeXt-101 32x8d that the reference's monodepth/midas_v2/blocks.py:6-31 builds -- on device
 * arrays, f32, forward only, launches on `stream` with no host synchronisation.  No atomics: a call repeats bit for bit.  An axis of
 * `height` gives (height - 1) / stride + 1 outputs.  norm: host array of the 4 device vectors {weight, bias, running_mean,
 * running_var} of the nn.BatchNorm2d behind the convolution, applied as y = (y - mean) / sqrt(var + eps) * weight + bias, or null
 * for none. ---- */
/* nn.Conv2d(groups channels_per_group, groups channels_per_group, 3, stride, padding=1, groups=groups, bias=False), the norm, and
 * ReLU where relu != 0, in ONE launch:
 *   x [batch][groups channels_per_group][height][width], weight [groups channels_per_group][channels_per_group][3][3] (torch's
 *   layout) -> out [batch][groups channels_per_group][ho][wo].
 * channels_per_group is 8, 16, 32 or 64 (the four stages of 32x8d); any groups >= 1; stride 1 or 2.  Rejected before any device
 * work, with an error that names the value: null arrays, sizes < 1, another channels_per_group or stride, eps <= 0 with a norm,
 * height width above 2^31, an output that overlaps the input. */
int32_t cvd_resnext_grouped_conv_device(cvd_handle* h, int32_t batch, int32_t height, int32_t width, int32_t groups,
                                        int32_t channels_per_group, int32_t stride, const float* x, const float* weight,
                                        const float* const* norm, float eps, int32_t relu, float* out, void* stream);
/* The dense convolutions, WITHOUT bias: kernel_size 7 at stride 2 (the stem, padding 3) or kernel_size 1 at stride 1 or 2, then the
 * norm, ReLU where relu != 0, and with a residual [batch][out_channels][ho][wo] y = max(residual + y, 0):
 *   x [batch][in_channels][height][width], weight [out_channels][in_channels][kernel_size][kernel_size] -> out [batch][out_channels][ho][wo].
 * split: 0 = the rule -- K = in_channels kernel_size^2 is cut into as many slices as bring the 64-pixel tiles of ONE image's output
 * to 64 workgroups, whole chains each (8 chunks of 32 channels; 3 chunks of 2 channels x 49 taps), at most 32; a function of K and
 * ho wo alone -- otherwise the forced slice count (1 .. the chunks of K).  A split convolution is two launches: partial sums to
 * scratch of the handle (the GRU's rule: calls on one device are ordered on one stream), then a fold in f64 in slice order, rounded
 * once, with the epilogue.  Rejected before any device work: as above, a kernel_size / stride pair that is not built, a split
 * outside its range, an output that overlaps x or the residual. */
int32_t cvd_resnext_conv_device(cvd_handle* h, int32_t batch, int32_t height, int32_t width, int32_t in_channels, int32_t out_channels,
                                int32_t kernel_size, int32_t stride, const float* x, const float* weight, const float* const* norm,
                                float eps, int32_t relu, const float* residual, int32_t split, float* out, void* stream);
/* nn.MaxPool2d(3, 2, 1): x [batch][channels][height][width] -> out [batch][channels][ho][wo] at stride 2, ONE launch, one thread per
 * output element; padding counts as minus infinity.  out must not overlap x. */
int32_t cvd_resnext_maxpool_device(cvd_handle* h, int32_t batch, int32_t channels, int32_t height, int32_t width, const float* x,
                                   float* out, void* stream);
/* ResNet.forward up to layer4, as MidasNet.forward reads it:
 *   blocks4    host array: the block counts of layer1 .. layer4 ((3, 4, 23, 3) with groups 32, width_per_group 8 is ResNeXt-101
 *              32x8d: 104 convolutions and one pool)
 *   images     [batch][3][height][width], height and width multiples of 32
 *   weights    host array of one device array per convolution in the state dict's order: conv1 (the stem), then per block conv1,
 *              conv2, conv3 and, in every stage's first block, downsample.0.  Stage k has planes = 64 2^k, width = planes
 *              width_per_group / 64 * groups: conv1 1 x 1 in -> width, conv2 grouped 3 x 3 with the block's stride, conv3 1 x 1
 *              width -> 4 planes, downsample.0 1 x 1 with the stride (torchvision's v1.5 form)
 *   norms      host array of 4 device vectors per convolution, {weight, bias, running_mean, running_var}, in the same order
 *   outs4      host array of the four caller-owned output maps [batch][256 2^k][height / 2^(k+2)][width / 2^(k+2)]
 * One launch per convolution (and the folds of those that split) and the pool.  Intermediates are scratch of the handle under the
 * same rule.  The result equals, bit for bit, the stages chained through the three entry points above.
 * Rejected before any device work: null arrays, sizes < 1, channels per group that are not built, eps <= 0, image sides that are not
 * multiples of 32, height width above 2^31, output maps that overlap the images or each other. */
int32_t cvd_midas_backbone_device(cvd_handle* h, int32_t batch, int32_t height, int32_t width, const int32_t* blocks4, int32_t groups,
                                  int32_t width_per_group, float eps, const float* images, const float* const* weights,
                                  const float* const* norms, float* const* outs4, void* stream);
/* The same call for measurement (tools/midasnet_bench.py): HIP events around every launch on `stream` and a host wait; kernel_ms
 * [2 n + 1] for n convolutions: entry 2 i is convolution i of the weight table, 2 i + 1 its fold (0 without a split), 2 n the pool,
 * in milliseconds. */
int32_t cvd_midas_backbone_timed(cvd_handle* h, int32_t batch, int32_t height, int32_t width, const int32_t* blocks4, int32_t groups,
                                 int32_t width_per_group, float eps, const float* images, const float* const* weights,
                                 const float* const* norms, float* const* outs4, void* stream, double* kernel_ms);

/* ---- the same backbone in training (csrc/cvd_resnext_grad.h): nn.BatchNorm2d on batch statistics and what torch's
 * autograd computes for the backbone's layers, on device arrays, f32, launches on `stream` with no host synchronisation.  No atomics:
 * every reduction runs in a fixed order in f64 and is rounded once, so a call repeats bit for bit.  Scratch is the handle's (calls
 * on one device are ordered on one stream).  `height` and `width` are those of the layer's INPUT; ho = (height - 1) / stride + 1.
 * Every entry point rejects, before any device work and with an error that names the value: null arrays, sizes < 1, outputs that
 * overlap an input or each other, and (channels per group, stride, kernel_size) combinations that are not built. ---- */
/* nn.BatchNorm2d behind a convolution called with a null norm: c [batch][channels][height][width] is its raw output.
 *   training != 0: mean and biased variance of each channel over M = batch height width in f64 (sums of x and x^2, dealt to slices by
 *   a rule of (channels, M) and added in slice order); save_mean and save_invstd = 1 / sqrt(var + eps) rounded once to f32;
 *   running = (1 - momentum) running + momentum stat with the unbiased variance M / (M - 1).  M = 1 is rejected.
 *   training == 0: save_mean = running_mean, save_invstd = 1 / sqrt(running_var + eps); nothing else is updated.
 * Then y = (c - save_mean) save_invstd gamma + beta; max(y, 0) where relu != 0; with a residual (or null) max(residual + y, 0). */
int32_t cvd_resnext_norm_train_device(cvd_handle* h, int32_t batch, int32_t channels, int32_t height, int32_t width, const float* c,
                                      const float* gamma, const float* beta, float* running_mean, float* running_var, double eps,
                                      double momentum, int32_t training, int32_t relu, const float* residual, float* save_mean,
                                      float* save_invstd, float* y, void* stream);
/* Its backward.  y (or null): the tensor the forward wrote, given where the forward applied a ReLU or the residual form; then
 * g = gy where y > 0, else 0.  g_beta = sum g, g_gamma = sum g xhat with xhat = (c - mean) invstd, f64 sums rounded once.
 * training != 0: gc = gamma invstd (g - g_beta / M - xhat g_gamma / M); else gc = g gamma invstd.  g_residual (or null) = g. */
int32_t cvd_resnext_norm_grad_device(cvd_handle* h, int32_t batch, int32_t channels, int32_t height, int32_t width, const float* gy,
                                     const float* c, const float* y, const float* mean, const float* invstd, const float* gamma,
                                     int32_t training, float* gc, float* g_gamma, float* g_beta, float* g_residual, void* stream);
/* The grouped 3 x 3 convolution of cvd_resnext_grouped_conv_device: gy [batch][groups channels_per_group][ho][wo] ->
 * gx [batch][groups channels_per_group][height][width] (ONE launch, gather form), resp. with the convolution's input x ->
 * g_weight [groups channels_per_group][channels_per_group][3][3].  split: 0 = the rule -- the output pixels are dealt to as many
 * slices of whole chains of 256 pixels as bring the launch to 1024 workgroups, at most 128; a function of the pixel and weight
 * counts alone -- otherwise the forced slice count (1 .. 128; it shrinks to whole chains). */
int32_t cvd_resnext_grouped_conv_grad_input_device(cvd_handle* h, int32_t batch, int32_t height, int32_t width, int32_t groups,
                                                   int32_t channels_per_group, int32_t stride, const float* gy, const float* weight,
                                                   float* gx, void* stream);
int32_t cvd_resnext_grouped_conv_grad_weight_device(cvd_handle* h, int32_t batch, int32_t height, int32_t width, int32_t groups,
                                                    int32_t channels_per_group, int32_t stride, const float* gy, const float* x,
                                                    int32_t split, float* g_weight, void* stream);
/* The dense convolutions of cvd_resnext_conv_device.  Input gradient: kernel_size 1 at stride 1 or 2 (the stem's images need none):
 * gx = conv_transpose(gy, weight) + add (add or null: [batch][in_channels][height][width], the residual branch's gradient); at
 * stride 2 gx is exactly `add` (or zero) at the odd positions.  Weight gradient: kernel_size 1 at stride 1 or 2, and kernel_size 7
 * at stride 2.  The 1 x 1 paths run cvd_midas_conv_grad_input_device / _grad_weight_device (at stride 2 around a scatter resp. a
 * gather); split is the weight gradient's, as there resp. as above for the stem. */
int32_t cvd_resnext_conv_grad_input_device(cvd_handle* h, int32_t batch, int32_t height, int32_t width, int32_t in_channels,
                                           int32_t out_channels, int32_t kernel_size, int32_t stride, const float* gy, const float* weight,
                                           const float* add, float* gx, void* stream);
int32_t cvd_resnext_conv_grad_weight_device(cvd_handle* h, int32_t batch, int32_t height, int32_t width, int32_t in_channels,
                                            int32_t out_channels, int32_t kernel_size, int32_t stride, const float* gy, const float* x,
                                            int32_t split, float* g_weight, void* stream);
/* Backward of cvd_resnext_maxpool_device: x [batch][channels][height][width] its input, gy [batch][channels][ho][wo] ->
 * gx [batch][channels][height][width].  Each window's gradient goes to its argmax as torch picks it (row-major scan, padding
 * excluded, the first maximum wins, a NaN wins). */
int32_t cvd_resnext_maxpool_grad_device(cvd_handle* h, int32_t batch, int32_t channels, int32_t height, int32_t width, const float* x,
                                        const float* gy, float* gx, void* stream);
/* One torchvision Bottleneck (v1.5) per call, training form: conv1 1 x 1 in_channels -> mid_channels, bn1, ReLU; conv2 grouped 3 x 3
 * with the stride, bn2, ReLU; downsample.0 1 x 1 with the stride and downsample.1 where downsample != 0; conv3 1 x 1 -> out_channels,
 * bn3, + identity, ReLU.
 *   weights    host array of the 3 (4) device weights: conv1, conv2, conv3 (, downsample.0)
 *   norms      host array of 4 device vectors per convolution {weight, bias, running_mean, running_var}; the running statistics
 *              of a norm whose flag in `training` (host array, one per convolution) is != 0 are updated
 *   saved      host array of 4 caller-owned device tensors per convolution {c, mean, invstd, y}: the raw convolution output, the
 *              two saved vectors and the post-activation tensor; y of conv3 is the block's OUTPUT, y of downsample.0 the identity
 *              (shapes: api.resnext_block_saved_shapes).  Everything is saved, nothing is recomputed.
 * The backward writes gx (or null: skipped) [batch][in_channels][height][width], and per convolution g_weights, g_gammas, g_betas;
 * `gammas` is the host array of the norms' weights.  Both calls run the operator entry points above in order (the forward's
 * convolutions are cvd_resnext_conv_device / _grouped_conv_device with a null norm), so their results equal the chained operator
 * calls' bit for bit; the gradients between the operators are scratch of the handle. */
int32_t cvd_resnext_block_train_device(cvd_handle* h, int32_t batch, int32_t height, int32_t width, int32_t in_channels,
                                       int32_t mid_channels, int32_t out_channels, int32_t groups, int32_t stride, int32_t downsample,
                                       const float* x, const float* const* weights, float* const* norms, double eps, double momentum,
                                       const int32_t* training, float* const* saved, void* stream);
int32_t cvd_resnext_block_backward_device(cvd_handle* h, int32_t batch, int32_t height, int32_t width, int32_t in_channels,
                                          int32_t mid_channels, int32_t out_channels, int32_t groups, int32_t stride, int32_t downsample,
                                          const float* gy, const float* x, const float* const* weights, const float* const* gammas,
                                          const float* const* saved, const int32_t* training, float* gx, float* const* g_weights,
                                          float* const* g_gammas, float* const* g_betas, void* stream);

/* ---- measurement hooks (bench.py) --------------------------------------------------------------------- */
/* Average duration (ms) of the dominant kernels over the last solve, measured with HIP events on the
 * solver's own stream: fills {evaluate_assemble, matvec_pairs, matvec_finish, cg_update, block_inverse,
 * cost} and their launch counts. */
int32_t cvd_get_kernel_times(cvd_handle* h, double* avg_ms6, int64_t* launches6);
/* Exchange steps of the pair-sharded mode (RCCL on the solver stream), timed with HIP events whenever kernel timing is on:
 * fills {evaluation exchange: all-reduce g / cost, reduce-scatter H_ff, all-gather diag(H) and the f32 block inverses;
 * product exchange: per PCG iteration, owner-sharded update (default): reduce-scatter q to the frames' owners + all-reduce
 * [Z^T q | p.q] after the product, all-gather z / c / the r^T z shares after the update (two grouped collectives per iteration);
 * replicated update (dist_owner_update = 0): ONE all-reduce of [q | Z^T q | p.q]; coarse exchange: edge blocks, diagonal blocks}
 * -- average ms per occurrence and counts. */
int32_t cvd_get_comm_times(cvd_handle* h, double* avg_ms3, int64_t* counts3);
/* Dense mode (cvd_set_pair_flows) inside the explicit-block scope: the two kernels of the Jacobian evaluation that walk the pixels,
 * timed on their own whenever kernel timing is on -- {k_dense_walk: flow / mask / depth read once, every contribution of a pixel
 * constraint formed once (replaces the reference's per-constraint residual blocks, lib/PoseOptimizer.cpp:1185-1232, for
 * matchSeparation = 0, lib/FlowConstraints.cpp:381-395); k_dense_gg: grid x grid part of the cross blocks} -- average ms, launches. */
int32_t cvd_get_dense_times(cvd_handle* h, double* avg_ms2, int64_t* launches2);
/* Per-launch HIP-event timing: 0 = off (default), 1 = every class, otherwise a bit mask (bit k = class k in the
 * order of cvd_get_kernel_times). Two event records per timed launch. Bits 8..15 = sampling stride - 1 for the hot
 * kernel's start/stop events (0: every launch, 3: every 4th launch of k_matvec_pairs carries an event pair). */
int32_t cvd_set_kernel_timing(cvd_handle* h, int32_t enabled);
/* Number of (valid static) constraints in the compiled table of the last solve. */
int64_t cvd_num_active_constraints(cvd_handle* h);
/* Diagnostics (no counterpart in the reference): which variant of the linear solver the LAST solve of the handle ran --
 * out8 = { pose-graph level on, its form (0 exact sparse factor, 1 exact dense inverse, 2 temporal pose level), depth-grid
 * temporal level on, PCG tail (bit field), fused tail disabled after an abandoned barrier, depth taps per
 * sample (1 / 4 / 16), work items of the pair-major kernels, explicit cross blocks (dense mode) }.  tools/defaults_sweep.py.
 * out8[3], PCG tail: bit 0 = fused into one launch (k_pcg_tail); bit 1 = that launch's temporal-level workgroups staged their rows
 * of the inverse in LDS (set only together with bit 0).  Test bit 0, not == 1, for "fused". */
int32_t cvd_path_info(cvd_handle* h, int32_t* out8);

#ifdef __cplusplus
}
#endif

#endif /* CVD_HIP_H_ */
