/* include/cvd_hip_debug.h -- TEST and MEASUREMENT hooks of libcvd_hip.so.
 *
 * Nothing here is part of the drop-in boundary (include/cvd_hip.h): these entry points exist for tests/ (parity hooks, simulated
 * ranks on one GPU, forced code paths) and tools/ (profiling aids).  A caller of the library never needs them; the reference has
 * no counterpart for any of them.  They live in the same shared object so that the tests exercise the product binary.
 */
#ifndef CVD_HIP_DEBUG_H
#define CVD_HIP_DEBUG_H

#include "cvd_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Hooks that change what a solve does for the sake of a test or a measurement (per handle; all default 0 = the product path).
 * Until round 5 these sat in cvd_solver_options. */
typedef struct cvd_debug_options {
  uint64_t struct_size;          /* CVD_STRUCT_STAMP(cvd_debug_options): cvd_debug_options_default sets, cvd_set_debug_options checks */
  int32_t force_iterations;      /* measurement: ignore the convergence tests, run exactly max_iterations */
  int32_t force_sharded_path;    /* 1: a 1-rank communicator runs the multi-rank code path (owner chunks, exchange calls) */
  int32_t pcg_lockstep;          /* profiling: 1 = the host never enqueues a PCG iteration ahead of the convergence flag, so
                                    that per-launch counter averages contain no early-exit launches */
  int32_t stall_fused_tail_once; /* 1: the host treats the third PCG iteration of the handle's first solve as a stalled grid barrier
                                    of k_pcg_tail (exercises the fall-back to the two-launch tail; until round 5: pcg_fused_tail = 2) */
  int32_t tail_no_row_staging;   /* 1: the temporal levels' workgroups of k_pcg_tail read their rows of the inverse from memory behind
                                    the grid barrier (the path a launch takes when the staged rows would not fit the LDS or the device)
                                    instead of staging them in LDS in front of it; cvd_path_info reports which ran */
  int32_t tail_closes_scalars;   /* 1: k_pcg_tail always sums the r^T z shares and finishes the PCG scalars itself (its last workgroup),
                                    also where the next product would sum them in its prologue (the shares mode); cvd_path_info
                                    reports which ran */
  int32_t asm_force_stage_depth; /* the segment walk of the assembly (fast list kernel, SPEC 1 / 2): 0 = as many staging rows per wave
                                    for the other frame's parameters as the LDS holds (2, 1 or 0); 1 + k = exactly k rows (k = 0, 1, 2;
                                    an evaluation fails if they do not fit); cvd_assembly_launch_debug reports which ran */
  int32_t asm_force_part_units;  /* work list of the fast list assembly: 0 = the product rule for the units (128 constraints each) a part
                                    (one workgroup) gets at most; k > 0 = at most k, so that a test problem of a few frames has parts
                                    whose waves walk several units and segments as a 300-frame problem's do */
} cvd_debug_options;
void cvd_debug_options_default(cvd_debug_options* o);
int32_t cvd_set_debug_options(cvd_handle* h, const cvd_debug_options* o);

/* Test hook: 1 = run the generic all-variants kernels even where a specialised fast kernel exists. */
int32_t cvd_set_generic_kernels(cvd_handle* h, int32_t enabled);

/* Test backend of the exchange layer: the `world` ranks are handles of THIS process on ONE device, each driven by its
 * own host thread; handles that pass the same `group_key` form one group.  RCCL refuses two ranks on one device, so
 * this is how the multi-rank code paths run with world > 1 on a single-GPU box (tests/test_gpu_two_ranks.py).
 * Host-synchronous; never used by a multi-GPU run. */
int32_t cvd_comm_init_local_group(cvd_handle* h, int32_t rank, int32_t world, uint64_t group_key);
/* Measurement aid (tools/shard_sim.py): this handle becomes rank `rank` of a `world`-rank run whose OTHER ranks do not exist --
 * every collective returns at once and the other ranks' contributions are simply missing.  The sharded code path runs with the
 * real owner chunks, offsets and launch geometry of that rank, so its kernels can be timed on one GPU; the numbers the solve
 * produces mean nothing. */
int32_t cvd_comm_init_phantom(cvd_handle* h, int32_t rank, int32_t world);

/* Parity hook for the per-frame dense solve of the block-Jacobi preconditioner (no reference counterpart: Ceres'
 * SPARSE_NORMAL_CHOLESKY, lib/PoseOptimizer.cpp:956, is replaced by PCG): inverts `num_blocks` symmetric positive
 * definite block_size x block_size f64 matrices `a` (row-major, block after block) with the very kernel the solver uses
 * and returns the f32 inverses.  variant 0: blocked sweep on the f64 matrix cores (the default path), 1: scalar
 * register-tile sweep, 2: LDS Cholesky.  failed = number of non-positive pivots met. */
int32_t cvd_block_inverse_debug(cvd_handle* h, int32_t num_blocks, int32_t block_size, const double* a, int32_t variant,
                                float* inverse, int32_t* failed);

/* Test hook for the coarse level of the preconditioner (state of the last LM iteration of the last solve):
 * n = 8 * frames (0 when the level was off), a_c = Z^T (J^T J + diag(lam)) Z as a dense n x n matrix assembled
 * from its blocks, a_c_inverse = the inverse the solver applied, failed = pivot failures of the factorisation.
 * Any output pointer may be NULL. */
/* Test hook: the dense SPD inverse of the dense coarse level (cvd_dense_inverse.h) on one n x n f64 matrix (row-major,
 * symmetric); inverse = n x n f64; failed = 1 on a non-positive pivot (inverse untouched), bit 30 = barrier timeout. */
/* Parity hook of cvd_epipolar_static_flags: the same call, plus every hypothesis's inlier count counts_out [P][K] (-1: invalid
 * hypothesis or all-static pair) and its denormalised F hypotheses_out [P][K][9] (0 when invalid); either may be NULL. */
int32_t cvd_epipolar_debug(cvd_handle* h, int32_t num_pairs, const int64_t* offsets, const float* loc, double pixel_scale,
                           double threshold_px, int32_t iterations, uint64_t seed, uint8_t* is_static_out,
                           double* fundamental_out, int32_t* best_out, int32_t* counts_out, double* hypotheses_out);
/* Test and measurement hook of cvd_flow_consistency_masks: the same call with the thread-to-pixel map chosen by the caller --
 * pixels_per_thread 0 = the product choice (4 when width % 4 == 0, else 1), 1 = one pixel per thread, 4 = four consecutive
 * pixels of a row per thread (needs width % 4 == 0).  Both maps produce the same bits. */
int32_t cvd_flow_masks_debug(cvd_handle* h, int32_t num_frames, int32_t height, int32_t width, int32_t channels,
                             const float* color, int32_t num_pairs, const int32_t* pair_frames, const float* flow_ab,
                             const float* flow_ba, float flow_thresh, float color_thresh, uint8_t* mask_ab, uint8_t* mask_ba,
                             int32_t* kept, float* errors, double* kernel_ms, int32_t pixels_per_thread);
int32_t cvd_dense_inverse_debug(cvd_handle* h, int32_t n, const double* a, double* inverse, int32_t* failed);
int32_t cvd_coarse_debug(cvd_handle* h, int32_t* num_unknowns, double* a_c, double* a_c_inverse, int32_t* failed);
/* Test hook for the third level of the preconditioner (cvd_solver_options::temporal_level; state of its last build in the last
 * solve): dims6 = {NT unknowns (0: the level was off), S hats per node, nn nodes, step, Sx, Sy}; a_t = the assembled Galerkin
 * matrix (NT x NT, unknown s * nn + a, diagonal shifted by coarse_dense_shift), a_t_inverse = the inverse in use, lam = the LM
 * damping vector (frames x block) of the last LM iteration.  Any output pointer but dims6 may be NULL. */
int32_t cvd_temporal_debug(cvd_handle* h, int32_t* dims6, double* a_t, double* a_t_inverse, double* lam, int32_t* failed);
/* Test hook: what the handle's last product launch (PCG product, J^T J hook of cvd_evaluate) was.  out6 = {threads per workgroup,
 * SPEC (1 / 2: the compile-time ReproDisparity Cauchy / Huber variant, 0: runtime loss branches), KD (depth taps per side: 1, 4, 16),
 * kind (0: generic list kernel, 1: fast list kernel, 2: fast dense-mode kernel, 3: explicit cross blocks; -1: no product yet),
 * work items (= workgroups of the launch), compute units the workgroup-size rule counted}. */
int32_t cvd_product_launch_debug(cvd_handle* h, int32_t* out6);
/* Test hook: what the handle's last assembly launch (gradient and frame blocks of cvd_evaluate or of an LM iteration) was.  out8 =
 * {threads per workgroup, SPEC (as above), KD, kind (0: generic kernel, 1: fast list kernel, 2: fast dense-mode kernel, 3: fold of the
 * dense walk's records; -1: no assembly yet), workgroups of the launch (list mode: parts of the work list), parts that belong to
 * frames split into several parts (0: no frame is split), staging rows per wave of the segment walk (0, 1, 2; -1: the launch walked
 * units, not segments), segments of that walk's work list (0 with -1)}.  cost_frame (optional, one double per frame): the per-frame costs that
 * launch left behind -- a frame's regularisers and the constraints of the pairs it is the source of; their sum is the cost. */
int32_t cvd_assembly_launch_debug(cvd_handle* h, int32_t* out8, double* cost_frame);

#ifdef __cplusplus
}
#endif
#endif
