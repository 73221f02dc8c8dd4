"""Seeded problems that send a solve to the generic <KD, KS> kernels with a spatial transform (KS != 0).

Every kernel-level GPU test but the golden vectors resets the spatial transform to identity, so the generic kernels run there
with KS = 0 only (set_generic_kernels).  Of the six KS != 0 instantiations, (1,16) and (4,16) are compared with the oracle by no
kernel-level test, (16,4) by one test of tests/test_gpu_model_branches.py, and the golden vectors hold (1,4), (4,4), (16,16) on
pairs of at most about 40 constraints: one partial trip of a 256-thread workgroup.  The table
below is fixed and small: ten list-mode cases on small videos, two with scene-flow triplets, three on a workload-shaped item list
and an identity-spatial control.

  KD  depth taps: 1 global, 4 bilinear grid, 16 bicubic grid        KS  spatial taps: 4 VerticalLinear / CornersBilinear /
  loss 0 Euclidean, 1 disparity, 2 depth ratio, 3 log depth             BilinearGrid, 16 BicubicGrid (tapCounts, cvd_setup.hip)
  intr 0 fixed, 1 shared, 2 per frame                               robust 0 Cauchy, 1 Huber

The list-mode videos are synth.make_video(4, 64, 40, seed, spacing) -- the row-panel case 3 frames of 96 x 56 -- and the
spacing sets how often a 256-thread workgroup of k_assemble, which walks whole pairs, goes round a pair's constraints: 9 -> at
most 256 (one partial trip), 3 -> (256, 512] (two, the second ragged), 2 -> above 512 (three).  The item kernels (k_matvec_pairs,
k_cost_items, k_coarse_edges) walk the work items compileTable cuts from the pairs: on a device with more workgroup slots than
these videos have items, that is chunks of at most 128 constraints per direction (tests/product_cases.expected_items), one
partial trip whatever the spacing.  The three items_* cases are there for them: the 110-frame list of tests/product_cases.py
keeps its items whole, up to 768 constraints per direction.

States follow random_state of tests/test_oracle_problem.py (poses N(0, 0.05) with frame 0's rotation zero, focal 0.2 + U(0, 0.05),
depth parameters 0.15 + U(0, 0.05), shifts U(0, 0.3), spatial parameters N(0, 0.01)); about 10 % of the constraints are dynamic
and the depth pixels at [::7, ::5] are zero, as in tests/golden/make_golden.py.  Seeds count up from 61, but for four cases in which
the spatial parameters move the cost by less than the 1e-3 that tests/test_generic_cases.py asks for at most seeds.  Each of these
has the first seed of a progression that meets it: cubic4x4ss_vertical_euclid_fixed 315 of 65, 90, 115, ... (3 of 40 seeds do,
the median moves the cost by 1.5e-4: four parameters of N(0, 0.01) against a residual in scene units), trip_cubic4x4_bilinear
91 of 71, 81, 91, ... (2 of 5), and on the 110-frame list, where the warps of many frames largely cancel in the sum,
items_grid4x3_corners 145 of 75, 85, ... (2 of 10) and items_cubic3x2_bicubic 106 of 76, 86, ... (1 of 10).
tests/test_generic_cases.py holds every case to its conditions with the oracle alone; nothing here builds a Solver.
"""
import collections
import dataclasses
import functools

import numpy as np

from robust_cvd_amd import synth
from robust_cvd_amd.ctypes_types import (DepthXformType, IntrinsicsOptimization, OptParams, SmoothLossType, SpatialXformType,
                                         ValueXformType, XformDesc)
from tests import product_cases
from tests.test_oracle_problem import random_state

CAUCHY, HUBER = 0, 1
_SS = ValueXformType.ScaleShift
_BICUBIC = lambda: XformDesc.spatial(SpatialXformType.BicubicGrid, 4, 3)
_BILINEAR = lambda: XformDesc.spatial(SpatialXformType.BilinearGrid, 3, 2)
_VERTICAL = lambda: XformDesc.spatial(SpatialXformType.VerticalLinear)
_CORNERS = lambda: XformDesc.spatial(SpatialXformType.CornersBilinear)
_IDENTITY = XformDesc.spatial

# smooth: (smooth loss type, static weight, dynamic weight) of a triplet case, else None
Case = collections.namedtuple("Case", "id kd ks depth spatial intr loss robust spacing frames width height seed block smooth")

CASES = [
    Case("global_bicubic", 1, 16, XformDesc.global_depth, _BICUBIC, 2, 1, CAUCHY, 3, 4, 64, 40, 61, 7 + 1 + 24, None),
    Case("globalss_bicubic_log_huber", 1, 16, lambda: XformDesc.global_depth(_SS), _BICUBIC, 2, 3, HUBER, 9, 4, 64, 40, 62,
         7 + 2 + 24, None),
    Case("grid4x3_bicubic_ratio", 4, 16, lambda: XformDesc.grid_depth(4, 3), _BICUBIC, 2, 2, CAUCHY, 2, 4, 64, 40, 63,
         7 + 12 + 24, None),
    Case("cubic4x4_bilinear_shared_huber", 16, 4, lambda: XformDesc.grid_depth(4, 4, cubic=True), _BILINEAR, 1, 1, HUBER, 3, 4, 64,
         40, 64, 7 + 16 + 12, None),
    Case("cubic4x4ss_vertical_euclid_fixed", 16, 4, lambda: XformDesc.grid_depth(4, 4, _SS, cubic=True), _VERTICAL, 0, 0, CAUCHY,
         9, 4, 64, 40, 315, 7 + 32 + 4, None),
    Case("cubic5x4_corners_log", 16, 4, lambda: XformDesc.grid_depth(5, 4, cubic=True), _CORNERS, 2, 3, CAUCHY, 9, 4, 64, 40, 66,
         7 + 20 + 8, None),
    Case("grid4x3_corners_shared", 4, 4, lambda: XformDesc.grid_depth(4, 3), _CORNERS, 1, 1, CAUCHY, 2, 4, 64, 40, 67, 7 + 12 + 8,
         None),
    Case("cubic5x4ss_bicubic_trips", 16, 16, lambda: XformDesc.grid_depth(5, 4, _SS, cubic=True), _BICUBIC, 2, 1, CAUCHY, 2, 4, 64,
         40, 68, 7 + 40 + 24, None),
    # (1,4) beyond one trip: the golden vectors hold it at about 40 constraints per pair
    Case("global_bilinear_trips", 1, 4, XformDesc.global_depth, _BILINEAR, 2, 1, CAUCHY, 3, 4, 64, 40, 73, 7 + 1 + 12, None),
    # B = 201 > 199: the packed triangle of a frame block no longer fits one row panel of k_assemble
    Case("panels_17x10_bicubic", 4, 16, lambda: XformDesc.grid_depth(17, 10), _BICUBIC, 2, 1, CAUCHY, 9, 3, 96, 56, 69,
         7 + 170 + 24, None),
    Case("trip_grid4x3_bicubic", 4, 16, lambda: XformDesc.grid_depth(4, 3), _BICUBIC, 2, 1, CAUCHY, 9, 6, 64, 40, 70, 7 + 12 + 24,
         (SmoothLossType.ReproDisparityLaplacian, 2.0, 0.5)),
    Case("trip_cubic4x4_bilinear", 16, 4, lambda: XformDesc.grid_depth(4, 4, cubic=True), _BILINEAR, 2, 1, CAUCHY, 9, 6, 64, 40, 91,
         7 + 16 + 12, (SmoothLossType.EuclideanLaplacian, 1.5, 1.0)),
    # The item kernels at several trips: the 110-frame list of tests/product_cases.py (spacing None), whose 848 work items stay uncut on
    # a 256-CU device -- items of 768 + 1, 385 + 6, about 500 + 500, about 500 + 0 and 3 + about 500 constraints among hundreds of
    # 3 to 40 -- for the three instantiations the golden vectors hold at one partial trip
    Case("items_global_vertical", 1, 4, XformDesc.global_depth, _VERTICAL, 2, 1, CAUCHY, None, 110, 64, 40, 74, 7 + 1 + 4, None),
    Case("items_grid4x3_corners", 4, 4, lambda: XformDesc.grid_depth(4, 3), _CORNERS, 2, 1, CAUCHY, None, 110, 64, 40, 145, 7 + 12 + 8,
         None),
    Case("items_cubic3x2_bicubic", 16, 16, lambda: XformDesc.grid_depth(3, 2, cubic=True), _BICUBIC, 2, 1, CAUCHY, None, 110, 64, 40,
         106, 7 + 6 + 24, None),
    # control: identity spatial transform at three trips, sent to the generic kernels by set_generic_kernels -- a failure of the
    # cases above that this one does not share lies in the spatial taps, not in the generic walk
    Case("control_grid4x3_identity", 4, 0, lambda: XformDesc.grid_depth(4, 3), _IDENTITY, 2, 1, CAUCHY, 2, 4, 64, 40, 72, 7 + 12,
         None),
]
IDS = [c.id for c in CASES]
SPATIAL_IDS = [c.id for c in CASES if c.ks]
ITEMS_IDS = [c.id for c in CASES if c.spacing is None]
COARSE_IDS = ["global_bicubic", "grid4x3_bicubic_ratio", "cubic4x4ss_vertical_euclid_fixed", "cubic5x4_corners_log",
              "items_grid4x3_corners"]
LM_IDS = ["global_bicubic", "grid4x3_bicubic_ratio", "cubic4x4_bilinear_shared_huber"]
# constraints of a directed pair, by spacing: (more than, at most); 768 = three trips of 256 threads
WINDOWS = {9: (0, 256), 3: (256, 512), 2: (512, 768)}


def case(cid):
    return next(c for c in CASES if c.id == cid)


def tap_counts(dd, sd):
    """tapCounts of cvd_setup.hip, from the two descriptors."""
    kd = 1
    if dd.depth_type == DepthXformType.Grid:
        kd = 16 if dd.cubic_interpolation else 4
        if dd.grid_size[2] > 1:
            kd = 16 if dd.grid_size[0] > 1 else 4
    ks = {SpatialXformType.Identity: 0, SpatialXformType.BicubicGrid: 16}.get(sd.spatial_type, 4)
    return kd, ks


def params(c, smooth=True):
    p = OptParams.defaults()
    p.num_threads = 2 if c.spacing is not None else 8
    p.intr_opt = c.intr
    p.static_loss_type = c.loss
    if c.smooth is not None and smooth:
        p.smooth_loss_type, p.smooth_static_weight, p.smooth_dynamic_weight = c.smooth
    return p


@functools.lru_cache(maxsize=None)
def problem(cid):
    """(video, triplets or None, state) of a case; state = (pose [F, 7], depth parameters, spatial parameters).  The video carries the
    zeroed depth pixels and the dynamic flags.  Shared, never modified."""
    from oracle.oracle import Oracle
    c = case(cid)
    if c.spacing is None:
        v = product_cases.make_case("items850")
        assert (v.num_frames, v.width, v.height) == (c.frames, c.width, c.height)
    else:
        v = synth.make_video(c.frames, c.width, c.height, seed=c.seed, spacing=c.spacing)
    rng = np.random.default_rng(c.seed)
    o = Oracle()
    synth.load_into(o, v)
    o.reset_depth_xforms(c.depth())
    o.reset_spatial_xforms(c.spatial())
    state = random_state(o, c.frames, c.depth(), rng)
    is_static = (rng.uniform(size=v.num_constraints) > 0.1).astype(np.uint8)
    depth = v.depth.copy()
    depth[:, ::7, ::5] = 0.0
    v = dataclasses.replace(v, depth=depth, is_static=is_static)
    trip = synth.make_triplets(v, spacing=9.0, seed=c.seed + 100) if c.smooth is not None else None
    for a in (depth, is_static) + tuple(state):
        a.setflags(write=False)
    return v, trip, state


def load(ctor, cid):
    """A Solver or an Oracle with the case's video, constraints, transforms and robustifier (the parameters still at their reset)."""
    c = case(cid)
    v, trip, _ = problem(cid)
    s = ctor()
    synth.load_into(s, v)
    if trip is not None:
        s.set_triplet_constraints(*trip)
    s.reset_depth_xforms(c.depth())
    s.reset_spatial_xforms(c.spatial())
    s.set_robust_loss(c.robust)
    return s


def put(s, state):
    pose, dx, sx = state
    if dx.size:
        s.set_xform_params(dx)
    if sx.size:
        s.set_xform_params(sx, True)
    return pose


def static_constraints_with_valid_depth(v):
    """Static constraints whose two depth fetches are positive: the truncating fetch of the constraint table, restated."""
    inv = np.float32(v.inv_aspect)
    W, H = np.float32(v.width), np.float32(v.height)
    n = 0
    for p, (fa, fb) in enumerate(v.pairs):
        l = v.loc[v.offsets[p]:v.offsets[p + 1]]
        da = v.depth[fa][(l[:, 1] / inv * H).astype(int), (l[:, 0] * W).astype(int)]
        db = v.depth[fb][(l[:, 3] / inv * H).astype(int), (l[:, 2] * W).astype(int)]
        n += int(((da > 0) & (db > 0) & (v.is_static[v.offsets[p]:v.offsets[p + 1]] != 0)).sum())
    return n


def triplets_with_valid_depth(v, trip):
    centers, off, loc6, _ = trip
    inv = np.float32(v.inv_aspect)
    W, H = np.float32(v.width), np.float32(v.height)
    n = 0
    for k, ce in enumerate(centers):
        l = loc6[off[k]:off[k + 1]]
        ok = np.ones(len(l), bool)
        for side, f in ((0, ce - 1), (2, ce), (4, ce + 1)):
            ok &= v.depth[f][(l[:, side + 1] / inv * H).astype(int), (l[:, side] * W).astype(int)] > 0
        n += int(ok.sum())
    return n


def regulariser_blocks(c, p):
    """Residual blocks of the regularisers at default weights: per frame the depth grid's deformation cost, the spatial
    transform's, scale_reg_grid_size x round(scale_reg_grid_size / aspect) scale samples and, unless the intrinsics are fixed, the
    focal prior."""
    per_frame = int(c.depth().depth_type == DepthXformType.Grid) + int(c.ks != 0)
    per_frame += p.scale_reg_grid_size * int(round(np.float32(p.scale_reg_grid_size) * (np.float32(c.height) / np.float32(c.width))))
    per_frame += int(c.intr != IntrinsicsOptimization.Fixed)
    return c.frames * per_frame


def num_depth_params(c):
    """(value parameters per vertex, vertices) of the depth transform."""
    d = c.depth()
    n = 2 if d.value_xform == _SS else 1
    return n, (d.grid_size[0] * d.grid_size[1] if d.depth_type == DepthXformType.Grid else 1)


def coarse_basis(c):
    """Z [F B, 8 F] of the pose-graph level (cvd_coarse.h): per frame the seven pose unknowns and one mode that moves every depth
    SCALE of the frame together -- rows 7 + v N of the N value parameters of vertex v (k_coarse_diag: cidx = 7 + v * N;
    k_coarse_edges: JD x source depth, the scale's derivative).  Shifts (rows 7 + v N + 1) and spatial parameters are in no mode."""
    n, vertices = num_depth_params(c)
    F, B = c.frames, c.block
    Z = np.zeros((F * B, 8 * F))
    for f in range(F):
        Z[f * B:f * B + 7, f * 8:f * 8 + 7] = np.eye(7)
        Z[f * B + 7 + n * np.arange(vertices), f * 8 + 7] = 1.0
    return Z


def dense_lm_step(H, g):
    """The first LM step from (J^T J, gradient) by a dense solve: Ceres' column scaling 1 / (1 + sqrt(H_ii)), damping
    clamp(H_ii scale^2, 1e-6, 1e32) / radius at the initial radius 1e4 (tests/test_gpu_product_shapes.py)."""
    hd = np.diag(H)
    sc = 1.0 / (1.0 + np.sqrt(hd))
    lam = np.clip(hd * sc * sc, 1e-6, 1e32) / 1e4 / (sc * sc)
    return np.linalg.solve(H + np.diag(lam), -g.reshape(-1))


def one_lm_iteration(s, c, state):
    """One LM iteration of `s` from `state`: (step [F, B], accepted, summary)."""
    p = params(c)
    p.max_iterations = 1
    s.set_pose_params(put(s, state))
    s.pose_optimization_step(p, 0.1, convert_poses=False)
    after = np.concatenate([s.get_pose_params(), s.get_xform_params(), s.get_xform_params(True)], axis=1)
    sm = s.summary()
    return after - np.concatenate(state, axis=1), sm["num_successful_steps"] > 0, sm


@functools.lru_cache(maxsize=None)
def lm_state(cid):
    """The state of the one-LM-step comparison, chosen by the oracle alone: the raw draw where the oracle accepts the first
    iteration from it, else the draw advanced by the oracle's first 8 LM iterations and read back in f64, as
    tests/test_gpu_product_shapes.test_one_lm_step_matches_the_exact_step does; where a fresh iteration from there (the trust
    radius back at its start) is rejected too, by its first 9, 10, ... up to 16.  Returns (state, iterations advanced):
    grid4x3_bicubic_ratio 0, global_bicubic 8, cubic4x4_bilinear_shared_huber 10 (rejected after 8 and after 9)."""
    from oracle.oracle import Oracle
    c = case(cid)
    _, _, raw = problem(cid)
    o = load(Oracle, cid)
    _, accepted, _ = one_lm_iteration(o, c, raw)
    if accepted:
        return raw, 0
    for n in range(8, 17):
        p = params(c)
        p.max_iterations = n
        o.set_pose_params(put(o, raw))
        o.pose_optimization_step(p, 0.1, convert_poses=False)
        state = (o.get_pose_params(), o.get_xform_params(), o.get_xform_params(True))
        _, accepted, _ = one_lm_iteration(o, c, state)
        if accepted:
            for a in state:
                a.setflags(write=False)
            return state, n
    raise AssertionError(f"{cid}: the oracle accepts no fresh LM iteration after 8 .. 16 of its own")
