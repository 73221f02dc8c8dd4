"""Seeded states that put flow constraints on the clamped and behind-camera branches of the constraint model.

Every GPU parity test draws its state like tests/test_gpu_huber._state: poses N(0, 0.05), depth parameters in 0.15 .. 0.20,
shifts >= 0.  There z' (the depth of the source point in the target camera) and D_b (the target's transformed depth) are
positive for every constraint, so max(z', 1e-6), max(D_b, 1e-6) never clamp and the ratio / log-ratio residuals never see a
negative argument.  The LM driver does evaluate such points (a rejected first step lands there), so the states below plant
them, on two small videos (`video(4)`, `video(5)`: 4 and 5 frames of 64 x 40):

  behind             frame 2 moved forward along its optical axis past part of the scene: constraints INTO frame 2 get z' < eps (Z)
  negative_depth     frame 1's depth made negative (ScaleShift: a negative shift on every vertex; Scale: every vertex's value times
                     -0.04, the draw's jitter of the values kept) AND frame 1 moved forward: constraints into frame 1 have
                     D_b < eps, with z' >= eps (B) or z' < eps (ZB)
  both_negative_log  Global ScaleShift: a large negative shift on frame 1 and frame 1 far forward: every constraint into frame 1
                     has z' < 0 and D_b < 0, no constraint anywhere has mixed signs -- the finite log-ratio state
  mixed_sign_log     `behind` under the log-ratio loss: z' < 0 < D_b, log of a negative number, the oracle's cost is NaN
  lm_candidate       the raw draw plus the damped Gauss-Newton step at the initial trust radius (the point the driver asks about
                     first), from the oracle's J^T J and gradient by the dense solve of
                     tests/test_gpu_product_shapes.test_one_lm_step_matches_the_exact_step

`forward` is a numpy restatement of z', D_a and D_b per constraint (closed form for Global, the bilinear / bicubic weights of
tests/test_oracle_kat for grids, the bilinear spatial warp included); `classify` sorts the constraints into R (regular), Z, B, ZB
and drops what sits too close to a threshold.  tests/test_branch_cases.py holds all of it to the oracle on the CPU.
"""
import functools
import types

import numpy as np

from robust_cvd_amd import synth
from robust_cvd_amd.ctypes_types import (IntrinsicsOptimization, OptParams, SpatialXformType, StaticLossType, ValueXformType,
                                         XformDesc)
from tests.test_gpu_huber import _state
from tests.test_oracle_kat import ref_bicubic, ref_bilinear
from tests.test_oracle_problem import rodrigues

EPS = 1e-6          # the model's clamp
NEAR = 1e-3         # a constraint this close to a threshold is dropped from the lists
SMALL_Z = 1e-2      # |z'| below this: u = q_x / z' swamps everything else, dropped
CAUCHY, HUBER = 0, 1
POPULATIONS = ("R", "Z", "B", "ZB")

# depth transform name -> (constructor, spatial transform constructor)
DEPTHS = {
    "global": (XformDesc.global_depth, XformDesc.spatial),
    "global_scaleshift": (lambda: XformDesc.global_depth(ValueXformType.ScaleShift), XformDesc.spatial),
    "grid5x4": (lambda: XformDesc.grid_depth(5, 4), XformDesc.spatial),
    "grid4x3": (lambda: XformDesc.grid_depth(4, 3), XformDesc.spatial),
    "cubic4x4": (lambda: XformDesc.grid_depth(4, 4, cubic=True), XformDesc.spatial),
    "grid3x2": (lambda: XformDesc.grid_depth(3, 2), XformDesc.spatial),
    "grid6x4": (lambda: XformDesc.grid_depth(6, 4), XformDesc.spatial),
    "cubic4x3_scaleshift_spatial": (lambda: XformDesc.grid_depth(4, 3, ValueXformType.ScaleShift, cubic=True),
                                    lambda: XformDesc.spatial(SpatialXformType.BilinearGrid, 3, 2)),
}
# name -> (grid x, grid y, cubic, value parameters per vertex, spatial grid or None): what `forward` needs, stated apart from XformDesc
SHAPES = {
    "global": (1, 1, False, 1, None),
    "global_scaleshift": (1, 1, False, 2, None),
    "grid5x4": (5, 4, False, 1, None),
    "grid4x3": (4, 3, False, 1, None),
    "cubic4x4": (4, 4, True, 1, None),
    "grid3x2": (3, 2, False, 1, None),
    "grid6x4": (6, 4, False, 1, None),
    "cubic4x3_scaleshift_spatial": (4, 3, True, 2, (3, 2)),
}


@functools.lru_cache(maxsize=None)
def video(frames):
    """The two videos of the issue: 4 frames (seed 41) and 5 frames (seed 43) of 64 x 40.  Shared, never modified."""
    return synth.make_video(frames, 64, 40, seed={4: 41, 5: 43}[frames], spacing=9)


def params(loss=StaticLossType.ReproDisparity, scale_reg=0.0, intr=IntrinsicsOptimization.PerFrame):
    """OptParams of an evaluation.  scale_reg = 0 wherever D < eps occurs: the regulariser's own clamp (1 / 1e-6 squared) would
    bury the constraints; None keeps the default."""
    p = OptParams.defaults()
    p.num_threads = 2
    p.static_loss_type = loss
    p.intr_opt = intr
    if scale_reg is not None:
        p.scale_reg = scale_reg
    return p


def load(ctor, v, depth, robust=CAUCHY, subset=None, all_dynamic=False):
    """A Solver or an Oracle with the video, the transforms of `depth` and the robustifier set; `subset` (indices into the
    constraint list) keeps those constraints only, pair by pair."""
    s = ctor()
    synth.load_into(s, v)
    if subset is not None or all_dynamic:
        pairs, offsets, loc = (v.pairs, v.offsets, v.loc) if subset is None else sublist(v, subset)
        flags = np.zeros(loc.shape[0], np.uint8) if all_dynamic else np.ones(loc.shape[0], np.uint8)
        s.set_pair_constraints(pairs, offsets, loc, flags)
    dd, sd = DEPTHS[depth]
    s.reset_depth_xforms(dd())
    s.reset_spatial_xforms(sd())
    s.set_robust_loss(robust)
    return s


def sublist(v, keep):
    """(pairs, offsets, loc) of the constraints `keep` (sorted indices) of v's list; a pair that keeps none leaves the list."""
    keep = np.asarray(keep, np.int64)
    assert (np.diff(keep) > 0).all()
    counts = np.array([int(((keep >= v.offsets[k]) & (keep < v.offsets[k + 1])).sum()) for k in range(len(v.pairs))])
    some = counts > 0
    return v.pairs[some], np.concatenate([[0], np.cumsum(counts[some])]).astype(np.int64), v.loc[keep]


def put(s, state):
    pose, dx, sx = state
    if dx.size:
        s.set_xform_params(dx)
    if sx.size:
        s.set_xform_params(sx, True)
    return pose


# ----------------------------------------------------------------------------------------------------------------------------
# the forward quantities, in numpy
# ----------------------------------------------------------------------------------------------------------------------------
def _taps(gx, gy, cubic, lx, ly):
    if gx == 1 and gy == 1:
        return [0], [1.0]
    return ref_bicubic(lx, ly, gx, gy) if cubic else ref_bilinear(lx, ly, gx, gy)


def forward(v, depth, state, shared_intrinsics=False, dtype=np.float64):
    """z' [C], D_a [C], D_b [C] of every constraint of v's list at `state` = (pose [F, 7], depth parameters, spatial
    parameters): D = sum_k w_k (d theta_k0 + theta_k1), X = t_a + D_a R_a (x_a f_a A, y_a f_a, -1), z' = -(R_b^T (X - t_b))_z,
    with (x, y) the stored float NDC plus the spatial warp."""
    gx, gy, cubic, nv, sgrid = SHAPES[depth]
    pose, dx, sx = state
    W, H = v.width, v.height
    A = dtype(np.float32(v.aspect))
    inv = np.float32(v.inv_aspect)
    R = [rodrigues(pose[f, 3:6]).astype(dtype) for f in range(v.num_frames)]
    z, Da, Db = (np.zeros(v.num_constraints, dtype) for _ in range(3))
    for p, (fa, fb) in enumerate(v.pairs):
        for c in range(v.offsets[p], v.offsets[p + 1]):
            l = v.loc[c]
            side = []
            for f, x, y in ((fa, l[0], l[1]), (fb, l[2], l[3])):
                n = (np.float32(-1) + np.float32(2) * x, np.float32(1) - np.float32(2) * y / inv)
                d = dtype(v.depth[f][int(y / inv * np.float32(H)), int(x * np.float32(W))])
                idx, w = _taps(gx, gy, cubic, n[0], n[1])
                D = dtype(0)
                for i, wi in zip(idx, w):
                    D += dtype(wi) * (d * dtype(dx[f, i * nv]) + (dtype(dx[f, i * nv + 1]) if nv == 2 else dtype(0)))
                nx, ny = dtype(n[0]), dtype(n[1])
                if sgrid is not None:
                    sidx, sw = ref_bilinear(n[0], n[1], *sgrid)
                    for i, wi in zip(sidx, sw):
                        nx += dtype(wi) * dtype(sx[f, 2 * i])
                        ny += dtype(wi) * dtype(sx[f, 2 * i + 1])
                side.append((nx, ny, D))
            fya = dtype(pose[0 if shared_intrinsics else fa, 6])
            nx, ny, D = side[0]
            X = pose[fa, :3].astype(dtype) + D * (R[fa] @ np.array([nx * fya * A, ny * fya, -1.0], dtype))
            q = R[fb].T @ (X - pose[fb, :3].astype(dtype))
            z[c], Da[c], Db[c] = -q[2], D, side[1][2]
    return z, Da, Db


def classify(z, Db):
    """{"R" | "Z" | "B" | "ZB": sorted constraint indices} and the dropped indices: within NEAR of a threshold, or |z'| < SMALL_Z."""
    drop = (np.abs(z - EPS) < NEAR) | (np.abs(Db - EPS) < NEAR) | (np.abs(z) < SMALL_Z)
    zc, bc = z < EPS, Db < EPS
    pops = {"R": ~zc & ~bc, "Z": zc & ~bc, "B": ~zc & bc, "ZB": zc & bc}
    return {k: np.flatnonzero(m & ~drop) for k, m in pops.items()}, np.flatnonzero(drop)


# ----------------------------------------------------------------------------------------------------------------------------
# the states
# ----------------------------------------------------------------------------------------------------------------------------
def raw_state(v, depth):
    """The draw every GPU parity test uses (tests/test_gpu_huber._state, seed 17), for this depth transform."""
    from oracle.oracle import Oracle
    return _state(load(Oracle, v, depth), v.num_frames, np.random.default_rng(17))


def _forward_axis(pose, f):
    return rodrigues(pose[f, 3:6]) @ np.array([0.0, 0.0, -1.0])


def _push(v, depth, state, frame, quantile):
    """`frame` moved forward along its optical axis by that quantile of the z' of the constraints INTO it."""
    z, _, _ = forward(v, depth, state)
    into = np.concatenate([np.arange(v.offsets[k], v.offsets[k + 1]) for k, (_, b) in enumerate(v.pairs) if b == frame])
    pose = state[0].copy()
    pose[frame, :3] += np.quantile(z[into], quantile) * _forward_axis(pose, frame)
    return pose, state[1], state[2]


@functools.lru_cache(maxsize=None)
def behind(depth, frames=4):
    v = video(frames)
    return _push(v, depth, raw_state(v, depth), 2, 0.5)


@functools.lru_cache(maxsize=None)
def negative_depth(depth, frames=4):
    """Frame 1's depth negative everywhere, and frame 1 forward by the median z' of what projects into it (B and ZB)."""
    v = video(frames)
    pose, dx, sx = raw_state(v, depth)
    dx = dx.copy()
    nv = SHAPES[depth][3]
    if nv == 2:
        # D = d scale + shift with shift = -median(d) scale on every vertex: negative below the median only, so the shift is
        # taken at twice the largest raw depth -- D < 0 on the whole frame
        dx[1, 1::2] = -2.0 * float(v.depth[1].max()) * dx[1, 0::2]
    else:
        dx[1] = -0.04 * dx[1]   # |D_b| of the size of the |z'| just behind the camera: both sides of z' < D_b among ZB
    return _push(v, depth, (pose, dx, sx), 1, 0.5)


@functools.lru_cache(maxsize=None)
def both_negative_log(frames=4):
    """Global ScaleShift: D_1 = (d - 1.15 max d) scale < 0 and frame 1 forward by 1.15 max d scale, more than any z' into it:
    z' < 0 and D_b < 0 for every constraint into frame 1, of like size (both sides of z' < D_b); what leaves frame 1 starts
    |D_a| behind it, about d scale in front of where frame 1 stood, so in front of the other cameras."""
    v = video(frames)
    depth = "global_scaleshift"
    pose, dx, sx = raw_state(v, depth)
    dx = dx.copy()
    shift = 1.15 * float(v.depth[1].max()) * dx[1, 0]
    dx[1, 1] = -shift
    z, _, Db = forward(v, depth, (pose, dx, sx))
    into = np.concatenate([np.arange(v.offsets[k], v.offsets[k + 1]) for k, (_, b) in enumerate(v.pairs) if b == 1])
    pose = pose.copy()
    pose[1, :3] += float(np.median(z[into] - Db[into])) * _forward_axis(pose, 1)   # (median z' = median D_b afterwards)
    return pose, dx, sx


def mixed_sign_log(frames=4):
    return behind("global_scaleshift", frames)


def gauss_newton_step(H, g):
    """The first LM step of the driver: Ceres' column scaling 1 / (1 + sqrt(H_ii)), damping clamp(H_ii scale^2, 1e-6, 1e32) /
    radius at the initial radius 1e4 (tests/test_gpu_product_shapes.test_one_lm_step_matches_the_exact_step)."""
    hd = np.diag(H)
    sc = 1.0 / (1.0 + np.sqrt(hd))
    lam = np.clip(hd * sc * sc, 1e-6, 1e32) / 1e4 / (sc * sc)
    return np.linalg.solve(H + np.diag(lam), -g.reshape(-1))


@functools.lru_cache(maxsize=None)
def lm_candidate(depth, loss=StaticLossType.ReproDisparity, robust=CAUCHY, frames=5):
    """The raw draw plus its damped Gauss-Newton step, default parameters (the driver's), oracle J^T J and gradient."""
    from oracle.oracle import Oracle
    v = video(frames)
    state = raw_state(v, depth)
    o = load(Oracle, v, depth, robust)
    pose = put(o, state)
    ev = o.evaluate(params(loss, scale_reg=None), 0.1, pose, want_hfull=True)
    step = gauss_newton_step(ev["hfull"], ev["gradient"]).reshape(v.num_frames, -1)
    nd = state[1].shape[1]
    return pose + step[:, :7], state[1] + step[:, 7:7 + nd], state[2] + step[:, 7 + nd:]


def populations(v, depth, state, shared_intrinsics=False):
    z, _, Db = forward(v, depth, state, shared_intrinsics)
    pops, dropped = classify(z, Db)
    return pops, dropped, z, Db


def lists(v, depth, state, shared_intrinsics=False, at_least=1):
    """The constraint lists of a case: "all" (everything that is not dropped) and each population with at least `at_least`
    constraints on its own, so that a branch's contribution cannot hide behind the bulk."""
    pops, _, _, _ = populations(v, depth, state, shared_intrinsics)
    out = {"all": np.sort(np.concatenate(list(pops.values())))}
    out.update({k: idx for k, idx in pops.items() if len(idx) >= at_least})
    return out


# ----------------------------------------------------------------------------------------------------------------------------
# the variants of tests/test_gpu_model_branches.py and their states
# ----------------------------------------------------------------------------------------------------------------------------
_ABE = ("behind", "negative_depth", "lm_candidate")
_AB = ("behind", "negative_depth")
_PF, _SH = IntrinsicsOptimization.PerFrame, IntrinsicsOptimization.Shared
# (id, depth transform, static loss, robustifier, intrinsics, taps KD, SPEC of the fast kernels or None = outside the fast scope, states)
VARIANTS = [
    ("global-disparity-cauchy", "global", StaticLossType.ReproDisparity, CAUCHY, _PF, 1, 1, _ABE),
    ("grid5x4-disparity-huber", "grid5x4", StaticLossType.ReproDisparity, HUBER, _PF, 4, 2, _ABE),
    ("cubic4x4-disparity-cauchy", "cubic4x4", StaticLossType.ReproDisparity, CAUCHY, _PF, 16, 1, _ABE),
    ("grid5x4-ratio-cauchy", "grid5x4", StaticLossType.ReproDepthRatio, CAUCHY, _PF, 4, 0, _ABE),
    ("global_scaleshift-logdepth-cauchy", "global_scaleshift", StaticLossType.ReproLogDepth, CAUCHY, _PF, 1, 0, ("both_negative_log",)),
    ("grid4x3-disparity-shared", "grid4x3", StaticLossType.ReproDisparity, CAUCHY, _SH, 4, 0, _AB),
    ("generic-cubic4x3_scaleshift-spatial", "cubic4x3_scaleshift_spatial", StaticLossType.ReproDisparity, CAUCHY, _PF, 16, None, _AB),
    ("generic-euclidean", "global", StaticLossType.Euclidean, CAUCHY, _PF, 1, None, _AB),
]
CASES = [(v[0], st) for v in VARIANTS for st in v[7]]


def variant(vid):
    return next(v for v in VARIANTS if v[0] == vid)


def case(vid, state_name):
    """(video, state) of a variant at one of its states."""
    _, depth, loss, robust, _, _, _, _ = variant(vid)
    if state_name == "behind":
        return video(4), behind(depth)
    if state_name == "negative_depth":
        return video(4), negative_depth(depth)
    if state_name == "both_negative_log":
        return video(4), both_negative_log()
    if state_name == "mixed_sign_log":
        return video(4), mixed_sign_log()
    assert state_name == "lm_candidate"
    return video(5), lm_candidate(depth, loss, robust)


# ----------------------------------------------------------------------------------------------------------------------------
# state `behind` for the triplet loss and for the dense mode (the cases of tests/test_gpu_triplets.py, tests/test_gpu_dense_mode.py)
# ----------------------------------------------------------------------------------------------------------------------------
def _as_list(v, pairs, offsets, loc):
    """v's frames with another constraint list: what `forward` reads."""
    return types.SimpleNamespace(num_frames=v.num_frames, width=v.width, height=v.height, aspect=v.aspect, inv_aspect=v.inv_aspect,
                                 depth=v.depth, pairs=np.asarray(pairs), offsets=np.asarray(offsets, np.int64), loc=loc,
                                 num_constraints=int(offsets[-1]))


def _perturbed_state(v, depth, pose_sigma, pose_seed):
    """The state of the triplet / dense tests: poses N(0, sigma), focal 0.2 + U(0, 0.02), reset depth parameters times 1 + 0.05 N."""
    from oracle.oracle import Oracle
    F = v.num_frames
    rng = np.random.default_rng(pose_seed)
    pose = np.zeros((F, 7))
    pose[:, :6] = rng.normal(0, pose_sigma, (F, 6))
    pose[:, 6] = 0.2 + rng.uniform(0, 0.02, F)
    o = load(Oracle, v, depth)
    th = o.get_xform_params()
    return pose, th * (1.0 + 0.05 * np.random.default_rng(9).standard_normal(th.shape)), o.get_xform_params(True)


@functools.lru_cache(maxsize=None)
def triplet_case():
    """The grid3x2 case of tests/test_gpu_triplets.py (6 frames of 96 x 56, seed 5) with frames 2 and 4 moved forward by the
    median depth of the outer points of the triplets centred on them: about half of those project behind the centre camera.
    Returns (video, state, triplets, outer z [n, 2], other depth [n]) with the triplets kept: no outer z within NEAR of eps or
    with |z| < SMALL_Z, and |c01.z + c21.z - D_c| >= SMALL_Z (the ratio consistency loss divides by it)."""
    depth = "grid3x2"
    v = synth.make_video(6, 96, 56, seed=5)
    ce, off, loc6, st = synth.make_triplets(v, spacing=20.0)
    pairs, poff, locs = [], [0], []
    for k, c in enumerate(ce):                       # per group: c-1 -> c, then c+1 -> c
        for side, o in ((0, c - 1), (4, c + 1)):
            pairs.append((o, c))
            locs.append(np.concatenate([loc6[off[k]:off[k + 1], side:side + 2], loc6[off[k]:off[k + 1], 2:4]], axis=1))
            poff.append(poff[-1] + int(off[k + 1] - off[k]))
    lv = _as_list(v, pairs, poff, np.concatenate(locs, axis=0))

    def outer(state):
        z, _, Db = forward(lv, depth, state)
        zo, dc = np.zeros((len(loc6), 2)), np.zeros(len(loc6))
        for k in range(len(ce)):
            n = int(off[k + 1] - off[k])
            zo[off[k]:off[k + 1], 0] = z[poff[2 * k]:poff[2 * k] + n]
            zo[off[k]:off[k + 1], 1] = z[poff[2 * k + 1]:poff[2 * k + 1] + n]
            dc[off[k]:off[k + 1]] = Db[poff[2 * k]:poff[2 * k] + n]
        return zo, dc

    state = _perturbed_state(v, depth, 0.03, 3)
    zo, _ = outer(state)
    pose = state[0].copy()
    for c in (2, 4):
        k = int(np.flatnonzero(ce == c)[0])
        pose[c, :3] += float(np.median(zo[off[k]:off[k + 1]])) * _forward_axis(pose, c)
    state = (pose, state[1], state[2])
    zo, dc = outer(state)
    other = zo.sum(axis=1) - dc
    keep = ~((np.abs(zo - EPS) < NEAR).any(axis=1) | (np.abs(zo) < SMALL_Z).any(axis=1) | (np.abs(other) < SMALL_Z))
    counts = np.array([int(keep[off[k]:off[k + 1]].sum()) for k in range(len(ce))])
    trip = (ce, np.concatenate([[0], np.cumsum(counts)]).astype(np.int64), loc6[keep], st[keep])
    return v, state, trip, zo[keep], other[keep]


@functools.lru_cache(maxsize=None)
def dense_case(depth):
    """Dense mode on the smallest raster of tests/test_gpu_dense_mode.py (6 frames of 20 x 12, seed 67) at state `behind`: frame 2
    moved forward by the median z' of the pixels that project into it.  Pixels that `classify` drops are masked out (the dense
    kernels read the images, there is no list to drop them from).  Returns (video, state, flow, mask, offsets, loc, z')."""
    v = synth.make_video(6, 20, 12, seed=67)
    flow, mask = synth.make_dense_flows(v)
    mask = mask.copy()
    state = _perturbed_state(v, depth, 0.02, 3)
    off, loc = synth.dense_constraints_from_flows(v, flow, mask)
    state = _push(_as_list(v, v.pairs, off, loc), depth, state, 2, 0.5)
    lv = _as_list(v, v.pairs, off, loc)
    z, _, Db = forward(lv, depth, state)
    _, dropped = classify(z, Db)
    px = np.rint(loc[:, 0] * np.float32(v.width)).astype(int)
    py = np.rint(loc[:, 1] / np.float32(v.inv_aspect) * np.float32(v.height)).astype(int)
    pair_of = np.repeat(np.arange(len(v.pairs)), np.diff(off))
    assert (mask[pair_of, py, px] != 0).all()
    mask[pair_of[dropped], py[dropped], px[dropped]] = 0
    off, loc = synth.dense_constraints_from_flows(v, flow, mask)
    z, _, _ = forward(_as_list(v, v.pairs, off, loc), depth, state)
    mask.setflags(write=False)
    return v, state, flow, mask, off, loc, z
