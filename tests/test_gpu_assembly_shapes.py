"""GPU parity (-m gpu) of the frame-major assembly kernel (k_assemble_fast) at the shapes where it can go wrong.

The specialised walk (SPEC 1 / 2: one value parameter per vertex, ReproDisparity, Cauchy / Huber) accumulates the rotation
columns in each frame's local basis and transforms the frame's sums with the left Jacobian of SO(3) afterwards.  At the
sigma = 0.05 rad states of the other parity tests that Jacobian is the identity to a few per cent, and a wrong or transposed
transform would hide behind small numbers: here some frames are rotated by 0.5 - 0.9 rad.

One problem serves every variant: 8 frames, a hub frame (0) in enough pairs to be split into several parts (so the fold of
the parts meets the transform; asserted from the launch read-out), per-direction constraint counts 1, 63, 64, 65, 128, 129
and 300 (a partial wave, one unit of 128 exactly, a unit plus one, several units), a pair with only its backward direction
(5 -> 2) and a frame without constraints (7).  Gradient, the full frame blocks and the cost of Solver.evaluate are compared
against the CPU oracle at the bar of tests/test_gpu_parity.py (1e-9 relative, f64 on both sides) and against the generic
all-variants kernels.  The evaluate hook and the oracle return the total cost only; the per-frame costs the kernel writes
are read from the launch read-out and compared against the generic kernel's, frame by frame, and their sum against the total.
"""
import numpy as np
import pytest

from oracle.oracle import Oracle
from robust_cvd_amd import synth
from robust_cvd_amd.ctypes_types import IntrinsicsOptimization, OptParams, StaticLossType, XformDesc
from tests.helpers import rel

pytestmark = pytest.mark.gpu

TOL = 1e-9

# directed pair -> constraints kept
COUNTS = {(0, 1): 300, (1, 0): 129, (0, 2): 128, (2, 0): 65, (0, 3): 64, (3, 0): 63, (0, 4): 1, (4, 0): 300,
          (0, 5): 129, (5, 0): 128, (0, 6): 65, (6, 0): 1, (1, 2): 64, (2, 1): 63, (3, 4): 129, (4, 3): 1, (5, 2): 300}
FRAMES = 8

VARIANTS = [
    # id, depth transform, loss, robustifier (0 Cauchy, 1 Huber), intrinsics, regularisers, expected SPEC
    ("cauchy_grid", "grid", StaticLossType.ReproDisparity, 0, IntrinsicsOptimization.PerFrame, "default", 1),
    ("huber_grid", "grid", StaticLossType.ReproDisparity, 1, IntrinsicsOptimization.PerFrame, "default", 2),
    ("cauchy_global", "global", StaticLossType.ReproDisparity, 0, IntrinsicsOptimization.PerFrame, "default", 1),
    ("huber_global", "global", StaticLossType.ReproDisparity, 1, IntrinsicsOptimization.PerFrame, "default", 2),
    ("ratio_grid", "grid", StaticLossType.ReproDepthRatio, 0, IntrinsicsOptimization.PerFrame, "default", 0),
    ("shared_grid", "grid", StaticLossType.ReproDisparity, 0, IntrinsicsOptimization.Shared, "default", 0),
    ("fixed_grid", "grid", StaticLossType.ReproDisparity, 0, IntrinsicsOptimization.Fixed, "default", 1),
    # the constraints alone, and every regulariser that touches the pose rows / columns on: the basis transform comes BEFORE them
    ("cauchy_grid_no_regularisers", "grid", StaticLossType.ReproDisparity, 0, IntrinsicsOptimization.PerFrame, "off", 1),
    ("cauchy_grid_pose_and_deform_regularisers", "grid", StaticLossType.ReproDisparity, 0, IntrinsicsOptimization.PerFrame, "all", 1),
    ("huber_global_pose_regulariser", "global", StaticLossType.ReproDisparity, 1, IntrinsicsOptimization.PerFrame, "all", 2),
    # bicubic taps (KD = 16) go through the same specialised walk
    ("cauchy_bicubic", "cubic", StaticLossType.ReproDisparity, 0, IntrinsicsOptimization.PerFrame, "default", 1),
    ("huber_bicubic_pose_and_deform_regularisers", "cubic", StaticLossType.ReproDisparity, 1, IntrinsicsOptimization.PerFrame, "all", 2),
]
TAPS = {"grid": 4, "global": 1, "cubic": 16}


@pytest.fixture(scope="module")
def Solver():
    from robust_cvd_amd import api
    return api.Solver


@pytest.fixture(scope="module")
def problem():
    """(video, pose parameters): built once, never modified."""
    v = synth.make_video(FRAMES, 96, 56, seed=53, pairs=sorted(COUNTS), spacing=3.0, rot_sigma_deg=2.0)
    rng = np.random.default_rng(29)
    loc, off = [], [0]
    for k, (a, b) in enumerate(map(tuple, v.pairs)):
        have = int(v.offsets[k + 1] - v.offsets[k])
        want = COUNTS[(int(a), int(b))]
        assert have >= want, (a, b, have)
        keep = np.sort(rng.choice(have, want, replace=False)) + int(v.offsets[k])   # spread over the image: every grid cell is hit
        loc.append(v.loc[keep])
        off.append(off[-1] + want)
    v.loc = np.concatenate(loc, axis=0)
    v.offsets = np.asarray(off, dtype=np.int64)
    v.is_static = np.ones(v.loc.shape[0], dtype=np.uint8)
    assert sorted(np.diff(v.offsets).tolist()) == sorted(COUNTS.values())
    assert not (v.pairs == 7).any() and not any((2, 5) == tuple(p) for p in v.pairs)

    pose = np.zeros((FRAMES, 7))
    pose[:, :3] = rng.normal(0, 0.05, (FRAMES, 3))
    pose[:, 3:6] = rng.normal(0, 0.05, (FRAMES, 3))
    for f, angle in ((0, 0.6), (2, 0.9), (3, 0.5), (5, 0.75), (7, 0.55)):   # the hub among them; different axes
        axis = rng.normal(size=3)
        pose[f, 3:6] = angle * axis / np.linalg.norm(axis)
    assert (np.linalg.norm(pose[:, 3:6], axis=1) >= 0.5).sum() >= 5
    pose[:, 6] = 0.2 + rng.uniform(0, 0.02, FRAMES)
    return v, pose


def _params(loss, intr, regs):
    p = OptParams.defaults()
    p.num_threads = 2
    p.static_loss_type = loss
    p.intr_opt = intr
    if regs == "off":
        p.scale_reg = 0.0
        p.focal_reg = 0.0
    elif regs == "all":
        p.position_reg = 2.0
        p.adaptive_deformation_cost = 0.0
    return p, {"off": 0.0, "default": 0.1, "all": 0.7}[regs]


def _evaluate(ctor, problem, depth, loss, robust, intr, regs, generic=False):
    v, pose = problem
    s = ctor()
    synth.load_into(s, v)
    s.reset_depth_xforms(XformDesc.global_depth() if depth == "global" else XformDesc.grid_depth(4, 3, cubic=depth == "cubic"))
    s.reset_spatial_xforms(XformDesc.spatial())
    dx = s.get_xform_params()
    dx = 0.15 + np.random.default_rng(31).uniform(0, 0.05, dx.shape)
    s.set_xform_params(dx)
    s.set_robust_loss(robust)
    if generic:
        s.set_generic_kernels(True)
    p, deform = _params(loss, intr, regs)
    return s, s.evaluate(p, deform, pose, want_hdiag=True)


@pytest.mark.parametrize("vid,depth,loss,robust,intr,regs,spec", VARIANTS, ids=[c[0] for c in VARIANTS])
def test_assembly_matches_oracle_and_generic_kernels(Solver, problem, vid, depth, loss, robust, intr, regs, spec):
    _, o = _evaluate(Oracle, problem, depth, loss, robust, intr, regs)
    s, h = _evaluate(lambda: Solver(0), problem, depth, loss, robust, intr, regs)
    launch = s.assembly_launch_debug()
    sg, g = _evaluate(lambda: Solver(0), problem, depth, loss, robust, intr, regs, generic=True)
    cf_h, cf_g = launch["cost_frame"], sg.assembly_launch_debug()["cost_frame"]

    hd_h, hd_o, hd_g = h["hdiag"].copy(), o["hdiag"].copy(), g["hdiag"].copy()
    if intr == IntrinsicsOptimization.Shared:
        # (one focal length: the focal row / column of a frame's block is frame 0's slot, tests/test_gpu_parity.py compares it through
        # the full J^T J; here the rest of the blocks against the oracle, and everything against the generic kernel)
        hd_h[:, 6, :] = hd_h[:, :, 6] = 0.0
        hd_o[:, 6, :] = hd_o[:, :, 6] = 0.0
    print(f"{vid}: launch {launch}  cost rel {abs(h['cost'] - o['cost']) / abs(o['cost']):.2e}  "
          f"gradient rel {rel(h['gradient'], o['gradient']):.2e}  blocks rel {rel(hd_h, hd_o):.2e}  "
          f"hub block rel {rel(hd_h[0], hd_o[0]):.2e}  rotation rows rel {rel(hd_h[:, 3:6, :], hd_o[:, 3:6, :]):.2e}  "
          f"vs generic: gradient {rel(h['gradient'], g['gradient']):.2e} blocks {rel(h['hdiag'], hd_g):.2e} "
          f"per-frame cost {np.abs(cf_h - cf_g).max() / np.abs(cf_g).max():.2e}")

    # the instantiation under test really ran, and the hub frame really is split into parts
    assert launch["kind_name"] == "fast list" and launch["spec"] == spec and launch["kd"] == TAPS[depth], launch
    assert launch["split_parts"] >= 2 and launch["workgroups"] == FRAMES - 1 + launch["split_parts"], launch

    assert h["num_residual_blocks"] == o["num_residual_blocks"]
    assert abs(h["cost"] - o["cost"]) <= TOL * abs(o["cost"])
    assert rel(h["gradient"], o["gradient"]) < TOL
    assert rel(hd_h, hd_o) < TOL
    # per frame too (a small frame's error must not hide behind the hub's large block), and the rotation rows on their own
    for f in range(FRAMES):
        assert rel(hd_h[f], hd_o[f]) < TOL, f
        assert rel(h["gradient"][f], o["gradient"][f]) < TOL, f
    assert rel(hd_h[:, 3:6, :], hd_o[:, 3:6, :]) < TOL
    assert rel(h["gradient"][:, 3:6], o["gradient"][:, 3:6]) < TOL
    # the frame without constraints carries its regularisers only
    assert np.abs(h["gradient"][7, :6]).max() == 0.0 or regs == "all"

    assert abs(h["cost"] - g["cost"]) <= TOL * abs(g["cost"])
    assert rel(h["gradient"], g["gradient"]) < TOL
    assert rel(h["hdiag"], hd_g) < TOL
    # per-frame cost (a frame's regularisers and the constraints of the pairs it is the source of), frame by frame
    assert sg.assembly_launch_debug()["kind_name"] == "generic"
    assert cf_h.shape == (FRAMES,) and (cf_g[:7] > 0).all()
    assert (np.abs(cf_h - cf_g) <= TOL * np.abs(cf_g)).all(), (cf_h, cf_g)
    assert abs(cf_h.sum() - h["cost"]) <= TOL * abs(h["cost"])
