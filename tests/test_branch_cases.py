"""The planted states of tests/branch_cases.py, held to their conditions on the CPU (no GPU needed).

Why the file exists: at the draw every GPU parity test uses, no constraint is on a clamped or negative branch of the model
(test_the_benign_draw_reaches_no_branch).  The planted states reach them with the populations below; the conditions are
requirements, not measurements:
  * a constraint within 1e-3 of a threshold, or with |z'| < 1e-2, is dropped; at most 10 % of a case is dropped,
  * each planted population holds >= 32 constraints and >= 5 % of the case's whole list,
  * for the ratio / log-ratio cases both sides of z' < D_b hold >= 5 % within each sign class (both positive: R, both negative: ZB),
  * the oracle is finite at every state but mixed_sign_log, where it is not.
"""
import numpy as np
import pytest

from oracle import oracle as om
from oracle.oracle import Oracle
from robust_cvd_amd.ctypes_types import IntrinsicsOptimization, SmoothLossType, StaticLossType
from tests import branch_cases as bc

PLANTED = {"behind": ("Z",), "negative_depth": ("B", "ZB"), "both_negative_log": ("ZB",)}
RATIO_LIKE = (StaticLossType.ReproDepthRatio, StaticLossType.ReproLogDepth)


@pytest.mark.parametrize("depth", sorted(bc.DEPTHS))
@pytest.mark.parametrize("frames", [4, 5])
def test_the_benign_draw_reaches_no_branch(depth, frames):
    v = bc.video(frames)
    pops, dropped, z, Db = bc.populations(v, depth, bc.raw_state(v, depth))
    assert len(pops["R"]) == v.num_constraints and len(dropped) == 0
    assert all(len(pops[k]) == 0 for k in ("Z", "B", "ZB"))
    assert z.min() > 0.4 and Db.min() > 0.4     # nowhere near a clamp


@pytest.mark.parametrize("vid,state_name", bc.CASES, ids=[f"{a}-{b}" for a, b in bc.CASES])
def test_populations_and_oracle_at_the_planted_states(vid, state_name):
    _, depth, loss, robust, intr, _, _, _ = bc.variant(vid)
    v, state = bc.case(vid, state_name)
    shared = intr == IntrinsicsOptimization.Shared
    pops, dropped, z, Db = bc.populations(v, depth, state, shared)
    kept = sum(len(x) for x in pops.values())
    assert kept + len(dropped) == v.num_constraints
    assert len(dropped) <= 0.10 * v.num_constraints, len(dropped)
    for k in PLANTED.get(state_name, ()):
        assert len(pops[k]) >= 32 and len(pops[k]) >= 0.05 * kept, (k, len(pops[k]), kept)
    if loss in RATIO_LIKE and state_name != "lm_candidate":
        for k in ("R", "ZB"):
            if len(pops[k]):
                below = int((z[pops[k]] < Db[pops[k]]).sum())
                assert min(below, len(pops[k]) - below) >= 0.05 * len(pops[k]), (k, below, len(pops[k]))
    if state_name == "both_negative_log":
        into1 = np.concatenate([np.arange(v.offsets[k], v.offsets[k + 1]) for k, (_, b) in enumerate(v.pairs) if b == 1])
        assert len(dropped) == 0 and sorted(pops["ZB"]) == sorted(into1)
        assert (z * Db > 0).all()                # no mixed signs anywhere: the log-ratio loss is finite

    # the numpy restatement of D_a, D_b against the oracle's own (z' has no read-out: it is the restatement's alone)
    o = bc.load(Oracle, v, depth, robust)
    pose = bc.put(o, state)
    p = bc.params(loss, intr=intr)
    sr = om.static_residuals(o, p, 0.1, pose)
    _, Da, _ = bc.forward(v, depth, state, shared)
    assert np.abs(sr["cam_a"][:, 2] - Da).max() <= 1e-12 * np.abs(Da).max()
    assert np.abs(sr["depth_b"] - Db).max() <= 1e-12 * np.abs(Db).max()

    # the oracle is finite on every list the GPU test compares
    for name, idx in bc.lists(v, depth, state, shared).items():
        o = bc.load(Oracle, v, depth, robust, subset=idx)
        ev = o.evaluate(p, 0.1, bc.put(o, state), want_hdiag=True, want_hfull=True)
        assert np.isfinite(ev["cost"]) and np.isfinite(ev["gradient"]).all() and np.isfinite(ev["hfull"]).all(), name
        assert np.isfinite(ev["hdiag"]).all(), name


def test_mixed_signs_make_the_log_ratio_loss_non_finite():
    v, state = bc.video(4), bc.mixed_sign_log()
    pops, _, z, Db = bc.populations(v, "global_scaleshift", state)
    assert len(pops["Z"]) >= 32 and (z[pops["Z"]] < 0).all() and (Db[pops["Z"]] > 0).all()
    o = bc.load(Oracle, v, "global_scaleshift", subset=bc.lists(v, "global_scaleshift", state)["all"])
    ev = o.evaluate(bc.params(StaticLossType.ReproLogDepth), 0.1, bc.put(o, state), want_gradient=False)
    assert not np.isfinite(ev["cost"])


@pytest.mark.parametrize("loss", [StaticLossType.ReproDisparity, StaticLossType.ReproDepthRatio, StaticLossType.ReproLogDepth])
def test_the_first_lm_step_from_the_raw_draw_is_rejected_by_the_oracle(loss):
    """What tests/test_gpu_model_branches.py asks of the driver: on video(5) with grid_depth(5, 4) the oracle rejects the first
    step from the raw draw under each of the three reprojection losses."""
    v = bc.video(5)
    state = bc.raw_state(v, "grid5x4")
    o = bc.load(Oracle, v, "grid5x4")
    p = bc.params(loss, scale_reg=None)
    p.max_iterations = 1
    o.set_pose_params(bc.put(o, state))
    o.pose_optimization_step(p, 0.1, convert_poses=False)
    sm, rec = o.summary(), o.records()
    assert sm["num_successful_steps"] == 0 and sm["final_cost"] == sm["initial_cost"]
    assert rec[1]["step_is_successful"] == 0 and rec[1]["cost_change"] < 0
    assert np.array_equal(o.get_pose_params(), state[0]) and np.array_equal(o.get_xform_params(), state[1])


def test_triplets_with_an_outer_point_behind_the_centre_camera():
    v, state, trip, zo, other = bc.triplet_case()
    assert len(zo) == int(trip[1][-1]) and (np.diff(trip[1]) > 0).all()
    assert int((zo < bc.EPS).any(axis=1).sum()) >= 16
    assert np.abs(zo).min() >= bc.SMALL_Z and np.abs(other).min() >= bc.SMALL_Z
    for stype in (SmoothLossType.ReproDisparityLaplacian, SmoothLossType.ReproDepthRatioConsistency):
        o = bc.load(Oracle, v, "grid3x2", all_dynamic=True)
        o.set_triplet_constraints(*trip)
        p = bc.params(scale_reg=None)
        p.smooth_loss_type = stype
        p.smooth_static_weight, p.smooth_dynamic_weight = 2.0, 0.5
        ev = o.evaluate(p, 0.1, bc.put(o, state), want_hdiag=True)
        assert np.isfinite(ev["cost"]) and np.isfinite(ev["gradient"]).all() and np.isfinite(ev["hdiag"]).all()


@pytest.mark.parametrize("depth", ["global", "grid6x4"])
def test_dense_pixels_behind_the_camera(depth):
    v, state, flow, mask, off, loc, z = bc.dense_case(depth)
    assert len(z) == int(off[-1])
    assert int((z < bc.EPS).sum()) >= 0.05 * len(z)
    assert np.abs(z).min() >= bc.SMALL_Z and np.abs(z - bc.EPS).min() >= bc.NEAR
