"""GPU parity (-m gpu) of the flow-constraint model on its clamped and behind-camera branches (tests/branch_cases.py).

The states of the other parity tests keep z' and D_b positive for every constraint, so the clamps of the disparity residual
(1 / max(z', 1e-6) - 1 / max(D_b, 1e-6), a clamped side without derivative), the role switch of the ratio / log-ratio residuals
at z' = D_b with negative arguments, the clamp of the scale regulariser and of NormalizeDisparity are reached by no GPU test --
while the LM driver evaluates such points whenever a step overshoots.  Here Solver.evaluate is held to the CPU oracle at
planted states, on each case's whole list and on each population's list alone (R regular, Z: z' < eps, B: D_b < eps, ZB both), so
that a branch's contribution cannot hide behind the bulk; with the default (fast) kernels and with the generic ones; and which
instantiation ran is read from the launch read-outs.  Bar: 1e-9 relative, f64 on both sides, as tests/test_gpu_parity.py;
every comparison is logged through tests/margins.py.  scale_reg = 0 wherever D < eps occurs (the regulariser's clamp has its own
test).

Measured on a MI355X, product build and deterministic build alike (1099 logged comparisons each): every distance to the oracle is
below 1e-13 -- cost 5.8e-15, gradient 1.1e-14, frame blocks and J^T J 3.4e-14, Jacobi-scaled J^T J 7.4e-14 (a Z population under
the bicubic grid), cost-only call against the full call 4.8e-16 and against the oracle 2.6e-15, coarse edge blocks 5.6e-15 -- on
the whole lists and on every population's list alone, so no comparison needed a CPU-measured rounding floor in place of 1e-9.
Fast against generic kernels: cost 4.8e-16, gradient 6.5e-15, frame blocks and J^T J 1.4e-14; every case is below the 1e-12 that
tests/test_gpu_parity.test_fast_and_generic_product_kernels_agree uses at benign states, so 1e-12 is what is asserted here.
With the `zo ?` select of fastDepthResidual's d r2 / d z' removed (a clamped z' then keeps a derivative of -1e12) 15 of the 37
tests fail: every disparity case that holds a Z population, the coarse edge blocks and the four dense cases.
profiles/model_branches_margins.txt lists every comparison's worst value with its share of the bar (the largest: 1.4 %).
"""
import numpy as np
import pytest

from oracle.oracle import Oracle
from robust_cvd_amd.ctypes_types import IntrinsicsOptimization, OptParams, SmoothLossType, StaticLossType, XformDesc
from tests import branch_cases as bc
from tests import margins
from tests.helpers import rel

pytestmark = pytest.mark.gpu

TOL = 1e-9
FAST_VS_GENERIC = 1e-12   # (the bar at benign states holds here too: see the module docstring)
COST_ONLY_VS_FULL = 1e-12   # (two kernels, the same sums: the bar of tests/test_gpu_product_shapes.py)
# the product kernel's SPEC where it is not the assembly's: one shared focal length sends the assembly to its runtime-variant
# walk (SPEC 0, cvd_eval.hip), the product's rule (cvd_matvec.hip) does not look at the intrinsics and keeps the specialised form
PRODUCT_SPEC = {"grid4x3-disparity-shared": 1}


@pytest.fixture(scope="module")
def Solver():
    from robust_cvd_amd import api
    return api.Solver


class Checks:
    """Every comparison is made and logged (margins.below) before the test fails on the ones that missed."""

    def __init__(self, tag):
        self.tag, self.failed = tag, []

    def below(self, name, value, limit, info=None):
        try:
            margins.below(f"{self.tag}:{name}", value, limit, info)
        except AssertionError as e:
            self.failed.append(str(e))

    def true(self, name, cond, info=None):
        if not cond:
            self.failed.append(f"{self.tag}:{name}: {info}")

    def done(self):
        assert not self.failed, "\n".join(self.failed)


def _relcost(a, b):
    return abs(a - b) / abs(b)


def _evaluate(s, p, pose, hfull=True):
    return s.evaluate(p, 0.1, pose, want_hdiag=True, want_hfull=hfull)


_ORACLE = {}


def _oracle(vid, state_name, list_name, idx):
    """The oracle's evaluation of one list of a case: computed once, shared by the default and the generic kernels' comparisons."""
    key = (vid, state_name, list_name)
    if key not in _ORACLE:
        _, depth, loss, robust, intr, _, _, _ = bc.variant(vid)
        v, state = bc.case(vid, state_name)
        o = bc.load(Oracle, v, depth, robust, subset=idx)
        ev = _evaluate(o, bc.params(loss, intr=intr), bc.put(o, state))
        for a in ev.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _ORACLE[key] = ev
    return _ORACLE[key]


def _compare(ck, name, h, o, B, shared):
    """cost, gradient, frame blocks, J^T J (relative to the largest entry and Jacobi-scaled entry by entry) of h against o."""
    ck.true(f"{name}:num_residual_blocks", h["num_residual_blocks"] == o["num_residual_blocks"],
            (h["num_residual_blocks"], o["num_residual_blocks"]))
    ck.below(f"{name}:cost", _relcost(h["cost"], o["cost"]), TOL)
    ck.below(f"{name}:gradient", rel(h["gradient"], o["gradient"]), TOL)
    hd_h, hd_o = h["hdiag"].copy(), o["hdiag"].copy()
    if shared:   # one focal length: the focal row / column of a frame's block is frame 0's slot, compared through the full J^T J
        hd_h[:, 6, :] = hd_h[:, :, 6] = 0.0
        hd_o[:, 6, :] = hd_o[:, :, 6] = 0.0
    ck.below(f"{name}:hdiag", rel(hd_h, hd_o), TOL)
    ck.below(f"{name}:hfull", rel(h["hfull"], o["hfull"]), TOL)          # matrix-free product, column by column
    # Jacobi-scaled, entry by entry, over the unknowns the list reaches (a population's list leaves some frames without constraints)
    d = np.sqrt(np.diag(o["hfull"]))
    on = d > 0.0
    ck.true(f"{name}:unreached_unknowns_are_zero", not h["hfull"][~on].any() and not h["hfull"][:, ~on].any())
    scaled = np.abs(h["hfull"] - o["hfull"])[np.ix_(on, on)]
    scaled /= d[on][:, None]
    scaled /= d[on][None, :]
    worst = np.unravel_index(int(np.argmax(scaled)), scaled.shape)
    rows = np.flatnonzero(on)
    ck.below(f"{name}:hfull_jacobi_scaled", float(scaled[worst]), TOL,
             info={"row (frame, unknown)": divmod(int(rows[worst[0]]), B), "column": divmod(int(rows[worst[1]]), B)})


def _check_launches(ck, name, s, generic, kd, spec, product_spec):
    """Which instantiation ran: a case that silently fell to another kernel fails."""
    P, A = s.product_launch_debug(), s.assembly_launch_debug()
    A = {k: v for k, v in A.items() if k != "cost_frame"}
    if generic or spec is None:
        ck.true(f"{name}:product_kernel", P["kind_name"] == "generic list", P)
        ck.true(f"{name}:assembly_kernel", A["kind_name"] == "generic", A)
    else:
        ck.true(f"{name}:product_kernel", (P["kind_name"], P["spec"], P["kd"]) == ("fast list", product_spec, kd), P)
        ck.true(f"{name}:assembly_kernel", (A["kind_name"], A["spec"], A["kd"]) == ("fast list", spec, kd), A)


@pytest.mark.parametrize("vid,state_name", bc.CASES, ids=[f"{a}-{b}" for a, b in bc.CASES])
def test_evaluation_matches_the_oracle_on_every_branch(Solver, vid, state_name):
    _, depth, loss, robust, intr, kd, spec, _ = bc.variant(vid)
    v, state = bc.case(vid, state_name)
    shared = intr == IntrinsicsOptimization.Shared
    p = bc.params(loss, intr=intr)
    ck = Checks(f"{vid}@{state_name}")
    for list_name, idx in bc.lists(v, depth, state, shared).items():
        o = _oracle(vid, state_name, list_name, idx)
        got = {}
        for kernels in (("fast", "generic") if spec is not None else ("generic",)):
            s = bc.load(lambda: Solver(0), v, depth, robust, subset=idx)
            if kernels == "generic":
                s.set_generic_kernels(True)
            pose = bc.put(s, state)
            h = got[kernels] = _evaluate(s, p, pose)
            name = f"{list_name}:{kernels}"
            _check_launches(ck, name, s, kernels == "generic", kd, spec, PRODUCT_SPEC.get(vid, spec))
            _compare(ck, name, h, o, s.block_size(), shared)
            # candidate-cost kernel (k_cost_items*): the cost-only call, against the full call and against the oracle
            c_only = s.evaluate(p, 0.1, pose, want_gradient=False)
            ck.true(f"{name}:cost_only_shape", c_only["gradient"] is None and c_only["num_residual_blocks"] == o["num_residual_blocks"])
            ck.below(f"{name}:cost_only_vs_full", _relcost(c_only["cost"], h["cost"]), COST_ONLY_VS_FULL)
            ck.below(f"{name}:cost_only_vs_oracle", _relcost(c_only["cost"], o["cost"]), TOL)
        if len(got) == 2:
            f, g = got["fast"], got["generic"]
            ck.below(f"{list_name}:fast_vs_generic:cost", _relcost(f["cost"], g["cost"]), FAST_VS_GENERIC)
            for key in ("gradient", "hdiag", "hfull"):
                ck.below(f"{list_name}:fast_vs_generic:{key}", rel(f[key], g[key]), FAST_VS_GENERIC)
    ck.done()


@pytest.mark.parametrize("kernels", ["fast", "generic"])
def test_a_non_finite_cost_stays_non_finite(Solver, kernels):
    """Log-ratio loss with z' < 0 < D_b (state mixed_sign_log): the oracle's cost is NaN.  The driver maps a non-finite candidate
    to a rejection; a reduction that dropped the NaN would accept garbage.  Both calls must return a non-finite cost."""
    depth = "global_scaleshift"
    v, state = bc.video(4), bc.mixed_sign_log()
    idx = bc.lists(v, depth, state)["all"]
    p = bc.params(StaticLossType.ReproLogDepth)
    o = bc.load(Oracle, v, depth, subset=idx)
    assert not np.isfinite(o.evaluate(p, 0.1, bc.put(o, state), want_gradient=False)["cost"])
    s = bc.load(lambda: Solver(0), v, depth, subset=idx)
    if kernels == "generic":
        s.set_generic_kernels(True)
    pose = bc.put(s, state)
    full = s.evaluate(p, 0.1, pose)
    assert s.product_launch_debug()["kind_name"] in ("none", "fast list" if kernels == "fast" else "generic list")
    assert s.assembly_launch_debug()["kind_name"] == ("fast list" if kernels == "fast" else "generic")
    assert not np.isfinite(full["cost"]), full["cost"]
    c_only = s.evaluate(p, 0.1, pose, want_gradient=False)
    assert not np.isfinite(c_only["cost"]), c_only["cost"]


@pytest.mark.parametrize("loss", [StaticLossType.ReproDisparity, StaticLossType.ReproDepthRatio, StaticLossType.ReproLogDepth],
                         ids=["disparity", "ratio", "logdepth"])
def test_the_driver_rejects_the_first_step_from_the_raw_draw(Solver, loss):
    """One LM iteration from the raw draw on video(5), grid_depth(5, 4): the step lands on the clamped / negative branches and the
    oracle rejects it under each loss (tests/test_branch_cases.py).  The decision rests on the candidate-cost kernel there.  The
    candidate's cost itself is compared at state lm_candidate above: the PCG step and the Cholesky step differ."""
    v = bc.video(5)
    state = bc.raw_state(v, "grid5x4")
    p = bc.params(loss, scale_reg=None)
    p.max_iterations = 1
    for k, ctor in (("oracle", Oracle), ("hip", lambda: Solver(0))):
        s = bc.load(ctor, v, "grid5x4")
        if k == "hip":
            s.set_options(pcg_relative_tolerance=1e-10)
        s.set_pose_params(bc.put(s, state))
        s.pose_optimization_step(p, 0.1, convert_poses=False)
        sm, rec = s.summary(), s.records()
        assert sm["num_successful_steps"] == 0, (k, sm)
        assert sm["final_cost"] == sm["initial_cost"], (k, sm)
        assert len(rec) >= 2 and rec[1]["step_is_successful"] == 0 and rec[1]["cost_change"] < 0, (k, rec)
        assert np.array_equal(s.get_pose_params(), state[0]), k
        assert np.array_equal(s.get_xform_params(), state[1]), k


@pytest.mark.parametrize("kernels", ["fast", "generic"])
@pytest.mark.parametrize("depth", ["global", "grid5x4"])
def test_the_scale_regularisers_clamp_alone(Solver, depth, kernels):
    """State negative_depth with every constraint flagged dynamic: only the regularisers remain, and the scale regulariser
    (default scale_reg) samples frame 1 where D < eps: residual 1 / 1e-6 - 1, no derivative."""
    v, state = bc.video(4), bc.negative_depth(depth)
    p = bc.params(scale_reg=None)
    res = {}
    for k, ctor in (("oracle", Oracle), ("hip", lambda: Solver(0))):
        s = bc.load(ctor, v, depth, all_dynamic=True)
        if k == "hip" and kernels == "generic":
            s.set_generic_kernels(True)
        res[k] = s.evaluate(p, 0.1, bc.put(s, state), want_hdiag=True)
    h, o = res["hip"], res["oracle"]
    assert o["cost"] > 1e10                      # the clamp is what the cost consists of
    assert h["num_residual_blocks"] == o["num_residual_blocks"]
    ck = Checks(f"scale_reg:{depth}:{kernels}")
    ck.below("cost", _relcost(h["cost"], o["cost"]), TOL)
    ck.below("gradient", rel(h["gradient"], o["gradient"]), TOL)
    ck.below("hdiag", rel(h["hdiag"], o["hdiag"]), TOL)
    # frame by frame: the clamped frame's (small) entries must not hide behind the others
    for f in range(v.num_frames):
        if np.abs(o["gradient"][f]).max() > 0:
            ck.below(f"gradient_frame{f}", rel(h["gradient"][f], o["gradient"][f]), TOL)
        else:
            ck.true(f"gradient_frame{f}_is_zero", not h["gradient"][f].any())
        ck.below(f"hdiag_frame{f}", rel(h["hdiag"][f], o["hdiag"][f]), TOL)
    ck.done()


@pytest.mark.parametrize("depth", ["global", "global_scaleshift"])
def test_normalize_depth_from_a_negative_depth_state(Solver, depth):
    """NormalizeDisparity clamps D like the disparity residual: normalize_depth with the pair loop
    (tests/test_gpu_parity.test_normalize_depth_pair_loop_matches_oracle) started at state negative_depth.  scale_reg = 0 (its
    clamp, 3e13, would bury the loss under test; without it the depth scale is free and a converged solve has nothing to
    compare), so one LM iteration: the initial cost holds the loss, the accepted first step its gradient and J^T J."""
    v, state = bc.video(4), bc.negative_depth(depth)
    p = OptParams.defaults()
    p.num_threads = 2
    p.normalize_depth_from_first_frame = 0
    p.scale_reg = 0.0
    p.max_iterations = 1
    th, sm = {}, {}
    for k, ctor in (("oracle", Oracle), ("hip", lambda: Solver(0))):
        s = bc.load(ctor, v, depth)
        s.set_pose_params(bc.put(s, state))
        s.normalize_depth(p)
        th[k], sm[k] = s.get_xform_params(), s.summary()
    assert sm["hip"]["num_residual_blocks"] == sm["oracle"]["num_residual_blocks"]
    assert sm["oracle"]["num_successful_steps"] == 1 and sm["hip"]["num_successful_steps"] == 1, sm
    assert np.abs(th["oracle"] - state[1]).max() > 0.1          # a real step
    margins.below("normalize:initial_cost", _relcost(sm["hip"]["initial_cost"], sm["oracle"]["initial_cost"]), TOL)
    margins.below("normalize:final_cost", abs(sm["hip"]["final_cost"] - sm["oracle"]["final_cost"]),
                  1e-6 * abs(sm["oracle"]["final_cost"]) + 1e-12)
    margins.below("normalize:parameters", rel(th["hip"], th["oracle"]), 1e-3)


@pytest.mark.parametrize("smooth_type", [SmoothLossType.ReproDisparityLaplacian, SmoothLossType.ReproDepthRatioConsistency],
                         ids=["disparity_laplacian", "depth_ratio_consistency"])
def test_triplets_behind_the_centre_camera(Solver, smooth_type):
    """cvd_triplets.h has its own clamps: the grid3x2 case of tests/test_gpu_triplets.py with frames 2 and 4 moved forward, so that
    28 of 59 triplets have an outer point behind the centre camera (bc.triplet_case).  The pair constraints are flagged dynamic:
    the triplets and the regularisers alone."""
    v, state, trip, _, _ = bc.triplet_case()
    p = bc.params(scale_reg=None)
    p.smooth_loss_type = smooth_type
    p.smooth_static_weight, p.smooth_dynamic_weight = 2.0, 0.5
    res = {}
    for k, ctor in (("oracle", Oracle), ("hip", lambda: Solver(0))):
        s = bc.load(ctor, v, "grid3x2", all_dynamic=True)
        s.set_triplet_constraints(*trip)
        res[k] = s.evaluate(p, 0.1, bc.put(s, state), want_hdiag=True)
    h, o = res["hip"], res["oracle"]
    assert h["num_residual_blocks"] == o["num_residual_blocks"]
    ck = Checks(f"triplets:{int(smooth_type)}")
    ck.below("cost", _relcost(h["cost"], o["cost"]), TOL)
    ck.below("gradient", rel(h["gradient"], o["gradient"]), TOL)
    ck.below("hdiag", rel(h["hdiag"], o["hdiag"]), TOL)
    ck.done()


def test_coarse_edge_blocks_behind_the_camera(Solver):
    """k_coarse_edges_fast at state behind (Global, Disparity, Cauchy), as
    tests/test_gpu_product_shapes.test_coarse_edge_blocks_at_workload_item_shapes: off-diagonal 8 x 8 blocks of the coarse matrix
    against Z^T H Z of the oracle's J^T J at the linearisation point."""
    depth = "global"
    v, state = bc.video(4), bc.behind(depth)
    idx = bc.lists(v, depth, state)["all"]
    F = v.num_frames
    s = bc.load(lambda: Solver(0), v, depth, subset=idx)
    s.set_options(coarse_level=2)
    orc = bc.load(Oracle, v, depth, subset=idx)
    p = bc.params(scale_reg=None)
    p.max_iterations = 1
    s.set_pose_params(bc.put(s, state))
    s.pose_optimization_step(p, 0.1, convert_poses=False)   # one LM iteration from the state: the coarse matrix is built there
    dbg = s.coarse_debug()
    assert dbg is not None and dbg["failed"] == 0
    A = dbg["a_c"]
    n = A.shape[0]
    assert n == 8 * F
    H = orc.evaluate(bc.params(scale_reg=None), 0.1, bc.put(orc, state), want_hfull=True)["hfull"]
    B = orc.block_size()
    Z = np.zeros((F * B, n))
    for f in range(F):
        Z[f * B:f * B + 7, f * 8:f * 8 + 7] = np.eye(7)
        Z[f * B + 7:(f + 1) * B, f * 8 + 7] = 1.0
    ZHZ = Z.T @ H @ Z
    off = np.ones((n, n), bool)
    for f in range(F):
        off[f * 8:(f + 1) * 8, f * 8:(f + 1) * 8] = False
    margins.below("coarse_off_diagonal_blocks", np.abs((A - ZHZ)[off]).max() / np.abs(ZHZ[off]).max(), TOL)
    # the pairs into the moved frame, block by block (their entries are the ones the clamp shapes)
    for a in (0, 1, 3):
        blk, ref = A[a * 8:(a + 1) * 8, 16:24], ZHZ[a * 8:(a + 1) * 8, 16:24]
        margins.below(f"coarse_block_{a}_2", np.abs(blk - ref).max() / np.abs(ref).max(), TOL)
    assert (A - ZHZ)[~off].min() > -TOL * np.abs(ZHZ).max()     # diagonal blocks = Z^T (H + diag(lam)) Z with lam >= 0


@pytest.mark.parametrize("product", ["explicit_blocks", "matrix_free"])
@pytest.mark.parametrize("depth", ["global", "grid6x4"])
def test_dense_mode_behind_the_camera(Solver, depth, product):
    """dwChain of k_dense_walk and the dense products at state behind, on the smallest raster of tests/test_gpu_dense_mode.py (20 x 12):
    a tenth of the valid pixels project behind frame 2 (bc.dense_case).  The oracle gets the equivalent list."""
    v, state, flow, mask, off, loc, _ = bc.dense_case(depth)
    hip, orc = Solver(0), Oracle()
    hip.set_options(dense_matrix_free=int(product == "matrix_free"))
    for s in (hip, orc):
        s.set_video(v.num_frames, v.width, v.height, v.aspect, v.inv_aspect)
        s.set_depth_all(v.depth)
        s.reset_poses()
    hip.set_pair_flows(v.pairs, flow, mask)
    orc.set_pair_constraints(v.pairs, off, loc, None)
    p = bc.params(scale_reg=None)
    res = {}
    for k, s in (("hip", hip), ("oracle", orc)):
        s.reset_depth_xforms(bc.DEPTHS[depth][0]())
        s.reset_spatial_xforms(XformDesc.spatial())
        res[k] = s.evaluate(p, 0.1, bc.put(s, state), want_hdiag=True, want_hfull=True)
    h, o = res["hip"], res["oracle"]
    assert hip.num_active_constraints() == int(off[-1])
    assert h["num_residual_blocks"] == o["num_residual_blocks"]
    ck = Checks(f"dense:{depth}:{product}")
    ck.below("cost", _relcost(h["cost"], o["cost"]), TOL)
    ck.below("gradient", rel(h["gradient"], o["gradient"]), TOL)
    ck.below("hdiag", rel(h["hdiag"], o["hdiag"]), TOL)
    ck.below("hfull", rel(h["hfull"], o["hfull"]), TOL)
    ck.done()
