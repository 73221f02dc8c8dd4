"""GPU parity (-m gpu) of the pair product at workload-shaped item lists (tests/product_cases.py).

The other parity tests reach the matrix-free product (k_matvec_pairs_fast / k_matvec_pairs) with a few dozen work items of at
most 128 constraints per direction, always at 256 threads.  Here the items hold up to 768 constraints per direction (three trips
of the constraint loop at 256 threads, six at 128), long pairs are split into several items with their partial rows, and the
item counts (850 / 1090) put every (KD, SPEC) variant of the fast kernel once inside and once outside its 128-thread window on a
256-CU device:
  a. J^T J (column by column through the product), gradient, frame blocks and cost against the CPU oracle, the candidate-cost
     kernel against both, and which instantiation ran (Solver.product_launch_debug),
  b. one LM step -- the product inside the PCG, with damping and the fused p = z + beta p -- against the oracle's exact step,
  c. the coarse level's edge blocks (k_coarse_edges_*) at the same item shapes.
Same bars as tests/test_gpu_parity.py: 1e-9 relative, f64 on both sides.
"""
import numpy as np
import pytest

from oracle.oracle import Oracle
from robust_cvd_amd import synth
from robust_cvd_amd.ctypes_types import OptParams, StaticLossType, ValueXformType, XformDesc
from tests import margins
from tests import product_cases as pc
from tests.helpers import rel
from tests.test_gpu_huber import _state

pytestmark = pytest.mark.gpu

TOL = 1e-9
CAUCHY, HUBER = 0, 1
GLOBAL = XformDesc.global_depth
GRID = lambda: XformDesc.grid_depth(4, 3)
CUBIC = lambda: XformDesc.grid_depth(4, 4, cubic=True)

# (id, case, depth transform, static loss, robustifier, generic kernels, KD, SPEC, kind, threads expected on 256 CUs)
VARIANTS = [
    ("items850-global-cauchy", "items850", GLOBAL, StaticLossType.ReproDisparity, CAUCHY, False, 1, 1, 1, 256),
    ("items850-grid4x3-huber", "items850", GRID, StaticLossType.ReproDisparity, HUBER, False, 4, 2, 1, 256),
    ("items850-cubic4x4-cauchy", "items850", CUBIC, StaticLossType.ReproDisparity, CAUCHY, False, 16, 1, 1, 128),
    ("items850-grid4x3-depthratio", "items850", GRID, StaticLossType.ReproDepthRatio, CAUCHY, False, 4, 0, 1, 128),
    ("items850-global_scaleshift-logdepth", "items850", lambda: XformDesc.global_depth(ValueXformType.ScaleShift),
     StaticLossType.ReproLogDepth, CAUCHY, False, 1, 0, 1, 128),
    ("items850-grid4x3-generic", "items850", GRID, StaticLossType.ReproDisparity, CAUCHY, True, 4, 0, 0, 256),
    ("items1090-global-cauchy", "items1090", GLOBAL, StaticLossType.ReproDisparity, CAUCHY, False, 1, 1, 1, 128),
    ("items1090-grid4x3-cauchy", "items1090", GRID, StaticLossType.ReproDisparity, CAUCHY, False, 4, 1, 1, 128),
    ("items1090-grid4x3-huber", "items1090", GRID, StaticLossType.ReproDisparity, HUBER, False, 4, 2, 1, 128),
    ("items1090-cubic4x4-depthratio", "items1090", CUBIC, StaticLossType.ReproDepthRatio, CAUCHY, False, 16, 0, 1, 256),
    ("items1090-cubic4x4-huber", "items1090", CUBIC, StaticLossType.ReproDisparity, HUBER, False, 16, 2, 1, 128),
]
LAUNCHES = {}   # variant id -> product_launch_debug() of its J^T J hook (the coverage condition reads it)


@pytest.fixture(scope="module")
def Solver():
    from robust_cvd_amd import api
    return api.Solver


def _params(loss=StaticLossType.ReproDisparity):
    p = OptParams.defaults()
    p.num_threads = 8
    p.static_loss_type = loss
    return p


def _loaded(ctor, video, ddesc, robust=CAUCHY, generic=False):
    s = ctor()
    synth.load_into(s, video)
    s.reset_depth_xforms(ddesc)
    s.reset_spatial_xforms(XformDesc.spatial())
    s.set_robust_loss(robust)
    if generic:
        s.set_generic_kernels(True)
    return s


def _hip_product(Solver, variant, state=None, **want):
    """The HIP side of a variant: evaluation with the J^T J hook, and what its last product launch was."""
    vid, case, ddesc, loss, robust, generic = variant[:6]
    v = pc.make_case(case)
    s = _loaded(lambda: Solver(0), v, ddesc(), robust, generic)
    if state is None:
        state = _state(s, v.num_frames, np.random.default_rng(17))
    pose, dx, _ = state
    s.set_xform_params(dx)
    r = s.evaluate(_params(loss), 0.1, pose, want_hfull=True, **want)
    LAUNCHES[vid] = s.product_launch_debug()
    return s, r, state


@pytest.mark.parametrize("variant", VARIANTS, ids=[v[0] for v in VARIANTS])
def test_product_gradient_blocks_and_cost_match_the_oracle(Solver, variant):
    vid, case, ddesc, loss, robust, generic, kd, spec, kind, _ = variant
    v = pc.make_case(case)
    F = v.num_frames
    s, h, state = _hip_product(Solver, variant, want_hdiag=True)
    pose, dx, _ = state
    p = _params(loss)
    orc = _loaded(Oracle, v, ddesc(), robust)
    orc.set_xform_params(dx)
    o = orc.evaluate(p, 0.1, pose, want_hdiag=True, want_hfull=True)

    assert h["num_residual_blocks"] == o["num_residual_blocks"]
    margins.below("cost", abs(h["cost"] - o["cost"]) / abs(o["cost"]), TOL)
    margins.below("gradient", rel(h["gradient"], o["gradient"]), TOL)
    margins.below("hdiag", rel(h["hdiag"], o["hdiag"]), TOL)
    margins.below("hfull", rel(h["hfull"], o["hfull"]), TOL)          # matrix-free product, column by column
    # Jacobi-scaled, entry by entry: an error confined to the depth rows cannot hide behind the much larger pose entries
    d = np.sqrt(np.diag(o["hfull"]))
    assert d.min() > 0.0
    scaled = np.abs(h["hfull"] - o["hfull"])
    scaled /= d[:, None]
    scaled /= d[None, :]
    worst = np.unravel_index(int(np.argmax(scaled)), scaled.shape)
    B = s.block_size()
    margins.below("hfull_jacobi_scaled", float(scaled[worst]), TOL,
                  info={"row (frame, unknown)": divmod(int(worst[0]), B), "column": divmod(int(worst[1]), B)})
    # candidate-cost kernel (k_cost_items*): the cost-only call
    c_only = s.evaluate(p, 0.1, pose, want_gradient=False)
    assert c_only["gradient"] is None and c_only["num_residual_blocks"] == o["num_residual_blocks"]
    margins.below("cost_only_vs_full", abs(c_only["cost"] - h["cost"]) / abs(h["cost"]), 1e-12)
    margins.below("cost_only_vs_oracle", abs(c_only["cost"] - o["cost"]) / abs(o["cost"]), TOL)

    # which instantiation ran
    L = LAUNCHES[vid]
    items = pc.expected_items(v, L["num_cu"])
    assert L["work_items"] == len(items), (L, len(items))
    assert (L["kind"], L["spec"], L["kd"]) == (kind, spec, kd), L
    if kind == 1 and margins.deterministic_build():
        assert L["threads"] == 64, L                                  # one wave per item: LDS atomics in program order
    elif kind == 1:
        assert L["threads"] == pc.expected_threads(kd, spec, B, L["num_cu"], len(items)), L
    else:
        assert L["threads"] == 256, L


def test_both_workgroup_sizes_ran_for_every_kd_and_spec(Solver):
    """The parametrisation above covers the 128- and the 256-thread instantiation of the fast list kernel for each of KD 1, 4, 16
    and for each of SPEC 0, 1, 2 (on a 256-CU device).  Read from what the launches reported, not from the table."""
    if margins.deterministic_build():
        pytest.skip("deterministic build: every fast list launch runs 64 threads, the workgroup-size rule is not exercised")
    for variant in VARIANTS:
        if variant[0] not in LAUNCHES:   # (this test selected alone)
            _hip_product(Solver, variant)
    fast = {vid: LAUNCHES[vid] for vid, *_rest in VARIANTS if LAUNCHES[vid]["kind"] == 1}
    by_kd = {(L["threads"], L["kd"]) for L in fast.values()}
    by_spec = {(L["threads"], L["spec"]) for L in fast.values()}
    moved = [f"{v[0]}: {LAUNCHES[v[0]]['threads']} threads for {LAUNCHES[v[0]]['work_items']} items on "
             f"{LAUNCHES[v[0]]['num_cu']} CUs, {v[9]} expected on 256 CUs" for v in VARIANTS
             if v[8] == 1 and LAUNCHES[v[0]]["threads"] != v[9]]
    missing = [("KD", kd, nt) for kd in (1, 4, 16) for nt in (128, 256) if (nt, kd) not in by_kd]
    missing += [("SPEC", sp, nt) for sp in (0, 1, 2) for nt in (128, 256) if (nt, sp) not in by_spec]
    assert not missing, {"instantiations not reached": missing, "variants outside their window": moved}


@pytest.mark.parametrize("case,ddesc", [("items850", GRID), ("items1090", GLOBAL)], ids=["items850-grid4x3", "items1090-global"])
def test_one_lm_step_matches_the_exact_step(Solver, case, ddesc):
    """One LM iteration from the same f64 state on both sides: the HIP step comes out of the PCG (product with damping and the
    fused p = z + beta p, two-level preconditioner) stopped at a relative residual of 1e-10 in the preconditioned norm, the
    oracle's out of a block Cholesky factorisation.  |dx_hip - dx_oracle| <= 1e-6 |dx_oracle|: the project's notes put the
    condition number of the damped, Jacobi-scaled system at up to ~1e8 (include/cvd_hip.h, coarse_dense_shift), a square-root
    factor of 1e4 on the 1e-10.  The oracle's own step is compared with a dense numpy solve of its (H + diag(lam)) dx = -g: ten
    times that distance has to stay below the bar for the bar to mean anything (logged as oracle_vs_dense_solve; ~1e-11 on
    the CPU, where the Jacobi-scaled damped systems of the two cases have condition numbers of 5e4 and 4e4).

    The state: from the raw draw of test_gpu_huber._state no first step is accepted -- the Gauss-Newton step at the initial
    trust radius (norm 1.7 to 3.4) lands where constraints project behind cameras, for every one of seeds 0..39 -- and a
    rejected step leaves nothing to compare.  The draw is therefore advanced by the ORACLE's first 8 LM iterations (the first
    five shrink the radius, three are accepted: cost 4.8e3 -> 9e1 and 6.5e3 -> 2.4e2, the minima are at 7.4 and 37), and that
    state, read back in f64, is what both sides start from.  A fresh step from there is accepted and is large (norm 1.1 / 1.7).
    The HIP solver takes no part in choosing it.  Measured on a MI355X: 2.0e-10 after 55 PCG iterations (items850, 256
    threads) and 5.3e-10 after 84 (items1090, 128 threads), the same on the deterministic build."""
    v = pc.make_case(case)
    F = v.num_frames
    hip = _loaded(lambda: Solver(0), v, ddesc())
    hip.set_options(pcg_relative_tolerance=1e-10)
    orc = _loaded(Oracle, v, ddesc())
    pose, dx, _ = _state(orc, F, np.random.default_rng(17))
    p = _params()
    p.max_iterations = 8
    orc.set_pose_params(pose)
    orc.set_xform_params(dx)
    orc.pose_optimization_step(p, 0.1, convert_poses=False)
    pose, dx = orc.get_pose_params(), orc.get_xform_params()
    ev = orc.evaluate(p, 0.1, pose, want_hfull=True)
    steps, accepted = {}, {}
    p.max_iterations = 1
    for k, s in (("hip", hip), ("oracle", orc)):
        s.set_pose_params(pose)
        s.set_xform_params(dx)
        s.pose_optimization_step(p, 0.1, convert_poses=False)
        steps[k] = np.concatenate([s.get_pose_params() - pose, s.get_xform_params() - dx], axis=1)
        sm = s.summary()
        accepted[k] = sm["num_successful_steps"] > 0
        assert sm["num_iterations"] == 1, (k, sm)
    assert accepted["oracle"], "the oracle must accept the step that is compared"
    assert accepted["hip"] == accepted["oracle"]
    ref = np.linalg.norm(steps["oracle"])
    assert ref > 0.0
    # the oracle against a dense solve of its own system: Ceres' LM on the column-scaled problem, scale = 1 / (1 + sqrt(H_ii)),
    # damping clamp(H_ii scale^2, 1e-6, 1e32) / radius with the initial radius 1e4
    H, g = ev["hfull"], ev["gradient"].reshape(-1)
    hd = np.diag(H)
    sc = 1.0 / (1.0 + np.sqrt(hd))
    lam = np.clip(hd * sc * sc, 1e-6, 1e32) / 1e4 / (sc * sc)
    exact = np.linalg.solve(H + np.diag(lam), -g).reshape(F, -1)
    margins.below("oracle_vs_dense_solve", float(10.0 * np.linalg.norm(steps["oracle"] - exact) / ref), 1e-6)
    print(f"lm step {case}: |dx| {ref:.3e}, hip vs oracle {np.linalg.norm(steps['hip'] - steps['oracle']) / ref:.3e}, "
          f"PCG iterations {hip.summary()['total_linear_iterations']}, launch {hip.product_launch_debug()}")
    margins.below("lm_step", float(np.linalg.norm(steps["hip"] - steps["oracle"]) / ref), 1e-6,
                  info={"linear_iterations": hip.summary()["total_linear_iterations"]})
    L = hip.product_launch_debug()
    assert L["kind"] == 1 and L["work_items"] == len(pc.expected_items(v, L["num_cu"])), L


def test_coarse_edge_blocks_at_workload_item_shapes(Solver):
    """k_coarse_edges_fast / k_coarse_edges_mfma walk the same work items as the product: off-diagonal 8 x 8 blocks of
    A_c = Z^T (J^T J + diag(lam)) Z against Z^T H Z of the oracle's dense J^T J at the linearisation point, with multi-trip
    items, split pairs and an absent direction (test_two_level_preconditioner does this on 20 frames of single-trip items)."""
    v = pc.make_case("items850")
    F = v.num_frames
    s = _loaded(lambda: Solver(0), v, GLOBAL())
    s.set_options(coarse_level=2)
    orc = _loaded(Oracle, v, GLOBAL())
    pose, dx, _ = _state(orc, F, np.random.default_rng(17))
    p = _params()
    p.max_iterations = 1
    s.set_pose_params(pose)
    s.set_xform_params(dx)
    s.pose_optimization_step(p, 0.1, convert_poses=False)   # one LM iteration from (pose, dx): the coarse matrix is built there
    assert s.path_info()["pose_graph_level"] == "exact sparse factor"
    dbg = s.coarse_debug()
    assert dbg is not None and dbg["failed"] == 0
    A = dbg["a_c"]
    n = A.shape[0]
    assert n == 8 * F
    orc.set_xform_params(dx)
    H = orc.evaluate(_params(), 0.1, pose, want_hfull=True)["hfull"]
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
    # every undirected pair of the list has its block, the long pairs included
    for e in pc.EDGES:
        a, b = pc.edge_frames(e, F)
        assert np.abs(A[a * 8:(a + 1) * 8, b * 8:(b + 1) * 8]).max() > 0.0
    # diagonal blocks = Z^T (H + diag(lam)) Z with lam >= 0
    assert (A - ZHZ)[~off].min() > -TOL * np.abs(ZHZ).max()
