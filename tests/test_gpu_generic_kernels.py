"""GPU parity (-m gpu) of the generic <KD, KS> solve kernels with a spatial transform (tests/generic_cases.py).

A solve with a spatial transform (KS != 0) leaves the fast kernels: k_assemble<KD, KS>, k_matvec_pairs<KD, KS>, k_cost_items<KD, KS>,
k_coarse_edges<KD, KS> and the triplet kernels run instead.  Nearly every other kernel-level test resets the spatial transform to
identity; the golden vectors reach (1,4), (4,4), (16,16) on pairs of about 40 constraints.  Here, against the CPU oracle at the
same f64 state (the oracle pinned on each crossing by tests/test_generic_cases.py):
  1. cost, gradient, frame blocks and J^T J (column by column through the product; relative to the largest entry and
     Jacobi-scaled entry by entry: the spatial rows are orders of magnitude below the pose rows), the cost-only call against both,
     and which kernel ran, for every case;
  2. the off-diagonal blocks of the coarse matrix against Z^T H Z, Z built from the scale / shift layout of cvd_coarse.h;
  3. one LM step -- candidate cost, product, preconditioner and update together -- against the oracle's exact step;
  4. an identity-spatial control through the same body with set_generic_kernels.
What a 256-thread workgroup walks: k_assemble whole pairs (up to three trips on the small videos), the item kernels the work items
of compileTable -- at most 128 constraints on the small videos, up to 768 on the items_* cases.  Bars: 1e-9 relative for f64 cost,
gradient and J^T J (tests/test_gpu_parity.py), 1e-12 between the two cost kernels, 1e-6 for the LM step
(tests/test_gpu_product_shapes.py).  Every comparison is logged through tests/margins.py;
profiles/generic_kernels_margins.txt lists them.

Measured on a MI355X, product build and deterministic build alike (173 logged comparisons each): every distance to the oracle is
below 7e-15, the two cost kernels agree to 2.4e-16, the LM steps to 2.0e-9 (global_bicubic, 8 oracle iterations in), 7.6e-9
(grid4x3_bicubic_ratio, 82 PCG iterations) and 3e-10 (cubic4x4_bilinear_shared_huber); no kernel had to change.

Mutations, on scratch builds, against this module and against the GPU suite as it stood before it (885 tests; it was run once with the
second form of the first mutation and the other two in place together: 879 pass, and the six that fail were then run with each alone):
  * two tap weights of the KS = 16 gather swapped in evalSample: 11 tests here fail (every bicubic-spatial case of all three
    tests); before, the (16,16) golden vector noticed.  With the swap kept to KD != 16 -- (1,16), (4,16) -- 9 tests here fail;
    before, three converged solves did (the deferred-spatial schedules of test_gpu_parity.py and test_gpu_dense_mode.py, at their
    end-state bars) and no kernel-level test.
  * direction 1 dropped in k_cost_items<KD, KS != 0>: all 15 spatial evaluation cases here fail.  Before, the cost-only calls of
    test_gpu_model_branches.py (generic-cubic4x3_scaleshift-spatial: (16,4)) and test_reference_residuals.py (perframe_spatial3x2:
    (4,4)) noticed, and the same three converged solves.
  * the source depth in the target's scale column of k_coarse_edges<KD, KS != 0>: the five coarse tests here fail; before, nothing.
"""
import numpy as np
import pytest

from oracle.oracle import Oracle
from robust_cvd_amd.ctypes_types import IntrinsicsOptimization
from tests import generic_cases as gc
from tests import margins
from tests import product_cases as pc
from tests.helpers import rel

pytestmark = pytest.mark.gpu

TOL = 1e-9
COST_ONLY_VS_FULL = 1e-12
SYMMETRY = 1e-12
LM_STEP = 1e-6


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


_ORACLE = {}


def _oracle(cid):
    """The oracle's evaluation of a case at its state: computed once, shared, read-only."""
    if cid not in _ORACLE:
        c = gc.case(cid)
        o = gc.load(Oracle, cid)
        ev = o.evaluate(gc.params(c), 0.1, gc.put(o, gc.problem(cid)[2]), want_hdiag=True, want_hfull=True)
        for a in ev.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _ORACLE[cid] = ev
    return _ORACLE[cid]


def _hip(Solver, cid):
    s = gc.load(lambda: Solver(0), cid)
    if gc.case(cid).ks == 0:
        s.set_generic_kernels(True)    # the control: identity spatial transform, generic kernels by request
    return s


def _where(B):
    return lambda k: divmod(int(k), B)


@pytest.mark.parametrize("cid", gc.IDS)
def test_evaluation_and_candidate_cost_match_the_oracle(Solver, cid):
    c = gc.case(cid)
    v, trip, state = gc.problem(cid)
    F, B = c.frames, c.block
    p = gc.params(c)
    o = _oracle(cid)
    s = _hip(Solver, cid)
    pose = gc.put(s, state)
    h = s.evaluate(p, 0.1, pose, want_hdiag=True, want_hfull=True)
    ck = Checks(cid)

    # which kernel ran: a case that lands on a fast kernel fails
    A, P = s.assembly_launch_debug(), s.product_launch_debug()
    ck.true("block_size", s.block_size() == B, s.block_size())
    ck.true("spatial_transform", int(s.xform_desc(True).spatial_type) == int(c.spatial().spatial_type))
    ck.true("assembly_kernel", (A["kind"], A["kind_name"], A["threads"], A["kd"]) == (0, "generic", 256, c.kd),
            {k: x for k, x in A.items() if k != "cost_frame"})
    ck.true("product_kernel", (P["kind"], P["kind_name"], P["threads"], P["kd"]) == (0, "generic list", 256, c.kd), P)
    # what the item kernels walk (compileTable's rule, restated by tests/product_cases.py)
    items = pc.expected_items(v, P["num_cu"])
    ck.true("work_items", P["work_items"] == len(items), (P, len(items)))
    longest = max(max(m0, m1) for _, _, m0, m1 in items)
    print(f"{cid}: {len(items)} work items on {P['num_cu']} CUs, the longest direction {longest} constraints; "
          f"pairs of {int(np.diff(v.offsets).min())} .. {int(np.diff(v.offsets).max())}")
    if c.spacing is None and P["num_cu"] <= 256:
        ck.true("items_of_three_trips", longest == 768, longest)

    # 1. evaluation
    ck.true("num_residual_blocks", h["num_residual_blocks"] == o["num_residual_blocks"],
            (h["num_residual_blocks"], o["num_residual_blocks"]))
    ck.below("cost", _relcost(h["cost"], o["cost"]), TOL)
    ck.below("gradient", rel(h["gradient"], o["gradient"]), TOL)
    first = B - state[2].shape[1]
    if c.ks:   # the spatial rows on their own scale
        ck.below("gradient_spatial_rows", rel(h["gradient"][:, first:], o["gradient"][:, first:]), TOL)
    hd_h, hd_o = h["hdiag"].copy(), o["hdiag"].copy()
    if c.intr == IntrinsicsOptimization.Shared:
        # one focal length: the focal row / column of a frame's block is frame 0's slot, compared through the full J^T J
        hd_h[:, 6, :] = hd_h[:, :, 6] = 0.0
        hd_o[:, 6, :] = hd_o[:, :, 6] = 0.0
    ck.below("hdiag", rel(hd_h, hd_o), TOL)
    if c.ks:
        ck.below("hdiag_spatial_rows", rel(hd_h[:, first:, :], hd_o[:, first:, :]), TOL)
    Hh, Ho = h["hfull"], o["hfull"]
    ck.below("hfull", rel(Hh, Ho), TOL)                               # matrix-free product, column by column
    ck.below("hfull_symmetry", float(np.abs(Hh - Hh.T).max() / np.abs(Hh).max()), SYMMETRY)
    # Jacobi-scaled, entry by entry, over the unknowns the problem reaches (fixed / shared intrinsics leave focal slots empty)
    d = np.sqrt(np.diag(Ho))
    on = d > 0.0
    ck.true("unreached_unknowns_are_zero", not Hh[~on].any() and not Hh[:, ~on].any())
    ck.true("spatial_unknowns_are_reached", on.reshape(F, B)[:, first:].all())
    scaled = np.abs(Hh - Ho)[np.ix_(on, on)]
    scaled /= d[on][:, None]
    scaled /= d[on][None, :]
    worst = np.unravel_index(int(np.argmax(scaled)), scaled.shape)
    rows = np.flatnonzero(on)
    ck.below("hfull_jacobi_scaled", float(scaled[worst]), TOL,
             info={"row (frame, unknown)": _where(B)(rows[worst[0]]), "column": _where(B)(rows[worst[1]])})

    # 2. candidate cost (k_cost_items<KD, KS>, k_cost_triplets<KD, KS>): the cost-only call
    c_only = s.evaluate(p, 0.1, pose, want_gradient=False)
    ck.true("cost_only_shape", c_only["gradient"] is None and c_only["num_residual_blocks"] == o["num_residual_blocks"],
            c_only["num_residual_blocks"])
    ck.below("cost_only_vs_full", _relcost(c_only["cost"], h["cost"]), COST_ONLY_VS_FULL)
    ck.below("cost_only_vs_oracle", _relcost(c_only["cost"], o["cost"]), TOL)

    if trip is not None:
        # the smoothness weights on above; without them the cost is another one, on both sides and by both calls
        p0 = gc.params(c, smooth=False)
        orc = gc.load(Oracle, cid)
        o0 = orc.evaluate(p0, 0.1, gc.put(orc, state), want_gradient=False)
        h0 = s.evaluate(p0, 0.1, pose)
        ck.true("triplets_are_live", abs(h0["cost"] - h["cost"]) > 1e-3 * abs(h["cost"]), (h0["cost"], h["cost"]))
        ck.true("triplets_off:num_residual_blocks", h0["num_residual_blocks"] == o0["num_residual_blocks"])
        ck.below("triplets_off:cost", _relcost(h0["cost"], o0["cost"]), TOL)
    ck.done()


@pytest.mark.parametrize("cid", gc.COARSE_IDS)
def test_coarse_edge_blocks_match_the_projected_hessian(Solver, cid):
    """k_coarse_edges<KD, KS>: the off-diagonal 8 x 8 blocks of A_c = Z^T (J^T J + diag(lam)) Z against Z^T H Z of the oracle's
    J^T J at the linearisation point.  Z (gc.coarse_basis) has the seven pose columns and one column that is 1 on the frame's depth
    SCALES, 0 on its shifts and on its spatial parameters."""
    c = gc.case(cid)
    _, _, state = gc.problem(cid)
    F = c.frames
    s = _hip(Solver, cid)
    s.set_options(coarse_level=2)
    p = gc.params(c)
    p.max_iterations = 1
    s.set_pose_params(gc.put(s, state))
    s.pose_optimization_step(p, 0.1, convert_poses=False)   # one LM iteration from the state: the coarse matrix is built there
    assert s.path_info()["pose_graph_level"] == "exact sparse factor"
    assert s.product_launch_debug()["kind_name"] == "generic list" and s.path_info()["taps"] == c.kd
    dbg = s.coarse_debug()
    assert dbg is not None and dbg["failed"] == 0
    A = dbg["a_c"]
    n = A.shape[0]
    assert n == 8 * F
    Z = gc.coarse_basis(c)
    ZHZ = Z.T @ _oracle(cid)["hfull"] @ Z
    off = np.ones((n, n), bool)
    for f in range(F):
        off[f * 8:(f + 1) * 8, f * 8:(f + 1) * 8] = False
    ck = Checks(f"coarse:{cid}")
    scale = np.abs(ZHZ[off]).max()
    ck.below("off_diagonal_blocks", float(np.abs((A - ZHZ)[off]).max() / scale), TOL)
    # the depth-scale mode (row / column 7 of a block) on its own scale
    mode = np.zeros((n, n), bool)
    mode[7::8, :] = mode[:, 7::8] = True
    ck.below("off_diagonal_scale_mode", float(np.abs((A - ZHZ)[off & mode]).max() / np.abs(ZHZ[off & mode]).max()), TOL)
    v = gc.problem(cid)[0]
    for a, b in {(min(a, b), max(a, b)) for a, b in v.pairs.tolist()}:
        ck.true(f"block_{a}_{b}_is_there", np.abs(A[a * 8:(a + 1) * 8, b * 8:(b + 1) * 8]).max() > 0.0)
    # diagonal blocks = Z^T (H + diag(lam)) Z with lam >= 0 (an inactive mode -- the focal length when it is fixed -- is an identity row)
    ck.true("diagonal_blocks_exceed_by_damping_only", (A - ZHZ)[~off].min() > -TOL * np.abs(ZHZ).max(), (A - ZHZ)[~off].min())
    ck.done()


@pytest.mark.parametrize("cid", gc.LM_IDS)
def test_one_lm_step_matches_the_exact_step(Solver, cid):
    """The protocol of tests/test_gpu_product_shapes.test_one_lm_step_matches_the_exact_step on a spatial problem: one LM iteration
    from the same f64 state (gc.lm_state: chosen by the oracle alone), the PCG stopped at 1e-10; the HIP step against the oracle's
    block-Cholesky step.  tests/test_generic_cases.py holds the oracle's step to a dense solve of its own damped system at a
    tenth of this bar."""
    c = gc.case(cid)
    state, _ = gc.lm_state(cid)
    steps, accepted = {}, {}
    for k, ctor in (("oracle", Oracle), ("hip", lambda: Solver(0))):
        s = gc.load(ctor, cid)
        if k == "hip":
            s.set_options(pcg_relative_tolerance=1e-10)
        steps[k], accepted[k], sm = gc.one_lm_iteration(s, c, state)
        assert sm["num_iterations"] == 1, (k, sm)
    hip = s
    assert accepted["oracle"], "the oracle must accept the step that is compared"
    assert accepted["hip"] == accepted["oracle"]
    ref = np.linalg.norm(steps["oracle"])
    assert ref > 0.0
    L = hip.product_launch_debug()
    assert (L["kind_name"], L["threads"], L["kd"]) == ("generic list", 256, c.kd), L
    first = c.block - state[2].shape[1]
    diff = steps["hip"] - steps["oracle"]
    print(f"lm step {cid}: |dx| {ref:.3e}, hip vs oracle {np.linalg.norm(diff) / ref:.3e} (spatial rows on their own norm "
          f"{np.linalg.norm(diff[:, first:]) / np.linalg.norm(steps['oracle'][:, first:]):.3e}), "
          f"PCG iterations {hip.summary()['total_linear_iterations']}")
    margins.below(f"lm:{cid}:lm_step", float(np.linalg.norm(diff) / ref), LM_STEP,
                  info={"linear_iterations": hip.summary()["total_linear_iterations"]})
