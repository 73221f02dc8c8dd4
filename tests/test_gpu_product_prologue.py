"""GPU parity (-m gpu) of the pair product at the shapes where its prologue can go wrong.

k_matvec_pairs_fast requests every load of its prologue unconditionally, from clamped or substituted addresses, takes one wait and
stores to LDS behind it; the item comes from one packed record and the epilogue's frame constants from LDS.  What that can get
wrong is an address or a predicate at an edge, so the cases are edges, on six frames:
  * the Global level (KD = 1, B = 8: almost every thread lies beyond B),
  * a bilinear grid with B = 139, just above 128, at 256 threads and -- on a list long enough for the 128-thread window of a
    256-CU device -- at 128 threads, two elements per thread,
  * the benchmark's B = 177,
  * shared intrinsics (the p[6] path),
  * items with one empty direction on the FIRST and on the LAST pair of the table (the empty range of the latter starts at the
    table's end), an item whose reverse pair does not exist at all, and items of frame 0 and frame F - 1,
  * inside the PCG: the first product of a solve (useBeta = 0) and the later ones, with the pose-graph level and the temporal
    depth-grid level on and off (null CoarseView pointers).
Entry points, comparisons and bars are those of tests/test_gpu_product_shapes.py: J^T J column by column through the product
against the CPU oracle and against the generic kernel at 1e-9 relative, one LM step out of the PCG against the oracle's exact step
at 1e-6.
"""
import functools

import numpy as np
import pytest

from oracle.oracle import Oracle
from robust_cvd_amd import synth
from robust_cvd_amd.ctypes_types import IntrinsicsOptimization, OptParams, XformDesc
from tests import margins
from tests import product_cases as pc
from tests.helpers import rel
from tests.test_gpu_huber import _state

pytestmark = pytest.mark.gpu

TOL = 1e-9
F = 6


@pytest.fixture(scope="module")
def Solver():
    from robust_cvd_amd import api
    return api.Solver


def _cut(video, counts):
    """The video with the constraint lists of the directed pairs in `counts` cut to that many entries (spread over the list, order
    kept); the other pairs stay."""
    chunks, off = [], [0]
    for k, p in enumerate(video.pairs.tolist()):
        loc = video.loc[video.offsets[k]:video.offsets[k + 1]]
        want = counts.get(tuple(p))
        if want is not None:
            assert loc.shape[0] >= want, (p, loc.shape[0], want)
            loc = loc[np.unique(np.linspace(0, loc.shape[0] - 1, want).astype(np.int64))]
            assert loc.shape[0] == want
        chunks.append(loc)
        off.append(off[-1] + loc.shape[0])
    video.loc = np.ascontiguousarray(np.concatenate(chunks, axis=0))
    video.offsets = np.asarray(off, dtype=np.int64)
    video.is_static = np.ones(video.loc.shape[0], dtype=np.uint8)
    return video


@functools.lru_cache(maxsize=None)
def edge_video():
    """Six frames at 64 x 40, pairs up to two frames apart in both directions (~300 constraints each: several 128-constraint items
    per pair), and:
      (0, 1) cut to ONE constraint, the FIRST pair of the table: the later items of {0, 1} have an empty forward direction;
      (5, 4) cut to ONE constraint, the LAST pair of the table: the later items of {4, 5} have an empty backward direction whose
             range starts at the table's end;
      (0, 5) without (5, 0): an item of frames 0 and F - 1 whose backward pair does not exist (range 0 .. 0)."""
    pairs = [(a, b) for a in range(F) for b in range(F) if a != b and abs(a - b) <= 2] + [(0, F - 1)]
    v = synth.make_video(F, pc.WIDTH, pc.HEIGHT, seed=77, pairs=pairs, spacing=3.0)
    assert tuple(v.pairs[0]) == (0, 1) and tuple(v.pairs[-1]) == (F - 1, F - 2)
    return _cut(v, {(0, 1): 1, (F - 1, F - 2): 1})


@functools.lru_cache(maxsize=None)
def long_video():
    """Six frames at 280 x 176, every forward pair sampled at every pixel (~55 000 constraints: 73 items of 768), the backward
    pairs cut to 5: ~1100 items, the fewest that lie inside the 128-thread window (1024, 1536] of B = 139 on a 256-CU device."""
    pairs = [(a, b) for a in range(F) for b in range(F) if a != b]
    v = synth.make_video(F, 280, 176, seed=78, pairs=pairs, spacing=1.0)
    return _cut(v, {(a, b): 5 for a, b in pairs if a > b})


def _params(intr=None):
    p = OptParams.defaults()
    p.num_threads = 16
    if intr is not None:
        p.intr_opt = intr
    return p


def _loaded(ctor, video, ddesc, generic=False):
    s = ctor()
    synth.load_into(s, video)
    s.reset_depth_xforms(ddesc)
    s.reset_spatial_xforms(XformDesc.spatial())
    if generic:
        s.set_generic_kernels(True)
    return s


# (id, video, depth transform, intrinsics, KD, threads expected on 256 CUs)
CASES = [
    ("global-b8", edge_video, XformDesc.global_depth, None, 1, 256),
    ("grid11x12-b139-256", edge_video, lambda: XformDesc.grid_depth(11, 12), None, 4, 256),
    ("grid11x12-b139-128", long_video, lambda: XformDesc.grid_depth(11, 12), None, 4, 128),
    ("grid17x10-b177", edge_video, lambda: XformDesc.grid_depth(17, 10), None, 4, 256),
    ("grid4x3-shared-intrinsics", edge_video, lambda: XformDesc.grid_depth(4, 3), IntrinsicsOptimization.Shared, 4, 256),
]


def test_edge_items_are_what_the_cases_claim():
    """(No launch: the host's item rule restated by product_cases.)  The first and the last pair of the table each own an item with
    an empty direction, and frames 0 and F - 1 share an item whose backward direction is absent."""
    v = edge_video()
    items = pc.expected_items(v, 256)
    assert any(fa == 0 and fb == 1 and m0 == 0 and m1 > 0 for fa, fb, m0, m1 in items), items
    assert any(fa == F - 2 and fb == F - 1 and m0 > 0 and m1 == 0 for fa, fb, m0, m1 in items), items
    assert any(fa == 0 and fb == F - 1 and m0 > 0 and m1 == 0 for fa, fb, m0, m1 in items), items
    assert int(v.offsets[-1]) - int(v.offsets[-2]) == 1                     # the last pair of the table is the one-constraint pair
    n = len(pc.expected_items(long_video(), 256))
    assert pc.expected_threads(4, 1, 139, 256, n) == 128 and pc.expected_threads(4, 1, 139, 256, len(items)) == 256, n


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_product_matches_oracle_and_generic_kernel(Solver, case):
    cid, video, ddesc, intr, kd, threads256 = case
    v = video()
    p = _params(intr)
    hip = _loaded(lambda: Solver(0), v, ddesc())
    pose, dx, _ = _state(hip, F, np.random.default_rng(17))
    hip.set_xform_params(dx)
    h = hip.evaluate(p, 0.1, pose, want_hfull=True)
    L = hip.product_launch_debug()
    orc = _loaded(Oracle, v, ddesc())
    orc.set_xform_params(dx)
    o = orc.evaluate(p, 0.1, pose, want_hfull=True)
    gen = _loaded(lambda: Solver(0), v, ddesc(), generic=True)
    gen.set_xform_params(dx)
    g = gen.evaluate(p, 0.1, pose, want_hfull=True)
    assert gen.product_launch_debug()["kind"] == 0

    B = hip.block_size()
    items = pc.expected_items(v, L["num_cu"])
    assert (L["kind"], L["spec"], L["kd"], L["work_items"]) == (1, 1, kd, len(items)), L
    if margins.deterministic_build():
        assert L["threads"] == 64, L
    else:
        assert L["threads"] == pc.expected_threads(kd, 1, B, L["num_cu"], len(items)), L
        if L["num_cu"] == 256:
            assert L["threads"] == threads256, L

    assert h["num_residual_blocks"] == o["num_residual_blocks"]
    margins.below("cost", abs(h["cost"] - o["cost"]) / abs(o["cost"]), TOL)
    margins.below("gradient", rel(h["gradient"], o["gradient"]), TOL)
    margins.below("hfull", rel(h["hfull"], o["hfull"]), TOL)
    margins.below("hfull_vs_generic", rel(h["hfull"], g["hfull"]), TOL)
    # Jacobi-scaled, entry by entry: an error confined to a few rows (one frame's pose rows, the depth rows of one thread's
    # elements) cannot hide behind the largest entries
    d = np.sqrt(np.diag(o["hfull"]))
    assert d.min() > 0.0
    scaled = np.abs(h["hfull"] - o["hfull"]) / d[:, None] / d[None, :]
    worst = np.unravel_index(int(np.argmax(scaled)), scaled.shape)
    margins.below("hfull_jacobi_scaled", float(scaled[worst]), TOL,
                  info={"row (frame, unknown)": divmod(int(worst[0]), B), "column": divmod(int(worst[1]), B)})


# (id, solver options, pose-graph level expected, temporal level expected)
LEVELS = [
    ("coarse-and-temporal", {"coarse_level": 2, "temporal_level": 2, "temporal_step": 2}, True, True),
    ("coarse-only", {"coarse_level": 2, "temporal_level": 0}, True, False),
    ("temporal-only", {"coarse_level": 0, "temporal_level": 2, "temporal_step": 2}, False, True),
    ("block-jacobi-only", {"coarse_level": 0, "temporal_level": 0}, False, False),
]


@functools.lru_cache(maxsize=None)
def _lm_start():
    """State both sides start from, chosen by the oracle alone, and the oracle's step from there.  As in
    tests/test_gpu_product_shapes.py the raw draw is advanced by the oracle's first LM iterations: two here (cost 1289 -> 166; on
    this small problem the oracle accepts every step and has converged after eight, where a ninth step is rejected and leaves
    nothing to compare).  The fresh step from there is accepted and large (norm 0.2, cost 166 -> 17.5)."""
    v = edge_video()
    ddesc = XformDesc.grid_depth(5, 4)
    orc = _loaded(Oracle, v, ddesc)
    pose, dx, _ = _state(orc, F, np.random.default_rng(17))
    p = _params()
    p.max_iterations = 2
    orc.set_pose_params(pose)
    orc.set_xform_params(dx)
    orc.pose_optimization_step(p, 0.1, convert_poses=False)
    pose, dx = orc.get_pose_params(), orc.get_xform_params()
    p.max_iterations = 1
    orc.pose_optimization_step(p, 0.1, convert_poses=False)
    sm = orc.summary()
    assert sm["num_iterations"] == 1 and sm["num_successful_steps"] > 0, "the oracle must accept the step that is compared"
    step = np.concatenate([orc.get_pose_params() - pose, orc.get_xform_params() - dx], axis=1)
    return pose, dx, step


@pytest.mark.parametrize("level", LEVELS, ids=[c[0] for c in LEVELS])
def test_one_lm_step_with_the_levels_on_and_off(Solver, level):
    """The product inside the PCG (fused p = z + beta p with the coarse correction c_f and the temporal level's taps; the first
    product of the solve has useBeta = 0 and must not read p_old) on a 5 x 4 grid (B = 27): the HIP step, stopped at a relative
    residual of 1e-10, against the oracle's exact step.  |dx_hip - dx_oracle| <= 1e-6 |dx_oracle|, the bar and its derivation
    of test_one_lm_step_matches_the_exact_step."""
    lid, opts, want_coarse, want_temporal = level
    pose, dx, ref_step = _lm_start()
    hip = _loaded(lambda: Solver(0), edge_video(), XformDesc.grid_depth(5, 4))
    hip.set_options(pcg_relative_tolerance=1e-10, **opts)
    p = _params()
    p.max_iterations = 1
    hip.set_pose_params(pose)
    hip.set_xform_params(dx)
    hip.pose_optimization_step(p, 0.1, convert_poses=False)
    sm = hip.summary()
    assert sm["num_iterations"] == 1 and sm["num_successful_steps"] > 0, sm
    assert sm["total_linear_iterations"] >= 3, sm    # a first product and later ones
    path = hip.path_info()
    assert (path["pose_graph_level"] != "none", path["depth_grid_level"]) == (want_coarse, want_temporal), path
    L = hip.product_launch_debug()
    assert L["kind"] == 1 and L["spec"] == 1 and L["kd"] == 4, L
    step = np.concatenate([hip.get_pose_params() - pose, hip.get_xform_params() - dx], axis=1)
    ref = np.linalg.norm(ref_step)
    print(f"lm step {lid}: |dx| {ref:.3e}, hip vs oracle {np.linalg.norm(step - ref_step) / ref:.3e}, "
          f"PCG iterations {sm['total_linear_iterations']}")
    margins.below("lm_step", float(np.linalg.norm(step - ref_step) / ref), 1e-6,
                  info={"linear_iterations": sm["total_linear_iterations"]})
